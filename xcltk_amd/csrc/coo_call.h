// coo_call.h - the host steps that the derived-matrix calls share (xck_snp_counts, snp_counts.h; xck_group_counts, group_counts.h): they
// count on the device, read the totals with ONE host synchronise, size a result of their own and emit into it.  Included by finish.hip
// inside namespace xck, behind fold_partition.h and ahead of refold.h, snp_counts.h and group_counts.h; the state the steps work on is
// CooCall (engine_impl.h), the copy-out rule they apply is deliver_words() (finish.hip).  A call is, in this order: coo_begin; a
// ScratchLayout and coo_scratch; ev[0], its first phase, ev[1], its count pass and scans; coo_publish_totals (ev[2] and the ONE
// synchronise); coo_reserve (ev[3]); its emit pass; coo_deliver (ev[4], the copy-out, the closing synchronises, the times); coo_fill.
#pragma once

// Pieces of one device block, each at a multiple of 256 B, in the order they were added (so a call can clear its leading pieces with
// one memset up to offs[i])
struct ScratchLayout {
    size_t offs[16], bytes = 0;
    int n = 0;
    int add(size_t b) { assert(n < 16); offs[n] = bytes; bytes += (b + 255) & ~size_t(255); return n++; }
    size_t total() const { return bytes; }
    template <class T> T* at(char* base, int i) const { return reinterpret_cast<T*>(base + offs[i]); }
};

constexpr int COO_TOT_WORDS = 4, COO_FLAG_WORD = 3;                       // the mapped words of a call: three totals and a flag
// the n (<= 3) 32-bit totals of a call and, if the call has one, its flag word -> the call's mapped words
__global__ void k_coo_totals(const uint32_t* __restrict__ tot, int n, const uint32_t* __restrict__ flag, unsigned long long* __restrict__ host_alias) {
    if ((int)threadIdx.x < n) host_alias[threadIdx.x] = tot[threadIdx.x];
    if (threadIdx.x == COO_FLAG_WORD && flag) host_alias[COO_FLAG_WORD] = *flag;
}

// the mapped words (pinned, of the call's own: none of the handle's control words is used) and the events on first use; nnz and times cleared
static int coo_begin(EngineImpl* im, CooCall& c) {
    if (!c.h_tot) {
        HIP_TRY(hipHostMalloc((void**)&c.h_tot, COO_TOT_WORDS * sizeof(unsigned long long), hipHostMallocMapped));
        HIP_TRY(hipHostGetDevicePointer((void**)&c.d_tot_alias, c.h_tot, 0));
    }
    for (auto& ev : c.ev) if (!ev) HIP_TRY(hipEventCreate(&ev));
    c.ms_total = c.ms_copy = 0; for (int q = 0; q < 3; q++) { c.nnz[q] = 0; c.ms_phase[q] = 0; }
    return 0;
}
static int coo_scratch(EngineImpl* im, CooCall& c, const ScratchLayout& L) { return grow_device(im, (void**)&c.d_scratch, &c.scratch_cap, L.total(), L.total() / 8 + 4096); }

// behind the count pass: d_tot[0 .. n) and *d_flag (null: none) reach the host; c.nnz[] holds the totals, c.h_tot[COO_FLAG_WORD] the flag
static int coo_publish_totals(EngineImpl* im, CooCall& c, const uint32_t* d_tot, int n, const uint32_t* d_flag) {
    hipLaunchKernelGGL(k_coo_totals, dim3(1), dim3(64), 0, im->s_comp, d_tot, n, d_flag, c.d_tot_alias);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev[2], im->s_comp));
    HIP_TRY(hipStreamSynchronize(im->s_comp));
    for (int y = 0; y < n; y++) c.nnz[y] = (size_t)c.h_tot[y];
    return 0;
}
static inline size_t coo_words(const CooCall& c) { return 3 * (c.nnz[0] + c.nnz[1] + c.nnz[2]); }

// room for the blocks of c.nnz[] entries on the device and in pinned memory; d_out[y] is where block y starts on the device
static int coo_reserve(EngineImpl* im, CooCall& c, int32_t* d_out[3]) {
    const size_t words = coo_words(c);
    if (int rc = grow_device(im, (void**)&c.d_res, &c.d_res_cap, std::max<size_t>(words, 1) * 4, words + 4096)) return rc;
    if (int rc = grow_pinned(im, (void**)&c.h_res, &c.h_res_cap, std::max<size_t>(words, 1) * 4, words + 4096)) return rc;
    { size_t at = 0; for (int y = 0; y < 3; y++) { d_out[y] = c.d_res + at; at += 3 * c.nnz[y]; } }
    HIP_TRY(hipEventRecord(c.ev[3], im->s_comp));
    return 0;
}

// behind the emit pass: the result crosses to the host, both streams are waited for, the times of the call are read.  ms_total ends at
// the compute stream's synchronise; ms_copy is the wait for the copy stream behind it (the wait xck_refold spends in result_host()).
static int coo_deliver(EngineImpl* im, CooCall& c, std::chrono::steady_clock::time_point t0) {
    const size_t words = coo_words(c);
    HIP_TRY(hipEventRecord(c.ev[4], im->s_comp));
    if (int rc = deliver_words(im, c.d_res, c.h_res, words, c.ev[4])) return rc;
    HIP_TRY(hipStreamSynchronize(im->s_comp));
    c.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (on_copy_stream(words)) {
        const auto t1 = std::chrono::steady_clock::now();
        HIP_TRY(hipStreamSynchronize(im->s_copy));
        c.ms_copy = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    HIP_TRY(hipEventElapsedTime(&c.ms_phase[0], c.ev[0], c.ev[1])); HIP_TRY(hipEventElapsedTime(&c.ms_phase[1], c.ev[1], c.ev[2])); HIP_TRY(hipEventElapsedTime(&c.ms_phase[2], c.ev[3], c.ev[4]));
    return 0;
}

// the first n blocks of the pinned result as xck_coo (an empty block keeps its null pointers)
static void coo_fill(const CooCall& c, int n, xck_coo* const dst[3]) {
    size_t at = 0;
    for (int y = 0; y < n; y++) {
        const size_t z = c.nnz[y];
        dst[y]->nnz = (int64_t)z;
        if (z) { dst[y]->row = c.h_res + at; dst[y]->col = c.h_res + at + z; dst[y]->val = c.h_res + at + 2 * z; }
        at += 3 * z;
    }
}
// a call that failed part-way: what it queued is waited for; nothing of the handle was overwritten, so it is not marked failed
static int coo_fail(EngineImpl* im, int rc) { hipStreamSynchronize(im->s_comp); hipStreamSynchronize(im->s_copy); return rc; }
