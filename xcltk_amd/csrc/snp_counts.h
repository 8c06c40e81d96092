// snp_counts.h - xck_snp_counts (include/xck.h): the SNP x cell AD / DP / OTH matrices of a finished pileup, counted straight from what
// the molecule stage of the last xck_finish left (finish.hip fold_molecules): the hits sorted by (SNP, cell, UMI) and, at the head of
// every molecule, the base its first read shows (EngineImpl::mol_keys / mol_al / mol_n).  Included by finish.hip inside namespace xck,
// behind fold_partition.h (pf_scan), refold.h and coo_call.h: the host steps around the kernels below (scratch layout, totals, result buffers, copy-out, times) are that file's.
//
// Per (SNP, cell) run of the stream: AD = molecules that show the SNP's ALT, DP = those that show REF or ALT, OTH = those that show
// another base (allele_side(), the rule k_expand uses); molecules claimed by a gap record (al == 0) count nowhere.  No region table,
// no fan-out, no sort, no per-SNP filter: every SNP of the sorted table counts, under the handle's current REF / ALT.
//
//   k_snc_heads   one flag byte per entry of the stream: first / last entry of its SNP, and at the head of every (SNP, cell) run which
//                 of the three counts are non-zero.  The head walks at most RUN_WALK followers; a longer run is queued and finished by
//                 one block (k_snc_long).  The three counts go to the head's slots of `sums`; the non-zero flags of a tile are counted.
//   pf_scan       per matrix, over the tiles' counts: with a block scan inside the tile every entry knows P(i) = non-zero entries
//                 of the matrix before it in the stream.
//   k_snc_rows    P at the first and behind the last entry of every SNP.  Their difference is the SNP's number of non-zeros.
//   k_snc_row_counts + pf_scan   those numbers scattered to the caller's SNP order and scanned: the base of every caller row.
//   k_snc_emit    entry i of sorted SNP s goes to base[caller row of s] + P(i) - P(first entry of s): the stream is in sorted-SNP
//                 order with every SNP's entries contiguous and in cell order, so the output is sorted by (caller row, cell) without
//                 a sort and without a counter per row.
//
// Memory: buffers of the call's own (the CooCall EngineImpl::sc, and d_sc_perm; grow-only, freed at destroy) - nothing from
// workspace 1, workspace 2 or the shard slices, so the call invalidates nothing xck_finish / xck_refold / xck_get_result_device
// handed out.  Scratch: 13 bytes per entry of the stream (flag byte, three 32-bit sums) + 8 bytes per RUN_WALK entries (long runs)
// + 12 bytes per tile + 24 bytes per SNP of the sorted table + 12 bytes per SNP of the caller's list.
#pragma once

constexpr int SNC_BLOCK = 256, SNC_ITEMS = 8, SNC_TILE = SNC_BLOCK * SNC_ITEMS;
constexpr uint32_t SNC_AD = 1, SNC_DP = 2, SNC_OTH = 4, SNC_ROW_FIRST = 8, SNC_ROW_LAST = 16;      // bits of a flag byte
static_assert(SNC_BLOCK == FD_BLOCK, "block_excl_scan64 is written for FD_BLOCK threads");

// one molecule's contribution, packed: ALT | REF << 21 | OTH << 42
__device__ __forceinline__ unsigned long long snc_class(uint32_t code, uint32_t inf) {
    if (!code) return 0ull;
    const int side = allele_side(int(code) - 1, inf);
    return side == 1 ? 1ull : side == 0 ? (1ull << 21) : (1ull << 42);
}
__device__ __forceinline__ uint32_t snc_flags(uint32_t a, uint32_t r, uint32_t o) { return (a ? SNC_AD : 0u) | ((a | r) ? SNC_DP : 0u) | (o ? SNC_OTH : 0u); }
// the non-zero flags of a flag byte as three 21-bit counters (a tile holds 2048 entries)
__device__ __forceinline__ unsigned long long snc_pack(uint32_t b) { return (unsigned long long)(b & 1u) | ((unsigned long long)((b >> 1) & 1u) << 21) | ((unsigned long long)((b >> 2) & 1u) << 42); }

struct SncBufs {
    uint8_t* f;                   // [n] flag bytes
    uint32_t* sums;               // [3][n]: AD, DP, OTH at the heads whose flag says non-zero
    uint32_t* tcnt;               // [3][nt]: non-zero entries per tile, then (scanned) before the tile
    unsigned long long* long_runs;   // [0] = count, then the heads of the (SNP, cell) runs longer than RUN_WALK
    uint32_t *p0, *p1;            // [3][ns]: P at the first entry of the sorted SNP, P behind its last
    uint32_t* cc;                 // [3][stride]: non-zeros per caller row, then (scanned) the row's base
    long long n, nt, ns, stride;
};

template <class K>
__global__ __launch_bounds__(SNC_BLOCK) void k_snc_heads(const K* __restrict__ k, const uint8_t* __restrict__ al, KeyLayout<K> kl, const uint32_t* __restrict__ info, SncBufs B) {
    __shared__ unsigned long long s_w[SNC_BLOCK / 64];
    const long long n = B.n, base = (long long)blockIdx.x * SNC_TILE;
    unsigned long long c = 0;
#pragma unroll 1
    for (int t = 0; t < SNC_ITEMS; t++) {                                 // striped: lane-contiguous loads
        const long long i = base + (long long)t * SNC_BLOCK + threadIdx.x;
        if (i >= n) break;
        const K me = k[i];
        const K kp = i > 0 ? k[i - 1] : me, kn = i + 1 < n ? k[i + 1] : me;
        const uint32_t row = kl.row(me);
        uint32_t bits = 0;
        if (i == 0 || kl.row(kp) != row) bits |= SNC_ROW_FIRST;
        if (i + 1 == n || kl.row(kn) != row) bits |= SNC_ROW_LAST;
        if (i == 0 || kl.rc(kp) != kl.rc(me)) {                           // head of a (SNP, cell) run
            const uint32_t inf = info[row];
            const K rc = kl.rc(me);
            unsigned long long x = snc_class(al[i], inf);
            long long j = i + 1;
            for (; j < n && j <= i + RUN_WALK && kl.rc(k[j]) == rc; j++) x += snc_class(al[j], inf);
            if (j < n && j > i + RUN_WALK && kl.rc(k[j]) == rc) B.long_runs[1 + atomicAdd(&B.long_runs[0], 1ull)] = (unsigned long long)i;   // finished by k_snc_long
            else {
                const uint32_t a = (uint32_t)(x & 0x1fffffu), r = (uint32_t)((x >> 21) & 0x1fffffu), o = (uint32_t)(x >> 42);
                const uint32_t fl = snc_flags(a, r, o);
                if (fl & SNC_AD) B.sums[i] = a;
                if (fl & SNC_DP) B.sums[B.n + i] = a + r;
                if (fl & SNC_OTH) B.sums[2 * B.n + i] = o;
                bits |= fl; c += snc_pack(fl);
            }
        }
        B.f[i] = (uint8_t)bits;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x < 3) { const unsigned long long t = s_w[0] + s_w[1] + s_w[2] + s_w[3]; B.tcnt[(long long)threadIdx.x * B.nt + blockIdx.x] = (uint32_t)(t >> (21 * threadIdx.x)) & 0x1fffffu; }
}

// A (SNP, cell) run longer than RUN_WALK (UMI-less and bulk input: 10^5 molecules of one cell over one SNP) is not walked by its head
// lane: ONE BLOCK per run finds the run's end by bisection and counts in parallel (the idiom of k_first_long / k_hap_class_long).
template <class K>
__global__ __launch_bounds__(256) void k_snc_long(const K* __restrict__ k, const uint8_t* __restrict__ al, KeyLayout<K> kl, const uint32_t* __restrict__ info, SncBufs B) {
    __shared__ uint32_t s_c[4][3];
    const long long n = B.n;
    const unsigned long long n_long = B.long_runs[0];
    for (unsigned long long r = blockIdx.x; r < n_long; r += gridDim.x) {
        const long long h = (long long)B.long_runs[1 + r];
        const K rc = kl.rc(k[h]);
        const uint32_t inf = info[kl.row(k[h])];
        long long lo = h + 1, hi = n;                                     // first index past the run
        while (lo < hi) { const long long mid = lo + ((hi - lo) >> 1); if (kl.rc(k[mid]) == rc) lo = mid + 1; else hi = mid; }
        uint32_t c[3] = {0, 0, 0};
        for (long long j = h + threadIdx.x; j < lo; j += 256) {
            const unsigned long long x = snc_class(al[j], inf);
            c[0] += (uint32_t)(x & 1u); c[1] += (uint32_t)((x >> 21) & 1u); c[2] += (uint32_t)(x >> 42);
        }
#pragma unroll
        for (int q = 0; q < 3; q++) { for (int d = 32; d; d >>= 1) c[q] += __shfl_xor(c[q], d, 64); }
        if ((threadIdx.x & 63) == 0) { for (int q = 0; q < 3; q++) s_c[threadIdx.x >> 6][q] = c[q]; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t a = s_c[0][0] + s_c[1][0] + s_c[2][0] + s_c[3][0], rf = s_c[0][1] + s_c[1][1] + s_c[2][1] + s_c[3][1], o = s_c[0][2] + s_c[1][2] + s_c[2][2] + s_c[3][2];
            const uint32_t fl = snc_flags(a, rf, o);
            const long long tile = h / SNC_TILE;
            if (fl & SNC_AD) { B.sums[h] = a; atomicAdd(&B.tcnt[tile], 1u); }
            if (fl & SNC_DP) { B.sums[B.n + h] = a + rf; atomicAdd(&B.tcnt[B.nt + tile], 1u); }
            if (fl & SNC_OTH) { B.sums[2 * B.n + h] = o; atomicAdd(&B.tcnt[2 * B.nt + tile], 1u); }
            B.f[h] = (uint8_t)(B.f[h] | fl);                              // (k_snc_heads left the row bits; this block is the head's only writer now)
        }
        __syncthreads();
    }
}

// the flag bytes of a thread's SNC_ITEMS consecutive entries, and P of the first of them for the three matrices (21-bit fields of `excl`
// plus the tile's bases)
__device__ __forceinline__ void snc_tile_scan(const SncBufs& B, unsigned long long* s_w, long long i0, uint32_t (&b)[SNC_ITEMS], uint32_t (&P)[3]) {
    unsigned long long c = 0;
#pragma unroll
    for (int q = 0; q < SNC_ITEMS; q++) { b[q] = i0 + q < B.n ? (uint32_t)B.f[i0 + q] : 0u; c += snc_pack(b[q]); }
    unsigned long long total;
    const unsigned long long excl = block_excl_scan64(c, s_w, total);
#pragma unroll
    for (int y = 0; y < 3; y++) P[y] = B.tcnt[(long long)y * B.nt + blockIdx.x] + (uint32_t)((excl >> (21 * y)) & 0x1fffffu);
}

template <class K>
__global__ __launch_bounds__(SNC_BLOCK) void k_snc_rows(const K* __restrict__ k, KeyLayout<K> kl, SncBufs B) {
    __shared__ unsigned long long s_w[SNC_BLOCK / 64];
    const long long i0 = (long long)blockIdx.x * SNC_TILE + (long long)threadIdx.x * SNC_ITEMS;    // blocked: a thread owns SNC_ITEMS consecutive entries
    uint32_t b[SNC_ITEMS], P[3];
    snc_tile_scan(B, s_w, i0, b, P);
#pragma unroll
    for (int q = 0; q < SNC_ITEMS; q++) {
        if (b[q] & (SNC_ROW_FIRST | SNC_ROW_LAST)) {                      // (only inside the stream: the flag byte of an entry beyond it reads 0)
            const long long row = (long long)kl.row(k[i0 + q]);
#pragma unroll
            for (int y = 0; y < 3; y++) {
                if (b[q] & SNC_ROW_FIRST) B.p0[y * B.ns + row] = P[y];
                if (b[q] & SNC_ROW_LAST) B.p1[y * B.ns + row] = P[y] + ((b[q] >> y) & 1u);
            }
        }
#pragma unroll
        for (int y = 0; y < 3; y++) P[y] += (b[q] >> y) & 1u;
    }
}

// non-zeros of every sorted SNP, at the caller's index of the SNP (cc is zero on entry: a SNP the tables left out keeps 0)
__global__ __launch_bounds__(256) void k_snc_row_counts(const int32_t* __restrict__ perm, SncBufs B) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= B.ns) return;
    const long long c = perm[s];
#pragma unroll
    for (int y = 0; y < 3; y++) B.cc[y * B.stride + c] = B.p1[y * B.ns + s] - B.p0[y * B.ns + s];
}

template <class K>
__global__ __launch_bounds__(SNC_BLOCK) void k_snc_emit(const K* __restrict__ k, KeyLayout<K> kl, const int32_t* __restrict__ perm, SncBufs B, CooOut3 out) {
    __shared__ unsigned long long s_w[SNC_BLOCK / 64];
    const long long i0 = (long long)blockIdx.x * SNC_TILE + (long long)threadIdx.x * SNC_ITEMS;
    uint32_t b[SNC_ITEMS], P[3];
    snc_tile_scan(B, s_w, i0, b, P);
#pragma unroll
    for (int q = 0; q < SNC_ITEMS; q++) {
        if (b[q] & (SNC_AD | SNC_DP | SNC_OTH)) {
            const K key = k[i0 + q];
            const long long s = (long long)kl.row(key);
            const int32_t crow = perm[s], cell = (int32_t)kl.cell(key);
#pragma unroll
            for (int y = 0; y < 3; y++) {
                if (!((b[q] >> y) & 1u)) continue;
                const unsigned long long d = (unsigned long long)B.cc[y * B.stride + crow] + (P[y] - B.p0[y * B.ns + s]);
                if (d >= out.total[y]) continue;                          // (never: the totals are the sums of what is placed here)
                int32_t* __restrict__ o = out.o[y];
                o[d] = crow; o[out.total[y] + d] = cell; o[2 * out.total[y] + d] = (int32_t)B.sums[(long long)y * B.n + i0 + q];
            }
        }
#pragma unroll
        for (int y = 0; y < 3; y++) P[y] += (b[q] >> y) & 1u;
    }
}

// the kernels of one call on the compute stream, between the shared steps of coo_call.h
template <class K>
static int snp_counts_run(EngineImpl* im, std::chrono::steady_clock::time_point t0) {
    CooCall& c = im->sc;
    const KeyLayout<K> kl = key_layout<K>(im);
    const K* keys = (const K*)im->mol_keys;
    const size_t n = im->mol_n, ns = (size_t)im->n_snps_sorted, nt = (n + SNC_TILE - 1) / SNC_TILE, stride = ((size_t)im->n_snps_in + 1 + 63) & ~size_t(63);
    if (n >> 32) { im->eng->err = "xck_snp_counts: the sorted stream holds 2^32 hits or more: its 32-bit prefix counts do not reach that far"; return XCK_E_CAPACITY; }
    if (!im->d_sc_perm) {                                                 // sorted SNP -> the caller's index: fixed at xck_create
        int32_t* p = nullptr;
        HIP_TRY(hipMalloc((void**)&p, ns * sizeof(int32_t)));
        if (hipMemcpy(p, im->snp_perm.data(), ns * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { hipFree(p); im->eng->err = "xck_snp_counts: upload of the SNP order failed"; return XCK_E_DEVICE; }
        im->d_sc_perm = p;
    }
    // scratch: the pieces that start as zero come first (p0, p1, cc, the count word of the long-run list)
    const size_t n_bsum = (std::max(nt, stride) + SC_TILE - 1) / SC_TILE + 8;
    ScratchLayout L;
    const int i_p0 = L.add(3 * ns * 4), i_p1 = L.add(3 * ns * 4), i_cc = L.add(3 * stride * 4), i_long = L.add((n / (size_t)RUN_WALK + 3) * 8);
    const int i_f = L.add(n + 8), i_sums = L.add(3 * n * 4), i_tcnt = L.add(3 * nt * 4), i_bsum = L.add((n_bsum + 4) * 4);   // (the last: the scans' block sums + the three totals)
    if (int rc = coo_scratch(im, c, L)) return rc;
    char* d = c.d_scratch;
    SncBufs B;
    B.p0 = L.at<uint32_t>(d, i_p0); B.p1 = L.at<uint32_t>(d, i_p1); B.cc = L.at<uint32_t>(d, i_cc); B.long_runs = L.at<unsigned long long>(d, i_long);
    B.f = L.at<uint8_t>(d, i_f); B.sums = L.at<uint32_t>(d, i_sums); B.tcnt = L.at<uint32_t>(d, i_tcnt);
    uint32_t* bsum = L.at<uint32_t>(d, i_bsum); uint32_t* d_tot = bsum + n_bsum;
    B.n = (long long)n; B.nt = (long long)nt; B.ns = (long long)ns; B.stride = (long long)stride;
    HIP_TRY(hipEventRecord(c.ev[0], im->s_comp));
    HIP_TRY(hipMemsetAsync(d, 0, L.offs[i_long] + 8, im->s_comp));
    hipLaunchKernelGGL((k_snc_heads<K>), dim3((unsigned)nt), dim3(SNC_BLOCK), 0, im->s_comp, keys, (const uint8_t*)im->mol_al, kl, (const uint32_t*)im->d_snp_info, B);
    hipLaunchKernelGGL((k_snc_long<K>), dim3(256), dim3(256), 0, im->s_comp, keys, (const uint8_t*)im->mol_al, kl, (const uint32_t*)im->d_snp_info, B);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev[1], im->s_comp));
    for (int y = 0; y < 3; y++) if (int rc = pf_scan(im, B.tcnt + (size_t)y * nt, nt, bsum, nullptr)) return rc;
    hipLaunchKernelGGL((k_snc_rows<K>), dim3((unsigned)nt), dim3(SNC_BLOCK), 0, im->s_comp, keys, kl, B);
    hipLaunchKernelGGL(k_snc_row_counts, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, im->s_comp, (const int32_t*)im->d_sc_perm, B);
    HIP_TRY(hipGetLastError());
    for (int y = 0; y < 3; y++) if (int rc = pf_scan(im, B.cc + (size_t)y * stride, (size_t)im->n_snps_in + 1, bsum, d_tot + y)) return rc;
    if (int rc = coo_publish_totals(im, c, d_tot, 3, nullptr)) return rc;
    CooOut3 out; memset(&out, 0, sizeof out);
    for (int y = 0; y < 3; y++) out.total[y] = c.nnz[y];
    if (int rc = coo_reserve(im, c, out.o)) return rc;
    if (coo_words(c)) {
        hipLaunchKernelGGL((k_snc_emit<K>), dim3((unsigned)nt), dim3(SNC_BLOCK), 0, im->s_comp, keys, kl, (const int32_t*)im->d_sc_perm, B, out);
        HIP_TRY(hipGetLastError());
    }
    return coo_deliver(im, c, t0);
}

int engine_snp_counts(EngineImpl* im, xck_result* out) {
    xck_engine* e = im->eng;
    CooCall& c = im->sc;
    if (im->mode != XCK_MODE_BAF) { e->err = "xck_snp_counts: not a pileup pipeline"; return XCK_E_ARG; }
    if (im->fold_failed || !im->finished || !im->mol_valid) { e->err = "xck_snp_counts: valid between a successful xck_finish and the next xck_reset"; return XCK_E_STATE; }
    HIP_TRY(hipSetDevice(im->device));
    const auto t0 = std::chrono::steady_clock::now();
    clear_stale_error("snp_counts", e->knobs.debug_timing);
    im->sc_valid = false;
    if (int rc = coo_begin(im, c)) return rc;
    if (im->mol_n)
        if (int rc = im->key_bits == 64 ? snp_counts_run<uint64_t>(im, t0) : snp_counts_run<u128>(im, t0)) return coo_fail(im, rc);
    im->sc_valid = true;
    if (e->knobs.debug_timing) fprintf(stderr, "[xck] snp_counts: total %.3f ms (host clock to the stream synchronise): flags + long runs %.3f, scans + row bases %.3f, emit %.3f; wait for the copy-out %.3f; "
                                               "%zu entries, nnz %zu / %zu / %zu\n", c.ms_total, c.ms_phase[0], c.ms_phase[1], c.ms_phase[2], c.ms_copy, im->mol_n, c.nnz[0], c.nnz[1], c.nnz[2]);
    memset(out, 0, sizeof *out);
    xck_coo* const dst[3] = { &out->ad, &out->dp, &out->oth };
    coo_fill(c, 3, dst);
    return 0;
}
