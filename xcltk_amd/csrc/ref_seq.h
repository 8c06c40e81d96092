// ref_seq.h - the genome's sequence of a tally handle, packed on the device (xck_set_contig_ref, xck_get_contig_ref,
// xck_get_base_tally_contigs, include/xck.h).  Included by engine.hip inside namespace xck, behind base_tally.h,
// whose candidate kernels read what is packed here (k_bt_candidates<EMIT, true>, bt_candidate_ref).
//
// Per contig the handle keeps (len + 7) / 8 dwords of 4-bit codes (BAM's: =ACMGRSVTWYHKDBN), half a byte a position.  The FASTA text goes
// to the device as it lies in the file, line ends included, in chunks of XCK_REF_CHUNK_BYTES through two pinned staging chunks (the host
// fills one while the other's copy and kernel run on s_comp); no host loop looks at a base.  ref_geom.h (included by engine.hip) holds the arithmetic - where a
// position lies, what a chunk covers, how a dword is made - for the kernel, this file and tools/asan/ref_geom_check.cpp alike.
//
// k_ref_pack: a thread makes one dword, 8 positions, and consecutive lanes make consecutive dwords: a wave instruction stores 256
// consecutive bytes.  The thread's 8 raw bytes are one (unaligned) 8-byte load unless a line ends among them - then, and at the contig's
// end, it walks byte by byte and steps over the line end where it meets it - so a wave reads 512 consecutive bytes plus its line ends.
// Letters map to codes through 256 bytes of LDS the block fills itself (rg_code); there is no other LDS, no scratch, and one atomic per
// block that met a byte below 33 where a base must be: the stale-index count that fails the call.
#pragma once

constexpr int RS_BLOCK = 256;

__global__ __launch_bounds__(RS_BLOCK) void k_ref_pack(const uint8_t* __restrict__ chunk, long long n_chunk, long long base0, long long p0, long long p1, int32_t lb, int32_t lw,
                                                       uint32_t* __restrict__ out, unsigned long long* __restrict__ n_bad) {
    __shared__ uint8_t s_map[256];
    __shared__ uint32_t s_bad[RS_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    s_map[tid] = rg_code((uint32_t)tid);
    __syncthreads();
    const long long p = p0 + ((long long)blockIdx.x * RS_BLOCK + tid) * RG_POS_PER_THREAD;
    uint32_t bad = 0;
    if (p < p1) out[p >> 3] = rg_pack_dword(chunk, n_chunk, base0, p, p1, lb, lw, s_map, bad);   // (p < p1 <= len: inside the (len + 7) / 8 dwords)
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) bad += __shfl_xor(bad, dd, 64);
    if (lane == 0) s_bad[wave] = bad;
    __syncthreads();
    if (tid == 0) { uint32_t a = 0; for (int w = 0; w < RS_BLOCK / 64; w++) a += s_bad[w]; if (a) atomicAdd(n_bad, (unsigned long long)a); }
}
static_assert(RS_BLOCK == 256, "a thread of k_ref_pack fills one entry of the 256-entry code table");

// ---- host side ----
void ref_seq_free(EngineImpl* im) {
    for (uint32_t* p : im->rs_tab) if (p) hipFree(p);
    for (int k = 0; k < 2; k++) {
        if (im->h_rs_stage[k]) hipHostFree(im->h_rs_stage[k]);
        if (im->d_rs_stage[k]) hipFree(im->d_rs_stage[k]);
        if (im->rs_ev[k]) hipEventDestroy(im->rs_ev[k]);
    }
    if (im->d_rs_bad) hipFree(im->d_rs_bad);
}

static int ref_seq_drop(EngineImpl* im, int32_t c) {
    if (im->rs_tab[c]) { HIP_TRY(hipFree(im->rs_tab[c])); im->rs_tab[c] = nullptr; }
    return 0;
}

// xck_set_contig_ref for the pileup pipeline
int engine_set_contig_ref(EngineImpl* im, int32_t contig, const char* raw, int64_t n_raw, int32_t line_bases, int32_t line_width) {
    if (!im->base_tally) { im->eng->err = "handle made without XCK_F_BASE_TALLY"; return XCK_E_STATE; }
    if (im->bt_len.empty()) { im->eng->err = "xck_set_contig_ref: no contig lengths (xck_set_contig_lengths)"; return XCK_E_STATE; }
    if (contig < 0 || contig >= (int32_t)im->bt_len.size()) { im->eng->err = "xck_set_contig_ref: contig outside the handle's contigs"; return XCK_E_ARG; }
    if (line_bases < 1 || line_width < line_bases) { im->eng->err = "xck_set_contig_ref: line_bases < 1 or line_width < line_bases"; return XCK_E_ARG; }
    const int64_t len = im->bt_len[contig], lb = line_bases, lw = line_width;
    if (!raw || n_raw < rg_offset(len - 1, lb, lw) + 1) {
        char b[200]; snprintf(b, sizeof b, "xck_set_contig_ref: %lld raw bytes, the last of the contig's %lld positions lies at offset %lld", (long long)n_raw, (long long)len, (long long)rg_offset(len - 1, lb, lw));
        im->eng->err = b; return XCK_E_ARG;
    }
    HIP_TRY(hipSetDevice(im->device));
    const auto t0 = std::chrono::steady_clock::now();
    if (!im->rs_tab[contig]) {
        const size_t bytes = (size_t)((len + 7) / 8) * 4;
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            char b[200]; snprintf(b, sizeof b, "out of device memory for the packed sequence of contig %d (%lld positions, %.2f GB)", (int)contig, (long long)len, bytes * 1e-9);
            im->eng->err = b; return e == hipErrorOutOfMemory ? XCK_E_NOMEM : XCK_E_DEVICE;
        }
        im->rs_tab[contig] = (uint32_t*)p;
    }
    if (!im->d_rs_bad) { if (const int rc = dev_zeroed(im, (void**)&im->d_rs_bad, sizeof(unsigned long long))) return rc; }
    HIP_TRY(hipMemsetAsync(im->d_rs_bad, 0, sizeof(unsigned long long), im->s_comp));
    const int64_t chunk_knob = std::max<int64_t>(RG_MIN_CHUNK, im->eng->knobs.ref_chunk_bytes);
    int64_t n_chunks = 0;
    int k = 0;
    for (int64_t p0 = 0; p0 < len; k ^= 1, n_chunks++) {
        const int64_t p1 = rg_chunk_end(p0, len, lb, lw, chunk_knob);
        const size_t nb = (size_t)rg_chunk_bytes(p0, p1, lb, lw);                 // (<= the knob unless fewer than 8 positions fit into it)
        if (!im->rs_ev[k]) HIP_TRY(hipEventCreateWithFlags(&im->rs_ev[k], hipEventDisableTiming));
        else HIP_TRY(hipEventSynchronize(im->rs_ev[k]));                          // the copy that last read this pinned chunk has ended
        int rc = grow_pinned(im, &im->h_rs_stage[k], &im->rs_hcap[k], nb, 0);
        if (!rc) rc = grow_device(im, &im->d_rs_stage[k], &im->rs_dcap[k], nb, 0);
        if (rc) { (void)hipStreamSynchronize(im->s_comp); (void)ref_seq_drop(im, contig); return rc; }   // (half a sequence is none)
        memcpy(im->h_rs_stage[k], raw + rg_offset(p0, lb, lw), nb);
        HIP_TRY(hipMemcpyAsync(im->d_rs_stage[k], im->h_rs_stage[k], nb, hipMemcpyHostToDevice, im->s_comp));
        const long long n_dw = (long long)((p1 - p0 + 7) / 8);
        hipLaunchKernelGGL(k_ref_pack, dim3((unsigned)((n_dw + RS_BLOCK - 1) / RS_BLOCK)), dim3(RS_BLOCK), 0, im->s_comp, (const uint8_t*)im->d_rs_stage[k], (long long)nb,
                           (long long)rg_offset(p0, lb, lw), (long long)p0, (long long)p1, line_bases, line_width, im->rs_tab[contig], im->d_rs_bad);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(im->rs_ev[k], im->s_comp));
        p0 = p1;
    }
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, im->d_rs_bad, sizeof bad, hipMemcpyDeviceToHost, im->s_comp));
    HIP_TRY(hipStreamSynchronize(im->s_comp));
    if (bad) {
        if (const int rc = ref_seq_drop(im, contig)) return rc;
        char b[240]; snprintf(b, sizeof b, "xck_set_contig_ref: the FASTA line geometry does not match its index (contig %d: %llu byte(s) below 33 where line_bases %d / line_width %d put a base)",
                              (int)contig, bad, (int)line_bases, (int)line_width);
        im->eng->err = b; return XCK_E_ARG;
    }
    if (im->eng->knobs.debug_timing) {
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        fprintf(stderr, "[xck] set_contig_ref: contig %d, %lld positions, %lld chunk(s), %.3f ms (host clock), %.2f GB/s of raw bytes\n", (int)contig, (long long)len, (long long)n_chunks, ms,
                (double)(rg_offset(len - 1, lb, lw) + 1) * 1e-6 / std::max(ms, 1e-6));
    }
    return 0;
}

// xck_get_contig_ref for the pileup pipeline: the letters of [pos0, pos0 + n)
int engine_get_contig_ref(EngineImpl* im, int32_t contig, int32_t pos0, int32_t n, char* out) {
    if (!im->base_tally) { im->eng->err = "handle made without XCK_F_BASE_TALLY"; return XCK_E_STATE; }
    if (im->bt_len.empty()) { im->eng->err = "xck_get_contig_ref: no contig lengths (xck_set_contig_lengths)"; return XCK_E_STATE; }
    if (contig < 0 || contig >= (int32_t)im->bt_len.size() || pos0 < 0 || n < 0 || (int64_t)pos0 + n > im->bt_len[contig] || (n > 0 && !out)) {
        im->eng->err = "xck_get_contig_ref: contig or position range outside the handle's contigs"; return XCK_E_ARG; }
    if (!im->rs_tab[contig]) { im->eng->err = "xck_get_contig_ref: the contig has no sequence (xck_set_contig_ref)"; return XCK_E_STATE; }
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(im->device));
    const size_t b0 = (size_t)pos0 >> 1, b1 = ((size_t)pos0 + n + 1) >> 1;          // (b1 <= (len + 1) / 2 <= the table's bytes)
    std::vector<uint8_t> h(b1 - b0);
    HIP_TRY(hipMemcpy(h.data(), (const uint8_t*)im->rs_tab[contig] + b0, b1 - b0, hipMemcpyDeviceToHost));
    for (int32_t i = 0; i < n; i++) {
        const size_t p = (size_t)pos0 + i;
        const uint8_t by = h[(p >> 1) - b0];
        out[i] = "=ACMGRSVTWYHKDBN"[(p & 1) ? (by & 15) : (by >> 4)];
    }
    return 0;
}

// xck_get_base_tally_contigs for the pileup pipeline
int engine_base_tally_contigs(EngineImpl* im, uint8_t* has_table, int32_t n) {
    if (!im->base_tally) { im->eng->err = "handle made without XCK_F_BASE_TALLY"; return XCK_E_STATE; }
    if (!has_table || n != im->eng->n_contigs) { im->eng->err = "xck_get_base_tally_contigs: one byte per contig of the handle"; return XCK_E_ARG; }
    for (int32_t c = 0; c < n; c++) has_table[c] = (size_t)c < im->bt_tab.size() && im->bt_tab[c] ? 1 : 0;
    return 0;
}
