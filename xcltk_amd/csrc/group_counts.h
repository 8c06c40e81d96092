// group_counts.h - xck_group_counts (include/xck.h): the row x group sums of matrices the handle already holds in HBM - the result
// blocks of the last xck_finish / xck_refold (EngineImpl::d_res) or the SNP x cell blocks of the last xck_snp_counts (sc.d_res) - under a
// cell -> group mapping given with the call.  Included by finish.hip inside namespace xck, behind fold_partition.h (pf_scan), snp_counts.h
// and coo_call.h: the host steps around the kernels below (scratch layout, totals and overflow flag, result buffers, copy-out, times) are that file's.
//
// A source matrix is [row | col | val], sorted by (row, col).  Inside a row the groups arrive in cell order, not in group order, so the
// output order is made here: every row is summed per group and its non-zero groups leave in ascending order.
//
//   k_grp_row_ptr   one thread per source row bisects the row array for the row's first entry (the idiom of k_snp_regions, refold.h).
//   k_grp_short     one WAVE per row of fewer than `long_row` (<= 64) entries, four rows per block: every lane holds one entry and its
//                   group; a lane sums the entries of its own group by reading the others' with uniform lane reads, the first lane of
//                   every group is its head, and a head's place in the row is the number of heads with a smaller group.  No table, no
//                   LDS.  A longer row is queued (count pass) and left to k_grp_long.
//   k_grp_long      one BLOCK per queued row, striding over it: LDS table of n_groups 32-bit sums (16 KB at XCK_GROUP_MAX), LDS atomics;
//                   then every thread owns a run of consecutive slots, and a block scan of the non-zero slots gives their places.
//   Both run twice, as k_expand and k_snp_regions do: the count pass leaves the number of non-zero groups per row, pf_scan (k_scan_reduce /
//   _top / _apply) turns them into the rows' bases, ONE host synchronise reads the totals of all matrices, the emit pass writes.
//
// Integer only; every output entry has one writer (no global atomics on the output); the only global atomics are the cursor of the
// long-row queue, whose order does not reach the output, and the overflow flag.  A sum that does not fit int32 is found, not wrapped:
// the wave path sums in 64 bits, the block path checks every LDS add against the value it replaced (values are positive, so the first
// add that crosses 2^31 - 1 sees it before the 32-bit word can wrap) - XCK_E_CAPACITY.
//
// Memory: buffers of the call's own (the CooCall EngineImpl::gc; grow-only, freed at destroy).  Traffic per source
// entry: the column and the value twice (count pass, emit pass), the row array only along the bisections, one gathered word of the
// mapping per pass: 16 bytes + 2 gathers; 12 bytes per output entry; 12 bytes of scratch per source row and matrix.
#pragma once

constexpr int GC_BLOCK = 256, GC_WAVES = GC_BLOCK / 64, GC_LONG_GRID = 512;
static_assert(XCK_GROUP_MAX % GC_BLOCK == 0, "k_grp_long gives every thread XCK_GROUP_MAX / GC_BLOCK slots at most");

struct GcMat {
    const int32_t* src;           // [row | col | val], nnz entries each
    uint32_t nnz;
    uint32_t* ptr;                // [n_rows + 1] first entry of every row
    uint32_t* cnt;                // [n_rows] non-zero groups of the row, then (scanned) the row's base in the output
    uint32_t* list;               // [n_rows] the rows left to k_grp_long
    int32_t* out;                 // [row | col | val], total entries each
    uint32_t total;
};
struct GcArgs {
    GcMat m[3];
    uint32_t n_rows, n_cells, long_row;
    int32_t n_groups;
    const int32_t* cg;            // [n_cells] group of every cell, -1 = left out
    uint32_t* ctl;                // [0..2] rows queued per matrix, [3] overflow flag
};

__global__ __launch_bounds__(GC_BLOCK) void k_grp_row_ptr(GcArgs A) {
    const GcMat& M = A.m[blockIdx.y];
    const uint32_t r = blockIdx.x * GC_BLOCK + threadIdx.x;
    if (r > A.n_rows) return;
    uint32_t lo = 0, hi = M.nnz;                                          // first entry whose row is >= r
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if ((uint32_t)M.src[mid] < r) lo = mid + 1; else hi = mid; }
    M.ptr[r] = lo;
}

template <bool EMIT>
__global__ __launch_bounds__(GC_BLOCK) void k_grp_short(GcArgs A) {
    const GcMat& M = A.m[blockIdx.y];
    const uint32_t row = blockIdx.x * GC_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= A.n_rows) return;
    const uint32_t lo = __builtin_amdgcn_readfirstlane(M.ptr[row]);
    const int len = (int)(__builtin_amdgcn_readfirstlane(M.ptr[row + 1]) - lo);
    if (len == 0) { if (!EMIT && lane == 0) M.cnt[row] = 0; return; }
    if ((uint32_t)len >= A.long_row) {                                    // k_grp_long's: it also writes the row's count
        if (!EMIT && lane == 0) M.list[atomicAdd(&A.ctl[blockIdx.y], 1u)] = row;
        return;
    }
    int g = -1, v = 0;
    if (lane < len) {
        const uint32_t c = (uint32_t)M.src[(size_t)M.nnz + lo + lane];
        if (c < A.n_cells) g = A.cg[c];
        v = M.src[2 * (size_t)M.nnz + lo + lane];
    }
    unsigned long long sum = 0;
    bool first = true;
    for (int j = 0; j < len; j++) {                                       // (j is uniform: scalar lane reads)
        const int gj = __builtin_amdgcn_readlane(g, j), vj = __builtin_amdgcn_readlane(v, j);
        if (gj == g) { sum += (unsigned long long)(uint32_t)vj; first = first && j >= lane; }
    }
    const bool head = g >= 0 && first;
    unsigned long long heads = __ballot(head);
    const uint32_t n_out = (uint32_t)__popcll(heads);
    if (!EMIT) {
        if (lane == 0) M.cnt[row] = n_out;
        if (head && sum > 0x7fffffffull) atomicOr(&A.ctl[3], 1u);
        return;
    }
    uint32_t rank = 0;
    while (heads) {
        const int j = __builtin_ctzll(heads);
        heads &= heads - 1;
        rank += __builtin_amdgcn_readlane(g, j) < g ? 1u : 0u;
    }
    if (head) {
        const uint32_t d = M.cnt[row] + rank;
        if (d < M.total) { M.out[d] = (int32_t)row; M.out[(size_t)M.total + d] = g; M.out[2 * (size_t)M.total + d] = (int32_t)sum; }   // (always: the total is the sum of what is placed here)
    }
}

template <bool EMIT>
__global__ __launch_bounds__(GC_BLOCK) void k_grp_long(GcArgs A) {
    __shared__ uint32_t s_tab[XCK_GROUP_MAX];
    __shared__ uint32_t s_w[GC_WAVES];
    const GcMat& M = A.m[blockIdx.y];
    const uint32_t n_long = A.ctl[blockIdx.y], ng = (uint32_t)A.n_groups;
    const uint32_t per = (ng + GC_BLOCK - 1) / GC_BLOCK, s0 = threadIdx.x * per, s1 = min(s0 + per, ng);
    for (uint32_t q = blockIdx.x; q < n_long; q += gridDim.x) {
        const uint32_t row = M.list[q], lo = M.ptr[row], hi = M.ptr[row + 1];
        for (uint32_t s = threadIdx.x; s < ng; s += GC_BLOCK) s_tab[s] = 0;
        __syncthreads();
        bool over = false;
        for (uint32_t i = lo + threadIdx.x; i < hi; i += GC_BLOCK) {
            const uint32_t c = (uint32_t)M.src[(size_t)M.nnz + i];
            const int g = c < A.n_cells ? A.cg[c] : -1;
            if (g < 0 || (uint32_t)g >= ng) continue;                     // (the second never: api.cpp checked the mapping)
            const uint32_t v = (uint32_t)M.src[2 * (size_t)M.nnz + i];
            const uint32_t old = atomicAdd(&s_tab[g], v);
            over = over || (unsigned long long)old + v > 0x7fffffffull;
        }
        if (!EMIT && over) atomicOr(&A.ctl[3], 1u);
        __syncthreads();
        uint32_t nz = 0;
        for (uint32_t s = s0; s < s1; s++) nz += s_tab[s] ? 1u : 0u;
        uint32_t total;
        uint32_t d = block_excl_scan_t<GC_BLOCK>(nz, s_w, total);
        if (!EMIT) { if (threadIdx.x == 0) M.cnt[row] = total; }
        else {
            d += M.cnt[row];
            for (uint32_t s = s0; s < s1; s++) {
                const uint32_t x = s_tab[s];
                if (!x) continue;
                if (d < M.total) { M.out[d] = (int32_t)row; M.out[(size_t)M.total + d] = (int32_t)s; M.out[2 * (size_t)M.total + d] = (int32_t)x; }
                d++;
            }
        }
        __syncthreads();                                                  // the table is cleared for the block's next row
    }
}

// the kernels of one call on the compute stream, between the shared steps of coo_call.h
static int group_counts_run(EngineImpl* im, const int32_t* const* src, const size_t* nnz, int nm, size_t n_rows, int n_groups, const int32_t* cell_group,
                            std::chrono::steady_clock::time_point t0) {
    CooCall& c = im->gc;
    // scratch: the control words (zero at the start) first, then the mapping, the scans' block sums and totals, the per-row arrays
    const size_t n_bsum = pf_scan_words(n_rows);
    ScratchLayout L;
    const int i_ctl = L.add(4 * 4), i_cg = L.add((size_t)im->n_cells * 4), i_bsum = L.add((n_bsum + 4) * 4), i_rows = L.add(3 * (3 * n_rows + 1) * 4);
    if (int rc = coo_scratch(im, c, L)) return rc;
    char* d = c.d_scratch;
    GcArgs A; memset(&A, 0, sizeof A);
    A.ctl = L.at<uint32_t>(d, i_ctl);
    int32_t* d_cg = L.at<int32_t>(d, i_cg); A.cg = d_cg;
    uint32_t* bsum = L.at<uint32_t>(d, i_bsum); uint32_t* d_tot = bsum + n_bsum;
    { uint32_t* w = L.at<uint32_t>(d, i_rows);
      for (int y = 0; y < nm; y++) { A.m[y].src = src[y]; A.m[y].nnz = (uint32_t)nnz[y]; A.m[y].ptr = w; A.m[y].cnt = w + n_rows + 1; A.m[y].list = w + 2 * n_rows + 1; w += 3 * n_rows + 1; } }
    A.n_rows = (uint32_t)n_rows; A.n_cells = (uint32_t)im->n_cells; A.n_groups = n_groups; A.long_row = (uint32_t)im->eng->knobs.group_long_row;
    const dim3 g_ptr((unsigned)((n_rows + 1 + GC_BLOCK - 1) / GC_BLOCK), nm), g_short((unsigned)((n_rows + GC_WAVES - 1) / GC_WAVES), nm), g_long(GC_LONG_GRID, nm);
    HIP_TRY(hipEventRecord(c.ev[0], im->s_comp));
    HIP_TRY(hipMemsetAsync(A.ctl, 0, 4 * 4, im->s_comp));
    HIP_TRY(hipMemsetAsync(d_tot, 0, 4 * 4, im->s_comp));
    HIP_TRY(hipMemcpyAsync(d_cg, cell_group, (size_t)im->n_cells * 4, hipMemcpyHostToDevice, im->s_comp));
    hipLaunchKernelGGL(k_grp_row_ptr, g_ptr, dim3(GC_BLOCK), 0, im->s_comp, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c.ev[1], im->s_comp));
    hipLaunchKernelGGL(k_grp_short<false>, g_short, dim3(GC_BLOCK), 0, im->s_comp, A);
    hipLaunchKernelGGL(k_grp_long<false>, g_long, dim3(GC_BLOCK), 0, im->s_comp, A);
    HIP_TRY(hipGetLastError());
    for (int y = 0; y < nm; y++) if (int rc = pf_scan(im, A.m[y].cnt, n_rows, bsum, d_tot + y)) return rc;
    if (int rc = coo_publish_totals(im, c, d_tot, nm, A.ctl + 3)) return rc;
    if (c.h_tot[COO_FLAG_WORD]) { im->eng->err = "xck_group_counts: the sum of a group does not fit int32"; return XCK_E_CAPACITY; }
    int32_t* d_out[3];
    if (int rc = coo_reserve(im, c, d_out)) return rc;
    for (int y = 0; y < nm; y++) { A.m[y].total = (uint32_t)c.nnz[y]; A.m[y].out = d_out[y]; }
    if (coo_words(c)) {
        hipLaunchKernelGGL(k_grp_short<true>, g_short, dim3(GC_BLOCK), 0, im->s_comp, A);
        hipLaunchKernelGGL(k_grp_long<true>, g_long, dim3(GC_BLOCK), 0, im->s_comp, A);
        HIP_TRY(hipGetLastError());
    }
    return coo_deliver(im, c, t0);
}

// One pipeline's share of xck_group_counts: a basefc pipeline fills out->count, a pileup pipeline out->ad / dp / oth; the rest of *out is
// left alone (api.cpp clears it and merges the pipelines of a fused handle, and adds up their times in *gt).  The arguments were checked there.
int engine_group_counts(EngineImpl* im, int source, int n_groups, const int32_t* cell_group, xck_result* out, GroupTimes* gt) {
    xck_engine* e = im->eng;
    CooCall& c = im->gc;
    if (im->fold_failed || !im->finished) { e->err = "xck_group_counts: valid between a successful xck_finish and the next xck_reset"; return XCK_E_STATE; }
    const bool snp = source == XCK_GROUP_SRC_SNP;
    if (snp && !im->sc_valid) { e->err = "xck_group_counts: source SNP needs an xck_snp_counts since the last xck_finish / xck_reset"; return XCK_E_STATE; }
    const bool baf = im->mode == XCK_MODE_BAF;
    const int nm = baf ? 3 : 1;
    const int32_t* src[3] = {nullptr, nullptr, nullptr}; size_t nnz[3] = {0, 0, 0}, any = 0;
    for (int y = 0; y < nm; y++) {
        nnz[y] = snp ? im->sc.nnz[y] : im->res_nnz[(baf ? 1 : 0) + y];
        if (nnz[y] >> 32) { e->err = "xck_group_counts: a source matrix holds 2^32 entries or more: the row pointers are 32-bit"; return XCK_E_CAPACITY; }
        any += nnz[y];
    }
    if (snp) { size_t at = 0; for (int y = 0; y < 3; y++) { src[y] = im->sc.d_res + at; at += 3 * nnz[y]; } }
    else for (int y = 0; y < nm; y++) {
        src[y] = im->d_res[(baf ? 1 : 0) + y];
        if (nnz[y] && !src[y]) { e->err = "internal: result block without a device copy"; return XCK_E_STATE; }
    }
    const size_t n_rows = snp ? (size_t)im->n_snps_in : (size_t)im->n_regions;
    HIP_TRY(hipSetDevice(im->device));
    const auto t0 = std::chrono::steady_clock::now();
    clear_stale_error("group_counts", e->knobs.debug_timing);
    if (int rc = coo_begin(im, c)) return rc;
    if (any && n_rows)
        if (int rc = group_counts_run(im, src, nnz, nm, n_rows, n_groups, cell_group, t0)) return coo_fail(im, rc);
    gt->ms_total += c.ms_total; gt->ms_ptr += c.ms_phase[0]; gt->ms_count += c.ms_phase[1]; gt->ms_emit += c.ms_phase[2]; gt->ms_copy += c.ms_copy;
    gt->entries += (long long)any;
    xck_coo* const dst[3] = { baf ? &out->ad : &out->count, &out->dp, &out->oth };
    coo_fill(c, nm, dst);
    for (int y = 0; y < nm; y++) gt->nnz[(baf ? 1 : 0) + y] = (long long)c.nnz[y];
    return 0;
}
