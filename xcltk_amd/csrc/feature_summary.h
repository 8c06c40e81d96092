// feature_summary.h - opt-in per-feature and per-SNP tables (XCK_F_FEATURE_SUMMARY / XCK_FEATURE_SUMMARY=1; xck_get_feature_summary,
// include/xck.h).  Included by engine.hip inside namespace xck, behind read_fate.h: it uses that file's FateArgs, read_fate_walk and
// rf_targets (the read filter and the accept rule are stated there and nowhere else), the grouped accumulation and the marginal
// launcher (launch_marginals, k_cell_marginals) of cell_summary.h, and snp_verdicts() of finish.hip.
//
// The read half.  One more pass over the batches the join has just been launched on, like k_read_fate - but where a read adds one
// (row, column) to the per-cell table it adds one per (read, region) pair or covered SNP to these, so the loop is a different one:
//   basefc  per fetched region of a read that passes the filter: include_fail, or pairs - and shared when two or more regions
//           accept the read.  A count walk (read_fate_walk) gives the read's number of accepting regions, a second walk (rf_targets,
//           resumed region by region) attributes the pairs.
//   pileup  per SNP under the read's fetch span: reads.
// The mirror image of DESIGN.md 3.5: in a coordinate-sorted 10x file the 1024 reads of a tile sit in the same one to ten regions
// and over the same few dozen SNPs, so almost everything combines; with one tiny region per read nothing does.  The second walk
// is a WAVE loop: in each round every lane offers its next candidate or nothing, and cs_add() (cell_summary.h) collapses the lanes
// that offer the same row - the lanes of a hot gene walk the same list, so they offer the same region in the same round.  The
// waves meet in an LDS table keyed by row (three counters a row for regions, one for SNPs), and a tile whose rows fit it ends
// in at most one 64-bit atomic per occupied (row, column); rows that do not fit go straight to HBM.
//
// The tables in HBM are indexed by the caller's region index (reg_row) and by the engine's sorted SNP index; the host turns the
// latter into the caller's order (EngineImpl::snp_perm).
#pragma once

constexpr int FS_SLOTS = 1024;            // rows of the LDS table: 1024 * 16 B + list = 18 KB (regions), 1024 * 8 B + list = 10 KB (SNPs)
constexpr int FS_REG_WORDS = 4;           // 64-bit words of a region's row in HBM: include_fail, pairs, shared, padding
constexpr int FS_INCLUDE_FAIL = 0, FS_PAIRS = 1, FS_SHARED = 2, FS_READ_COLS = 3;
constexpr int FS_SNP_COLS = 8;            // xck_feature_summary.snp: reads, a c g t n, kept, regions
template <int MODE> struct FeatLds { typedef SumLds<MODE == XCK_MODE_BASEFC ? FS_READ_COLS : 1, FS_SLOTS, false> type; };

template <int MODE>
__global__ __launch_bounds__(JOIN_BLOCK) void k_feature_fate(FateArgs a, const int32_t* reg_row, CellArgs ca) {
    __shared__ typename FeatLds<MODE>::type s;
    const int tid = threadIdx.x, lane = tid & 63;
    cs_init(s, ca, tid);
    __syncthreads();
    const int t = blockIdx.x;
    int lo = 0, hi = a.bt.n_batches - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.bt.desc[mid].tile0 <= t) lo = mid; else hi = mid - 1; }
    const BatchDesc& d = a.bt.desc[lo];
    const int32_t r0 = (t - d.tile0) * TILE;
#pragma unroll 1
    for (int j = 0; j < TILE_ITEMS; j++) {
        const int32_t i = r0 + j * JOIN_BLOCK + tid;
        RfSpan sp = {}; uint32_t np = 0;
        if (MODE == XCK_MODE_BASEFC) {
            // the count walk: np = regions that accept the read, k = the first region that fetches it
            int32_t k = d.reg_hi;
            if (i < d.n) read_fate_walk<MODE>(a, d, i, np, sp, [&](int32_t q, bool) { k = min(k, q); return true; }, [](int32_t, int32_t) {});
            const bool shared = np >= 2u;
            // the contributing walk: in every round a lane offers its next fetched region, if it has one left
            while (__ballot(k < d.reg_hi)) {
                int col = -1; int32_t at = d.reg_hi; uint32_t np1 = 0;
                if (k < d.reg_hi) rf_targets<MODE>(a, d, sp, k, np1, [&](int32_t q, bool acc) { at = q; col = acc ? FS_PAIRS : FS_INCLUDE_FAIL; return false; }, [](int32_t, int32_t) {});
                k = at < d.reg_hi ? at + 1 : d.reg_hi;
                const int32_t row = col >= 0 ? as_global(reg_row)[at] : 0;
                cs_add(s, ca, lane, col >= 0, row, col, 0u, col == FS_PAIRS && shared, FS_SHARED);
            }
        } else {
            int32_t k0 = 0, k1 = 0;
            if (i < d.n) read_fate_walk<MODE>(a, d, i, np, sp, [](int32_t, bool) { return true; }, [&](int32_t q0, int32_t q1) { k0 = q0; k1 = q1; });
            for (; __ballot(k0 < k1); k0++) cs_add(s, ca, lane, k0 < k1, k0, 0, 0u, false, 0);
        }
    }
    __syncthreads();
    cs_flush(s, ca, tid);
}

// the tables' own memory (summaries_init; off: nothing), and their zeroing on s_comp (summaries_reset)
static int feature_summary_init(EngineImpl* im) {
    const size_t words = im->mode == XCK_MODE_BASEFC ? (size_t)im->n_regions * FS_REG_WORDS : (size_t)im->n_snps_sorted;
    if (const int rc = dev_zeroed(im, (void**)&im->d_feat, std::max<size_t>(words, 1) * sizeof(unsigned long long))) return rc;
    im->fmat_cap_bytes = std::max<size_t>((size_t)im->n_regions * 6, 1) * sizeof(unsigned long long);
    HIP_TRY(hipMalloc((void**)&im->d_fmat, im->fmat_cap_bytes));
    if (im->mode == XCK_MODE_BAF) {
        // (a finish that finds no hit returns before the fold clears the tallies: they start, and after every reset are, zero)
        HIP_TRY(hipMemset(im->d_tally, 0, std::max<size_t>((size_t)im->n_snps_sorted * 5, 1) * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void**)&im->d_kept, std::max<size_t>((size_t)im->n_snps_sorted, 1) * sizeof(uint32_t)));
    }
    return 0;
}
static int feature_summary_reset(EngineImpl* im) {
    const size_t words = im->mode == XCK_MODE_BASEFC ? (size_t)im->n_regions * FS_REG_WORDS : (size_t)im->n_snps_sorted;
    HIP_TRY(hipMemsetAsync(im->d_feat, 0, std::max<size_t>(words, 1) * sizeof(unsigned long long), im->s_comp));
    if (im->mode == XCK_MODE_BAF) HIP_TRY(hipMemsetAsync(im->d_tally, 0, std::max<size_t>((size_t)im->n_snps_sorted * 5, 1) * sizeof(uint32_t), im->s_comp));
    im->fmat_valid = false;
    return 0;
}

// Runs once per batch, where launch_read_fate() runs: behind the FIRST join launch of the batches in im->inflight, on the same stream,
// never from the overflow replay.
static int launch_feature_fate(EngineImpl* im) {
    if (!im->d_feat || im->inflight.empty()) return 0;
    FateArgs a;
    const int32_t tiles = fill_fate_args(im, a);                 // (a.out stays null: nothing of the global words is written here)
    CellArgs ca;
    ca.tab = im->d_feat; ca.slot_mask = cs_slot_mask(im, FS_SLOTS); ca.c32_base = 0; ca.wide_col = 0;
    if (im->mode == XCK_MODE_BASEFC) {
        ca.n_rows = im->n_regions; ca.stride = FS_REG_WORDS;
        hipLaunchKernelGGL((k_feature_fate<XCK_MODE_BASEFC>), dim3(tiles), dim3(JOIN_BLOCK), 0, im->s_comp, a, (const int32_t*)im->d_reg_row, ca);
    } else {
        ca.n_rows = im->n_snps_sorted; ca.stride = 1;
        hipLaunchKernelGGL((k_feature_fate<XCK_MODE_BAF>), dim3(tiles), dim3(JOIN_BLOCK), 0, im->s_comp, a, (const int32_t*)nullptr, ca);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// row marginals of the matrices of the last finish -> im->h_fmat ([n_regions * k]), and for the pileup the tallies and verdicts of
// its SNPs -> im->h_tally / im->h_kept (sorted SNP order); once per finish.  launch_marginals() of cell_summary.h, keyed by the ROW
// array of a result block.
static int feature_marginals(EngineImpl* im, const int k) {
    const bool baf = im->mode != XCK_MODE_BASEFC;
    HIP_TRY(hipMemsetAsync(im->d_fmat, 0, std::max<size_t>((size_t)im->n_regions * k, 1) * sizeof(unsigned long long), im->s_comp));
    // basefc: umis = row sums of count, cells = its entries; BAF: snps, snps_kept (host, below), ad, dp, oth sums, cells = entries of DP
    const MargJob fc[1] = { {0, 0, 1} }, pile[3] = { {1, 2, -1}, {2, 3, 5}, {3, 4, -1} };
    if (int rc = launch_marginals(im, baf ? pile : fc, baf ? 3 : 1, true, im->d_fmat, im->n_regions, k)) return rc;
    im->h_fmat.resize((size_t)im->n_regions * k);
    if (!im->h_fmat.empty()) HIP_TRY(hipMemcpyAsync(im->h_fmat.data(), im->d_fmat, im->h_fmat.size() * sizeof(int64_t), hipMemcpyDeviceToHost, im->s_comp));
    if (baf) {
        const size_t ns = (size_t)im->n_snps_sorted;
        if (int rc = snp_verdicts(im, im->d_kept)) return rc;
        im->h_tally.resize(ns * 5); im->h_kept.resize(ns);
        if (ns) {
            HIP_TRY(hipMemcpyAsync(im->h_tally.data(), cur_tally(im), ns * 5 * sizeof(uint32_t), hipMemcpyDeviceToHost, im->s_comp));
            HIP_TRY(hipMemcpyAsync(im->h_kept.data(), im->d_kept, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, im->s_comp));
        }
        if (im->csr_host_stale) {                              // xck_refold built new SNP -> region tables on the device
            im->h_csr_off.resize(ns + 1);
            HIP_TRY(hipMemcpy(im->h_csr_off.data(), im->d_csr_off, (ns + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
            im->h_csr_reg.resize((size_t)im->h_csr_off[ns]);
            if (!im->h_csr_reg.empty()) HIP_TRY(hipMemcpy(im->h_csr_reg.data(), im->d_csr_reg, im->h_csr_reg.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            im->csr_host_stale = false;
        }
    }
    HIP_TRY(hipStreamSynchronize(im->s_comp));
    if (baf)                                                   // snps, snps_kept per region from the (small) SNP -> region relation
        for (size_t s = 0; s + 1 < im->h_csr_off.size(); s++)
            for (int32_t q = im->h_csr_off[s]; q < im->h_csr_off[s + 1]; q++) {
                int64_t* row = &im->h_fmat[(size_t)im->h_csr_reg[q] * k];
                row[0]++; row[1] += im->h_kept[s] ? 1 : 0;
            }
    return 0;
}

// xck_get_feature_summary() for one pipeline: waits for the queued work, copies the read half; the matrix half (and the tallies and
// verdicts of the SNPs) runs the first time after a finish and is kept until the next reset (a finished handle takes no more reads)
int engine_feature_summary(EngineImpl* im, xck_feature_summary* out) {
    if (!im->d_feat) { im->eng->err = "handle made without XCK_F_FEATURE_SUMMARY"; return XCK_E_STATE; }
    int rc = engine_flush(im); if (rc) return rc;
    const bool baf = im->mode != XCK_MODE_BASEFC;
    const size_t words = baf ? (size_t)im->n_snps_sorted : (size_t)im->n_regions * FS_REG_WORDS;
    im->h_feat_raw.resize(words);
    if (words) HIP_TRY(hipMemcpy(im->h_feat_raw.data(), im->d_feat, words * sizeof(int64_t), hipMemcpyDeviceToHost));
    const int k = baf ? 6 : 2;
    if (im->finished && !im->fmat_valid) { rc = feature_marginals(im, k); if (rc) return rc; im->fmat_valid = true; }
    out->mode = im->mode; out->n_regions = im->n_regions;
    out->has_matrix = im->finished ? 1 : 0; out->n_matrix_cols = k; out->matrix = im->finished ? im->h_fmat.data() : nullptr;
    if (!baf) {
        im->h_feat.resize((size_t)im->n_regions * FS_READ_COLS);
        for (size_t g = 0; g < (size_t)im->n_regions; g++) for (int c = 0; c < FS_READ_COLS; c++) im->h_feat[g * FS_READ_COLS + c] = im->h_feat_raw[g * FS_REG_WORDS + c];
        out->n_read_cols = FS_READ_COLS; out->reads = im->h_feat.data();
        return 0;
    }
    // per SNP, in the caller's order: a SNP the tables left out (contig outside the table, pos < 1) keeps a row of zeros
    im->h_feat.assign((size_t)im->n_snps_in * FS_SNP_COLS, 0);
    for (size_t s = 0; s < (size_t)im->n_snps_sorted; s++) {
        int64_t* row = &im->h_feat[(size_t)im->snp_perm[s] * FS_SNP_COLS];
        row[0] = im->h_feat_raw[s];
        if (im->finished) { for (int c = 0; c < 5; c++) row[1 + c] = im->h_tally[s * 5 + c]; row[6] = im->h_kept[s] ? 1 : 0; }
        row[7] = im->h_csr_off[s + 1] - im->h_csr_off[s];
    }
    out->n_snps = im->n_snps_in; out->n_snp_cols = FS_SNP_COLS; out->snp = im->h_feat.data();
    return 0;
}
