// refold.h - xck_refold (include/xck.h): the region stage of the pileup fold again, under new regions, REF / ALT, haplotype indices,
// exclusion pairs and per-SNP filters, on the molecule stage the last xck_finish left (finish.hip fold_molecules / fold_regions).
// Included by finish.hip inside namespace xck, behind fold_partition.h and coo_call.h: it uses the device-wide scan of the first (pf_scan)
// and lays out its upload block with the ScratchLayout of the second.
//
// The SNP -> region tables (d_csr_off / d_csr_reg) are built on the device.  The host handles only tables of at most n_regions
// entries: it validates the regions, sorts them per contig by (start, end, index) with the running maximum of the ends
// (sort_regions_by_contig, the code xck_create uses for the basefc table) and turns the exclusion pairs into sorted words
// `sorted SNP index << 32 | region`.  One thread per SNP of the sorted table then finds its first candidate by one bisection over the
// running maxima and walks the regions up to the first that starts behind the SNP, keeping those that contain it and are not
// excluded.  The same kernel runs twice, as k_expand does: a count pass, a device-wide exclusive scan of the counts (which is
// csr_off), and a fill pass.  The order of a SNP's list is free: k_expand's output is sorted next.
//
// Bound of the walk: a SNP visits the regions of its contig from the first whose running maximum reaches its position to the
// last that starts at or before it.  Tables whose regions nest little (genes, bins) give a walk of a few regions; one region that
// spans the contig and sorts first makes every SNP walk all regions left of it (DESIGN.md 3.7 states the bound and the measured time).
#pragma once

constexpr int RF_BLOCK = 256;

struct RefoldTabs {
    const int32_t* snp_p0; const uint8_t* enabled;                       // per sorted SNP: 0-based position; 0 = feeds no region (null = all feed)
    const int32_t *ct_snp_end, *ct_reg_base, *ct_reg_n; int32_t n_ct;    // per contig: one past its last sorted SNP, its slice of the sorted regions
    const int32_t *start, *end, *row, *pmax;                             // the sorted regions: 1-based inclusive bounds, the caller's index, running maximum of the ends
    const unsigned long long* excl; int32_t n_excl;                      // sorted (sorted SNP index << 32 | region)
    uint32_t n_snps;
};

// COUNT pass (EMIT = false): cnt[s] = regions of sorted SNP s for s < n_snps, cnt[n_snps] = 0 (the scan turns cnt into csr_off), and
// their sum, in 64 bits, added to *total.  EMIT pass: reg[off[s] ..] = the regions.
template <bool EMIT>
__global__ __launch_bounds__(RF_BLOCK) void k_snp_regions(RefoldTabs t, uint32_t* __restrict__ cnt, const int32_t* __restrict__ off, int32_t* __restrict__ reg,
                                                          unsigned long long* __restrict__ total) {
    const uint32_t s = blockIdx.x * RF_BLOCK + threadIdx.x;
    uint32_t c = 0;
    if (s < t.n_snps && (!t.enabled || t.enabled[s])) {
        int32_t lo = 0, hi = t.n_ct - 1;                                 // the SNP's contig: the first whose SNPs end behind s
        while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if ((int32_t)s < t.ct_snp_end[mid]) hi = mid; else lo = mid + 1; }
        const int32_t rb = t.ct_reg_base[lo], rn = t.ct_reg_n[lo];
        const int32_t pos = t.snp_p0[s] + 1;
        int32_t a = 0, b = rn;                                           // first region whose running maximum of the ends reaches pos
        while (a < b) { const int32_t mid = (a + b) >> 1; if (t.pmax[rb + mid] >= pos) b = mid; else a = mid + 1; }
        const int32_t dst = EMIT ? off[s] : 0;
        for (int32_t j = a; j < rn && t.start[rb + j] <= pos; j++) {
            if (t.end[rb + j] < pos) continue;
            const int32_t g = t.row[rb + j];
            if (t.n_excl) {
                const unsigned long long w = ((unsigned long long)s << 32) | (uint32_t)g;
                int32_t x = 0, y = t.n_excl;
                while (x < y) { const int32_t mid = (x + y) >> 1; if (t.excl[mid] < w) x = mid + 1; else y = mid; }
                if (x < t.n_excl && t.excl[x] == w) continue;
            }
            if (EMIT) reg[dst + (int32_t)c] = g;
            c++;
        }
    }
    if (!EMIT) {
        if (s <= t.n_snps) cnt[s] = c;
        unsigned long long sum = c;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(total, sum);
    }
}

static size_t refold_slack(size_t need) { return need / 4 + 4096; }      // head room of the grow-only buffers of this file (grow_device)

// what the host hands to the builder: one block, one copy
struct RefoldHost {
    std::vector<int32_t> start, end, row, pmax, ct_snp_end, ct_reg_base, ct_reg_n;
    std::vector<unsigned long long> excl;
    std::vector<uint8_t> enabled;
    std::vector<uint32_t> info;
};

static int refold_check(EngineImpl* im, const xck_refold_config* cfg) {
    xck_engine* e = im->eng;
    char b[320];
    if (cfg->n_regions < 0 || (cfg->n_regions > 0 && !cfg->regions)) { e->err = "xck_refold: invalid region table"; return XCK_E_ARG; }
    if ((int64_t)cfg->n_regions + 1 > (int64_t(1) << im->rbits)) {
        snprintf(b, sizeof b, "xck_refold: n_regions + 1 = %lld does not fit the %d-bit row field of this handle's key layout (sized at xck_create from max(n_regions, n_snps) + 1): "
                 "at most %lld regions", (long long)cfg->n_regions + 1, im->rbits, (long long)((int64_t(1) << im->rbits) - 1));
        e->err = b; return XCK_E_ARG;
    }
    if (cfg->snps || cfg->n_snps) {
        if (!cfg->snps || cfg->n_snps != im->n_snps_in) { e->err = "xck_refold: the SNP list must have the handle's number of SNPs"; return XCK_E_ARG; }
        for (int i = 0; i < cfg->n_snps; i++)
            if (cfg->snps[i].contig != im->snps_in[i].contig || cfg->snps[i].pos != im->snps_in[i].pos) {
                snprintf(b, sizeof b, "xck_refold: SNP %d is at another (contig, pos) than in the handle's list (only ref, alt, ref_hap, alt_hap may differ)", i);
                e->err = b; return XCK_E_ARG;
            }
    }
    if (cfg->n_excl_pairs < 0 || (cfg->n_excl_pairs > 0 && (!cfg->excl_region || !cfg->excl_snp))) { e->err = "xck_refold: invalid exclusion pairs"; return XCK_E_ARG; }
    for (int i = 0; i < cfg->n_excl_pairs; i++)
        if (cfg->excl_region[i] < 0 || cfg->excl_region[i] >= cfg->n_regions || cfg->excl_snp[i] < 0 || cfg->excl_snp[i] >= im->n_snps_in) {
            snprintf(b, sizeof b, "xck_refold: exclusion pair %d names a region or a SNP outside the tables", i);
            e->err = b; return XCK_E_ARG;
        }
    return 0;
}

static void refold_host_tables(const EngineImpl* im, const xck_refold_config* cfg, RefoldHost& h) {
    const int nc = (int)im->ctab.size();
    const size_t ns = (size_t)im->n_snps_sorted;
    sort_regions_by_contig(cfg->regions, cfg->n_regions, nc, [](const xck_region& r) { return r.end >= r.start; }, [](const xck_region& r) { return r.start; },
                           h.start, h.end, h.row, h.pmax, h.ct_reg_base, h.ct_reg_n);
    h.ct_snp_end.resize(nc);
    for (int c = 0; c < nc; c++) h.ct_snp_end[c] = im->ctab[c].snp_base + im->ctab[c].n_snp;
    if (cfg->snp_enabled) { h.enabled.resize(ns); for (size_t s = 0; s < ns; s++) h.enabled[s] = cfg->snp_enabled[im->snp_perm[s]] ? 1 : 0; }
    if (cfg->n_excl_pairs > 0) {
        std::vector<int32_t> inv((size_t)im->n_snps_in, -1);              // the caller's index -> sorted SNP (-1: the tables left it out)
        for (size_t s = 0; s < ns; s++) inv[(size_t)im->snp_perm[s]] = (int32_t)s;
        for (int i = 0; i < cfg->n_excl_pairs; i++) {
            const int32_t s = inv[(size_t)cfg->excl_snp[i]];
            if (s >= 0) h.excl.push_back(((unsigned long long)(uint32_t)s << 32) | (uint32_t)cfg->excl_region[i]);
        }
        std::sort(h.excl.begin(), h.excl.end());
    }
    if (cfg->snps) {
        h.info.resize(ns);
        for (size_t s = 0; s < ns; s++) {
            const xck_snp& x = cfg->snps[im->snp_perm[s]];
            h.info[s] = snp_info_word(x);
        }
    }
}

// upload + count + scan + fill: the new d_csr_off / d_csr_reg / d_snp_info.  Up to the check of the total nothing of the handle's
// tables is touched.
static int refold_build_tables(EngineImpl* im, const xck_refold_config* cfg, bool* touched) {
    const auto t0 = std::chrono::steady_clock::now();
    RefoldHost h;
    refold_host_tables(im, cfg, h);
    const size_t ns = (size_t)im->n_snps_sorted, nsb = (ns + 1 + SC_TILE - 1) / SC_TILE;
    const struct { const void* src; size_t bytes; } up[9] = {
        { h.start.data(), h.start.size() * 4 }, { h.end.data(), h.end.size() * 4 }, { h.row.data(), h.row.size() * 4 }, { h.pmax.data(), h.pmax.size() * 4 },
        { h.ct_snp_end.data(), h.ct_snp_end.size() * 4 }, { h.ct_reg_base.data(), h.ct_reg_base.size() * 4 }, { h.ct_reg_n.data(), h.ct_reg_n.size() * 4 },
        { h.excl.data(), h.excl.size() * 8 }, { h.enabled.data(), h.enabled.size() } };
    ScratchLayout L;                                                      // (coo_call.h) the uploaded tables - an empty one still takes four bytes -, then the scan's block sums
    for (const auto& u : up) L.add(std::max<size_t>(u.bytes, 4));
    const int i_bsum = L.add(nsb * 4);
    if (int rc = grow_device(im, (void**)&im->d_rf, &im->rf_cap, L.total(), refold_slack(L.total()))) return rc;
    if (!im->d_csr_alt) HIP_TRY(hipMalloc((void**)&im->d_csr_alt, (ns + 1) * sizeof(int32_t)));
    if (!im->ev_r0) { HIP_TRY(hipEventCreate(&im->ev_r0)); HIP_TRY(hipEventCreate(&im->ev_r1)); HIP_TRY(hipEventCreate(&im->ev_r2)); HIP_TRY(hipEventCreate(&im->ev_r3)); }
    { std::vector<char> blk(L.offs[i_bsum]);
      for (int q = 0; q < 9; q++) if (up[q].bytes) memcpy(blk.data() + L.offs[q], up[q].src, up[q].bytes);
      if (!blk.empty()) HIP_TRY(hipMemcpyAsync(im->d_rf, blk.data(), blk.size(), hipMemcpyHostToDevice, im->s_comp));
      HIP_TRY(hipStreamSynchronize(im->s_comp)); }
    im->rf_ms_upload = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    RefoldTabs t;
    t.snp_p0 = im->d_snp_p0; t.enabled = cfg->snp_enabled ? L.at<const uint8_t>(im->d_rf, 8) : nullptr;
    t.ct_snp_end = L.at<const int32_t>(im->d_rf, 4); t.ct_reg_base = L.at<const int32_t>(im->d_rf, 5); t.ct_reg_n = L.at<const int32_t>(im->d_rf, 6);
    t.n_ct = (int32_t)h.ct_snp_end.size();
    t.start = L.at<const int32_t>(im->d_rf, 0); t.end = L.at<const int32_t>(im->d_rf, 1); t.row = L.at<const int32_t>(im->d_rf, 2); t.pmax = L.at<const int32_t>(im->d_rf, 3);
    t.excl = L.at<const unsigned long long>(im->d_rf, 7); t.n_excl = (int32_t)h.excl.size();
    t.n_snps = (uint32_t)ns;
    uint32_t* bsum = L.at<uint32_t>(im->d_rf, i_bsum);
    const unsigned grid = (unsigned)((ns + 1 + RF_BLOCK - 1) / RF_BLOCK);
    HIP_TRY(hipEventRecord(im->ev_r0, im->s_comp));
    HIP_TRY(hipMemsetAsync(im->d_ctl + CTL_SCRATCH, 0, sizeof(unsigned long long), im->s_comp));
    hipLaunchKernelGGL((k_snp_regions<false>), dim3(grid), dim3(RF_BLOCK), 0, im->s_comp, t, (uint32_t*)im->d_csr_alt, (const int32_t*)nullptr, (int32_t*)nullptr, im->d_ctl + CTL_SCRATCH);
    HIP_TRY(hipGetLastError());
    if (int rc = pf_scan(im, (uint32_t*)im->d_csr_alt, ns + 1, bsum, nullptr)) return rc;
    HIP_TRY(hipEventRecord(im->ev_r1, im->s_comp));
    const unsigned long long* h_total;
    if (int rc = read_ctl_words(im, CTL_SCRATCH, 1, h_total)) return rc;
    const unsigned long long total = *h_total;
    if (total > (unsigned long long)INT32_MAX) {
        char b[200]; snprintf(b, sizeof b, "xck_refold: %llu (SNP, region) pairs: the SNP -> region table holds at most 2^31 - 1", total);
        im->eng->err = b; return XCK_E_NOMEM;
    }
    *touched = true;
    const size_t reg_bytes = std::max<size_t>((size_t)total, 1) * sizeof(int32_t);
    if (int rc = grow_device(im, (void**)&im->d_csr_reg, &im->csr_reg_cap_bytes, reg_bytes, refold_slack(reg_bytes))) return rc;
    HIP_TRY(hipEventRecord(im->ev_r2, im->s_comp));
    hipLaunchKernelGGL((k_snp_regions<true>), dim3(grid), dim3(RF_BLOCK), 0, im->s_comp, t, (uint32_t*)nullptr, (const int32_t*)im->d_csr_alt, im->d_csr_reg, (unsigned long long*)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(im->ev_r3, im->s_comp));
    std::swap(im->d_csr_off, im->d_csr_alt);
    if (!h.info.empty()) {
        const auto t1 = std::chrono::steady_clock::now();
        HIP_TRY(hipMemcpyAsync(im->d_snp_info, h.info.data(), h.info.size() * sizeof(uint32_t), hipMemcpyHostToDevice, im->s_comp));
        HIP_TRY(hipStreamSynchronize(im->s_comp));                          // (h.info leaves with this function)
        im->rf_ms_upload += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    }
    return 0;
}

// The cell mask of a call as a bit table, one bit per cell of the handle; empty = the call counts every cell (a NULL mask, or one that
// enables all: both take the unmasked kernels).
static std::vector<uint32_t> refold_cell_bits(const EngineImpl* im, const uint8_t* cell_enabled) {
    std::vector<uint32_t> w;
    if (!cell_enabled) return w;
    bool all = true;
    for (int c = 0; c < im->n_cells; c++) all = all && cell_enabled[c];
    if (all) return w;
    w.assign(((size_t)im->n_cells + 31) / 32, 0u);
    for (int c = 0; c < im->n_cells; c++) if (cell_enabled[c]) w[(size_t)c >> 5] |= 1u << (c & 31);
    return w;
}

// Per-SNP tallies of the molecules of the enabled cells, from what the molecule stage left (mol_keys / mol_al): the bit table goes up,
// one bisection per SNP finds its slice of the sorted hits (k_first_base's bounds exist on the split path only, and workspace 1 is not
// this call's to take from), and the masked forms of k_tally_rows / k_tally_long count.  Everything lives in one grow-only block of its
// own (d_cm), so the handle's tallies over all cells stay for the next call without a mask.
template <class K>
static int refold_mask_tallies(EngineImpl* im, const std::vector<uint32_t>& bits) {
    const size_t ns = std::max<size_t>((size_t)im->n_snps_sorted, 1), n = im->mol_n, nw = bits.size();
    const KeyLayout<K> kl = key_layout<K>(im);
    ScratchLayout L;
    const int i_bits = L.add(nw * 4), i_lo = L.add((ns + 1) * 8), i_long = L.add((n / (size_t)TALLY_LONG + 2) * 8), i_tally = L.add(ns * 5 * 4);
    if (int rc = grow_device(im, (void**)&im->d_cm, &im->cm_cap, L.total(), refold_slack(L.total()))) return rc;
    if (!im->ev_m0) { HIP_TRY(hipEventCreate(&im->ev_m0)); HIP_TRY(hipEventCreate(&im->ev_m1)); }
    uint32_t* d_bits = L.at<uint32_t>(im->d_cm, i_bits); unsigned long long* row_lo = L.at<unsigned long long>(im->d_cm, i_lo);
    unsigned long long* long_rows = L.at<unsigned long long>(im->d_cm, i_long); uint32_t* tally = L.at<uint32_t>(im->d_cm, i_tally);
    HIP_TRY(hipEventRecord(im->ev_m0, im->s_comp));
    HIP_TRY(hipMemcpyAsync(d_bits, bits.data(), nw * 4, hipMemcpyHostToDevice, im->s_comp));
    HIP_TRY(hipMemsetAsync(tally, 0, ns * 5 * sizeof(uint32_t), im->s_comp));          // (the pieces of a deep SNP add to its counters)
    HIP_TRY(hipMemsetAsync(long_rows, 0, sizeof(unsigned long long), im->s_comp));
    if (n) {
        const K* keys = (const K*)im->mol_keys;
        hipLaunchKernelGGL((k_row_bounds<K>), dim3((unsigned)((ns + 1 + 255) / 256)), dim3(256), 0, im->s_comp, keys, (long long)n, kl, (uint32_t)ns, row_lo);
        const dim3 g_rows((unsigned)((ns * 8 + 255) / 256)), g_long(1024);
        if (nw <= CM_LDS_WORDS) {
            hipLaunchKernelGGL((k_tally_rows_cells<K, true>), g_rows, dim3(256), 0, im->s_comp, keys, (const uint8_t*)im->mol_al, kl, (const unsigned long long*)row_lo, (uint32_t)ns,
                               (const uint32_t*)d_bits, (uint32_t)nw, tally, long_rows);
            hipLaunchKernelGGL((k_tally_long_cells<K, true>), g_long, dim3(256), 0, im->s_comp, keys, (const uint8_t*)im->mol_al, kl, (const unsigned long long*)row_lo,
                               (const uint32_t*)d_bits, (uint32_t)nw, (const unsigned long long*)long_rows, tally);
        } else {
            hipLaunchKernelGGL((k_tally_rows_cells<K, false>), g_rows, dim3(256), 0, im->s_comp, keys, (const uint8_t*)im->mol_al, kl, (const unsigned long long*)row_lo, (uint32_t)ns,
                               (const uint32_t*)d_bits, (uint32_t)nw, tally, long_rows);
            hipLaunchKernelGGL((k_tally_long_cells<K, false>), g_long, dim3(256), 0, im->s_comp, keys, (const uint8_t*)im->mol_al, kl, (const unsigned long long*)row_lo,
                               (const uint32_t*)d_bits, (uint32_t)nw, (const unsigned long long*)long_rows, tally);
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(im->ev_m1, im->s_comp));
    HIP_TRY(hipStreamSynchronize(im->s_comp));                                          // (`bits` is the caller's local)
    im->d_tally_cur = tally; im->d_cell_bits = d_bits;
    return 0;
}

int engine_refold(EngineImpl* im, const xck_refold_config* cfg, xck_result* out) {
    xck_engine* e = im->eng;
    if (im->fold_failed) { e->err = "xck_refold: an earlier fold of this handle failed (call xck_reset)"; return XCK_E_STATE; }
    if (!im->finished || !im->mol_valid) { e->err = "xck_refold: valid between a successful xck_finish and the next xck_reset"; return XCK_E_STATE; }
    if (int rc = refold_check(im, cfg)) return rc;
    HIP_TRY(hipSetDevice(im->device));
    const auto t0 = std::chrono::steady_clock::now();
    if (im->copy_pending) { HIP_TRY(hipStreamSynchronize(im->s_copy)); im->copy_pending = false; }   // the last fold's copy-out reads workspace 2
    clear_stale_error("refold", e->knobs.debug_timing);
    const std::vector<uint32_t> cell_bits = refold_cell_bits(im, cfg->cell_enabled);
    bool touched = false;
    int rc = refold_build_tables(im, cfg, &touched);
    if (rc) { if (touched || rc != XCK_E_NOMEM) im->fold_failed = true; hipStreamSynchronize(im->s_comp); return rc; }
    im->d_tally_cur = nullptr; im->d_cell_bits = nullptr; im->rf_ms_mask = 0;      // the mask is the call's: without one every cell counts again
    if (!cell_bits.empty()) {
        rc = im->key_bits == 64 ? refold_mask_tallies<uint64_t>(im, cell_bits) : refold_mask_tallies<u128>(im, cell_bits);
        if (rc) { im->fold_failed = true; hipStreamSynchronize(im->s_comp); return rc; }
        float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, im->ev_m0, im->ev_m1)); im->rf_ms_mask = ms;
    }
    im->n_regions = cfg->n_regions;
    im->sf.min_count = cfg->min_count <= 0.0 ? 0 : (int32_t)std::min(2147483647.0, std::ceil(cfg->min_count));
    im->sf.min_maf = cfg->min_maf;
    im->no_dup_hap = cfg->no_dup_hap;
    im->cmat_valid = false; im->fmat_valid = false; im->csr_host_stale = im->d_feat != nullptr;
    im->copy_timed = false;
    const auto fold = [&]() -> int {
        const size_t fmat_bytes = std::max<size_t>((size_t)im->n_regions * 6, 1) * sizeof(unsigned long long);
        if (im->d_feat) if (int r = grow_device(im, (void**)&im->d_fmat, &im->fmat_cap_bytes, fmat_bytes, refold_slack(fmat_bytes))) return r;
        Timer tm{im, im->ev0, im->ev1};
        double ms = 0;
        if (int r = tm.start()) return r;
        if (int r = im->key_bits == 64 ? fold_regions<uint64_t>(im) : fold_regions<u128>(im)) return r;
        if (int r = tm.stop(&ms)) return r;
        im->st.ms_sort += ms; im->rf_ms_regions = ms;
        HIP_TRY(hipStreamSynchronize(im->s_comp));
        return 0;
    };
    if ((rc = fold())) { im->fold_failed = true; hipStreamSynchronize(im->s_comp); hipStreamSynchronize(im->s_copy); return rc; }
    { float a = 0, b = 0; HIP_TRY(hipEventElapsedTime(&a, im->ev_r0, im->ev_r1)); HIP_TRY(hipEventElapsedTime(&b, im->ev_r2, im->ev_r3)); im->rf_ms_build = (double)a + b; }
    im->rf_ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (e->knobs.debug_timing) fprintf(stderr, "[xck] refold: total %.3f ms (host clock to the stream synchronise): table upload %.3f, builder kernels + scan %.3f, region stage %.3f, cell mask %.3f\n",
                                       im->rf_ms_total, im->rf_ms_upload, im->rf_ms_build, im->rf_ms_regions, im->rf_ms_mask);
    im->copy_pending = true;
    return result_host(im, out);
}
