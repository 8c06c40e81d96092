// read_fate.h - opt-in read assignment summary (XCK_F_READ_FATE / XCK_READ_FATE=1; xck_get_read_fate, include/xck.h).
// Included by engine.hip inside namespace xck, behind launch_join(): it uses the join's ReadInfo, TILE, fill_batch_table, cigar_summary, included_len and
// frac_below, from engine_impl.h BatchTable, JOIN_BLOCK, ReadFilter, BatchDesc, as_global, EngineImpl, dev_zeroed and HIP_TRY, and the grouped accumulation of cell_summary.h.
//
// One more pass over the batches the join has just been launched on: every read gets exactly ONE class, the first that applies in
// the order of the reference's check_read() (rdr/fc/core.py:46-62 == baf/fc/core.py:18-34) followed by the fetch overlap and the
// include test of fc_fet1 (rdr/fc/core.py:140-165) - or, for the pileup, the SNPs under the read's fetch span.  The classes are
// counted, nothing else leaves the kernel: it answers "where did the reads go" when a matrix comes out thin.
//
// A kernel of its own on purpose.  k_join<u64, pileup> sits one VGPR under its occupancy bound and both joins are bound by VALU
// issue: a reason code carried through load_read() / join_regions() would put the hot instantiations' code at
// risk for a diagnostic.  The price is a second statement of the accept rule's control flow (its two CIGAR loops are the join's own,
// cigar_summary() and included_len() over plain global loads); `pairs` below must equal the join's own count of
// accepted pairs (xck_stats.n_hits), which tests/test_gpu_read_fate.py holds on every input it has.
//
// One lane per read, CIGAR words and tables straight from global memory (no LDS staging: the pass is opt-in and small next to the
// join).  Regions: bisect the running maximum of the ends for the first candidate, as k_tile_meta does for a tile, and walk
// while start < read end.  SNPs: two bisections on the contig's sorted positions.
#pragma once

// counter words of one pipeline (uint64_t[RF_WORDS] in HBM), in the order of xck_read_fate from low_mapq on
constexpr int RF_LOW_MAPQ = 0, RF_EXCL_FLAG = 1, RF_INCL_FLAG = 2, RF_ORPHAN = 3, RF_NO_CELL = 4, RF_NO_UMI = 5, RF_SHORT = 6,
              RF_NO_TARGET = 7, RF_INCLUDE_FAIL = 8, RF_ASSIGNED = 9, RF_CLASSES = 10, RF_MULTI = 10, RF_PAIRS = 11, RF_USED = 12, RF_WORDS = 16;

struct FateArgs {
    BatchTable bt;                        // the batches of the join launch this pass follows (same tile numbering: TILE reads per block)
    ReadFilter f;
    const int32_t* reg_s0; const int32_t* reg_e0; const int32_t* reg_pmax;
    const int32_t* snp_p0;
    unsigned long long* out;              // [RF_WORDS]
};
static_assert(sizeof(FateArgs) <= 4000, "kernel arguments must stay under the 4 KiB kernarg limit");

// first index in [lo, hi) whose value is >= x (UPPER: > x)
template <bool UPPER>
__device__ __forceinline__ int32_t rf_bisect(const int32_t* v, int32_t lo, int32_t hi, int32_t x) {
    while (lo < hi) { const int32_t mid = lo + ((hi - lo) >> 1); const int32_t y = as_global(v)[mid]; if (UPPER ? y > x : y >= x) hi = mid; else lo = mid + 1; }
    return lo;
}

// What the walk keeps of a read that passed the filter, for a caller that comes back to it: fetch span, aligned bases, CIGAR words
struct RfSpan { int32_t pos, endpos, n_al; uint32_t c0, c1; bool span_is_cigar; };

// The targets of a read that passed the filter, seen through two hooks:
//   on_region(k, accepted)  basefc: region k of the start-sorted arrays fetches the read; false stops the walk
//   on_snps(k0, k1)         pileup: SNPs [k0, k1) of the sorted table lie under the read's fetch span
// k_from: first region to look at (< 0: the read's first candidate).  Returns the class; n_pairs as read_fate_walk.
template <int MODE, class OnRegion, class OnSnps>
__device__ __forceinline__ int rf_targets(const FateArgs& a, const BatchDesc& d, const RfSpan sp, const int32_t k_from, uint32_t& n_pairs, OnRegion on_region, OnSnps on_snps) {
    const int32_t pos = sp.pos, endpos = sp.endpos, n_al = sp.n_al; const uint32_t c0 = sp.c0, c1 = sp.c1; const bool span_is_cigar = sp.span_is_cigar;
    const auto word_at = [&](uint32_t c) { return as_global(d.cigar)[c]; };
    if (MODE == XCK_MODE_BASEFC) {
        ReadInfo r = {}; r.pos = pos; r.endpos = endpos; r.n_al = n_al; r.c0 = c0; r.c1 = c1; r.span_is_cigar = span_is_cigar;   // (what included_len() and frac_below() read)
        uint32_t n_ov = 0;
        // every region before the first one whose running-maximum end lies beyond pos ends at or before pos
        for (int32_t k = k_from < 0 ? rf_bisect<true>(a.reg_pmax, d.reg_lo, d.reg_hi, pos) : k_from; k < d.reg_hi; k++) {
            const int32_t s0 = as_global(a.reg_s0)[k];
            if (s0 >= endpos) break;                                  // sorted by start
            const int32_t e0 = as_global(a.reg_e0)[k];
            if (!(pos < e0)) continue;                                // htslib fetch overlap: pos < end0 && endpos > start0
            n_ov++;
            const int32_t m = included_len(word_at, r, s0, e0);
            if (a.f.frac_mode) {                                      // rdr/fc/core.py:160-165, exactly as join_regions()
                if (n_al <= 0) { if (on_region(k, false)) continue; break; }
                if (m != n_al && frac_below(m, r, a.f.min_inc_frac)) { if (on_region(k, false)) continue; break; }
            } else if (m < a.f.min_inc_len) { if (on_region(k, false)) continue; break; }
            n_pairs++;
            if (!on_region(k, true)) break;
        }
        return n_pairs ? RF_ASSIGNED : n_ov ? RF_INCLUDE_FAIL : RF_NO_TARGET;
    } else {
        // SNPs of the contig with pos <= p0 < endpos (whether a SNP lies in a region is not asked: the join does not ask either)
        const int32_t snp_lo = d.n_swin > 0 ? as_global(d.snp_win)[0] : d.snp_end;   // window 0 starts at the contig's first SNP
        const int32_t k0 = rf_bisect<false>(a.snp_p0, snp_lo, d.snp_end, pos);
        const int32_t k1 = rf_bisect<false>(a.snp_p0, k0, d.snp_end, endpos);
        n_pairs = (uint32_t)(k1 - k0);
        on_snps(k0, k1);
        return n_pairs ? RF_ASSIGNED : RF_NO_TARGET;
    }
}

// The read filter alone, the one statement of it outside the join: the class that turns read i of batch d away, or -1 when it passes -
// then sp holds its fetch span, aligned bases and CIGAR words.  read_fate_walk asks the targets next; the base tally (base_tally.h),
// which asks about neither regions nor SNPs, stops here.
__device__ __forceinline__ int rf_filter(const ReadFilter& f, const BatchDesc& d, const int32_t i, RfSpan& sp) {
    const uint32_t flag = as_global(d.flag)[i];
    const int32_t mapq = as_global(d.mapq)[i];
    if (mapq < f.min_mapq) return RF_LOW_MAPQ;
    if (f.excl_flag && (flag & f.excl_flag)) return RF_EXCL_FLAG;
    if (f.incl_flag && !(flag & f.incl_flag)) return RF_INCL_FLAG;
    if (f.no_orphan && (flag & BAM_FPAIRED) && !(flag & BAM_FPROPER_PAIR)) return RF_ORPHAN;
    if (as_global(d.cell)[i] < 0) return RF_NO_CELL;
    if (as_global(d.umi)[i] == XCK_UMI_NONE) return RF_NO_UMI;
    const uint32_t c0 = as_global(d.cig_off)[i], c1 = as_global(d.cig_off)[i + 1];
    const auto word_at = [&](uint32_t c) { return as_global(d.cigar)[c]; };
    int32_t rlen = 0, n_al = 0;
    cigar_summary(word_at, c0, c1, rlen, n_al);
    if (n_al < f.min_len) return RF_SHORT;
    // the fetch span, as load_read(): htslib bam_endpos() gives an unmapped-flagged read, or one without reference-consuming
    // CIGAR, one base
    const bool span_is_cigar = !((flag & BAM_FUNMAP) || c1 == c0 || rlen == 0);
    if (!span_is_cigar) rlen = 1;
    const int32_t pos = as_global(d.pos)[i], endpos = pos + rlen;
    sp.pos = pos; sp.endpos = endpos; sp.n_al = n_al; sp.c0 = c0; sp.c1 = c1; sp.span_is_cigar = span_is_cigar;
    return -1;
}

// Class of read i of batch d; n_pairs = regions that accept it / SNPs it covers (0 unless the class is RF_ASSIGNED).  The read filter
// (rf_filter) in front of the one statement of the accept rule (rf_targets): every pass that follows the join and asks about targets
// (k_read_fate*, k_feature_fate of feature_summary.h) goes through here.  sp: filled when the read passes the filter.
template <int MODE, class OnRegion, class OnSnps>
__device__ __forceinline__ int read_fate_walk(const FateArgs& a, const BatchDesc& d, const int32_t i, uint32_t& n_pairs, RfSpan& sp, OnRegion on_region, OnSnps on_snps) {
    n_pairs = 0;
    const int cls = rf_filter(a.f, d, i, sp);
    if (cls >= 0) return cls;
    return rf_targets<MODE>(a, d, sp, -1, n_pairs, on_region, on_snps);
}
// ... for a pass that only counts: no hooks
template <int MODE>
__device__ __forceinline__ int read_fate_of(const FateArgs& a, const BatchDesc& d, const int32_t i, uint32_t& n_pairs) {
    RfSpan sp;
    return read_fate_walk<MODE>(a, d, i, n_pairs, sp, [](int32_t, bool) { return true; }, [](int32_t, int32_t) {});
}

// Block t covers the TILE reads of join tile t.  Per class a wave ballot + popcount (wave-uniform counts), the sums by a wave
// reduction; the waves add into a small LDS array and the block sends one 64-bit atomicAdd per non-zero counter to HBM.
// PER_CELL (XCK_F_CELL_SUMMARY): the same classification also feeds the per-cell table, grouped by the read's row - its cell, or
// the table's last row when it has none (cell_summary.h); without it nothing of that is in the code.
template <int MODE, bool PER_CELL>
__device__ __forceinline__ void read_fate_block(const FateArgs a, const CellArgs ca) {
    __shared__ unsigned long long s_cnt[RF_WORDS];
    CellLds* const s_cell = cs_lds<PER_CELL>();
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < RF_WORDS) s_cnt[tid] = 0ull;
    if (PER_CELL) cs_init(*s_cell, ca, tid);
    __syncthreads();
    const int t = blockIdx.x;
    int lo = 0, hi = a.bt.n_batches - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.bt.desc[mid].tile0 <= t) lo = mid; else hi = mid - 1; }
    const BatchDesc& d = a.bt.desc[lo];
    const int32_t r0 = (t - d.tile0) * TILE;
    uint32_t cnt[RF_CLASSES];
#pragma unroll
    for (int c = 0; c < RF_CLASSES; c++) cnt[c] = 0;
    unsigned long long pairs = 0; uint32_t multi = 0;
#pragma unroll 1
    for (int j = 0; j < TILE_ITEMS; j++) {
        const int32_t i = r0 + j * JOIN_BLOCK + tid;
        int cls = -1; uint32_t np = 0;
        if (i < d.n) cls = read_fate_of<MODE>(a, d, i, np);
#pragma unroll
        for (int c = 0; c < RF_CLASSES; c++) cnt[c] += (uint32_t)__popcll(__ballot(cls == c));
        pairs += np; multi += np >= 2u ? 1u : 0u;
        if (PER_CELL) {
            // (a cell index outside the table - a device-resident batch is the caller's word - counts in the last row, never beyond it)
            int32_t row = ca.n_rows - 1;
            if (cls >= 0) { const int32_t cell = as_global(d.cell)[i]; if ((uint32_t)cell < (uint32_t)(ca.n_rows - 1)) row = cell; }
            cs_add(*s_cell, ca, lane, cls >= 0, row, cls, np, np >= 2u, RF_MULTI);   // (np != 0 only for RF_ASSIGNED)
        }
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) { pairs += __shfl_xor(pairs, dd, 64); multi += __shfl_xor(multi, dd, 64); }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < RF_CLASSES; c++) if (cnt[c]) atomicAdd(&s_cnt[c], (unsigned long long)cnt[c]);
        if (multi) atomicAdd(&s_cnt[RF_MULTI], (unsigned long long)multi);
        if (pairs) atomicAdd(&s_cnt[RF_PAIRS], pairs);
    }
    __syncthreads();
    if (tid < RF_USED) { const unsigned long long v = s_cnt[tid]; if (v) atomicAdd(&a.out[tid], v); }
    if (PER_CELL) cs_flush(*s_cell, ca, tid);
}
template <int MODE>
__global__ __launch_bounds__(JOIN_BLOCK) void k_read_fate(FateArgs a) { read_fate_block<MODE, false>(a, CellArgs{}); }
template <int MODE>
__global__ __launch_bounds__(JOIN_BLOCK) void k_read_fate_cell(FateArgs a, CellArgs ca) { read_fate_block<MODE, true>(a, ca); }
static_assert(sizeof(FateArgs) + sizeof(CellArgs) <= 4000, "kernel arguments must stay under the 4 KiB kernarg limit");
static_assert(RF_WORDS == CS_ROW_WORDS && RF_USED == CS_COLS && RF_MULTI < CS_C32 && RF_PAIRS == CS_C32, "the per-cell table keeps the columns of the global words");

// The arguments every pass behind the join shares (launch_read_fate, launch_feature_fate of feature_summary.h): the batches in
// im->inflight with the join's tile numbering, the filter, the tables.  -> tiles = blocks of the launch; a.out is the caller's.
static int32_t fill_fate_args(const EngineImpl* im, FateArgs& a) {
    const int32_t tiles = fill_batch_table(im, a.bt);
    a.f = im->rf;
    a.reg_s0 = im->d_reg_s0; a.reg_e0 = im->d_reg_e0; a.reg_pmax = im->d_reg_pmax; a.snp_p0 = im->d_snp_p0;
    a.out = nullptr;
    return tiles;
}

// the counters' own memory (summaries_init), and their zeroing on s_comp (summaries_reset); both only with the flag on
static int read_fate_init(EngineImpl* im) { return dev_zeroed(im, (void**)&im->d_fate, RF_WORDS * sizeof(unsigned long long)); }
static int read_fate_reset(EngineImpl* im) {
    HIP_TRY(hipMemsetAsync(im->d_fate, 0, RF_WORDS * sizeof(unsigned long long), im->s_comp));
    return 0;
}

// Runs once per batch: called by launch_queue() (launch_summaries) behind the FIRST join launch of the batches in im->inflight, on the
// same stream - so it is over before complete_pending() hands their staging slot back - and never by the overflow replay.
static int launch_read_fate(EngineImpl* im) {
    if (!im->d_fate || im->inflight.empty()) return 0;
    FateArgs a;
    const int32_t tiles = fill_fate_args(im, a);
    a.out = im->d_fate;
    if (im->d_cell) {                                          // (XCK_F_CELL_SUMMARY: the instantiation that also fills the per-cell table)
        CellArgs ca;
        ca.tab = im->d_cell; ca.n_rows = im->n_cells + 1; ca.slot_mask = cs_slot_mask(im); ca.stride = CS_ROW_WORDS; ca.c32_base = 0; ca.wide_col = RF_PAIRS;
        if (im->mode == XCK_MODE_BASEFC) hipLaunchKernelGGL((k_read_fate_cell<XCK_MODE_BASEFC>), dim3(tiles), dim3(JOIN_BLOCK), 0, im->s_comp, a, ca);
        else hipLaunchKernelGGL((k_read_fate_cell<XCK_MODE_BAF>), dim3(tiles), dim3(JOIN_BLOCK), 0, im->s_comp, a, ca);
    } else if (im->mode == XCK_MODE_BASEFC) hipLaunchKernelGGL((k_read_fate<XCK_MODE_BASEFC>), dim3(tiles), dim3(JOIN_BLOCK), 0, im->s_comp, a);
    else hipLaunchKernelGGL((k_read_fate<XCK_MODE_BAF>), dim3(tiles), dim3(JOIN_BLOCK), 0, im->s_comp, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// xck_get_read_fate() for one pipeline: waits for the queued work, copies the counters
int engine_read_fate(EngineImpl* im, xck_read_fate* out) {
    if (!im->d_fate) { im->eng->err = "handle made without XCK_F_READ_FATE"; return XCK_E_STATE; }
    int rc = engine_flush(im); if (rc) return rc;
    unsigned long long h[RF_WORDS];
    HIP_TRY(hipMemcpy(h, im->d_fate, sizeof h, hipMemcpyDeviceToHost));
    out->mode = im->mode;
    out->n_reads = im->st.n_reads; out->not_joined = im->n_not_joined;
    int64_t* f[RF_USED] = { &out->low_mapq, &out->excl_flag, &out->incl_flag, &out->orphan, &out->no_cell, &out->no_umi, &out->short_aligned,
                            &out->no_target, &out->include_fail, &out->assigned, &out->multi, &out->pairs };
    for (int k = 0; k < RF_USED; k++) *f[k] = (int64_t)h[k];
    return 0;
}
