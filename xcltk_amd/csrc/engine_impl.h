// engine_impl.h - what the three translation units of the engine share: engine.hip (tables, join kernels, summary passes),
// pipeline.hip (buffers, launch queue, push paths, lifecycle; host code only) and finish.hip (fold kernels, finish driver).  Types,
// control-word layout, the per-GPU state (EngineImpl), the tuning macros more than one unit reads, and the host helpers one unit
// defines for the others.  Of the join the pipeline sees the batch table it queues for and the handful of functions declared at the
// end - its tile size, capacities and kernels stay private to engine.hip.
#pragma once
#include <algorithm>
#include <cstdint>
#include <climits>
#include <cstdio>
#include <vector>
#include <hip/hip_runtime.h>
#include "xck_internal.h"
#include "fold_ws.h"                     // Arena, and the fold workspaces cut from it

namespace xck {
typedef unsigned __int128 u128;
constexpr int JOIN_BLOCK = 256;

// hipGetLastError() after a launch also returns (and clears) an error that some EARLIER, unchecked runtime call of this thread
// left behind; the launch sites clear it first, and XCK_DEBUG_TIMING reports what was there.
static inline void clear_stale_error(const char* where, bool report = false) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess && report) fprintf(stderr, "[xck] %s: cleared a stale HIP error left by an earlier call: %s [%d]\n", where, hipGetErrorString(e), (int)e);
}
#define HIP_TRY(expr)                                                                      \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) {                                   \
        char b_[512]; snprintf(b_, sizeof b_, "%s failed: %s [%d] (%s:%d)", #expr,         \
                               hipGetErrorString(e_), (int)e_, __FILE__, __LINE__);        \
        im->eng->err = b_; return XCK_E_DEVICE; } } while (0)

template <class K> struct KeyLayout {
    int ubits, cbits;
    __host__ __device__ K make(uint32_t row, uint32_t cell, uint64_t umi) const {
        return (K(row) << (cbits + ubits)) | (K(cell) << ubits) | K(umi);
    }
    __host__ __device__ K rc(K k) const { return k >> ubits; }
    __host__ __device__ uint32_t row(K k) const { return uint32_t(k >> (cbits + ubits)); }
    __host__ __device__ uint32_t cell(K k) const { return uint32_t((k >> ubits) & ((K(1) << cbits) - 1)); }
    __host__ __device__ uint64_t umi(K k) const { return ubits >= 64 ? uint64_t(k) : uint64_t(k & ((K(1) << ubits) - 1)); }
};

struct ReadFilter {                      // check_read(), rdr/fc/core.py:46-62
    int32_t min_mapq, min_len;
    uint32_t incl_flag, excl_flag;
    int32_t no_orphan;
    int32_t frac_mode;                   // rdr/fc/core.py:160-165
    double  min_inc_frac;
    int32_t min_inc_len;
};

struct SnpFilter { int32_t min_count; double min_maf; };

#define XCK_GLOBAL __attribute__((address_space(1)))
template <class T> __device__ __forceinline__ const XCK_GLOBAL T* as_global(const T* p) { return (const XCK_GLOBAL T*)p; }

// One queued record batch (device pointers) inside a fused launch.
struct BatchDesc {
    int32_t n, tile0;                       // reads, first tile of this batch in the fused grid
    const int32_t* pos; const uint16_t* flag; const uint8_t* mapq; const int32_t* cell;
    const uint64_t* umi; const uint32_t* cig_off; const uint32_t* cigar;
    const uint32_t* seq_off; const uint8_t* seq;
    uint64_t ordinal_base;
    int32_t reg_lo, reg_hi;                                 // regions of the batch's contig: [reg_lo, reg_hi) of the start-sorted arrays
    const int32_t* snp_win; int32_t n_swin; int32_t snp_end; // SNP window table of the batch's contig
    const uint8_t* qual;                                    // pileup with a base-quality floor: quality of query offset qi of the read at seq offset s0 = qual[2 * s0 + qi] (else null)
    int32_t contig, pad_;                                   // the batch's contig (the base tally finds its table by it; the join does not read it)
};

constexpr int MAX_FUSE = 24;              // batches per fused launch (the table travels in the kernel arguments)

// Batch table, passed BY VALUE: it lives in the kernarg segment and is read with scalar loads
// through the constant cache instead of costing a dependent round trip to HBM per tile.
struct BatchTable { int32_t n_batches; int32_t n_tiles; BatchDesc desc[MAX_FUSE]; };

// Per-tile facts computed once by k_tile_meta (one thread per tile, all tiles in parallel) so that
// the join kernel's prologue is ONE load of this record plus ONE round of independent staging loads.
struct TileMeta {
    uint32_t c_lo, cg_n;                  // CIGAR words of the tile: [c_lo, c_lo + cg_n) are staged
    int32_t  w0, nw, e0, n_ent;           // basefc: staged regions [e0, e0 + n_ent) of the start-sorted arrays; pileup: staged SNP windows [w0, w0 + nw)
    int32_t  k0, nk;                      // pileup: staged SNPs [k0, k0+nk); basefc: k0 = position of the tile's first read
    int32_t  b, r0, r1, pad;              // batch index, first / one-past-last read of the tile
};

// The append cursor is sharded: a returning atomicAdd on one word tops out near 88 ops/us on gfx950
// (one L2 channel), which bounded the first two versions of this kernel.  Tiles use shard
// blockIdx % NSHARD; every shard owns its own cursor word (128 B apart -> different channels) and
// its own slice [shard*cap, (shard+1)*cap) of the hit buffer; finish() packs the slices.
constexpr int NSHARD = 16;
constexpr int CTL_OVERFLOW = 1, CTL_GIANT = 2, CTL_SCRATCH = 3, CTL_SHARD0 = 16, CTL_STRIDE = 16;
constexpr int XSHARD = NSHARD;            // k_expand: sharded totals / cursors (one shared word serialises at ~90 atomics/us); = NSHARD: its output slices feed the partition sort
constexpr int CTL_X0 = CTL_SHARD0 + 2 * NSHARD * CTL_STRIDE;
constexpr int CTL_WORDS = CTL_X0 + XSHARD * CTL_STRIDE;
struct XBases { unsigned long long base[XSHARD]; };
struct ShardSpan { unsigned long long start[NSHARD + 1]; };               // first packed index of every shard slice
__host__ __device__ inline int ctl_cursor(int shard) { return CTL_SHARD0 + shard * CTL_STRIDE; }
__host__ __device__ inline int ctl_umi_or(int shard) { return CTL_SHARD0 + shard * CTL_STRIDE + 1; }   // OR of the UMI codes seen
__host__ __device__ inline int ctl_ncursor(int shard) { return CTL_SHARD0 + shard * CTL_STRIDE + 2; }  // cursor of the no-base stream
__host__ __device__ inline int ctl_accepted(int shard) { return CTL_SHARD0 + (NSHARD + shard) * CTL_STRIDE; }
__host__ __device__ inline int ctl_bq_base(int shard) { return ctl_accepted(shard) + 1; }     // min_baseq: (read, SNP) pairs with a stored base
__host__ __device__ inline int ctl_bq_masked(int shard) { return ctl_accepted(shard) + 2; }   // ... and those of them the floor masked

// tuning macros that both translation units read (a variant build passes its -D flags to both)
#ifndef XCK_BAF_SPLIT
#define XCK_BAF_SPLIT 1           // pileup, 64-bit keys: hits without a base go to a second stream that is never sorted
#endif

// slot of a 64-bit key: full-rate VALU only (a 64-bit multiply is four quarter-rate v_mul ops on CDNA)
template <int SLOTS>
__device__ __forceinline__ uint32_t set_slot(unsigned long long kk) {
    const uint32_t lo = (uint32_t)kk, hi = (uint32_t)(kk >> 32);
    uint32_t x = lo ^ ((hi << 9) | (hi >> 23));
    x ^= x >> 15;
    // (written as asm: only bits 12.. of the product are used, so the compiler narrows __umul24 to a plain 32-bit multiply -
    // v_mul_lo_u32, a quarter-rate instruction on gfx9 - where the 24-bit form issues at full rate)
    uint32_t p;
    asm("v_mul_u32_u24 %0, %1, %2" : "=v"(p) : "v"(x), "v"(0x9E3779u));
    return (p >> 12) & (SLOTS - 1);
}

struct ContigTab { int32_t reg_base = 0, n_reg = 0, snp_base = 0, n_snp = 0, swin_base = 0, n_swin = 0; };

struct BatchSlot {
    int32_t* pos = nullptr; uint16_t* flag = nullptr; uint8_t* mapq = nullptr; int32_t* cell = nullptr;
    uint64_t* umi = nullptr; uint32_t* cig_off = nullptr; uint32_t* cigar = nullptr; uint32_t* seq_off = nullptr; uint8_t* seq = nullptr;
    uint8_t* qual = nullptr; size_t cap_qual = 0;            // min_baseq handles only: two bytes per sequence byte
    size_t cap_reads = 0, cap_cig = 0, cap_seq = 0;          // reads (the seven per-read columns); bytes; bytes
    bool busy = false;
};

// State of one derived-matrix call (xck_snp_counts, xck_group_counts; the host steps that work on it are in coo_call.h).  Buffers of
// the call's own, grow-only, freed at destroy (coo_call_free): nothing of it comes from the workspaces or the shard slices.
struct CooCall {
    char* d_scratch = nullptr; size_t scratch_cap = 0;                   // one block, laid out anew by every call (ScratchLayout)
    int32_t* d_res = nullptr; size_t d_res_cap = 0;                      // the call's COO blocks [row | col | val], back to back, on the device
    int32_t* h_res = nullptr; size_t h_res_cap = 0;                      // ... and in pinned host memory (capacities in bytes)
    unsigned long long *h_tot = nullptr, *d_tot_alias = nullptr;         // the totals and a flag word: pinned + mapped words and their device alias
    size_t nnz[3] = {0, 0, 0};                                           // entries of the blocks of the last call
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};    // first phase [0, 1], second [1, 2], emit [3, 4]
    double ms_total = 0, ms_copy = 0; float ms_phase[3] = {0, 0, 0};     // the last call (host clock; HIP events), for XCK_DEBUG_TIMING and tools/*_counts_time.py
};
static inline void coo_call_free(CooCall& c) {
    for (void* p : { (void*)c.d_scratch, (void*)c.d_res }) if (p) hipFree(p);
    for (void* p : { (void*)c.h_res, (void*)c.h_tot }) if (p) hipHostFree(p);
    for (hipEvent_t ev : c.ev) if (ev) hipEventDestroy(ev);
}

struct EngineImpl {
    xck_engine* eng = nullptr;
    int mode = 0, device = 0;
    int key_bits = 64, ubits = 0, cbits = 0, rbits = 0;
    ReadFilter rf{};
    SnpFilter sf{};
    int no_dup_hap = 1;
    int n_cells = 0, n_regions = 0, n_snps_sorted = 0;
    std::vector<ContigTab> ctab;
    // device tables
    int32_t *d_reg_s0 = nullptr, *d_reg_e0 = nullptr, *d_reg_row = nullptr, *d_reg_pmax = nullptr;   // basefc: regions per contig sorted by start
    int32_t *d_snp_p0 = nullptr, *d_snp_win = nullptr, *d_csr_off = nullptr, *d_csr_reg = nullptr;
    uint32_t *d_snp_info = nullptr, *d_tally = nullptr;
    hipStream_t s_copy = nullptr, s_comp = nullptr;
    BatchSlot slot[2];
    int next_slot = 0;
    int64_t max_batch_reads = 0;
    // hit accumulators (ping-pong pair so that sort results can stay where they land)
    void* d_keys = nullptr; uint64_t* d_vals = nullptr; size_t hit_cap = 0;
    void* d_nkeys = nullptr; uint64_t* d_nvals = nullptr;   // pileup split mode: hits without a base (same per-shard capacity)
    unsigned long long ncur[NSHARD] = {0}, ncur_before[NSHARD] = {0}, ncursor = 0;
    unsigned long long* d_ctl = nullptr;       // CTL_WORDS control words (overflow flag, scratch, sharded cursors)
    unsigned long long* h_ctl = nullptr;       // pinned + mapped mirror
    unsigned long long* d_hctl = nullptr;      // device alias of h_ctl (written by k_publish)
    unsigned long long cur[NSHARD] = {0};      // host view of the shard cursors after the last completed launch
    unsigned long long cur_before[NSHARD] = {0}, acc_before[NSHARD] = {0};
    int min_baseq = 0;                         // pileup: base-quality floor of the join (xck_config.min_baseq / XCK_MIN_BASEQ; 0 = off: the default kernels, no quality column)
    unsigned long long bqb_before[NSHARD] = {0}, bqm_before[NSHARD] = {0};   // its pair counters before the launch in flight (rewound with acc_before on a replay)
    unsigned long long cursor = 0;             // sum of cur[]; hit_cap is the capacity of ONE shard
    int fold_extra_digits = 0;                 // basefc hash fold: extra radix digits that earlier finishes needed (giant runs)
    int fold_path = 0, fold_fallbacks = 0;     // xck_stats: which basefc fold ran last (1 partition, 2 radix sort), hand-overs so far
    int pileup_sort_path = 0;                  // pileup hits of the last finish: 1 sorted by partition + LDS sort, 2 by the radix sort
    int pileup_sort2_path = 0;                 // ... and its region-level hits
    int fold_refinements = 0;                  // partition fold of the last finish: refinements of the level-2 geometry
    // fused launch queue
    std::vector<BatchDesc> queue;              // not yet launched (device-resident pushes are deferred)
    std::vector<BatchDesc> inflight;           // launched, not yet confirmed (kept for overflow replay)
    int inflight_slot = -1;
    int inflight_shared = -1;                  // staging slot (Stager) the launch in flight reads, -1 = none
    int64_t queued_reads = 0, inflight_reads = 0;
    TileMeta* d_meta = nullptr; size_t meta_cap = 0;        // (bytes)
    // timing
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_res = nullptr, ev_c0 = nullptr, ev_c1 = nullptr;
    hipEvent_t ev_f1 = nullptr, ev_f2 = nullptr;   // partition fold: level-1 bucket pass on the copy stream (fold_partition.h)
    bool copy_timed = false, copy_pending = false;
    xck_stats st{};
    int64_t n_join_launches = 0;
    bool fold_failed = false;             // xck_finish returned an error from inside a fold: only xck_reset makes the handle usable again
    unsigned long long stamp_sum[12] = {0}; int stamp_tiles = 0; float stamp_ms = 0;   // XCK_STAMPS builds: phase cycles of the last join launch
    // workspace + results
    Arena ws1, ws2;
    int32_t* h_res[4] = {nullptr, nullptr, nullptr, nullptr}; size_t h_res_cap[4] = {0, 0, 0, 0} /* bytes */; size_t res_nnz[4] = {0, 0, 0, 0};
    int32_t* d_res[4] = {nullptr, nullptr, nullptr, nullptr};   // device copies [row | col | val] inside the workspace, valid until the next finish / reset
    bool finished = false;
    // read assignment summary (XCK_F_READ_FATE, read_fate.h): device counters (null = off), reads of the batches no kernel saw
    unsigned long long* d_fate = nullptr;
    int64_t n_not_joined = 0;
    // per-cell table (XCK_F_CELL_SUMMARY, cell_summary.h): [(n_cells + 1) * 16] words in HBM (null = off), the column marginals of the
    // last finish, and the host copies xck_get_cell_summary hands out
    unsigned long long* d_cell = nullptr; unsigned long long* d_cmat = nullptr;
    std::vector<int64_t> h_cell_raw, h_cell, h_cmat;
    bool cmat_valid = false;
    // per-feature / per-SNP tables (XCK_F_FEATURE_SUMMARY, feature_summary.h): the read half in HBM (null = off; basefc [n_regions * 4]
    // words by the caller's region index, pileup one word per SNP of the sorted table), the row marginals of the last finish, the
    // verdicts of snp_passes(), and the host copies xck_get_feature_summary hands out.  snp_perm: sorted SNP -> the caller's index;
    // h_csr_off / h_csr_reg: the SNP -> region relation as uploaded (these three are kept only with the flag)
    unsigned long long* d_feat = nullptr; unsigned long long* d_fmat = nullptr; uint32_t* d_kept = nullptr;
    std::vector<int64_t> h_feat_raw, h_feat, h_fmat;
    std::vector<uint32_t> h_tally, h_kept;
    std::vector<int32_t> snp_perm, h_csr_off, h_csr_reg;
    int n_snps_in = 0;
    bool fmat_valid = false;
    // what the molecule stage of the pileup fold leaves for the region stage (finish.hip fold_molecules / fold_regions): the hits sorted
    // by key - in workspace 1 after the partition sort, in d_keys after the radix sort - and the base the first read of every key
    // shows (workspace 1).  Valid from a successful finish to the next reset; nothing in the region stage takes memory in either place.
    const void* mol_keys = nullptr; uint8_t* mol_al = nullptr; size_t mol_n = 0; bool mol_valid = false;
    // UMI consensus (XCK_F_UMI_CONSENSUS, umi_consensus.h): the five agreement counters in HBM, MOL_SLOTS copies that the getter sums (null = off: the molecule stage keeps the
    // first read's base), filled by the molecule stage of xck_finish and valid from a successful finish to the next reset
    unsigned long long* d_mol = nullptr; bool mol_stats_valid = false;
    // unique-feature molecules (XCK_F_UNIQUE_FEATURE, umi_feature.h; null = off: the fold counts every key): row -> rank in the join
    // table's (contig, start, end, index) order; per rank the first and one-past-last rank of its contig; the four counters of the last
    // xck_finish, valid from a successful finish to the next reset
    uint32_t* d_uf_rank = nullptr; uint2* d_uf_span = nullptr;
    long long uf_stats[4] = {0, 0, 0, 0}; bool uf_stats_valid = false;
    // 1-mismatch UMI collapsing (XCK_F_UMI_COLLAPSE, umi_collapse.h; false = off: the fold counts every key): the six counters of the last
    // xck_finish, valid from a successful finish to the next reset
    bool umi_collapse = false; long long uc_stats[6] = {0, 0, 0, 0, 0, 0}; bool uc_stats_valid = false;
    // base tallies (XCK_F_BASE_TALLY, base_tally.h; false = off): the contigs' lengths (empty until xck_set_contig_lengths), per contig its
    // table [len * 4] in HBM (null until the contig's first batch is queued), the pass's counters in BT_SLOTS copies, and what
    // xck_find_candidates needs: per-block counts, the scan's two totals, one contig's output on the device, the host arrays it hands out
    bool base_tally = false;
    std::vector<int64_t> bt_len; std::vector<uint32_t*> bt_tab;
    unsigned long long* d_bt_stats = nullptr; unsigned long long* d_bt_tot = nullptr;
    char* d_bt_blk = nullptr; size_t bt_blk_cap = 0; char* d_bt_out = nullptr; size_t bt_out_cap = 0;
    std::vector<int32_t> h_bt_contig, h_bt_pos; std::vector<char> h_bt_ref, h_bt_alt; std::vector<uint32_t> h_bt_cnt;
    // the genome's sequence of a tally handle (ref_seq.h): per contig its (bt_len + 7) / 8 dwords of 4-bit codes in HBM (null: no sequence),
    // the two pinned and the two device staging chunks of xck_set_contig_ref with the events behind their kernels, the stale-index counter
    std::vector<uint32_t*> rs_tab;
    void* h_rs_stage[2] = {nullptr, nullptr}; size_t rs_hcap[2] = {0, 0}; void* d_rs_stage[2] = {nullptr, nullptr}; size_t rs_dcap[2] = {0, 0};
    hipEvent_t rs_ev[2] = {nullptr, nullptr}; unsigned long long* d_rs_bad = nullptr;
    int batch_rc = 0;                                     // describe_batch: the code of the error it reported (XCK_E_ARG unless a table could not be had)
    // xck_refold (refold.h): the caller's SNP list as given to xck_create, the regrown tables' capacities, and the builder's own buffers
    std::vector<xck_snp> snps_in;
    size_t csr_reg_cap_bytes = 0, fmat_cap_bytes = 0;     // of d_csr_reg and d_fmat, which a refold may have to regrow
    bool csr_host_stale = false;                          // h_csr_off / h_csr_reg lag behind the device tables (feature_summary.h reloads them)
    int32_t* d_csr_alt = nullptr;                         // the next d_csr_off: counted and scanned here, swapped in once the total is known
    char* d_rf = nullptr; size_t rf_cap = 0;              // sorted regions, exclusion words, SNP mask, contig table, scan block sums
    hipEvent_t ev_r0 = nullptr, ev_r1 = nullptr, ev_r2 = nullptr, ev_r3 = nullptr;   // count pass + scan, fill pass
    double rf_ms_upload = 0, rf_ms_build = 0, rf_ms_regions = 0, rf_ms_total = 0;   // the last refold, for XCK_DEBUG_TIMING and tools/refold_time.py
    // xck_refold with a cell mask (refold.h refold_mask_tallies): one grow-only block holding the mask as a bit table (one bit per cell), the
    // first index of every SNP in the sorted hits, the list of the deep SNPs' pieces and the tallies of the enabled cells.  d_tally_cur /
    // d_cell_bits: the tallies and the bit table the last fold counted with - null = d_tally and all cells (every finish, every unmasked refold)
    char* d_cm = nullptr; size_t cm_cap = 0;
    uint32_t* d_tally_cur = nullptr; const uint32_t* d_cell_bits = nullptr;
    hipEvent_t ev_m0 = nullptr, ev_m1 = nullptr;
    double rf_ms_mask = 0;                                // the last refold: bit table upload, SNP bounds and masked tallies (0 without a mask)
    // xck_snp_counts (snp_counts.h): a CooCall holding the three blocks [ad | dp | oth] (valid until the next xck_snp_counts / reset),
    // and the sorted SNP -> caller index table on the device
    CooCall sc;
    int32_t* d_sc_perm = nullptr;
    bool sc_valid = false;
    // xck_group_counts (group_counts.h): a CooCall holding the blocks of this pipeline's matrices (valid until the next xck_group_counts / reset)
    CooCall gc;
};

// the per-SNP tallies the verdicts are decided on: the handle's own, or those of the last masked xck_refold
static inline const uint32_t* cur_tally(const EngineImpl* im) { return im->d_tally_cur ? im->d_tally_cur : im->d_tally; }

// d_snp_info: ref nibble | alt nibble << 4 | ref_hap << 8 | alt_hap << 9
static inline uint32_t nib_of(uint8_t ch) {
    switch (ch) { case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8; default: return 15; }
}
static inline uint32_t snp_info_word(const xck_snp& x) { return nib_of(x.ref) | (nib_of(x.alt) << 4) | ((uint32_t)(x.ref_hap & 1) << 8) | ((uint32_t)(x.alt_hap & 1) << 9); }

// Regions per contig sorted by (start, end, index), with the running maximum of the ends (the first candidate of a position is one
// bisection over it).  keep(region) says which regions enter the table; base[c] / count[c] are the contig's slice.  s0 holds what
// start0(region) returns: the basefc join stores 0-based starts, the SNP -> region builder 1-based ones.
template <class Keep, class Start>
static inline void sort_regions_by_contig(const xck_region* regions, int n_regions, int nc, Keep keep, Start start0, std::vector<int32_t>& s0, std::vector<int32_t>& e0,
                                          std::vector<int32_t>& row, std::vector<int32_t>& pmax, std::vector<int32_t>& base, std::vector<int32_t>& count) {
    std::vector<std::vector<int32_t>> by_c(nc);
    for (int g = 0; g < n_regions; g++) {
        const xck_region& r = regions[g];
        if (r.contig < 0 || r.contig >= nc || !keep(r)) continue;
        by_c[r.contig].push_back(g);
    }
    base.assign(std::max(nc, 1), 0); count.assign(std::max(nc, 1), 0);
    for (int c = 0; c < nc; c++) {
        auto& v = by_c[c];
        std::sort(v.begin(), v.end(), [&](int32_t a, int32_t b) {
            const xck_region &x = regions[a], &y = regions[b];
            if (x.start != y.start) return x.start < y.start;
            if (x.end != y.end) return x.end < y.end;
            return a < b; });
        base[c] = (int32_t)s0.size(); count[c] = (int32_t)v.size();
        int32_t max_e = INT32_MIN;
        for (int32_t g : v) {
            const xck_region& r = regions[g];
            s0.push_back(start0(r)); e0.push_back(r.end); row.push_back(g);
            max_e = std::max(max_e, r.end); pmax.push_back(max_e);          // running maximum of the ends: first candidate of a position by binary search
        }
    }
}

// host helpers defined in pipeline.hip
size_t key_bytes(const EngineImpl* im);
size_t hit_slack(const EngineImpl* im);
bool split_mode(const EngineImpl* im);
int arena_begin(EngineImpl* im, Arena& a, size_t need);
int grow_device(EngineImpl* im, void** p, size_t* cap, size_t need, size_t slack);   // grow-only buffers (capacities in bytes); contents are not kept
int grow_pinned(EngineImpl* im, void** p, size_t* cap, size_t need, size_t slack);
int dev_zeroed(EngineImpl* im, void** p, size_t bytes);    // a device buffer of its own, all zero
int res_reserve(EngineImpl* im, int m, size_t nnz);
int complete_pending(EngineImpl* im);
int launch_queue(EngineImpl* im, int slot_idx, int shared_slot = -1);
// defined in engine.hip: all the pipeline sees of the join and of the summaries behind it
int build_tables(EngineImpl* im, const xck_config* cfg);   // engine_create: the region / SNP tables the join reads, uploaded
int launch_join(EngineImpl* im);                           // ONE fused join launch over im->inflight, then the control words to the host
int join_stamps_collect(EngineImpl* im, float ms);         // XCK_STAMPS builds: sums the stamp records of the launch just waited for
void join_stamps_report(const EngineImpl* im);             // ... and prints the phase table of the last join launch
int summaries_init(EngineImpl* im, uint32_t flags);        // engine_create: the memory of the summaries the flags ask for
int summaries_reset(EngineImpl* im);                       // engine_reset: their tables zeroed on s_comp (the caller synchronises)
int launch_summaries(EngineImpl* im);                      // launch_queue: their passes behind the first join launch of im->inflight
int base_tally_touch(EngineImpl* im, int32_t contig);      // describe_batch, XCK_F_BASE_TALLY: the table of a contig whose batch is about to be queued (base_tally.h)
void base_tally_free(EngineImpl* im);                      // engine_destroy: the tables and buffers of base_tally.h
void ref_seq_free(EngineImpl* im);                         // ... and, called by it, the packed sequences and staging chunks of ref_seq.h
// defined in finish.hip
int finish_init(EngineImpl* im);                           // engine_create: per-device attributes of the fold kernels
int snp_verdicts(EngineImpl* im, uint32_t* d_kept);        // d_kept[s] = snp_passes() of sorted SNP s on the tallies of the last finish (enqueued on s_comp)
int molecule_stats_init(EngineImpl* im);                   // engine_create, XCK_F_UMI_CONSENSUS on a pileup pipeline: the counters' memory (umi_consensus.h)
int molecule_stats_reset(EngineImpl* im);                  // engine_reset: the counters zeroed on s_comp (the caller synchronises)
int unique_feature_init(EngineImpl* im, const xck_config* cfg);   // engine_create, XCK_F_UNIQUE_FEATURE on a basefc pipeline: the rank tables (umi_feature.h)
int unique_feature_reset(EngineImpl* im);                  // engine_reset: the counters are no longer valid
int umi_collapse_reset(EngineImpl* im);                    // engine_reset: the counters of umi_collapse.h are no longer valid
// Control words go to the host through MAPPED pinned memory written by a tiny kernel, never through the DMA engines: a 4 KB hipMemcpy
// D2H would queue behind a 170 MB result copy-out of another engine.  One block of `threads` on s_comp copies src[0, n) to host_alias
// (a device alias of pinned words, d_hctl); the caller checks hipGetLastError().
void publish_words(EngineImpl* im, const unsigned long long* src, unsigned long long* host_alias, int n, int threads);

}  // namespace xck
