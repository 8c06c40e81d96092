// engine.hip - MI355X (gfx950) counting engine: the join.  k_tile_meta, k_join and every device helper they use, the device tables
// the join reads (build_tables) and its launch (launch_join), and behind it the opt-in summary passes and the base tally pass, whose kernels use the
// join's own CIGAR loops and tile size.  Nothing else lives here, for one reason: this is the file the traffic stamp covers
// (profiles/pmc_traffic.json: bench.py reports roofline.traffic only while engine.hip + fold_partition.h hash to the stamp), so an
// edit here says "the join's bytes have to be counted again" and a feature's host code must not say that.  The per-GPU push
// pipeline (buffers, launch queue, overflow replay, push paths, create / reset / destroy) is pipeline.hip.
//
// Replaces the reference's per-region / per-SNP fetch loops
//   xcltk/rdr/fc/core.py:96-178  (fc_features -> fc_fet1 -> check_read / include test / MCount)
//   xcltk/baf/fc/core.py:70-247  (fc_features -> fc_fet1 -> plp_snp -> MCount/SCount/UCount)
// with ONE streaming pass over coordinate-sorted record batches:
//
//   k_tile_meta : one thread per 1024-read tile: extent, first candidate region (bisection on the running maximum of the
//                 region ends) or staged SNP windows (48-byte record).
//   k_join      : one block per tile; CIGAR run and the next regions / SNPs staged in LDS.
//                 basefc: read x region interval join, region-major and wave-uniform (the 64 reads of a wave walk the same
//                 candidate list once) + CIGAR-walk include test, accepted keys de-duplicated in an LDS hash set.
//                 pileup: single-block reads walk the SNPs under them SNP-major; spliced / indel reads are set aside and
//                 processed together after the sweeps ((read, SNP) pairs dealt evenly over each wave's lanes); hits with
//                 a base and "gap records" (SNPs inside N / D gaps) leave in two streams.
//                 Fragments are appended through sharded cursors.
//   finish      : finish.hip.  What the three files share is in engine_impl.h.
//
// Integer / byte work only - HBM-bound, no MFMA.  See DESIGN.md for layouts, byte counts and measurements.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <chrono>
#include <type_traits>
#include <hip/hip_runtime.h>
#include "engine_impl.h"
#include "ref_geom.h"

namespace xck {
#ifndef XCK_WS_SNP
#define XCK_WS_SNP 10           // 1 kb: the first probe lands within a SNP or two of the read (32 kb windows needed a binary search per read)
#endif
constexpr int WSS = XCK_WS_SNP;        // window shift of the SNP index (window -> first SNP)


// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool op_aligned(uint32_t op) { return (0x181u >> op) & 1u; }   // M,=,X
__device__ __forceinline__ bool op_ref(uint32_t op)     { return (0x18Du >> op) & 1u; }   // M,D,N,=,X
__device__ __forceinline__ bool op_query(uint32_t op)   { return (0x193u >> op) & 1u; }   // M,I,S,=,X

template <class K> struct JoinArgs {
    BatchTable bt;
    const TileMeta* meta;                 // [n_tiles]
    ReadFilter f;
    const int32_t* reg_s0; const int32_t* reg_e0; const int32_t* reg_row;   // regions per contig sorted by start (0-based half-open + output row)
    const int32_t* reg_pmax;                                                 // running maximum of reg_e0 inside the contig
    const int32_t* snp_p0;
    KeyLayout<K> kl;
    K* keys; uint64_t* vals; unsigned long long cap;   // cap = capacity of ONE shard
    K* nkeys; uint64_t* nvals;                          // pileup split mode: the stream of hits without a base (same shard capacity)
    unsigned long long* ctl;             // control block, see CTL_* below
    int32_t min_baseq;                   // pileup, BASEQ kernels only: a base whose quality byte is below it (and not 0xff) is not shown
};

static_assert(sizeof(JoinArgs<unsigned __int128>) <= 4000, "kernel arguments must stay under the 4 KiB kernarg limit");

struct ReadInfo { int32_t pos, endpos, n_al; uint32_t c0, c1; int32_t cell; uint64_t umi; bool ok;
                  bool span_is_cigar;        // endpos - pos is the CIGAR's reference length (false: unmapped flag / no CIGAR: 1)
                  int32_t m_rej, m_acc; };   // fraction mode: m < m_rej fails, m >= m_acc passes, between: divide

// `m / float(n) < min_include` (rdr/fc/core.py:160-165) is an IEEE double comparison of a ROUNDED quotient.  The
// fp64 divide costs ~40 VALU per (read, region) pair, so each read carries two integer bounds instead: with
// p = RN(f * n), any m < p(1 - 2^-50) has RN(m/n) < f and any m > p(1 + 2^-50) has RN(m/n) >= f (three roundings
// of 2^-53 each stay inside the 2^-50 margin); only an m between the bounds (f * n within 2^-50 of an integer)
// takes the exact divide.  tests/test_host_logic.py::test_fraction_bounds checks the equivalence exhaustively.
__device__ __forceinline__ void frac_bounds(ReadInfo& r, double f) {
    const double p = f * (double)r.n_al;
    r.m_rej = (int32_t)ceil(p * (1.0 - 0x1p-50));
    r.m_acc = (int32_t)floor(p * (1.0 + 0x1p-50)) + 1;
}
__device__ __forceinline__ bool frac_below(int32_t m, const ReadInfo& r0, double f) {
    ReadInfo r = r0;
    asm volatile("" : "+v"(r.n_al));                                  // (keeps the fp64 bounds here: hoisted, they cost every read of every sweep ~14 instructions)
    frac_bounds(r, f);                                                // only (read, region) pairs with a partial overlap get here
    if (m < r.m_rej) return true;
    if (m >= r.m_acc) return false;
    return (double)m / (double)r.n_al < f;
}

// ---- join kernel: one 256-thread block per tile of 1024 consecutive reads ---------------------
// Reads are coordinate sorted, so a tile touches a handful of index windows, regions / SNPs and
// one contiguous run of CIGAR words: all of that is staged in LDS once per tile (with a global
// fallback for anything outside the staged range - the staging is a cache, never a correctness
// assumption).  Accepted (read, region) keys go into an LDS hash set (64-bit keys), which removes
// the PCR/UMI duplicates that sit next to each other in a sorted BAM before they ever reach HBM;
// pileup hits and 128-bit keys go through an LDS queue.  The set / queue is flushed as one
// contiguous COO fragment: ONE atomicAdd on the global cursor per flush (a cursor word saturates
// at ~88 returning atomics/us on gfx950 - one per 256 reads was the bottleneck of the first
// version), wave ballot + mbcnt prefix compaction, coalesced 8/16-byte stores.
#ifndef XCK_STAMPS
#define XCK_STAMPS 0
#endif
// which of the 16 cursor shards a join block appends to: block index modulo 16 (XCK_SHARD_SHIFT 0), or runs of 2^shift
// consecutive tiles per shard (experiment for a cross-tile duplicate filter)
#ifndef XCK_SHARD_SHIFT
#define XCK_SHARD_SHIFT 0
#endif
#define JOIN_SHARD ((int)((blockIdx.x >> XCK_SHARD_SHIFT) & (NSHARD - 1)))
#ifndef XCK_TILE_ITEMS
#define XCK_TILE_ITEMS 4
#endif
#ifndef XCK_BAF_NQUEUE_BYTES
#define XCK_BAF_NQUEUE_BYTES 3072   // split mode: queue of the gap records (16 B each, about one per spliced read), flushed at the tile end
#endif
#ifndef XCK_BAF_BQUEUE_BYTES
#define XCK_BAF_BQUEUE_BYTES 3072   // split mode: queue of the hits with a base (~1 in 10), flushed at the tile end
#endif
#ifndef XCK_CX_CAP
#define XCK_CX_CAP 128            // pileup: spliced / indel reads of a tile set aside for the joint walk (beyond it they are walked in place)
#endif
#ifndef XCK_HS_BYTES
#define XCK_HS_BYTES 16384
#endif
#ifndef XCK_CG_CAP
#define XCK_CG_CAP 1536
#endif
#ifndef XCK_ST_CAP
#define XCK_ST_CAP 256
#endif
constexpr int TILE_ITEMS = XCK_TILE_ITEMS;
constexpr int TILE = JOIN_BLOCK * TILE_ITEMS;
constexpr int HS_BYTES = XCK_HS_BYTES;   // LDS set / queue storage per block
constexpr int HS_SLOTS = HS_BYTES / 8;   // slots of the 64-bit key set
constexpr int CG_CAP = XCK_CG_CAP;       // staged CIGAR words (basefc)
#ifndef XCK_CG_CAP_BAF
#define XCK_CG_CAP_BAF 1408       // pileup: with the 3 KB queues and 128 set-aside reads below its block fits 26.5 KB of LDS, i.e. 6 blocks per CU (6.14 -> 5.94 ms)
#endif
template <int MODE> struct CigCap { static constexpr int value = MODE == XCK_MODE_BAF ? XCK_CG_CAP_BAF : CG_CAP; };
constexpr int ST_CAP = XCK_ST_CAP;       // staged regions / SNPs
constexpr int ST_WIN = 64;               // staged index windows

template <class K, int MODE> struct JoinSmem {
    // basefc, 64-bit keys: accepted keys go through an LDS hash SET (a duplicate (region, cell, UMI) is dropped): the PCR /
    // UMI duplicates that sit next to each other in a sorted BAM never reach HBM.  Everything else uses plain queues.
    static constexpr bool USE_SET = sizeof(K) == 8 && MODE == XCK_MODE_BASEFC;
    static constexpr bool HAS_VAL = MODE == XCK_MODE_BAF;
    static constexpr int  SLOTS = HS_SLOTS;
    // pileup split mode (64-bit keys): a hit whose read shows NO base at the SNP (the SNP sits in an N / D gap - the
    // bulk of the hits of spliced reads) only matters if a read of the same (SNP, cell, UMI) WITH a base comes later in
    // fetch order (baf/fc/mcount.py:118-119: the earlier read holds the key).  Those hits go to their own queue / HBM
    // stream, which finish() never sorts: it is only looked up against the (small) sorted stream of hits with a base.
    static constexpr bool SPLIT = MODE == XCK_MODE_BAF && sizeof(K) == 8 && XCK_BAF_SPLIT;
    static constexpr int  STORE_BYTES = USE_SET ? SLOTS * 8 : (HAS_VAL ? (SPLIT ? XCK_BAF_BQUEUE_BYTES : 6144) : HS_BYTES);
    static constexpr int  QCAP = STORE_BYTES / (int)(sizeof(K) + (HAS_VAL ? 8 : 0));
    alignas(16) unsigned char store[STORE_BYTES];
    uint32_t cig[CigCap<MODE>::value];
    static constexpr int ST_BC = MODE == XCK_MODE_BASEFC ? ST_CAP : 1;    // region ends / rows: basefc only
    int32_t  st_a[ST_CAP], st_b[ST_BC], st_c[ST_BC];
    int32_t  st_w[ST_WIN + 1];
    uint32_t cg_lo, cg_n;                // staged CIGAR range [cg_lo, cg_lo + cg_n)
    int32_t  cg_all;                     // 1: that is the tile's whole CIGAR run
    int32_t  w0, nw;                     // basefc: staged regions [w0, w0 + nw) of the start-sorted arrays; pileup: staged SNP windows
    int32_t  k0, nk;                     // pileup: staged SNPs [k0, k0 + nk); basefc: k0 = position of the tile's first read
    uint32_t count;                      // entries currently in the queue
    uint32_t wuor[2 * (JOIN_BLOCK / 64)];  // per-wave OR of the UMI codes
    uint32_t wcnt[JOIN_BLOCK / 64];
    unsigned long long base;
    static constexpr int  NQCAP = SPLIT ? XCK_BAF_NQUEUE_BYTES / 16 : 1;
    uint64_t nq_key[NQCAP], nq_val[NQCAP];
    uint32_t ncount;
    unsigned long long nbase;
    // pileup: (read, SNP) pairs under aligned blocks, parked per wave (64 slots each) until their bases are fetched together
    static constexpr int PR = MODE == XCK_MODE_BAF ? JOIN_BLOCK : 1;
    uint64_t pk_umi[PR];
    // pileup: reads with N / D gaps (or without a CIGAR span) of the whole tile, set aside for pileup_complex()
    static constexpr int CXCAP = MODE == XCK_MODE_BAF ? XCK_CX_CAP : 1;
    uint64_t cx_umi[CXCAP]; int32_t cx_pos[CXCAP], cx_end[CXCAP], cx_cell[CXCAP], cx_idx[CXCAP]; uint32_t cx_c0[CXCAP], cx_c1[CXCAP], cx_s0[CXCAP], cx_sl[CXCAP];
    uint32_t cx_n;
    int32_t  pk_k[PR], pk_qi[PR], pk_cell[PR], pk_idx[PR];
    uint32_t pk_s0[PR], pk_sl[PR];
    __device__ K* keys() { return reinterpret_cast<K*>(store); }
    __device__ uint64_t* vals() { return reinterpret_cast<uint64_t*>(store + (size_t)QCAP * sizeof(K)); }
    __device__ unsigned long long* hkeys() { return reinterpret_cast<unsigned long long*>(store); }            // set mode
};

// (sm.cg_all - block-uniform, from k_tile_meta - says that the tile's whole CIGAR run is staged: practically always at the capacities
// above, and the two-path form costs a handful of exec-mask instructions per word)
template <class K, int MODE>
__device__ __forceinline__ uint32_t cig_at(const JoinArgs<K>& a, const BatchDesc& d, const JoinSmem<K, MODE>& sm, uint32_t c) {
    uint32_t rel = c - sm.cg_lo;
    if (__builtin_amdgcn_readfirstlane(sm.cg_all)) return sm.cig[rel];
    return rel < sm.cg_n ? sm.cig[rel] : as_global(d.cigar)[c];
}

// the seven SoA fields of one read, fetched one sweep ahead of their use (software prefetch)
struct RawRead { int32_t pos, cell; uint64_t umi; uint32_t c0, c1; uint32_t flag; int32_t mapq; uint32_t s0, s1; bool valid; };
// The arrays are addressed as (scalar base + tile start) + a per-lane offset below 8 KB: the loads then take the base from SGPRs
// and ONE 32-bit offset register per element size, where base + 64-bit index arithmetic cost ~12 VALU instructions per sweep -
// in a kernel that is bound by VALU issue.  tile0 is wave-uniform; k = read of the tile (< TILE).
template <bool WITH_SEQ>
__device__ __forceinline__ RawRead fetch_read(const BatchDesc& d, int tile0, uint32_t k, bool valid) {
    RawRead w; w.valid = valid; w.pos = 0; w.cell = -1; w.umi = 0; w.c0 = w.c1 = 0; w.flag = 0; w.mapq = 0; w.s0 = w.s1 = 0;
    if (valid) { w.flag = (as_global(d.flag) + tile0)[k]; w.mapq = (as_global(d.mapq) + tile0)[k]; w.cell = (as_global(d.cell) + tile0)[k]; w.umi = (as_global(d.umi) + tile0)[k];
                 w.pos = (as_global(d.pos) + tile0)[k]; w.c0 = (as_global(d.cig_off) + tile0)[k]; w.c1 = (as_global(d.cig_off) + tile0)[k + 1];
                 if (WITH_SEQ) { w.s0 = (as_global(d.seq_off) + tile0)[k]; w.s1 = (as_global(d.seq_off) + tile0)[k + 1]; } }
    return w;
}

// The two pure CIGAR loops, generic over where a word comes from (word_at(c): cig_at in the join, a plain global load in
// read_fate.h).  Reference length and aligned bases of the words [c0, c1):
template <class WordAt>
__device__ __forceinline__ void cigar_summary(WordAt word_at, uint32_t c0, uint32_t c1, int32_t& rlen, int32_t& n_al) {
    for (uint32_t c = c0; c < c1; c++) {
        uint32_t w = word_at(c); uint32_t op = w & 15u; int32_t l = int32_t(w >> 4);
        if (op_ref(op)) rlen += l;
        if (op_aligned(op)) n_al += l;
    }
}
// __get_include_len(): aligned bases with s0 <= p < e0 (reads pos, endpos, n_al, c0, c1 and span_is_cigar of r)
template <class WordAt>
__device__ __forceinline__ int32_t included_len(WordAt word_at, const ReadInfo& r, int32_t s0, int32_t e0) {
    // both shortcuts need endpos to be the CIGAR's own end (an unmapped-flagged read with a CIGAR is fetched by its first base
    // only, yet its aligned positions are counted over the whole CIGAR)
    if (r.span_is_cigar && r.pos >= s0 && r.endpos <= e0) return r.n_al;
    // no D / N in the CIGAR (reference span == aligned length): the aligned bases are one block, no walk needed
    if (r.span_is_cigar && r.endpos - r.pos == r.n_al) return max(min(r.endpos, e0) - max(r.pos, s0), 0);
    int32_t p = r.pos, m = 0;
    for (uint32_t c = r.c0; c < r.c1; c++) {
        uint32_t w = word_at(c); uint32_t op = w & 15u; int32_t l = int32_t(w >> 4);
        if (op_aligned(op)) {
            int32_t lo = max(p, s0), hi = min(p + l, e0);
            if (hi > lo) m += hi - lo;
            p += l;
        } else if (op_ref(op)) p += l;
    }
    return m;
}

// filter + CIGAR summary of a read (endpos = htslib bam_endpos, n_al = len(read.positions))
template <class K, int MODE>
__device__ __forceinline__ ReadInfo load_read(const JoinArgs<K>& a, const BatchDesc& d, const JoinSmem<K, MODE>& sm, const RawRead& w) {
    ReadInfo r; r.ok = false; r.span_is_cigar = false; r.pos = 0; r.endpos = 0; r.n_al = 0; r.c0 = r.c1 = 0; r.cell = -1; r.umi = 0; r.m_rej = 0; r.m_acc = 0;
    if (!w.valid) return r;
    uint32_t flag = w.flag;
    int32_t mapq = w.mapq;
    r.cell = w.cell;
    r.umi = w.umi;
    r.pos = w.pos;
    r.c0 = w.c0; r.c1 = w.c1;
    bool ok = mapq >= a.f.min_mapq;
    ok = ok && !(a.f.excl_flag && (flag & a.f.excl_flag));
    ok = ok && !(a.f.incl_flag && !(flag & a.f.incl_flag));
    ok = ok && !(a.f.no_orphan && (flag & BAM_FPAIRED) && !(flag & BAM_FPROPER_PAIR));
    ok = ok && r.cell >= 0 && r.umi != XCK_UMI_NONE;                  // (a negative pos is kept: fetch() only asks pos < stop && endpos > start)
    if (!ok) return r;
    int32_t rlen = 0, n_al = 0;
    cigar_summary([&](uint32_t c) { return cig_at(a, d, sm, c); }, r.c0, r.c1, rlen, n_al);
    // htslib bam_endpos(): an unmapped-flagged read, or one without reference-consuming CIGAR, spans one base for fetch();
    // read.positions (the include test) still follows the CIGAR
    r.span_is_cigar = !((flag & BAM_FUNMAP) || r.c1 == r.c0 || rlen == 0);
    if (!r.span_is_cigar) rlen = 1;
    r.endpos = r.pos + rlen;
    r.n_al = n_al;
    r.ok = n_al >= a.f.min_len;
    return r;
}

// ---- appending to the sharded HBM streams (ctl_word: ctl_cursor / ctl_ncursor of the block's shard) ----
// one record straight to HBM (slow path: the LDS set / queue is saturated)
template <class K, bool WITH_VAL>
__device__ __forceinline__ void append_one(const JoinArgs<K>& a, int ctl_word, K* keys, uint64_t* vals, K key, uint64_t val) {
    const int shard = JOIN_SHARD;
    unsigned long long idx = atomicAdd(&a.ctl[ctl_word], 1ull);
    if (idx < a.cap) { idx += (unsigned long long)shard * a.cap; keys[idx] = key; if (WITH_VAL) vals[idx] = val; }
    else atomicExch(&a.ctl[CTL_OVERFLOW], 1ull);
}
// room for a fragment of `total` records: its first index in the stream, or ~0 (with the overflow flag raised) when it does not fit
template <class K>
__device__ __forceinline__ unsigned long long reserve_fragment(const JoinArgs<K>& a, int ctl_word, uint32_t total) {
    unsigned long long b = 0;
    if (total) {
        const int shard = JOIN_SHARD;
        b = atomicAdd(&a.ctl[ctl_word], (unsigned long long)total);
        if (b + total > a.cap) { atomicExch(&a.ctl[CTL_OVERFLOW], 1ull); b = ~0ull; }
        else b += (unsigned long long)shard * a.cap;
    }
    return b;
}

template <class K, int MODE>
__device__ __forceinline__ void emit(const JoinArgs<K>& a, JoinSmem<K, MODE>& sm, K key, uint64_t val) {
    if constexpr (JoinSmem<K, MODE>::USE_SET) {
        constexpr int SLOTS = JoinSmem<K, MODE>::SLOTS;
        unsigned long long* set = sm.hkeys();
        const unsigned long long kk = (unsigned long long)key;
        uint32_t slot = set_slot<SLOTS>(kk);
        // double hashing: the 64 lanes of a wave wait for the LONGEST probe sequence among their keys, and linear probing's
        // clusters make that 8 - 10 probes at the fill a tile reaches; an odd, key-dependent stride (any odd stride visits every
        // slot of a power-of-two table) keeps the sequences geometric
        const uint32_t stride = (((uint32_t)(kk >> 7) ^ (uint32_t)(kk >> 41)) | 1u) & (SLOTS - 1);
        for (int probe = 0; probe < 24; probe++) {
            unsigned long long prev = atomicCAS(&set[slot], ~0ull, kk);
            if (prev == ~0ull || prev == kk) return;                 // new key, or a duplicate (same region, cell, UMI); no shared counter: flush points are static
            slot = (slot + stride) & (SLOTS - 1);
        }
        append_one<K, MODE == XCK_MODE_BAF>(a, ctl_cursor(JOIN_SHARD), a.keys, a.vals, key, val);
    } else {
        uint32_t idx = atomicAdd(&sm.count, 1u);
        if (idx < (uint32_t)JoinSmem<K, MODE>::QCAP) { sm.keys()[idx] = key; if (MODE == XCK_MODE_BAF) sm.vals()[idx] = val; }
        else append_one<K, MODE == XCK_MODE_BAF>(a, ctl_cursor(JOIN_SHARD), a.keys, a.vals, key, val);
    }
}

// no-base pileup hit (split mode): second LDS queue, spill straight to the second HBM stream
template <class K, int MODE>
__device__ __forceinline__ void emit_nobase(const JoinArgs<K>& a, JoinSmem<K, MODE>& sm, K key, uint64_t val) {
    const uint32_t idx = atomicAdd(&sm.ncount, 1u);
    if (idx < (uint32_t)JoinSmem<K, MODE>::NQCAP) { sm.nq_key[idx] = (uint64_t)key; sm.nq_val[idx] = val; }
    else append_one<K, true>(a, ctl_ncursor(JOIN_SHARD), a.nkeys, a.nvals, key, val);
}
// phase stamps of the join kernel (build with -DXCK_STAMPS=1): cycles of wave 0 of every block between two stamps, kept in
// registers and stored over the block's own TileMeta record (12 words, read in the prologue and dead since) - no atomics, no
// extra traffic worth the name (the first version added 12 global atomics per block: 48 ms instead of 7.5).  The host sums
// the records after the launch; finish_t() prints the table.  Slots: 0 tile record, 1 prologue loads + staging, 2 staging barrier,
// 3-6 the four sweeps, 7 barrier before the flush, 8 flush: count, 9 flush: cursor atomic, 10 flush: stores, 11 tail.
struct StampRec { long long t; uint32_t d[12]; };
#if XCK_STAMPS
#define XCK_STAMP(sr, slot) do { const long long t_ = clock64(); (sr)->d[slot] += (uint32_t)(t_ - (sr)->t); (sr)->t = t_; } while (0)
#else
#define XCK_STAMP(sr, slot) do {} while (0)
#endif
// split mode: both queues leave in ONE round (two cursor atomics in flight together, one set of barriers)
template <class K, int MODE>
__device__ __forceinline__ void flush_split(const JoinArgs<K>& a, JoinSmem<K, MODE>& sm, StampRec* ts = nullptr) {   // block-wide; all inserts are complete (barrier before)
    const uint32_t tb = min(sm.count, (uint32_t)JoinSmem<K, MODE>::QCAP), tn = min(sm.ncount, (uint32_t)JoinSmem<K, MODE>::NQCAP);
    if (threadIdx.x < 2) {
        const unsigned long long b = reserve_fragment(a, threadIdx.x ? ctl_ncursor(JOIN_SHARD) : ctl_cursor(JOIN_SHARD), threadIdx.x ? tn : tb);
        if (threadIdx.x) sm.nbase = b; else sm.base = b;
    }
    __syncthreads();
    XCK_STAMP(ts, 9);
    const unsigned long long db = sm.base, dn = sm.nbase;
    if (db != ~0ull) for (uint32_t t = threadIdx.x; t < tb; t += JOIN_BLOCK) { a.keys[db + t] = sm.keys()[t]; a.vals[db + t] = sm.vals()[t]; }
    if (dn != ~0ull) for (uint32_t t = threadIdx.x; t < tn; t += JOIN_BLOCK) { a.nkeys[dn + t] = (K)sm.nq_key[t]; a.nvals[dn + t] = sm.nq_val[t]; }
    __syncthreads();
    if (threadIdx.x == 0) { sm.count = 0; sm.ncount = 0; }
    __syncthreads();
    XCK_STAMP(ts, 10);
}

// write the LDS set / queue to HBM as one contiguous fragment; block-wide call
template <class K, int MODE>
__device__ __forceinline__ void flush(const JoinArgs<K>& a, JoinSmem<K, MODE>& sm, StampRec* ts = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if constexpr (JoinSmem<K, MODE>::USE_SET) {
        unsigned long long* set = sm.hkeys();
        constexpr int PER_WAVE = JoinSmem<K, MODE>::SLOTS / (JOIN_BLOCK / 64);
        uint32_t c = 0;
        for (int s = wave * PER_WAVE + lane; s < (wave + 1) * PER_WAVE; s += 64) c += (set[s] != ~0ull) ? 1u : 0u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
        if (lane == 0) sm.wcnt[wave] = c;
        __syncthreads();
        XCK_STAMP(ts, 8);
        if (threadIdx.x == 0) {
            sm.base = reserve_fragment(a, ctl_cursor(JOIN_SHARD), sm.wcnt[0] + sm.wcnt[1] + sm.wcnt[2] + sm.wcnt[3]);
            sm.count = 0;
        }
        __syncthreads();
        XCK_STAMP(ts, 9);
        unsigned long long dst = sm.base;
        for (int w = 0; w < wave; w++) dst += sm.wcnt[w];
        // (wave-uniform: kept in SGPRs, so that the stores take base + fragment start from scalars and one 32-bit lane offset)
        dst = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(dst >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)dst);
        const bool fits = sm.base != ~0ull;
        for (int s = wave * PER_WAVE + lane; s < (wave + 1) * PER_WAVE; s += 64) {
            unsigned long long v = set[s];
            bool valid = v != ~0ull;
            unsigned long long m = __ballot(valid);
            if (valid) {
                uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (fits) (a.keys + dst)[pre] = (K)v;
                set[s] = ~0ull;
            }
            dst += __popcll(m);
        }
        __syncthreads();
        XCK_STAMP(ts, 10);
    } else {
        __syncthreads();
        const uint32_t total = min(sm.count, (uint32_t)JoinSmem<K, MODE>::QCAP);
        if (threadIdx.x == 0) sm.base = reserve_fragment(a, ctl_cursor(JOIN_SHARD), total);
        __syncthreads();
        const unsigned long long dst = sm.base;
        if (dst != ~0ull)
            for (uint32_t t = threadIdx.x; t < total; t += JOIN_BLOCK) {
                a.keys[dst + t] = sm.keys()[t];
                if (MODE == XCK_MODE_BAF) a.vals[dst + t] = sm.vals()[t];
            }
        __syncthreads();
        if (threadIdx.x == 0) sm.count = 0;
        __syncthreads();
    }
}

// basefc: read x region interval join, region-major.  Regions are sorted by start inside the contig, the reads of a wave are
// (in a sorted BAM) a narrow position range, so the whole wave walks ONE short list together: from the tile's first
// candidate (first region whose running-maximum end lies beyond the tile's first position, k_tile_meta) up to the first
// region that starts at or after the end of every read of the wave (one ballot per step, no reduction).  Start, end and row of a region are wave-uniform (LDS
// broadcast reads of the staged slice); each lane only compares its own read against them - no per-lane index lookups,
// no divergent loop counts.  A wave that holds a read left of the tile's first read (unsorted input) scans from the
// contig's first region: its chunks left of the staged slice [lb, lb + n_st) take start / end / row from global memory, lane
// by lane (`whole` below is false for them), so sortedness is a speed assumption, never a correctness one
// (tests/test_gpu_parity.py::test_unsorted_reads).
// minimum / maximum of one int32 per lane over the 64 lanes of a wave (all lanes active): four row_shr steps inside the rows
// of 16 lanes, row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3 - lane 63 then holds the result.  Six DPP
// VALU ops and one v_readlane; no LDS traffic (a __shfl_xor butterfly is six ds_bpermute round trips).
template <bool MAX>
__device__ __forceinline__ int32_t wave_minmax(int32_t v) {
    constexpr int32_t ID = MAX ? std::numeric_limits<int32_t>::min() : std::numeric_limits<int32_t>::max();
#define XCK_DPP_STEP(ctrl, rows) { const int32_t t_ = __builtin_amdgcn_update_dpp(ID, v, ctrl, rows, 0xf, false); v = MAX ? max(v, t_) : min(v, t_); }
    XCK_DPP_STEP(0x111, 0xf) XCK_DPP_STEP(0x112, 0xf) XCK_DPP_STEP(0x114, 0xf) XCK_DPP_STEP(0x118, 0xf)   // row_shr:1,2,4,8
    XCK_DPP_STEP(0x142, 0xa) XCK_DPP_STEP(0x143, 0xc)                                                       // row_bcast:15, row_bcast:31
#undef XCK_DPP_STEP
    return __builtin_amdgcn_readlane(v, 63);
}

// The walk is done 64 regions at a time with the REGIONS in the lanes: lane l loads start / end of region kb + l (one
// conflict-free LDS read per array) and asks whether the region can meet any read of the wave at all - start below the
// largest read end, end beyond the smallest read position (two DPP reductions per sweep).  One ballot gives the candidate
// regions of the chunk; only those are visited, their start / end / row taken from the lanes by v_readlane (no memory
// round trip, scalar operands for the per-read compare).  The first version visited every region from the tile's first
// candidate on, each visit two dependent LDS reads + readfirstlane (7.76 -> 7.44 ms at configs[2]; the walk it replaces is in
// the history: commit 97658ab).  What bounds the kernel now is VALU issue: 1756 VALU instructions per wave x 4 cycles x 6
// waves per SIMD = 88 % of a wave's 48 k-cycle life; by ablation (profiles/experiments/join_r04/) 676 of them are the read
// summary + prologue + flush, 583 the walk, ~500 the set inserts.
template <class K, int MODE>
__device__ __forceinline__ uint32_t join_regions(const JoinArgs<K>& a, const BatchDesc& d, JoinSmem<K, MODE>& sm, const ReadInfo& r,
                                                 const int32_t lb, const int32_t n_st, const int32_t p_first, StampRec* ts = nullptr, int sweep = 0) {   // staged slice: regions [lb, lb + n_st); scalars
    uint32_t n_acc = 0;
    if (!__ballot(r.ok)) return 0;                                   // no read of this wave passed the filter (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int32_t reg_lo = __builtin_amdgcn_readfirstlane(d.reg_lo), reg_hi = __builtin_amdgcn_readfirstlane(d.reg_hi);
    const int32_t wmin = wave_minmax<false>(r.ok ? r.pos : std::numeric_limits<int32_t>::max());
    const int32_t wmax = wave_minmax<true>(r.ok ? r.endpos : std::numeric_limits<int32_t>::min());
    // A region that CONTAINS the whole wave (start <= smallest position, end >= largest read end - two scalar compares; genes are
    // kilobases long, the 64 reads of a wave span a few hundred bases at most, so this is the usual case) takes every read of the
    // wave that passed the filter: all its aligned bases are inside (included_len's first shortcut), m == n, the fraction is 1.
    // What is left per read is the key and the set insert; the overlap / include arithmetic runs only for regions whose
    // boundary falls inside the wave.  (A read whose fetch span is not its CIGAR's - unmapped flag - rules the shortcut out.)
    const bool all_span = !__ballot(r.ok && !r.span_is_cigar);
    const bool full_ok = r.ok && (a.f.frac_mode ? r.n_al > 0 : r.n_al >= a.f.min_inc_len);
    const K kbase = a.kl.make(0u, (uint32_t)r.cell, r.umi);
    // p_first = position of the tile's first read: a read left of it means unsorted input, the list is then walked from its start
    for (int32_t kb = __ballot(r.ok && r.pos < p_first) ? reg_lo : lb; kb < reg_hi; kb += 64) {
        const int32_t k = kb + lane;
        const uint32_t rel = (uint32_t)(k - lb);
        // (scalar: the whole chunk is staged and inside the contig - the usual case; the per-lane form below is the general one.
        // kb < lb happens on the walk from reg_lo: a chunk that starts up to 63 regions left of the staged slice is not "whole",
        // although (uint32_t)(kb - lb) + 64 wraps to a small number)
        const bool whole = kb >= lb && (uint32_t)(kb - lb) + 64u <= (uint32_t)n_st && kb + 64 <= reg_hi;
        bool in = true, staged = true;
        int32_t s0 = std::numeric_limits<int32_t>::max(), e0 = std::numeric_limits<int32_t>::min(), row = 0;
        if (whole) { s0 = sm.st_a[rel]; e0 = sm.st_b[rel]; }
        else {
            in = k < reg_hi; staged = rel < (uint32_t)n_st;
            if (in) { s0 = staged ? sm.st_a[rel] : as_global(a.reg_s0)[k]; e0 = staged ? sm.st_b[rel] : as_global(a.reg_e0)[k]; }
        }
        const bool last = __ballot(!in || s0 >= wmax) != 0;          // sorted by start: no read of the wave reaches a region after this chunk
        unsigned long long cand = __ballot(in && s0 < wmax && e0 > wmin);
        if (cand) { if (whole) row = sm.st_c[rel]; else if (in) row = staged ? sm.st_c[rel] : as_global(a.reg_row)[k]; }
#if XCK_STAMPS == 2
        if (sweep == 0) { XCK_STAMP(ts, 4); ts->d[11] += (uint32_t)__popcll(cand); }      // (slot 11: candidate regions of sweep 0)
#endif
        while (cand) {
            const int b = (int)__builtin_ctzll(cand); cand &= cand - 1;
            const int32_t rs0 = __builtin_amdgcn_readlane(s0, b), re0 = __builtin_amdgcn_readlane(e0, b), rrow = __builtin_amdgcn_readlane(row, b);
            const K krow = K((uint32_t)rrow) << (a.kl.cbits + a.kl.ubits);      // wave-uniform: scalar shift
            if (all_span && wmin >= rs0 && wmax <= re0) {             // the region contains every read of the wave
                if (full_ok) { emit<K, MODE>(a, sm, kbase | krow, 0); n_acc++; }
                continue;
            }
            if (!(r.ok && r.pos < re0 && r.endpos > rs0)) continue;  // htslib fetch overlap
            const int32_t m = included_len([&](uint32_t c) { return cig_at(a, d, sm, c); }, r, rs0, re0);
            if (a.f.frac_mode) {
                if (r.n_al <= 0) continue;
                // m == n gives exactly 1.0, never below a threshold in (0,1): skip the fp64 divide
                if (m != r.n_al && frac_below(m, r, a.f.min_inc_frac)) continue;   // IEEE double, as m / float(n)
            } else if (m < a.f.min_inc_len) continue;
            emit<K, MODE>(a, sm, kbase | krow, 0);
            n_acc++;
        }
        if (last) break;
    }
    return n_acc;
}


// position of SNP k (staged slice first)
template <class K, int MODE>
__device__ __forceinline__ int32_t snp_p0(const JoinArgs<K>& a, const JoinSmem<K, MODE>& sm, int32_t k) {
    const uint32_t dl = (uint32_t)(k - sm.k0);
    return dl < (uint32_t)sm.nk ? sm.st_a[dl] : as_global(a.snp_p0)[k];
}

template <class K, int MODE>
__device__ __forceinline__ int32_t lower_snp_tail(const JoinArgs<K>& a, const BatchDesc& d, int32_t k, int32_t x) {
    while (k < d.snp_end && as_global(a.snp_p0)[k] < x) k++;
    return k;
}
// first SNP k >= k_from of the contig with position >= x: binary search in the staged slice, linear beyond it
template <class K, int MODE>
__device__ __forceinline__ int32_t lower_snp(const JoinArgs<K>& a, const BatchDesc& d, const JoinSmem<K, MODE>& sm, int32_t k_from, int32_t x) {
    int32_t k = k_from;
    const uint32_t dl = (uint32_t)(k - sm.k0);
    if (dl < (uint32_t)sm.nk) {
        int32_t lo = (int32_t)dl, hi = sm.nk;
#pragma unroll
        for (int q = 0; q < 3; q++) if (lo < hi && sm.st_a[lo] < x) lo++;       // the answer is usually 0-2 SNPs away
        if (lo < hi && sm.st_a[lo] >= x) return sm.k0 + lo;
        while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (sm.st_a[mid] < x) lo = mid + 1; else hi = mid; }
        k = sm.k0 + lo;
        if (lo < sm.nk) return k;
    }
    return lower_snp_tail<K, MODE>(a, d, k, x);
}
// base of a read at query offset qi: the allele nibble of its 4-bit sequence [s0, s0 + sl), or -1 where no sequence is stored for that offset
__device__ __forceinline__ int base_at(const BatchDesc& d, uint32_t s0, uint32_t sl, int32_t qi) {
    int al = -1;
    if ((uint32_t)(qi >> 1) < sl) { const uint32_t by = as_global(d.seq)[s0 + (uint32_t)(qi >> 1)]; al = (qi & 1) ? int(by & 15u) : int(by >> 4); }
    return al;
}
// ... under a base-quality floor (xck_config.min_baseq; the BASEQ kernels only): the quality byte of the same query offset lies at
// 2 * s0 + qi of the batch's quality column (two bytes per sequence byte, the pad of an odd read 0xff) and is loaded beside the nibble.
// A stored base with 0xff != q < min_q is masked: the pair keeps its key and shows no base (stored / masked say which of the two happened).
// BqCount: the pairs drain() has fetched for this wave, wave-uniform (one ballot + popcount each per batch of parked pairs).  The pairs of
// the set-aside reads, whose walks diverge, are summed per walk and added to the block's two LDS words - st_b[0] / st_c[0], which the
// pileup's staging leaves unused (JoinSmem::ST_BC), so the default kernels' LDS and registers are what they were.
struct BqCount { uint32_t w_base = 0, w_masked = 0; };
template <class K, int MODE> __device__ __forceinline__ uint32_t* bq_lds_base(JoinSmem<K, MODE>& sm) { return (uint32_t*)&sm.st_b[0]; }
template <class K, int MODE> __device__ __forceinline__ uint32_t* bq_lds_masked(JoinSmem<K, MODE>& sm) { return (uint32_t*)&sm.st_c[0]; }
__device__ __forceinline__ int base_at_q(const BatchDesc& d, uint32_t s0, uint32_t sl, int32_t qi, int32_t min_q, bool& stored, bool& masked) {
    int al = -1;
    stored = (uint32_t)(qi >> 1) < sl; masked = false;
    if (stored) {
        const uint32_t by = as_global(d.seq)[s0 + (uint32_t)(qi >> 1)];
        const int32_t q = as_global(d.qual)[2u * s0 + (uint32_t)qi];          // (a 32-bit offset beside the scalar base, as for the nibble: the push paths keep sequence offsets of such batches below 2^31)
        al = (qi & 1) ? int(by & 15u) : int(by >> 4);
        masked = q != 0xff && q < min_q;
        if (masked) al = -1;
    }
    return al;
}
// One read whose reference span is not one aligned block (N / D gaps, no CIGAR span, unmapped flag): the pileup of
// baf/fc/mcount.py:109-127 + utils/sam.py:4-40 over its CIGAR.  SNPs under aligned blocks are hits with a base (fetched
// here: these reads are few); the SNPs inside a gap - where the read holds the key but shows no base - leave as ONE range
// record per gap, (first SNP, cell, UMI | ordinal, count - 1), in pieces of 32 SNPs: a spliced read over 20 SNPs costs one
// 16-byte record instead of 20 hits.  Such reads are collected per tile and walked together (k_join), so that the waves
// that walk them are full and the other 85 % of the reads never wait for them.
template <class K, int MODE, bool BASEQ>
__device__ __forceinline__ uint32_t pileup_complex(const JoinArgs<K>& a, const BatchDesc& d, JoinSmem<K, MODE>& sm, int32_t pos, int32_t endpos,
                                                   uint32_t c0, uint32_t c1, int32_t cell, uint64_t umi, uint32_t s0, uint32_t sl, int32_t idx, BqCount& bq) {
    const int32_t w_lo = max(pos, 0) >> WSS;
    if (w_lo >= d.n_swin) return 0;
    const int32_t k_w = (uint32_t)(w_lo - sm.w0) < (uint32_t)sm.nw ? sm.st_w[w_lo - sm.w0] : as_global(d.snp_win)[w_lo];
    int32_t k = lower_snp<K, MODE>(a, d, sm, k_w, pos);
    const uint64_t ordv = (d.ordinal_base + (uint64_t)idx) << ALLELE_BITS;
    uint32_t n = 0;
    uint32_t nb = 0, nm = 0;                                                  // BASEQ: pairs of this read with a stored base / masked
    auto gap = [&](int32_t ka, int32_t kb) {
        if constexpr (JoinSmem<K, MODE>::SPLIT) {
            for (int32_t ks = ka; ks < kb; ks += 32)
                emit_nobase<K, MODE>(a, sm, a.kl.make((uint32_t)ks, (uint32_t)cell, umi), ordv | (uint64_t)(min(kb - ks, 32) - 1));
        } else for (int32_t ks = ka; ks < kb; ks++) emit<K, MODE>(a, sm, a.kl.make((uint32_t)ks, (uint32_t)cell, umi), ordv);
        n += (uint32_t)(kb - ka);
    };
    int32_t rp = pos, q = 0;
    for (uint32_t cc = c0; cc < c1 && rp < endpos; cc++) {
        const uint32_t w = cig_at(a, d, sm, cc); const uint32_t op = w & 15u; const int32_t l = int32_t(w >> 4);
        if (op_ref(op) && l != 0) {
            const int32_t k2 = lower_snp<K, MODE>(a, d, sm, k, min(rp + l, endpos));
            if (op_aligned(op)) {
                for (int32_t kk = k; kk < k2; kk++) {
                    const int32_t qi = q + (snp_p0<K, MODE>(a, sm, kk) - rp);
                    int al;
                    if constexpr (BASEQ) { bool st, mk; al = base_at_q(d, s0, sl, qi, a.min_baseq, st, mk); nb += st; nm += mk; }
                    else al = base_at(d, s0, sl, qi);
                    const K key = a.kl.make((uint32_t)kk, (uint32_t)cell, umi);
                    if (JoinSmem<K, MODE>::SPLIT && al < 0) emit_nobase<K, MODE>(a, sm, key, ordv);
                    else emit<K, MODE>(a, sm, key, ordv | (uint64_t)(al + 1));
                }
                n += (uint32_t)(k2 - k);
            } else if (k2 > k) gap(k, k2);
            k = k2; rp += l;
        }
        if (op_aligned(op) || op == 1u || op == 4u) q += l;
    }
    if (rp < endpos) {                                                        // no CIGAR / zero reference length: the position itself, without a base
        const int32_t k2 = lower_snp<K, MODE>(a, d, sm, k, endpos);
        if (k2 > k) gap(k, k2);
    }
    if constexpr (BASEQ) { if (nb) atomicAdd(bq_lds_base(sm), nb); if (nm) atomicAdd(bq_lds_masked(sm), nm); }
    return n;
}

// one thread per tile: locate the batch, read the tile's extent, size the LDS staging
template <int MODE>
__global__ __launch_bounds__(256) void k_tile_meta(BatchTable bt, TileMeta* __restrict__ out, const int32_t* __restrict__ rpmax) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= bt.n_tiles) return;
    int lo = 0, hi = bt.n_batches - 1;
    while (lo < hi) { int mid = (lo + hi + 1) >> 1; if (bt.desc[mid].tile0 <= t) lo = mid; else hi = mid - 1; }
    const BatchDesc& d = bt.desc[lo];
    TileMeta m;
    m.b = lo; m.r0 = (t - d.tile0) * TILE; m.r1 = min(m.r0 + TILE, d.n); m.pad = 0;
    const uint32_t c_lo = as_global(d.cig_off)[m.r0], c_hi = as_global(d.cig_off)[m.r1];
    const int32_t p_first = max(as_global(d.pos)[m.r0], 0);
    m.c_lo = c_lo; m.cg_n = min(c_hi - c_lo, (uint32_t)CigCap<MODE>::value); m.pad = c_hi - c_lo <= (uint32_t)CigCap<MODE>::value ? 1 : 0;
    m.w0 = p_first >> WSS; m.nw = 0; m.e0 = 0; m.n_ent = 0; m.k0 = 0; m.nk = 0;
    if (MODE == XCK_MODE_BASEFC) {
        // first candidate region of the tile: the first one whose running-maximum end lies beyond the first read's position
        // (every region before it ends at or before that position; reads further right cannot reach them either)
        const int32_t p0 = as_global(d.pos)[m.r0];
        int32_t lo = d.reg_lo, hi = d.reg_hi;
        while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (as_global(rpmax)[mid] > p0) hi = mid; else lo = mid + 1; }
        m.e0 = lo; m.n_ent = min(d.reg_hi - lo, ST_CAP); m.k0 = p0;
    } else {
        if (m.w0 < d.n_swin) { m.k0 = as_global(d.snp_win)[m.w0]; m.nk = min(d.snp_end - m.k0, ST_CAP); m.nw = min(d.n_swin - m.w0, ST_WIN); }
    }
    out[t] = m;
}

// ---- the pileup walk of one sweep: the counterpart of join_regions() ----
// the bases of the pairs a wave has parked (pr_n of them, wave-uniform) are fetched together and leave as hits; the segment is free again
template <class K, int MODE, bool BASEQ>
__device__ __forceinline__ void drain(const JoinArgs<K>& a, const BatchDesc& d, JoinSmem<K, MODE>& sm, int& pr_n, BqCount& bq) {
    const int lane = threadIdx.x & 63, wb = threadIdx.x & ~63;          // wb: first slot of this wave's segment
    constexpr uint64_t AL_MASK = (uint64_t)((1u << ALLELE_BITS) - 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    bool st = false, mk = false;
    if (lane < pr_n) {
        const int u = wb + lane;
        int al;                                                             // -1: key held, no base
        if constexpr (BASEQ) al = base_at_q(d, sm.pk_s0[u], sm.pk_sl[u], sm.pk_qi[u], a.min_baseq, st, mk); else al = base_at(d, sm.pk_s0[u], sm.pk_sl[u], sm.pk_qi[u]);
        const K key = a.kl.make((uint32_t)sm.pk_k[u], (uint32_t)sm.pk_cell[u], sm.pk_umi[u]);
        const uint64_t val = ((d.ordinal_base + (uint64_t)sm.pk_idx[u]) << ALLELE_BITS) | (uint64_t)(al + 1);
        if (JoinSmem<K, MODE>::SPLIT && al < 0) emit_nobase<K, MODE>(a, sm, key, val & ~AL_MASK);   // a record of one SNP
        else emit<K, MODE>(a, sm, key, val);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if constexpr (BASEQ) { bq.w_base += (uint32_t)__popcll(__ballot(st)); bq.w_masked += (uint32_t)__popcll(__ballot(mk)); }
    pr_n = 0;
}

// read x SNP join, SNP-major: the 64 reads of a wave are (in a sorted BAM) a narrow position range, so the wave walks the few
// SNPs of that range TOGETHER - position of SNP k is wave-uniform, every lane only asks "inside my read?" - instead of every
// read searching the SNP table for itself (two or three binary searches per read, most of them to learn that a 91-base read
// covers no SNP).  A hit parks its (SNP, query offset) pair in the wave's LDS segment; the bases of the parked pairs are
// fetched together later (drain: one HBM latency per batch, not per hit).  i = the read's index in its batch; pr_n = parked
// pairs of this wave, wave-uniform state that lives across the sweeps; last_sweep: drain what is parked and walk the tile's
// set-aside reads.  Returns the (read, SNP) pairs of this lane.
template <class K, int MODE, bool BASEQ>
__device__ __forceinline__ uint32_t pileup_sweep(const JoinArgs<K>& a, const BatchDesc& d, JoinSmem<K, MODE>& sm, const ReadInfo& r, const RawRead& cur,
                                                 const int i, int& pr_n, const bool last_sweep, BqCount& bq) {
    const int tid = threadIdx.x, wb = tid & ~63;
    uint32_t c = 0, n_gap = 0;
    // reads whose reference span is ONE aligned block (no N / D; 85 % of a 10x run) take the wave-uniform walk below; the
    // others are set aside in LDS and walked together after the last sweep (pileup_complex)
    const bool simple = r.ok && r.span_is_cigar && r.endpos - r.pos == r.n_al;
    const unsigned long long cxm = __ballot(r.ok && !simple);
    if (cxm) {
        uint32_t base = 0;
        if ((tid & 63) == 0) base = atomicAdd(&sm.cx_n, (uint32_t)__popcll(cxm));
        base = __builtin_amdgcn_readfirstlane(base);
        if (r.ok && !simple) {
            const uint32_t u = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(cxm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cxm, 0u));
            if (u < (uint32_t)JoinSmem<K, MODE>::CXCAP) {
                sm.cx_pos[u] = r.pos; sm.cx_end[u] = r.endpos; sm.cx_c0[u] = r.c0; sm.cx_c1[u] = r.c1; sm.cx_cell[u] = r.cell; sm.cx_umi[u] = r.umi;
                sm.cx_s0[u] = cur.s0; sm.cx_sl[u] = cur.s1 - cur.s0; sm.cx_idx[u] = i;
            } else n_gap += pileup_complex<K, MODE, BASEQ>(a, d, sm, r.pos, r.endpos, r.c0, r.c1, r.cell, r.umi, cur.s0, cur.s1 - cur.s0, i, bq);   // list full: walk it here
        }
    }
    if (__ballot(simple)) {                                         // wave-uniform
        // first SNP to look at: the 1 kb window of the wave's first read (lane 0 exists whenever any lane does); a read
        // left of it means unsorted input - then the contig's SNPs are walked from the start (speed, never correctness)
        const int32_t p_w = __builtin_amdgcn_readfirstlane(cur.pos);
        int32_t k;
        if (__ballot(simple && r.pos < p_w)) k = d.n_swin > 0 ? as_global(d.snp_win)[0] : d.snp_end;
        else { const int32_t w = max(p_w, 0) >> WSS;
               k = w >= d.n_swin ? d.snp_end : ((uint32_t)(w - sm.w0) < (uint32_t)sm.nw ? sm.st_w[w - sm.w0] : as_global(d.snp_win)[w]); }
        k = __builtin_amdgcn_readfirstlane(k);
        for (; k < d.snp_end; k++) {
            const int32_t p = __builtin_amdgcn_readfirstlane(snp_p0<K, MODE>(a, sm, k));
            const bool reach = simple && p < r.endpos;
            if (!__ballot(reach)) break;                            // SNPs are sorted: no read of the wave reaches this or any later one
            const bool hit = reach && p >= r.pos;
            const unsigned long long am = __ballot(hit);
            if (!am) continue;
            int32_t qi = p - r.pos;                                 // one aligned op: query offset = reference offset
            if (hit && r.c1 - r.c0 != 1) {                          // I / S / H / P around the aligned blocks shift the query offset
                int32_t rp = r.pos, q = 0;
                for (uint32_t cc = r.c0; cc < r.c1; cc++) {
                    const uint32_t w = cig_at(a, d, sm, cc); const uint32_t op = w & 15u; const int32_t l = int32_t(w >> 4);
                    if (op_aligned(op)) { if (p < rp + l) { qi = q + (p - rp); break; } rp += l; q += l; }
                    else if (op == 1u || op == 4u) q += l;
                }
            }
            const int n_new = __popcll(am);
            if (pr_n + n_new > 64) drain<K, MODE, BASEQ>(a, d, sm, pr_n, bq);
            if (hit) {
                const int u = wb + pr_n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(am >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)am, 0u));
                sm.pk_k[u] = k; sm.pk_qi[u] = qi; sm.pk_cell[u] = r.cell; sm.pk_umi[u] = r.umi; sm.pk_s0[u] = cur.s0; sm.pk_sl[u] = cur.s1 - cur.s0; sm.pk_idx[u] = i;
                c++;
            }
            pr_n += n_new;
        }
    }
    if (last_sweep) {
        if (pr_n) drain<K, MODE, BASEQ>(a, d, sm, pr_n, bq);
        // the set-aside reads of the whole tile, one per thread: full waves of long walks instead of one long walk per wave and sweep
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const uint32_t cx_n = min(sm.cx_n, (uint32_t)JoinSmem<K, MODE>::CXCAP);
        for (uint32_t u = tid; u < cx_n; u += JOIN_BLOCK)
            n_gap += pileup_complex<K, MODE, BASEQ>(a, d, sm, sm.cx_pos[u], sm.cx_end[u], sm.cx_c0[u], sm.cx_c1[u], sm.cx_cell[u], sm.cx_umi[u], sm.cx_s0[u], sm.cx_sl[u], sm.cx_idx[u], bq);
    }
    return c + n_gap;
}

// ---- the pieces of k_join around the sweeps ----
// Staging: the empty set / queues, the tile's facts (m: its record from k_tile_meta), its CIGAR run and its slice of the region /
// SNP tables go to LDS.  Every global load is issued BEFORE the first LDS store: written as load/store loops the compiler waits
// (s_waitcnt vmcnt(0)) inside each iteration, which serialised ~7 HBM round trips per tile.  u_lb: the first staged region, a scalar.
template <class K, int MODE>
__device__ __forceinline__ void stage_tile(const JoinArgs<K>& a, const BatchDesc& d, JoinSmem<K, MODE>& sm, const TileMeta& m, const int32_t u_lb) {
    const int tid = threadIdx.x;
    const uint32_t c_lo = m.c_lo, cg_n = m.cg_n;
    const int32_t w0 = m.w0, nw = m.nw, e0 = m.e0, n_ent = m.n_ent, k0 = m.k0, nk = m.nk;
    if constexpr (JoinSmem<K, MODE>::USE_SET) {
        unsigned long long* set = sm.hkeys();                         // all ones = empty
        for (int s = tid; s < JoinSmem<K, MODE>::SLOTS; s += JOIN_BLOCK) set[s] = ~0ull;
    }
    if (tid == 0) { sm.count = 0; sm.ncount = 0; sm.cx_n = 0; sm.cg_lo = c_lo; sm.cg_n = cg_n; sm.cg_all = m.pad; sm.k0 = k0; sm.nk = nk;
                    if (MODE == XCK_MODE_BASEFC) { sm.w0 = e0; sm.nw = n_ent; } else { sm.w0 = w0; sm.nw = nw; } }
    static_assert(ST_CAP <= JOIN_BLOCK && ST_WIN + 1 <= JOIN_BLOCK, "staging assumes one element per thread");
    constexpr int CG_IT = (CigCap<MODE>::value + JOIN_BLOCK - 1) / JOIN_BLOCK;
    uint32_t cw[CG_IT];
    const uint32_t u_clo = __builtin_amdgcn_readfirstlane(c_lo);      // (scalar starts: the loads below take base + start from SGPRs, like fetch_read)
#pragma unroll
    for (int q = 0; q < CG_IT; q++) { const uint32_t c = tid + q * JOIN_BLOCK; cw[q] = c < cg_n ? (as_global(d.cigar) + u_clo)[c] : 0u; }
    int32_t g_a = 0, g_b = 0, g_c = 0, g_w = 0;
    if (MODE == XCK_MODE_BASEFC) {
        if (tid < n_ent) { g_a = (as_global(a.reg_s0) + u_lb)[(uint32_t)tid]; g_b = (as_global(a.reg_e0) + u_lb)[(uint32_t)tid]; g_c = (as_global(a.reg_row) + u_lb)[(uint32_t)tid]; }
    } else {
        const int32_t u_k0 = __builtin_amdgcn_readfirstlane(k0), u_w0 = __builtin_amdgcn_readfirstlane(w0);
        if (tid < nk) g_a = (as_global(a.snp_p0) + u_k0)[(uint32_t)tid];
        if (tid < nw) g_w = (as_global(d.snp_win) + u_w0)[(uint32_t)tid];   // first SNP of each window
    }
#pragma unroll
    for (int q = 0; q < CG_IT; q++) { const uint32_t c = tid + q * JOIN_BLOCK; if (c < cg_n) sm.cig[c] = cw[q]; }
    if (MODE == XCK_MODE_BASEFC) {
        if (tid < n_ent) { sm.st_a[tid] = g_a; sm.st_b[tid] = g_b; sm.st_c[tid] = g_c; }
    } else {
        if (tid < nk) sm.st_a[tid] = g_a;
        if (tid < nw) sm.st_w[tid] = g_w;
    }
}

// The tile's totals, one atomic each per block on the shard cursor's cache line (a single shared word serialises at ~90 atomics/us):
// acc = accepted (read, region|SNP) pairs before the LDS de-duplication, the algorithmic unit of the join; uor = OR of the UMI codes of
// the accepted reads (highest UMI-code bit in use: the radix-sort fold drops the dead bits between the UMI codes and the cell field)
template <class K, int MODE>
__device__ __forceinline__ void publish_tile_totals(const JoinArgs<K>& a, JoinSmem<K, MODE>& sm, uint32_t acc, unsigned long long uor) {
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) acc += __shfl_xor(acc, dd, 64);
    {
        uint32_t ulo = (uint32_t)uor, uhi = (uint32_t)(uor >> 32);
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) { ulo |= __shfl_xor(ulo, dd, 64); uhi |= __shfl_xor(uhi, dd, 64); }
        if (lane == 0) { sm.wuor[2 * (tid >> 6)] = ulo; sm.wuor[2 * (tid >> 6) + 1] = uhi; }
    }
    if (lane == 0) sm.wcnt[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        uor = 0;
#pragma unroll
        for (int w = 0; w < JOIN_BLOCK / 64; w++) uor |= ((unsigned long long)sm.wuor[2 * w + 1] << 32) | sm.wuor[2 * w];
        if (uor) atomicOr(&a.ctl[ctl_umi_or(JOIN_SHARD)], uor);
    }
    if (tid == 0) { acc = sm.wcnt[0] + sm.wcnt[1] + sm.wcnt[2] + sm.wcnt[3];
                    if (acc) atomicAdd(&a.ctl[ctl_accepted(JOIN_SHARD)], (unsigned long long)acc); }
}

// The BASEQ kernels' pair counts (xck_get_baseq_stats): the waves' counts join the set-aside reads' in LDS, then one atomic each per block
// that has any, on words of the shard's `accepted` cache line in device memory - rewound with it when a launch is replayed, so a replayed tile counts once.
template <class K, int MODE>
__device__ __forceinline__ void publish_baseq(const JoinArgs<K>& a, JoinSmem<K, MODE>& sm, const BqCount& bq) {
    if ((threadIdx.x & 63) == 0) { if (bq.w_base) atomicAdd(bq_lds_base(sm), bq.w_base); if (bq.w_masked) atomicAdd(bq_lds_masked(sm), bq.w_masked); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t nb = *bq_lds_base(sm), nm = *bq_lds_masked(sm);
        if (nb) atomicAdd(&a.ctl[ctl_bq_base(JOIN_SHARD)], (unsigned long long)nb);
        if (nm) atomicAdd(&a.ctl[ctl_bq_masked(JOIN_SHARD)], (unsigned long long)nm);
    }
}

// (64-bit pileup: asked to stay at 80 VGPRs, i.e. 6 waves per SIMD beside its 26.5 KB of LDS; the others have room anyway, and the
// 128-bit pileup kernel would spill under that bound)
// BASEQ (pileup only): the instantiation of a handle with a base-quality floor; the default one holds no trace of it
template <class K, int MODE, bool BASEQ = false>
__global__ __launch_bounds__(JOIN_BLOCK) __attribute__((amdgpu_waves_per_eu((sizeof(K) == 8 && MODE == XCK_MODE_BAF) ? 6 : 4, 8))) void k_join(JoinArgs<K> a) {
    __shared__ JoinSmem<K, MODE> sm;
    const int tid = threadIdx.x;
    StampRec t_s0;
#if XCK_STAMPS
    for (int q = 0; q < 12; q++) t_s0.d[q] = 0;
    t_s0.t = clock64();
#endif
#define STAMP(slot) XCK_STAMP(&t_s0, slot)
    // ---- prologue: one record from k_tile_meta, then ONE round of independent loads ----
    const XCK_GLOBAL TileMeta* mp = as_global(a.meta) + blockIdx.x;
    const TileMeta m = { mp->c_lo, mp->cg_n, mp->w0, mp->nw, mp->e0, mp->n_ent, mp->k0, mp->nk, mp->b, mp->r0, 0, mp->pad };
    const int b = __builtin_amdgcn_readfirstlane(m.b);
    const int tile0 = __builtin_amdgcn_readfirstlane(m.r0);
    const BatchDesc& d = a.bt.desc[b];                                // kernarg: scalar loads through the constant cache
    const int32_t u_lb = __builtin_amdgcn_readfirstlane(m.e0), u_nst = __builtin_amdgcn_readfirstlane(m.n_ent), u_p0 = __builtin_amdgcn_readfirstlane(m.k0);   // basefc: the tile's region slice as scalars
    STAMP(0);
    RawRead W[TILE_ITEMS];
    if (__builtin_amdgcn_readfirstlane(tile0 + TILE <= d.n)) {        // a full tile (all but the last of a batch): no per-lane bounds
#pragma unroll
        for (int j = 0; j < TILE_ITEMS; j++) W[j] = fetch_read<MODE == XCK_MODE_BAF>(d, tile0, (uint32_t)(j * JOIN_BLOCK + tid), true);
    } else {
#pragma unroll
        for (int j = 0; j < TILE_ITEMS; j++) W[j] = fetch_read<MODE == XCK_MODE_BAF>(d, tile0, (uint32_t)(j * JOIN_BLOCK + tid), tile0 + j * JOIN_BLOCK + tid < d.n);
    }                                                                 // the whole tile's loads fly during the staging
    stage_tile<K, MODE>(a, d, sm, m, u_lb);
    if constexpr (BASEQ) { if (tid == 0) { *bq_lds_base(sm) = 0; *bq_lds_masked(sm) = 0; } }
    STAMP(1);
    __syncthreads();
    STAMP(2);
    // ---- TILE_ITEMS coalesced sweeps over the tile (the reads were requested in the prologue) ----
    uint32_t acc = 0;
    unsigned long long uor = 0;
    int pr_n = 0;                                                     // pileup: parked pairs of this wave (wave-uniform)
    BqCount bq;                                                       // BASEQ: this lane's pairs with a base / masked
    // sweeps between two flushes: keep the expected fill (256 reads x ~2 pairs per sweep) under half the set / queue
    constexpr int CAP_ENTRIES = JoinSmem<K, MODE>::USE_SET ? JoinSmem<K, MODE>::SLOTS : JoinSmem<K, MODE>::QCAP;
    // set mode: the de-duplicated fill of a 1024-read tile is a few hundred keys, so flush once, at the end
    // (better de-duplication, half the cursor atomics); saturation still spills correctly through append_one()
#ifndef XCK_SET_FLUSH_EVERY
#define XCK_SET_FLUSH_EVERY TILE_ITEMS
#endif
    constexpr int FLUSH_EVERY = JoinSmem<K, MODE>::USE_SET ? XCK_SET_FLUSH_EVERY : JoinSmem<K, MODE>::SPLIT ? TILE_ITEMS
                              : ((CAP_ENTRIES / 2 / (JOIN_BLOCK * 2)) < 1 ? 1 : (CAP_ENTRIES / 2 / (JOIN_BLOCK * 2)));
#pragma unroll
    for (int j = 0; j < TILE_ITEMS; j++) {
        const ReadInfo r = load_read<K, MODE>(a, d, sm, W[j]);
#if XCK_STAMPS == 2
        if (j == 0) { uint32_t x_ = (uint32_t)r.endpos ^ (uint32_t)r.n_al; asm volatile("" :: "v"(x_)); STAMP(3); }   // (the summary is complete)
#endif
        if (r.ok) uor |= r.umi;                                       // (finish() puts the haplotype class of the region-level keys into UMI-field bits no code uses)
        // wave-uniform calls: the walk over the regions / SNPs is shared by all 64 lanes
        if constexpr (MODE == XCK_MODE_BAF) acc += pileup_sweep<K, MODE, BASEQ>(a, d, sm, r, W[j], tile0 + j * JOIN_BLOCK + tid, pr_n, j + 1 == TILE_ITEMS, bq);
        else acc += join_regions<K, MODE>(a, d, sm, r, u_lb, u_nst, u_p0, &t_s0, j);
        // Flush points are fixed at compile time, never decided from sm.count: a count-based decision read
        // after the barrier races with the next sweep's inserts (threads could disagree and split at the
        // barriers inside flush()).  A set / queue that saturates between two flush points spills through
        // append_one(), which is always correct.
#if XCK_STAMPS == 2
        if (j == 0) STAMP(5); else STAMP(6);                          // sweep 0 in three parts (3 read summary, 4 chunk scan, 5 candidates), 6 = sweeps 1-3
#else
        STAMP(3 + j);
#endif
        if ((j + 1) % FLUSH_EVERY == 0 || j + 1 == TILE_ITEMS) {
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // LDS only: global prefetches stay in flight
            STAMP(7);
            if constexpr (JoinSmem<K, MODE>::SPLIT) flush_split<K, MODE>(a, sm, &t_s0); else flush<K, MODE>(a, sm, &t_s0);
        }
    }
    publish_tile_totals<K, MODE>(a, sm, acc, uor);
    if constexpr (BASEQ) publish_baseq<K, MODE>(a, sm, bq);
#if XCK_STAMPS != 2
    STAMP(11);
#endif
#if XCK_STAMPS
    if (tid == 0) { uint32_t* o = (uint32_t*)(a.meta + blockIdx.x); for (int q = 0; q < 12; q++) o[q] = t_s0.d[q]; }
    static_assert(sizeof(TileMeta) == 48, "the stamp record reuses the tile record");
#endif
}

// ------------------------------------------------------------------------------------------
// host side: the tables the join reads and its launch
// ------------------------------------------------------------------------------------------
template <class T> static int dev_upload(EngineImpl* im, T** dptr, const std::vector<T>& h) {
    size_t n = std::max<size_t>(h.size(), 1);
    HIP_TRY(hipMalloc((void**)dptr, n * sizeof(T)));
    if (!h.empty()) HIP_TRY(hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

int build_tables(EngineImpl* im, const xck_config* cfg) {
    const int nc = cfg->n_contigs;
    im->ctab.assign(std::max(nc, 1), ContigTab());
    std::vector<int32_t> reg_s0, reg_e0, reg_row, reg_pmax;
    std::vector<int32_t> snp_p0, snp_win, csr_off, csr_reg;
    std::vector<uint32_t> snp_info;
    if (im->mode == XCK_MODE_BASEFC) {
        // regions valid for fetch(): pysam raises (-> region silently gets 0, utils/sam.py:105-118)
        // when start-1 < 0 or start-1 > end.
        std::vector<int32_t> base, count;
        sort_regions_by_contig(cfg->regions, cfg->n_regions, nc, [](const xck_region& r) { return !(r.start < 1 || (int64_t)r.start - 1 > (int64_t)r.end); },
                               [](const xck_region& r) { return r.start - 1; }, reg_s0, reg_e0, reg_row, reg_pmax, base, count);
        for (int c = 0; c < nc; c++) { im->ctab[c].reg_base = base[c]; im->ctab[c].n_reg = count[c]; }
    } else {
        std::vector<std::vector<int32_t>> by_c(nc);
        for (int s = 0; s < cfg->n_snps; s++) {
            const xck_snp& x = cfg->snps[s];
            if (x.contig < 0 || x.contig >= nc || x.pos < 1) continue;   // fetch(pos-1 < 0) raises -> no reads
            by_c[x.contig].push_back(s);
        }
        // regions per contig sorted by start for the SNP -> region join (baf/fc/main.py:92-101)
        std::vector<std::vector<int32_t>> reg_c(nc);
        for (int g = 0; g < cfg->n_regions; g++) { const xck_region& r = cfg->regions[g]; if (r.contig >= 0 && r.contig < nc) reg_c[r.contig].push_back(g); }
        std::vector<uint64_t> excl;                                       // (snp index << 32 | region index), sorted
        for (int i = 0; i < cfg->n_excl_pairs; i++) excl.push_back(((uint64_t)(uint32_t)cfg->excl_snp[i] << 32) | (uint32_t)cfg->excl_region[i]);
        std::sort(excl.begin(), excl.end());
        double ms_csr = 0;                                               // XCK_DEBUG_TIMING: the SNP -> region loop alone (refold.h builds the same relation on the device)
        csr_off.push_back(0);
        for (int c = 0; c < nc; c++) {
            auto& v = by_c[c];
            std::sort(v.begin(), v.end(), [&](int32_t a, int32_t b) {
                if (cfg->snps[a].pos != cfg->snps[b].pos) return cfg->snps[a].pos < cfg->snps[b].pos; return a < b; });
            ContigTab& t = im->ctab[c];
            t.snp_base = (int32_t)snp_p0.size(); t.n_snp = (int32_t)v.size();
            for (int32_t s : v) {
                const xck_snp& x = cfg->snps[s];
                snp_p0.push_back(x.pos - 1);
                snp_info.push_back(snp_info_word(x));
            }
            int32_t max_p = v.empty() ? 0 : cfg->snps[v.back()].pos;
            t.n_swin = v.empty() ? 0 : (max_p >> WSS) + 1;
            t.swin_base = (int32_t)snp_win.size();
            { int32_t k = 0; for (int32_t w = 0; w < t.n_swin; w++) { while (k < t.n_snp && snp_p0[t.snp_base + k] < (w << WSS)) k++; snp_win.push_back(t.snp_base + k); } }
            // SNP -> regions: start <= pos <= end_incl; rows ascending so keys stay deterministic
            // (minus the caller's exclusion pairs: SNPs that local phasing removed from one region's list)
            const auto t_csr = std::chrono::steady_clock::now();
            std::vector<std::vector<int32_t>> hits(t.n_snp);
            for (int32_t g : reg_c[c]) {
                const xck_region& r = cfg->regions[g];
                if (r.end < r.start) continue;
                auto lo = std::lower_bound(snp_p0.begin() + t.snp_base, snp_p0.begin() + t.snp_base + t.n_snp, r.start - 1);
                for (auto it = lo; it != snp_p0.begin() + t.snp_base + t.n_snp && *it <= r.end - 1; ++it) {
                    const size_t k = (size_t)((it - snp_p0.begin()) - t.snp_base);
                    if (!excl.empty() && std::binary_search(excl.begin(), excl.end(), ((uint64_t)(uint32_t)v[k] << 32) | (uint32_t)g)) continue;
                    hits[k].push_back(g);
                }
            }
            for (int32_t k = 0; k < t.n_snp; k++) { std::sort(hits[k].begin(), hits[k].end()); for (int32_t g : hits[k]) csr_reg.push_back(g); csr_off.push_back((int32_t)csr_reg.size()); }
            ms_csr += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_csr).count();
        }
        if (im->eng->knobs.debug_timing) fprintf(stderr, "[xck] create: host SNP -> region CSR loop %.3f ms (%d SNPs, %d regions, %zu pairs)\n", ms_csr, cfg->n_snps, cfg->n_regions, csr_reg.size());
        im->n_snps_sorted = (int)snp_p0.size();
        // sorted SNP -> the caller's index: the per-SNP summary answers in the caller's order, and xck_refold takes its tables in it
        for (int c = 0; c < nc; c++) im->snp_perm.insert(im->snp_perm.end(), by_c[c].begin(), by_c[c].end());
        im->n_snps_in = cfg->n_snps;
        im->snps_in.assign(cfg->snps, cfg->snps + cfg->n_snps);
        im->csr_reg_cap_bytes = std::max<size_t>(csr_reg.size(), 1) * sizeof(int32_t);
        if (cfg->flags & XCK_F_FEATURE_SUMMARY) { im->h_csr_off = csr_off; im->h_csr_reg = csr_reg; }
    }
    int rc;
    if ((rc = dev_upload(im, &im->d_reg_s0, reg_s0))) return rc;
    if ((rc = dev_upload(im, &im->d_reg_e0, reg_e0))) return rc;
    if ((rc = dev_upload(im, &im->d_reg_row, reg_row))) return rc;
    if ((rc = dev_upload(im, &im->d_reg_pmax, reg_pmax))) return rc;
    if ((rc = dev_upload(im, &im->d_snp_p0, snp_p0))) return rc;
    if ((rc = dev_upload(im, &im->d_snp_win, snp_win))) return rc;
    if ((rc = dev_upload(im, &im->d_snp_info, snp_info))) return rc;
    if ((rc = dev_upload(im, &im->d_csr_off, csr_off))) return rc;
    if ((rc = dev_upload(im, &im->d_csr_reg, csr_reg))) return rc;
    if (im->mode == XCK_MODE_BAF) {
        size_t n = std::max<size_t>((size_t)im->n_snps_sorted * 5, 1);
        HIP_TRY(hipMalloc((void**)&im->d_tally, n * sizeof(uint32_t)));
    }
    return 0;
}

// The batches in im->inflight as the table a kernel takes, each with its first tile in the fused grid (TILE reads a tile): the one
// numbering the join and every pass behind it use.  -> tiles = blocks of the launch
static int32_t fill_batch_table(const EngineImpl* im, BatchTable& bt) {
    const int nb = (int)im->inflight.size();
    int32_t tiles = 0;
    for (int i = 0; i < nb; i++) { bt.desc[i] = im->inflight[i]; bt.desc[i].tile0 = tiles; tiles += (im->inflight[i].n + TILE - 1) / TILE; }
    bt.n_batches = nb; bt.n_tiles = tiles;
    return tiles;
}

// launch ONE fused join kernel over every batch in im->inflight
template <class K>
static int launch_join_t(EngineImpl* im) {
    JoinArgs<K> a;
    const int32_t tiles = fill_batch_table(im, a.bt);
    if (const int rc = grow_device(im, (void**)&im->d_meta, &im->meta_cap, (size_t)tiles * sizeof(TileMeta), (size_t)(tiles / 2 + 1024) * sizeof(TileMeta))) return rc;
    a.meta = im->d_meta; a.f = im->rf;
    a.reg_s0 = im->d_reg_s0; a.reg_e0 = im->d_reg_e0; a.reg_row = im->d_reg_row; a.reg_pmax = im->d_reg_pmax;
    a.snp_p0 = im->d_snp_p0;
    a.kl.ubits = im->ubits; a.kl.cbits = im->cbits;
    a.keys = (K*)im->d_keys; a.vals = im->d_vals; a.cap = im->hit_cap; a.ctl = im->d_ctl;
    a.nkeys = (K*)im->d_nkeys; a.nvals = im->d_nvals;
    a.min_baseq = im->min_baseq;
    dim3 grid(tiles), block(JOIN_BLOCK);
    clear_stale_error("launch_join", im->eng->knobs.debug_timing);
    HIP_TRY(hipEventRecord(im->ev0, im->s_comp));
    const dim3 mgrid((tiles + 255) / 256), mblock(256);
    if (im->mode == XCK_MODE_BASEFC) {
        hipLaunchKernelGGL((k_tile_meta<XCK_MODE_BASEFC>), mgrid, mblock, 0, im->s_comp, a.bt, im->d_meta, (const int32_t*)im->d_reg_pmax);
        hipLaunchKernelGGL((k_join<K, XCK_MODE_BASEFC>), grid, block, 0, im->s_comp, a);
    } else {
        hipLaunchKernelGGL((k_tile_meta<XCK_MODE_BAF>), mgrid, mblock, 0, im->s_comp, a.bt, im->d_meta, (const int32_t*)nullptr);
        if (im->min_baseq > 0) hipLaunchKernelGGL((k_join<K, XCK_MODE_BAF, true>), grid, block, 0, im->s_comp, a);
        else hipLaunchKernelGGL((k_join<K, XCK_MODE_BAF>), grid, block, 0, im->s_comp, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(im->ev1, im->s_comp));
    publish_words(im, im->d_ctl, im->d_hctl, CTL_WORDS, 256);
    HIP_TRY(hipGetLastError());
    return 0;
}
int launch_join(EngineImpl* im) { return im->key_bits == 64 ? launch_join_t<uint64_t>(im) : launch_join_t<u128>(im); }

#include "cell_summary.h"
#include "read_fate.h"
#include "feature_summary.h"
#include "base_tally.h"
#include "ref_seq.h"

// What the pipeline (pipeline.hip) knows of the summaries and the base tally: their memory at create, their zeroing at reset (on s_comp, in front
// of the reset's synchronise), and their passes behind the FIRST join launch of a queue (each returns at once when its flag is off).
int summaries_init(EngineImpl* im, uint32_t flags) {
    if (flags & XCK_F_READ_FATE) { if (const int rc = read_fate_init(im)) return rc; }
    if (flags & XCK_F_CELL_SUMMARY) { if (const int rc = cell_summary_init(im)) return rc; }
    if (flags & XCK_F_FEATURE_SUMMARY) { if (const int rc = feature_summary_init(im)) return rc; }
    if ((flags & XCK_F_BASE_TALLY) && im->mode == XCK_MODE_BAF) { if (const int rc = base_tally_init(im)) return rc; }
    return 0;
}
int summaries_reset(EngineImpl* im) {
    if (im->d_fate) { if (const int rc = read_fate_reset(im)) return rc; }
    if (const int rc = cell_summary_reset(im)) return rc;
    if (im->d_feat) { if (const int rc = feature_summary_reset(im)) return rc; }
    if (im->base_tally) { if (const int rc = base_tally_reset(im)) return rc; }
    return 0;
}
int launch_summaries(EngineImpl* im) {
    if (const int rc = launch_read_fate(im)) return rc;
    if (const int rc = launch_feature_fate(im)) return rc;
    return launch_base_tally(im);
}

// XCK_STAMPS builds: the stamp records of the join launch that has just been waited for (ms: its time), summed per slot
int join_stamps_collect(EngineImpl* im, float ms) {
#if XCK_STAMPS
    { int32_t tiles = 0; for (auto& b : im->inflight) tiles += (b.n + TILE - 1) / TILE;
      std::vector<uint32_t> h((size_t)tiles * 12);
      HIP_TRY(hipMemcpy(h.data(), im->d_meta, h.size() * 4, hipMemcpyDeviceToHost));
      for (int q = 0; q < 12; q++) im->stamp_sum[q] = 0;
      for (size_t t = 0; t < (size_t)tiles; t++) for (int q = 0; q < 12; q++) im->stamp_sum[q] += h[t * 12 + q];
      im->stamp_tiles = tiles; im->stamp_ms = ms; }
#endif
    return 0;
}
// ... and their table (finish_t() prints it; compiled out by default)
void join_stamps_report(const EngineImpl* im) {
#if XCK_STAMPS
    { static const char* nm[12] = {"record", "prologue", "stage_barrier", "sweep0", "sweep1", "sweep2", "sweep3", "flush_barrier", "flush_count", "flush_cursor", "flush_stores", "tail"};
      unsigned long long tot = 0; for (int q = 0; q < 12; q++) tot += im->stamp_sum[q];
      fprintf(stderr, "[stamps mode=%d] last join launch: %d tiles, %.3f ms; cycles of wave 0 per tile (share of the block's life):", im->mode, im->stamp_tiles, im->stamp_ms);
      for (int q = 0; q < 12; q++) fprintf(stderr, " %s=%.0f (%.1f%%)", nm[q], (double)im->stamp_sum[q] / std::max(1, im->stamp_tiles), 100.0 * im->stamp_sum[q] / std::max(1ull, tot));
      fprintf(stderr, " | total=%.0f\n", (double)tot / std::max(1, im->stamp_tiles)); }
#endif
}

}  // namespace xck
