// finish.hip - MI355X (gfx950) counting engine: the finish side.  Folds the hits that the join kernels (engine.hip) appended to the
// shard slices into the COO matrices and hands them to the host.
//
//   finish      : basefc: the partition fold of fold_partition.h (no sort); fallback: radix sort (rocPRIM) over the (row, cell) bits,
//                 k_fold_heads / k_fold_emit_unsorted (distinct UMIs of a run told apart by an LDS hash set) straight into COO.
//                 pileup: hits with a base sorted by row partition + LDS radix sort per item (fold_partition.h; fallback: rocPRIM),
//                 k_first_base (first read per key, SNP-mask filter laid out along the sorted stream; k_first_long for runs longer
//                 than 64), k_claim (gap records that hold a key earlier in fetch order), k_tally_rows, k_expand (per-SNP filters,
//                 SNP -> region fan-out), region-level hits partitioned again and classified per item by an LDS hash set
//                 (k_hap_items; fallback: sort + k_hap_class / k_hap_sum), k_hap_count / k_hap_scatter (AD / DP / OTH -> COO);
//                 128-bit keys: k_first_read and the sorted path.  XCK_F_UMI_CONSENSUS: a vote per key instead of the first read and no
//                 claims (umi_consensus.h: k_consensus_base / k_consensus_read / k_consensus_long, the agreement counters).  XCK_F_UNIQUE_FEATURE (basefc): the keys grouped by
//                 molecule first and those of the molecules on two or more rows removed (umi_feature.h), then the radix-sort fold.  XCK_F_UMI_COLLAPSE (basefc): one key per connected component of the 1-mismatch graph of every (row, cell) (umi_collapse.h), counted by fold_coo.  xck_refold (refold.h) runs the half behind k_tally_rows again; with a
//                 cell mask: k_row_bounds, k_tally_rows_cells / k_tally_long_cells (tallies of the enabled cells), k_expand<MASK>.
//   snp_counts  : the SNP x cell matrices of the finished pileup from the molecule stage alone (snp_counts.h).
//   group_counts: the row x group sums of the result blocks or of the SNP x cell blocks under a cell -> group mapping (group_counts.h).
//                 The host steps the two calls share are coo_call.h's.  Copy-out (deliver_words) on the copy stream (xck_finish_async).
//
// Integer / byte work only - HBM-bound, no MFMA.  See DESIGN.md for layouts, byte counts and measurements.
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <type_traits>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include "engine_impl.h"

namespace xck {
// control words -> the host's mapped pinned mirror (engine_impl.h publish_words: the one copy of this kernel, for all three units)
static __global__ void k_publish(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ host_alias, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) host_alias[i] = src[i];
}
void publish_words(EngineImpl* im, const unsigned long long* src, unsigned long long* host_alias, int n, int threads) {
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(threads), 0, im->s_comp, src, host_alias, n);
}
// ... and waited for: control words [at, at + n) as the compute stream leaves them, h = their place in the host mirror.  Also reports
// a failed launch of the kernels queued just before.
static int read_ctl_words(EngineImpl* im, int at, int n, const unsigned long long*& h) {
    publish_words(im, im->d_ctl + at, im->d_hctl + at, n, n > 64 ? 256 : 64);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(im->s_comp));
    h = im->h_ctl + at;
    return 0;
}

template <class K> static KeyLayout<K> key_layout(const EngineImpl* im) { KeyLayout<K> kl; kl.ubits = im->ubits; kl.cbits = im->cbits; return kl; }
// first packed index of every shard slice holding cnt[shard] entries
static ShardSpan shard_span(const unsigned long long* cnt) {
    ShardSpan sp; sp.start[0] = 0;
    for (int sh = 0; sh < NSHARD; sh++) sp.start[sh + 1] = sp.start[sh] + cnt[sh];
    return sp;
}

// exclusive scan of one uint32 per thread over a 256-thread block; returns block total in `total`
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_wave, uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { uint32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t base = 0; total = 0;
#pragma unroll
    for (int w = 0; w < JOIN_BLOCK / 64; w++) { uint32_t t = s_wave[w]; if (w < wave) base += t; total += t; }
    __syncthreads();
    return base + inc - v;
}

// ------------------------------------------------------------------------------------------
// finish kernels
// ------------------------------------------------------------------------------------------
// basefc fold without a dense intermediate: pass A counts the (row, cell) run heads of every 2048-key tile,
// a one-block scan turns that into output offsets, pass B writes (row, col, #distinct keys of the run)
// straight into the COO arrays.  Heads walk their run (runs average ~2 keys; the walk stays in L2).
constexpr int FD_BLOCK = 256, FD_ITEMS = 8, FD_TILE = FD_BLOCK * FD_ITEMS;

template <class K>
__global__ __launch_bounds__(FD_BLOCK) void k_fold_heads(const K* __restrict__ k, long long n, KeyLayout<K> kl, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_wave[FD_BLOCK / 64];
    const long long base = (long long)blockIdx.x * FD_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int t = 0; t < FD_ITEMS; t++) {                                  // striped: lane-contiguous, fully coalesced
        const long long i = base + t * FD_BLOCK + threadIdx.x;
        if (i < n) { if (i == 0 || kl.rc(k[i]) != kl.rc(k[i - 1])) c++; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

template <class K>
__global__ __launch_bounds__(FD_BLOCK) void k_fold_emit(const K* __restrict__ k, long long n, KeyLayout<K> kl, const unsigned long long* __restrict__ off,
                                                        int32_t* __restrict__ row, int32_t* __restrict__ col, int32_t* __restrict__ val) {
    // val[] is zero on entry.  A tile knows the distinct keys of every (row, cell) run that STARTS in it only up to
    // the tile end; what a later tile holds of that run (its "lead": distinct keys before its first head) is added
    // with one atomicAdd to the slot of the last head before it.  No thread ever walks a run, so a hot (gene, cell)
    // pair with thousands of UMIs costs the same per key as a cold one.
    __shared__ uint32_t s_wave[FD_BLOCK / 64];
    __shared__ K tile[FD_TILE + 1];                                       // tile[0] = key before the tile (halo)
    __shared__ uint16_t s_hx[FD_TILE + 1], s_he[FD_TILE];                 // per head: distinct keys before it / its element
    const long long base = (long long)blockIdx.x * FD_TILE;
    const int n_loc = (int)min((long long)FD_TILE, n - base);
#pragma unroll
    for (int t = 0; t < FD_ITEMS; t++) { const int e = t * FD_BLOCK + threadIdx.x; if (e < n_loc) tile[1 + e] = k[base + e]; }
    if (threadIdx.x == 0) tile[0] = base > 0 ? k[base - 1] : K(0);
    __syncthreads();
    // blocked arrangement: thread t owns elements [t*FD_ITEMS, (t+1)*FD_ITEMS)
    const int e0 = threadIdx.x * FD_ITEMS;
    uint32_t hmask = 0, dmask = 0;
    K prev = tile[e0];
#pragma unroll
    for (int q = 0; q < FD_ITEMS; q++) {
        const int e = e0 + q;
        if (e < n_loc) {
            const K me = tile[1 + e];
            const bool first = base + e == 0;
            if (first || kl.rc(me) != kl.rc(prev)) hmask |= 1u << q;
            if (first || me != prev) dmask |= 1u << q;
            prev = me;
        }
    }
    uint32_t total;
    const uint32_t excl = block_excl_scan((uint32_t)__popc(hmask) | ((uint32_t)__popc(dmask) << 16), s_wave, total);
    const uint32_t n_heads = total & 0xffffu, n_dist = total >> 16;
    uint32_t r = excl & 0xffffu, xd = excl >> 16;
#pragma unroll
    for (int q = 0; q < FD_ITEMS; q++) {
        if (hmask & (1u << q)) { s_hx[r] = (uint16_t)xd; s_he[r] = (uint16_t)(e0 + q); r++; }
        if (dmask & (1u << q)) xd++;
    }
    if (threadIdx.x == 0) s_hx[n_heads] = (uint16_t)n_dist;
    __syncthreads();
    const unsigned long long out = off[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < n_heads; i += FD_BLOCK) {
        const K me = tile[1 + s_he[i]];
        const int32_t cnt = (int32_t)s_hx[i + 1] - (int32_t)s_hx[i];
        const unsigned long long d = out + i;
        row[d] = (int32_t)kl.row(me); col[d] = (int32_t)kl.cell(me);
        if (i + 1 == n_heads) atomicAdd(&val[d], cnt); else val[d] = cnt;  // the last run may continue in later tiles
    }
    if (threadIdx.x == 0) {
        const uint32_t lead = n_heads ? s_hx[0] : n_dist;
        if (lead && out > 0) atomicAdd(&val[out - 1], (int32_t)lead);
    }
}

// Same fold for keys that are sorted by (row, cell) ONLY (the UMI bits were left out of the radix sort: 4 passes instead
// of 7).  Inside a run the UMIs are in arbitrary order, so "distinct" is decided by an LDS hash set: the tile first
// inserts the part of its leading run that lies in earlier tiles (its lead-in, at most FU_LEAD keys), then its own keys -
// a key is counted by the one thread whose compare-and-swap claims the slot.  A key therefore counts in the tile that
// holds its first occurrence and nowhere else.  A run with a longer lead-in raises *giant and the host redoes the fold on
// fully sorted keys.  64-bit keys only.
constexpr int FU_LEAD = 4096, FU_SLOTS = 8192;                           // <= 2048 + 4096 keys in 8192 slots (64 KB, dynamic LDS)
// 1024 threads per tile: the 72 KB of LDS allow two blocks per CU, and with 256-thread blocks the two waves per SIMD could not
// hide the chains of LDS atomics (4.3 ms for 380 M keys; 3.0 ms with 512 threads, 2.8 ms with 1024)
constexpr int FU_BLOCK = 1024, FU_ITEMS = FD_TILE / FU_BLOCK, FU_STRIDE = FU_LEAD / FU_BLOCK;
static_assert(FU_ITEMS * FU_BLOCK == FD_TILE && FU_STRIDE * FU_BLOCK == FU_LEAD && FU_STRIDE <= 64, "lead-in search / sweep layout");
__global__ __launch_bounds__(FU_BLOCK) void k_fold_emit_unsorted(const unsigned long long* __restrict__ k, long long n, KeyLayout<unsigned long long> kl,
                                                                 const unsigned long long* __restrict__ off,
                                                                 int32_t* __restrict__ row, int32_t* __restrict__ col, int32_t* __restrict__ val,
                                                                 unsigned long long* __restrict__ giant, int sub_shift) {
    // sub_shift = lowest key bit the radix sort covered (<= kl.ubits): the sort's whole digits usually reach a few bits into
    // the UMI field, so a (row, cell) run is a sequence of sub-runs by UMI prefix - and only the sub-run of the tile's first
    // key can have keys (hence duplicates) in earlier tiles.  That is what the lead-in covers.
    typedef unsigned long long K;
    extern __shared__ K set[];                                            // FU_SLOTS slots (a tile with a short lead-in uses half)
    __shared__ uint16_t s_hx[FD_TILE + 1], s_he[FD_TILE];                 // per head: distinct keys before it / its element
    __shared__ uint32_t s_wh[FU_BLOCK / 64], s_wd[FU_BLOCK / 64];
    __shared__ long long s_lead;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = (long long)blockIdx.x * FD_TILE;
    const int n_loc = (int)min((long long)FD_TILE, n - base);
    // the tile's own keys (and each key's predecessor) are requested first: the loads fly during the lead-in search and
    // the table set-up.  Wave w owns FD_TILE / 8 consecutive elements in FU_ITEMS coalesced sweeps of 64; element order = (wave, sweep, lane).
    K me[FU_ITEMS], pv[FU_ITEMS];
    const int e_w = wave * (FD_TILE / (FU_BLOCK / 64));
#pragma unroll
    for (int q = 0; q < FU_ITEMS; q++) {
        const int e = e_w + q * 64 + lane;
        me[q] = ~0ull; pv[q] = ~0ull;
        if (e < n_loc) { me[q] = k[base + e]; if (base + e > 0) pv[q] = k[base + e - 1]; }
    }
    const unsigned long long out = off[blockIdx.x];
    // ---- lead-in of the first run: keys of earlier tiles with the (row, cell) of the tile's first key (a suffix of
    //      what precedes the tile).  One coarse probe per thread, FU_STRIDE keys apart, then FU_STRIDE fine ones: two L2 round trips.
    const K rc0 = k[base] >> sub_shift;
    const long long w0 = max(0ll, base - FU_LEAD);
    long long lead0 = base;
    if (base > 0 && (k[base - 1] >> sub_shift) == rc0) {                      // block-uniform
        if (tid == 0) s_lead = base - 1;
        __syncthreads();
        const long long g = base - 1 - (long long)FU_STRIDE * tid;
        if (g >= w0 && (k[g] >> sub_shift) == rc0) atomicMin((unsigned long long*)&s_lead, (unsigned long long)g);
        __syncthreads();
        const long long c = s_lead;                                       // smallest coarse match: the run starts in (c - FU_STRIDE, c]
        __syncthreads();
        if (tid < FU_STRIDE) { const long long g2 = c - tid; if (g2 >= w0 && (k[g2] >> sub_shift) == rc0) atomicMin((unsigned long long*)&s_lead, (unsigned long long)g2); }
        __syncthreads();
        lead0 = s_lead;
        if (tid == 0 && lead0 == w0 && w0 > 0 && (k[w0 - 1] >> sub_shift) == rc0) *giant = 1ull;   // the sub-run starts before the window
    }
    const int slots = ((int)(base - lead0) + n_loc <= 3072) ? FU_SLOTS / 2 : FU_SLOTS;      // block-uniform; load factor <= 0.75
    const uint32_t smask = (uint32_t)slots - 1;
    for (int t = tid; t < slots; t += FU_BLOCK) set[t] = ~0ull;
    __syncthreads();
    auto probe_on = [&](K key, uint32_t slot) -> bool {                  // continue after a first probe that hit another key
        for (;;) {
            slot = (slot + 1) & smask;
            const K prev = atomicCAS(&set[slot], ~0ull, key);
            if (prev == ~0ull) return true;
            if (prev == key) return false;
        }
    };
    for (long long g = lead0 + tid; g < base; g += FU_BLOCK) {
        const K key = k[g]; const uint32_t sl = set_slot<FU_SLOTS>(key) & smask;
        const K prev = atomicCAS(&set[sl], ~0ull, key);
        if (prev != ~0ull && prev != key) (void)probe_on(key, sl);
    }
    __syncthreads();
    // ---- own keys
    K got[FU_ITEMS]; uint32_t sl[FU_ITEMS]; bool hd[FU_ITEMS];
#pragma unroll
    for (int q = 0; q < FU_ITEMS; q++) {
        const int e = e_w + q * 64 + lane;
        hd[q] = false; sl[q] = 0; got[q] = 0;
        if (e < n_loc) {
            hd[q] = base + e == 0 || kl.rc(me[q]) != kl.rc(pv[q]);
            sl[q] = set_slot<FU_SLOTS>(me[q]) & smask;
        }
    }
#pragma unroll
    for (int q = 0; q < FU_ITEMS; q++)                                    // independent LDS atomics in flight per lane
        if (e_w + q * 64 + lane < n_loc) got[q] = atomicCAS(&set[sl[q]], ~0ull, me[q]);
    unsigned long long hb[FU_ITEMS], db[FU_ITEMS];
    uint32_t th = 0, td = 0;
#pragma unroll
    for (int q = 0; q < FU_ITEMS; q++) {
        bool dist = false;
        if (e_w + q * 64 + lane < n_loc) dist = got[q] == ~0ull ? true : (got[q] == me[q] ? false : probe_on(me[q], sl[q]));   // first occurrence of this (row, cell, UMI)
        hb[q] = __ballot(hd[q]); db[q] = __ballot(dist);
        th += (uint32_t)__popcll(hb[q]); td += (uint32_t)__popcll(db[q]);
    }
    if (lane == 0) { s_wh[wave] = th; s_wd[wave] = td; }
    __syncthreads();
    uint32_t r = 0, xd = 0, n_heads = 0, n_dist = 0;
#pragma unroll
    for (int w = 0; w < FU_BLOCK / 64; w++) { if (w < wave) { r += s_wh[w]; xd += s_wd[w]; } n_heads += s_wh[w]; n_dist += s_wd[w]; }
    const unsigned long long lt = (1ull << lane) - 1;
#pragma unroll
    for (int q = 0; q < FU_ITEMS; q++) {
        if (hd[q]) { const uint32_t rr = r + (uint32_t)__popcll(hb[q] & lt); s_hx[rr] = (uint16_t)(xd + (uint32_t)__popcll(db[q] & lt)); s_he[rr] = (uint16_t)(e_w + q * 64 + lane); }
        r += (uint32_t)__popcll(hb[q]); xd += (uint32_t)__popcll(db[q]);
    }
    if (tid == 0) s_hx[n_heads] = (uint16_t)n_dist;
    __syncthreads();
    for (uint32_t i = tid; i < n_heads; i += FU_BLOCK) {
        const K key = k[base + s_he[i]];
        const int32_t cnt = (int32_t)s_hx[i + 1] - (int32_t)s_hx[i];
        const unsigned long long d = out + i;
        row[d] = (int32_t)kl.row(key); col[d] = (int32_t)kl.cell(key);
        if (i + 1 == n_heads) atomicAdd(&val[d], cnt); else val[d] = cnt;  // the last run may continue in later tiles
    }
    if (tid == 0) {
        const uint32_t lead = n_heads ? s_hx[0] : n_dist;
        if (lead && out > 0) atomicAdd(&val[out - 1], (int32_t)lead);
    }
}

constexpr long long RUN_WALK = 64;     // a run head walks at most this many followers itself; longer runs go to k_first_long
__device__ __forceinline__ int nib_bucket(int nib) { return nib == 1 ? 0 : nib == 2 ? 1 : nib == 4 ? 2 : nib == 8 ? 3 : 4; }

// BAF step 1: per (snp, cell, umi) run keep the value with the smallest ordinal (first read in
// fetch order, baf/fc/mcount.py:118-119); tally its allele per SNP (mcount.py:140-150).
template <class K>
__global__ void k_first_read(const K* __restrict__ k, const uint64_t* __restrict__ v, long long n, KeyLayout<K> kl,
                             uint8_t* __restrict__ al_out, uint32_t* __restrict__ tally, unsigned long long* __restrict__ long_runs) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    K me = k[i];
    if (i > 0 && k[i - 1] == me) { al_out[i] = 0; return; }
    uint64_t best = v[i];
    long long j = i + 1;
    for (; j < n && j <= i + RUN_WALK && k[j] == me; j++) { uint64_t x = v[j]; if (x < best) best = x; }
    if (j < n && j > i + RUN_WALK && k[j] == me) { long_runs[1 + atomicAdd(&long_runs[0], 1ull)] = (unsigned long long)i; return; }   // finished by k_first_long
    uint32_t code = uint32_t(best & ((1u << ALLELE_BITS) - 1));      // nibble + 1, 0 = no base
    al_out[i] = (uint8_t)code;
    if (code) atomicAdd(&tally[(size_t)kl.row(me) * 5 + nib_bucket(int(code) - 1)], 1u);
}

// A key run longer than RUN_WALK (a molecule with many reads over one SNP: constant UMI tags, UMI-less deep pileups) is not
// walked by its head lane: the head only queues it, and here ONE BLOCK per run finds the run's end by bisection on the sorted
// keys and takes the minimum (ordinal, allele) value in parallel.  SPLIT: k_first_base's outputs, else k_first_read's.
template <class K, bool SPLIT>
__global__ void __launch_bounds__(256) k_first_long(const K* __restrict__ k, const uint64_t* __restrict__ v, long long n, KeyLayout<K> kl,
                                                      const unsigned long long* __restrict__ long_runs, uint8_t* __restrict__ al_out,
                                                      uint64_t* __restrict__ ord_out, uint32_t* __restrict__ tally) {
    __shared__ unsigned long long s_min[4];
    const unsigned long long n_long = long_runs[0];
    for (unsigned long long r = blockIdx.x; r < n_long; r += gridDim.x) {
        const long long h = (long long)long_runs[1 + r];
        const K me = k[h];
        long long lo = h + 1, hi = n;                                     // first index past the run (every lane bisects: same loads, broadcast by the cache)
        while (lo < hi) { const long long mid = lo + ((hi - lo) >> 1); if (k[mid] == me) lo = mid + 1; else hi = mid; }
        unsigned long long best = ~0ull;
        for (long long j = h + threadIdx.x; j < lo; j += blockDim.x) { const unsigned long long x = v[j]; if (x < best) best = x; }
        for (int d = 32; d; d >>= 1) { const unsigned long long o = __shfl_xor(best, d); if (o < best) best = o; }
        if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = best;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++) if (s_min[w] < best) best = s_min[w];
            const uint32_t code = uint32_t(best & ((1u << ALLELE_BITS) - 1));
            al_out[h] = (uint8_t)code;
            if (SPLIT) ord_out[h] = best >> ALLELE_BITS;
            else if (code) atomicAdd(&tally[(size_t)kl.row(me) * 5 + nib_bucket(int(code) - 1)], 1u);
        }
        __syncthreads();
    }
}

// ---- split mode (64-bit keys): the sorted stream holds only hits WITH a base; the hits without one are looked up ----
// Filter in front of the exact lookups: per (molecule = cell | UMI, block of 32 SNPs) ONE hashed 64-bit word that holds the
// block's SNPs at which the molecule shows a base twice - SNP offset o as bit (o + r1) & 31 of the low half and bit (o + r2) & 31 of
// the high half, r1 / r2 two rotations hashed from the molecule.  A gap record loads the word, rotates the halves back and ANDs
// them: a foreign molecule in the same word must hit the same offset under both of ITS rotations (~0.4 % per SNP), and only the
// SNPs left in the mask are looked up exactly.  One atomic per key run, one load per (record, block) whatever the gap's length.
// The table is laid out ALONG THE SORTED STREAM: the entries of SNP block b go to the words [lo_b, lo_b + len_b), lo_b / len_b =
// the block's index range in the sorted keys (k_blk_bounds) - one word per key, whatever the depth of the block.  The inserts of
// k_first_base therefore land next to the keys being read, and the gap records - which arrive in position order - ask a window of
// the table that moves along with them and stays in L2 (a table hashed over all of its 230 MB cost one HBM round trip per record).
__device__ __forceinline__ void bloom_slot(unsigned long long cellumi, uint32_t blk, unsigned long long lo, unsigned long long len, unsigned long long& word, uint32_t& r1, uint32_t& r2) {
    unsigned long long x = cellumi ^ ((unsigned long long)blk * 0x9E3779B97F4A7C15ull);
    x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    word = lo + (unsigned long long)(((x & 0xffffffffull) * (len & 0xffffffffull)) >> 32);   // len < 2^32 (checked on the host)
    r1 = (uint32_t)(x >> 32) & 31u; r2 = (uint32_t)(x >> 40) & 31u;
}
// first index of every block of 32 SNPs in the sorted keys (blk_lo[n_blk] = n): one bisection per block
template <class K>
__global__ void k_blk_bounds(const K* __restrict__ k, long long n, KeyLayout<K> kl, uint32_t n_blk, unsigned long long* __restrict__ blk_lo) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > n_blk) return;
    if (b == n_blk) { blk_lo[b] = (unsigned long long)n; return; }
    long long lo = 0, hi = n;
    const uint32_t row0 = b << 5;
    while (lo < hi) { const long long mid = lo + ((hi - lo) >> 1); if (kl.row(k[mid]) < row0) lo = mid + 1; else hi = mid; }
    blk_lo[b] = (unsigned long long)lo;
}
// per key run: allele code + ordinal of its first read with a base, at the run head; first / one-past-last index of every SNP
template <class K>
__global__ void k_first_base(const K* __restrict__ k, const uint64_t* __restrict__ v, long long n, KeyLayout<K> kl,
                             uint8_t* __restrict__ al_out, uint64_t* __restrict__ ord_out, unsigned long long* __restrict__ row_lo, unsigned long long* __restrict__ row_hi,
                             unsigned long long* __restrict__ bloom, const unsigned long long* __restrict__ blk_lo, unsigned long long* __restrict__ long_runs) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // The kernel waits for memory 91 % of its wave cycles (profiles/r03_X_sq_counters_resident.txt): a wave's time is the number of
    // DEPENDENT load stages.  Everything a short run needs - the neighbours' keys and the next two values - is therefore loaded up front,
    // without looking at the keys first (the lines are the neighbouring lanes' own), and the filter block's bounds as soon as the row is known.
    const long long ip = i > 0 ? i - 1 : 0, i1 = i + 1 < n ? i + 1 : n - 1, i2 = i + 2 < n ? i + 2 : n - 1;
    const K kp = k[ip], me = k[i], kn1 = k[i1], kn2 = k[i2];
    const uint64_t v0 = v[i], v1 = v[i1], v2 = v[i2];
    const uint32_t row = kl.row(me);
    const unsigned long long b_lo = blk_lo[row >> 5], b_len = blk_lo[(row >> 5) + 1] - b_lo;   // (this key is inside: b_len >= 1)
    if (i == 0 || kl.row(kp) != row) row_lo[row] = (unsigned long long)i;
    if (i + 1 == n || kl.row(kn1) != row) row_hi[row] = (unsigned long long)(i + 1);
    if (i > 0 && kp == me) { al_out[i] = 0; return; }
    uint64_t best = v0;
    long long j = i + 1;
    if (j < n && kn1 == me) {
        if (v1 < best) best = v1;
        j = i + 2;
        if (j < n && kn2 == me) {
            if (v2 < best) best = v2;
            for (j = i + 3; j < n && j <= i + RUN_WALK && k[j] == me; j++) { uint64_t x = v[j]; if (x < best) best = x; }
        }
    }
    if (j < n && j > i + RUN_WALK && k[j] == me) long_runs[1 + atomicAdd(&long_runs[0], 1ull)] = (unsigned long long)i;   // al / ord of this head: k_first_long
    else {
        al_out[i] = (uint8_t)(best & ((1u << ALLELE_BITS) - 1));      // nibble + 1 (never 0 here)
        ord_out[i] = best >> ALLELE_BITS;
    }
    unsigned long long word; uint32_t r1, r2;
    const unsigned long long cu = (unsigned long long)(me & ((K(1) << (kl.cbits + kl.ubits)) - 1));
    bloom_slot(cu, row >> 5, b_lo, b_len, word, r1, r2);
    atomicOr(&bloom[word], (1ull << ((row + r1) & 31u)) | (1ull << (32u + ((row + r2) & 31u))));
}
// every gap record (first SNP, cell, UMI | ordinal, count - 1): for each of its SNPs, if (SNP, cell, UMI) has a run and
// this read comes EARLIER in fetch order than the run's first read with a base, the key belongs to this read
// (baf/fc/mcount.py:118-119) and the run contributes nothing.  The Bloom filter answers "no" for almost every record;
// the exact lookups that remain are binary searches inside one SNP's run (the stream is in tile order, so
// neighbouring threads search the same few SNPs and stay in L2).
constexpr int CL_U = 4;                    // gap records per thread
template <class K>
__global__ void __launch_bounds__(256) k_claim(const K* __restrict__ nk, const uint64_t* __restrict__ nv, unsigned long long cap, ShardSpan sp, unsigned long long n_units,
                                                 const K* __restrict__ keys, KeyLayout<K> kl, const unsigned long long* __restrict__ row_lo, const unsigned long long* __restrict__ row_hi,
                                                 const uint64_t* __restrict__ ord, uint8_t* __restrict__ al,
                                                 const unsigned long long* __restrict__ bloom, const unsigned long long* __restrict__ blk_lo, uint32_t n_rows,
                                                 const uint32_t* __restrict__ p_rowtab, const uint32_t* __restrict__ p_end) {
    const int low = kl.cbits + kl.ubits;
    // unit u = records [256 * CL_U * (u / NSHARD), + 256 * CL_U) of shard slice u % NSHARD: the slices are filled round-robin by consecutive
    // join tiles, so the blocks in flight together hold ONE narrow position range of the file (and one window of the filter table).
    // The kernel is a chain of dependent loads per record (record -> block bounds -> filter word, then for the few survivors cell bounds
    // -> ~9 bisection probes -> ordinal), and nearly every wave holds a survivor: a thread therefore takes CL_U records - all their filter
    // probes are in flight together (a gap covers at most 32 SNPs: two blocks), and the survivors of all of them are looked up in ONE
    // loop whose trip count is the most survivors any lane has, not a loop per record.
    for (unsigned long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const int sh = (int)(u % NSHARD);
        const unsigned long long n_sh = sp.start[sh + 1] - sp.start[sh], idx0 = (u / NSHARD) * (256 * CL_U) + threadIdx.x;
        K cu[CL_U]; uint64_t ordn[CL_U]; uint32_t k1[CL_U], m[CL_U][2];
#pragma unroll
        for (int q = 0; q < CL_U; q++) {
            const unsigned long long idx = idx0 + (unsigned long long)q * 256;
            cu[q] = 0; ordn[q] = 0; k1[q] = 0; m[q][0] = m[q][1] = 0;
            if (idx >= n_sh) continue;
            const unsigned long long j = (unsigned long long)sh * cap + idx;
            const K rec = __builtin_nontemporal_load(&nk[j]);           // (read once: keep the L2 for the table window and the key look-ups)
            const uint64_t v = __builtin_nontemporal_load(&nv[j]);
            ordn[q] = v >> ALLELE_BITS;
            k1[q] = kl.row(rec);
            const uint32_t k2 = min(k1[q] + (uint32_t)(v & ((1u << ALLELE_BITS) - 1)) + 1u, n_rows);
            cu[q] = rec & ((K(1) << low) - 1);
#pragma unroll
            for (int b = 0; b < 2; b++) {                               // (at most 32 SNPs from k1: the block of k1 and the next)
                const uint32_t blk = (k1[q] >> 5) + b;
                if (blk > (k2 - 1) >> 5) continue;
                const unsigned long long b_lo = blk_lo[blk], b_len = blk_lo[blk + 1] - b_lo;
                if (!b_len) continue;                                   // no read shows a base anywhere in this block of SNPs
                unsigned long long word; uint32_t r1, r2;
                bloom_slot((unsigned long long)cu[q], blk, b_lo, b_len, word, r1, r2);
                const uint32_t o0 = max(k1[q], blk << 5) & 31u, o1 = (min(k2, (blk + 1) << 5) - 1u) & 31u;     // the gap's SNPs inside this block: offsets o0 .. o1
                const unsigned long long w = bloom[word];
                const uint32_t h1 = (uint32_t)w, h2 = (uint32_t)(w >> 32);
                m[q][b] = ((h1 >> r1) | (h1 << ((32u - r1) & 31u))) & ((h2 >> r2) | (h2 << ((32u - r2) & 31u))) & ((0xffffffffu >> (31u - o1)) & (0xffffffffu << o0));
            }
        }
        // SNPs at which one of this thread's molecules (or one that shares its filter word) shows a base
        for (;;) {
            int sq = -1, sb = 0;
#pragma unroll
            for (int q = CL_U - 1; q >= 0; q--) { if (m[q][1]) { sq = q; sb = 1; } if (m[q][0]) { sq = q; sb = 0; } }
            if (sq < 0) break;
            K cellumi = 0; uint64_t my_ord = 0; uint32_t my_k1 = 0, mm = 0;
#pragma unroll
            for (int q = 0; q < CL_U; q++) if (q == sq) { cellumi = cu[q]; my_ord = ordn[q]; my_k1 = k1[q]; mm = m[q][sb]; }
            const uint32_t srow = (((my_k1 >> 5) + (uint32_t)sb) << 5) + (uint32_t)__builtin_ctz(mm);
            mm &= mm - 1;
#pragma unroll
            for (int q = 0; q < CL_U; q++) if (q == sq) m[q][sb] = mm;
            // the key's place: inside its (SNP, cell group) cell of the partition sort where there was one (<= 2048 entries: ~9 probes
            // on a few lines; a hot SNP's whole range is 100 k entries), else inside the SNP's range
            unsigned long long lo, hi;
            if (p_rowtab) {
                const uint32_t t = p_rowtab[srow], z = (t >> 5) + ((uint32_t)((unsigned long long)cellumi >> kl.ubits) >> (t & 31u));
                lo = z ? p_end[z - 1] : 0u; hi = p_end[z];
            } else { lo = row_lo[srow]; hi = row_hi[srow]; }
            if (lo >= hi) continue;
            const unsigned long long end = hi;
            const K key = (K(srow) << low) | cellumi;
            while (lo < hi) { const unsigned long long mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
            if (lo < end && keys[lo] == key && my_ord < ord[lo]) al[lo] = 0;   // benign race: every writer stores 0
        }
    }
}
// per-SNP allele tallies (baf/fc/mcount.py:140-150) of the keys that kept an allele.  The keys are sorted by SNP and k_first_base has
// left every SNP's index range, so nothing is searched or added atomically: EIGHT LANES PER SNP walk the SNP's slice of `al` (one
// byte per key; neighbouring SNPs are neighbouring slices, so a wave reads one contiguous stretch), three shuffles put the five
// counts together and lanes 0..4 of the group store them.  (The first form - one thread per key, ballots per wave segment, atomics
// on the SNP's counters - spent 0.77 ms at configs[2] queueing on counter lines shared by neighbouring SNPs.)
// A SNP deeper than TALLY_LONG keys (a hot gene: 100 k keys at configs[2]; bulk input) is queued in pieces of TALLY_PIECE keys, one
// block per piece (k_tally_long), which add their counts to the SNP's (zeroed) counters.
constexpr unsigned long long TALLY_LONG = 2048, TALLY_PIECE = 4096;
__device__ __forceinline__ void tally_code(uint32_t code, uint32_t (&c)[5]) {
    const int b = code ? nib_bucket(int(code) - 1) : -1;
#pragma unroll
    for (int q = 0; q < 5; q++) c[q] += (b == q) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_tally_rows(const uint8_t* __restrict__ al, const unsigned long long* __restrict__ row_lo, const unsigned long long* __restrict__ row_hi,
                                                    uint32_t n_rows, uint32_t* __restrict__ tally, unsigned long long* __restrict__ long_rows) {
    const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, s = gid >> 3; const uint32_t sub = (uint32_t)gid & 7u;
    unsigned long long lo = 0, len = 0;
    if (s < n_rows) { lo = row_lo[s]; const unsigned long long hi = row_hi[s]; len = hi > lo ? hi - lo : 0; }
    const bool is_long = len > TALLY_LONG;
    if (is_long) {
        if (sub == 0) {
            const unsigned long long np = (len + TALLY_PIECE - 1) / TALLY_PIECE, at = atomicAdd(&long_rows[0], np);
            for (unsigned long long q = 0; q < np; q++) long_rows[1 + at + q] = (s << 32) | q;      // (at most len / 2048 entries per SNP: the list holds n / 64)
        }
        len = 0;
    }
    uint32_t c[5] = {0, 0, 0, 0, 0};
    for (unsigned long long t = sub; t < len; t += 8) tally_code(al[lo + t], c);
#pragma unroll
    for (int q = 0; q < 5; q++) { c[q] += __shfl_xor(c[q], 1); c[q] += __shfl_xor(c[q], 2); c[q] += __shfl_xor(c[q], 4); }
    if (s < n_rows && !is_long && sub < 5) tally[(size_t)s * 5 + sub] = sub == 0 ? c[0] : sub == 1 ? c[1] : sub == 2 ? c[2] : sub == 3 ? c[3] : c[4];
}
__global__ void __launch_bounds__(256) k_tally_long(const uint8_t* __restrict__ al, const unsigned long long* __restrict__ row_lo, const unsigned long long* __restrict__ row_hi,
                                                    const unsigned long long* __restrict__ long_rows, uint32_t* __restrict__ tally) {
    __shared__ uint32_t s_c[4][5];
    const unsigned long long n_long = long_rows[0];
    for (unsigned long long r = blockIdx.x; r < n_long; r += gridDim.x) {
        const unsigned long long ent = long_rows[1 + r];
        const size_t s = (size_t)(ent >> 32);
        const unsigned long long lo = row_lo[s] + (ent & 0xffffffffull) * TALLY_PIECE, hi = min(row_hi[s], lo + TALLY_PIECE);
        uint32_t c[5] = {0, 0, 0, 0, 0};
        for (unsigned long long t = lo + threadIdx.x; t < hi; t += 256) tally_code(al[t], c);
#pragma unroll
        for (int q = 0; q < 5; q++) { for (int d = 32; d; d >>= 1) c[q] += __shfl_xor(c[q], d); }
        if ((threadIdx.x & 63) == 0) { for (int q = 0; q < 5; q++) s_c[threadIdx.x >> 6][q] = c[q]; }
        __syncthreads();
        if (threadIdx.x < 5) { const uint32_t v = s_c[0][threadIdx.x] + s_c[1][threadIdx.x] + s_c[2][threadIdx.x] + s_c[3][threadIdx.x]; if (v) atomicAdd(&tally[s * 5 + threadIdx.x], v); }
        __syncthreads();
    }
}

// ---- the same tallies over the molecules of the ENABLED cells only (xck_refold with a cell mask, refold.h) ----
// The mask is a bit table, one bit per cell of the handle.  The walk is the one above - eight lanes per SNP, no atomics on the short
// path, pieces of TALLY_PIECE for the deep SNPs - but every entry's key is read beside its allele byte (both loads are issued before
// either is looked at), because the cell is a field of the key.  A block asks the table once per entry it walks (32 SNPs' slices, or
// one piece of 4096), so a table of up to CM_LDS_WORDS words is copied to LDS first (LDS = true: 10 k cells are 313 words, two loads
// per thread); a larger one is read where it lies (LDS = false: 16 KB and more per block would cost more than they save).
constexpr uint32_t CM_LDS_WORDS = 4096;                                  // 131072 cells, 16 KB of LDS
__device__ __forceinline__ bool cell_on(const uint32_t* __restrict__ bits, uint32_t n_words, uint32_t cell) {
    const uint32_t w = cell >> 5;
    return w < n_words && ((bits[w] >> (cell & 31u)) & 1u);              // (a cell past the table - no key holds one - is off, not out of bounds)
}
// first index of every SNP in the sorted keys, row_lo[n_rows] = n: one bisection per SNP.  k_first_base leaves the same bounds
// in workspace 1 on the split path only, so a masked recount rebuilds them from the keys (the idiom of k_blk_bounds).
template <class K>
__global__ void k_row_bounds(const K* __restrict__ k, long long n, KeyLayout<K> kl, uint32_t n_rows, unsigned long long* __restrict__ row_lo) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s > n_rows) return;
    long long lo = 0, hi = n;
    if (s == n_rows) lo = n;
    while (lo < hi) { const long long mid = lo + ((hi - lo) >> 1); if (kl.row(k[mid]) < s) lo = mid + 1; else hi = mid; }
    row_lo[s] = (unsigned long long)lo;
}
template <class K, bool LDS>
__global__ void __launch_bounds__(256) k_tally_rows_cells(const K* __restrict__ k, const uint8_t* __restrict__ al, KeyLayout<K> kl, const unsigned long long* __restrict__ row_lo,
                                                          uint32_t n_rows, const uint32_t* __restrict__ bits, uint32_t n_words,
                                                          uint32_t* __restrict__ tally, unsigned long long* __restrict__ long_rows) {
    __shared__ uint32_t s_bits[LDS ? CM_LDS_WORDS : 1];
    if (LDS) { for (uint32_t w = threadIdx.x; w < n_words; w += 256) s_bits[w] = bits[w]; __syncthreads(); }
    const unsigned long long gid = (unsigned long long)blockIdx.x * 256 + threadIdx.x, s = gid >> 3; const uint32_t sub = (uint32_t)gid & 7u;
    unsigned long long lo = 0, len = 0;
    if (s < n_rows) { lo = row_lo[s]; len = row_lo[s + 1] - lo; }
    const bool is_long = len > TALLY_LONG;
    if (is_long) {
        if (sub == 0) {
            const unsigned long long np = (len + TALLY_PIECE - 1) / TALLY_PIECE, at = atomicAdd(&long_rows[0], np);
            for (unsigned long long q = 0; q < np; q++) long_rows[1 + at + q] = (s << 32) | q;      // (at most len / 2048 entries per SNP: the list holds n / 2048 + 1)
        }
        len = 0;
    }
    uint32_t c[5] = {0, 0, 0, 0, 0};
    for (unsigned long long t = sub; t < len; t += 8) {
        const uint32_t code = al[lo + t]; const K me = k[lo + t];
        const bool on = LDS ? cell_on(s_bits, n_words, kl.cell(me)) : cell_on(bits, n_words, kl.cell(me));
        tally_code(on ? code : 0u, c);
    }
#pragma unroll
    for (int q = 0; q < 5; q++) { c[q] += __shfl_xor(c[q], 1); c[q] += __shfl_xor(c[q], 2); c[q] += __shfl_xor(c[q], 4); }
    if (s < n_rows && !is_long && sub < 5) tally[(size_t)s * 5 + sub] = sub == 0 ? c[0] : sub == 1 ? c[1] : sub == 2 ? c[2] : sub == 3 ? c[3] : c[4];
}
template <class K, bool LDS>
__global__ void __launch_bounds__(256) k_tally_long_cells(const K* __restrict__ k, const uint8_t* __restrict__ al, KeyLayout<K> kl, const unsigned long long* __restrict__ row_lo,
                                                          const uint32_t* __restrict__ bits, uint32_t n_words,
                                                          const unsigned long long* __restrict__ long_rows, uint32_t* __restrict__ tally) {
    __shared__ uint32_t s_bits[LDS ? CM_LDS_WORDS : 1];
    __shared__ uint32_t s_c[4][5];
    const unsigned long long n_long = long_rows[0];
    if (LDS) { if (blockIdx.x < n_long) for (uint32_t w = threadIdx.x; w < n_words; w += 256) s_bits[w] = bits[w]; __syncthreads(); }   // (a block without a piece copies nothing)
    for (unsigned long long r = blockIdx.x; r < n_long; r += gridDim.x) {
        const unsigned long long ent = long_rows[1 + r];
        const size_t s = (size_t)(ent >> 32);
        const unsigned long long lo = row_lo[s] + (ent & 0xffffffffull) * TALLY_PIECE, hi = min(row_lo[s + 1], lo + TALLY_PIECE);
        uint32_t c[5] = {0, 0, 0, 0, 0};
        for (unsigned long long t = lo + threadIdx.x; t < hi; t += 256) {
            const uint32_t code = al[t]; const K me = k[t];
            const bool on = LDS ? cell_on(s_bits, n_words, kl.cell(me)) : cell_on(bits, n_words, kl.cell(me));
            tally_code(on ? code : 0u, c);
        }
#pragma unroll
        for (int q = 0; q < 5; q++) { for (int d = 32; d; d >>= 1) c[q] += __shfl_xor(c[q], d); }
        if ((threadIdx.x & 63) == 0) { for (int q = 0; q < 5; q++) s_c[threadIdx.x >> 6][q] = c[q]; }
        __syncthreads();
        if (threadIdx.x < 5) { const uint32_t v = s_c[0][threadIdx.x] + s_c[1][threadIdx.x] + s_c[2][threadIdx.x] + s_c[3][threadIdx.x]; if (v) atomicAdd(&tally[s * 5 + threadIdx.x], v); }
        __syncthreads();
    }
}

// plp_snp() filters, baf/fc/core.py:238-246.  info: ref nibble | alt nibble << 4 | ref_hap << 8 | alt_hap << 9
__device__ __forceinline__ bool snp_passes(const uint32_t* tally, const uint32_t* info, uint32_t s, SnpFilter f) {
    const uint32_t* t = tally + (size_t)s * 5;
    uint32_t tot = t[0] + t[1] + t[2] + t[3] + t[4];
    if ((int64_t)tot < (int64_t)f.min_count) return false;
    uint32_t inf = info[s];
    uint32_t a = t[nib_bucket(inf & 15)], b = t[nib_bucket((inf >> 4) & 15)];
    uint32_t minor = a < b ? a : b;
    if ((double)minor < (double)tot * f.min_maf) return false;
    return true;
}

// the verdict itself, per SNP of the sorted table, for the per-SNP summary (feature_summary.h): the rule is stated above and only there
__global__ void __launch_bounds__(256) k_snp_verdict(const uint32_t* __restrict__ tally, const uint32_t* __restrict__ info, uint32_t n, SnpFilter f, uint32_t* __restrict__ kept) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s < n) kept[s] = snp_passes(tally, info, s, f) ? 1u : 0u;
}

// which allele of its SNP a base is: 1 = ALT, 0 = REF, -1 = another base (snp.gt = {ref: ref_idx, alt: alt_idx}: ALT wins when REF == ALT).
// nib: the base's nibble; inf: the SNP's d_snp_info word.  k_expand and the SNP-level counts (snp_counts.h) both decide with it.
__device__ __forceinline__ int allele_side(int nib, uint32_t inf) {
    int side = -1;
    if (nib == int(inf & 15)) side = 0;
    if (nib == int((inf >> 4) & 15)) side = 1;
    return side;
}

// BAF step 2: expand each surviving (snp, cell, umi, allele) to the regions that contain the SNP
// (baf/fc/main.py:92-101, core.py:156-166).  COUNT pass sums the fan-out, EMIT pass writes.
// MASK (xck_refold with a cell mask): a molecule of a cell whose bit in cell_bits is clear expands to nothing, in both passes, and
// `tally` is the tallies of the enabled cells; the table is read where it lies (a block asks 256 times: staging ~300 words would not pay).
template <class K, bool EMIT, class V, bool MASK = false>
__global__ __launch_bounds__(JOIN_BLOCK) void k_expand(const K* __restrict__ k, const uint8_t* __restrict__ al, long long n,
                                  KeyLayout<K> kl, const uint32_t* __restrict__ tally, const uint32_t* __restrict__ info,
                                  SnpFilter f, const int32_t* __restrict__ csr_off, const int32_t* __restrict__ csr_reg,
                                  K* __restrict__ k2, V* __restrict__ v2, unsigned long long* ctl, XBases xb, int pack_shift,
                                  const uint32_t* __restrict__ cell_bits = nullptr, uint32_t n_words = 0) {
    // pack_shift >= 0 (emit pass, 64-bit keys): no values are written - the haplotype class goes into two UMI-field bits that no UMI code
    // uses (k_join ORs the UMI codes of the reads it accepts into ctl_umi_or; the host finds the free bits)
    __shared__ uint32_t s_wave[JOIN_BLOCK / 64];
    __shared__ unsigned long long s_base;
    long long i = (long long)blockIdx.x * JOIN_BLOCK + threadIdx.x;
    uint32_t cnt = 0, s = 0, code = 0; K me = 0;
    int32_t c0 = 0, c1 = 0;
    if (i < n) {
        // (the kernel waits for memory 83 % of its wave cycles: key and allele code are loaded together, and the SNP's region list bounds
        // together with its tallies - three dependent stages instead of five)
        code = al[i]; me = k[i]; s = kl.row(me);
        c0 = csr_off[s]; c1 = csr_off[s + 1];
        if (code && (!MASK || cell_on(cell_bits, n_words, kl.cell(me))) && snp_passes(tally, info, s, f)) cnt = uint32_t(c1 - c0);
    }
    uint32_t total;
    uint32_t excl = block_excl_scan(cnt, s_wave, total);
    if (total == 0) return;
    // count pass: per-shard totals in word 0 of the shard's line; emit pass: per-shard cursor in word 1, inside the
    // shard's slice [xb.base[sh], xb.base[sh] + total_sh) of the output (the order of k2 is irrelevant: it is sorted next)
    const int sh = blockIdx.x & (XSHARD - 1);
    if (threadIdx.x == 0) s_base = xb.base[sh] + atomicAdd(&ctl[CTL_X0 + sh * CTL_STRIDE + (EMIT ? 1 : 0)], (unsigned long long)total);
    if (!EMIT) return;
    __syncthreads();
    if (!cnt) return;
    unsigned long long dst = s_base + excl;
    uint32_t inf = info[s];
    int nib = int(code) - 1;
    const int side = allele_side(nib, inf);
    const int idx = side < 0 ? -1 : int((inf >> (8 + side)) & 1);   // the haplotype index of that allele
    const V bits = idx == 0 ? 1 : idx == 1 ? 2 : 4;
    uint32_t cell = kl.cell(me); uint64_t umi = kl.umi(me);
    if (pack_shift >= 0) umi |= (uint64_t)(idx == 0 ? 0u : idx == 1 ? 1u : 2u) << pack_shift;
    for (int32_t c = c0; c < c1; c++, dst++) {
        k2[dst] = kl.make((uint32_t)csr_reg[c], cell, umi);
        if (pack_shift < 0) v2[dst] = bits;
    }
}

// BAF step 3: haplotype set algebra per (row, cell) run, baf/fc/core.py:173-192, without any thread walking a (row, cell) run
// (a SMART-seq cell holds hundreds of thousands of read names in its most expressed gene; one run = one thread would serialise).
//   k_hap_class: head of every (row, cell, UMI) run: OR of the run's haplotype bits (one entry per SNP the molecule meets: a few)
//   k_hap_sum  : per 2048-key tile, ONE block scan of four packed counters (REF-hap, ALT-hap, either, other-only keys); a run
//                that starts in the tile gets its counts up to the tile end, what later tiles hold of it arrives by atomicAdd
//   k_hap_count / k_hap_scatter: the no_dup_hap arithmetic on the per-run sums -> AD / DP / OTH, compacted into COO
template <class K, class V>
__global__ void k_hap_class(const K* __restrict__ k, const V* __restrict__ v, long long n, uint8_t* __restrict__ cls, unsigned long long* __restrict__ long_runs) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const K me = k[i];
    if (i > 0 && k[i - 1] == me) { cls[i] = 0; return; }
    uint32_t bits = (uint32_t)v[i];
    long long j = i + 1;
    for (; j < n && j <= i + RUN_WALK && k[j] == me; j++) bits |= (uint32_t)v[j];
    // a molecule that meets more than RUN_WALK SNPs of one region (constant UMI tags, bulk input: thousands) is not walked by its
    // head lane: the head queues the run and one block per run finishes it (k_hap_class_long)
    if (j < n && j > i + RUN_WALK && k[j] == me) { cls[i] = 4; long_runs[1 + atomicAdd(&long_runs[0], 1ull)] = (unsigned long long)i; return; }
    cls[i] = (uint8_t)bits;                                               // 1 REF haplotype, 2 ALT haplotype, 4 other allele; never 0 at a head
}
template <class K, class V>
__global__ void __launch_bounds__(256) k_hap_class_long(const K* __restrict__ k, const V* __restrict__ v, long long n, const unsigned long long* __restrict__ long_runs, uint8_t* __restrict__ cls) {
    __shared__ uint32_t s_or[4];
    const unsigned long long n_long = long_runs[0];
    for (unsigned long long r = blockIdx.x; r < n_long; r += gridDim.x) {
        const long long h = (long long)long_runs[1 + r];
        const K me = k[h];
        long long lo = h + 1, hi = n;                                     // first index past the run
        while (lo < hi) { const long long mid = lo + ((hi - lo) >> 1); if (k[mid] == me) lo = mid + 1; else hi = mid; }
        uint32_t bits = 0;
        for (long long j = h + threadIdx.x; j < lo; j += blockDim.x) bits |= (uint32_t)v[j];
        for (int d = 32; d; d >>= 1) bits |= __shfl_xor(bits, d);
        if ((threadIdx.x & 63) == 0) s_or[threadIdx.x >> 6] = bits;
        __syncthreads();
        if (threadIdx.x == 0) cls[h] = (uint8_t)(s_or[0] | s_or[1] | s_or[2] | s_or[3]);
        __syncthreads();
    }
}

__device__ __forceinline__ unsigned long long block_excl_scan64(unsigned long long v, unsigned long long* s_wave, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned long long base = 0; total = 0;
#pragma unroll
    for (int w = 0; w < FD_BLOCK / 64; w++) { const unsigned long long t = s_wave[w]; if (w < wave) base += t; total += t; }
    __syncthreads();
    return base + inc - v;
}

template <class K>
__global__ __launch_bounds__(FD_BLOCK) void k_hap_sum(const K* __restrict__ k, const uint8_t* __restrict__ cls, long long n, KeyLayout<K> kl,
                                                      const unsigned long long* __restrict__ off, K* __restrict__ run_key, uint32_t* __restrict__ acc, long long stride) {
    // acc[f * stride + run]: f = 0 REF-hap keys, 1 ALT-hap keys, 2 keys on either haplotype, 3 keys with only another allele; zero on entry
    __shared__ uint32_t s_wave[FD_BLOCK / 64];
    __shared__ unsigned long long s_wave64[FD_BLOCK / 64];
    __shared__ K tile[FD_TILE + 1];                                       // tile[0] = key before the tile (halo)
    __shared__ unsigned long long s_x[FD_TILE + 1];                       // per head: packed counters before it (4 x 16 bits: a tile holds 2048 keys)
    __shared__ uint16_t s_he[FD_TILE];
    const long long base = (long long)blockIdx.x * FD_TILE;
    const int n_loc = (int)min((long long)FD_TILE, n - base);
#pragma unroll
    for (int t = 0; t < FD_ITEMS; t++) { const int e = t * FD_BLOCK + threadIdx.x; if (e < n_loc) tile[1 + e] = k[base + e]; }
    if (threadIdx.x == 0) tile[0] = base > 0 ? k[base - 1] : K(0);
    __syncthreads();
    const int e0 = threadIdx.x * FD_ITEMS;                                // blocked: thread t owns elements [t * FD_ITEMS, (t + 1) * FD_ITEMS)
    uint32_t hmask = 0; unsigned long long c[FD_ITEMS], sum = 0;
    K prev = tile[e0];
#pragma unroll
    for (int q = 0; q < FD_ITEMS; q++) {
        const int e = e0 + q; c[q] = 0;
        if (e < n_loc) {
            const K me = tile[1 + e];
            if (base + e == 0 || kl.rc(me) != kl.rc(prev)) hmask |= 1u << q;
            const uint32_t bits = cls[base + e];
            c[q] = (unsigned long long)(bits & 1u) | ((unsigned long long)((bits >> 1) & 1u) << 16) | ((unsigned long long)((bits & 3u) ? 1u : 0u) << 32)
                 | ((unsigned long long)((!(bits & 3u) && (bits & 4u)) ? 1u : 0u) << 48);
            sum += c[q];
            prev = me;
        }
    }
    uint32_t n_heads; unsigned long long tot;
    uint32_t r = block_excl_scan((uint32_t)__popc(hmask), s_wave, n_heads);
    unsigned long long xd = block_excl_scan64(sum, s_wave64, tot);
#pragma unroll
    for (int q = 0; q < FD_ITEMS; q++) {
        if (hmask & (1u << q)) { s_x[r] = xd; s_he[r] = (uint16_t)(e0 + q); r++; }
        xd += c[q];
    }
    if (threadIdx.x == 0) s_x[n_heads] = tot;
    __syncthreads();
    const unsigned long long out = off[blockIdx.x];
    auto add = [&](unsigned long long d, unsigned long long x, bool atomic) {
#pragma unroll
        for (int f = 0; f < 4; f++) { const uint32_t val = (uint32_t)((x >> (16 * f)) & 0xffffu); if (!val) continue;
            if (atomic) atomicAdd(&acc[(size_t)f * stride + d], val); else acc[(size_t)f * stride + d] = val; }
    };
    for (uint32_t i = threadIdx.x; i < n_heads; i += FD_BLOCK) {
        const unsigned long long d = out + i;
        run_key[d] = tile[1 + s_he[i]];
        add(d, s_x[i + 1] - s_x[i], i + 1 == n_heads);                    // monotone fields: the packed difference needs no borrow; the last run may continue
    }
    if (threadIdx.x == 0) {
        const unsigned long long lead = n_heads ? s_x[0] : tot;          // keys of the run that the previous tiles started
        if (lead && out > 0) add(out - 1, lead, true);
    }
}

__global__ void k_copy_words(const int32_t* __restrict__ src, int32_t* __restrict__ host_alias, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) host_alias[i] = src[i];
}
struct CopySeg3 { const int32_t* src[3]; int32_t* dst[3]; size_t n[3]; };
__global__ void k_copy_words3(CopySeg3 sg) {                              // blockIdx.y = segment
    const int32_t* __restrict__ src = sg.src[blockIdx.y]; int32_t* __restrict__ dst = sg.dst[blockIdx.y]; const size_t n = sg.n[blockIdx.y];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
// The copy-out rule, stated here and nowhere else: a block of COPY_STREAM_BYTES or more crosses PCIe on the copy stream while the compute
// stream (and other engines) keep the CUs busy; the CUs store a smaller one into mapped pinned memory (no DMA queue shared with another
// engine's bulk copy).  deliver_words: `words` of d_src -> the mapped pinned block h_dst, behind the compute stream's work up to `after`
// (an event the caller recorded there; only the large side reads it); copy_begin, if given, is recorded on the copy stream ahead of the copy.
constexpr size_t COPY_STREAM_BYTES = size_t(8) << 20;
static inline bool on_copy_stream(size_t words) { return words * sizeof(int32_t) >= COPY_STREAM_BYTES; }
static inline unsigned copy_grid(size_t words) { return (unsigned)std::min<size_t>((words + 255) / 256, 1024); }   // blocks of 256 for k_copy_words / k_copy_words3
static int host_alias(EngineImpl* im, int32_t* h, int32_t** alias) { HIP_TRY(hipHostGetDevicePointer((void**)alias, h, 0)); return 0; }
static int deliver_words(EngineImpl* im, const int32_t* d_src, int32_t* h_dst, size_t words, hipEvent_t after, hipEvent_t copy_begin = nullptr) {
    if (on_copy_stream(words)) {
        HIP_TRY(hipStreamWaitEvent(im->s_copy, after, 0));
        if (copy_begin) HIP_TRY(hipEventRecord(copy_begin, im->s_copy));
        HIP_TRY(hipMemcpyAsync(h_dst, d_src, words * sizeof(int32_t), hipMemcpyDeviceToHost, im->s_copy));
    } else if (words) {
        int32_t* alias = nullptr;
        if (int rc = host_alias(im, h_dst, &alias)) return rc;
        hipLaunchKernelGGL(k_copy_words, dim3(copy_grid(words)), dim3(256), 0, im->s_comp, d_src, alias, words);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
// shard slices of (key, value) pairs -> contiguous arrays, one launch (the shard count would be that many copy commands)
template <class K>
__global__ void __launch_bounds__(256) k_pack_pairs(const K* __restrict__ sk, const uint64_t* __restrict__ sv, unsigned long long cap, ShardSpan sp,
                                                      K* __restrict__ dk, uint64_t* __restrict__ dv) {
    const unsigned long long n = sp.start[NSHARD];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        int sh = 0;
#pragma unroll
        for (int q = 1; q < NSHARD; q++) sh += (i >= sp.start[q]) ? 1 : 0;
        const unsigned long long j = (unsigned long long)sh * cap + (i - sp.start[sh]);
        dk[i] = sk[j]; dv[i] = sv[j];
    }
}

// ordered compaction of the haplotype matrices into COO -------------------------------------------
constexpr int CP_BLOCK = 256, CP_ITEMS = 8, CP_TILE = CP_BLOCK * CP_ITEMS;

// single block: exclusive scan of nb block counts (64-bit running sum), total -> out_total
__global__ __launch_bounds__(1024) void k_cp_scan(const uint32_t* __restrict__ blk, long long nb, unsigned long long* __restrict__ off,
                                                  unsigned long long* out_total) {
    __shared__ unsigned long long s_w[16];
    __shared__ unsigned long long s_carry;
    blk += (long long)blockIdx.x * nb; off += (long long)blockIdx.x * nb; out_total += blockIdx.x;   // one block per matrix
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (long long b0 = 0; b0 < nb; b0 += 1024) {
        long long i = b0 + threadIdx.x;
        unsigned long long v = i < nb ? blk[i] : 0, inc = v;
        int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        for (int d = 1; d < 64; d <<= 1) { unsigned long long t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        unsigned long long wb = 0, tot = 0;
        for (int x = 0; x < 16; x++) { if (x < w) wb += s_w[x]; tot += s_w[x]; }
        unsigned long long carry = s_carry;
        if (i < nb) off[i] = carry + wb + inc - v;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) *out_total = s_carry;
}

struct CooOut3 { int32_t* o[3]; unsigned long long total[3]; };       // per matrix: [row | col | val] block and its nnz
// The haplotype matrices straight from the per-run sums: the no_dup_hap arithmetic (baf/fc/core.py:173-192) is done by the count pass
// and by the scatter pass instead of going through three dense arrays (written once, read twice, 2 x the runs long because the arrays
// were sized for the keys).  Eight consecutive runs per thread (two 16-byte loads per sum array; `stride` is a multiple of 8 and the
// arrays are zero beyond the runs, so nothing is bounds-checked per element); tiles beyond the runs leave at once.  One block scan
// of the three counts packed into one 64-bit word.  Output order = run order = (row, cell) order.
struct HapSrc { const uint32_t* acc; long long stride; const unsigned long long* n_runs; long long n_fixed; int no_dup_hap; const unsigned long long* packed; };
// runs: *n_runs, or n_fixed (staging area with holes) when n_runs is null.  packed != null: the four sums of a run as 4 x 16 bits of one
// word (k_hap_items: an item holds at most 2048 keys), instead of the four 32-bit arrays `acc` (k_hap_sum: a run can be millions of keys)
__device__ __forceinline__ void hap_load8(const HapSrc& h, long long i0, int32_t (&ad)[CP_ITEMS], int32_t (&dp)[CP_ITEMS], int32_t (&oth)[CP_ITEMS]) {
    static_assert(CP_ITEMS == 8, "two uint4 per array");
    uint32_t a[4][CP_ITEMS];
    if (h.packed) {
        const uint4* p = reinterpret_cast<const uint4*>(h.packed + i0);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint4 x = p[q];
            a[0][2 * q] = x.x & 0xffffu; a[1][2 * q] = x.x >> 16; a[2][2 * q] = x.y & 0xffffu; a[3][2 * q] = x.y >> 16;
            a[0][2 * q + 1] = x.z & 0xffffu; a[1][2 * q + 1] = x.z >> 16; a[2][2 * q + 1] = x.w & 0xffffu; a[3][2 * q + 1] = x.w >> 16;
        }
    } else {
#pragma unroll
        for (int f = 0; f < 4; f++) {
            const uint4* p = reinterpret_cast<const uint4*>(h.acc + (size_t)f * h.stride + i0);
            const uint4 x = p[0], y = p[1];
            a[f][0] = x.x; a[f][1] = x.y; a[f][2] = x.z; a[f][3] = x.w; a[f][4] = y.x; a[f][5] = y.y; a[f][6] = y.z; a[f][7] = y.w;
        }
    }
#pragma unroll
    for (int t = 0; t < CP_ITEMS; t++) {
        int32_t ref = (int32_t)a[0][t], alt = (int32_t)a[1][t], d = (int32_t)a[2][t]; const int32_t ot = (int32_t)a[3][t];
        if (ref + alt != d) {
            if (h.no_dup_hap) { const int32_t share = ref + alt - d; ref -= share; alt -= share; }
            d = ref + alt;
        }
        const bool keep = d + ot > 0;
        ad[t] = keep && alt > 0 ? alt : 0; dp[t] = keep && d > 0 ? d : 0; oth[t] = keep && ot > 0 ? ot : 0;
    }
}
__global__ __launch_bounds__(CP_BLOCK) void k_hap_count(HapSrc h, uint32_t* __restrict__ blk) {
    __shared__ unsigned long long s_w[CP_BLOCK / 64];
    const long long n = h.n_runs ? (long long)*h.n_runs : h.n_fixed, i0 = (long long)blockIdx.x * CP_TILE + (long long)threadIdx.x * CP_ITEMS;
    if ((long long)blockIdx.x * CP_TILE >= n) { if (threadIdx.x < 3) blk[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = 0; return; }
    unsigned long long c = 0;
    if (i0 < n) {
        int32_t ad[CP_ITEMS], dp[CP_ITEMS], oth[CP_ITEMS];
        hap_load8(h, i0, ad, dp, oth);
#pragma unroll
        for (int t = 0; t < CP_ITEMS; t++) c += (unsigned long long)(ad[t] > 0) | ((unsigned long long)(dp[t] > 0) << 21) | ((unsigned long long)(oth[t] > 0) << 42);
    }
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x < 3) { const unsigned long long t = s_w[0] + s_w[1] + s_w[2] + s_w[3]; blk[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (uint32_t)(t >> (21 * threadIdx.x)) & 0x1fffffu; }
}
template <class K>
__global__ __launch_bounds__(CP_BLOCK) void k_hap_scatter(HapSrc h, const K* __restrict__ k, KeyLayout<K> kl, const unsigned long long* __restrict__ off, CooOut3 out) {
    __shared__ unsigned long long s_w[FD_BLOCK / 64];
    __shared__ int32_t s_row[CP_TILE], s_col[CP_TILE], s_val[CP_TILE];    // one matrix's entries of this tile, compacted: they leave with coalesced stores
    static_assert(FD_BLOCK == CP_BLOCK, "block_excl_scan64 is written for FD_BLOCK threads");
    const long long n = h.n_runs ? (long long)*h.n_runs : h.n_fixed, i0 = (long long)blockIdx.x * CP_TILE + (long long)threadIdx.x * CP_ITEMS;
    if ((long long)blockIdx.x * CP_TILE >= n) return;
    int32_t v[3][CP_ITEMS];
    unsigned long long c = 0;
    if (i0 < n) {
        hap_load8(h, i0, v[0], v[1], v[2]);
#pragma unroll
        for (int t = 0; t < CP_ITEMS; t++) c += (unsigned long long)(v[0][t] > 0) | ((unsigned long long)(v[1][t] > 0) << 21) | ((unsigned long long)(v[2][t] > 0) << 42);
    } else {
#pragma unroll
        for (int t = 0; t < CP_ITEMS; t++) v[0][t] = v[1][t] = v[2][t] = 0;
    }
    unsigned long long total;
    const unsigned long long excl = block_excl_scan64(c, s_w, total);
    int32_t krow[CP_ITEMS], kcol[CP_ITEMS];
#pragma unroll
    for (int t = 0; t < CP_ITEMS; t++) {                                 // (`k` holds one key per staging entry and is at least stride long; only entries with a value are used)
        krow[t] = 0; kcol[t] = 0;
        if (c && (v[0][t] > 0 || v[1][t] > 0 || v[2][t] > 0)) { const K key = k[i0 + t]; krow[t] = (int32_t)kl.row(key); kcol[t] = (int32_t)kl.cell(key); }
    }
    // (a thread's entries sit next to each other, eight threads' worth apart: stored straight from the registers they kept the address
    // unit busy 62 % of the wave cycles)
#pragma unroll
    for (int y = 0; y < 3; y++) {
        uint32_t d = (uint32_t)((excl >> (21 * y)) & 0x1fffffull);
        const uint32_t tot = (uint32_t)((total >> (21 * y)) & 0x1fffffull);
#pragma unroll
        for (int t = 0; t < CP_ITEMS; t++)
            if (v[y][t] > 0) { s_row[d] = krow[t]; s_col[d] = kcol[t]; s_val[d] = v[y][t]; d++; }
        __syncthreads();
        int32_t* __restrict__ row = out.o[y]; int32_t* __restrict__ col = row + out.total[y]; int32_t* __restrict__ val = col + out.total[y];
        const unsigned long long base = off[(size_t)y * gridDim.x + blockIdx.x];
        for (uint32_t j = threadIdx.x; j < tot; j += CP_BLOCK) { row[base + j] = s_row[j]; col[base + j] = s_col[j]; val[base + j] = s_val[j]; }
        __syncthreads();
    }
}

// ---- finish -------------------------------------------------------------------------------
struct Timer {
    EngineImpl* im; hipEvent_t a, b;
    int start() { HIP_TRY(hipEventRecord(a, im->s_comp)); return 0; }
    int stop(double* acc) { HIP_TRY(hipEventRecord(b, im->s_comp)); HIP_TRY(hipEventSynchronize(b)); float ms; HIP_TRY(hipEventElapsedTime(&ms, a, b)); *acc += ms; im->st.ms_device += ms; return 0; }
};

// One radix sort over key bits [0, top).  (rocPRIM's mid-size merge path is not stable, so the classic
// "sort the low range, then the high range" trick to skip the all-zero bits between the used UMI bits and
// the cell field is NOT safe with it - measured on gfx950, profiles/experiments/sorttest.hip.)
// Keys-only sort of 64-bit keys: sort kernel at 1024 threads x 8 keys and histogram kernel at 512 x 32 instead of rocPRIM
// 4.2's tuned default for gfx950 (512 x 12 for both): 7.90 ms instead of 9.42 ms for 380 M keys over 32 bits
// (profiles/experiments/sortcfg.hip, profiles/r01_g_sort_configs.log; 10-bit digits, which would need one pass fewer, are
// slower: 5.3 ms vs 4.5 ms at 200 M keys).  Everything else keeps the defaults.
template <class K>
using KeySortConfig = typename std::conditional<sizeof(K) == 8,
    rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                               rocprim::radix_sort_onesweep_config<rocprim::kernel_config<512, 32>, rocprim::kernel_config<1024, 8>, 8,
                                                                   rocprim::block_radix_rank_algorithm::match>>,
    rocprim::default_config>::type;
// pairs with 64-bit keys: 1024 x 6 with 8-byte values (4.29 ms vs 4.56 ms for 72 M pairs over 56 bits), 1024 x 8 with 1-byte values
// (1.31 ms vs 1.45 ms for 25 M pairs)
template <class K, class V>
using PairSortConfig = typename std::conditional<sizeof(K) == 8 && (sizeof(V) == 8 || sizeof(V) == 1),
    rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config,
                               rocprim::radix_sort_onesweep_config<rocprim::kernel_config<512, 32>, rocprim::kernel_config<1024, sizeof(V) == 8 ? 6 : 8>, 8,
                                                                   rocprim::block_radix_rank_algorithm::match>>,
    rocprim::default_config>::type;

template <class K, class V>
static size_t sort_tmp_bytes(size_t n, int top) {
    size_t tb = 0; K* k = nullptr; V* v = nullptr;
    if constexpr (std::is_same<V, rocprim::empty_type>::value) (void)rocprim::radix_sort_keys<KeySortConfig<K>>(nullptr, tb, k, k, n, 0u, (unsigned)top, (hipStream_t)0);
    else (void)rocprim::radix_sort_pairs<PairSortConfig<K, V>>(nullptr, tb, k, k, v, v, n, 0u, (unsigned)top, (hipStream_t)0);
    return tb + 256;
}
template <class K, class V>
static int sort_run(EngineImpl* im, void* tmp, size_t tmp_bytes, K* kin, K* kout, V* vin, V* vout, size_t n, int top, int begin = 0) {
    hipError_t er;
    if constexpr (std::is_same<V, rocprim::empty_type>::value) er = rocprim::radix_sort_keys<KeySortConfig<K>>(tmp, tmp_bytes, kin, kout, n, (unsigned)begin, (unsigned)top, im->s_comp);
    else er = rocprim::radix_sort_pairs<PairSortConfig<K, V>>(tmp, tmp_bytes, kin, kout, vin, vout, n, 0u, (unsigned)top, im->s_comp);
    HIP_TRY(er);
    return 0;
}

// hand matrix m ([row|col|val] at d_o) to the host
static int copy_out(EngineImpl* im, int m, int32_t* d_o, size_t total) {
    im->d_res[m] = d_o;
    // a copy on the copy stream waits for the scatter (ev_res) and is timed from the first of a finish (ev_c0) to the last (ev_c1); xck_finish_async() does not wait for it
    const bool big = on_copy_stream(total * 3);
    if (big) HIP_TRY(hipEventRecord(im->ev_res, im->s_comp));
    if (int rc = deliver_words(im, d_o, im->h_res[m], total * 3, im->ev_res, im->copy_timed ? nullptr : im->ev_c0)) return rc;
    if (big) { im->copy_timed = true; HIP_TRY(hipEventRecord(im->ev_c1, im->s_copy)); }
    return 0;
}

// ordered compaction of the runs' AD / DP / OTH (hap: per-run sums, n staging entries) into the COO blocks of matrices m0..m0+2:
// counts and scans of all three first, ONE read-back of the totals, then the scatter and the copy-out.  The COO blocks are taken
// exactly, at the place `ws` reserved for their upper bound (w.coo_at).
static const char* const WS_REGION_FULL = "workspace exhausted (region-level hits)";
template <class K>
static int compact_coo(EngineImpl* im, Arena& ws, const RegionWs& w, const HapSrc& hap, const K* keys, size_t n, KeyLayout<K> kl, int m0) {
    const int nm = 3;
    size_t nb = (n + CP_TILE - 1) / CP_TILE;
    const unsigned long long* h_tot;
    hipLaunchKernelGGL(k_hap_count, dim3(nb), dim3(CP_BLOCK), 0, im->s_comp, hap, w.d_blk);
    hipLaunchKernelGGL(k_cp_scan, dim3(nm), dim3(1024), 0, im->s_comp, w.d_blk, (long long)nb, w.d_off, im->d_ctl + CTL_X0);   // the k_expand words are free again at this point
    if (int rc = read_ctl_words(im, CTL_X0, nm, h_tot)) return rc;
    CooOut3 out; memset(&out, 0, sizeof out);
    bool any = false;
    ws.off = w.coo_at;
    for (int y = 0; y < nm; y++) {
        const size_t total = h_tot[y];
        im->res_nnz[m0 + y] = total; im->d_res[m0 + y] = nullptr; out.total[y] = total;
        if (!total) continue;
        int rc = res_reserve(im, m0 + y, total); if (rc) return rc;
        out.o[y] = ws.get<int32_t>(total * 3);
        if (!out.o[y]) { im->eng->err = WS_REGION_FULL; return XCK_E_NOMEM; }   // (more non-zeros than runs: the bound the block was reserved at is broken)
        any = true;
    }
    if (!any) return 0;
    hipLaunchKernelGGL((k_hap_scatter<K>), dim3(nb), dim3(CP_BLOCK), 0, im->s_comp, hap, keys, kl, (const unsigned long long*)w.d_off, out);
    HIP_TRY(hipGetLastError());
    // copy-out: large blocks go through copy_out() (copy stream); the small ones share one store kernel into mapped pinned memory
    CopySeg3 sg; memset(&sg, 0, sizeof sg); size_t mx = 0;
    for (int y = 0; y < nm; y++) {
        const size_t total = out.total[y];
        if (!total) continue;
        if (on_copy_stream(total * 3)) { int rc = copy_out(im, m0 + y, out.o[y], total); if (rc) return rc; continue; }
        im->d_res[m0 + y] = out.o[y];
        if (int rc = host_alias(im, im->h_res[m0 + y], &sg.dst[y])) return rc;
        sg.src[y] = out.o[y]; sg.n[y] = total * 3; mx = std::max(mx, total * 3);
    }
    if (mx) {
        hipLaunchKernelGGL(k_copy_words3, dim3(copy_grid(mx), nm), dim3(256), 0, im->s_comp, sg);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// basefc: sorted keys -> COO (row, col, count of distinct keys) without a dense intermediate
constexpr int FOLD_GIANT = 1;              // fold_coo(): a (row, cell) run too long for the hash fold - redo on fully sorted keys
static const char* const WS_RADIX_FULL = "workspace exhausted (radix-sort fold)";
template <class K>
static int fold_coo(EngineImpl* im, Arena& ws, const RadixFoldWs& w, const K* keys, size_t n, KeyLayout<K> kl, int m, int sorted_from = 0) {   // sorted_from: lowest key bit the sort covered
    size_t nb = (n + FD_TILE - 1) / FD_TILE;
    uint32_t* d_blk = w.d_blk; unsigned long long* d_off = w.d_off;
    const unsigned long long* h;
    hipLaunchKernelGGL((k_fold_heads<K>), dim3(nb), dim3(FD_BLOCK), 0, im->s_comp, keys, (long long)n, kl, d_blk);
    hipLaunchKernelGGL(k_cp_scan, dim3(1), dim3(1024), 0, im->s_comp, d_blk, (long long)nb, d_off, im->d_ctl + CTL_SCRATCH);
    int rc = read_ctl_words(im, CTL_SCRATCH, 1, h); if (rc) return rc;
    size_t total = h[0];
    im->res_nnz[m] = total; im->d_res[m] = nullptr;
    if (!total) return 0;
    rc = res_reserve(im, m, total); if (rc) return rc;
    ws.off = w.coo_at;                                                    // (an attempt that ended in FOLD_GIANT took its block here as well)
    int32_t* d_o = ws.get<int32_t>(total * 3);
    if (!d_o) { im->eng->err = WS_RADIX_FULL; return XCK_E_NOMEM; }       // (more non-zeros than keys: the bound the block was reserved at is broken)
    HIP_TRY(hipMemsetAsync(d_o + 2 * total, 0, total * sizeof(int32_t), im->s_comp));       // k_fold_emit accumulates run pieces into val[]
    if constexpr (sizeof(K) == 8) {
        if (sorted_from > 0) {
            HIP_TRY(hipMemsetAsync(im->d_ctl + CTL_GIANT, 0, sizeof(unsigned long long), im->s_comp));
            KeyLayout<unsigned long long> kl8; kl8.ubits = kl.ubits; kl8.cbits = kl.cbits;
            hipLaunchKernelGGL(k_fold_emit_unsorted, dim3(nb), dim3(FU_BLOCK), FU_SLOTS * 8, im->s_comp, (const unsigned long long*)keys, (long long)n, kl8, d_off,
                               d_o, d_o + total, d_o + 2 * total, im->d_ctl + CTL_GIANT, sorted_from);
            if ((rc = read_ctl_words(im, CTL_GIANT, 1, h))) return rc;
            if (im->eng->knobs.debug_timing) fprintf(stderr, "[xck] hash fold: n=%zu nnz=%zu ubits=%d cbits=%d giant=%llu\n", n, total, kl.ubits, kl.cbits, h[0]);
            if (h[0]) return FOLD_GIANT;
            return copy_out(im, m, d_o, total);
        }
    }
    hipLaunchKernelGGL((k_fold_emit<K>), dim3(nb), dim3(FD_BLOCK), 0, im->s_comp, keys, (long long)n, kl, d_off, d_o, d_o + total, d_o + 2 * total);
    HIP_TRY(hipGetLastError());
    return copy_out(im, m, d_o, total);
}

// shard slices -> one contiguous array, with the UMI field narrowed from `ubits` to `used` bits (the row and cell
// fields move down): every dead bit removed is one bit the radix sort does not have to pass over
__global__ void __launch_bounds__(256) k_pack_squeeze(const unsigned long long* __restrict__ src, unsigned long long cap, ShardSpan sp,
                                                        int ubits, int used, unsigned long long* __restrict__ dst) {
    const unsigned long long n = sp.start[NSHARD];
    const unsigned long long lowmask = (1ull << used) - 1;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        int sh = 0;
#pragma unroll
        for (int q = 1; q < NSHARD; q++) sh += (i >= sp.start[q]) ? 1 : 0;
        const unsigned long long k = src[(unsigned long long)sh * cap + (i - sp.start[sh])];
        dst[i] = ((k >> ubits) << used) | (k & lowmask);
    }
}

// copy the used prefix of every shard slice into one contiguous array (sort input)
template <class K>
static int pack_shards(EngineImpl* im, K* dst_keys, uint64_t* dst_vals) {
    size_t off = 0;
    for (int sh = 0; sh < NSHARD; sh++) {
        const size_t c = im->cur[sh];
        if (!c) continue;
        HIP_TRY(hipMemcpyAsync(dst_keys + off, (K*)im->d_keys + (size_t)sh * im->hit_cap, c * sizeof(K), hipMemcpyDeviceToDevice, im->s_comp));
        if (dst_vals) HIP_TRY(hipMemcpyAsync(dst_vals + off, im->d_vals + (size_t)sh * im->hit_cap, c * sizeof(uint64_t), hipMemcpyDeviceToDevice, im->s_comp));
        off += c;
    }
    return 0;
}

#include "fold_partition.h"

// ---- finish: basefc ----------------------------------------------------------------------
// the radix-sort fold: takes every input.  64-bit keys: the sort only orders (row, cell) and fold_coo() tells the UMIs of a run apart
template <class K>
static int fold_by_radix_sort(EngineImpl* im, size_t n) {
    KeyLayout<K> kl = key_layout<K>(im);
    Timer tm{im, im->ev0, im->ev1};
    int rc;
    const int top = im->ubits + im->cbits + im->rbits;
    K* keys = (K*)im->d_keys;
    im->fold_path = 2;
    const size_t tmpb = sort_tmp_bytes<K, rocprim::empty_type>(n, top);
    RadixFoldWs w;
    if ((rc = pf_carve(im, im->ws1, true, [&](Arena& ar) { radix_fold_carve(ar, n, sizeof(K), tmpb, w); }, WS_RADIX_FULL))) return rc;
    K* alt = (K*)w.alt; void* tmp = w.tmp;
    if ((rc = tm.start())) return rc;
    int used = im->ubits;                                                       // UMI bits actually in use
    if (sizeof(K) == 8) { unsigned long long uor = 0; for (int sh = 0; sh < NSHARD; sh++) uor |= im->h_ctl[ctl_umi_or(sh)]; used = uor ? 64 - __builtin_clzll(uor) : 1; if (used > im->ubits) used = im->ubits; }
    if (used < im->ubits) {
        hipLaunchKernelGGL(k_pack_squeeze, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, im->s_comp,
                           (const unsigned long long*)im->d_keys, (unsigned long long)im->hit_cap, shard_span(im->cur), im->ubits, used, (unsigned long long*)alt);
        HIP_TRY(hipGetLastError());
        kl.ubits = used;
    } else
    if ((rc = pack_shards(im, alt, (uint64_t*)nullptr))) return rc;             // shard slices -> contiguous
    const int top_fc = kl.ubits + im->cbits + im->rbits;
    // 64-bit keys: the radix sort only orders (row, cell) - 4 passes instead of 7 - and the fold tells the UMIs of a run
    // apart with an LDS hash set; a run too long for that (FOLD_GIANT) is redone on fully sorted keys
    const bool full_sort = im->eng->knobs.full_sort;
    // (rocPRIM 4.2 returns garbage for begin_bit > 0 with end_bit = 64 - profiles/experiments/sortpart.hip - so keys that could not be
    // squeezed below 63 bits take the classic path)
    const bool partial = sizeof(K) == 8 && !full_sort && top_fc <= 62;
    // whole 8-bit digits from the top: the (row, cell) bits plus whatever UMI bits the last digit reaches for free.  A run
    // that is still too long for the fold's lead-in window (FOLD_GIANT: one gene holding a large share of a cell's reads)
    // is split further - one more digit per attempt, remembered for the next finish() of this handle.
    auto begin_for = [&](int extra) { const int passes = (top_fc - kl.ubits + 7) / 8 + extra; return std::max(0, top_fc - 8 * passes); };
    int begin = partial ? begin_for(im->fold_extra_digits) : 0;
    K* src = alt; K* dst = keys;
    if ((rc = sort_run<K, rocprim::empty_type>(im, tmp, tmpb, src, dst, nullptr, nullptr, n, top_fc, begin))) return rc;
    rc = fold_coo<K>(im, im->ws1, w, dst, n, kl, 0, begin);
    while (rc == FOLD_GIANT) {                                        // (the next attempt works in the same blocks)
        im->fold_extra_digits++;
        begin = begin_for(im->fold_extra_digits);
        std::swap(src, dst);                                          // any order of the same keys is a valid sort input
        if ((rc = sort_run<K, rocprim::empty_type>(im, tmp, tmpb, src, dst, nullptr, nullptr, n, top_fc, begin))) return rc;
        rc = fold_coo<K>(im, im->ws1, w, dst, n, kl, 0, begin);   // begin == 0: fully sorted, classic fold, cannot be giant
    }
    if (rc) return rc;
    return tm.stop(&im->st.ms_sort);
}

// the same fold over the keys of the unique-feature molecules alone (XCK_F_UNIQUE_FEATURE)
#include "umi_feature.h"
// the connected components of the 1-mismatch graph of every (row, cell) instead of its keys (XCK_F_UMI_COLLAPSE)
#include "umi_collapse.h"

template <class K>
static int finish_basefc(EngineImpl* im, size_t n) {
    // unique-feature molecules: the stage of umi_feature.h leaves its survivors cell-major in the shard slices, an order level 1 of the
    // partition fold is not built for - the radix-sort fold counts them
    if (im->d_uf_rank) {
        im->fold_path = 2;
        if (int rc = unique_feature_keys<K>(im, n, &n)) return rc;
        if (n == 0) return 0;                                             // (every molecule dropped: empty matrix, and the counters of umi_collapse.h stay zero)
        if (im->umi_collapse) return umi_collapse_fold<K>(im, n);          // (the survivors on exact UMIs, collapsed afterwards)
        return fold_by_radix_sort<K>(im, n);
    }
    if (im->umi_collapse) { im->fold_path = 2; return umi_collapse_fold<K>(im, n); }
    // 64-bit keys: the partition fold (fold_partition.h - no sort); it hands back PF_FALLBACK for the inputs it cannot place
    // (one (row, cell) with more keys than a work item holds, ...), and the radix-sort fold then takes over
    if constexpr (sizeof(K) == 8) {
        const bool want_sort = im->eng->knobs.fold_sort;
        if (!want_sort) {
            Timer tm{im, im->ev0, im->ev1};
            int rc;
            if ((rc = tm.start())) return rc;
            rc = fold_partition(im, key_layout<unsigned long long>(im), n);
            if (rc == 0) {
                im->fold_path = 1;
                return tm.stop(&im->st.ms_sort);
            }
            if (rc != PF_FALLBACK) return rc;
            im->fold_fallbacks++;
            if (im->eng->knobs.debug_timing) fprintf(stderr, "[xck] partition fold: handing over to the radix-sort fold\n");
        }
    }
    return fold_by_radix_sort<K>(im, n);
}

// ---- finish: pileup ----------------------------------------------------------------------
// what one stage of the pileup fold hands to the next
template <class K> struct PileupFold {
    // region-level values: 64-bit words beside 64-bit keys (the partition sort carries 64-bit values), bytes beside 128-bit keys
    typedef typename std::conditional<sizeof(K) == 8, uint64_t, uint8_t>::type V2;
    // the hits with a base: workspace 1 (fold_ws.h; the region stage sees w1.al alone)
    MoleculeWs w1;
    const K* keys; const uint64_t* vals;   // sorted by (key, value), wherever sort_pileup_hits left them
    PartIndex pidx;                        // the partition's cells, for k_claim's look-ups (stays null after the radix sort)
    // count_region_hits: region-level hits per k_expand shard, their sum, the widest shard (rounded up to 64), UMI-field bits in use
    unsigned long long tot2[XSHARD], cap2; size_t n2; int used2;
    // the region-level hits: workspace 2, and its key and value blocks under their types
    RegionWs w2;
    K* k2; V2* v2;                         // as k_expand wrote them; k2 holds the run keys once they are partitioned / sorted
    K* k2b; V2* v2b;                       // sorted
    size_t tmpb2;
};
static_assert(FD_TILE == (int)WS_TILE && CP_TILE == (int)WS_TILE && RUN_WALK == (long long)WS_RUN_WALK && XSHARD == (int)WS_SLICES, "fold_ws.h sizes its blocks by these");
static const char* const WS_MOLECULE_FULL = "workspace exhausted (pileup fold)";

// the hits sorted by (key, value): by row partition + one LDS sort per item (fold_partition.h); a SNP deeper than an item, or
// 128-bit keys, take the radix sort
template <class K>
static int sort_pileup_hits(EngineImpl* im, size_t n, size_t tmpb, PileupFold<K>& pf) {
    int rc;
    K* alt = (K*)pf.w1.alt; uint64_t* valt = pf.w1.valt; void* tmp = pf.w1.tmp;
    pf.pidx = PartIndex{nullptr, nullptr};
    if constexpr (sizeof(K) == 8) {
        // (default since the items are sorted by an LDS radix sort: 1.7 ms at configs[2] against 2.3 ms for pack + rocPRIM's eight passes;
        // XCK_PILEUP_SORT=radix forces the library sort)
        const bool want_part = !im->eng->knobs.pileup_radix;
        if (want_part) {
            rc = pileup_partition_sort(im, im->ws2, true, key_layout<unsigned long long>(im), (const unsigned long long*)im->d_keys, (const uint64_t*)im->d_vals, im->hit_cap, im->cur,
                                       (uint32_t)std::max(im->n_snps_sorted, 1), n, (unsigned long long*)alt, valt, nullptr, &pf.pidx);
            if (rc == 0) { im->pileup_sort_path = 1; pf.keys = alt; pf.vals = valt; return 0; }
            else if (rc != PF_FALLBACK) return rc;
        }
    }
    im->pileup_sort_path = 2;
    hipLaunchKernelGGL((k_pack_pairs<K>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, im->s_comp,
                       (const K*)im->d_keys, (const uint64_t*)im->d_vals, (unsigned long long)im->hit_cap, shard_span(im->cur), alt, valt);
    HIP_TRY(hipGetLastError());
    const int top = im->ubits + im->cbits + im->rbits;
    if ((rc = sort_run<K, uint64_t>(im, tmp, tmpb, alt, (K*)im->d_keys, valt, im->d_vals, n, top))) return rc;
    pf.keys = (const K*)im->d_keys; pf.vals = im->d_vals;       // sorted data now lives in d_keys / d_vals
    return 0;
}

// first read per key, pileup split mode (64-bit keys): SNP-mask filter laid out along the sorted stream, gap records claimed against it
template <class K>
static int first_reads_split(EngineImpl* im, size_t n, const PileupFold<K>& pf) {
    static_assert(sizeof(K) == 8, "the join kernel splits the pileup hits for 64-bit keys only (split_mode())");
    const KeyLayout<K> kl = key_layout<K>(im);
    const unsigned gs = (unsigned)((n + 255) / 256);
    const MoleculeWs& w = pf.w1;
    uint8_t* al = w.al; unsigned long long* long_runs = w.long_runs;
    const size_t ns = std::max<size_t>((size_t)im->n_snps_sorted, 1);
    uint64_t* ordv = w.ordv; unsigned long long *row_lo = w.row_lo, *row_hi = w.row_hi;
    if (n >> 32) { im->eng->err = "pileup fold: more than 2^32 hits with a base in one finish"; return XCK_E_NOMEM; }
    const uint32_t n_blk = (uint32_t)((ns + 31) >> 5);
    unsigned long long *bloom = w.bloom, *blk_lo = w.blk_lo;          // bloom: one word per key, laid out along the sorted stream (bloom_slot)
    HIP_TRY(hipMemsetAsync(row_lo, 0, 2 * ns * sizeof(unsigned long long), im->s_comp));
    HIP_TRY(hipMemsetAsync(bloom, 0, n * sizeof(unsigned long long), im->s_comp));
    hipLaunchKernelGGL((k_blk_bounds<K>), dim3((n_blk + 256) / 256), dim3(256), 0, im->s_comp, pf.keys, (long long)n, kl, n_blk, blk_lo);
    hipLaunchKernelGGL((k_first_base<K>), dim3(gs), dim3(256), 0, im->s_comp, pf.keys, pf.vals, (long long)n, kl, al, ordv, row_lo, row_hi,
                       bloom, (const unsigned long long*)blk_lo, long_runs);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_first_long<K, true>), dim3(1024), dim3(256), 0, im->s_comp, pf.keys, pf.vals, (long long)n, kl, (const unsigned long long*)long_runs, al, ordv, im->d_tally);
    HIP_TRY(hipGetLastError());
    if (im->ncursor) {
        const ShardSpan nsp = shard_span(im->ncur);
        const unsigned long long mx = *std::max_element(im->ncur, im->ncur + NSHARD);
        const unsigned long long n_units = ((mx + 256 * CL_U - 1) / (256 * CL_U)) * NSHARD;
        // (one block per unit: blocks start in index order, so the resident ones hold consecutive units = ONE window of the table; a grid-stride
        // loop over 16 k blocks mixed up to 11 windows and every probe went to HBM: 5.5 GB read for 0.74 GB of records)
        hipLaunchKernelGGL((k_claim<K>), dim3((unsigned)std::min<unsigned long long>(n_units, 1ull << 30)), dim3(256), 0, im->s_comp,
                           (const K*)im->d_nkeys, (const uint64_t*)im->d_nvals, (unsigned long long)im->hit_cap, nsp, n_units,
                           pf.keys, kl, (const unsigned long long*)row_lo, (const unsigned long long*)row_hi, (const uint64_t*)ordv, al,
                           (const unsigned long long*)bloom, (const unsigned long long*)blk_lo, (uint32_t)ns, pf.pidx.rowtab, pf.pidx.end);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetAsync(long_runs, 0, sizeof(unsigned long long), im->s_comp));   // (k_first_long is done with the list: now the SNPs deeper than TALLY_LONG)
    hipLaunchKernelGGL(k_tally_rows, dim3((unsigned)((ns * 8 + 255) / 256)), dim3(256), 0, im->s_comp, (const uint8_t*)al, (const unsigned long long*)row_lo, (const unsigned long long*)row_hi,
                       (uint32_t)ns, im->d_tally, long_runs);
    hipLaunchKernelGGL(k_tally_long, dim3(1024), dim3(256), 0, im->s_comp, (const uint8_t*)al, (const unsigned long long*)row_lo, (const unsigned long long*)row_hi,
                       (const unsigned long long*)long_runs, im->d_tally);
    HIP_TRY(hipGetLastError());
    return 0;
}

// first read per key when every hit, with a base or without, is in the sorted stream (128-bit keys; -DXCK_BAF_SPLIT=0 builds)
template <class K>
static int first_reads_plain(EngineImpl* im, size_t n, const PileupFold<K>& pf) {
    const KeyLayout<K> kl = key_layout<K>(im);
    const unsigned gs = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL((k_first_read<K>), dim3(gs), dim3(256), 0, im->s_comp, pf.keys, pf.vals, (long long)n, kl, pf.w1.al, im->d_tally, pf.w1.long_runs);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_first_long<K, false>), dim3(1024), dim3(256), 0, im->s_comp, pf.keys, pf.vals, (long long)n, kl, (const unsigned long long*)pf.w1.long_runs, pf.w1.al, (uint64_t*)nullptr, im->d_tally);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the same stage under the handle's other rule (XCK_F_UMI_CONSENSUS): a plurality vote per key, and the agreement counters
#include "umi_consensus.h"

// one k_expand pass over the molecule stage: all cells, or (after xck_refold with a cell mask) the enabled ones under their tallies
template <class K, bool EMIT>
static void launch_expand(EngineImpl* im, size_t n, const PileupFold<K>& pf, const XBases& xb, int pack_shift) {
    typedef typename PileupFold<K>::V2 V2;
    const KeyLayout<K> kl = key_layout<K>(im);
    const unsigned gs = (unsigned)((n + 255) / 256);
    K* k2 = EMIT ? pf.k2 : (K*)nullptr; V2* v2 = EMIT ? pf.v2 : (V2*)nullptr;
    if (!im->d_cell_bits)
        hipLaunchKernelGGL((k_expand<K, EMIT, V2>), dim3(gs), dim3(JOIN_BLOCK), 0, im->s_comp, pf.keys, pf.w1.al, (long long)n, kl, im->d_tally, im->d_snp_info,
                           im->sf, im->d_csr_off, im->d_csr_reg, k2, v2, im->d_ctl, xb, pack_shift);
    else
        hipLaunchKernelGGL((k_expand<K, EMIT, V2, true>), dim3(gs), dim3(JOIN_BLOCK), 0, im->s_comp, pf.keys, pf.w1.al, (long long)n, kl, cur_tally(im), im->d_snp_info,
                           im->sf, im->d_csr_off, im->d_csr_reg, k2, v2, im->d_ctl, xb, pack_shift, im->d_cell_bits, (uint32_t)((im->n_cells + 31) / 32));
}

// the k_expand count pass: how many region-level hits every shard will write
template <class K>
static int count_region_hits(EngineImpl* im, size_t n, PileupFold<K>& pf) {
    XBases xb; memset(&xb, 0, sizeof xb);
    HIP_TRY(hipMemsetAsync(im->d_ctl + CTL_X0, 0, XSHARD * CTL_STRIDE * sizeof(unsigned long long), im->s_comp));
    launch_expand<K, false>(im, n, pf, xb, -1);
    const unsigned long long* h;
    if (int rc = read_ctl_words(im, CTL_X0, XSHARD * CTL_STRIDE, h)) return rc;
    pf.n2 = 0; pf.cap2 = 0;
    unsigned long long uor2 = 0;
    for (int sh = 0; sh < XSHARD; sh++) { pf.tot2[sh] = h[sh * CTL_STRIDE]; pf.n2 += pf.tot2[sh]; pf.cap2 = std::max(pf.cap2, pf.tot2[sh]); }
    for (int sh = 0; sh < NSHARD; sh++) uor2 |= im->h_ctl[ctl_umi_or(sh)];
    pf.used2 = uor2 ? 64 - __builtin_clzll(uor2) : 0;            // UMI-field bits in use by the reads the join accepted (a superset of the region-level keys')
    pf.cap2 = (pf.cap2 + 63) & ~63ull;
    return 0;
}

// workspace 2 for the region-level hits, carved whole (fold_ws.h region_carve): everything from here to the COO blocks
template <class K>
static int reserve_region_hits(EngineImpl* im, bool try_part, PileupFold<K>& pf) {
    typedef typename PileupFold<K>::V2 V2;
    RegionWs& w = pf.w2;
    pf.tmpb2 = sort_tmp_bytes<K, V2>(pf.n2, im->ubits + im->cbits + im->rbits);
    const size_t part_bytes = partition_sort_scratch(im, pf.n2, (size_t)std::max(im->n_regions, 1));
    if (int rc = pf_carve(im, im->ws2, true, [&](Arena& ar) { region_carve(ar, pf.n2, (size_t)pf.cap2, sizeof(K), sizeof(V2), pf.tmpb2, part_bytes, try_part, w); }, WS_REGION_FULL)) return rc;
    pf.k2 = (K*)w.k2; pf.k2b = (K*)w.k2b; pf.v2 = (V2*)w.v2; pf.v2b = (V2*)w.v2b;
    HIP_TRY(hipMemsetAsync(w.acc, 0, 2 * w.stride2 * sizeof(uint32_t), im->s_comp));   // (the half that k_hap_items' packed sums use; the rest in sum_sorted_runs, if it runs)
    return 0;
}

// 64-bit keys: k_expand writes its 16 slices at a fixed stride and the partition sort (fold_partition.h) orders them; when it hands
// back PF_FALLBACK (a (region, cell group) deeper than an item), or with 128-bit keys, k_expand writes the slices back to back and
// the library radix sort orders them.  XCK_PILEUP_SORT=radix forces the latter.
// *summed: k_hap_items has left the per-run sums (packed) in acc and the run keys in k2; otherwise the sorted hits are in k2b / v2b
template <class K>
static int sort_region_hits(EngineImpl* im, size_t n, bool try_part, PileupFold<K>& pf, bool* summed) {
    typedef typename PileupFold<K>::V2 V2;
    int rc;
    const int top = im->ubits + im->cbits + im->rbits;
    const size_t n2 = pf.n2;
    XBases xb; memset(&xb, 0, sizeof xb);
    *summed = false;
    if constexpr (sizeof(K) == 8) {
        if (try_part) {
            for (int sh = 0; sh < XSHARD; sh++) xb.base[sh] = (unsigned long long)sh * pf.cap2;
            // (XCK_PILEUP_HAP=sorted: sort the items completely and run k_hap_class / k_hap_sum on them, as after the radix sort;
            //  XCK_PILEUP_HAP=values: keep the haplotype class in a value word beside the key, as when the UMI field has no two free bits)
            const bool hap_items = im->eng->knobs.pileup_hap != 1;
            const int pack_shift = hap_items && im->eng->knobs.pileup_hap != 2 && pf.used2 + 2 <= im->ubits ? pf.used2 : -1;
            launch_expand<K, true>(im, n, pf, xb, pack_shift);
            HIP_TRY(hipGetLastError());
            const HapItemsOut ho{(unsigned long long*)pf.w2.acc, (unsigned long long*)pf.k2, pack_shift};   // (the packed sums use the first half of acc)
            im->ws2.off = pf.w2.scratch_at;                            // its scratch: the shared region (the radix sort's tmp, should it hand over)
            rc = pileup_partition_sort(im, im->ws2, false, key_layout<unsigned long long>(im), (const unsigned long long*)pf.k2, pack_shift >= 0 ? (const uint64_t*)nullptr : (const uint64_t*)pf.v2, (size_t)pf.cap2, pf.tot2,
                                       (uint32_t)std::max(im->n_regions, 1), n2, (unsigned long long*)pf.k2b, pack_shift >= 0 ? (uint64_t*)nullptr : (uint64_t*)pf.v2b, hap_items ? &ho : nullptr);
            if (rc == 0) { *summed = hap_items; im->pileup_sort2_path = hap_items ? 1 : 3; return 0; }
            else if (rc != PF_FALLBACK) return rc;
            else {                                                 // the cursors of the emit pass start again
                for (int sh = 0; sh < XSHARD; sh++) HIP_TRY(hipMemsetAsync(im->d_ctl + CTL_X0 + sh * CTL_STRIDE + 1, 0, sizeof(unsigned long long), im->s_comp));
            }
        }
    }
    im->pileup_sort2_path = 2;
    void* tmp2 = pf.w2.scratch;                                        // (the kernels that used it as the partition sort's scratch are ordered before the sort)
    { unsigned long long at = 0; for (int sh = 0; sh < XSHARD; sh++) { xb.base[sh] = at; at += pf.tot2[sh]; } }
    launch_expand<K, true>(im, n, pf, xb, -1);
    HIP_TRY(hipGetLastError());
    return sort_run<K, V2>(im, tmp2, pf.tmpb2, pf.k2, pf.k2b, pf.v2, pf.v2b, n2, top);
}

// sorted keys: classes per (row, cell, UMI) run, sums per (row, cell) run; the run keys go to k2, the number of runs to CTL_SCRATCH
template <class K>
static int sum_sorted_runs(EngineImpl* im, const PileupFold<K>& pf) {
    typedef typename PileupFold<K>::V2 V2;
    const KeyLayout<K> kl = key_layout<K>(im);
    const RegionWs& w = pf.w2;
    const size_t n2 = pf.n2;
    HIP_TRY(hipMemsetAsync(w.acc + 2 * w.stride2, 0, 2 * w.stride2 * sizeof(uint32_t), im->s_comp));
    const unsigned gs2 = (unsigned)((n2 + 255) / 256);
    const size_t nt2 = (n2 + FD_TILE - 1) / FD_TILE;
    HIP_TRY(hipMemsetAsync(w.long2, 0, sizeof(unsigned long long), im->s_comp));
    hipLaunchKernelGGL((k_hap_class<K, V2>), dim3(gs2), dim3(256), 0, im->s_comp, (const K*)pf.k2b, (const V2*)pf.v2b, (long long)n2, w.cls, w.long2);
    hipLaunchKernelGGL((k_hap_class_long<K, V2>), dim3(256), dim3(256), 0, im->s_comp, (const K*)pf.k2b, (const V2*)pf.v2b, (long long)n2, (const unsigned long long*)w.long2, w.cls);
    hipLaunchKernelGGL((k_fold_heads<K>), dim3((unsigned)nt2), dim3(FD_BLOCK), 0, im->s_comp, (const K*)pf.k2b, (long long)n2, kl, w.d_blk2);
    hipLaunchKernelGGL(k_cp_scan, dim3(1), dim3(1024), 0, im->s_comp, w.d_blk2, (long long)nt2, w.d_off2, im->d_ctl + CTL_SCRATCH);
    hipLaunchKernelGGL((k_hap_sum<K>), dim3((unsigned)nt2), dim3(FD_BLOCK), 0, im->s_comp, (const K*)pf.k2b, (const uint8_t*)w.cls, (long long)n2, kl,
                       (const unsigned long long*)w.d_off2, pf.k2, w.acc, (long long)w.stride2);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The pileup fold in two stages, cut where the dependence on the regions ends.
// fold_molecules: the hits sorted by key, the base the first read of every (SNP, cell, UMI) shows, the tallies per SNP.  It reads
// nothing but the hits and the SNP positions, and what it leaves (EngineImpl::mol_keys / mol_al / mol_n, d_tally) stays valid until
// the next reset.
template <class K>
static int fold_molecules(EngineImpl* im, size_t n) {
    int rc;
    const int top = im->ubits + im->cbits + im->rbits;
    PileupFold<K> pf{};
    const size_t tmpb = sort_tmp_bytes<K, uint64_t>(n, top);
    im->mol_valid = false;
    // (the join kernel splits the hits for 64-bit keys only - split_mode() - so the split path is not instantiated for 128-bit keys)
    const bool split = sizeof(K) == 8 && split_mode(im);
    if ((rc = pf_carve(im, im->ws1, true, [&](Arena& ar) { molecule_carve(ar, n, sizeof(K), tmpb, (size_t)im->n_snps_sorted, split, pf.w1); }, WS_MOLECULE_FULL))) return rc;
    if ((rc = sort_pileup_hits<K>(im, n, tmpb, pf))) return rc;
    HIP_TRY(hipMemsetAsync(im->d_tally, 0, std::max<size_t>((size_t)im->n_snps_sorted * 5, 1) * sizeof(uint32_t), im->s_comp));
    HIP_TRY(hipMemsetAsync(pf.w1.long_runs, 0, sizeof(unsigned long long), im->s_comp));
    if (im->d_mol) {                                                   // (XCK_F_UMI_CONSENSUS: the vote instead of the first read, no claims)
        HIP_TRY(hipMemsetAsync(im->d_mol, 0, MOL_BUF_WORDS * sizeof(unsigned long long), im->s_comp));
        if constexpr (sizeof(K) == 8) rc = split ? consensus_split<K>(im, n, pf) : consensus_plain<K>(im, n, pf);
        else rc = consensus_plain<K>(im, n, pf);
    } else
    if constexpr (sizeof(K) == 8) rc = split ? first_reads_split<K>(im, n, pf) : first_reads_plain<K>(im, n, pf);
    else rc = first_reads_plain<K>(im, n, pf);
    if (rc) return rc;
    im->mol_keys = pf.keys; im->mol_al = pf.w1.al; im->mol_n = n; im->mol_valid = true;
    return 0;
}

// fold_regions: everything that depends on the regions, REF / ALT, the haplotype indices, the exclusion pairs and the per-SNP filters -
// the fan-out of the molecules to the regions of their SNP, the haplotype algebra per (region, cell), the COO blocks and their
// copy-out.  Allocates from workspace 2 only, so it runs again under new tables (xck_refold) on what fold_molecules left.
template <class K>
static int fold_regions(EngineImpl* im) {
    int rc;
    const size_t n = im->mol_n;
    PileupFold<K> pf{};
    pf.keys = (const K*)im->mol_keys; pf.w1.al = im->mol_al;
    for (int m = 1; m < 4; m++) { im->res_nnz[m] = 0; im->d_res[m] = nullptr; }
    if (n == 0) return 0;
    if ((rc = count_region_hits<K>(im, n, pf))) return rc;
    if (pf.n2) {
        const bool try_part = sizeof(K) == 8 && !im->eng->knobs.pileup_radix;
        bool summed = false;
        if ((rc = reserve_region_hits<K>(im, try_part, pf))) return rc;
        if ((rc = sort_region_hits<K>(im, n, try_part, pf, &summed))) return rc;
        HapSrc hs{(const uint32_t*)pf.w2.acc, (long long)pf.w2.stride2, (const unsigned long long*)nullptr, (long long)pf.n2, im->no_dup_hap, (const unsigned long long*)pf.w2.acc};   // k_hap_items: runs staged (packed) at their items' offsets
        if (!summed) {
            if ((rc = sum_sorted_runs<K>(im, pf))) return rc;
            hs.n_runs = (const unsigned long long*)(im->d_ctl + CTL_SCRATCH); hs.packed = nullptr;
        }
        if ((rc = compact_coo<K>(im, im->ws2, pf.w2, hs, pf.k2, pf.n2, key_layout<K>(im), 1))) return rc;   // AD, DP, OTH together, from the per-run sums
    }
    return 0;
}

template <class K>
static int finish_pileup(EngineImpl* im, size_t n) {
    Timer tm{im, im->ev0, im->ev1};
    int rc;
    if ((rc = tm.start())) return rc;
    if ((rc = fold_molecules<K>(im, n))) return rc;
    if ((rc = fold_regions<K>(im))) return rc;
    return tm.stop(&im->st.ms_sort);
}

template <class K>
static int finish_t(EngineImpl* im) {
    clear_stale_error("finish", im->eng->knobs.debug_timing);
    const size_t n = im->cursor;
    im->d_tally_cur = nullptr; im->d_cell_bits = nullptr;          // (a finish counts every cell)
    for (int m = 0; m < 4; m++) { im->res_nnz[m] = 0; im->d_res[m] = nullptr; }
    im->mol_stats_valid = false; im->uf_stats_valid = false; im->uc_stats_valid = false;
    if (im->umi_collapse) for (long long& v : im->uc_stats) v = 0;
    { int64_t acc = 0; for (int sh = 0; sh < NSHARD; sh++) acc += (int64_t)im->h_ctl[ctl_accepted(sh)];
      im->st.n_hits = acc; }                          // accepted pairs (before the LDS de-duplication)
    im->st.n_hits_unique = (int64_t)(n + im->ncursor);   // keys that reached HBM
    join_stamps_report(im);
    if (n == 0) { im->mol_keys = nullptr; im->mol_al = nullptr; im->mol_n = 0; im->mol_valid = im->mode == XCK_MODE_BAF; im->mol_stats_valid = im->d_mol != nullptr; im->uf_stats_valid = im->d_uf_rank != nullptr; im->uc_stats_valid = im->umi_collapse; return 0; }   // (the counters are zero since the reset)
    const int rc = im->mode == XCK_MODE_BASEFC ? finish_basefc<K>(im, n) : finish_pileup<K>(im, n);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(im->s_comp));
    im->mol_stats_valid = im->d_mol != nullptr; im->uf_stats_valid = im->d_uf_rank != nullptr; im->uc_stats_valid = im->umi_collapse;
    return 0;
}

// fold everything on the GPU and ENQUEUE the copy-out of the matrices; does not wait for the copy
int engine_finish_async(EngineImpl* im) {
    HIP_TRY(hipSetDevice(im->device));
    int rc = launch_queue(im, -1); if (rc) return rc;
    rc = complete_pending(im); if (rc) return rc;
    if (!im->finished) {
        // a finish that failed half-way may have overwritten the accumulated keys (the folds reuse the shard slices as scratch): it
        // cannot be tried again on them
        if (im->fold_failed) { im->eng->err = "an earlier xck_finish failed inside the fold: the accumulated hits are gone (call xck_reset)"; return XCK_E_STATE; }
        im->copy_timed = false;
        rc = im->key_bits == 64 ? finish_t<uint64_t>(im) : finish_t<u128>(im);
        if (rc) { im->fold_failed = true; hipStreamSynchronize(im->s_comp); hipStreamSynchronize(im->s_copy); return rc; }   // (nothing of the failed fold is still running when the arenas are reused)
        im->finished = true; im->copy_pending = true;
    }
    return 0;
}

// wait for the copy-out of the last fold and hand out the host blocks
static int result_host(EngineImpl* im, xck_result* out) {
    if (im->copy_pending) {
        const bool dbg = im->eng->knobs.debug_timing;
        const auto t0_ = std::chrono::steady_clock::now();
        const hipError_t q_ = dbg ? hipStreamQuery(im->s_copy) : hipSuccess;
        HIP_TRY(hipStreamSynchronize(im->s_copy));
        if (dbg) fprintf(stderr, "[xck] finish: copy stream %s at entry, waited %.3f ms\n", q_ == hipSuccess ? "idle" : "busy",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count());
        if (im->copy_timed) { float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, im->ev_c0, im->ev_c1)); im->st.ms_d2h += ms; }
        im->copy_pending = false;
    }
    memset(out, 0, sizeof *out);
    xck_coo* dst[4] = { &out->count, &out->ad, &out->dp, &out->oth };
    for (int m = 0; m < 4; m++) {
        const size_t z = im->res_nnz[m];
        dst[m]->nnz = (int64_t)z;
        dst[m]->row = im->h_res[m]; dst[m]->col = im->h_res[m] ? im->h_res[m] + z : nullptr; dst[m]->val = im->h_res[m] ? im->h_res[m] + 2 * z : nullptr;
    }
    return 0;
}
int engine_finish(EngineImpl* im, xck_result* out) {
    if (int rc = engine_finish_async(im)) return rc;
    return result_host(im, out);
}

// device-resident copy of the last finish() result (for device-to-device exchanges such as the RCCL gather)
int engine_result_device(EngineImpl* im, xck_result* out) {
    if (!im->finished) { im->eng->err = "xck_get_result_device before xck_finish"; return XCK_E_STATE; }
    memset(out, 0, sizeof *out);
    xck_coo* dst[4] = { &out->count, &out->ad, &out->dp, &out->oth };
    for (int m = 0; m < 4; m++) {
        const size_t z = im->res_nnz[m];
        dst[m]->nnz = (int64_t)z;
        if (z && im->d_res[m]) { dst[m]->row = im->d_res[m]; dst[m]->col = im->d_res[m] + z; dst[m]->val = im->d_res[m] + 2 * z; }
    }
    return 0;
}

int snp_verdicts(EngineImpl* im, uint32_t* d_kept) {
    const uint32_t n = (uint32_t)im->n_snps_sorted;
    if (!n) return 0;
    hipLaunchKernelGGL(k_snp_verdict, dim3((n + 255) / 256), dim3(256), 0, im->s_comp, cur_tally(im), (const uint32_t*)im->d_snp_info, n, im->sf, d_kept);
    HIP_TRY(hipGetLastError());
    return 0;
}

#include "coo_call.h"
#include "refold.h"
#include "snp_counts.h"
#include "group_counts.h"

int finish_init(EngineImpl* im) {
    // the hash fold needs 64 KB of dynamic LDS: raise the limit on THIS engine's device (a per-process flag would leave every
    // device but the first at the 64 KB default and race between engines created from different threads)
    HIP_TRY(hipFuncSetAttribute((const void*)k_fold_emit_unsorted, hipFuncAttributeMaxDynamicSharedMemorySize, FU_SLOTS * 8));
    HIP_TRY(hipFuncSetAttribute((const void*)k_pf_bucket, hipFuncAttributeMaxDynamicSharedMemorySize, pf_bucket_lds(PF_SB_MAX)));
    return 0;
}

}  // namespace xck
