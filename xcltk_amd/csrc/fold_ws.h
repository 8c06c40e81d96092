// fold_ws.h - the device workspaces of the finish path that are not the partition fold's: the arena they are cut from, and per
// workspace ONE struct of pointers with ONE carve function that holds its get<>() calls.  A carve function runs twice (finish.hip, through
// fold_partition.h pf_carve): on an arena without memory, which yields the workspace's size, then on the real arena begun with that
// many bytes.  There is no second statement of any size.  Plain numbers in, pointers out; no HIP and no EngineImpl, so that a host
// program can run the same functions over a grid of inputs (tools/asan/fold_ws_check.cpp).
//
// A block whose size is known only after a device read-back (the COO blocks) is reserved at its upper bound and its offset kept
// (coo_at); after the read-back the caller sets Arena::off to that offset and gets the exact sizes, which cannot end further out.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace xck {
// grow-only device workspace: finish() sub-allocates from it instead of hipMalloc/hipFree per call
struct Arena {
    char* base = nullptr; size_t cap = 0, off = 0;
    template <class T> T* get(size_t n) {
        off = (off + 255) & ~size_t(255);
        T* p = reinterpret_cast<T*>(base + off);
        off += std::max<size_t>(n, 1) * sizeof(T);
        return off <= cap ? p : nullptr;
    }
};

// what the carve functions share with the kernels that work on the blocks (finish.hip holds its own constants against these)
constexpr size_t WS_TILE = 2048;          // keys per tile of k_fold_heads / k_hap_count (FD_TILE == CP_TILE)
constexpr size_t WS_RUN_WALK = 64;        // at most one long run per so many hits (RUN_WALK)
constexpr size_t WS_SLICES = 16;          // slices k_expand writes at a fixed stride for the partition sort (XSHARD)

// ---- basefc, the radix-sort fold: workspace 1 ----------------------------------------------------------------------------------------
struct RadixFoldWs {
    void *alt, *tmp;                                   // n keys beside the shard slices (the sort's ping-pong partner); the sort's scratch
    uint32_t* d_blk; unsigned long long* d_off;        // per tile of WS_TILE keys: run heads, their exclusive scan
    size_t coo_at;                                     // [row | col | val] of at most n non-zeros
};
inline void radix_fold_carve(Arena& ar, size_t n, size_t key_bytes, size_t tmp_bytes, RadixFoldWs& w) {
    const size_t nt = (n + WS_TILE - 1) / WS_TILE;
    w.alt = ar.get<char>(n * key_bytes); w.tmp = ar.get<char>(tmp_bytes);
    w.d_blk = ar.get<uint32_t>(nt); w.d_off = ar.get<unsigned long long>(nt);
    w.coo_at = ar.off; ar.get<int32_t>(n * 3);
}

// ---- basefc, unique-feature molecules (umi_feature.h): workspace 1, ahead of the radix-sort fold, which begins the arena anew ----------
struct UniqueFeatureWs {
    void *a, *b, *tmp;                                 // n molecule-major keys: the sort's input, later the distinct keys D; the sorted keys; the sort's scratch
    uint8_t* drop;                                     // per key of D: 1 = its molecule has another row on the contig
    uint32_t* d_blk; unsigned long long* d_off;        // per tile of WS_TILE keys, three rows of nt: [distinct keys, later survivors | molecules | multi-feature molecules] and their scans
};
inline void unique_feature_carve(Arena& ar, size_t n, size_t key_bytes, size_t tmp_bytes, UniqueFeatureWs& w) {
    const size_t nt = (n + WS_TILE - 1) / WS_TILE;
    w.a = ar.get<char>(n * key_bytes); w.b = ar.get<char>(n * key_bytes); w.tmp = ar.get<char>(tmp_bytes);
    w.drop = ar.get<uint8_t>(n);
    w.d_blk = ar.get<uint32_t>(3 * nt); w.d_off = ar.get<unsigned long long>(3 * nt);
}

// ---- basefc, 1-mismatch UMI collapsing (umi_collapse.h): workspace 1; it ends with the radix-sort fold's COO block, counted in place ----
constexpr size_t WS_UC_SMALL = 64;        // a group of more keys than this is listed for k_uc_big (UC_SMALL)
constexpr size_t WS_UC_ROWS = 5;          // rows of per-tile words of k_uc_small (UCW_ROWS)
struct UmiCollapseWs {
    void *a, *b, *tmp;                                 // n packed keys: the sort's input, later the distinct keys D; the sorted keys, later one parent word per key of D; the sort's scratch
    uint8_t* root;                                     // per key of D: 1 = the root of its component
    unsigned long long* big_start; uint32_t* big_size; // per group of more than WS_UC_SMALL keys (at most big_cap): its first key in D, its keys
    uint32_t* big_words; unsigned long long* big_off;  // ... three rows of big_cap: [changed | keys if medium | keys if giant] and their scans
    size_t big_cap;
    uint32_t* d_blk; unsigned long long* d_off;        // per tile of WS_TILE keys, WS_UC_ROWS rows of nt: the counters of k_uc_small, later the roots, later the fold's run heads; their scans
    size_t coo_at;                                     // [row | col | val] of at most n non-zeros
};
inline void umi_collapse_carve(Arena& ar, size_t n, size_t key_bytes, size_t tmp_bytes, UmiCollapseWs& w) {
    const size_t nt = (n + WS_TILE - 1) / WS_TILE;
    w.big_cap = n / (WS_UC_SMALL + 1) + 1;
    w.a = ar.get<char>(n * key_bytes); w.b = ar.get<char>(n * key_bytes); w.tmp = ar.get<char>(tmp_bytes);
    w.root = ar.get<uint8_t>(n);
    w.big_start = ar.get<unsigned long long>(w.big_cap); w.big_size = ar.get<uint32_t>(w.big_cap);
    w.big_words = ar.get<uint32_t>(3 * w.big_cap); w.big_off = ar.get<unsigned long long>(3 * w.big_cap);
    w.d_blk = ar.get<uint32_t>(WS_UC_ROWS * nt); w.d_off = ar.get<unsigned long long>(WS_UC_ROWS * nt);
    w.coo_at = ar.off; ar.get<int32_t>(n * 3);
}

// ---- pileup, the molecule stage: workspace 1 -----------------------------------------------------------------------------------------
struct MoleculeWs {
    void* alt; uint64_t* valt; void* tmp;              // n keys and values: the sorted hits, or the radix sort's input; the radix sort's scratch
    uint8_t* al;                                       // per sorted hit: what the first read of its key shows at the SNP
    unsigned long long* long_runs;                     // [0] = count, then the heads of the runs longer than WS_RUN_WALK
    // split mode only (null otherwise): fetch order of every key's first read; first / one-past-last hit per SNP (one block, row_hi =
    // row_lo + SNPs); one filter word per key along the sorted stream; first hit per block of 32 SNPs
    uint64_t* ordv; unsigned long long *row_lo, *row_hi, *bloom, *blk_lo;
};
inline void molecule_carve(Arena& ar, size_t n, size_t key_bytes, size_t tmp_bytes, size_t n_snps, bool split, MoleculeWs& w) {
    const size_t ns = std::max<size_t>(n_snps, 1);
    w.alt = ar.get<char>(n * key_bytes); w.valt = ar.get<uint64_t>(n); w.tmp = ar.get<char>(tmp_bytes);
    w.al = ar.get<uint8_t>(n);
    w.long_runs = ar.get<unsigned long long>(n / WS_RUN_WALK + 2);
    w.ordv = nullptr; w.row_lo = w.row_hi = w.bloom = w.blk_lo = nullptr;
    if (!split) return;
    w.ordv = ar.get<uint64_t>(n);
    w.row_lo = ar.get<unsigned long long>(2 * ns); w.row_hi = w.row_lo + ns;
    w.bloom = ar.get<unsigned long long>(n);
    w.blk_lo = ar.get<unsigned long long>(((ns + 31) >> 5) + 1);
}

// ---- pileup, the region stage: workspace 2 -------------------------------------------------------------------------------------------
struct RegionWs {
    void *k2, *v2;                                     // the n2 region-level hits as k_expand writes them: try_part, WS_SLICES slices of slice_cap entries; else back to back
    void *k2b, *v2b;                                   // sorted
    uint8_t* cls; uint32_t* acc; size_t stride2;       // haplotype class per hit; per run, stride2 = n2 rounded up to 8 apart: REF-hap, ALT-hap, either, other-only keys
    void* scratch; size_t scratch_at;                  // ONE region: the partition sort carves its scratch at scratch_at, the radix sort that follows a hand-over uses it as tmp
    uint32_t* d_blk2; unsigned long long *d_off2, *long2;   // sorted hits: run heads per tile and their scan; [0] = count, then the (row, cell, UMI) runs longer than WS_RUN_WALK
    uint32_t* d_blk; unsigned long long* d_off;        // compaction: non-zeros per tile of WS_TILE runs and their scan, for AD | DP | OTH
    size_t coo_at;                                     // three blocks [row | col | val] of at most n2 non-zeros each
};
inline void region_carve(Arena& ar, size_t n2, size_t slice_cap, size_t key_bytes, size_t val_bytes, size_t tmp_bytes, size_t part_bytes, bool try_part, RegionWs& w) {
    const size_t n2s = try_part ? std::max(WS_SLICES * slice_cap, n2) : n2, nt = (n2 + WS_TILE - 1) / WS_TILE;
    const size_t scratch = std::max(tmp_bytes, try_part ? part_bytes : size_t(0));
    w.k2 = ar.get<char>((n2s + 8) * key_bytes); w.k2b = ar.get<char>(n2 * key_bytes); w.v2 = ar.get<char>(n2s * val_bytes); w.v2b = ar.get<char>(n2 * val_bytes);
    w.cls = ar.get<uint8_t>(n2);
    w.stride2 = (n2 + 7) & ~size_t(7);                 // (k_hap_count / k_hap_scatter read eight runs with two 16-byte loads)
    w.acc = ar.get<uint32_t>(4 * w.stride2);
    w.scratch = ar.get<char>(scratch); w.scratch_at = ar.off - std::max<size_t>(scratch, 1);
    w.d_blk2 = ar.get<uint32_t>(nt); w.d_off2 = ar.get<unsigned long long>(nt); w.long2 = ar.get<unsigned long long>(n2 / WS_RUN_WALK + 2);
    w.d_blk = ar.get<uint32_t>(3 * nt); w.d_off = ar.get<unsigned long long>(3 * nt);
    w.coo_at = ar.off; for (int y = 0; y < 3; y++) ar.get<int32_t>(n2 * 3);
}
}  // namespace xck
