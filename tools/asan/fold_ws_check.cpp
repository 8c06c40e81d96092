// Host-only check of the fold workspaces (csrc/fold_ws.h: radix_fold_carve, unique_feature_carve, umi_collapse_carve, molecule_carve, region_carve) under AddressSanitizer /
// UBSan.  For every point of a grid of sizes each function runs as the engine runs it - on an arena without memory, which gives the
// size, then on a malloc'ed block of exactly that size - and every block it hands out must be non-null, at a multiple of 256 bytes
// from the base, inside the block and disjoint from every other; each is then written over its full stated extent, the blocks taken
// after a read-back (the COO blocks, the partition sort's scratch) at their remembered offsets.  The carved size is also held
// against the hand-counted formula the function replaced, which lives on here as the bound it was: the new size never exceeds it.
// No device, no HIP call.
//   make -C tools/asan fold_ws_check && tools/asan/fold_ws_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../xcltk_amd/csrc/fold_ws.h"

using namespace xck;
typedef unsigned long long u64;

// ---- the formulas finish.hip held before fold_ws.h (n: hits, kb / vb: key / value bytes, tmpb: the radix sort's scratch) ----
static size_t old_need_radix(size_t n, size_t kb, size_t tmpb) {
    const size_t nb = (n + 2047) / 2048;
    return n * kb + tmpb + nb * 12 + n * 12 + (1 << 20);
}
static size_t old_need_molecule(size_t n, size_t kb, size_t tmpb, size_t n_snps) {
    return n * kb + n * 8 + tmpb + n + n / 8 + n * 8 + std::max<size_t>(n_snps, 1) * 17 + std::max<size_t>(n * 8, 8192) + (1 << 16);
}
static size_t old_need_region(size_t n2, size_t cap2, size_t kb, size_t vb, size_t tmpb2, size_t part_scratch, bool try_part) {
    const size_t n2s = try_part ? std::max<size_t>(16 * cap2, n2) : n2, nb2 = (n2 + 2047) / 2048, part_bytes = try_part ? part_scratch : 0;
    return (n2s + 8) * kb + n2 * kb + (n2s + 8) * vb + n2 * vb + n2 + 4 * (n2 + 8) * 4 + std::max(tmpb2, part_bytes) + ((n2 + 2047) / 2048) * 12 + (n2 / 64 + 2) * 8
         + 3 * (nb2 * 12 + n2 * 12) + (1 << 16);
}

// ---- the blocks of a carved workspace with their stated extents ----
struct Block { const char* name; const void* p; size_t bytes; };
static int g_fail = 0;
static long g_points = 0, g_blocks = 0;
static void fail(const char* what, const char* ws, const char* block, size_t n) {
    if (g_fail++ < 20) fprintf(stderr, "%s: %s %s (n = %zu)\n", ws, block, what, n);
}
// non-null, aligned, inside [base, base + size), pairwise disjoint; then written
static void check_blocks(const char* ws, char* base, size_t size, const std::vector<Block>& bl, size_t n) {
    for (const Block& b : bl) {
        const char* p = (const char*)b.p;
        g_blocks++;
        if (!p) { fail("is null", ws, b.name, n); continue; }
        if (p < base || p + b.bytes > base + size) { fail("leaves the workspace", ws, b.name, n); continue; }
        if ((size_t)(p - base) % 256) fail("is not 256-byte aligned", ws, b.name, n);
        for (const Block& o : bl) if (&o != &b && o.p && p < (const char*)o.p + o.bytes && (const char*)o.p < p + b.bytes) fail("overlaps another block", ws, b.name, n);
        memset((void*)p, 0xA5, b.bytes);
    }
}
template <class F> static size_t measure(F carve) { Arena m; m.cap = ~size_t(0); carve(m); return m.off; }
// carve(ar) on a block of exactly the measured size; blocks(ar) lists what it handed out (and takes the read-back blocks)
template <class F, class G> static void run_point(const char* ws, size_t n, size_t old_need, bool measure_only, F carve, G blocks) {
    const size_t size = measure(carve);
    g_points++;
    if (size > old_need) { fail("workspace larger than the formula it replaced", ws, "", n); fprintf(stderr, "  %zu > %zu\n", size, old_need); }
    if (measure_only) return;
    Arena ar; ar.base = (char*)malloc(size); ar.cap = size;
    if (!ar.base) { fprintf(stderr, "malloc(%zu) failed\n", size); exit(2); }
    carve(ar);
    if (ar.off != size) fail("second carve ends elsewhere than the first", ws, "", n);
    check_blocks(ws, ar.base, size, blocks(ar), n);
    if (ar.off > ar.cap) fail("a read-back block ends outside the workspace", ws, "", n);
    free(ar.base);
}

static void radix_point(size_t n, size_t kb, size_t tmpb, bool measure_only) {
    RadixFoldWs w;
    run_point("radix fold", n, old_need_radix(n, kb, tmpb), measure_only, [&](Arena& ar) { radix_fold_carve(ar, n, kb, tmpb, w); }, [&](Arena& ar) {
        const size_t nt = (n + WS_TILE - 1) / WS_TILE;
        std::vector<Block> bl = { {"alt", w.alt, n * kb}, {"tmp", w.tmp, tmpb}, {"d_blk", w.d_blk, nt * 4}, {"d_off", w.d_off, nt * 8} };
        for (size_t total : { n, n / 2 + 1 }) {                            // the COO block after the read-back: every key a non-zero, or fewer
            if (total > n) continue;
            ar.off = w.coo_at;
            std::vector<Block> b2 = bl; b2.push_back({"coo", ar.get<int32_t>(total * 3), total * 12});
            check_blocks("radix fold", ar.base, ar.cap, b2, n);
        }
        return bl;
    });
}
// (no formula came before this one: the bound is the sum of its blocks' stated extents plus one alignment gap each)
static void unique_feature_point(size_t n, size_t kb, size_t tmpb, bool measure_only) {
    UniqueFeatureWs w;
    const size_t nt = (n + WS_TILE - 1) / WS_TILE;
    const size_t bound = 2 * std::max<size_t>(n * kb, 1) + std::max<size_t>(tmpb, 1) + std::max<size_t>(n, 1) + std::max<size_t>(3 * nt, 1) * 12 + 6 * 256;
    run_point("unique-feature stage", n, bound, measure_only, [&](Arena& ar) { unique_feature_carve(ar, n, kb, tmpb, w); }, [&](Arena&) {
        return std::vector<Block>{ {"a", w.a, n * kb}, {"b", w.b, n * kb}, {"tmp", w.tmp, tmpb}, {"drop", w.drop, n}, {"d_blk", w.d_blk, 3 * nt * 4}, {"d_off", w.d_off, 3 * nt * 8} };
    });
}
// (no formula came before this one either)
static void umi_collapse_point(size_t n, size_t kb, size_t tmpb, bool measure_only) {
    UmiCollapseWs w;
    const size_t nt = (n + WS_TILE - 1) / WS_TILE, nbig = n / (WS_UC_SMALL + 1) + 1;
    const size_t bound = 2 * std::max<size_t>(n * kb, 1) + std::max<size_t>(tmpb, 1) + std::max<size_t>(n, 1) + nbig * (8 + 4 + 12 + 24) + std::max<size_t>(WS_UC_ROWS * nt, 1) * 12
                         + std::max<size_t>(n * 3, 1) * 4 + 11 * 256;
    run_point("UMI collapsing stage", n, bound, measure_only, [&](Arena& ar) { umi_collapse_carve(ar, n, kb, tmpb, w); }, [&](Arena& ar) {
        if (w.big_cap != nbig) { fprintf(stderr, "FAIL: UMI collapsing stage n=%zu: big_cap %zu, expected %zu\n", n, w.big_cap, nbig); exit(1); }
        ar.off = w.coo_at;
        return std::vector<Block>{ {"a", w.a, n * kb}, {"b", w.b, n * kb}, {"tmp", w.tmp, tmpb}, {"root", w.root, n}, {"big_start", w.big_start, nbig * 8}, {"big_size", w.big_size, nbig * 4},
                                   {"big_words", w.big_words, 3 * nbig * 4}, {"big_off", w.big_off, 3 * nbig * 8}, {"d_blk", w.d_blk, WS_UC_ROWS * nt * 4}, {"d_off", w.d_off, WS_UC_ROWS * nt * 8},
                                   {"coo", ar.get<int32_t>(n * 3), n * 3 * 4} };
    });
}
static void molecule_point(size_t n, size_t kb, size_t tmpb, size_t n_snps, bool split, bool measure_only) {
    MoleculeWs w;
    run_point("molecule stage", n, old_need_molecule(n, kb, tmpb, n_snps), measure_only, [&](Arena& ar) { molecule_carve(ar, n, kb, tmpb, n_snps, split, w); }, [&](Arena&) {
        const size_t ns = std::max<size_t>(n_snps, 1);
        std::vector<Block> bl = { {"alt", w.alt, n * kb}, {"valt", w.valt, n * 8}, {"tmp", w.tmp, tmpb}, {"al", w.al, n}, {"long_runs", w.long_runs, (n / WS_RUN_WALK + 2) * 8} };
        if (split) {
            bl.insert(bl.end(), { {"ordv", w.ordv, n * 8}, {"row_lo", w.row_lo, ns * 8}, {"bloom", w.bloom, n * 8}, {"blk_lo", w.blk_lo, (((ns + 31) >> 5) + 1) * 8} });
            if (w.row_hi != w.row_lo + ns) fail("does not follow row_lo", "molecule stage", "row_hi", n);
            if (w.row_hi) memset(w.row_hi, 0x5A, ns * 8);                  // (one block with row_lo: carved as 2 * ns words)
        } else if (w.ordv || w.row_lo || w.row_hi || w.bloom || w.blk_lo) fail("is set without split mode", "molecule stage", "a split block", n);
        return bl;
    });
}
static void region_point(size_t n2, size_t cap2, size_t kb, size_t vb, size_t tmpb2, size_t partb, bool try_part, bool measure_only) {
    RegionWs w;
    run_point("region stage", n2, old_need_region(n2, cap2, kb, vb, tmpb2, partb, try_part), measure_only,
              [&](Arena& ar) { region_carve(ar, n2, cap2, kb, vb, tmpb2, partb, try_part, w); }, [&](Arena& ar) {
        const size_t n2s = try_part ? std::max(WS_SLICES * cap2, n2) : n2, nt = (n2 + WS_TILE - 1) / WS_TILE, scratch = std::max(tmpb2, try_part ? partb : size_t(0));
        if (w.stride2 < n2 || w.stride2 % 8 || w.stride2 > n2 + 7) fail("is not n2 rounded up to 8", "region stage", "stride2", n2);
        std::vector<Block> bl = { {"k2", w.k2, (n2s + 8) * kb}, {"k2b", w.k2b, n2 * kb}, {"v2", w.v2, n2s * vb}, {"v2b", w.v2b, n2 * vb}, {"cls", w.cls, n2}, {"acc", w.acc, 4 * w.stride2 * 4},
                                  {"scratch", w.scratch, scratch}, {"d_blk2", w.d_blk2, nt * 4}, {"d_off2", w.d_off2, nt * 8}, {"long2", w.long2, (n2 / WS_RUN_WALK + 2) * 8},
                                  {"d_blk", w.d_blk, 3 * nt * 4}, {"d_off", w.d_off, 3 * nt * 8} };
        // the declared shared region: the radix sort's tmp is its front; the partition sort carves at scratch_at (its bytes allow for one alignment gap)
        if (w.scratch && ar.base + w.scratch_at != (char*)w.scratch) fail("is not where scratch_at says", "region stage", "scratch", n2);
        if (try_part && partb >= 1024) {                                  // two gets that fill partb - 256 bytes, as partition_sort_carve's fill what it measured
            const size_t h1 = ((partb - 256) / 2) & ~size_t(255), h2 = partb - 256 - h1;
            ar.off = w.scratch_at;
            char* a = ar.get<char>(h1); char* b = ar.get<char>(h2);
            if (!a || !b || a != (char*)w.scratch || b + h2 > (char*)w.scratch + scratch) fail("does not hold the partition sort's carve", "region stage", "scratch", n2);
            else { memset(a, 0x11, h1); memset(b, 0x22, h2); }
        }
        for (size_t total : { n2, n2 / 3 + 1 }) {                          // the three COO blocks after the read-back
            if (total > n2) continue;
            ar.off = w.coo_at;
            std::vector<Block> b2 = bl;
            for (const char* name : { "ad", "dp", "oth" }) b2.push_back({name, ar.get<int32_t>(total * 3), total * 12});
            check_blocks("region stage", ar.base, ar.cap, b2, n2);
        }
        return bl;
    });
}

int main() {
    const size_t counts[] = { 0, 1, 7, 8, 9, 2047, 2049, 1000000, (size_t(1) << 32) - 1 };
    for (size_t n : counts) {
        const bool measure_only = n > 1000000;                            // (2^32 - 1 hits: hundreds of GB; the sizes alone)
        // sort-tmp and partition-scratch bytes on both sides of each other, and equal
        const size_t sizes[3][2] = { { 256 + n, 4096 + 2 * n }, { 4096 + 2 * n, 256 + n }, { size_t(1) << 20, size_t(1) << 20 } };
        for (size_t kb : { size_t(8), size_t(16) }) {
            const size_t vb = kb == 8 ? 8 : 1;                             // region-level values: words beside 64-bit keys, bytes beside 128-bit keys
            for (const auto& s : sizes) {
                radix_point(n, kb, s[0], measure_only);
                unique_feature_point(n, kb, s[0], measure_only);
                umi_collapse_point(n, kb, s[0], measure_only);
                for (size_t n_snps : { size_t(0), size_t(1) })
                    for (bool split : { false, true }) molecule_point(n, kb, s[0], n_snps, split, measure_only);
                // the widest of the 16 slices: even slices, or every hit in one (rounded up to 64 as count_region_hits does)
                for (size_t cap2 : { ((n + 15) / 16 + 63) & ~size_t(63), (n + 63) & ~size_t(63) })
                    for (bool try_part : { false, true }) region_point(n, cap2, kb, vb, s[0], s[1], try_part, measure_only);
            }
        }
    }
    // the sizes at the order of bench.py's default resident workload (380 M basefc keys; 29 M pileup hits with a base,
    // 1 M SNPs; taken here: as many region-level hits, evenly over the slices, 16 MiB of sort scratch, 64 MiB of partition scratch)
    { const size_t n_fc = 380123237, n_mol = 29000000, n2 = 29000000, cap2 = ((n2 + 15) / 16 + 63) & ~size_t(63), tmpb = size_t(16) << 20, partb = size_t(64) << 20;
      RadixFoldWs a; MoleculeWs b; RegionWs c;
      const size_t s_a = measure([&](Arena& ar) { radix_fold_carve(ar, n_fc, 8, tmpb, a); }), s_b = measure([&](Arena& ar) { molecule_carve(ar, n_mol, 8, tmpb, 1000000, true, b); }),
                   s_c = measure([&](Arena& ar) { region_carve(ar, n2, cap2, 8, 8, tmpb, partb, true, c); });
      printf("resident shapes, bytes carved / bytes of the replaced formula: radix fold %zu / %zu, molecule stage %zu / %zu, region stage %zu / %zu\n",
             s_a, old_need_radix(n_fc, 8, tmpb), s_b, old_need_molecule(n_mol, 8, tmpb, 1000000), s_c, old_need_region(n2, cap2, 8, 8, tmpb, partb, true)); }
    printf("%ld grid points, %ld blocks checked and written: %s\n", g_points, g_blocks, g_fail ? "FAILED" : "workspaces sound");
    return g_fail ? 1 : 0;
}
