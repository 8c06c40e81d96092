// Host-only check of the packed reference's arithmetic (csrc/ref_geom.h: rg_offset, rg_chunk_end, rg_chunk_bytes, rg_code, rg_pack_dword)
// under AddressSanitizer / UBSan.  For every point of a grid of contig lengths, line lengths, line ends, file ends and places in a file of
// three sequences the contig is packed as the engine packs it (ref_seq.h engine_set_contig_ref): chunk by chunk, every chunk copied into
// a malloc'ed block of exactly rg_chunk_bytes bytes - a load past it is the sanitizer's to report -, every dword made by rg_pack_dword,
// the function k_ref_pack runs per thread.  The result must equal a plain line-by-line parse of the same text; chunks start at multiples
// of 8, cover the contig without gaps and stay within the chunk size (or 8 positions); no byte below 33 is met.  A stale geometry
// (line_bases and line_width one larger) is packed too: it must stay inside its blocks, and is counted where it meets a line end.
// No device, no HIP call.
//   make -C tools/asan ref_geom_check && tools/asan/ref_geom_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../xcltk_amd/csrc/ref_geom.h"

using namespace xck;

static int g_fail = 0;
static long g_points = 0, g_chunks = 0, g_stale = 0, g_stale_seen = 0;
static void fail(const char* what, long len, long lb, long chunk) { if (g_fail++ < 20) fprintf(stderr, "FAIL: %s (length %ld, line_bases %ld, chunk %ld)\n", what, len, lb, chunk); }

// the engine's loop over raw[0, n_raw) -> the packed dwords; *bad: the stale-index count
static std::vector<uint32_t> pack(const char* raw, int64_t n_raw, int64_t len, int64_t lb, int64_t lw, int64_t chunk, const uint8_t* map, uint64_t* bad, bool sound) {
    std::vector<uint32_t> out((size_t)((len + 7) / 8), 0xFFFFFFFFu);
    for (int64_t p0 = 0; p0 < len;) {
        const int64_t p1 = rg_chunk_end(p0, len, lb, lw, chunk), nb = rg_chunk_bytes(p0, p1, lb, lw), base0 = rg_offset(p0, lb, lw);
        g_chunks++;
        if (p0 % 8 || p1 <= p0 || p1 > len || (p1 < len && p1 % 8)) fail("a chunk does not run from a multiple of 8 to one, or to the end", len, lb, chunk);
        if (nb > std::max(chunk, 8 * lw)) fail("a chunk larger than the chunk size and 8 lines", len, lb, chunk);
        if (base0 + nb > n_raw) { if (sound) fail("a chunk ends behind the raw bytes", len, lb, chunk); return out; }
        uint8_t* blk = (uint8_t*)malloc((size_t)nb);
        if (!blk) { fprintf(stderr, "malloc(%ld) failed\n", (long)nb); exit(2); }
        memcpy(blk, raw + base0, (size_t)nb);
        for (int64_t p = p0; p < p1; p += 8) { uint32_t b = 0; out[(size_t)(p >> 3)] = rg_pack_dword(blk, nb, base0, p, p1, lb, lw, map, b); *bad += b; }
        free(blk);
        p0 = p1;
    }
    return out;
}

int main() {
    uint8_t map[256];
    for (int k = 0; k < 256; k++) map[k] = rg_code((uint32_t)k);
    const char* L = "=ACMGRSVTWYHKDBN";
    for (int k = 1; k < 16; k++) if (map[(uint8_t)L[k]] != k || map[(uint8_t)(L[k] | 32)] != k) { fprintf(stderr, "FAIL: rg_code('%c')\n", L[k]); g_fail++; }
    for (int c : { (int)'=', (int)'*', (int)'-', (int)'.', (int)'U', (int)'u', (int)'0', (int)'9', (int)' ', (int)'\n', (int)'\r', 0, 255, (int)'E', (int)'z' }) if (map[c] != 15) { fprintf(stderr, "FAIL: rg_code(%d) is not N\n", c); g_fail++; }
    const char* alphabet = "ACGTNacgtnRYKMSWBDHVrykmswbdhv=*-.U7";
    const long lengths[] = { 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 2049 };
    for (long len : lengths) {
        for (long lb : { 1l, 3l, 8l, 60l, len, len + 5 }) {
            for (const char* eol : { "\n", "\r\n" }) {
                const long lw = lb + (long)strlen(eol);
                for (int final_nl = 0; final_nl < 2; final_nl++) {
                    for (int place = 0; place < 3; place++) {
                        // three sequences, the one under test at `place`; the others are 11 and 70 bases long
                        std::string text, seq;
                        int64_t off = 0;
                        for (int s = 0; s < 3; s++) {
                            const long n = s == place ? len : s == 0 ? 11 : 70;
                            text += ">s" + std::to_string(s) + " x" + eol;
                            if (s == place) off = (int64_t)text.size();
                            for (long p = 0; p < n; p++) {
                                const char c = alphabet[(size_t)(p * 7 + s + len) % 36];
                                if (s == place) seq += c;
                                text += c;
                                if ((p + 1) % lb == 0 && p + 1 < n) text += eol;
                            }
                            if (s < 2 || final_nl) text += eol;
                        }
                        const int64_t n_raw = std::min<int64_t>(rg_offset(len - 1, lb, lw) + 1, (int64_t)text.size() - off);
                        if (n_raw != rg_offset(len - 1, lb, lw) + 1) fail("the text ends in front of the contig's last base", len, lb, 0);
                        for (long chunk : { 64l, 100l, 1l << 20 }) {
                            g_points++;
                            uint64_t bad = 0;
                            const std::vector<uint32_t> w = pack(text.data() + off, n_raw, len, lb, lw, chunk, map, &bad, true);
                            if (bad) fail("a byte below 33 under the true geometry", len, lb, chunk);
                            for (long p = 0; p < (long)w.size() * 8; p++) {
                                const uint32_t by = (w[(size_t)(p >> 3)] >> (8 * ((p & 7) >> 1))) & 255u, nib = (p & 1) ? (by & 15u) : (by >> 4);
                                const uint32_t want = p < len ? map[(uint8_t)seq[(size_t)p]] : 0u;
                                if (nib != want) { fail("a packed code differs from the plain parse", len, lb, chunk); break; }
                            }
                            // a stale index: one base more a line.  Whatever it reads lies inside its blocks
                            uint64_t sbad = 0;
                            g_stale++;
                            pack(text.data() + off, n_raw, len, lb + 1, lw + 1, chunk, map, &sbad, false);
                            if (sbad) g_stale_seen++;
                        }
                    }
                }
            }
        }
    }
    // the chunks of a chr1-sized contig at the default chunk size: 60 bases a line
    { const int64_t len = 248956422, lb = 60, lw = 61, chunk = 32ll << 20; long n = 0; int64_t most = 0;
      for (int64_t p0 = 0; p0 < len; n++) { const int64_t p1 = rg_chunk_end(p0, len, lb, lw, chunk); most = std::max(most, rg_chunk_bytes(p0, p1, lb, lw)); p0 = p1; }
      printf("a contig of %lld positions at 60 bases a line: %ld chunks of at most %lld bytes\n", (long long)len, n, (long long)most);
      if (most > chunk) { fprintf(stderr, "FAIL: a chunk of %lld bytes\n", (long long)most); g_fail++; } }
    printf("%ld grid points, %ld chunks packed, %ld of %ld stale geometries met a line end: %s\n", g_points, g_chunks, g_stale_seen, g_stale, g_fail ? "FAILED" : "geometry sound");
    return g_fail ? 1 : 0;
}
