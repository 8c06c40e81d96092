// ref_geom.h - the arithmetic of the packed reference sequence (ref_seq.h) that host and device share: where a
// position lies in a FASTA contig's raw bytes, which positions a staging chunk covers, and how one dword of eight 4-bit codes is made
// from the chunk.  Plain numbers and pointers in; no HIP call and no EngineImpl, so that a host program can run the same functions over
// a grid of geometries (tools/asan/ref_geom_check.cpp).  tests/refseq_cases.py states the same arithmetic again in Python.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define XCK_RG_HD __host__ __device__ inline
#else
#define XCK_RG_HD inline
#endif

namespace xck {
constexpr int64_t RG_MIN_CHUNK = 64;                 // the least XCK_REF_CHUNK_BYTES
constexpr int RG_POS_PER_THREAD = 8;                 // positions of one dword

// raw offset of position p of a contig whose first base is raw[0]: lb bases a line, lw bytes a line (the .fai's line_bases, line_width)
XCK_RG_HD int64_t rg_offset(int64_t p, int64_t lb, int64_t lw) { return (p / lb) * lw + p % lb; }
// positions whose offset lies below r
XCK_RG_HD int64_t rg_pos_below(int64_t r, int64_t lb, int64_t lw) { const int64_t c = r % lw; return (r / lw) * lb + (c < lb ? c : lb); }
// A chunk starts at position p0, a multiple of 8, and takes the positions whose bytes fit into chunk_bytes from p0's offset on, cut down to a
// multiple of 8 unless the contig ends there; a geometry so sparse that fewer than 8 positions fit takes 8 (the caller sizes its buffer
// by rg_chunk_bytes, not by the knob).  -> p1, the chunk's end; p0 < p1 <= len.
XCK_RG_HD int64_t rg_chunk_end(int64_t p0, int64_t len, int64_t lb, int64_t lw, int64_t chunk_bytes) {
    int64_t p1 = rg_pos_below(rg_offset(p0, lb, lw) + chunk_bytes, lb, lw);
    if (p1 >= len) return len;
    p1 &= ~int64_t(7);
    if (p1 <= p0) p1 = p0 + 8 < len ? p0 + 8 : len;
    return p1;
}
// the raw bytes of positions [p0, p1): from p0's offset through the last position's byte
XCK_RG_HD int64_t rg_chunk_bytes(int64_t p0, int64_t p1, int64_t lb, int64_t lw) { return rg_offset(p1 - 1, lb, lw) + 1 - rg_offset(p0, lb, lw); }

// BAM's 4-bit code of a FASTA byte: the 15 letters of "=ACMGRSVTWYHKDBN" behind '=', lower case as upper case; everything else - '=' too - N
XCK_RG_HD uint8_t rg_code(uint32_t byte) {
    const char* const L = "=ACMGRSVTWYHKDBN";
    const uint32_t u = byte >= 'a' && byte <= 'z' ? byte - 32u : byte;
    uint8_t code = 15;
    for (int k = 1; k < 16; k++) if (u == (uint32_t)L[k]) code = (uint8_t)k;
    return code;
}

// One dword of the packed sequence: the codes of positions [p, p + 8), p a multiple of 8 inside the chunk [p0, p1) whose n_chunk raw bytes
// start at chunk (chunk[0] is the byte of p0, at offset base0 = rg_offset(p0) of the contig).  p < 2^31, as every position of a contig.
// Position p + 2 j lies in the high nibble of byte j (BAM's order), p + 2 j + 1 in the low one;
// positions at or past p1 - the contig's end: only its last chunk ends off a multiple of 8 - are 0.  map: the 256 codes of rg_code.
// The 8 bytes are ONE load where they lie inside one line; otherwise the walk steps over the line end where it meets it.
// bad: + 1 for every byte below 33 met where a base must be (a stale index), and for every offset outside the chunk (never, by
// rg_chunk_bytes; such a byte reads as N and is not loaded).
XCK_RG_HD uint32_t rg_pack_dword(const uint8_t* chunk, int64_t n_chunk, int64_t base0, int64_t p, int64_t p1, int64_t lb, int64_t lw, const uint8_t* map, uint32_t& bad) {
    const int64_t line = (int64_t)((uint32_t)p / (uint32_t)lb), col = p - line * lb;   // (the one division a thread makes: 32 bits suffice)
    int64_t o = line * lw + col - base0;
    uint64_t v = 0;                                                      // byte j: the raw byte of position p + j (little endian)
    if (col + 8 <= lb && p + 8 <= p1 && o >= 0 && o + 8 <= n_chunk) {
        memcpy(&v, chunk + o, 8);
    } else {
        int64_t c = col;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (p + j < p1) {
                uint64_t x = 'N';
                if (o >= 0 && o < n_chunk) x = chunk[o]; else bad++;
                v |= x << (8 * j);
                if (++c == lb) { c = 0; o += lw - lb + 1; } else o++;
            }
        }
    }
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (p + j < p1) {
            const uint32_t x = (uint32_t)(v >> (8 * j)) & 255u;
            if (x < 33u) bad++;
            w |= (uint32_t)map[x] << (8 * (j >> 1) + ((j & 1) ? 0 : 4));
        }
    }
    return w;
}
}  // namespace xck
