// inflate_dev.hip - raw-DEFLATE decoder for BGZF blocks on the GPU (gfx950): one 64-lane wave per block.
//
// Replaces, for the share of the chunks the host decoder hands over (csrc/bam.cpp, XCK_GPU_INFLATE), the inflate that pysam / htslib
// do inside AlignmentFile.fetch (xcltk/rdr/fc/core.py:73-76, utils/sam.py:105-118).  With the device parse (XCK_GPU_PARSE, csrc/parse_dev.hip)
// the record walk and the field parse of these chunks follow on the same stream and the inflated bytes stay in HBM; without it they go
// back to the host's walk and parse.
// Why: end to end the engine was bound by the host's BGZF inflate (73 - 85 % of the ingest CPU time on 16 cores,
// profiles/r02_d_ingest_*.log) while the GPU idled.  BGZF blocks are independent <= 64 KiB deflate streams, so a chunk of
// ~750 blocks is 750 waves of work.  Inside a block the SYMBOL BOUNDARIES are serial - they are only known after the previous
// symbol - but what would be decoded at a given bit offset is not:
//   * block headers: the chain of code-length symbols is serial and stays with lane 0 - one look-up in a 128-entry table the lanes build
//     and one LDS store per symbol, which marks where a run of equal lengths begins; the wave spreads the marks over the lengths (a
//     prefix maximum), and writes a fixed block's lengths;
//   * decode tables: built by all lanes into LDS (9-bit primary + sub-tables for literal / length, 8-bit for distance; a code that
//     needs more LDS than the block's budget marks the block "not done" and the host inflates it - the compressed bytes never left
//     the host).  Lane i owns the symbols i, i + 64, ...: counts and ranks per length by ballots, codes from first code + rank, the
//     sub-table sizes as an LDS maximum on the primary entries, their offsets by a scan over the prefixes; nothing of it is serial
//     (it was lane 0's, with the header a tenth of a block's time) and no array but the tables and the lengths is left in LDS - 8.4 KB
//     and 83 VGPRs, so LDS no longer holds a CU at 15 waves (profiles/r36_inflate_setup.txt);
//   * symbols: 64 bit offsets per round - every lane decodes the code that would start at ITS offset, a scalar walk over the lanes'
//     code lengths (four symbols per hop, prepared by two rounds of ds_bpermute) finds the offsets where symbols really start, those
//     lanes store their literals at positions from a prefix sum, and the wave copies the matches
//     (out[dst + i] = out[dst - dist + i % dist] reads only bytes that already exist, so overlapping matches need no serial loop);
//     a round's batched match copy loads in that round and stores in the next, so the wave never sleeps on the round trip;
//   * the finished block stays in HBM for the device walk (host_out == nullptr); only when the host is to walk the chunk does the same
//     wave also store it to the chunk's pinned host block (16-byte stores over PCIe).
// Measured: DESIGN.md section 6, profiles/experiments/gpu_inflate/ (every step of the way, against zlib block by block).
//   * check_crc: the same epilogue computes the block's CRC-32 and compares it with the footer's (DevBlock.crc).
// Status per block: 0 = inflated (exactly isize bytes; with check_crc also CRC-checked), non-zero = left to the host decoder
// (csrc/inflate_fast.h / zlib); INFLATE_ST_CRC = inflated, but the CRC-32 differs from the footer's.
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <hip/hip_runtime.h>
#include "parse_dev.h"

namespace xck {

__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x);
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t x);

namespace {

struct DHuff { uint16_t val; uint8_t len; uint8_t op; };
// op: 0 literal | 0x10+x length / distance base in val with x extra bits | 0x20 end of block | 0x40 invalid | 0x80+s sub-table link

// A 9-bit primary literal / length table: in the 64-offsets loop some lane takes the sub-table path in (nearly) every round anyway, so
// a smaller primary costs nothing there and 3.5 KB less LDS is one to four more waves per CU (measured in the harness: + 23 - 30 %).
#ifndef XCK_D_LIT_TB
#define XCK_D_LIT_TB 9
#endif
constexpr int D_LIT_TB = XCK_D_LIT_TB, D_DIST_TB = 8;
constexpr int D_LIT_MAX = (1 << D_LIT_TB) + 768;          // primary + sub-table budget (blocks that need more go to the host)
constexpr int D_DIST_MAX = (1 << D_DIST_TB) + 256;

__device__ const uint16_t d_len_base[29] = {3,4,5,6,7,8,9,10,11,13,15,17,19,23,27,31,35,43,51,59,67,83,99,115,131,163,195,227,258};
__device__ const uint8_t  d_len_extra[29] = {0,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,0};
__device__ const uint16_t d_dist_base[30] = {1,2,3,4,5,7,9,13,17,25,33,49,65,97,129,193,257,385,513,769,1025,1537,2049,3073,4097,6145,8193,12289,16385,24577};
__device__ const uint8_t  d_dist_extra[30] = {0,0,0,0,1,1,2,2,3,3,4,4,5,5,6,6,7,7,8,8,9,9,10,10,11,11,12,12,13,13};
__device__ const uint8_t  d_cl_order[19] = {16,17,18,0,8,7,9,6,10,5,11,4,12,3,13,2,14,1,15};

__host__ __device__ constexpr uint32_t dh(uint32_t val, uint32_t len, uint32_t op) { return val | len << 16 | op << 24; }   // a DHuff as the 32-bit word the tables hold
constexpr uint32_t DH_INVAL = dh(0, 1, 0x40);

// What a block header needs only until its code lengths stand in lens[]: it lies over lit[], which is dead from the end of one
// DEFLATE block's symbols to the next table build.
struct HdrScratch {
    uint16_t mark[320];                   // mark[i] = (i + 1) << 4 | v where a run of length v starts at lens[i], 0 inside a run
    uint8_t  cl[128];                     // code-length code: the next 7 stream bits -> symbol | bits << 5
    uint8_t  pl[32];                      // its 19 code lengths
};
constexpr int IN_WIN = 1024;                               // bytes of the compressed stream staged per fill (a multiple of 256; see BitIn)
// 8,576 B: 19 workgroups of one wave fit a CU's 160 KB of LDS (10,832 B held it at 15), and the kernel's 83 VGPRs allow them: 5 waves per SIMD.
struct Smem {
    union { uint32_t lit[D_LIT_MAX]; HdrScratch hdr; };   // (DHuff words)
    uint32_t dist[D_DIST_MAX];
    uint8_t lens[320];                    // code lengths: literal / length alphabet, then distance alphabet
    uint32_t first[16];                   // first canonical code of every length (build_table)
    uint32_t win[IN_WIN / 4];             // the input window (last: the CRC tables of the epilogue end in it)
};

__device__ __forceinline__ uint32_t brev(uint32_t v, int n) { return __brev(v) >> (32 - n); }
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }   // bits of m below this lane

// all 64 lanes: decode table for `n_sym` (<= 64 NCH) code lengths at lens[]; kind 0 literal / length, 1 distance.  Returns false
// (uniform) when the code is over-subscribed or does not fit the LDS budget.  Lane i owns the symbols i, i + 64, ... and keeps their
// lengths and codes in registers; no step's trip count is the number of symbols or the size of the primary table.
template <int NCH>
__device__ bool build_table(Smem& sm, const uint8_t* lens, int n_sym, int tb, uint32_t* tab, int tab_max, int kind, int lane) {
    const int psize = 1 << tb;
    // counts per length, and every symbol's rank among the symbols of its length: a ballot per length over each chunk of 64 symbols
    // (lane L keeps the count of length L; a symbol's rank is the count before its chunk + the equal lengths below it in the chunk)
    uint32_t len_[NCH], code_[NCH], cnt = 0;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const int s = c * 64 + lane;
        const uint32_t l = s < n_sym ? lens[s] : 0u;
        uint32_t below = 0, add = 0;
#pragma unroll 1
        for (uint32_t L = 1; L <= 15; L++) { const uint64_t m = __ballot(l == L); below = l == L ? lanes_below(m) : below; add = (uint32_t)lane == L ? (uint32_t)__popcll(m) : add; }
        len_[c] = l; code_[c] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(l << 2), (int)cnt) + below;
        cnt += add;
    }
    // over-subscribed at any length: no table.  The first canonical code of length L goes to lane L, and from there to LDS
    int left = 1; bool ok = true; uint32_t c0 = 0, f = 0, before = 0;
#pragma unroll 1
    for (int L = 1; L <= 15; L++) {
        const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)cnt, L);
        left = left * 2 - (int)n; ok = ok && left >= 0; c0 = (c0 + before) << 1; before = n; f = lane == L ? c0 : f;
    }
    if (!ok) return false;
    if (lane < 16) sm.first[lane] = f;
    for (int i = lane; i < psize; i += 64) tab[i] = DH_INVAL;
    __builtin_amdgcn_wave_barrier();
    // canonical codes (bit-reversed) from first code + rank.  A long code raises its primary entry to a link with its extra bits: links
    // compare above the invalid entry and by their bits, so the LDS maximum leaves every prefix with the longest code under it
    bool is_long = false;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const uint32_t l = len_[c];
        if (l) {
            const uint32_t r = brev(sm.first[l] + code_[c], (int)l);
            code_[c] = r;
            if ((int)l > tb) { is_long = true; atomicMax(&tab[r & (uint32_t)(psize - 1)], dh(0, (uint32_t)tb, 0x80u | (l - (uint32_t)tb))); }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (__ballot(is_long)) {
        // sub-tables in ascending order of their prefixes: offsets by a scan over the sizes, 64 prefixes at a time; the link entry
        // is the record.  The sum decides whether the table fits.
        uint32_t used = (uint32_t)psize;
        for (int p0 = 0; p0 < psize; p0 += 64) {
            const uint32_t e = tab[p0 + lane];
            const uint32_t sz = (e >> 31) ? 1u << ((e >> 24) & 15u) : 0u;
            const uint32_t inc = wave_scan_incl(sz);
            if (sz) tab[p0 + lane] = e | (used + inc - sz);                  // (at most 2^tb + 2^tb 2^(15 - tb) <= 33,280: the 16 bits of val)
            used += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        }
        if ((int)used > tab_max) return false;
        for (int i = psize + lane; i < (int)used; i += 64) tab[i] = DH_INVAL;   // what an incomplete code leaves uncovered stays invalid
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int c = 0; c < NCH; c++) {                        // every lane fills the entries of its symbols
        const int s = c * 64 + lane; const uint32_t l = len_[c];
        if (!l) continue;
        uint32_t e;
        if (kind == 0) {
            if (s < 256) e = dh((uint32_t)s, 0, 0);
            else if (s == 256) e = dh(0, 0, 0x20);
            else if (s <= 285) e = dh(d_len_base[s - 257], 0, 0x10u | d_len_extra[s - 257]);
            else e = dh(0, 0, 0x40);
        } else {
            e = s < 30 ? dh(d_dist_base[s], 0, 0x10u | d_dist_extra[s]) : dh(0, 0, 0x40);
        }
        const uint32_t r = code_[c];
        if ((int)l <= tb) { e |= l << 16; for (uint32_t k = r; k < (uint32_t)psize; k += 1u << l) tab[k] = e; }
        else {
            const uint32_t lk = tab[r & (uint32_t)(psize - 1)], sb = (lk >> 24) & 15u, off = lk & 0xffffu;
            e |= (l - (uint32_t)tb) << 16;
            for (uint32_t k = r >> tb; k < (1u << sb); k += 1u << (l - (uint32_t)tb)) tab[off + k] = e;
        }
    }
    __builtin_amdgcn_wave_barrier();
    return true;
}

// all 64 lanes: the code-length code's 7-bit look-up table (hdr.cl) from its 19 lengths (hdr.pl).  False (uniform) unless the code is
// complete - zlib refuses an incomplete code-length code as well as an over-subscribed one, and a complete one fills the table.
__device__ bool build_cl_table(Smem& sm, int lane) {
    const uint32_t l = lane < 19 ? sm.hdr.pl[lane] : 0u;
    uint32_t r = 0, c0 = 0, f = 0, kraft = 0, prev = 0;
#pragma unroll
    for (uint32_t L = 1; L <= 7; L++) {
        const uint64_t m = __ballot(l == L); const uint32_t n = (uint32_t)__popcll(m);
        c0 = (c0 + prev) << 1; prev = n; kraft += n << (7 - L);
        if (l == L) { r = lanes_below(m); f = c0; }
    }
    if (kraft != 128u) return false;
    if (l) { const uint32_t code = brev(f + r, (int)l), e = (uint32_t)lane | l << 5; for (uint32_t k = code; k < 128u; k += 1u << l) sm.hdr.cl[k] = (uint8_t)e; }
    __builtin_amdgcn_wave_barrier();
    return true;
}

// The compressed stream reaches lane 0 through an LDS window: the whole wave loads IN_WIN bytes at a time (aligned dwords,
// coalesced), lane 0 takes aligned dwords out of LDS.  (A per-lane byte pointer into global memory cost four dependent byte
// loads - about a microsecond - per 32 bits of input.)  Coordinates: byte s of the stream sits at c = s + A of the 4-byte
// aligned buffer that starts at (stream address - A), A = address & 3.  (IN_WIN bytes per fill: above, with Smem.)
// A round of the symbol loop starts with its first bit's byte (byte0) at least WIN_MARGIN bytes before the window's end: lane 63 begins at
// bit 7 + 63 of byte0 at most, i.e. in a dword that starts at byte0 + 8 or earlier, and reads that dword and the two after it (64 stream
// bits: a length + distance pair is 48) - bytes up to byte0 + 8 + 11.
constexpr int WIN_MARGIN = 32;
static_assert(IN_WIN % 256 == 0 && WIN_MARGIN % 4 == 0 && WIN_MARGIN >= 8 + 12 && IN_WIN >= 512 + WIN_MARGIN, "a round's three-dword window reads must stay inside win[]");
struct BitIn {
    uint32_t pos;                                          // next aligned-buffer coordinate to load (multiple of 2)
    uint32_t wlo;                                          // the window holds coordinates [wlo, wlo + IN_WIN)
    uint64_t bb; int bc;
    __device__ __forceinline__ uint32_t bits(int n) const { return (uint32_t)(bb & ((1ull << n) - 1)); }
    __device__ __forceinline__ void drop(int n) { bb >>= n; bc -= n; }
    // 16 bits at a time until more than 48 bits are buffered (a length + distance pair needs at most 48); false = the window
    // is used up before that
    __device__ __forceinline__ bool refill(const uint32_t* win) {
        const uint16_t* w16 = (const uint16_t*)win;
        while (bc <= 48) {
            if (pos + 2 > wlo + IN_WIN) return false;
            bb |= (uint64_t)w16[(pos - wlo) >> 1] << bc; bc += 16; pos += 2;
        }
        return true;
    }
};

}  // namespace

// inclusive prefix sum over the wave (DPP: shifts inside the rows of 16, then the row totals travel on)
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);    // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);    // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);    // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);    // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);    // row_bcast:15 -> rows 1, 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);    // row_bcast:31 -> rows 2, 3
    return x;
}

// inclusive prefix maximum over the wave (the same steps; the missing neighbours read as 0)
__device__ __forceinline__ uint32_t wave_scan_max(uint32_t x) {
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false));    // row_shr:1
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false));    // row_shr:2
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false));    // row_shr:4
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false));    // row_shr:8
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false));    // row_bcast:15 -> rows 1, 3
    x = max(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false));    // row_bcast:31 -> rows 2, 3
    return x;
}

// XOR of x over the wave, in every lane (the same DPP steps; the missing neighbours read as 0)
__device__ __forceinline__ uint32_t wave_xor_all(uint32_t x) {
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);    // row_shr:1
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);    // row_shr:2
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);    // row_shr:4
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);    // row_shr:8
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);    // row_bcast:15
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);    // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// ---- CRC-32 of a finished block (check_crc): zlib's crc32(), reflected polynomial 0xEDB88320, init and xorout 0xFFFFFFFF ----
// The epilogue reads the block in 16-byte pieces, lane l taking pieces l, l + 64, ... (the coalesced form of the host store).  The
// CRC register is linear: crc(A | B) = crc(A) x^(8|B|) + crc(B) mod P (zlib's crc32_combine).  So every lane keeps a register of its
// own pieces as if 1008 zero bytes stood between them - per piece R = R x^(8 * 1024) + crc(piece), the product by table (4 look-ups)
// and crc(piece) by slice-by-4 from a zero register, independent of R - then shifts it over the bytes that follow its last piece
// (< 1024: one product by x^(8 s) from a table) and the wave XORs the registers.  Lane 0 starts from the register of the bytes before
// the first aligned piece (init included) and adds the bytes after the last one.
constexpr uint32_t CRC_POLY = 0xEDB88320u;
struct CrcTables {
    uint32_t slice[4][256];        // slice[k][b]: register after byte b and k zero bytes (slice[0] is the byte-wise table)
    uint32_t step[4][256];         // step[k][b]: (b << 8k) x^(8 * 1024) mod P - one lane's register moved past a round of the store loop
    uint32_t xpow[1024];           // x^(8 s) mod P (in zlib's bit order: x^0 = 0x80000000)
};
constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b) {          // a b mod P (zlib multmodp)
    uint32_t p = 0;
    for (int k = 31; k >= 0; k--) { if ((a >> k) & 1u) p ^= b; b = (b >> 1) ^ ((b & 1u) ? CRC_POLY : 0u); }
    return p;
}
constexpr CrcTables make_crc_tables() {
    CrcTables t{};
    for (uint32_t i = 0; i < 256; i++) { uint32_t c = i; for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? CRC_POLY : 0u); t.slice[0][i] = c; }
    for (int k = 1; k < 4; k++) for (uint32_t i = 0; i < 256; i++) t.slice[k][i] = (t.slice[k - 1][i] >> 8) ^ t.slice[0][t.slice[k - 1][i] & 0xffu];
    t.xpow[0] = 0x80000000u;
    for (int s = 1; s < 1024; s++) t.xpow[s] = (t.xpow[s - 1] >> 8) ^ t.slice[0][t.xpow[s - 1] & 0xffu];   // one more zero byte
    const uint32_t x1024 = (t.xpow[1023] >> 8) ^ t.slice[0][t.xpow[1023] & 0xffu];
    for (int k = 0; k < 4; k++) for (uint32_t i = 0; i < 256; i++) t.step[k][i] = crc_mulmod(i << (8 * k), x1024);
    return t;
}
__device__ const CrcTables d_crc = make_crc_tables();
constexpr int CRC_LDS_WORDS = 2 * 4 * 256;                      // slice + step tables, staged in the decode tables' LDS once a block is decoded

__device__ __forceinline__ uint32_t crc_word(const uint32_t* tab, uint32_t c, uint32_t w) {   // four bytes, slice-by-4
    c ^= w;
    return tab[3 * 256 + (c & 0xffu)] ^ tab[2 * 256 + ((c >> 8) & 0xffu)] ^ tab[256 + ((c >> 16) & 0xffu)] ^ tab[c >> 24];
}
__device__ __forceinline__ uint32_t crc_byte(const uint32_t* tab, uint32_t c, uint8_t v) { return tab[(c ^ v) & 0xffu] ^ (c >> 8); }

// Output bytes go straight to global memory and a match reads them back from there (behind a fence when they were stored since the
// last one).  (A variant that kept the last 4 / 8 KB in an LDS ring - near matches as LDS-to-LDS copies, aligned 1 KB flushes - cost a
// third of the occupancy and measured equal or slower: profiles/experiments/gpu_inflate/inflate_dev_with_lds_ring.hip.)
__device__ unsigned long long d_prof[8];          // PROF builds only (tools/gpu_inflate_bench): cycles of wave-time per phase, summed over the blocks
#define XCK_PROF_AT(k) do { if constexpr (PROF) { const long long t_ = clock64(); prof[k] += (unsigned long long)(t_ - t_prev); t_prev = t_; } } while (0)

template <bool PROF, bool CRC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_inflate(const uint8_t* __restrict__ in, const DevBlock* __restrict__ blocks, int n_blocks,
                                                uint8_t* out, int32_t* __restrict__ status, uint8_t* host_out) {
    static_assert(sizeof(Smem) >= CRC_LDS_WORDS * sizeof(uint32_t), "the CRC tables live in the decode tables' LDS (and the head of the window's)");
    static_assert(sizeof(Smem) <= 10240, "at least the 16 workgroups per CU that 128 VGPRs would allow");
    __shared__ Smem sm;
    uint32_t* const win = sm.win;
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= n_blocks) return;
    unsigned long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0}; long long t_prev = PROF ? clock64() : 0;   // 0 header, 1 tables, 2 window, 3 decode, 4 walk, 5 scan + literals, 6 matches, 7 flush / rest
    const DevBlock blk = blocks[b];
    uint8_t* const o0v = out + blk.out_off;                            // the block's output
    const uint32_t out_end = blk.out_len;
    if (blk.out_len == 0) { if (lane == 0) status[b] = 0; return; }
    const uint8_t* const sp = in + blk.in_off;
    const uint32_t A = (uint32_t)((uintptr_t)sp & 3u);
    const uint32_t* const abase = (const uint32_t*)(sp - A);           // 4-byte aligned view of the stream
    const uint32_t c_end = A + blk.in_len;                             // first coordinate past the stream
    if (blk.in_len == 0) { if (lane == 0) status[b] = 10; return; }    // (no stream: the stored-header check's status; fill() clamps to the last byte)
    // all lanes; words past the stream read as zero.  The loads are unconditional (index clamped to the dword the stream's last byte lies in, zero selected afterwards) so
    // that all of them are in flight before the one wait: the stream is in mapped host memory, every wait is a PCIe round trip.
    auto fill = [&](uint32_t wlo) {
        uint32_t w[IN_WIN / 256];
#pragma unroll
        for (int j = 0; j < IN_WIN / 256; j++) { const uint32_t c = wlo + (uint32_t)(j * 256 + lane * 4); w[j] = abase[min(c, c_end - 1u) >> 2]; }
#pragma unroll
        for (int j = 0; j < IN_WIN / 256; j++) { const uint32_t c = wlo + (uint32_t)(j * 256 + lane * 4); win[j * 64 + lane] = c < c_end ? w[j] : 0u; }
        __builtin_amdgcn_wave_barrier();
    };
    BitIn bi; bi.pos = 0; bi.wlo = 0; bi.bb = 0; bi.bc = 0;            // (lane 0's state; the other lanes carry dead copies)
    fill(0);
    if (lane == 0) { bi.refill(win); bi.drop((int)(8 * A)); }          // skip the A bytes before the stream
    uint32_t op = 0;                                                   // output position (wave-uniform)
    int err = 0;
    for (;;) {
        // ---- block header: its fields and the 19 lengths of the code-length code by lane 0, broadcast; the window is moved first so that
        // a whole header (< 400 bytes) fits.  The header's scratch (over lit[], dead here) starts from zero: no mark, no length ----
        { uint32_t pos = __builtin_amdgcn_readfirstlane(bi.pos), wlo = __builtin_amdgcn_readfirstlane(bi.wlo);
          if (pos > wlo + IN_WIN - 512) { fill(pos & ~3u); bi.wlo = pos & ~3u; } }
        __syncthreads();                                               // (every lane is past its last read of the tables the scratch lies over)
        for (int i = lane; i < 320; i += 64) sm.hdr.mark[i] = 0;
        if (lane < 32) sm.hdr.pl[lane] = 0;
        __builtin_amdgcn_wave_barrier();
        int btype = 0, bfinal = 0, hlit = 0, hdist = 0;
        if (lane == 0) {
            bi.refill(win);
            if (bi.bc < 3) err = 1;
            bfinal = (int)bi.bits(1); btype = (int)((bi.bb >> 1) & 3); bi.drop(3);
            if (btype == 3) err = 2;
            if (!err && btype == 2) {
                bi.refill(win);
                hlit = (int)bi.bits(5) + 257; bi.drop(5); hdist = (int)bi.bits(5) + 1; bi.drop(5);
                const int hclen = (int)bi.bits(4) + 4; bi.drop(4);
                if (hlit > 286 || hdist > 30) err = 3;
                for (int i = 0; i < hclen && !err; i++) { if (bi.bc < 3) bi.refill(win); if (bi.bc < 3) { err = 4; break; } sm.hdr.pl[d_cl_order[i]] = (uint8_t)bi.bits(3); bi.drop(3); }
            }
        }
        err = __builtin_amdgcn_readfirstlane(err);
        if (err) break;
        btype = __builtin_amdgcn_readfirstlane(btype); bfinal = __builtin_amdgcn_readfirstlane(bfinal);
        hlit = __builtin_amdgcn_readfirstlane(hlit); hdist = __builtin_amdgcn_readfirstlane(hdist);
        __builtin_amdgcn_wave_barrier();
        if (btype == 2) {
            // the code-length code as a 7-bit look-up table, by all lanes; the chain of its symbols is serial by nature and stays with
            // lane 0, which only MARKS where a run begins (one LDS store per symbol, whatever the run's length); the wave then spreads
            // every mark over its run: a prefix maximum - marks grow with their position - over 64 lengths at a time
            if (!build_cl_table(sm, lane)) { err = 5; break; }
            const int tot = hlit + hdist;
            if (lane == 0) {
                int n = 0; uint32_t last = 0;                              // last: the length before position n
                while (n < tot) {
                    bi.refill(win);
                    const uint32_t e = sm.hdr.cl[bi.bb & 127u]; const int l = (int)(e >> 5), sym = (int)(e & 31u);
                    if (l > bi.bc) { err = 5; break; }
                    bi.drop(l);
                    int r = 1;
                    if (sym < 16) last = (uint32_t)sym;
                    else if (sym == 16) { if (!n) { err = 6; break; } r = 3 + (int)bi.bits(2); bi.drop(2); }
                    else if (sym == 17) { r = 3 + (int)bi.bits(3); bi.drop(3); last = 0; }
                    else { r = 11 + (int)bi.bits(7); bi.drop(7); last = 0; }
                    if (n + r > tot) { err = 7; break; }
                    sm.hdr.mark[n] = (uint16_t)(((uint32_t)(n + 1) << 4) | last);
                    n += r;
                    if (bi.bc < 0) { err = 8; break; }
                }
            }
            err = __builtin_amdgcn_readfirstlane(err);
            if (err) break;
            __builtin_amdgcn_wave_barrier();
            uint32_t carry = 0;
            for (int i0 = 0; i0 < tot; i0 += 64) {
                const uint32_t x = max(wave_scan_max(sm.hdr.mark[i0 + lane]), carry);
                carry = (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
                sm.lens[i0 + lane] = (uint8_t)(x & 15u);
            }
            __builtin_amdgcn_wave_barrier();
            if (sm.lens[256] == 0) { err = 9; break; }
        } else if (btype == 1) {
            for (int i = lane; i < 320; i += 64) sm.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
            hlit = 288; hdist = 30;
            __builtin_amdgcn_wave_barrier();
        }
        XCK_PROF_AT(0);
        if (btype == 0) {                                              // stored block: lane 0 finds the byte position, the wave copies
            uint32_t len = 0, s_at = 0;
            if (lane == 0) {
                bi.drop(bi.bc & 7);
                uint32_t c = bi.pos - (uint32_t)(bi.bc >> 3);          // coordinate of the next unread byte
                bi.bb = 0; bi.bc = 0;
                if (c + 4 > c_end) err = 10;
                else {
                    const uint8_t* q = sp - A + c;
                    len = (uint32_t)q[0] | ((uint32_t)q[1] << 8); const uint32_t nlen = (uint32_t)q[2] | ((uint32_t)q[3] << 8);
                    if ((len ^ nlen) != 0xffff) err = 11;
                    c += 4;
                    if (!err && (c + len > c_end || out_end - op < len)) err = 12;
                    s_at = c;
                    // resume the bit stream after the stored bytes: aligned coordinate + partial dword
                    const uint32_t nxt = c + len;
                    bi.pos = nxt & ~3u;                                // the window is moved here below (4-byte aligned for the fill)
                    bi.bc = -(int)(8 * (nxt & 3u));                    // bits to discard once the next words are loaded
                }
            }
            err = __builtin_amdgcn_readfirstlane(err);
            if (err) break;
            len = __builtin_amdgcn_readfirstlane(len); s_at = __builtin_amdgcn_readfirstlane(s_at);
            const uint8_t* s0 = sp - A + s_at;
            for (uint32_t i = lane; i < len; i += 64) o0v[op + i] = s0[i];
            op += len;
            // re-prime the bit buffer for whatever follows the stored block
            { const uint32_t pos = __builtin_amdgcn_readfirstlane(bi.pos); fill(pos & ~3u); bi.wlo = pos & ~3u; }
            if (lane == 0) { const int skip = -bi.bc; bi.bc = 0; bi.bb = 0; bi.refill(win); if (skip) bi.drop(skip); }
        } else {
            __syncthreads();                                           // (the header's scratch is dead: lit[] is the table's again)
            if (!build_table<5>(sm, sm.lens, hlit, D_LIT_TB, sm.lit, D_LIT_MAX, 0, lane)) { err = 20; break; }
            if (!build_table<1>(sm, sm.lens + hlit, hdist, D_DIST_TB, sm.dist, D_DIST_MAX, 1, lane)) { err = 21; break; }
            XCK_PROF_AT(1);
            // ---- symbols, 64 bit offsets at a time.  A symbol's boundaries depend on all symbols before it, but WHAT would be decoded at a
            // given bit offset does not: lane i decodes the literal / length (+ distance) code that starts at bit `bitpos + i` - two
            // table look-ups per lane, all lanes at once -, then a scalar walk (readlane of the code lengths, no vector work) hops from
            // symbol start to symbol start across the 64 offsets.  The lanes that turned out to be starts store their literals in one
            // go (positions by a prefix sum of the output lengths); the matches among them are copied by the whole wave, in order.
            // (The first form of this kernel - lane 0 decoding symbol after symbol, ~45 vector instructions per literal - is archived
            // under profiles/experiments/gpu_inflate/; this loop is 2 - 2.9x faster on its own, r04_symbol_loop_ab.txt.)
            uint32_t bitpos = (uint32_t)__builtin_amdgcn_readfirstlane((int)(bi.pos * 8u - (uint32_t)bi.bc));
            uint32_t wlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)bi.wlo);
            uint32_t dirty_lo = 0;                                     // lowest position stored since the last fence (0 = assume everything)
            // The batched match copy of a round is a load in that round and a store in the NEXT one: what is pending between them is the
            // loaded byte and its destination per lane (PEND_NONE: this lane has none) and, wave-uniform, the batch's lowest destination
            // (PEND_NONE: nothing pending).  The store is issued - and only then counted in dirty_lo, so that a match reading those bytes
            // still finds a fence between that store and its load - before anything later loads output bytes: in the next round ahead
            // of its literal stores and its match phase (batched load or one-by-one copies alike), and behind the loop for whatever
            // follows the block (stored copy, next tables, the epilogue's read-back).  A round that ends in an error drops it: the
            // block's status is non-zero and the host inflates it again.  (Destinations were checked against out_end in their round.)
            constexpr uint32_t PEND_NONE = 0xffffffffu;
            uint32_t pend_dst = PEND_NONE, pend_first = PEND_NONE; uint8_t pend_bv = 0;
            auto retire_pending = [&]() {
                if (pend_first == PEND_NONE) return;
                if (pend_dst != PEND_NONE) o0v[pend_dst] = pend_bv;
                dirty_lo = min(dirty_lo, pend_first);
                pend_dst = PEND_NONE; pend_first = PEND_NONE;
            };
            bool eob = false;
            while (!eob) {
                const uint32_t byte0 = bitpos >> 3;
                if (byte0 < wlo || byte0 + WIN_MARGIN > wlo + IN_WIN) { wlo = byte0 & ~3u; fill(wlo); }   // (bits lane 0 had buffered may lie before a window the header code moved)
                XCK_PROF_AT(2);
                const uint32_t wbase = wlo >> 2;
                const uint32_t bp = bitpos + (uint32_t)lane;
                // 64 stream bits from offset bp in ONE trip to LDS (three dwords, issued together): v for the literal / length code, and the
                // distance code's bits are cut out of (vhi : v) below instead of being read from the window again behind the first look-up.
                // Bounds: bp <= 8 * byte0 + 7 + 63, so its dword starts at byte byte0 + 8 at most and the third dword ends at byte0 + 8 + 11;
                // the refill condition above keeps byte0 + WIN_MARGIN inside the window.
                uint32_t v, vhi;
                { const uint32_t wi = (bp >> 5) - wbase, sh = bp & 31u; const uint32_t w0 = win[wi], w1 = win[wi + 1], w2 = win[wi + 2];
                  v = __builtin_amdgcn_alignbit(w1, w0, sh); vhi = __builtin_amdgcn_alignbit(w2, w1, sh); }
                // a table entry as one 32-bit LDS read: val | len << 16 | op << 24
                uint32_t e = ((const uint32_t*)sm.lit)[v & ((1u << D_LIT_TB) - 1)];
                uint32_t used = (e >> 16) & 0xffu;
                if (e >> 31) { e = ((const uint32_t*)sm.lit)[(e & 0xffffu) + ((v >> D_LIT_TB) & ((1u << ((e >> 24) & 15u)) - 1))]; used = D_LIT_TB + ((e >> 16) & 0xffu); }
                const uint32_t eop = e >> 24;
                // kind: 0 literal, 1 match, 2 end of block, 3 invalid
                uint32_t kind = (eop & 0x50u) == 0x10u ? 1u : 3u;
                kind = eop == 0x20u ? 2u : kind; kind = eop == 0u ? 0u : kind;
                uint32_t mlen = 0, mdist = 0;
                if (kind == 1) {
                    const uint32_t x = eop & 15u;
                    mlen = (e & 0xffffu) + ((v >> used) & ((1u << x) - 1)); used += x;         // <= 20 bits so far
                    const uint32_t v2 = __builtin_amdgcn_alignbit(vhi, v, used);                // 32 bits from bp + used: a distance code + extra bits is <= 28
                    uint32_t dd = ((const uint32_t*)sm.dist)[v2 & ((1u << D_DIST_TB) - 1)];
                    uint32_t u2 = (dd >> 16) & 0xffu;
                    if (dd >> 31) { dd = ((const uint32_t*)sm.dist)[(dd & 0xffffu) + ((v2 >> D_DIST_TB) & ((1u << ((dd >> 24) & 15u)) - 1))]; u2 = D_DIST_TB + ((dd >> 16) & 0xffu); }
                    if (((dd >> 24) & 0xd0u) != 0x10u) kind = 3;
                    else { const uint32_t y = (dd >> 24) & 15u; mdist = (dd & 0xffffu) + ((v2 >> u2) & ((1u << y) - 1)); used += u2 + y; }   // <= 48 bits
                }
                if (used == 0) kind = 3;
                uint32_t olen = kind == 0 ? 1u : (kind == 1 ? mlen : 0u);
                const uint32_t packed = used | (kind << 6) | (olen << 8);
                if constexpr (PROF) { asm volatile("" :: "v"(packed)); }
                XCK_PROF_AT(3);
                // the walk: which lanes start a symbol (scalar); a round ends after 64 offsets or at the end of the block
                uint64_t starts = 0; uint32_t cur = 0, stop = 0, total = 0;
                {
                    // ... four symbols per hop: every lane first learns, through two rounds of ds_bpermute, what a walk that STARTED at it would
                    // cross with its next four symbols (bits, output bytes, which lanes, whether it stops) - the scalar walk then needs
                    // three readlanes per four symbols instead of a readlane and two branches per symbol (the walk was 51 % of a round on the
                    // literal-heavy streams, r04_phase_clocks.txt).  hop word: bits (8) | stop (2) << 8 | output bytes << 10
                    auto join = [](uint32_t a, uint32_t b) { return a + (b & 0xffu) + (b & ~0x3ffu) + (b & 0x300u); };     // (a's stop field is 0 where this is used)
                    const uint32_t h1 = used | ((kind >= 2 ? kind : 0u) << 8) | (olen << 10);
                    const uint32_t lo1 = lane < 32 ? 1u << lane : 0u, hi1 = lane >= 32 ? 1u << (lane - 32) : 0u;
                    const uint32_t s1 = (uint32_t)lane + used; const bool v1 = kind < 2 && s1 < 64;
                    const uint32_t q1 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((s1 & 63u) << 2), (int)h1);
                    const uint32_t h2 = v1 ? join(h1, q1) : h1;
                    const uint32_t lo2 = lo1 | (v1 && s1 < 32 ? 1u << s1 : 0u), hi2 = hi1 | (v1 && s1 >= 32 ? 1u << (s1 - 32) : 0u);
                    const uint32_t s2 = (uint32_t)lane + (h2 & 0xffu); const bool v2 = !(h2 & 0x300u) && s2 < 64;
                    const int a2 = (int)((s2 & 63u) << 2);
                    const uint32_t q2 = (uint32_t)__builtin_amdgcn_ds_bpermute(a2, (int)h2);
                    const uint32_t ql = (uint32_t)__builtin_amdgcn_ds_bpermute(a2, (int)lo2), qh = (uint32_t)__builtin_amdgcn_ds_bpermute(a2, (int)hi2);
                    const uint32_t h4 = v2 ? join(h2, q2) : h2, lo4 = v2 ? lo2 | ql : lo2, hi4 = v2 ? hi2 | qh : hi2;
                    uint32_t slo = 0, shi = 0;
                    while (cur < 64) {
                        const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)h4, (int)cur);
                        slo |= (uint32_t)__builtin_amdgcn_readlane((int)lo4, (int)cur); shi |= (uint32_t)__builtin_amdgcn_readlane((int)hi4, (int)cur);
                        total += p >> 10; cur += p & 0xffu;
                        if (p & 0x300u) { stop = (p >> 8) & 3u; break; }
                    }
                    starts = ((uint64_t)shi << 32) | slo;
                }
                XCK_PROF_AT(4);
                if (stop == 3) { err = 30; break; }
                eob = stop == 2;
                if (total > out_end - op) { err = 33; break; }
                const bool is_start = (starts >> lane) & 1;
                olen = is_start ? olen : 0u;
                const uint32_t off = op + wave_scan_incl(olen) - olen;  // where this lane's output goes
                retire_pending();                                       // (its load is a round old; nothing of this round has read output bytes yet)
                if (is_start && kind == 0) o0v[off] = (uint8_t)e;
                uint64_t mm = starts & __ballot(kind == 1);
                if (starts & ~mm) dirty_lo = min(dirty_lo, op);
                XCK_PROF_AT(5);
                {
                    // All matches of the round in ONE load / store pair, lane j taking the j-th matched byte - when they fit 64 bytes and none
                    // reads what an earlier match of the same round writes (the usual case: a round makes 30 - 60 bytes and a BAM record's
                    // matches reach back a record or more).  The scalar loop over the matches only hands out (source, destination) per lane;
                    // the memory round trip - and the fence, if any source was stored since the last one - is paid once per round instead of
                    // once per match (matches were 44 - 48 % of a round on zlib-6 / Cell Ranger-shaped streams, r04_phase_clocks_4hop.txt).
                    if (mm) {
                        const bool is_m = is_start && kind == 1;
                        const uint32_t minc = wave_scan_incl(is_m ? mlen : 0u);
                        const uint32_t mtot = (uint32_t)__builtin_amdgcn_readlane((int)minc, 63);
                        const uint32_t first_dst = (uint32_t)__builtin_amdgcn_readlane((int)off, __builtin_ctzll(mm));
                        const uint32_t src_lo = off - mdist, src_hi = src_lo + min(mlen, mdist);
                        const bool bad = is_m && mdist > off;
                        const bool dep = is_m && off != first_dst && src_hi > first_dst;        // reads bytes an earlier match of this round makes
                        if (__ballot(bad)) { err = 33; break; }
                        if (mtot <= 64 && !__ballot(dep)) {
                            const bool need_fence = __ballot(is_m && src_hi > dirty_lo) != 0;
                            uint32_t my_src = 0, my_dst = 0; bool act = false;
                            for (uint64_t m2 = mm; m2; m2 &= m2 - 1) {
                                const int l = __builtin_ctzll(m2);
                                const uint32_t ml = (uint32_t)__builtin_amdgcn_readlane((int)mlen, l), md = (uint32_t)__builtin_amdgcn_readlane((int)mdist, l);
                                const uint32_t dst = (uint32_t)__builtin_amdgcn_readlane((int)off, l), mo = (uint32_t)__builtin_amdgcn_readlane((int)minc, l) - ml;
                                const uint32_t t = (uint32_t)lane - mo;
                                if (t < ml) { act = true; my_dst = dst + t; my_src = dst - md + (md >= ml ? t : t % md); }   // (overlapping: the pattern repeats)
                            }
                            if (need_fence) { __threadfence_block(); dirty_lo = 0xffffffffu; }   // a source was stored since the last fence
                            // the load goes out now; its store waits for the next round (retire_pending), so the wave decodes and walks
                            // the next 64 offsets - which read input bits only - while the bytes travel
                            if (act) { pend_bv = o0v[my_src]; pend_dst = my_dst; }
                            pend_first = first_dst;
                            mm = 0;
                        }
                    }
                }
                while (mm) {
                    const int l = __builtin_ctzll(mm); mm &= mm - 1;
                    const uint32_t ml = (uint32_t)__builtin_amdgcn_readlane((int)mlen, l), md = (uint32_t)__builtin_amdgcn_readlane((int)mdist, l);
                    const uint32_t dst = (uint32_t)__builtin_amdgcn_readlane((int)off, l);
                    if (md > dst) { err = 33; break; }
                    const uint32_t src_hi = dst - md + min(ml, md);
                    if (src_hi > dirty_lo) { __threadfence_block(); dirty_lo = 0xffffffffu; }   // the bytes it reads were stored since the last fence
                    const uint8_t* src = o0v + dst - md;
                    if (md >= ml) { for (uint32_t i = lane; i < ml; i += 64) o0v[dst + i] = src[i]; }
                    else { for (uint32_t i = lane; i < ml; i += 64) o0v[dst + i] = src[i % md]; }   // overlapping: the pattern repeats
                    dirty_lo = min(dirty_lo, dst);
                }
                if (err) break;
                XCK_PROF_AT(6);
                op += total; bitpos += cur;
                XCK_PROF_AT(7);
            }
            if (err) break;
            retire_pending();                                          // the last round's batch: the block's output is complete behind this
            // hand the bit position back to lane 0's serial reader (block headers, stored blocks)
            { const uint32_t pos = (bitpos >> 4) << 1;
              if (pos < wlo || pos + 16 > wlo + IN_WIN) { wlo = pos & ~3u; fill(wlo); }
              bi.wlo = wlo; bi.pos = pos; bi.bb = 0; bi.bc = 0; bi.refill(win); bi.drop((int)(bitpos & 15u)); }
        }
        if (bfinal) break;
    }
    {
        // consumed input must lie inside the stream (the window is zero beyond it: a truncated stream must not pass)
        const long long used_bits = (long long)((uint32_t)__builtin_amdgcn_readfirstlane((int)bi.pos) - A) * 8 - __builtin_amdgcn_readfirstlane(bi.bc);
        if (!err && used_bits > (long long)blk.in_len * 8) err = 41;
        if (!err && op != out_end) err = 40;
        // the block's bytes -> the chunk's (mapped, pinned) host block, by the wave that made them: the copy-out then overlaps the other
        // waves' decoding instead of following the whole launch as a kernel of its own (which cost every chunk 1 - 3 ms of latency and
        // sent its 50 MB over PCIe in one burst).  16-byte stores where the block's own bytes fill an aligned 16, single bytes at its ends
        // (the neighbours' bytes are theirs to write).  host_out and out are equally aligned (both allocations are page aligned).
        // CRC: the same pass computes the block's CRC-32 over exactly these bytes (see CrcTables); a mismatch is INFLATE_ST_CRC.
        if ((host_out || CRC) && !err) {
            __threadfence_block();
            const uint8_t* ob = out + blk.out_off; uint8_t* hb = host_out ? host_out + blk.out_off : nullptr; const uint32_t n = blk.out_len;
            const uint32_t head = min((16u - (uint32_t)((uintptr_t)ob & 15u)) & 15u, n), body = (n - head) & ~15u;
            uint32_t* const ctab = reinterpret_cast<uint32_t*>(&sm);       // (the decode tables are dead now)
            if constexpr (CRC) {
                __syncthreads();                                            // every lane is past its last table read
                for (int k = lane; k < CRC_LDS_WORDS; k += 64) ctab[k] = reinterpret_cast<const uint32_t*>(&d_crc)[k];
                __syncthreads();
            }
            if (host_out && (uint32_t)lane < head) hb[lane] = ob[lane];
            uint32_t reg = 0, after = 0;                                    // this lane's register; bytes of the body behind its last piece
            uint32_t h = 0xffffffffu;                                       // lane 0: the register after the head bytes (init included)
            if constexpr (CRC) { if (lane == 0) for (uint32_t k = 0; k < head; k++) h = crc_byte(ctab, h, ob[k]); }
#pragma unroll 2
            for (uint32_t i = (uint32_t)lane * 16; i < body; i += 1024) {
                const uint4 v = *(const uint4*)(ob + head + i);
                if (host_out) *(uint4*)(hb + head + i) = v;
                if constexpr (CRC) {
                    const uint32_t* st = ctab + 4 * 256;
                    uint32_t c = i == 0 ? h : 0u;                           // (piece 0 follows the head: lane 0 goes on from there)
                    c = crc_word(ctab, c, v.x); c = crc_word(ctab, c, v.y); c = crc_word(ctab, c, v.z); c = crc_word(ctab, c, v.w);
                    reg = (st[3 * 256 + (reg >> 24)] ^ st[2 * 256 + ((reg >> 16) & 0xffu)] ^ st[256 + ((reg >> 8) & 0xffu)] ^ st[reg & 0xffu]) ^ c;
                    after = body - i - 16;
                }
            }
            for (uint32_t i = head + body + (uint32_t)lane; host_out && i < n; i += 64) hb[i] = ob[i];
            if constexpr (CRC) {
                if (body == 0 && lane == 0) reg = h;
                const uint32_t tail = n - head - body;
                // reg x^(8 (after + tail)): the bytes behind this lane's last piece (< 1024)
                uint32_t p = 0, m = d_crc.xpow[(after + tail) & 1023u];
#pragma unroll
                for (int k = 31; k >= 0; k--) { p ^= ((reg >> k) & 1u) ? m : 0u; m = (m >> 1) ^ ((m & 1u) ? CRC_POLY : 0u); }
                uint32_t all = wave_xor_all(p);
                if (lane == 0) {
                    uint32_t t = 0;                                         // the tail bytes, from a zero register
                    for (uint32_t k = head + body; k < n; k++) t = crc_byte(ctab, t, ob[k]);
                    if (((all ^ t) ^ 0xffffffffu) != blk.crc) err = INFLATE_ST_CRC;
                }
            }
        }
        if constexpr (PROF) { XCK_PROF_AT(7); if (lane == 0) for (int k = 0; k < 8; k++) atomicAdd(&d_prof[k], prof[k]); }
        if (lane == 0) status[b] = err;
    }
}


// PROF variants (10, 11): the per-phase cycle sums since the last call (and zeroes them)
void dev_inflate_read_prof(unsigned long long out[8]) {
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(d_prof), 8 * sizeof(unsigned long long));
    unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(d_prof), z, sizeof z);
}

int dev_inflate_launch(hipStream_t stream, const uint8_t* d_in, const DevBlock* d_blocks, int n_blocks, uint8_t* d_out, int32_t* d_status, uint8_t* host_out, int variant, bool check_crc) {
    if (n_blocks <= 0) return 0;
    const dim3 g((unsigned)n_blocks), t(64);
    if (variant >= 10) {
        if (check_crc) hipLaunchKernelGGL((k_inflate<true, true>), g, t, 0, stream, d_in, d_blocks, n_blocks, d_out, d_status, host_out);
        else hipLaunchKernelGGL((k_inflate<true, false>), g, t, 0, stream, d_in, d_blocks, n_blocks, d_out, d_status, host_out);
    } else if (check_crc) hipLaunchKernelGGL((k_inflate<false, true>), g, t, 0, stream, d_in, d_blocks, n_blocks, d_out, d_status, host_out);
    else hipLaunchKernelGGL((k_inflate<false, false>), g, t, 0, stream, d_in, d_blocks, n_blocks, d_out, d_status, host_out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int dev_inflate_occupancy(int variant, bool check_crc) {
    int n = 0; hipError_t e;
    if (variant >= 10) e = check_crc ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_inflate<true, true>, 64, 0) : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_inflate<true, false>, 64, 0);
    else e = check_crc ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_inflate<false, true>, 64, 0) : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_inflate<false, false>, 64, 0);
    if (e != hipSuccess) { (void)hipGetLastError(); return -1; }
    return n;
}

// ---- one chunk in flight (see inflate_dev.h) ------------------------------------------------------------------------------
GpuInflateSlot* gpu_inflate_slot_create(int device, int free_cus, bool verbose) {
    if (device < 0 || hipSetDevice(device) != hipSuccess) return nullptr;
    GpuInflateSlot* s = new GpuInflateSlot(); s->device = device;
    // LOWEST stream priority: an inflate launch runs for tens of milliseconds, and on a hardware queue it shares with the engine's
    // streams the join kernels of the chunks being pushed queued up behind it (first version: the coordinator's push time went from
    // 0.25 to 2.6 s per 100 M records)
    // ... and a CU mask that leaves 32 CUs to the engine: the inflate waves live for tens of milliseconds and hold ~14 KB of LDS
    // each; once a few chunks are in flight they fill every CU's LDS, and a join block (26 KB) found no room until some retired
    // (low stream priority does not evict running waves: push time 1.6 s per 100 M records).  Fallback: a low-priority stream.
    hipDeviceProp_t prop;
    bool masked = false;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 64) {
        const int n_cu = prop.multiProcessorCount, keep_free = std::max(8, std::min(free_cus, n_cu / 2));
        uint32_t mask[16] = {0};
        for (int cu = 0; cu < n_cu - keep_free && cu < 512; cu++) mask[cu >> 5] |= 1u << (cu & 31);
        masked = hipExtStreamCreateWithCUMask(&s->stream, (uint32_t)((n_cu + 31) / 32), mask) == hipSuccess;
        if (!masked) { (void)hipGetLastError(); s->stream = nullptr; }
        if (verbose) fprintf(stderr, "[xck] GPU inflate stream: %d CUs, %d kept free of inflate waves: CU mask %s\n", n_cu, keep_free, masked ? "applied" : "REFUSED (low-priority stream instead)");
    }
    if (!masked) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&s->stream, hipStreamNonBlocking, least) != hipSuccess) { gpu_inflate_slot_destroy(s); return nullptr; }
    }
    if (hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess) { gpu_inflate_slot_destroy(s); return nullptr; }
    return s;
}
static void slot_free_buffers(GpuInflateSlot* s) {
    if (s->h_in) hipHostFree(s->h_in); if (s->h_out) hipHostFree(s->h_out); if (s->d_out) hipFree(s->d_out);
    if (s->h_bl) hipHostFree(s->h_bl); if (s->h_st) hipHostFree(s->h_st);
    if (s->d_rec) hipFree(s->d_rec); if (s->d_cnt) hipFree(s->d_cnt); if (s->d_base) hipFree(s->d_base); if (s->h_sum) hipHostFree(s->h_sum); if (s->h_head) hipHostFree(s->h_head);
    if (s->d_nfilt) hipFree(s->d_nfilt); s->d_nfilt = nullptr;
    s->d_rec = nullptr; s->d_cnt = nullptr; s->d_base = nullptr; s->h_sum = s->a_sum = nullptr; s->h_head = s->a_head = nullptr;
    s->h_in = s->a_in = s->h_out = s->a_out = s->d_out = nullptr; s->h_bl = s->a_bl = nullptr; s->h_st = s->a_st = nullptr; s->cap_in = s->cap_out = s->cap_bl = 0;
}
void gpu_inflate_slot_destroy(GpuInflateSlot* s) {
    if (!s) return;
    if (hipSetDevice(s->device) == hipSuccess) {
        if (s->stream) hipStreamSynchronize(s->stream);
        slot_free_buffers(s);
        if (s->done) hipEventDestroy(s->done);
        if (s->stream) hipStreamDestroy(s->stream);
    }
    delete s;
}
bool gpu_inflate_slot_reserve(GpuInflateSlot* s, size_t in_bytes, size_t out_bytes, size_t n_blocks) {
    if (in_bytes <= s->cap_in && out_bytes <= s->cap_out && n_blocks <= s->cap_bl && (!s->parse || s->d_rec)) return true;
    if (hipSetDevice(s->device) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) return false;
    auto grow = [](size_t need, size_t have) { return need > have ? need + need / 4 + 4096 : have; };
    const size_t ci = grow(in_bytes, s->cap_in), co = grow(out_bytes, s->cap_out), cb = grow(n_blocks, s->cap_bl);
    slot_free_buffers(s);
    auto host = [](void** h, void** a, size_t bytes) { return hipHostMalloc(h, bytes, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(a, *h, 0) == hipSuccess; };
    bool ok = host((void**)&s->h_in, (void**)&s->a_in, ci + 16) && host((void**)&s->h_out, (void**)&s->a_out, co + 64) && hipMalloc((void**)&s->d_out, co + 64) == hipSuccess &&
              host((void**)&s->h_bl, (void**)&s->a_bl, cb * sizeof(DevBlock)) && host((void**)&s->h_st, (void**)&s->a_st, cb * sizeof(int32_t));
    if (ok && s->parse)                                                     // device walk + parse: record list, counts, bases, summaries
        ok = hipMalloc((void**)&s->d_rec, dp_rec_capacity(co + 64) * sizeof(DpRec)) == hipSuccess && hipMalloc((void**)&s->d_cnt, cb * sizeof(DpCnt)) == hipSuccess &&
             hipMalloc((void**)&s->d_base, cb * sizeof(DpBase)) == hipSuccess && host((void**)&s->h_sum, (void**)&s->a_sum, cb * sizeof(DpBlockSum)) &&
             host((void**)&s->h_head, (void**)&s->a_head, sizeof(DpHead)) &&
             hipMalloc((void**)&s->d_nfilt, 64) == hipSuccess && hipMemsetAsync(s->d_nfilt, 0, 64, s->stream) == hipSuccess && hipStreamSynchronize(s->stream) == hipSuccess;
    if (!ok) { slot_free_buffers(s); (void)hipGetLastError(); return false; }
    s->cap_in = ci; s->cap_out = co; s->cap_bl = cb;
    return true;
}
// No DMA engine on this path: the first version copied in and out with hipMemcpyAsync, and the engine's own copy of every decoded
// chunk (one hipMemcpyAsync per chunk, csrc/pipeline.hip engine_push_block) queued up behind the 48 MB copy-outs - the coordinator's
// push time rose from 0.25 to 1.6 s per 100 M records.  The kernel is bound by its serial Huffman chain, not by bytes: it takes
// the compressed stream from host memory in 1 KB coalesced windows, every wave stores its finished block to the host block, and the
// statuses go straight back.
int gpu_inflate_slot_launch(GpuInflateSlot* s, size_t in_bytes, size_t out_bytes, size_t n_blocks, bool check_crc, const DpWalk* walk) {
    (void)in_bytes;
    if (hipSetDevice(s->device) != hipSuccess) return -1;
    for (size_t i = 0; i < n_blocks; i++) s->h_st[i] = -1;                  // (a block the kernel never reaches is left to the host)
    (void)out_bytes;
    // (with a device walk behind it the chunk's bytes stay in HBM: nothing is stored to h_out unless the chunk falls back, dev_parse_copy_out)
    if (dev_inflate_launch(s->stream, s->a_in, s->a_bl, (int)n_blocks, s->d_out, s->a_st, walk ? nullptr : s->a_out, s->variant, check_crc) != 0) { (void)hipGetLastError(); return -1; }
    if (walk && dev_walk_launch(s, n_blocks, *walk) != 0) { (void)hipGetLastError(); return -1; }
    if (hipEventRecord(s->done, s->stream) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return 0;
}
bool gpu_inflate_slot_done(GpuInflateSlot* s) { return hipEventQuery(s->done) != hipErrorNotReady; }
int gpu_inflate_slot_wait(GpuInflateSlot* s) { return hipEventSynchronize(s->done) == hipSuccess ? 0 : -1; }

}  // namespace xck
