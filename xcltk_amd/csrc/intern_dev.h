// intern_dev.h - a string intern table in HBM (csrc/intern_dev.hip; XCK_GPU_NAMES): the read names of a UMI-less handle get their keys
// on the device, so the chunks the device walks and parses (parse_dev.h) never visit the host, and the chunks the host parses hand
// their names over with their SoA block.  One table per handle: the same name gets the same key whichever side parsed its chunk.
//
//   slots   open addressing over 64-bit words: bits 0-31 the entry's place in the arena (in 4-byte words, never 0), bits 32-39 the
//           string's length, bits 40-63 hash bits.  0 = empty.  A word is written once, by a CAS from empty, and read by atomic loads.
//   arena   append-only, 4-byte words: an entry is [id][the string's bytes, zero-padded to a word].  Ids are dense (a device counter).
//   insert  a lane that does not find its string reserves an id and arena words (one atomic each per WAVE, behind a ballot), writes
//           its entry, releases at agent scope and publishes with the CAS.  A lane whose CAS loses compares with the winner like any
//           finder and goes on probing; its id and words are wasted.  Nothing waits for anything: there is no locked state.
//           Entry words another workgroup of the same launch may have written are read behind the acquiring load of their slot word,
//           by agent-scope atomic loads (two entries can share a cache line, and a CU's L1 is not refreshed by other CUs' stores).
//   growth  between launches, decided on the host (DevIntern, below): ids and arena offsets are stable, the slots are re-hashed.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime_api.h>
#include "../../include/xck.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XCK_DI_HD __host__ __device__
#else
#define XCK_DI_HD
#endif

namespace xck {

struct DiCtl {                            // the table's counters, device memory; copied to pinned host memory behind every launch
    uint32_t next_id;                     // ids reserved (>= entries: an insert race wastes one)
    uint32_t n_entries;                   // entries published = distinct strings since the last clear
    uint32_t arena_words;                 // arena words reserved (starts at 1: no entry lies at 0)
    uint32_t flags;                       // DI_F_*
    unsigned long long n_lookups;         // strings looked up (found or inserted)
    uint32_t pad[2];
};
constexpr uint32_t DI_F_CAPACITY = 1;     // the id space of the key width is used up (XCK_E_CAPACITY)
constexpr uint32_t DI_F_FULL = 2;         // no free slot / no arena room / a string of more than 255 bytes: the host's arithmetic failed (XCK_E_DEVICE)
struct DiView {                           // what a kernel needs of the table
    unsigned long long* slots; uint64_t mask;
    uint32_t* arena; uint32_t arena_cap;  // in words
    DiCtl* ctl;
    uint64_t hash_keep;                   // hash bits the table uses (XCK_TEST_NAMES_HASH_BITS; all ones otherwise)
    uint64_t id_limit; int32_t umi_bits;  // key = (1 << (umi_bits - 1)) | id, id < id_limit
};
struct DiItem { uint32_t off, len; };     // a host-parsed record's name in the packed bytes behind its chunk's SoA block (len 0: its key is final)
XCK_DI_HD inline uint32_t di_entry_words(uint32_t n) { return 1 + (n + 3) / 4; }   // arena words of an entry of n bytes

// ---- host: the table of one handle ----------------------------------------------------------------------------------------------
// Every call runs on the thread that owns `stream` at that time (the push thread during an ingest, the caller between ingests).
// The host knows the exact counters whenever the stream was waited for (dev_intern_synced) and an upper bound in between: a launch of
// n names can add at most n entries and n entries' words.  dev_intern_reserve grows the table BEFORE a launch that could pass half
// load or the arena's end - a table of twice the slots plus a re-hash kernel, a larger arena plus a copy, all on `stream`.
struct DevIntern {
    int device = -1; size_t slots0 = 0, arena0 = 0; uint64_t hash_keep = ~0ull; bool timing = false;
    unsigned long long* d_slots = nullptr; size_t n_slots = 0; uint32_t* d_arena = nullptr; size_t cap_words = 0;
    DiCtl *d_ctl = nullptr, *h_ctl = nullptr, *h_init = nullptr;      // h_*: pinned
    uint64_t exact_entries = 0, exact_words = 1, exact_ids = 0, pend_names = 0, pend_words = 0;
    uint64_t base_lookups = 0, base_entries = 0;                        // of the clears before the last one (xck_decode_stats sums over clears)
    int growths = 0; double kernel_ms = 0; hipEvent_t ev0 = nullptr, ev1 = nullptr; bool ev_open = false;
};
DevIntern* dev_intern_create(int device, size_t slots0, size_t arena0_bytes, int hash_bits, bool timing);   // allocates nothing on the device yet
void dev_intern_destroy(DevIntern* t);
// room for a launch of up to n names of `bytes` bytes in all; 0, XCK_E_NOMEM or XCK_E_DEVICE
int  dev_intern_reserve(DevIntern* t, hipStream_t stream, size_t n, size_t bytes);
// `stream` has been waited for behind the last launch: the counters are exact; returns DiCtl.flags
uint32_t dev_intern_synced(DevIntern* t);
// empty table (waits for the stream, keeps the buffers); the memsets are ordered on `stream`
int  dev_intern_clear(DevIntern* t, hipStream_t stream);
void dev_intern_stats(const DevIntern* t, int64_t* lookups, int64_t* distinct);   // summed over clears, as of the last dev_intern_synced
void dev_intern_zero_stats(DevIntern* t);
DiView dev_intern_view(const DevIntern* t, int umi_bits, uint64_t id_limit);
// keys of the names of a host-parsed chunk: items[o] / bytes in device memory, umi[o] written where items[o].len != 0
struct GpuInflateSlot; struct SoaLayout;
int  dev_intern_launch_items(DevIntern* t, hipStream_t stream, const DiItem* items, const uint8_t* bytes, size_t n_bytes, uint64_t* umi, size_t n_out, int umi_bits, uint64_t id_limit);
// keys of the read names of a chunk the device walked (the grid of k_parse), into the umi column of its SoA block
int  dev_intern_launch_recs(DevIntern* t, hipStream_t stream, const GpuInflateSlot* s, size_t n_blocks, size_t max_rec, uint64_t* umi, size_t n_out, int umi_bits, uint64_t id_limit);

}  // namespace xck

// ---- device ---------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace xck {

// bam_records.cpp hash_bytes, byte for byte
__device__ inline uint64_t dp_hash_bytes(const uint8_t* s, uint32_t n) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)n * 0xff51afd7ed558ccdull);
    while (n >= 8) { uint64_t w = 0; for (int k = 0; k < 8; k++) w |= (uint64_t)s[k] << (8 * k); h = (h ^ w) * 0xbf58476d1ce4e5b9ull; h ^= h >> 32; s += 8; n -= 8; }
    if (n) { uint64_t w = 0; for (uint32_t k = 0; k < n; k++) w |= (uint64_t)s[k] << (8 * k); h = (h ^ w) * 0x94d049bb133111ebull; }
    h ^= h >> 29; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 32;
    return h;
}
// bam_records.cpp encode_key_direct: the keys that need no table - empty -> NONE, short ACGT -> 2-bit code.  false: the string is interned
__device__ inline bool dp_encode_direct(const uint8_t* s, size_t n, int umi_bits, uint64_t* out) {
    if (n == 0) { *out = XCK_UMI_NONE; return true; }
    bool ok = 2 * (long long)n + 1 <= (long long)umi_bits - 1;
    uint64_t v = 1;
    for (size_t k = 0; ok && k < n; k++) {
        const uint8_t ch = s[k];
        const uint32_t code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
        ok = code < 4u; v = (v << 2) | (code & 3u);
    }
    if (ok) *out = v;
    return ok;
}

#define XCK_DI_AGENT __HIP_MEMORY_SCOPE_AGENT
// word k of a string as the arena holds it (little-endian, zero-padded)
__device__ inline uint32_t di_src_word(const uint8_t* s, uint32_t n, uint32_t k) {
    uint32_t w = 0;
    for (uint32_t j = 0; j < 4; j++) { const uint32_t i = 4 * k + j; if (i < n) w |= (uint32_t)s[i] << (8 * j); }
    return w;
}
__device__ inline uint32_t di_tag(uint64_t h, uint32_t n) { return ((uint32_t)(h >> 40) << 8) | n; }   // the upper half of a slot word
// is the entry of slot word w the string (s, n) of hash h?  Length and hash bits first, then every byte: a hash never decides alone.
// (behind an acquiring load of w; the entry's words by agent-scope loads)
__device__ inline bool di_same(const DiView& v, unsigned long long w, const uint8_t* s, uint32_t n, uint64_t h, uint32_t* id) {
    if ((uint32_t)(w >> 32) != di_tag(h, n)) return false;
    const uint32_t at = (uint32_t)w, nw = (n + 3) / 4;
    if (at == 0 || (uint64_t)at + 1 + nw > v.arena_cap) return false;      // (never for a word this table wrote)
    for (uint32_t k = 0; k < nw; k++)
        if (__hip_atomic_load(v.arena + at + 1 + k, __ATOMIC_RELAXED, XCK_DI_AGENT) != di_src_word(s, n, k)) return false;
    *id = __hip_atomic_load(v.arena + at, __ATOMIC_RELAXED, XCK_DI_AGENT);
    return true;
}

// The key of string (s, n) of every lane with `want` (others: XCK_UMI_NONE): the host's rule - directly codable strings need no table,
// the rest is (1 << (umi_bits - 1)) | id.  ALL 64 lanes of a wave call this together, from convergent code: the reservation is one
// ballot and one atomic per counter for the wave.  The probe loops diverge, but no lane ever waits for another.
__device__ inline uint64_t di_key_wave(const DiView& v, const uint8_t* s, uint32_t n, bool want, int lane) {
    uint64_t key = XCK_UMI_NONE;
    bool need = false;
    if (want) need = !dp_encode_direct(s, n, v.umi_bits, &key);
    if (need && n > 255) { atomicOr(&v.ctl->flags, DI_F_FULL); need = false; }   // (a BAM read name has at most 254 bytes)
    uint64_t h = 0, pos = 0; uint32_t id = 0; bool found = false;
    if (need) {                                                            // find
        h = dp_hash_bytes(s, n) & v.hash_keep; pos = h & v.mask;
        for (uint64_t steps = 0;; steps++) {
            if (steps > v.mask) { atomicOr(&v.ctl->flags, DI_F_FULL); need = false; break; }
            const unsigned long long w = __hip_atomic_load(v.slots + pos, __ATOMIC_ACQUIRE, XCK_DI_AGENT);
            if (w == 0) break;
            if (di_same(v, w, s, n, h, &id)) { found = true; break; }
            pos = (pos + 1) & v.mask;
        }
    }
    const unsigned long long b_need = __ballot(need);
    const bool ins = need && !found;                                       // pos: the empty slot its probe ended at
    const unsigned long long b_ins = __ballot(ins);
    bool won = false;
    if (b_ins) {                                                           // (uniform) reserve ids and arena words for the wave
        const uint32_t words = ins ? di_entry_words(n) : 0u;
        uint32_t incl = words;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if (lane >= d) incl += t; }
        const uint32_t total = __shfl(incl, 63);
        uint32_t base_id = 0, base_w = 0;
        if (lane == 0) { base_id = atomicAdd(&v.ctl->next_id, (uint32_t)__popcll(b_ins)); base_w = atomicAdd(&v.ctl->arena_words, total); }
        base_id = __shfl(base_id, 0); base_w = __shfl(base_w, 0);
        if (ins) {
            const uint32_t my_id = base_id + (uint32_t)__popcll(b_ins & ((1ull << lane) - 1)), my_w = base_w + incl - words;
            if ((uint64_t)my_id >= v.id_limit || my_id < base_id) atomicOr(&v.ctl->flags, DI_F_CAPACITY);
            else if (my_w < base_w || (uint64_t)my_w + words > v.arena_cap) atomicOr(&v.ctl->flags, DI_F_FULL);
            else {
                v.arena[my_w] = my_id;
                for (uint32_t k = 0; k + 1 < words; k++) v.arena[my_w + 1 + k] = di_src_word(s, n, k);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");           // the entry before the word that publishes it
                const unsigned long long mine = (unsigned long long)my_w | ((unsigned long long)di_tag(h, n) << 32);
                for (uint64_t steps = 0;; steps++) {
                    if (steps > v.mask) { atomicOr(&v.ctl->flags, DI_F_FULL); break; }
                    unsigned long long seen = 0;
                    if (__hip_atomic_compare_exchange_strong(v.slots + pos, &seen, mine, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, XCK_DI_AGENT)) { id = my_id; found = true; won = true; break; }
                    if (di_same(v, seen, s, n, h, &id)) { found = true; break; }   // somebody else's entry of the same string: ours is wasted
                    pos = (pos + 1) & v.mask;
                }
            }
        }
    }
    if (found) key = (1ull << (v.umi_bits - 1)) | (uint64_t)id;
    const unsigned long long b_won = __ballot(won);
    if (lane == 0) {
        if (b_won) atomicAdd(&v.ctl->n_entries, (uint32_t)__popcll(b_won));
        if (b_need) atomicAdd(&v.ctl->n_lookups, (unsigned long long)__popcll(b_need));
    }
    return key;
}

}  // namespace xck
#endif
