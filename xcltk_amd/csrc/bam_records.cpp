// bam_records.cpp - the BAM decoder's work on one chunk, none of which knows a reader (bam.cpp): key codes and the host intern table,
// the barcode map, BGZF block header and inflate, the SoA block, the speculative record walk, the record parse and the layout.
//
// Written from the SAM/BAM specification (SAMv1 section 4); htslib is not available here.  What runs once per record or once per BGZF
// block inside a pool task lives in THIS unit, so that the compiler makes one loop of it: run_part -> bgzf_inflate -> inflate_raw, and
// parse_part -> parse_record -> aux_skip / lookup_cell / encode_key / hash_bytes / intern_batch.
#include <zlib.h>
#include <algorithm>
#include <cstdlib>
#include "bam_decode.h"
#include "inflate_fast.h"

namespace xck {

uint64_t hash_bytes(const char* s, size_t n) {                       // 8 bytes per step (read names are 20-40 characters)
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (n * 0xff51afd7ed558ccdull);
    while (n >= 8) { uint64_t w; memcpy(&w, s, 8); h = (h ^ w) * 0xbf58476d1ce4e5b9ull; h ^= h >> 32; s += 8; n -= 8; }
    if (n) { uint64_t w = 0; memcpy(&w, s, n); h = (h ^ w) * 0x94d049bb133111ebull; }
    h ^= h >> 29; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 32;
    return h;
}

void InternTable::Shard::grow() {
    const size_t ncap = slots.empty() ? 1024 : slots.size() * 2;
    std::vector<Slot> ns(ncap, Slot{0, 0, 0, 0, 0});
    for (const Slot& sl : slots) if (sl.epoch == epoch) {
        size_t i = (size_t)(sl.h >> 6) & (ncap - 1);
        while (ns[i].epoch == epoch) i = (i + 1) & (ncap - 1);
        ns[i] = sl;
    }
    slots.swap(ns);
}

// test hook: XCK_TEST_INTERN_LIMIT=<n> makes the id space of 64-bit keys overflow after n ids (tests/test_gpu_frontends.py
// exercises the front-ends' retry with 128-bit keys without 2^25 distinct read names)
static const uint64_t g_test_intern_limit = [] { const char* e = getenv("XCK_TEST_INTERN_LIMIT"); return e ? (uint64_t)strtoull(e, nullptr, 10) : ~0ull; }();
uint64_t intern_id_limit(int umi_bits) {
    return umi_bits >= 64 ? (1ull << 63) - 1 : std::min<uint64_t>((1ull << (umi_bits - 1)) - 1, g_test_intern_limit);
}

// the id of a string in its shard, added if it is new; the caller holds the shard's lock and has made room (grow)
inline uint64_t InternTable::probe_or_insert(Shard& sh, uint64_t h, const char* s, uint32_t n) {
    const size_t mask = sh.slots.size() - 1;
    size_t i = (size_t)(h >> 6) & mask;
    for (;;) {
        Slot& sl = sh.slots[i];
        if (sl.epoch != sh.epoch) {
            sl.h = h; sl.off = (uint32_t)sh.arena.size(); sl.len1 = n + 1; sl.idx = sh.count++; sl.epoch = sh.epoch;
            sh.arena.insert(sh.arena.end(), s, s + n);
            break;
        }
        if (sl.h == h && sl.len1 == n + 1 && memcmp(sh.arena.data() + sl.off, s, n) == 0) break;
        i = (i + 1) & mask;
    }
    return ((uint64_t)sh.slots[i].idx << 6) | (h & (NSHARD - 1));
}

uint64_t InternTable::intern(const char* s, size_t n) {
    const uint64_t h = hash_bytes(s, n);
    Shard& sh = shards_[h & (NSHARD - 1)];
    std::lock_guard<std::mutex> lk(sh.mu);
    if ((size_t)(sh.count + 1) * 2 > sh.slots.size()) sh.grow();
    return probe_or_insert(sh, h, s, (uint32_t)n);
}
uint64_t InternTable::hash(const char* s, size_t n) { return hash_bytes(s, n); }

// UMI-less mode interns every read name: per string the shared table costs a lock and two cache misses (the table of a
// 2 M-read BAM is ~100 MB).  A parse task therefore collects its names and hands them over here, sorted by shard: one
// lock per shard, and the probes of a shard (1/64 of the table) hit the cache.
void InternTable::intern_batch(std::vector<Item>& items, bool* overflow) {
    std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return (a.h & (NSHARD - 1)) < (b.h & (NSHARD - 1)); });
    size_t i = 0;
    while (i < items.size()) {
        const unsigned shard = (unsigned)(items[i].h & (NSHARD - 1));
        Shard& sh = shards_[shard];
        std::lock_guard<std::mutex> lk(sh.mu);
        for (; i < items.size() && (items[i].h & (NSHARD - 1)) == shard; i++) {
            const Item& it = items[i];
            if ((size_t)(sh.count + 1) * 2 > sh.slots.size()) sh.grow();
            const size_t mask = sh.slots.size() - 1;
            if (i + 4 < items.size()) __builtin_prefetch(&sh.slots[(size_t)(items[i + 4].h >> 6) & mask]);
            const uint64_t id = probe_or_insert(sh, it.h, it.s, it.n);
            const uint64_t lim = intern_id_limit(it.umi_bits);
            if (id >= lim) { if (overflow) *overflow = true; *it.out = XCK_UMI_NONE; }
            else *it.out = (1ull << (it.umi_bits - 1)) | id;
        }
    }
}
uint64_t InternTable::size() const { uint64_t n = 0; for (auto& s : shards_) n += s.count; return n; }
void InternTable::clear() {
    for (auto& s : shards_) {
        std::lock_guard<std::mutex> lk(s.mu);
        s.arena.clear(); s.count = 0;
        if (++s.epoch == 0) { std::fill(s.slots.begin(), s.slots.end(), Slot{0, 0, 0, 0, 0}); s.epoch = 1; }   // slots of older epochs read as empty
    }
}

// the part of encode_key() that needs no table: empty string -> NONE, short ACGT string -> 2-bit code
bool encode_key_direct(const char* s, size_t n, int umi_bits, uint64_t* out) {
    if (n == 0) { *out = XCK_UMI_NONE; return true; }
    if (2 * (int)n + 1 <= umi_bits - 1) {
        // A C G T -> 0 1 2 3, anything else 4: one table look-up per character, no branch inside the loop
        static const struct Lut { uint8_t t[256]; Lut() { memset(t, 4, sizeof t); t[(uint8_t)'A'] = 0; t[(uint8_t)'C'] = 1; t[(uint8_t)'G'] = 2; t[(uint8_t)'T'] = 3; } } lut;
        uint64_t v = 1; unsigned bad = 0;
        for (size_t i = 0; i < n; i++) { const unsigned c = lut.t[(uint8_t)s[i]]; bad |= c; v = (v << 2) | (c & 3u); }
        if (!(bad & 4u)) { *out = v; return true; }
    }
    return false;
}

uint64_t encode_key(const char* s, size_t n, int umi_bits, InternTable& tab, bool* overflow) {
    uint64_t direct;
    if (encode_key_direct(s, n, umi_bits, &direct)) return direct;
    uint64_t id = tab.intern(s, n);
    const uint64_t lim = intern_id_limit(umi_bits);
    if (id >= lim) { if (overflow) *overflow = true; return XCK_UMI_NONE; }
    return (1ull << (umi_bits - 1)) | id;
}

// Barcode -> column: open addressing over slots that hold the full 64-bit hash, the column and the barcode's own bytes (up to
// 18, the length of a 10x barcode), so a hit costs ONE cache line and still compares the exact string; longer barcodes compare against
// the string list.  (Slots -> std::string -> heap was three dependent misses per read.)
void DecodeCfg::build_barcodes(const char* const* names, int n) {
    barcodes.clear();
    for (int i = 0; i < n; i++) barcodes.emplace_back(names[i]);
    size_t cap = 16; while (cap < (size_t)n * 2) cap <<= 1;
    BcSlot empty; memset(&empty, 0, sizeof empty); empty.idx = -1;
    bc_slots.assign(cap, empty); bc_mask = cap - 1;
    for (int i = 0; i < n; i++) {
        const std::string& b = barcodes[i];
        const uint64_t hh = hash_bytes(b.data(), b.size());
        uint64_t h = hh & bc_mask;
        while (bc_slots[h].idx >= 0) h = (h + 1) & bc_mask;
        BcSlot& sl = bc_slots[h];
        sl.h = hh; sl.idx = i; sl.len = (uint16_t)std::min<size_t>(b.size(), 0xFFFF);
        memcpy(sl.key, b.data(), std::min<size_t>(b.size(), sizeof sl.key));
    }
}
int32_t DecodeCfg::lookup_cell(const char* s, size_t n) const {
    if (bc_slots.empty()) return -1;
    const uint64_t hh = hash_bytes(s, n);
    uint64_t h = hh & bc_mask;
    while (bc_slots[h].idx >= 0) {
        const BcSlot& sl = bc_slots[h];
        if (sl.h == hh && sl.len == (n > 0xFFFF ? 0xFFFF : (uint16_t)n)) {
            if (n <= sizeof sl.key) { if (memcmp(sl.key, s, n) == 0) return sl.idx; }
            else { const std::string& b = barcodes[sl.idx]; if (b.size() == n && memcmp(b.data(), s, n) == 0) return sl.idx; }
        }
        h = (h + 1) & bc_mask;
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------
// BGZF
// ---------------------------------------------------------------------------------------------
// parse one BGZF block header at file offset `coff`; returns false at EOF / on malformed data
bool bgzf_peek(const uint8_t* map, uint64_t fsize, uint64_t coff, BlockRef* out, std::string* err) {
    if (coff + 18 > fsize) { if (coff != fsize && err) *err = "truncated BGZF block header"; return false; }
    const uint8_t* p = map + coff;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) { if (err) *err = "not a BGZF block (bad gzip magic)"; return false; }
    uint32_t xlen = le16(p + 10);
    if (coff + 12 + xlen > fsize) { if (err) *err = "truncated BGZF extra field"; return false; }
    const uint8_t* x = p + 12; const uint8_t* xe = x + xlen;
    int64_t bsize = -1;
    while (x + 4 <= xe) { uint32_t sl = le16(x + 2); if (x + 4 + sl > xe) break;          // subfield payload must lie inside the extra field
                          if (x[0] == 'B' && x[1] == 'C' && sl == 2) { bsize = le16(x + 4); } x += 4 + sl; }
    if (bsize < 0) { if (err) *err = "BGZF block without BC subfield"; return false; }
    uint32_t total = (uint32_t)bsize + 1;
    if (coff + total > fsize || total < 12 + xlen + 8) { if (err) *err = "truncated BGZF block"; return false; }
    out->coff = coff; out->clen = total; out->data_off = 12 + xlen; out->data_len = total - (12 + xlen) - 8;
    out->isize = le32(p + total - 4); out->uoff = 0;
    if (out->isize > 65536) { if (err) *err = "BGZF block claims more than 64 KiB of data"; return false; }   // SAMv1 4.1: ISIZE <= 65536
    return true;
}

static std::atomic<long> g_inflate_fallbacks{0};
static const bool g_use_fast_inflate = [] { const char* e = getenv("XCK_INFLATE"); return !(e && strcmp(e, "zlib") == 0); }();
static thread_local InflateTables t_inflate_tables;
struct ZStream { z_stream zs; bool ok; ZStream() { memset(&zs, 0, sizeof zs); ok = inflateInit2(&zs, -15) == Z_OK; } ~ZStream() { if (ok) inflateEnd(&zs); } };
static thread_local ZStream t_zs;

bool bgzf_inflate(const uint8_t* map, const BlockRef& b, uint8_t* dst, bool verify_crc, std::string* err) {
    if (!t_zs.ok) { if (err && err->empty()) *err = "inflate init failed"; return false; }
    if (b.isize == 0) return true;
    z_stream* const zs = &t_zs.zs;
    bool done = false;
    if (g_use_fast_inflate) {                                  // own whole-buffer decoder (inflate_fast.h); zlib on any irregularity
        done = inflate_raw(map + b.coff + b.data_off, b.data_len, dst, b.isize, &t_inflate_tables) == 0;
        if (!done) g_inflate_fallbacks.fetch_add(1, std::memory_order_relaxed);
    }
    if (!done) {
        inflateReset(zs);
        zs->next_in = const_cast<Bytef*>(map + b.coff + b.data_off); zs->avail_in = b.data_len;
        zs->next_out = dst; zs->avail_out = b.isize;
        int rc = inflate(zs, Z_FINISH);
        if (rc != Z_STREAM_END || zs->avail_out != 0) { if (err) *err = "BGZF inflate failed"; return false; }
    }
    if (verify_crc) {
        uint32_t want = le32(map + b.coff + b.clen - 8);
        if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, b.isize) != want) { if (err) *err = "BGZF CRC mismatch in the block at compressed offset " + std::to_string(b.coff); return false; }
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// the SoA block of a chunk
// ---------------------------------------------------------------------------------------------
void soa_free(HostSoA& s) {
    if (s.fence) { fence_wait(s.fence); fence_destroy(s.fence); }
    if (s.base) { if (s.pinned) pinned_free(s.base); else free(s.base); }
    s = HostSoA();
}
// carve the columns of a chunk with n_reads kept records out of the block (growing it if needed)
bool soa_reserve(HostSoA& s, size_t n_reads, size_t n_cig, size_t n_seq, size_t name_items, size_t name_bytes, bool names, bool qual) {
    const SoaLayout l = soa_layout(n_reads, n_cig, n_seq);                // (parse_dev.h: the parse kernel writes the same block)
    const size_t items_bytes = (name_items * sizeof(DiItem) + 255) & ~size_t(255);
    const size_t qual_bytes = qual ? soa_qual_bytes(n_seq) : 0;           // (the qualities: behind the layout's total, in front of the names)
    const size_t total = l.total + qual_bytes + (names ? items_bytes + ((name_bytes + 255) & ~size_t(255)) : 0);   // (the names: a trailer behind them)
    if (total > s.cap) {
        if (s.fence) fence_wait(s.fence);
        if (s.base) { if (s.pinned) pinned_free(s.base); else free(s.base); }
        const size_t c = total + total / 4;
        s.base = (uint8_t*)pinned_alloc(c); s.pinned = s.base != nullptr;
        if (!s.base) s.base = (uint8_t*)malloc(c);
        if (!s.base) { s.cap = 0; return false; }
        s.cap = c;
    }
    s.used = total;
    s.umi = (uint64_t*)(s.base + l.o_umi); s.pos = (int32_t*)(s.base + l.o_pos); s.cell = (int32_t*)(s.base + l.o_cell);
    s.cig_off = (uint32_t*)(s.base + l.o_cgo); s.seq_off = (uint32_t*)(s.base + l.o_sqo); s.cigar = (uint32_t*)(s.base + l.o_cig);
    s.flag = (uint16_t*)(s.base + l.o_flag); s.mapq = s.base + l.o_mapq; s.seq = s.base + l.o_seq;
    s.qual = qual ? s.base + l.total : nullptr;
    s.has_names = names; s.nt = NameTrailer{l.total + qual_bytes, l.total + qual_bytes + items_bytes, name_bytes, names ? name_items : 0};
    s.items = names ? (DiItem*)(s.base + s.nt.items_off) : nullptr; s.name_bytes = names ? s.base + s.nt.bytes_off : nullptr;
    return true;
}

// a batch = a slice of the chunk's SoA block
void fill_batch(const HostSoA& s, const PendingBatch& pb, bool want_seq, xck_batch* bt) {
    memset(bt, 0, sizeof *bt);
    bt->contig = pb.contig; bt->n_reads = (int32_t)(pb.r1 - pb.r0); bt->ordinal_base = pb.ordinal_base;
    bt->pos = s.pos + pb.r0; bt->flag = s.flag + pb.r0; bt->mapq = s.mapq + pb.r0; bt->cell = s.cell + pb.r0; bt->umi = s.umi + pb.r0;
    bt->cig_off = s.cig_off + pb.r0; bt->cigar = s.cigar;
    if (want_seq) { bt->seq_off = s.seq_off + pb.r0; bt->seq = s.seq; }
}

// One part of a chunk: inflate its blocks (all of them, or - st given - only those the GPU kernel left: status != 0), then walk the
// records of its byte range speculatively.  Pool task.
// verify_crc: every non-empty block it inflates is CRC-checked (dstat: the reader's counters); a block the kernel found damaged
// (INFLATE_ST_CRC) that passes here is a disagreement of device and host.
void run_part(Chunk* cp, const uint8_t* map, bool verify_crc, WalkPart* wpp, DecodeTimes* tmp_, const ContigMap cm, bool want_seq, const int32_t* st,
              std::atomic<int64_t>* dstat) {
    if (!t_zs.ok) { cp->failed = true; return; }
    const auto t_a = std::chrono::steady_clock::now();
    struct Acc { DecodeTimes* t; std::chrono::steady_clock::time_point a, b; bool walked = false;
                 ~Acc() { const auto e = std::chrono::steady_clock::now(); if (!walked) b = e;
                          t->inflate += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count();
                          t->walk += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(e - b).count(); } } acc{tmp_, t_a, t_a};
    for (size_t i = wpp->i0; i < wpp->i1; i++) {
        if (st && st[i] == 0) continue;
        std::string e;
        if (!bgzf_inflate(map, cp->blocks[i], cp->ubase + cp->blocks[i].uoff, verify_crc, &e)) {
            std::lock_guard<std::mutex> lk(cp->emu); cp->failed = true; cp->err = e; return;
        }
        if (verify_crc && cp->blocks[i].isize) {
            dstat[DS_CRC_HOST].fetch_add(1, std::memory_order_relaxed);
            if (st && st[i] == INFLATE_ST_CRC) dstat[DS_CRC_DISAGREE].fetch_add(1, std::memory_order_relaxed);
        }
    }
    // speculative record walk over this range
    acc.b = std::chrono::steady_clock::now(); acc.walked = true;
    const uint8_t* u = cp->ubase; size_t o = wpp->spec_start; const size_t end = wpp->u_end;
    if (o > end) { wpp->stop = o; return; }
    int32_t cur_c = INT32_MIN;
    while (o + 4 <= end) {
        uint32_t bs = le32(u + o);
        if (bs < 32 || o + 4 + (size_t)bs > end) break;
        const uint8_t* r = u + o + 4;
        // (a device chunk's bytes come from the GPU, not from this core's inflate: the hop from header to header is a chain of cache
        // misses unless the lines a few records ahead are asked for early)
        { const uint8_t* pf = r + 4096; __builtin_prefetch(pf); __builtin_prefetch(pf + 64); __builtin_prefetch(pf + 128); __builtin_prefetch(pf + 192); }   // (every line of the stretch ~18 records ahead: a header may sit on any of them)
        const RecRef rr{r, bs, (int32_t)le32(r), le32(r + 16), le16(r + 12)};
        const int32_t ctg = cm(rr.tid, (int32_t)le32(r + 4));
        if (ctg != cur_c) { wpp->runs.push_back({(uint32_t)wpp->recs.size(), ctg}); cur_c = ctg; }
        if (ctg >= 0) { wpp->n_out++; wpp->n_cig += rr.n_cig; if (want_seq) wpp->n_seq += (rr.l_seq + 1) / 2; wpp->n_name += r[8]; }
        wpp->recs.push_back(rr);
        o += 4 + (size_t)bs;
    }
    wpp->stop = o;
}

// locate a 2-character aux tag; returns pointer to the type byte or nullptr
static inline const uint8_t* aux_skip(const uint8_t* p, const uint8_t* e) {       // p at type byte; returns next tag or nullptr
    if (p >= e) return nullptr;
    uint8_t t = *p++;
    switch (t) {
        case 'A': case 'c': case 'C': p += 1; break;
        case 's': case 'S': p += 2; break;
        case 'i': case 'I': case 'f': p += 4; break;
        case 'Z': case 'H': { const void* z = memchr(p, 0, (size_t)(e - p)); if (!z) return nullptr; p = (const uint8_t*)z + 1; break; }
        case 'B': { if (p + 5 > e) return nullptr; uint8_t st = *p; uint32_t n = le32(p + 1); p += 5;
                    size_t sz = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4; p += (size_t)n * sz; break; }
        default: return nullptr;
    }
    return p <= e ? p : nullptr;
}

// one record -> SoA slot o (cig_off[o] / seq_off[o] are already set); true: the handle's tag filter rejected it
static inline bool parse_record(const DecodeCfg& dc, xck_engine* e, HostSoA& s, const uint8_t* p, uint32_t len, int64_t o, int32_t sample,
                                std::vector<InternTable::Item>& names, std::atomic<int>* flags) {
        const uint8_t* end = p + len;
        uint32_t l_name = p[8], n_cig = le16(p + 12), l_seq = le32(p + 16);
        s.pos[o] = (int32_t)le32(p + 4);
        s.mapq[o] = p[9];
        s.flag[o] = le16(p + 14);
        const uint8_t* q = p + 32;
        const char* qname = (const char*)q; size_t qlen = l_name ? l_name - 1 : 0;
        q += l_name;
        if (q + (size_t)n_cig * 4 + (l_seq + 1) / 2 + l_seq > end) { flags->fetch_or(1); s.cell[o] = -1; s.umi[o] = XCK_UMI_NONE; return false; }
        memcpy(s.cigar + s.cig_off[o], q, (size_t)n_cig * 4);
        q += (size_t)n_cig * 4;
        if (dc.want_seq) memcpy(s.seq + s.seq_off[o], q, (l_seq + 1) / 2);
        if (s.qual) {                                                     // the l_seq quality bytes, two per sequence byte: the pad of an odd read is "no quality"
            uint8_t* const qd = s.qual + 2 * (size_t)s.seq_off[o];
            memcpy(qd, q + (l_seq + 1) / 2, l_seq);
            if (l_seq & 1) qd[l_seq] = 0xff;
        }
        q += (l_seq + 1) / 2 + l_seq;
        // aux tags: first occurrence wins (htslib bam_aux_get)
        // (xf: the handle's tag filter, looked for only when it is on - a record without the tag is then walked to its end)
        const uint8_t* cb = nullptr; const uint8_t* ub = nullptr; const uint8_t* xf = nullptr;
        bool need_cb = dc.use_barcodes, need_ub = dc.use_umi, need_xf = dc.filter_on;
        const uint8_t* a = q;
        while ((need_cb || need_ub || need_xf) && a && a + 3 <= end) {
            if (need_cb && a[0] == (uint8_t)dc.cell_tag[0] && a[1] == (uint8_t)dc.cell_tag[1]) { cb = a + 2; need_cb = false; }
            else if (need_ub && a[0] == (uint8_t)dc.umi_tag[0] && a[1] == (uint8_t)dc.umi_tag[1]) { ub = a + 2; need_ub = false; }
            else if (need_xf && a[0] == (uint8_t)dc.filter_tag[0] && a[1] == (uint8_t)dc.filter_tag[1]) { xf = a + 2; need_xf = false; }
            a = aux_skip(a + 2, end);
        }
        int32_t cell = -1;
        if (dc.use_barcodes) {
            if (cb && (*cb == 'Z' || *cb == 'A' || *cb == 'H')) {         // get_tag() returns str only for these
                const char* v = (const char*)cb + 1; size_t n = (*cb == 'A') ? 1 : strnlen(v, (size_t)(end - (cb + 1)));
                cell = dc.lookup_cell(v, n);
            }
        } else cell = sample;
        // the tag filter's verdict overrides the cell: absent, not an integer, negative or cut off -> filtered (parse_dev.h tag_filter_pass)
        const bool filtered = dc.filter_on && !(xf && aux_skip(xf, end) && tag_filter_pass(xf, dc.filter_mask, dc.filter_value));
        if (filtered) cell = XCK_CELL_FILTERED;
        s.cell[o] = cell;
        uint64_t key = XCK_UMI_NONE; bool ovf = false;
        if (dc.use_umi) {
            if (ub) {
                if (*ub == 'Z' || *ub == 'A' || *ub == 'H') {
                    const char* v = (const char*)ub + 1; size_t n = (*ub == 'A') ? 1 : strnlen(v, (size_t)(end - (ub + 1)));
                    key = encode_key(v, n, dc.umi_bits, e->intern, &ovf);
                } else {                                                   // numeric tag: get_tag() gives a number; the key is its VALUE
                    // (an int 0 / float 0.0 is falsy: `if not umi` skips the read, rdr/fc/mcount.py:41, baf/fc/mcount.py:116-117)
                    const uint8_t* nx = aux_skip(ub, end);
                    bool zero = false; std::string t("\1num:");
                    if (nx) {
                        const uint8_t* v = ub + 1; long long iv = 0; bool is_int = true;
                        switch (*ub) { case 'c': iv = (int8_t)v[0]; break; case 'C': iv = v[0]; break; case 's': iv = (int16_t)le16(v); break; case 'S': iv = le16(v); break;
                                       case 'i': iv = (int32_t)le32(v); break; case 'I': iv = le32(v); break; default: is_int = false; }
                        if (is_int) { zero = iv == 0; t += std::to_string(iv); }          // equal integers are equal keys whatever their storage width
                        else if (*ub == 'f') { float f; memcpy(&f, v, 4); zero = f == 0.0f; t.append("f", 1); t.append((const char*)v, 4); }
                        else t.append((const char*)ub, (size_t)(nx - ub));                 // B arrays: their bytes
                    }
                    if (!zero) key = encode_key(t.data(), t.size(), dc.umi_bits, e->intern, &ovf);
                }
            }
        } else if (encode_key_direct(qname, qlen, dc.umi_bits, &key)) { /* empty or 2-bit codable name */ }
        else { names.push_back(InternTable::Item{InternTable::hash(qname, qlen), qname, (uint32_t)qlen, 0, &s.umi[o], dc.umi_bits}); key = XCK_UMI_NONE; }
        if (ovf) flags->fetch_or(2);
        s.umi[o] = key;
        return filtered;
}

// the records of one piece of a chunk (a walk part, or a piece of the serial stitch), whose output slots start at the piece's bases
// (prefix sums over the pieces: layout_chunk)
void parse_part(DecodeTimes* tm, xck_engine* e, HostSoA* sp, int32_t sample, const WalkPart* wp, const ContigMap cm, std::atomic<int>* flags,
                std::atomic<int64_t>* n_filtered) {
    const auto t_parse0 = std::chrono::steady_clock::now();
    struct PAcc { DecodeTimes* tm; std::chrono::steady_clock::time_point t0; ~PAcc() { tm->parse += ns_since(t0); } } pacc{tm, t_parse0};
    const DecodeCfg& dc = e->dec;
    HostSoA& s = *sp;
    std::vector<InternTable::Item> names;
    if (!dc.use_umi) names.reserve(wp->n_out);
    int64_t nf = 0;                                                       // records of the piece the tag filter rejected
    int64_t o = (int64_t)wp->out_base; uint32_t co = (uint32_t)wp->cig_base, so = (uint32_t)wp->seq_base;
    const RecRef* const rend = wp->recs.data() + wp->recs.size();
    for (const RecRef& rr : wp->recs) {
        if (&rr + 3 < rend) { const RecRef& nx = (&rr)[3]; __builtin_prefetch(nx.p); __builtin_prefetch(nx.p + 64); __builtin_prefetch(nx.p + nx.len - 64); __builtin_prefetch(nx.p + nx.len - 128); }
        const int32_t ctg = cm(rr.tid, (int32_t)le32(rr.p + 4));
        if (ctg < 0) continue;
        s.cig_off[o] = co; s.seq_off[o] = so;
        nf += parse_record(dc, e, s, rr.p, rr.len, o, sample, names, flags);
        co += rr.n_cig; if (dc.want_seq) so += (rr.l_seq + 1) / 2;
        o++;
    }
    if (nf && n_filtered) n_filtered->fetch_add(nf, std::memory_order_relaxed);
    if (s.has_names) {
        // device-names mode: no host table.  One item per kept record of the piece (len 0: the key parse_record wrote is final) and the
        // bytes of the names to intern, packed into the piece's share of the block's trailer; the device table keys them behind the copy
        DiItem* it0 = s.items + wp->out_base;
        memset(it0, 0, wp->n_out * sizeof(DiItem));
        size_t at = wp->name_base; const size_t end = wp->name_base + wp->n_name;
        for (const InternTable::Item& it : names) {
            if (at + it.n > end) { flags->fetch_or(1); break; }            // (never: n_name counts every name with its NUL)
            memcpy(s.name_bytes + at, it.s, it.n);
            s.items[it.out - s.umi] = DiItem{(uint32_t)at, it.n};
            at += it.n;
        }
        return;
    }
    if (!names.empty()) { bool ovf = false; e->intern.intern_batch(names, &ovf); if (ovf) flags->fetch_or(2); }
}

// Stage 5 of a chunk's decode (bam.cpp decode_next_chunk), layout: where every piece's records go in the job's SoA block (prefix sums over the pieces), and the batches - runs of
// records on one contig, across piece boundaries.  Returns the number of records of the chunk (kept or not), < 0 on error.
int64_t layout_chunk(ChunkJob& j, std::vector<WalkPart>& pieces, const xck_ingest_opts* o, bool want_seq, int64_t records_before, std::string* err) {
    size_t n_out = 0, n_cig = 0, n_seq = 0, n_rec = 0, n_name = 0;
    for (WalkPart& wp : pieces) { wp.out_base = n_out; wp.cig_base = n_cig; wp.seq_base = n_seq; wp.name_base = n_name; n_out += wp.n_out; n_cig += wp.n_cig; n_seq += wp.n_seq; n_name += wp.n_name; n_rec += wp.recs.size(); }
    if (n_cig >= (size_t(1) << 32) || n_seq >= (size_t(1) << 32) || (j.qual && n_seq >= (size_t(1) << 31))) { *err = "chunk too large"; return XCK_E_IO; }
    HostSoA& s = j.soa;
    if (n_name >= (size_t(1) << 32)) { *err = "chunk too large"; return XCK_E_IO; }
    if (!soa_reserve(s, n_out + 1, n_cig + 1, want_seq ? n_seq + 1 : 1, n_out, n_name, j.names, j.qual && want_seq)) { *err = "out of host memory"; return XCK_E_NOMEM; }
    s.cig_off[n_out] = (uint32_t)n_cig; s.seq_off[n_out] = (uint32_t)n_seq;
    const uint64_t ord_hi = (uint64_t)(uint32_t)o->sample << ORD_REC_BITS;
    int32_t cur_c = -1; int64_t seg0 = 0, seg_r = 0, rec0 = 0;
    auto close_batch = [&](int64_t oi) { if (cur_c >= 0 && oi > seg0) j.batches.push_back({cur_c, seg0, oi, ord_hi | (uint64_t)(records_before + seg_r)}); };
    for (const WalkPart& wp : pieces) {
        int64_t oi = (int64_t)wp.out_base;
        for (size_t ri = 0; ri < wp.runs.size(); ri++) {
            const ContigRun& rn = wp.runs[ri];
            const uint32_t nxt = ri + 1 < wp.runs.size() ? wp.runs[ri + 1].first : (uint32_t)wp.recs.size();
            if (rn.contig != cur_c) { close_batch(oi); cur_c = rn.contig; seg0 = oi; seg_r = rec0 + rn.first; }
            if (rn.contig >= 0) oi += nxt - rn.first;
        }
        rec0 += (int64_t)wp.recs.size();
    }
    close_batch((int64_t)n_out);
    return (int64_t)n_rec;
}

}  // namespace xck
