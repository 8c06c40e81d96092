// Host-only check of what device-names mode (XCK_GPU_NAMES) adds to the decoder's host code (csrc/bam_records.cpp), under AddressSanitizer /
// UBSan: random chunks of records with names of 0 to 254 bytes - some directly codable - are walked by the decoder's walk tasks, laid
// out by layout_chunk with the name trailer behind the SoA columns, and parsed by parse_part, which packs the names instead of interning
// them.  For every kept record the trailer must hold what the device table needs: an item of length 0 exactly where parse_record's key
// is final (an empty or 2-bit codable name), otherwise the name's own bytes inside the block, no two names overlapping; the host table
// stays empty.  No device, no HIP call: the program links csrc/bam_records.cpp, and engine_stubs.cpp for the block's allocation and its fence.
//   make -C tools/asan names_pack_check && tools/asan/names_pack_check
#include <cstdio>
#include "../../xcltk_amd/csrc/bam_decode.h"

static uint64_t g_rng = 0x13198A2E03707344ull;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }

int main() {
    const int n_refs = 4, umi_bits = 38;
    DecodeTimes tm;
    xck_engine e; e.dec.use_umi = false; e.dec.use_barcodes = false; e.dec.umi_bits = umi_bits;
    long chunks = 0, names = 0, direct = 0, empty = 0;
    for (int round = 0; round < 600; round++) {
        const int nb = 1 + (int)rnd(30); const bool want_seq = rnd(2) != 0;
        e.dec.want_seq = want_seq;
        std::vector<uint8_t> u; std::vector<BlockRef> blocks; int32_t tid = 0;
        for (int bi = 0; bi < nb; bi++) {
            BlockRef br; memset(&br, 0, sizeof br); br.uoff = u.size();
            const int nr = rnd(6) == 0 ? (int)rnd(2) : 1 + (int)rnd(25);
            for (int r = 0; r < nr; r++) {
                if (rnd(30) == 0) tid = (int32_t)rnd(n_refs + 1) - 1;
                const uint32_t kind = rnd(8);
                const uint32_t qlen = kind == 0 ? 0 : kind == 1 ? 254 : kind == 2 ? 1 + rnd(18) : 1 + rnd(40);
                const uint32_t l_name = qlen + 1, n_cig = rnd(4), l_seq = rnd(90), aux = rnd(20);
                const uint32_t bs = 32 + l_name + n_cig * 4 + (l_seq + 1) / 2 + l_seq + aux;
                const size_t at = u.size(); u.resize(at + 4 + bs, (uint8_t)0);
                auto put32 = [&](size_t o, uint32_t v) { memcpy(u.data() + o, &v, 4); };
                put32(at, bs); put32(at + 4, (uint32_t)tid); put32(at + 8, rnd(1000000)); u[at + 12] = (uint8_t)l_name;
                const uint16_t nc = (uint16_t)n_cig; memcpy(u.data() + at + 16, &nc, 2); put32(at + 20, l_seq);
                for (uint32_t k = 0; k < qlen; k++) u[at + 36 + k] = kind == 2 || kind == 3 ? (uint8_t)"ACGT"[rnd(4)] : (uint8_t)(33 + rnd(90));   // (kind 3: ACGT, mostly too long for a code)
            }
            br.isize = (uint32_t)(u.size() - br.uoff); blocks.push_back(br);
        }
        u.resize(u.size() + 8192);                                                  // (run_part prefetches ahead; nothing is read there)
        std::vector<int32_t> t2c(n_refs); for (int t = 0; t < n_refs; t++) t2c[t] = rnd(5) == 0 ? -1 : t;
        ContigMap cm; cm.t2c = t2c.data(); cm.n_refs = n_refs;
        Chunk c; c.blocks = blocks; c.ubase = u.data(); c.usize = u.size() - 8192;
        const size_t per = 1 + rnd(4), n_parts = ((size_t)nb + per - 1) / per;
        c.parts.resize(n_parts);
        std::vector<int32_t> st((size_t)nb, 0); std::atomic<int64_t> ds[DS_N] = {};
        for (size_t pi = 0; pi < n_parts; pi++) {
            WalkPart& wp = c.parts[pi]; wp.i0 = pi * per; wp.i1 = std::min<size_t>((size_t)nb, wp.i0 + per);
            wp.u_begin = blocks[wp.i0].uoff; wp.u_end = blocks[wp.i1 - 1].uoff + blocks[wp.i1 - 1].isize; wp.spec_start = wp.u_begin; wp.stop = wp.spec_start;
            run_part(&c, nullptr, false, &wp, &tm, cm, want_seq, st.data(), ds);
            if (wp.stop != wp.u_end) { fprintf(stderr, "round %d: the walk task did not reach its range's end\n", round); return 1; }
        }
        xck_ingest_opts o; memset(&o, 0, sizeof o); o.struct_size = sizeof o;
        ChunkJob j; j.names = true; std::string err;
        if (layout_chunk(j, c.parts, &o, want_seq, 0, &err) < 0) { fprintf(stderr, "round %d: layout_chunk: %s\n", round, err.c_str()); return 1; }
        HostSoA& s = j.soa;
        size_t n_out = 0; for (const WalkPart& wp : c.parts) n_out += wp.n_out;
        const SoaLayout l = soa_layout(n_out + 1, s.cig_off[n_out] + 1, want_seq ? s.seq_off[n_out] + 1 : 1);
        if (!s.has_names || s.nt.items_off != l.total || s.nt.n_out != n_out || s.nt.bytes_off < s.nt.items_off + n_out * sizeof(DiItem) || s.nt.bytes_off + s.nt.n_bytes > s.used) {
            fprintf(stderr, "round %d: the trailer does not lie behind the columns\n", round); return 1; }
        memset(s.base + s.nt.items_off, 0xA5, s.used - s.nt.items_off);             // (whatever the tasks do not write shows)
        std::atomic<int> flags{0};
        for (const WalkPart& wp : c.parts) if (wp.n_out) parse_part(&tm, &e, &s, 0, &wp, cm, &flags);
        if (flags.load() || e.intern.size() != 0) { fprintf(stderr, "round %d: parse flags %d, %llu names in the host table\n", round, flags.load(), (unsigned long long)e.intern.size()); return 1; }
        // ---- every kept record, in output order ----
        std::vector<uint8_t> used(s.nt.n_bytes, 0); size_t oi = 0;
        for (const WalkPart& wp : c.parts) for (const RecRef& rr : wp.recs) {
            if (cm(rr.tid, (int32_t)le32(rr.p + 4)) < 0) continue;
            const uint32_t qlen = rr.p[8] ? rr.p[8] - 1u : 0u; const char* q = (const char*)rr.p + 32;
            uint64_t dkey = 0; const bool is_direct = encode_key_direct(q, qlen, umi_bits, &dkey);
            const DiItem it = s.items[oi];
            if (is_direct) { if (it.len != 0 || s.umi[oi] != dkey) { fprintf(stderr, "round %d: record %zu is directly codable, item length %u\n", round, oi, it.len); return 1; } (qlen ? direct : empty)++; }
            else {
                if (it.len != qlen || (size_t)it.off + it.len > s.nt.n_bytes || memcmp(s.name_bytes + it.off, q, qlen) != 0 || s.umi[oi] != XCK_UMI_NONE) {
                    fprintf(stderr, "round %d: record %zu: the packed name is not the record's (%u / %u bytes at %u of %zu)\n", round, oi, it.len, qlen, it.off, s.nt.n_bytes); return 1; }
                for (uint32_t k = 0; k < it.len; k++) { if (used[it.off + k]) { fprintf(stderr, "round %d: two names overlap\n", round); return 1; } used[it.off + k] = 1; }
                names++;
            }
            oi++;
        }
        if (oi != n_out) { fprintf(stderr, "round %d: %zu records, %zu slots\n", round, oi, n_out); return 1; }
        chunks++;
        soa_free(j.soa);
    }
    printf("%ld chunks: %ld names packed, %ld directly codable, %ld empty: all as the device table needs them\n", chunks, names, direct, empty);
    return names > 10000 && direct > 100 && empty > 100 ? 0 : 1;
}
