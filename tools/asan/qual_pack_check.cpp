// Host-only check of what a base-quality floor (xck_config.min_baseq) adds to the decoder's host code (csrc/bam_records.cpp), under
// AddressSanitizer / UBSan: random chunks of records with sequences of 0 to 90 bases - odd and even, some without - are walked by the
// decoder's walk tasks, then laid out by layout_chunk and parsed by parse_part four times: with and without the quality region, with and
// without the name trailer of device-names mode.  Checked:
//   - every kept record's l_seq quality bytes, and the 0xff pad of an odd one, are where 2 * seq_off says, inside the region behind the
//     layout's total and in front of the trailer, no two records overlapping, nothing else of the region's used part left unwritten;
//   - the layout without qualities is the present one: SoaLayout's offsets and total, byte for byte the same columns as with them;
//   - the name trailer is intact when both are on: the same items and bytes, moved back by exactly the region's size.
// No device, no HIP call: the program links csrc/bam_records.cpp, and engine_stubs.cpp for the block's allocation and its fence.
//   make -C tools/asan qual_pack_check && tools/asan/qual_pack_check
#include <cstdio>
#include "../../xcltk_amd/csrc/bam_decode.h"

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }

struct Run { ChunkJob j; size_t n_out = 0, n_cig = 0, n_seq = 0; };

// layout + parse of the chunk's parts into r.j.soa, the block pre-filled with 0xA5 (whatever the tasks do not write shows)
static bool run(Run& r, xck_engine& e, std::vector<WalkPart>& parts, const ContigMap& cm, bool want_seq, bool names, bool qual, int round) {
    DecodeTimes tm;
    e.dec.use_umi = !names; e.dec.umi_tag[0] = 'U'; e.dec.umi_tag[1] = 'B';          // (no record carries the tag: without names the key is NONE and nothing is interned)
    xck_ingest_opts o; memset(&o, 0, sizeof o); o.struct_size = sizeof o;
    r.j.names = names; r.j.qual = qual; std::string err;
    if (layout_chunk(r.j, parts, &o, want_seq, 0, &err) < 0) { fprintf(stderr, "round %d: layout_chunk: %s\n", round, err.c_str()); return false; }
    HostSoA& s = r.j.soa;
    r.n_out = 0; for (const WalkPart& wp : parts) r.n_out += wp.n_out;
    r.n_cig = s.cig_off[r.n_out]; r.n_seq = s.seq_off[r.n_out];
    const uint32_t c_end = s.cig_off[r.n_out], s_end = s.seq_off[r.n_out];
    memset(s.base, 0xA5, s.used);
    s.cig_off[r.n_out] = c_end; s.seq_off[r.n_out] = s_end;
    std::atomic<int> flags{0};
    for (const WalkPart& wp : parts) if (wp.n_out) parse_part(&tm, &e, &s, 0, &wp, cm, &flags);
    if (flags.load() || e.intern.size() != 0) { fprintf(stderr, "round %d: parse flags %d, %llu names in the host table\n", round, flags.load(), (unsigned long long)e.intern.size()); return false; }
    return true;
}

int main() {
    const int n_refs = 4, umi_bits = 38;
    DecodeTimes tm;
    xck_engine e; e.dec.use_barcodes = false; e.dec.umi_bits = umi_bits;
    long chunks = 0, recs = 0, odd = 0, no_seq = 0, qbytes = 0;
    for (int round = 0; round < 400; round++) {
        const int nb = 1 + (int)rnd(30); const bool want_seq = rnd(8) != 0;
        e.dec.want_seq = want_seq;
        std::vector<uint8_t> u; std::vector<BlockRef> blocks; int32_t tid = 0;
        for (int bi = 0; bi < nb; bi++) {
            BlockRef br; memset(&br, 0, sizeof br); br.uoff = u.size();
            const int nr = rnd(6) == 0 ? (int)rnd(2) : 1 + (int)rnd(25);
            for (int r = 0; r < nr; r++) {
                if (rnd(30) == 0) tid = (int32_t)rnd(n_refs + 1) - 1;
                const uint32_t qlen = rnd(4) == 0 ? 1 + rnd(18) : 20 + rnd(30);
                const uint32_t l_name = qlen + 1, n_cig = rnd(4), l_seq = rnd(6) == 0 ? rnd(3) : rnd(91), aux = rnd(20);
                const uint32_t bs = 32 + l_name + n_cig * 4 + (l_seq + 1) / 2 + l_seq + aux;
                const size_t at = u.size(); u.resize(at + 4 + bs, (uint8_t)0);
                auto put32 = [&](size_t o, uint32_t v) { memcpy(u.data() + o, &v, 4); };
                put32(at, bs); put32(at + 4, (uint32_t)tid); put32(at + 8, rnd(1000000)); u[at + 12] = (uint8_t)l_name;
                const uint16_t nc = (uint16_t)n_cig; memcpy(u.data() + at + 16, &nc, 2); put32(at + 20, l_seq);
                for (uint32_t k = 0; k < qlen; k++) u[at + 36 + k] = (uint8_t)(rnd(3) ? "ACGT"[rnd(4)] : 33 + rnd(90));   // (mostly too long for a direct code: packed into the trailer)
                const size_t sq = at + 36 + l_name + (size_t)n_cig * 4;
                for (uint32_t k = 0; k < (l_seq + 1) / 2; k++) u[sq + k] = (uint8_t)rnd(256);
                const bool star = rnd(10) == 0;                                         // `*`: every byte 0xff
                for (uint32_t k = 0; k < l_seq; k++) u[sq + (l_seq + 1) / 2 + k] = star ? (uint8_t)0xff : (uint8_t)rnd(94);
                for (uint32_t k = 0; k < aux; k++) u[at + 4 + bs - aux + k] = 0;         // (no aux tag parses out of zeros: the scan stops at once)
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
        Run R[4];                                                                   // [names * 2 + qual]
        for (int k = 0; k < 4; k++) if (!run(R[k], e, c.parts, cm, want_seq, (k & 2) != 0, (k & 1) != 0, round)) return 1;
        const size_t n_out = R[0].n_out, n_cig = R[0].n_cig, n_seq = want_seq ? R[0].n_seq : 0;
        const SoaLayout l = soa_layout(n_out + 1, n_cig + 1, want_seq ? n_seq + 1 : 1);
        const size_t qb = want_seq ? soa_qual_bytes(n_seq + 1) : 0;                  // (a handle without sequences keeps no qualities)
        for (int k = 0; k < 4; k++) {
            const HostSoA& s = R[k].j.soa; const bool names = (k & 2) != 0, qual = (k & 1) != 0 && want_seq;
            // ---- the columns are where the layout puts them, whatever follows them ----
            if ((uint8_t*)s.umi != s.base + l.o_umi || (uint8_t*)s.pos != s.base + l.o_pos || (uint8_t*)s.cell != s.base + l.o_cell || (uint8_t*)s.cig_off != s.base + l.o_cgo ||
                (uint8_t*)s.seq_off != s.base + l.o_sqo || (uint8_t*)s.cigar != s.base + l.o_cig || (uint8_t*)s.flag != s.base + l.o_flag || s.mapq != s.base + l.o_mapq || s.seq != s.base + l.o_seq) {
                fprintf(stderr, "round %d run %d: a column is not where soa_layout puts it\n", round, k); return 1; }
            if (memcmp(s.base, R[0].j.soa.base, l.total) != 0 && !names) { fprintf(stderr, "round %d run %d: the columns differ from the run without qualities\n", round, k); return 1; }
            if (names && memcmp(s.base, R[2].j.soa.base, l.total) != 0) { fprintf(stderr, "round %d run %d: the columns differ from the names run without qualities\n", round, k); return 1; }
            const size_t q_off = l.total, t_off = l.total + (qual ? qb : 0);
            if ((s.qual != nullptr) != qual || (qual && s.qual != s.base + q_off)) { fprintf(stderr, "round %d run %d: the quality region is not behind the layout's total\n", round, k); return 1; }
            if (names) {
                if (!s.has_names || s.nt.items_off != t_off || s.nt.bytes_off + s.nt.n_bytes > s.used) { fprintf(stderr, "round %d run %d: the trailer is not behind the quality region\n", round, k); return 1; }
            } else if (s.used != t_off) { fprintf(stderr, "round %d run %d: the block holds %zu bytes, expected %zu\n", round, k, s.used, t_off); return 1; }
        }
        if (R[0].j.soa.used != l.total) { fprintf(stderr, "round %d: the layout without qualities is not the present one\n", round); return 1; }
        // ---- the trailer with qualities = the trailer without them, moved back by the region ----
        { const HostSoA &a = R[2].j.soa, &b = R[3].j.soa;
          const size_t shift = want_seq ? qb : 0;
          if (b.nt.items_off != a.nt.items_off + shift || b.nt.bytes_off != a.nt.bytes_off + shift || b.nt.n_bytes != a.nt.n_bytes || b.nt.n_out != a.nt.n_out ||
              memcmp(a.base + a.nt.items_off, b.base + b.nt.items_off, a.nt.n_out * sizeof(DiItem)) != 0 || b.used != a.used + shift) {
              fprintf(stderr, "round %d: the name trailer changed with the quality region\n", round); return 1; }
          for (size_t o = 0; o < a.nt.n_out; o++) { const DiItem it = a.items[o];
              if (it.len && memcmp(a.name_bytes + it.off, b.name_bytes + it.off, it.len) != 0) { fprintf(stderr, "round %d: a packed name changed with the quality region\n", round); return 1; } } }
        // ---- every kept record's qualities, in output order, in both runs that keep them ----
        if (want_seq) for (int k = 1; k < 4; k += 2) {
            const HostSoA& s = R[k].j.soa;
            std::vector<uint8_t> used(2 * n_seq, 0); size_t oi = 0;
            for (const WalkPart& wp : c.parts) for (const RecRef& rr : wp.recs) {
                if (cm(rr.tid, (int32_t)le32(rr.p + 4)) < 0) continue;
                const uint32_t l_seq = rr.l_seq; const size_t at = 2 * (size_t)s.seq_off[oi], room = 2 * (size_t)(s.seq_off[oi + 1] - s.seq_off[oi]);
                if (room != l_seq + (l_seq & 1) || at + room > 2 * n_seq) { fprintf(stderr, "round %d: record %zu: %u bases in %zu quality bytes at %zu of %zu\n", round, oi, l_seq, room, at, 2 * n_seq); return 1; }
                const uint8_t* src = rr.p + 32 + rr.p[8] + (size_t)rr.n_cig * 4 + (l_seq + 1) / 2;
                if (memcmp(s.qual + at, src, l_seq) != 0) { fprintf(stderr, "round %d run %d: record %zu: its quality bytes are not at 2 * seq_off\n", round, k, oi); return 1; }
                if ((l_seq & 1) && s.qual[at + l_seq] != 0xff) { fprintf(stderr, "round %d run %d: record %zu: the pad byte is %u\n", round, k, oi, s.qual[at + l_seq]); return 1; }
                for (size_t b = 0; b < room; b++) { if (used[at + b]) { fprintf(stderr, "round %d: two records' qualities overlap\n", round); return 1; } used[at + b] = 1; }
                if (k == 1) { recs++; odd += l_seq & 1; no_seq += l_seq == 0; qbytes += l_seq; }
                oi++;
            }
            if (oi != n_out) { fprintf(stderr, "round %d: %zu records, %zu slots\n", round, oi, n_out); return 1; }
            for (size_t b = 0; b < 2 * n_seq; b++) if (!used[b]) { fprintf(stderr, "round %d: byte %zu of the quality region belongs to no record\n", round, b); return 1; }
        }
        chunks++;
        for (int k = 0; k < 4; k++) soa_free(R[k].j.soa);
    }
    printf("%ld chunks: %ld records, %ld of odd length, %ld without a sequence, %ld quality bytes: all where 2 * seq_off says, the layout without them unchanged, the name trailer intact\n",
           chunks, recs, odd, no_seq, qbytes);
    return recs > 10000 && odd > 1000 && no_seq > 100 ? 0 : 1;
}
