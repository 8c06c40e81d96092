// Host-only check of the device parse path's host logic (csrc/parse_dev.h summaries_to_batches) against the decoder's own layout
// (csrc/bam_records.cpp run_part + layout_chunk), under AddressSanitizer / UBSan: random chunks of records are walked twice - by the
// decoder's walk tasks, and by walk_block below, a host restatement of k_walk (csrc/parse_dev.hip) that fills the per-block summaries the
// kernel writes - and the batch lists, ordinals, totals and per-batch sizes made of either must be the same.  No device, no HIP call:
// the program links csrc/bam_records.cpp, and engine_stubs.cpp for the block's allocation and its fence.
//   make -C tools/asan parse_layout_check && tools/asan/parse_layout_check
#include <cstdio>
#include "../../xcltk_amd/csrc/bam_decode.h"

// k_walk of one block, on the host: the same loop, the same summary
static void walk_block(const uint8_t* u, uint32_t out_off, uint32_t out_len, uint32_t first_skip, const DpContigMap& cm, bool want_seq, DpBlockSum* sum) {
    DpBlockSum s; memset(&s, 0, sizeof s); s.last_tid = -1;
    size_t o = (size_t)out_off + first_skip; const size_t end = (size_t)out_off + out_len;
    if (o > end) s.flags |= DP_F_STRADDLE;
    else {
        int32_t cur_c = INT32_MIN;
        while (o + 4 <= end) {
            const uint32_t bs = le32(u + o);
            if (bs < 32) { s.flags |= DP_F_SHORT; break; }
            if (o + 4 + (size_t)bs > end) break;
            const uint8_t* r = u + o + 4;
            const int32_t tid = (int32_t)le32(r), pos = (int32_t)le32(r + 4);
            const uint32_t l_name = r[8], n_cig = le16(r + 12), l_seq = le32(r + 16);
            if (32ull + l_name + (unsigned long long)n_cig * 4 + ((unsigned long long)l_seq + 1) / 2 + l_seq > (unsigned long long)bs) s.flags |= DP_F_OVERRUN;
            const int32_t ctg = dp_contig(cm, tid, pos);
            if (ctg != cur_c) {
                if (s.n_runs < (uint32_t)DP_MAX_RUNS) s.runs[s.n_runs] = DpRun{s.n_rec, ctg, s.n_out, s.n_cig, s.n_seq}; else s.flags |= DP_F_RUNS;
                s.n_runs++; cur_c = ctg;
            }
            if (ctg >= 0 && !(s.flags & DP_F_OVERRUN)) { s.n_out++; s.n_cig += n_cig; if (want_seq) s.n_seq += (l_seq + 1) / 2; }
            s.n_rec++; s.last_tid = tid; s.last_pos = pos;
            o += 4 + (size_t)bs;
        }
        if (o != end) s.flags |= DP_F_STRADDLE;
    }
    s.stop = (uint32_t)o;
    *sum = s;
}

static uint64_t g_rng = 0x243F6A8885A308D3ull;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }

int main() {
    const int n_refs = 6;
    long chunks = 0, batches = 0, flagged = 0;
    for (int round = 0; round < 1500; round++) {
        // ---- a chunk: blocks of whole records; tid mostly non-decreasing, with a stretch of frequent changes now and then ----
        const int nb = 1 + (int)rnd(40); const bool want_seq = rnd(2) != 0, jumpy = rnd(12) == 0;
        std::vector<uint8_t> u; std::vector<BlockRef> blocks; int32_t tid = 0;
        const uint32_t first_skip = rnd(3) == 0 ? 1 + rnd(40) : 0;
        for (int b = 0; b < nb; b++) {
            BlockRef br; memset(&br, 0, sizeof br); br.uoff = u.size();
            if (b == 0) u.insert(u.end(), first_skip, (uint8_t)0xEE);               // (header bytes before the first record)
            const int nr = rnd(6) == 0 ? (int)rnd(2) : 1 + (int)rnd(30);               // blocks with 0 and 1 records too
            for (int r = 0; r < nr; r++) {
                if (jumpy ? rnd(3) == 0 : rnd(40) == 0) tid = jumpy ? (int32_t)rnd(n_refs + 1) - 1 : std::min(tid + 1, n_refs);   // (-1 / n_refs: unmapped, out of range)
                const uint32_t l_name = 1 + rnd(20), n_cig = rnd(5), l_seq = rnd(7) == 0 ? 0 : rnd(120), aux = rnd(30);
                const uint32_t bs = 32 + l_name + n_cig * 4 + (l_seq + 1) / 2 + l_seq + aux;
                const size_t at = u.size(); u.resize(at + 4 + bs, (uint8_t)rnd(256));
                auto put32 = [&](size_t o, uint32_t v) { memcpy(u.data() + o, &v, 4); };
                put32(at, bs); put32(at + 4, (uint32_t)tid); put32(at + 8, rnd(1000000)); u[at + 12] = (uint8_t)l_name;
                const uint16_t nc = (uint16_t)n_cig; memcpy(u.data() + at + 16, &nc, 2); put32(at + 20, l_seq);
            }
            br.isize = (uint32_t)(u.size() - br.uoff); blocks.push_back(br);
        }
        u.resize(u.size() + 8192);                                                  // (run_part prefetches ahead; nothing is read there)
        std::vector<int32_t> t2c(n_refs), t_end(n_refs);
        for (int t = 0; t < n_refs; t++) { t2c[t] = rnd(4) == 0 ? -1 : (int32_t)rnd(5); t_end[t] = rnd(3) == 0 ? (int32_t)rnd(1000000) : 0; }
        ContigMap cm; cm.t2c = t2c.data(); cm.n_refs = n_refs; cm.t_end = rnd(2) ? t_end.data() : nullptr; cm.only_tid = rnd(4) == 0 ? (int32_t)rnd(n_refs) : -1;
        const DpContigMap dcm{cm.t2c, cm.t_end, cm.n_refs, cm.only_tid};
        // ---- the decoder's way: walk parts of a few blocks each, then layout_chunk ----
        Chunk c; c.blocks = blocks; c.ubase = u.data(); c.usize = u.size() - 8192;
        const size_t per = 1 + rnd(5), n_parts = (nb + per - 1) / per;
        c.parts.resize(n_parts);
        std::vector<int32_t> st((size_t)nb, 0); DecodeTimes tm; std::atomic<int64_t> ds[DS_N] = {};
        for (size_t pi = 0; pi < n_parts; pi++) {
            WalkPart& wp = c.parts[pi]; wp.i0 = pi * per; wp.i1 = std::min<size_t>(nb, wp.i0 + per);
            wp.u_begin = blocks[wp.i0].uoff; wp.u_end = blocks[wp.i1 - 1].uoff + blocks[wp.i1 - 1].isize; wp.spec_start = wp.u_begin + (pi == 0 ? first_skip : 0); wp.stop = wp.spec_start;
            run_part(&c, nullptr, false, &wp, &tm, cm, want_seq, st.data(), ds);
            if (wp.stop != wp.u_end) { fprintf(stderr, "round %d: the walk task did not reach its range's end\n", round); return 1; }
        }
        xck_ingest_opts o; memset(&o, 0, sizeof o); o.struct_size = sizeof o; o.sample = (int32_t)rnd(100);
        const int64_t before = (int64_t)rnd(1u << 30) * 1000;
        ChunkJob j; std::string err;
        const int64_t n_rec = layout_chunk(j, c.parts, &o, want_seq, before, &err);
        if (n_rec < 0) { fprintf(stderr, "round %d: layout_chunk: %s\n", round, err.c_str()); return 1; }
        // ---- the device's way: one summary per block, then summaries_to_batches ----
        std::vector<DpBlockSum> sums((size_t)nb);
        for (int b = 0; b < nb; b++) walk_block(u.data(), (uint32_t)blocks[b].uoff, blocks[b].isize, b == 0 ? first_skip : 0, dcm, want_seq, &sums[b]);
        DpChunkLayout lay;
        summaries_to_batches(sums.data(), (size_t)nb, before, (uint64_t)(uint32_t)o.sample << ORD_REC_BITS, &lay);
        chunks++;
        if (lay.flags) {                                                    // more runs in a block than a summary holds: the host path takes the chunk
            bool over = false; for (auto& s : sums) over = over || s.n_runs > (uint32_t)DP_MAX_RUNS;
            if (lay.flags != DP_F_RUNS || !over) { fprintf(stderr, "round %d: flags %u\n", round, lay.flags); return 1; }
            flagged++; soa_free(j.soa); continue;
        }
        const HostSoA& s = j.soa;
        bool ok = (int64_t)lay.n_rec == n_rec && lay.batches.size() == j.batches.size() && s.cig_off[lay.n_out] == lay.n_cig && s.seq_off[lay.n_out] == lay.n_seq;
        // (per-batch sizes: the kept records' CIGAR words / sequence bytes, summed from the walk parts' lists in output order)
        std::vector<uint32_t> cig_at{0}, seq_at{0};
        for (const WalkPart& wp : c.parts) for (const RecRef& rr : wp.recs) if (cm(rr.tid, (int32_t)le32(rr.p + 4)) >= 0) {
            cig_at.push_back(cig_at.back() + rr.n_cig); seq_at.push_back(seq_at.back() + (want_seq ? (rr.l_seq + 1) / 2 : 0)); }
        ok = ok && cig_at.size() == lay.n_out + 1;
        for (size_t i = 0; ok && i < lay.batches.size(); i++) {
            const DpBatch& d = lay.batches[i]; const PendingBatch& p = j.batches[i];
            ok = d.contig == p.contig && d.r0 == p.r0 && d.r1 == p.r1 && d.ordinal_base == p.ordinal_base &&
                 d.n_cig == cig_at[(size_t)d.r1] - cig_at[(size_t)d.r0] && d.n_seq == seq_at[(size_t)d.r1] - seq_at[(size_t)d.r0];
        }
        // (the chunk's last record: what drop_range_past_window looks at)
        const RecRef* last = nullptr;
        for (size_t pi = c.parts.size(); pi-- > 0 && !last;) if (!c.parts[pi].recs.empty()) last = &c.parts[pi].recs.back();
        ok = ok && lay.has_last == (last != nullptr) && (!last || (lay.last_tid == last->tid && lay.last_pos == (int32_t)le32(last->p + 4)));
        // (one layout: the host's columns sit where soa_layout says)
        const SoaLayout l = soa_layout(lay.n_out + 1, lay.n_cig + 1, want_seq ? lay.n_seq + 1 : 1);
        ok = ok && (uint8_t*)s.umi == s.base + l.o_umi && (uint8_t*)s.cigar == s.base + l.o_cig && s.seq == s.base + l.o_seq && s.used == l.total;
        if (!ok) { fprintf(stderr, "round %d: summaries_to_batches and layout_chunk disagree (%zu / %zu batches, %zu / %lld records)\n", round, lay.batches.size(), j.batches.size(), lay.n_rec, (long long)n_rec); return 1; }
        batches += (long)lay.batches.size();
        soa_free(j.soa);
    }
    printf("%ld chunks: %ld batches identical, %ld chunks flagged for the host path\n", chunks, batches, flagged);
    return flagged > 0 && batches > 1000 ? 0 : 1;
}
