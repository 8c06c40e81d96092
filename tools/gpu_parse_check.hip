// xck_gpu_parse_check FILE.bam BARCODES.txt - the device's record walk and parse (csrc/parse_dev.hip) against the host's parse_part
// (csrc/bam_records.cpp) on the same bytes: the file's BGZF blocks go through k_inflate + k_walk + k_scan + k_parse in chunks of
// PARSE_CHUNK_BLOCKS (128) blocks, and every column of every kept record must equal what the host decoder writes for the chunk.
// A chunk the device flags (contig runs beyond the list, a UMI to intern, ...) is counted, and must be one the host would not have
// parsed with direct keys only.  Prints "N chunks, R records compared: D differences, F chunks flagged"; exit status 0 iff D == 0.
// PARSE_QUAL=1 (with sequence columns): both parsers also fill the quality region of a handle with a base-quality floor, and the regions -
// pad bytes included - are compared like a column; the line then ends in ", Q quality bytes compared".
// Environment: PARSE_SEQ=0 (no sequence columns), PARSE_DROP=k (every k-th reference is not wanted), PARSE_TEND=p (position windows end at p).
// The program links the decoder (bam.o, bam_records.o) and the device decoder; the engine is not part of it (tools/asan/engine_stubs.cpp).
#include "../xcltk_amd/csrc/bam_decode.h"
#include <hip/hip_runtime.h>
#include <cstdio>
#include <fstream>

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s FILE.bam BARCODES.txt\n", argv[0]); return 2; }
    const bool want_seq = !(getenv("PARSE_SEQ") && atoi(getenv("PARSE_SEQ")) == 0);
    const bool want_qual = want_seq && getenv("PARSE_QUAL") && atoi(getenv("PARSE_QUAL")) != 0;
    const int drop = getenv("PARSE_DROP") ? atoi(getenv("PARSE_DROP")) : 0, tend = getenv("PARSE_TEND") ? atoi(getenv("PARSE_TEND")) : 0;
    const size_t per = getenv("PARSE_CHUNK_BLOCKS") ? (size_t)atoi(getenv("PARSE_CHUNK_BLOCKS")) : 128;
    xck_bam* b = nullptr; char err[256] = {0};
    if (xck_bam_open(argv[1], 1, &b, err, sizeof err) != 0) { fprintf(stderr, "%s\n", err); return 2; }
    const int n_refs = (int)b->ref_names.size();
    xck_engine e;
    { std::vector<std::string> bcs; std::ifstream f(argv[2]); std::string s; while (f >> s) bcs.push_back(s);
      std::vector<const char*> p; for (auto& x : bcs) p.push_back(x.c_str());
      e.dec.use_barcodes = !p.empty(); if (!p.empty()) e.dec.build_barcodes(p.data(), (int)p.size()); }
    e.dec.use_umi = true; e.dec.cell_tag[0] = 'C'; e.dec.cell_tag[1] = 'B'; e.dec.umi_tag[0] = 'U'; e.dec.umi_tag[1] = 'B'; e.dec.umi_bits = 38; e.dec.want_seq = want_seq;
    std::vector<int32_t> t2c((size_t)std::max(n_refs, 1)), t_end((size_t)std::max(n_refs, 1), tend);
    for (int t = 0; t < n_refs; t++) t2c[t] = drop > 0 && t % drop == drop - 1 ? -1 : t;
    ContigMap cm; cm.t2c = t2c.data(); cm.n_refs = n_refs; cm.t_end = tend > 0 ? t_end.data() : nullptr;
    // ---- the file's blocks from the first record on ----
    std::vector<BlockRef> blocks; { uint64_t coff = b->next_coff; BlockRef br; std::string es; while (bgzf_peek(b->map, b->fsize, coff, &br, &es)) { blocks.push_back(br); coff += br.clen; } }
    GpuInflateSlot* gs = gpu_inflate_slot_create(0, 32, false);
    if (!gs) { fprintf(stderr, "no device\n"); return 2; }
    gs->parse = true;
    void* d_cm = dev_parse_upload(0, cm.t2c, (size_t)n_refs * 4, cm.t_end, cm.t_end ? (size_t)n_refs * 4 : 0);
    void* d_bc = e.dec.bc_slots.empty() ? nullptr : dev_parse_upload(0, e.dec.bc_slots.data(), e.dec.bc_slots.size() * sizeof(DecodeCfg::BcSlot), nullptr, 0);
    hipStream_t stream; if (hipStreamCreate(&stream) != hipSuccess) return 2;
    long n_chunks = 0, n_flagged = 0, n_bad_flag = 0, n_cmp = 0, n_diff = 0, n_qual = 0; uint32_t all_flags = 0;
    for (size_t i0 = 0; i0 < blocks.size(); i0 += per) {
        const size_t nb = std::min(per, blocks.size() - i0); const uint32_t skip = i0 == 0 ? b->first_skip : 0;
        size_t tin = 0, usz = 0;
        for (size_t i = 0; i < nb; i++) { tin += ((size_t)blocks[i0 + i].data_len + 3) & ~size_t(3); usz += blocks[i0 + i].isize; }
        if (!gpu_inflate_slot_reserve(gs, tin + 8, usz + 8, nb)) { fprintf(stderr, "no device memory\n"); return 2; }
        std::vector<uint8_t> u(usz + 64); std::vector<size_t> uoff(nb + 1, 0);
        { size_t at = 0, uo = 0;
          for (size_t i = 0; i < nb; i++) { const BlockRef& br = blocks[i0 + i];
              gs->h_bl[i] = DevBlock{(uint32_t)at, br.data_len, (uint32_t)uo, br.isize, 0u};
              memcpy(gs->h_in + at, b->map + br.coff + br.data_off, br.data_len); at += ((size_t)br.data_len + 3) & ~size_t(3);
              std::string es; if (!bgzf_inflate(b->map, br, u.data() + uo, false, &es)) { fprintf(stderr, "host inflate: %s\n", es.c_str()); return 2; }
              uoff[i] = uo; uo += br.isize; }
          uoff[nb] = usz; }
        const DpWalk dw{skip, DpContigMap{(const int32_t*)d_cm, cm.t_end ? (const int32_t*)d_cm + n_refs : nullptr, n_refs, -1}, want_seq};
        if (gpu_inflate_slot_launch(gs, tin, usz, nb, false, &dw) != 0 || gpu_inflate_slot_wait(gs) != 0) { fprintf(stderr, "device launch failed\n"); return 2; }
        n_chunks++;
        // ---- the host's chunk: every block walked from its first byte, the kept records parsed into one SoA block ----
        HostSoA s; WalkPart wp; size_t n_out = 0, n_cig = 0, n_seq = 0; bool aligned = true;
        for (size_t i = 0; i < nb && aligned; i++) {
            size_t o = uoff[i] + (i == 0 ? skip : 0); const size_t end = uoff[i + 1];
            while (o + 4 <= end) { const uint32_t bs = le32(u.data() + o); if (bs < 32 || o + 4 + (size_t)bs > end) break;
                const uint8_t* r = u.data() + o + 4;
                if (cm((int32_t)le32(r), (int32_t)le32(r + 4)) >= 0) { wp.recs.push_back(RecRef{r, bs, (int32_t)le32(r), le32(r + 16), le16(r + 12)}); n_out++; n_cig += le16(r + 12); if (want_seq) n_seq += (le32(r + 16) + 1) / 2; }
                o += 4 + (size_t)bs; }
            aligned = o == end;
        }
        DpChunkLayout lay; summaries_to_batches(gs->h_sum, nb, 0, 0, &lay);
        all_flags |= gs->h_head->walk_flags;
        std::atomic<int> hflags{0}; DecodeTimes tm; e.intern.clear();
        if (aligned && n_cig < (1u << 30) && n_seq < (1u << 30)) {
            if (!soa_reserve(s, n_out + 1, n_cig + 1, want_seq ? n_seq + 1 : 1, 0, 0, false, want_qual)) return 2;
            memset(s.base, 0, s.used);
            wp.n_out = n_out; wp.n_cig = n_cig; wp.n_seq = n_seq;                    // (one piece, at the block's start: what layout_chunk makes of a chunk of one part)
            parse_part(&tm, &e, &s, 0, &wp, cm, &hflags);
            s.cig_off[n_out] = (uint32_t)n_cig; s.seq_off[n_out] = (uint32_t)n_seq;
        }
        const bool host_direct = aligned && hflags.load() == 0 && e.intern.size() == 0;     // nothing the host interned, nothing it reports
        if (lay.flags || gs->h_head->walk_flags) {
            n_flagged++;
            if (host_direct && !(lay.flags & DP_F_RUNS)) { n_bad_flag++; fprintf(stderr, "chunk at block %zu: flagged %u by the walk for no reason the host sees\n", i0, lay.flags); }
            soa_free(s); continue;
        }
        if (!aligned || lay.n_out != n_out || lay.n_cig != n_cig || lay.n_seq != n_seq) { n_diff++; fprintf(stderr, "chunk at block %zu: counts differ (%zu/%zu records)\n", i0, lay.n_out, n_out); soa_free(s); continue; }
        uint8_t* d_soa = nullptr; if (hipMalloc((void**)&d_soa, s.used) != hipSuccess || hipMemset(d_soa, 0, s.used) != hipSuccess) return 2;
        DpParseCfg pc; memset(&pc, 0, sizeof pc);
        pc.bc = (const DpBcSlot*)d_bc; pc.bc_mask = e.dec.bc_mask; pc.use_barcodes = e.dec.use_barcodes; pc.want_seq = want_seq; pc.umi_bits = e.dec.umi_bits; pc.sample = 0; pc.want_qual = want_qual;
        memcpy(pc.cell_tag, e.dec.cell_tag, 2); memcpy(pc.umi_tag, e.dec.umi_tag, 2);
        if (dev_parse_launch(stream, gs, nb, lay.max_rec, pc, d_soa, n_out, n_cig, n_seq) != 0 || hipStreamSynchronize(stream) != hipSuccess) { fprintf(stderr, "parse launch failed\n"); return 2; }
        all_flags |= gs->h_head->parse_flags;
        if (gs->h_head->parse_flags) {
            n_flagged++;
            if (host_direct) { n_bad_flag++; fprintf(stderr, "chunk at block %zu: flagged %u by the parse for no reason the host sees\n", i0, gs->h_head->parse_flags); }
        } else if (!host_direct) { n_diff++; fprintf(stderr, "chunk at block %zu: the host interned or reported something, the device flagged nothing\n", i0); }
        else {
            std::vector<uint8_t> got(s.used); if (hipMemcpy(got.data(), d_soa, s.used, hipMemcpyDeviceToHost) != hipSuccess) return 2;
            const SoaLayout l = soa_layout(n_out + 1, n_cig + 1, want_seq ? n_seq + 1 : 1);
            struct { const char* name; size_t off, bytes; } col[10] = { {"umi", l.o_umi, n_out * 8}, {"pos", l.o_pos, n_out * 4}, {"cell", l.o_cell, n_out * 4}, {"cig_off", l.o_cgo, (n_out + 1) * 4},
                {"seq_off", l.o_sqo, (n_out + 1) * 4}, {"cigar", l.o_cig, n_cig * 4}, {"flag", l.o_flag, n_out * 2}, {"mapq", l.o_mapq, n_out}, {"seq", l.o_seq, want_seq ? n_seq : 0},
                {"qual", l.total, want_qual ? 2 * n_seq : 0} };                              // (behind the layout's total: two bytes per sequence byte, the pads among them)
            for (auto& c : col) if (memcmp(got.data() + c.off, s.base + c.off, c.bytes) != 0) {
                size_t k = 0; while (got[c.off + k] == s.base[c.off + k]) k++;
                n_diff++; fprintf(stderr, "chunk at block %zu: column %s differs at byte %zu of %zu\n", i0, c.name, k, c.bytes);
            }
            n_cmp += (long)n_out; if (want_qual) n_qual += (long)(2 * n_seq);
        }
        (void)hipFree(d_soa); soa_free(s);
    }
    printf("%ld chunks, %ld records compared: %ld differences, %ld chunks flagged (flags %u), %ld flagged without cause", n_chunks, n_cmp, n_diff, n_flagged, all_flags, n_bad_flag);
    if (want_qual) printf(", %ld quality bytes compared", n_qual);
    printf("\n");
    dev_parse_free(0, d_cm); dev_parse_free(0, d_bc); gpu_inflate_slot_destroy(gs); xck_bam_close(b);
    return n_diff == 0 && n_bad_flag == 0 ? 0 : 1;
}
