// parse_dev.h - record walk and parse on the device for GPU-inflated chunks (csrc/parse_dev.hip): what k_join reads of a record is
// in HBM when k_inflate ends, so the walk (one lane per BGZF block, behind k_inflate on the slot's stream), a scan of the per-block
// counts and the parse (launched by the engine's push path, straight into its staging slot) replace the chunk's trip to the host and
// back.  The host sees one small summary per block and turns the summaries into the chunk's batches (summaries_to_batches, no HIP).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define XCK_HD __host__ __device__
#else
#define XCK_HD
#endif

namespace xck {

// The SoA block of one decoded chunk: nine columns carved out of one block, every column 256-byte aligned.  One layout for the host
// decoder (bam_records.cpp soa_reserve) and for the parse kernel, which writes the same block in the engine's staging slot.
struct SoaLayout { size_t o_umi, o_pos, o_cell, o_cgo, o_sqo, o_cig, o_flag, o_mapq, o_seq, total; };
XCK_HD inline SoaLayout soa_layout(size_t n_reads, size_t n_cig, size_t n_seq) {
    auto up = [](size_t x) { return (x + 255) & ~size_t(255); };
    SoaLayout l;
    l.o_umi = 0; l.o_pos = l.o_umi + up(n_reads * 8); l.o_cell = l.o_pos + up(n_reads * 4); l.o_cgo = l.o_cell + up(n_reads * 4);
    l.o_sqo = l.o_cgo + up((n_reads + 1) * 4); l.o_cig = l.o_sqo + up((n_reads + 1) * 4); l.o_flag = l.o_cig + up(n_cig * 4);
    l.o_mapq = l.o_flag + up(n_reads * 2); l.o_seq = l.o_mapq + up(n_reads); l.total = l.o_seq + up(n_seq);
    return l;
}

// The quality region of a chunk whose handle has a base-quality floor (xck_config.min_baseq): two bytes per sequence byte behind the
// layout's total - the quality of query offset qi of the read at seq offset s0 at 2 * s0 + qi, the pad byte of an odd read 0xff.  The
// layout itself does not know it: without the floor a block is what it always was.
XCK_HD inline size_t soa_qual_bytes(size_t n_seq) { return (2 * n_seq + 255) & ~size_t(255); }

// chunk / block flags.  Any of them sends the chunk down the host path, which reports what there is to report.
constexpr uint32_t DP_F_SHORT = 1;        // a record with block_size < 32
constexpr uint32_t DP_F_STRADDLE = 2;     // the walk of a block did not end at the block's end (a record straddles blocks)
constexpr uint32_t DP_F_STATUS = 4;       // the block's inflate status is non-zero
constexpr uint32_t DP_F_RUNS = 8;         // more contig runs in a block than DpBlockSum holds
constexpr uint32_t DP_F_OVERRUN = 16;     // a record's fields overrun it
constexpr uint32_t DP_F_UMI = 32;         // a UMI that is not 2-bit codable (non-ACGT, too long, numeric type): the host interns it
constexpr uint32_t DP_DROPPED = 0xffffffffu;

constexpr int DP_MAX_RUNS = 4;
// records [first, next run's first) of the block are on `contig` (-1: not wanted); *_at: kept records, CIGAR words and sequence bytes
// of the block before the run
struct DpRun { uint32_t first; int32_t contig; uint32_t out_at, cig_at, seq_at; };
struct DpBlockSum {                       // one per BGZF block, in mapped host memory
    uint32_t n_rec, n_out, n_cig, n_seq;  // records, kept records, their CIGAR words and sequence bytes
    uint32_t stop;                        // where the walk stopped (byte offset in the chunk)
    uint32_t flags, n_runs;               // n_runs counts on past DP_MAX_RUNS (DP_F_RUNS is then set)
    int32_t last_tid, last_pos;           // of the block's last record
    DpRun runs[DP_MAX_RUNS];
    uint32_t pad[3];
};
static_assert(sizeof(DpBlockSum) == 128, "one summary is two cache lines");
struct DpRec { uint32_t off, slot, cig, seq; };     // a record: byte offset of its body in the chunk; output slot in the block (DP_DROPPED: none);
                                                    // CIGAR words / sequence bytes of the block's kept records before it
struct DpCnt { uint32_t n_rec, n_out, n_cig, n_seq, flags, rec_at, pad[2]; };   // per block, device memory: the walk's counts; rec_at: its first DpRec
struct DpBase { uint32_t out, cig, seq, pad; };     // per block, device memory: the scan's bases
struct DpHead { uint32_t walk_flags, parse_flags, n_rec, n_out, n_cig, n_seq, n_filtered, pad; };   // per chunk, mapped host memory; n_filtered: records the parse gave XCK_CELL_FILTERED (written by k_filtered_out behind the parse; zero with the tag filter off)
static_assert(sizeof(DpHead) == 32, "the head record keeps its size");
// most records n inflated bytes can hold (a record is at least 36 bytes): block b's list starts at out_off / 36, and the lists of
// neighbouring blocks cannot meet
XCK_HD inline size_t dp_rec_capacity(size_t out_bytes) { return out_bytes / 36 + 1; }

// what the walk applies per record (bam_decode.h ContigMap::operator())
struct DpContigMap { const int32_t* t2c; const int32_t* t_end; int32_t n_refs, only_tid; };
XCK_HD inline int32_t dp_contig(const DpContigMap& cm, int32_t tid, int32_t pos) {
    if (tid < 0 || tid >= cm.n_refs || !cm.t2c) return -1;
    if (cm.only_tid >= 0 && tid != cm.only_tid) return -1;
    if (cm.t_end && cm.t_end[tid] > 0 && pos >= cm.t_end[tid]) return -1;
    return cm.t2c[tid];
}

// ---- host: summaries -> the chunk's batches (what layout_chunk makes of the walk parts' lists) --------------------------------------
struct DpBatch { int32_t contig; int64_t r0, r1; uint64_t ordinal_base; uint32_t n_cig, n_seq; };
struct DpChunkLayout {
    std::vector<DpBatch> batches;
    size_t n_rec = 0, n_out = 0, n_cig = 0, n_seq = 0, max_rec = 0;      // totals; most records of one block
    uint32_t flags = 0;                   // OR of the blocks' flags: non-zero = the chunk takes the host path
    bool has_last = false; int32_t last_tid = -1, last_pos = 0;   // the chunk's last record (drop_range_past_window)
};
// runs of kept records on one contig, across block boundaries; ordinal_base = ord_hi | (records_before + index of the batch's first
// record in the chunk).  Every block is a piece that starts a run of its own, as a walk part does.
inline void summaries_to_batches(const DpBlockSum* s, size_t n_blocks, int64_t records_before, uint64_t ord_hi, DpChunkLayout* out) {
    out->batches.clear(); out->n_rec = out->n_out = out->n_cig = out->n_seq = 0; out->flags = 0; out->has_last = false; out->max_rec = 0;
    for (size_t b = 0; b < n_blocks; b++) { out->flags |= s[b].flags; if (s[b].n_runs > (uint32_t)DP_MAX_RUNS) out->flags |= DP_F_RUNS; }
    if (out->flags) return;
    int32_t cur_c = -1; int64_t seg0 = 0, seg_r = 0; size_t seg_cig = 0, seg_seq = 0;
    auto close_batch = [&](int64_t oi, size_t cg, size_t sq) {
        if (cur_c >= 0 && oi > seg0) out->batches.push_back({cur_c, seg0, oi, ord_hi | (uint64_t)(records_before + seg_r), (uint32_t)(cg - seg_cig), (uint32_t)(sq - seg_seq)});
    };
    for (size_t b = 0; b < n_blocks; b++) {
        const DpBlockSum& bs = s[b];
        for (uint32_t ri = 0; ri < bs.n_runs; ri++) {
            const DpRun& rn = bs.runs[ri];
            if (rn.contig != cur_c) {
                const int64_t oi = (int64_t)(out->n_out + rn.out_at); const size_t cg = out->n_cig + rn.cig_at, sq = out->n_seq + rn.seq_at;
                close_batch(oi, cg, sq);
                cur_c = rn.contig; seg0 = oi; seg_r = (int64_t)(out->n_rec + rn.first); seg_cig = cg; seg_seq = sq;
            }
        }
        if (bs.n_rec) { out->has_last = true; out->last_tid = bs.last_tid; out->last_pos = bs.last_pos; }
        if (bs.n_rec > out->max_rec) out->max_rec = bs.n_rec;
        out->n_rec += bs.n_rec; out->n_out += bs.n_out; out->n_cig += bs.n_cig; out->n_seq += bs.n_seq;
    }
    close_batch((int64_t)out->n_out, out->n_cig, out->n_seq);
}

// ---- what the parse kernel needs besides the slot's buffers ---------------------------------------------------------------------
struct DpBcSlot { uint64_t h; int32_t idx; uint16_t len; char key[18]; };   // = DecodeCfg::BcSlot (uploaded as it is)
struct DpParseCfg {
    const DpBcSlot* bc; uint64_t bc_mask;  // barcode table in device memory (bc == nullptr: empty list)
    int32_t use_barcodes, want_seq, umi_bits, sample;
    char cell_tag[2], umi_tag[2];
    int32_t names;                         // device-names mode (intern_dev.h): no UMI tag is looked for and the umi column is left to k_intern_recs
    int32_t filter_on;                     // the handle's tag filter (DecodeCfg::filter_*): 0 = the aux scan looks for nothing more and nothing is counted
    char filter_tag[2], pad[2];
    uint32_t filter_mask, filter_value;
    int32_t want_qual;                     // the handle has a base-quality floor: the records' quality bytes go to the block's quality region (wave-uniform, as every field here)
};

// The tag filter's verdict on the first occurrence of the tag: t at its type byte, its value bytes inside the record (the caller has
// skipped over it).  Integer types only; the value widened to 64 bits must lie in 0 .. 2^32 - 1 - which every type but a negative
// c / s / i does - and agree with `value` under `mask`.  One rule for parse_record (bam_records.cpp) and k_parse: byte loads.
XCK_HD inline bool tag_filter_pass(const uint8_t* t, uint32_t mask, uint32_t value) {
    long long v;
    switch (t[0]) {
        case 'c': v = (int8_t)t[1]; break;
        case 'C': v = t[1]; break;
        case 's': v = (int16_t)(uint16_t)((uint32_t)t[1] | ((uint32_t)t[2] << 8)); break;
        case 'S': v = (long long)((uint32_t)t[1] | ((uint32_t)t[2] << 8)); break;
        case 'i': v = (int32_t)((uint32_t)t[1] | ((uint32_t)t[2] << 8) | ((uint32_t)t[3] << 16) | ((uint32_t)t[4] << 24)); break;
        case 'I': v = (long long)((uint32_t)t[1] | ((uint32_t)t[2] << 8) | ((uint32_t)t[3] << 16) | ((uint32_t)t[4] << 24)); break;
        default: return false;             // A Z H f B
    }
    return v >= 0 && v <= 0xFFFFFFFFll && ((uint32_t)v & mask) == value;
}

}  // namespace xck

#include "inflate_dev.h"
namespace xck {
struct DpWalk { uint32_t first_skip; DpContigMap cm; bool want_seq; };       // (cm's tables in device memory)
// walk + scan of the chunk the slot's inflate kernel was just enqueued for, on the slot's stream; 0 = enqueued
int dev_walk_launch(GpuInflateSlot* s, size_t n_blocks, const DpWalk& w);
// the parse of a walked chunk into `out` (a SoA block of soa_layout(n_out + 1, n_cig + 1, want_seq ? n_seq + 1 : 1)) on `stream`
// (max_rec: most records of one block - a wave parses 64 records of a block)
// (cfg.want_qual: the block is followed by its quality region, soa_qual_bytes(n_seq + 1) bytes at the layout's total)
int dev_parse_launch(hipStream_t stream, const GpuInflateSlot* s, size_t n_blocks, size_t max_rec, const DpParseCfg& cfg, uint8_t* out, size_t n_out, size_t n_cig, size_t n_seq);
// the fallback: the chunk's inflated bytes d_out -> h_out on the slot's stream, waited for; 0 = they are there
int dev_parse_copy_out(GpuInflateSlot* s, size_t bytes);
void* dev_parse_upload(int device, const void* a, size_t a_bytes, const void* b, size_t b_bytes);   // a then b in one device buffer (nullptr: failed)
void  dev_parse_free(int device, void* p);
}
