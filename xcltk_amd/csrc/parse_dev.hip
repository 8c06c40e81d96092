// parse_dev.hip - record walk, scan and parse of a GPU-inflated chunk on the device (see parse_dev.h).
//
//   k_walk   one lane per BGZF block follows the block_size chain of its block (a few hundred dependent loads against bytes k_inflate
//            has just written; all blocks of the chunk at once), applies the contig map and notes per record where it lies and where
//            its output goes within the block; per block the counts, the contig runs and the last record's tid / pos.
//   k_scan   one workgroup: per-block counts -> bases, the chunk's totals and flags.
//   k_parse  one wave per 64 records of a block, one lane per record: the fixed fields and the aux scan (bam_records.cpp parse_record, restated bit for bit),
//            then CIGAR and sequence bytes wave-cooperatively - the outputs of 64 consecutive records are contiguous.  With the handle's tag
//            filter on, the aux scan also looks for that tag, a failing record gets XCK_CELL_FILTERED, and k_filtered_out (one thread,
//            behind it) hands the chunk's count to its head record.
// The walk and the scan run on the slot's stream behind k_inflate; the parse is launched by the engine's push path into its staging slot.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include "../../include/xck.h"
#include "parse_dev.h"
#include "intern_dev.h"

namespace xck {

__device__ __forceinline__ uint32_t ld32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// ---- walk --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_walk(const uint8_t* __restrict__ u, const DevBlock* __restrict__ bl, const int32_t* __restrict__ status, int n_blocks,
                                             uint32_t first_skip, DpContigMap cm, int want_seq, DpRec* __restrict__ rec, DpCnt* __restrict__ cnt, DpBlockSum* __restrict__ sum) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n_blocks) return;
    const DevBlock blk = bl[b];
    DpBlockSum s; memset(&s, 0, sizeof s);
    s.last_tid = -1;
    const uint32_t rec_at = blk.out_off / 36u;
    size_t o = (size_t)blk.out_off + (b == 0 ? first_skip : 0u); const size_t end = (size_t)blk.out_off + blk.out_len;
    if (status[b] != 0) s.flags |= DP_F_STATUS;
    else if (o > end) s.flags |= DP_F_STRADDLE;
    else {
        int32_t cur_c = INT32_MIN;
        DpRec* out = rec + rec_at;
        while (o + 4 <= end) {
            const uint32_t bs = ld32(u + o);
            if (bs < 32) { s.flags |= DP_F_SHORT; break; }
            if (o + 4 + (size_t)bs > end) break;
            const uint8_t* r = u + o + 4;
            const int32_t tid = (int32_t)ld32(r), pos = (int32_t)ld32(r + 4);
            const uint32_t l_name = r[8], n_cig = ld16(r + 12), l_seq = ld32(r + 16);
            // the fields must lie inside the record (parse_record's check): a record that fails it is left to the host, so the offsets
            // below never run ahead of what the chunk's bytes can hold
            if (32ull + l_name + (unsigned long long)n_cig * 4 + ((unsigned long long)l_seq + 1) / 2 + l_seq > (unsigned long long)bs) s.flags |= DP_F_OVERRUN;
            const int32_t ctg = dp_contig(cm, tid, pos);
            if (ctg != cur_c) {
                if (s.n_runs < (uint32_t)DP_MAX_RUNS) s.runs[s.n_runs] = DpRun{s.n_rec, ctg, s.n_out, s.n_cig, s.n_seq}; else s.flags |= DP_F_RUNS;
                s.n_runs++; cur_c = ctg;
            }
            out[s.n_rec] = DpRec{(uint32_t)(o + 4), ctg >= 0 ? s.n_out : DP_DROPPED, s.n_cig, s.n_seq};
            if (ctg >= 0 && !(s.flags & DP_F_OVERRUN)) { s.n_out++; s.n_cig += n_cig; if (want_seq) s.n_seq += (l_seq + 1) / 2; }
            s.n_rec++; s.last_tid = tid; s.last_pos = pos;
            o += 4 + (size_t)bs;
        }
        if (o != end) s.flags |= DP_F_STRADDLE;
    }
    s.stop = (uint32_t)o;
    DpCnt c; memset(&c, 0, sizeof c);
    c.n_rec = s.n_rec; c.n_out = s.n_out; c.n_cig = s.n_cig; c.n_seq = s.n_seq; c.flags = s.flags; c.rec_at = rec_at;
    cnt[b] = c;
    sum[b] = s;
}

// ---- scan --------------------------------------------------------------------------------------------------------------------------
constexpr int SCAN_T = 256;
__global__ __launch_bounds__(SCAN_T) void k_scan(const DpCnt* __restrict__ cnt, int n_blocks, DpBase* __restrict__ base, DpHead* __restrict__ head) {
    __shared__ uint32_t s_out[SCAN_T], s_cig[SCAN_T], s_seq[SCAN_T], s_rec[SCAN_T], s_fl[SCAN_T];
    const int t = (int)threadIdx.x, per = (n_blocks + SCAN_T - 1) / SCAN_T, b0 = min(t * per, n_blocks), b1 = min(b0 + per, n_blocks);
    uint32_t a_out = 0, a_cig = 0, a_seq = 0, a_rec = 0, fl = 0;
    for (int b = b0; b < b1; b++) { const DpCnt c = cnt[b]; a_out += c.n_out; a_cig += c.n_cig; a_seq += c.n_seq; a_rec += c.n_rec; fl |= c.flags; }
    s_out[t] = a_out; s_cig[t] = a_cig; s_seq[t] = a_seq; s_rec[t] = a_rec; s_fl[t] = fl;
    __syncthreads();
    if (t == 0) {
        uint32_t o = 0, c = 0, q = 0, r = 0, f = 0;
        for (int k = 0; k < SCAN_T; k++) { const uint32_t x = s_out[k], y = s_cig[k], z = s_seq[k]; s_out[k] = o; s_cig[k] = c; s_seq[k] = q; o += x; c += y; q += z; r += s_rec[k]; f |= s_fl[k]; }
        DpHead h; memset(&h, 0, sizeof h);
        h.walk_flags = f; h.n_rec = r; h.n_out = o; h.n_cig = c; h.n_seq = q;
        *head = h;
    }
    __syncthreads();
    uint32_t o = s_out[t], c = s_cig[t], q = s_seq[t];
    for (int b = b0; b < b1; b++) { const DpCnt x = cnt[b]; base[b] = DpBase{o, c, q, 0}; o += x.n_out; c += x.n_cig; q += x.n_seq; }
}

// ---- parse -------------------------------------------------------------------------------------------------------------------------
// (dp_hash_bytes = bam_records.cpp hash_bytes and dp_encode_direct = its encode_key_direct: intern_dev.h, which the name kernels share)
// DecodeCfg::lookup_cell for lists whose barcodes all fit a slot's key (the device path is on only then): same hash, same probe order
__device__ inline int32_t dp_lookup_cell(const DpParseCfg& cfg, const uint8_t* s, size_t n) {
    if (!cfg.bc) return -1;
    if (n > sizeof(DpBcSlot::key)) return -1;                              // no slot of such a list has this length
    const uint64_t hh = dp_hash_bytes(s, (uint32_t)n);
    uint64_t h = hh & cfg.bc_mask;
    for (;;) {
        const DpBcSlot& sl = cfg.bc[h];
        const int32_t idx = sl.idx;
        if (idx < 0) return -1;
        if (sl.h == hh && sl.len == (uint16_t)n) {
            bool same = true;
            for (size_t k = 0; k < n; k++) same = same && (uint8_t)sl.key[k] == s[k];
            if (same) return idx;
        }
        h = (h + 1) & cfg.bc_mask;
    }
}
// bam_records.cpp aux_skip on offsets: a at the type byte, e the record's end; returns the next tag's offset, or -1
__device__ inline long long dp_aux_skip(const uint8_t* r, long long a, long long e) {
    if (a >= e) return -1;
    const uint8_t t = r[a++];
    switch (t) {
        case 'A': case 'c': case 'C': a += 1; break;
        case 's': case 'S': a += 2; break;
        case 'i': case 'I': case 'f': a += 4; break;
        case 'Z': case 'H': { while (a < e && r[a] != 0) a++; if (a >= e) return -1; a++; break; }
        case 'B': { if (a + 5 > e) return -1; const uint8_t st = r[a]; const uint32_t n = ld32(r + a + 1); a += 5;
                    const long long sz = (st == 'c' || st == 'C') ? 1 : (st == 's' || st == 'S') ? 2 : 4; a += (long long)n * sz; break; }
        default: return -1;
    }
    return a <= e ? a : -1;
}
// strnlen(v, e - v)
__device__ inline size_t dp_strnlen(const uint8_t* r, long long v, long long e) { long long k = v; while (k < e && r[k] != 0) k++; return (size_t)(k - v); }

// dst[start[0] .. start[64]) is contiguous over the 64 records of a round; record i's bytes come from src[i]: every lane takes the
// bytes lane, lane + 64, ... of the range and finds the record a byte belongs to by bisection over the starts in LDS
__device__ inline void coop_copy(const uint8_t* __restrict__ u, uint8_t* __restrict__ dst, const uint32_t* start, const uint32_t* src, int lane) {
    const uint32_t lo = start[0], hi = start[64];
    for (uint32_t j = lo + (uint32_t)lane; j < hi; j += 64) {
        int a = 0, z = 64;                                                  // last i in [0, 64) with start[i] <= j
        while (z - a > 1) { const int m = (a + z) >> 1; if (start[m] <= j) a = m; else z = m; }
        dst[j] = u[(size_t)src[a] + (j - start[a])];
    }
}

// the quality bytes of the round (a handle with a base-quality floor): two per sequence byte, so the destination is [2 * start[0],
// 2 * start[64]) of the quality region; record i's l_seq[i] bytes lie behind its sequence bytes (src[i] + (start[i + 1] - start[i])
// for a kept record, carried as qsrc[i]), and the one byte an odd l_seq leaves over is the pad, 0xff = "no quality"
__device__ inline void coop_copy_qual(const uint8_t* __restrict__ u, uint8_t* __restrict__ dst, const uint32_t* start, const uint32_t* qsrc, const uint32_t* l_seq, int lane) {
    const size_t lo = 2 * (size_t)start[0], hi = 2 * (size_t)start[64];
    for (size_t j = lo + (size_t)lane; j < hi; j += 64) {
        const uint32_t by = (uint32_t)(j >> 1);
        int a = 0, z = 64;                                                  // last i in [0, 64) with start[i] <= by
        while (z - a > 1) { const int m = (a + z) >> 1; if (start[m] <= by) a = m; else z = m; }
        const uint32_t k = (uint32_t)(j - 2 * (size_t)start[a]);
        dst[j] = k < l_seq[a] ? u[(size_t)qsrc[a] + k] : (uint8_t)0xff;
    }
}

// the same for the CIGAR column in whole words: its destination is 4-byte aligned, start[] counts words, a record's source is not aligned
__device__ inline void coop_copy_words(const uint8_t* __restrict__ u, uint32_t* __restrict__ dst, const uint32_t* start, const uint32_t* src, int lane) {
    const uint32_t lo = start[0], hi = start[64];
    for (uint32_t j = lo + (uint32_t)lane; j < hi; j += 64) {
        int a = 0, z = 64;
        while (z - a > 1) { const int m = (a + z) >> 1; if (start[m] <= j) a = m; else z = m; }
        dst[j] = ld32(u + (size_t)src[a] + (size_t)(j - start[a]) * 4);
    }
}

__global__ __launch_bounds__(64) void k_parse(const uint8_t* __restrict__ u, const DpRec* __restrict__ rec, const DpCnt* __restrict__ cnt, const DpBase* __restrict__ base,
                                              DpParseCfg cfg, uint8_t* __restrict__ out, SoaLayout lay, uint32_t n_out_total, uint32_t n_cig_total, uint32_t n_seq_total,
                                              DpHead* __restrict__ head, uint32_t* __restrict__ n_filtered) {
    __shared__ uint32_t s_cst[65], s_csrc[64], s_sst[65], s_ssrc[64], s_qsrc[64], s_lseq[64];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    uint64_t* c_umi = (uint64_t*)(out + lay.o_umi); int32_t* c_pos = (int32_t*)(out + lay.o_pos); int32_t* c_cell = (int32_t*)(out + lay.o_cell);
    uint32_t* c_cgo = (uint32_t*)(out + lay.o_cgo); uint32_t* c_sqo = (uint32_t*)(out + lay.o_sqo); uint32_t* c_cig = (uint32_t*)(out + lay.o_cig);
    uint16_t* c_flag = (uint16_t*)(out + lay.o_flag); uint8_t* c_mapq = out + lay.o_mapq; uint8_t* c_seq = out + lay.o_seq;
    if (b == 0 && lane == 0) { c_cgo[n_out_total] = n_cig_total; c_sqo[n_out_total] = n_seq_total; }   // (layout_chunk closes the offset columns)
    const DpCnt c = cnt[b]; const DpBase bs = base[b];
    const DpRec* rl = rec + c.rec_at;
    uint32_t fl = 0;
    // (a wave per round of 64 records, not per block: the aux scan is a chain of dependent loads, and a chunk's ~800 blocks alone left
    // most of the device idle while the push thread waited for the kernel)
    const uint32_t r0 = blockIdx.y * 64u;
    if (r0 < c.n_rec) {
        const uint32_t ri = r0 + (uint32_t)lane;
        const bool have = ri < c.n_rec;
        DpRec rr = have ? rl[ri] : DpRec{0, DP_DROPPED, c.n_cig, c.n_seq};
        const bool kept = have && rr.slot != DP_DROPPED;
        uint32_t cig_len = 0, seq_len = 0, cig_src = 0, seq_src = 0, q_len = 0;
        bool filtered = false;
        if (kept) {
            const uint8_t* r = u + rr.off;
            const long long end = (long long)ld32(r - 4);                   // block_size: the record's bytes are r[0, end)
            const uint32_t l_name = r[8], n_cig = ld16(r + 12), l_seq = ld32(r + 16);
            const size_t o = (size_t)bs.out + rr.slot;
            if (o < n_out_total) {                                          // (always: the bases come from the same counts)
                c_pos[o] = (int32_t)ld32(r + 4); c_mapq[o] = r[9]; c_flag[o] = (uint16_t)ld16(r + 14);
                c_cgo[o] = bs.cig + rr.cig; c_sqo[o] = bs.seq + rr.seq;
                long long q = 32 + (long long)l_name;                       // (the walk checked that the fields lie inside the record)
                cig_src = rr.off + (uint32_t)q; cig_len = n_cig;
                q += (long long)n_cig * 4;
                if (cfg.want_seq) { seq_src = rr.off + (uint32_t)q; seq_len = (l_seq + 1) / 2; q_len = l_seq; }
                q += (long long)((l_seq + 1) / 2) + l_seq;
                // aux tags: first occurrence wins; the scan ends when all that are looked for are found or a value cannot be skipped
                // (xf: the handle's tag filter, looked for only when it is on - a record without the tag is then walked to its end)
                long long cb = -1, ub = -1, xf = -1; bool need_cb = cfg.use_barcodes != 0, need_ub = cfg.names == 0, need_xf = cfg.filter_on != 0; long long a = q;   // (names: the key is the read name, k_intern_recs writes it)
                while ((need_cb || need_ub || need_xf) && a >= 0 && a + 3 <= end) {
                    if (need_cb && r[a] == (uint8_t)cfg.cell_tag[0] && r[a + 1] == (uint8_t)cfg.cell_tag[1]) { cb = a + 2; need_cb = false; }
                    else if (need_ub && r[a] == (uint8_t)cfg.umi_tag[0] && r[a + 1] == (uint8_t)cfg.umi_tag[1]) { ub = a + 2; need_ub = false; }
                    else if (need_xf && r[a] == (uint8_t)cfg.filter_tag[0] && r[a + 1] == (uint8_t)cfg.filter_tag[1]) { xf = a + 2; need_xf = false; }
                    a = dp_aux_skip(r, a + 2, end);
                }
                int32_t cell = -1;
                if (cfg.use_barcodes) {
                    if (cb >= 0 && (r[cb] == 'Z' || r[cb] == 'A' || r[cb] == 'H')) {
                        const size_t n = r[cb] == 'A' ? 1 : dp_strnlen(r, cb + 1, end);
                        cell = dp_lookup_cell(cfg, r + cb + 1, n);
                    }
                } else cell = cfg.sample;
                // the tag filter's verdict overrides the cell (parse_record): absent, not an integer, negative or cut off -> filtered
                if (cfg.filter_on && !(xf >= 0 && dp_aux_skip(r, xf, end) >= 0 && tag_filter_pass(r + xf, cfg.filter_mask, cfg.filter_value))) { cell = XCK_CELL_FILTERED; filtered = true; }
                c_cell[o] = cell;
                uint64_t key = XCK_UMI_NONE;
                if (ub >= 0) {
                    if (r[ub] == 'Z' || r[ub] == 'A' || r[ub] == 'H') {
                        const size_t n = r[ub] == 'A' ? 1 : dp_strnlen(r, ub + 1, end);
                        if (!dp_encode_direct(r + ub + 1, n, cfg.umi_bits, &key)) { key = XCK_UMI_NONE; fl |= DP_F_UMI; }   // (the host interns it)
                    } else fl |= DP_F_UMI;                                  // numeric tag: its key is interned on the host
                }
                if (!cfg.names) c_umi[o] = key;
            }
        }
        // the CIGAR words and sequence bytes of the round, all lanes together
        s_cst[lane] = bs.cig + rr.cig; s_csrc[lane] = cig_src; s_sst[lane] = bs.seq + rr.seq; s_ssrc[lane] = seq_src;
        // (the end of the round's range: the last lane's start + length; lanes past the list start at the block's end, length 0)
        if (lane == 63) { s_cst[64] = bs.cig + rr.cig + cig_len; s_sst[64] = bs.seq + rr.seq + seq_len; }
        if (cfg.want_qual) { s_qsrc[lane] = seq_src + seq_len; s_lseq[lane] = q_len; }
        __syncthreads();
        if (s_cst[64] <= n_cig_total) coop_copy_words(u, c_cig, s_cst, s_csrc, lane);
        if (cfg.want_seq && s_sst[64] <= n_seq_total) coop_copy(u, c_seq, s_sst, s_ssrc, lane);
        if (cfg.want_qual && s_sst[64] <= n_seq_total) coop_copy_qual(u, out + lay.total, s_sst, s_qsrc, s_lseq, lane);   // (the region holds 2 * (n_seq_total + 1) bytes at least)
        // the chunk's filtered records: one ballot per wave, one add per wave that has any (the whole wave is here: r0 < c.n_rec is uniform).
        // The counter is in DEVICE memory (k_filtered_out hands it to the head record): with most waves adding, an atomic per wave on the
        // head's mapped host memory made the parse of a chunk wait for thousands of PCIe round trips
        if (cfg.filter_on) {
            const unsigned long long m = __ballot(filtered);
            if (lane == 0 && m) atomicAdd(n_filtered, (uint32_t)__popcll(m));
        }
    }
    if (fl) atomicOr(&head->parse_flags, fl);
}

// behind k_parse, tag filter on: the chunk's count -> its head record (mapped host memory), the slot's counter back to zero for its next chunk
__global__ void k_filtered_out(uint32_t* __restrict__ n_filtered, DpHead* __restrict__ head) { head->n_filtered = *n_filtered; *n_filtered = 0; }

// ---- host side ---------------------------------------------------------------------------------------------------------------------
int dev_walk_launch(GpuInflateSlot* s, size_t n_blocks, const DpWalk& w) {
    if (n_blocks == 0) return 0;
    const unsigned g = (unsigned)((n_blocks + 63) / 64);
    hipLaunchKernelGGL(k_walk, dim3(g), dim3(64), 0, s->stream, (const uint8_t*)s->d_out, (const DevBlock*)s->a_bl, (const int32_t*)s->a_st, (int)n_blocks,
                       w.first_skip, w.cm, w.want_seq ? 1 : 0, s->d_rec, s->d_cnt, s->a_sum);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(SCAN_T), 0, s->stream, (const DpCnt*)s->d_cnt, (int)n_blocks, s->d_base, s->a_head);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int dev_parse_launch(hipStream_t stream, const GpuInflateSlot* s, size_t n_blocks, size_t max_rec, const DpParseCfg& cfg, uint8_t* out, size_t n_out, size_t n_cig, size_t n_seq) {
    if (n_blocks == 0) return 0;
    const SoaLayout lay = soa_layout(n_out + 1, n_cig + 1, cfg.want_seq ? n_seq + 1 : 1);
    s->h_head->parse_flags = 0; s->h_head->n_filtered = 0;
    const unsigned rounds = (unsigned)std::min<size_t>(std::max<size_t>((max_rec + 63) / 64, 1), 65535);   // (a block holds at most 65536 / 36 records)
    hipLaunchKernelGGL(k_parse, dim3((unsigned)n_blocks, rounds), dim3(64), 0, stream, (const uint8_t*)s->d_out, (const DpRec*)s->d_rec, (const DpCnt*)s->d_cnt, (const DpBase*)s->d_base,
                       cfg, out, lay, (uint32_t)n_out, (uint32_t)n_cig, (uint32_t)n_seq, s->a_head, s->d_nfilt);
    if (cfg.filter_on) hipLaunchKernelGGL(k_filtered_out, dim3(1), dim3(1), 0, stream, s->d_nfilt, s->a_head);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int dev_parse_copy_out(GpuInflateSlot* s, size_t bytes) {
    if (hipSetDevice(s->device) != hipSuccess) return -1;
    if (hipMemcpyAsync(s->h_out, s->d_out, bytes, hipMemcpyDeviceToHost, s->stream) != hipSuccess || hipStreamSynchronize(s->stream) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return 0;
}

void* dev_parse_upload(int device, const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    void* d = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&d, a_bytes + b_bytes + 16) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if ((a_bytes && hipMemcpy(d, a, a_bytes, hipMemcpyHostToDevice) != hipSuccess) || (b_bytes && hipMemcpy((char*)d + a_bytes, b, b_bytes, hipMemcpyHostToDevice) != hipSuccess)) {
        (void)hipGetLastError(); (void)hipFree(d); return nullptr;
    }
    return d;
}
void dev_parse_free(int device, void* p) { if (p && hipSetDevice(device) == hipSuccess) (void)hipFree(p); }

}  // namespace xck
