// pipeline.hip - MI355X (gfx950) counting engine: the per-GPU push pipeline.  Host code only - no kernel is defined here.
//
//   buffers     : grow-only device / pinned buffers, the workspaces, the hit streams of the 16 shards (ensure_hits), the batch slots.
//   launch queue: launch_queue() turns the queued batches into ONE fused join launch (engine.hip launch_join) and the opt-in summary
//                 passes behind it (launch_summaries); complete_pending() waits for it, and when a fragment did not fit grows the
//                 streams, rewinds the cursors and replays the join alone.
//   push paths  : engine_push (host arrays -> a BatchSlot pair, or device-resident batches queued as they are), engine_push_block and
//                 engine_push_parsed (one decoded chunk in a staging slot of the Stager, shared by the handle's pipelines), and the
//                 read-name table of device-names mode, which lives with the staging.
//   lifecycle   : engine_create / engine_reset / engine_destroy / engine_stats.
//
// It is a unit of its own because nearly every feature edits this code and none of them changes what the join reads or writes: the
// traffic stamp (profiles/pmc_traffic.json) hashes engine.hip, and a host edit there made it stale.  Of the join it knows the batch
// table it fills the queue for and the functions engine_impl.h declares; of the summaries three calls and no constant.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <hip/hip_runtime.h>
#include "engine_impl.h"
#include "parse_dev.h"
#include "intern_dev.h"

namespace xck {
// Device staging of decoded chunks for the host ingest (engine_push_block): the decoder hands over one pinned block per
// chunk, it is copied with ONE hipMemcpyAsync into one of three slots, and every pipeline of the handle (basefc and pileup of a
// fused handle) reads the same copy.  A slot is reused once every launch that reads it has been confirmed (its hits fitted).
struct Stager {
    int device = 0; hipStream_t s_copy = nullptr;
    struct Slot { char* buf = nullptr; size_t cap = 0; hipEvent_t t0 = nullptr, copied = nullptr; int users = 0; bool timed = false; } slot[3];
    int next = 0;
    void* d_bc = nullptr;               // the decoder's barcode table, for the parse kernel (engine_push_parsed)
};


size_t key_bytes(const EngineImpl* im) { return im->key_bits == 64 ? 8 : 16; }

// Grow-only buffers (capacities in bytes): afterwards *p holds at least `need` bytes.  A buffer that is too small is freed and
// allocated anew with need + slack bytes - its contents are not kept - and a failure leaves it empty (null, capacity 0).
int grow_device(EngineImpl* im, void** p, size_t* cap, size_t need, size_t slack) {
    if (need <= *cap) return 0;
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc(p, need + slack));
    *cap = need + slack;
    return 0;
}
// ... and its twin for pinned, mapped host memory
int grow_pinned(EngineImpl* im, void** p, size_t* cap, size_t need, size_t slack) {
    if (need <= *cap) return 0;
    if (*p) HIP_TRY(hipHostFree(*p));
    *p = nullptr; *cap = 0;
    HIP_TRY(hipHostMalloc(p, need + slack, hipHostMallocMapped));
    *cap = need + slack;
    return 0;
}
// a device buffer of its own, all zero (the control words, the summaries' tables)
int dev_zeroed(EngineImpl* im, void** p, size_t bytes) {
    HIP_TRY(hipMalloc(p, bytes));
    HIP_TRY(hipMemset(*p, 0, bytes));
    return 0;
}

int arena_begin(EngineImpl* im, Arena& a, size_t need) {
    a.off = 0;
    return grow_device(im, (void**)&a.base, &a.cap, need, need / 4 + (1 << 20));
}

int res_reserve(EngineImpl* im, int m, size_t nnz) {
    return grow_pinned(im, (void**)&im->h_res[m], &im->h_res_cap[m], nnz * 3 * sizeof(int32_t), (nnz / 2 + 1024) * sizeof(int32_t));
}

// per-shard head room added to every capacity guess (XCK_HIT_SLACK: test knob that makes the overflow / replay path easy to reach)
size_t hit_slack(const EngineImpl* im) { return (size_t)im->eng->knobs.hit_slack; }
bool split_mode(const EngineImpl* im) { return XCK_BAF_SPLIT && im->mode == XCK_MODE_BAF && im->key_bits == 64; }

static int ensure_hits(EngineImpl* im, size_t need) {           // need = elements per shard
    if (need <= im->hit_cap) return 0;
    const size_t ncap = std::max<size_t>(need, im->hit_cap * 2), kb = key_bytes(im);
    // the four streams (keys, vals; no-base keys, vals), each with its element size (0 = this pipeline has no such stream)
    void* old[4] = { im->d_keys, im->d_vals, im->d_nkeys, im->d_nvals };
    void* nw[4] = { nullptr, nullptr, nullptr, nullptr };
    const size_t elt[4] = { kb, im->mode == XCK_MODE_BAF ? sizeof(uint64_t) : 0, split_mode(im) ? sizeof(uint64_t) : 0, split_mode(im) ? sizeof(uint64_t) : 0 };
    // new buffers, and what the shards hold moved to its place in them
    const auto move = [&]() -> int {
        for (int q = 0; q < 4; q++) {
            if (!elt[q]) continue;
            HIP_TRY(hipMalloc(&nw[q], ncap * NSHARD * elt[q]));
            const unsigned long long* cnt = q < 2 ? im->cur : im->ncur;
            for (int sh = 0; sh < NSHARD; sh++) if (cnt[sh])
                HIP_TRY(hipMemcpyAsync((char*)nw[q] + (size_t)sh * ncap * elt[q], (char*)old[q] + (size_t)sh * im->hit_cap * elt[q], cnt[sh] * elt[q], hipMemcpyDeviceToDevice, im->s_comp));
        }
        HIP_TRY(hipStreamSynchronize(im->s_comp));
        return 0;
    };
    if (const int rc = move()) {                                 // (the old buffers stay as they are; nothing new is kept)
        hipStreamSynchronize(im->s_comp);
        for (void* p : nw) if (p) hipFree(p);
        return rc;
    }
    for (void* p : old) if (p) HIP_TRY(hipFree(p));
    im->d_keys = nw[0]; im->d_vals = (uint64_t*)nw[1]; im->d_nkeys = nw[2]; im->d_nvals = (uint64_t*)nw[3]; im->hit_cap = ncap;
    return 0;
}

// (capacities: cap_reads in reads, shared by the seven per-read columns; cap_cig and cap_seq in bytes.  Every one at least doubles.)
static int slot_reserve(EngineImpl* im, BatchSlot& s, size_t n_reads, size_t n_cig, size_t n_seq) {
    if (n_reads > s.cap_reads) {
        const size_t c = std::max(n_reads, s.cap_reads * 2);
        struct { void** p; size_t bytes; } col[7] = { { (void**)&s.pos, c * 4 }, { (void**)&s.flag, c * 2 }, { (void**)&s.mapq, c }, { (void**)&s.cell, c * 4 }, { (void**)&s.umi, c * 8 },
                                                       { (void**)&s.cig_off, (c + 1) * 4 }, { (void**)&s.seq_off, (c + 1) * 4 } };
        s.cap_reads = 0;
        for (auto& x : col) { size_t cap = 0; if (const int rc = grow_device(im, x.p, &cap, x.bytes, 0)) return rc; }
        s.cap_reads = c;
    }
    const size_t cig = n_cig * 4;
    if (const int rc = grow_device(im, (void**)&s.cigar, &s.cap_cig, cig, std::max(cig, s.cap_cig * 2) - cig)) return rc;
    return grow_device(im, (void**)&s.seq, &s.cap_seq, n_seq, std::max(n_seq, s.cap_seq * 2) - n_seq);
}

// wait for the launch in flight, collect cursor / timing; if its fragments did not fit, grow, rewind and replay
int complete_pending(EngineImpl* im) {
    while (!im->inflight.empty()) {
        HIP_TRY(hipStreamSynchronize(im->s_comp));
        float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, im->ev0, im->ev1));
        im->st.ms_join += ms; im->st.ms_device += ms; im->n_join_launches++;
        if (const int rc = join_stamps_collect(im, ms)) return rc;   // (XCK_STAMPS builds; otherwise empty)
        if (im->h_ctl[CTL_OVERFLOW]) {                       // some fragment did not fit: grow, rewind, replay
            unsigned long long mx = 0;
            for (int sh = 0; sh < NSHARD; sh++) mx = std::max(mx, std::max(im->h_ctl[ctl_cursor(sh)], im->h_ctl[ctl_ncursor(sh)]));
            int rc = ensure_hits(im, std::max<size_t>(mx + mx / 4 + 65536, im->hit_cap * 2)); if (rc) return rc;
            for (int sh = 0; sh < NSHARD; sh++) { im->h_ctl[ctl_cursor(sh)] = im->cur_before[sh]; im->h_ctl[ctl_ncursor(sh)] = im->ncur_before[sh];
                                                  im->h_ctl[ctl_accepted(sh)] = im->acc_before[sh];
                                                  im->h_ctl[ctl_bq_base(sh)] = im->bqb_before[sh]; im->h_ctl[ctl_bq_masked(sh)] = im->bqm_before[sh]; }
            im->h_ctl[CTL_OVERFLOW] = 0;
            HIP_TRY(hipMemcpyAsync(im->d_ctl, im->h_ctl, CTL_WORDS * sizeof(unsigned long long), hipMemcpyHostToDevice, im->s_comp));
            HIP_TRY(hipStreamSynchronize(im->s_comp));
            rc = launch_join(im); if (rc) return rc;
            continue;
        }
        im->cursor = 0; im->ncursor = 0;
        for (int sh = 0; sh < NSHARD; sh++) { im->cur[sh] = im->h_ctl[ctl_cursor(sh)]; im->cursor += im->cur[sh];
                                              im->ncur[sh] = split_mode(im) ? im->h_ctl[ctl_ncursor(sh)] : 0; im->ncursor += im->ncur[sh]; }
        if (im->inflight_slot >= 0) im->slot[im->inflight_slot].busy = false;
        if (im->inflight_shared >= 0 && im->eng->stager) { im->eng->stager->slot[im->inflight_shared].users--; im->inflight_shared = -1; }
        im->inflight.clear(); im->inflight_slot = -1; im->inflight_reads = 0;
    }
    return 0;
}

// launch whatever is queued (after the previous launch has been confirmed)
int launch_queue(EngineImpl* im, int slot_idx, int shared_slot) {
    if (im->queue.empty()) return 0;
    int rc = complete_pending(im); if (rc) return rc;
    { unsigned long long mx = 0;
      for (int sh = 0; sh < NSHARD; sh++) mx = std::max(mx, std::max(im->cur[sh], im->ncur[sh]));
      // first guess: 1.25 keys per queued read (after the LDS de-duplication a 10x run leaves ~0.8); a launch that needs
      // more sets the overflow flag and is replayed into grown buffers, and the capacity is kept for the next pass
      rc = ensure_hits(im, mx + (size_t)im->queued_reads * 5 / 4 / NSHARD + hit_slack(im)); if (rc) return rc; }
    im->inflight.swap(im->queue); im->queue.clear();
    im->inflight_reads = im->queued_reads; im->queued_reads = 0;
    im->inflight_slot = slot_idx;
    im->inflight_shared = shared_slot;
    if (shared_slot >= 0) im->eng->stager->slot[shared_slot].users++;
    for (int sh = 0; sh < NSHARD; sh++) { im->cur_before[sh] = im->cur[sh]; im->ncur_before[sh] = im->ncur[sh]; im->acc_before[sh] = im->h_ctl[ctl_accepted(sh)];
                                          im->bqb_before[sh] = im->h_ctl[ctl_bq_base(sh)]; im->bqm_before[sh] = im->h_ctl[ctl_bq_masked(sh)]; }
    if (slot_idx >= 0) im->slot[slot_idx].busy = true;
    rc = launch_join(im); if (rc) return rc;
    return launch_summaries(im);                               // (off: returns at once)
}

// ---- the push paths ----
// Which columns of a batch may be null differs by where they live.  COLS_HOST (engine_push from host arrays): a null cigar / seq
// pointer is fine when its offset range is empty - the same rule as xck_push_batch's check and its packed form.  COLS_DEVICE
// (device-resident batches): the offsets live in HBM, so the pointers must be there.  COLS_BLOCK (engine_push_block): the columns are
// slices of the block, laid out by the decoder or by xck_push_batch's packed form; only the sequence columns are asked about.
enum Columns { COLS_HOST, COLS_DEVICE, COLS_BLOCK };
static const char* null_column(const EngineImpl* im, const xck_batch* b, Columns c) {
    const bool seq = im->mode == XCK_MODE_BAF;
    if (c == COLS_BLOCK) return seq && (!b->seq_off || !b->seq) ? "BAF mode needs seq arrays" : nullptr;
    const bool dev = c == COLS_DEVICE;
    if (!b->pos || !b->flag || !b->mapq || !b->cell || !b->umi || !b->cig_off) return "null batch array";
    if (!b->cigar && (dev || b->cig_off[b->n_reads] != b->cig_off[0])) return "null batch array";
    if (seq && (!b->seq_off || (!b->seq && (dev || b->seq_off[b->n_reads] != b->seq_off[0])))) return "BAF mode needs seq arrays";
    return nullptr;
}

// What a push does with one batch, decided in one place: the batch is counted, its contig and its columns are checked, and the table
// half of its BatchDesc is filled (the column pointers are the caller's: they are what differs between the paths).
enum BatchFate { BATCH_ERROR = -1, BATCH_SKIP = 0, BATCH_QUEUE = 1 };    // ERROR: im->batch_rc (XCK_E_ARG unless a tally table could not be had), the text is in the handle; SKIP: counted, no kernel will see it
static BatchFate describe_batch(EngineImpl* im, const xck_batch* b, Columns cols, BatchDesc& d) {
    im->st.n_batches++; im->st.n_reads += b->n_reads;
    im->batch_rc = XCK_E_ARG;
    if (b->n_reads <= 0 || b->contig < 0) { im->n_not_joined += std::max(b->n_reads, 0); return BATCH_SKIP; }
    if (b->contig >= (int)im->ctab.size()) { im->eng->err = "batch contig out of range"; return BATCH_ERROR; }
    const ContigTab& t = im->ctab[b->contig];
    // (XCK_F_BASE_TALLY: the tally pass reads every batch, so a batch on a contig without SNPs is queued too - the join finds nothing in it)
    const bool has_targets = im->mode == XCK_MODE_BASEFC ? t.n_reg > 0 : (t.n_snp > 0 || im->base_tally);
    if (cols != COLS_BLOCK || has_targets)                           // (a block's batch is asked about only if a kernel will read it)
        if (const char* what = null_column(im, b, cols)) { im->eng->err = what; return BATCH_ERROR; }
    if (!has_targets) { im->n_not_joined += b->n_reads; return BATCH_SKIP; }
    if (im->base_tally) { if (const int rc = base_tally_touch(im, b->contig)) { im->batch_rc = rc; return BATCH_ERROR; } }
    memset(&d, 0, sizeof d);
    d.n = b->n_reads; d.ordinal_base = b->ordinal_base; d.contig = b->contig;
    d.reg_lo = t.reg_base; d.reg_hi = t.reg_base + t.n_reg;
    d.snp_win = im->d_snp_win + t.swin_base; d.n_swin = t.n_swin; d.snp_end = t.snp_base + t.n_snp;
    return BATCH_QUEUE;
}
// algorithmic bytes the join reads for a batch whose sizes the host knows (xck_stats.algo_bytes_join; n_seq: 0 without sequences)
static int64_t join_bytes(size_t n, size_t n_cig, size_t n_seq) { return (int64_t)n * 20 + (int64_t)n_cig * 4 + (int64_t)(n_seq / 2); }

int engine_push(EngineImpl* im, const xck_batch* b, bool device_resident, const uint8_t* qual) {
    xck_engine* e = im->eng;
    if (im->finished) { e->err = "push after finish (call xck_reset)"; return XCK_E_STATE; }
    if (im->min_baseq > 0 && (device_resident || !qual)) { e->err = "internal: a batch without qualities on a pipeline with a base-quality floor"; return XCK_E_STATE; }   // (xck_push_batch* refuse first)
    HIP_TRY(hipSetDevice(im->device));
    BatchDesc d;
    const BatchFate fate = describe_batch(im, b, device_resident ? COLS_DEVICE : COLS_HOST, d);
    if (fate != BATCH_QUEUE) return fate == BATCH_SKIP ? 0 : im->batch_rc;
    if (device_resident) {
        // deferred: consecutive device-resident batches are fused into one launch (>> 256 workgroups)
        d.pos = b->pos; d.flag = b->flag; d.mapq = b->mapq; d.cell = b->cell; d.umi = b->umi;
        d.cig_off = b->cig_off; d.cigar = b->cigar; d.seq_off = b->seq_off; d.seq = b->seq;
        im->queue.push_back(d); im->queued_reads += b->n_reads;
        if ((int)im->queue.size() >= MAX_FUSE) return launch_queue(im, -1);
        return 0;
    }
    int rc = launch_queue(im, -1); if (rc) return rc;          // keep launch order == push order
    const bool seq = im->mode == XCK_MODE_BAF;
    size_t n = (size_t)b->n_reads;
    // offsets need not start at 0 (a batch may be a window into a larger decode buffer)
    const uint32_t c_lo = b->cig_off[0], s_lo = seq ? b->seq_off[0] : 0;
    if (b->cig_off[n] < c_lo || (seq && b->seq_off[n] < s_lo)) { e->err = "batch offsets are not monotonic"; return XCK_E_ARG; }
    uint32_t n_cig = b->cig_off[n] - c_lo, n_seq = seq ? b->seq_off[n] - s_lo : 0;
    int slot_idx = im->next_slot; im->next_slot ^= 1;
    BatchSlot& s = im->slot[slot_idx];
    if (s.busy) { rc = complete_pending(im); if (rc) return rc; }   // slot still feeds the launch in flight
    rc = slot_reserve(im, s, n, std::max<uint32_t>(n_cig, 1), std::max<uint32_t>(n_seq, 1)); if (rc) return rc;
    const bool with_qual = seq && im->min_baseq > 0;                  // the quality column: allocated and copied like seq, two bytes per sequence byte
    if (with_qual) { const size_t nq = 2 * (size_t)std::max<uint32_t>(n_seq, 1); rc = grow_device(im, (void**)&s.qual, &s.cap_qual, nq, std::max(nq, s.cap_qual * 2) - nq); if (rc) return rc; }
    auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipMemcpyAsync(s.pos, b->pos, n * 4, hipMemcpyHostToDevice, im->s_copy));
    HIP_TRY(hipMemcpyAsync(s.flag, b->flag, n * 2, hipMemcpyHostToDevice, im->s_copy));
    HIP_TRY(hipMemcpyAsync(s.mapq, b->mapq, n, hipMemcpyHostToDevice, im->s_copy));
    HIP_TRY(hipMemcpyAsync(s.cell, b->cell, n * 4, hipMemcpyHostToDevice, im->s_copy));
    HIP_TRY(hipMemcpyAsync(s.umi, b->umi, n * 8, hipMemcpyHostToDevice, im->s_copy));
    HIP_TRY(hipMemcpyAsync(s.cig_off, b->cig_off, (n + 1) * 4, hipMemcpyHostToDevice, im->s_copy));
    if (n_cig) HIP_TRY(hipMemcpyAsync(s.cigar, b->cigar + c_lo, (size_t)n_cig * 4, hipMemcpyHostToDevice, im->s_copy));
    if (seq) {
        HIP_TRY(hipMemcpyAsync(s.seq_off, b->seq_off, (n + 1) * 4, hipMemcpyHostToDevice, im->s_copy));
        if (n_seq) HIP_TRY(hipMemcpyAsync(s.seq, b->seq + s_lo, n_seq, hipMemcpyHostToDevice, im->s_copy));
        if (with_qual && n_seq) HIP_TRY(hipMemcpyAsync(s.qual, qual, 2 * (size_t)n_seq, hipMemcpyHostToDevice, im->s_copy));
    }
    HIP_TRY(hipStreamSynchronize(im->s_copy));                 // caller may reuse its arrays now
    im->st.ms_h2d += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    im->st.algo_bytes_join += join_bytes(n, n_cig, n_seq);
    d.pos = s.pos; d.flag = s.flag; d.mapq = s.mapq; d.cell = s.cell; d.umi = s.umi;
    d.cig_off = s.cig_off; d.cigar = s.cigar - c_lo; d.seq_off = s.seq_off; d.seq = s.seq - s_lo;   // rebased, never read below *_lo
    if (with_qual) d.qual = s.qual - 2 * (size_t)s_lo;
    im->queue.push_back(d); im->queued_reads += b->n_reads;
    return launch_queue(im, slot_idx);                         // the kernel overlaps the caller's next decode + copy
}

// ---- host ingest: one decoded chunk = one staging slot, shared by every pipeline of the handle (which has at least one) ----
// the next staging slot, grown to `bytes`, once every launch that still reads it has been confirmed
static int stager_get(xck_engine* e) {
    EngineImpl* im = e->impls[0];                                        // (errors of the shared part are reported through it)
    HIP_TRY(hipSetDevice(im->device));
    if (!e->stager) {
        Stager* st = new Stager(); st->device = im->device; e->stager = st;
        HIP_TRY(hipStreamCreateWithFlags(&st->s_copy, hipStreamNonBlocking));
        for (auto& sl : st->slot) { HIP_TRY(hipEventCreate(&sl.t0)); HIP_TRY(hipEventCreate(&sl.copied)); }
    }
    return 0;
}
static int stager_take(xck_engine* e, size_t bytes, int* si_out) {
    EngineImpl* im = e->impls[0];
    if (int rc = stager_get(e)) return rc;
    Stager* st = e->stager;
    const int si = st->next; st->next = (st->next + 1) % 3;
    Stager::Slot& sl = st->slot[si];
    for (int k = 0; k < e->n_impl && sl.users > 0; k++)                  // launches that still read this slot: confirm them
        if (e->impls[k]->inflight_shared == si) { int rc = complete_pending(e->impls[k]); if (rc) return rc; }
    if (sl.users != 0) { e->err = "internal: staging slot still in use"; return XCK_E_STATE; }
    if (sl.timed) { float ms = 0; if (hipEventElapsedTime(&ms, sl.t0, sl.copied) == hipSuccess) im->st.ms_h2d += ms; sl.timed = false; }
    if (int rc = grow_device(im, (void**)&sl.buf, &sl.cap, bytes, bytes / 4 + (1 << 20))) return rc;
    *si_out = si;
    return 0;
}
// The batches of the chunk in staging slot si -> every pipeline's queue and one fused launch per pipeline (and the opt-in summary
// passes behind it, launch_queue).  dev(): a column pointer of a batch -> its place in the slot; sizes(i): the batch's CIGAR words
// and sequence bytes (xck_stats.algo_bytes_join).
// qual: the chunk's quality column (same addressing as the batches' column pointers, indexed by 2 * seq_off + query offset), for the
// pipelines with a base-quality floor; null on a handle without one.
template <class Dev, class Sizes>
static int push_staged(xck_engine* e, int si, const xck_batch* batches, int n, Dev dev, Sizes sizes, const uint8_t* qual = nullptr) {
    Stager::Slot& sl = e->stager->slot[si];
    for (int k = 0; k < e->n_impl; k++) {
        EngineImpl* im = e->impls[k];
        if (im->finished) { e->err = "push after finish (call xck_reset)"; return XCK_E_STATE; }
        int rc = launch_queue(im, -1); if (rc) return rc;                 // earlier device-resident pushes keep their order
        HIP_TRY(hipStreamWaitEvent(im->s_comp, sl.copied, 0));
        const bool seq = im->mode == XCK_MODE_BAF;
        for (int i = 0; i < n; i++) {
            const xck_batch* b = &batches[i];
            BatchDesc d;
            const BatchFate fate = describe_batch(im, b, COLS_BLOCK, d);
            if (fate == BATCH_ERROR) return im->batch_rc;
            if (fate == BATCH_SKIP) continue;
            d.pos = (const int32_t*)dev(b->pos); d.flag = (const uint16_t*)dev(b->flag); d.mapq = (const uint8_t*)dev(b->mapq);
            d.cell = (const int32_t*)dev(b->cell); d.umi = (const uint64_t*)dev(b->umi);
            d.cig_off = (const uint32_t*)dev(b->cig_off); d.cigar = (const uint32_t*)dev(b->cigar);
            if (seq) { d.seq_off = (const uint32_t*)dev(b->seq_off); d.seq = (const uint8_t*)dev(b->seq); }
            if (seq && im->min_baseq > 0) {
                if (!qual) { e->err = "internal: a chunk without qualities on a pipeline with a base-quality floor"; return XCK_E_STATE; }
                d.qual = (const uint8_t*)dev(qual);
            }
            size_t n_cig = 0, n_seq = 0; sizes(i, seq, &n_cig, &n_seq);
            im->st.algo_bytes_join += join_bytes((size_t)b->n_reads, n_cig, n_seq);
            im->queue.push_back(d); im->queued_reads += b->n_reads;
            if ((int)im->queue.size() >= MAX_FUSE) { rc = launch_queue(im, -1, si); if (rc) return rc; }
        }
        rc = launch_queue(im, -1, si); if (rc) return rc;                  // one fused launch per chunk and pipeline
    }
    return XCK_OK;
}

// ---- device-names mode (intern_dev.h): the handle's table lives with the staging, its kernels run on the copy stream ----
static int names_table(xck_engine* e) {
    if (e->dnames) return 0;
    const Knobs& k = e->knobs;
    e->dnames = dev_intern_create(e->impls[0]->device, (size_t)std::max(64ll, k.gpu_names_slots0), (size_t)std::max(1024ll, k.gpu_names_arena0), k.names_hash_bits, k.debug_timing);
    return 0;
}
// what a reserve or a launch of the table answered -> the ingest's error
static int names_error(xck_engine* e, int rc) {
    if (rc == XCK_E_NOMEM) e->err = "out of device memory for the read-name table (XCK_GPU_NAMES)";
    else if (rc) e->err = "device error in the read-name table (XCK_GPU_NAMES)";
    return rc;
}
// ... what its kernels flagged, once the copy stream was waited for behind them
static int names_flags(xck_engine* e) {
    const uint32_t fl = dev_intern_synced(e->dnames);
    if (fl & DI_F_FULL) { e->err = "the read-name table on the device ran out of room (XCK_GPU_NAMES)"; return XCK_E_DEVICE; }
    if (fl & DI_F_CAPACITY) { e->err = "too many distinct non-ACGT keys for the key width"; return XCK_E_CAPACITY; }
    return 0;
}
int engine_names_clear(xck_engine* e, bool zero_stats) {
    if (!e->names_mode || !e->dnames || e->n_impl <= 0) return 0;
    if (int rc = stager_get(e)) return rc;
    if (int rc = dev_intern_clear(e->dnames, e->stager->s_copy)) return names_error(e, rc);
    if (zero_stats) dev_intern_zero_stats(e->dnames);
    return 0;
}
int engine_names_check(xck_engine* e) {
    if (!e->names_mode || !e->dnames || !e->stager) return 0;
    EngineImpl* im = e->impls[0];
    HIP_TRY(hipSetDevice(im->device));
    HIP_TRY(hipStreamSynchronize(e->stager->s_copy));
    return names_flags(e);
}
void engine_names_stats(const xck_engine* e, int64_t* interned, int64_t* distinct) {
    *interned = 0; *distinct = 0;
    if (e->dnames) dev_intern_stats(e->dnames, interned, distinct);
}
void engine_names_report(xck_engine* e) {                                // XCK_DEBUG_TIMING, at xck_destroy
    const DevIntern* t = e->dnames;
    if (!t || !t->d_ctl) return;
    int64_t lk = 0, di = 0; dev_intern_stats(t, &lk, &di);
    fprintf(stderr, "[xck] read names on the device: %lld looked up, %lld distinct | table %zu slots, arena %.1f MB (%.1f MB used), grown %d times | intern kernels %.1f ms (those a wait followed)\n",
            (long long)lk, (long long)di, t->n_slots, t->cap_words * 4e-6, t->exact_words * 4e-6, t->growths, t->kernel_ms);
}

// a chunk the host decoded: ONE H2D copy of its block into the slot
int engine_push_block(xck_engine* e, const void* host_base, size_t bytes, const xck_batch* batches, int n, void** fence, const NameTrailer* names, const uint8_t* qual) {
    int si = 0;
    if (int rc = stager_take(e, bytes, &si)) return rc;
    EngineImpl* im = e->impls[0];
    Stager* st = e->stager; Stager::Slot& sl = st->slot[si];
    if (!*fence) { hipEvent_t ev; HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); *fence = (void*)ev; }
    if (names && names->n_out) {                                         // (before the copy is queued: growing the table waits for the stream)
        if (names->items_off + names->n_out * sizeof(DiItem) > bytes || names->bytes_off + names->n_bytes > bytes) { e->err = "internal: name trailer outside its block"; return XCK_E_ARG; }
        if (int rc = names_table(e)) return rc;
        if (int rc = dev_intern_reserve(e->dnames, st->s_copy, names->n_out, names->n_bytes)) return names_error(e, rc);
    }
    HIP_TRY(hipEventRecord(sl.t0, st->s_copy));
    HIP_TRY(hipMemcpyAsync(sl.buf, host_base, bytes, hipMemcpyHostToDevice, st->s_copy));
    if (names && names->n_out) {
        // the keys of the chunk's names, into the staged umi column (soa_layout: at the block's start), before `copied`
        if (int rc = dev_intern_launch_items(e->dnames, st->s_copy, (const DiItem*)(sl.buf + names->items_off), (const uint8_t*)(sl.buf + names->bytes_off), names->n_bytes,
                                             (uint64_t*)sl.buf, names->n_out, e->dec.umi_bits, intern_id_limit(e->dec.umi_bits))) return names_error(e, rc);
    }
    HIP_TRY(hipEventRecord(sl.copied, st->s_copy));
    HIP_TRY(hipEventRecord((hipEvent_t)*fence, st->s_copy));
    sl.timed = true;
    const char* hb = (const char*)host_base;
    return push_staged(e, si, batches, n, [&](const void* hp) { return (void*)(sl.buf + ((const char*)hp - hb)); },   // a column's place in the staged copy
                       [&](int i, bool seq, size_t* n_cig, size_t* n_seq) { const xck_batch* b = &batches[i]; const size_t nr = (size_t)b->n_reads;
                                                                              *n_cig = b->cig_off[nr] - b->cig_off[0]; *n_seq = seq ? b->seq_off[nr] - b->seq_off[0] : 0; }, qual);
}

// A chunk the device inflated and walked (csrc/parse_dev.hip): no copy - the parse kernel writes the chunk's SoA block straight into the
// slot, in the place of the H2D copy (same stream, same event), and the batches follow as above.  The kernel's flags are waited for
// before anything is queued: 1 = it met a record it leaves to the host (nothing was queued; the caller takes the host path).
int engine_push_parsed(xck_engine* e, const GpuInflateSlot* gs, size_t n_blocks, size_t max_rec, size_t n_out, size_t n_cig, size_t n_seq, int32_t sample, const DpBatch* dbs, int n, size_t chunk_bytes) {
    const DecodeCfg& dc = e->dec;
    const SoaLayout lay = soa_layout(n_out + 1, n_cig + 1, dc.want_seq ? n_seq + 1 : 1);
    const bool with_qual = dc.want_qual && dc.want_seq;                  // the quality region: behind the layout's total (parse_dev.h soa_qual_bytes)
    int si = 0;
    if (int rc = stager_take(e, lay.total + (with_qual ? soa_qual_bytes(n_seq + 1) : 0), &si)) return rc;
    EngineImpl* im = e->impls[0];                                        // (HIP_TRY reports through it)
    Stager* st = e->stager; Stager::Slot& sl = st->slot[si];
    if (!st->d_bc && !dc.bc_slots.empty()) {                             // the barcode table, as it is (same hash, same probe order on the device)
        static_assert(sizeof(DpBcSlot) == sizeof(DecodeCfg::BcSlot) && offsetof(DpBcSlot, key) == offsetof(DecodeCfg::BcSlot, key), "the device reads the host's slots");
        HIP_TRY(hipMalloc(&st->d_bc, dc.bc_slots.size() * sizeof(DpBcSlot)));
        HIP_TRY(hipMemcpy(st->d_bc, dc.bc_slots.data(), dc.bc_slots.size() * sizeof(DpBcSlot), hipMemcpyHostToDevice));
    }
    DpParseCfg pc; memset(&pc, 0, sizeof pc);
    pc.bc = (const DpBcSlot*)st->d_bc; pc.bc_mask = dc.bc_mask; pc.use_barcodes = dc.use_barcodes; pc.want_seq = dc.want_seq; pc.umi_bits = dc.umi_bits; pc.sample = sample;
    memcpy(pc.cell_tag, dc.cell_tag, 2); memcpy(pc.umi_tag, dc.umi_tag, 2);
    pc.want_qual = with_qual ? 1 : 0;
    pc.filter_on = dc.filter_on ? 1 : 0; memcpy(pc.filter_tag, dc.filter_tag, 2); pc.filter_mask = dc.filter_mask; pc.filter_value = dc.filter_value;   // (the kernel counts what it filters in the chunk's head record: Pusher::run)
    const bool names = e->names_mode && n_out > 0;
    pc.names = e->names_mode ? 1 : 0;
    if (names) {                                                         // room for the chunk's names: a kept record has 36 bytes besides its name
        if (int rc = names_table(e)) return rc;
        const size_t name_bytes = std::min<size_t>(n_out * 254, chunk_bytes > n_out * 36 ? chunk_bytes - n_out * 36 : 0);
        if (int rc = dev_intern_reserve(e->dnames, st->s_copy, n_out, name_bytes)) return names_error(e, rc);
    }
    HIP_TRY(hipEventRecord(sl.t0, st->s_copy));
    // (a launch that fails - dev_parse_launch has taken the error - wrote nothing into the slot: the chunk takes the host path, whose
    // copy of the chunk's bytes reports a device that is gone)
    if (dev_parse_launch(st->s_copy, gs, n_blocks, max_rec, pc, (uint8_t*)sl.buf, n_out, n_cig, n_seq) != 0) return 1;
    // (the read names' keys behind the parse, same stream: the umi column is final before `copied`)
    if (names) { if (int rc = dev_intern_launch_recs(e->dnames, st->s_copy, gs, n_blocks, max_rec, (uint64_t*)(sl.buf + lay.o_umi), n_out, dc.umi_bits, intern_id_limit(dc.umi_bits))) return names_error(e, rc); }
    HIP_TRY(hipEventRecord(sl.copied, st->s_copy));
    HIP_TRY(hipEventSynchronize(sl.copied));
    if (names) { if (int rc = names_flags(e)) return rc; }
    if (gs->h_head->parse_flags) return 1;
    std::vector<xck_batch> bts((size_t)n);                               // (column pointers: already the slot's)
    for (int i = 0; i < n; i++) {
        xck_batch& bt = bts[(size_t)i]; const DpBatch& pb = dbs[i]; memset(&bt, 0, sizeof bt);
        bt.contig = pb.contig; bt.n_reads = (int32_t)(pb.r1 - pb.r0); bt.ordinal_base = pb.ordinal_base;
        bt.umi = (const uint64_t*)(sl.buf + lay.o_umi) + pb.r0; bt.pos = (const int32_t*)(sl.buf + lay.o_pos) + pb.r0; bt.cell = (const int32_t*)(sl.buf + lay.o_cell) + pb.r0;
        bt.cig_off = (const uint32_t*)(sl.buf + lay.o_cgo) + pb.r0; bt.cigar = (const uint32_t*)(sl.buf + lay.o_cig);
        bt.flag = (const uint16_t*)(sl.buf + lay.o_flag) + pb.r0; bt.mapq = (const uint8_t*)(sl.buf + lay.o_mapq) + pb.r0;
        if (dc.want_seq) { bt.seq_off = (const uint32_t*)(sl.buf + lay.o_sqo) + pb.r0; bt.seq = (const uint8_t*)(sl.buf + lay.o_seq); }
    }
    return push_staged(e, si, bts.data(), n, [](const void* p) { return (void*)p; },
                       [&](int i, bool seq, size_t* c, size_t* q) { *c = dbs[i].n_cig; *q = seq ? dbs[i].n_seq : 0; }, with_qual ? (const uint8_t*)(sl.buf + lay.total) : nullptr);
}

void engine_release_staging(xck_engine* e) {
    Stager* st = e->stager;
    if (!st) return;
    hipSetDevice(st->device);
    if (st->s_copy) hipStreamSynchronize(st->s_copy);
    for (auto& sl : st->slot) { if (sl.buf) hipFree(sl.buf); if (sl.t0) hipEventDestroy(sl.t0); if (sl.copied) hipEventDestroy(sl.copied); }
    if (st->d_bc) hipFree(st->d_bc);
    if (e->dnames) { if (e->knobs.debug_timing) engine_names_report(e); dev_intern_destroy(e->dnames); e->dnames = nullptr; }
    if (st->s_copy) hipStreamDestroy(st->s_copy);
    delete st; e->stager = nullptr;
}

void fence_wait(void* f) { if (f) hipEventSynchronize((hipEvent_t)f); }
void fence_destroy(void* f) { if (f) hipEventDestroy((hipEvent_t)f); }

int engine_flush(EngineImpl* im) {
    HIP_TRY(hipSetDevice(im->device));
    int rc = launch_queue(im, -1); if (rc) return rc;
    return complete_pending(im);
}

int engine_reset(EngineImpl* im) {
    HIP_TRY(hipSetDevice(im->device));
    int rc = launch_queue(im, -1); if (rc) return rc;
    rc = complete_pending(im); if (rc) return rc;
    if (im->copy_pending) { HIP_TRY(hipStreamSynchronize(im->s_copy)); im->copy_pending = false; }
    HIP_TRY(hipMemsetAsync(im->d_ctl, 0, CTL_WORDS * sizeof(unsigned long long), im->s_comp));
    rc = summaries_reset(im); if (rc) return rc;
    rc = molecule_stats_reset(im); if (rc) return rc;
    rc = unique_feature_reset(im); if (rc) return rc;
    rc = umi_collapse_reset(im); if (rc) return rc;
    im->n_not_joined = 0;
    HIP_TRY(hipStreamSynchronize(im->s_comp));
    im->cursor = 0; im->ncursor = 0; im->finished = false; im->fold_failed = false; im->mol_valid = false; im->sc_valid = false;
    for (int i = 0; i < CTL_WORDS; i++) im->h_ctl[i] = 0;
    for (int sh = 0; sh < NSHARD; sh++) { im->cur[sh] = 0; im->ncur[sh] = 0; }
    int kb = im->key_bits, ub = im->ubits;
    memset(&im->st, 0, sizeof im->st);
    im->st.key_bits = kb; im->st.umi_bits = ub; im->n_join_launches = 0;
    return 0;
}

// the join's pair counters (xck_get_baseq_stats): the control words of the last confirmed launch, summed over the shards
int engine_baseq_stats(EngineImpl* im, xck_baseq_stats* out) {
    if (const int rc = engine_flush(im)) return rc;
    out->min_baseq = im->min_baseq;
    for (int sh = 0; sh < NSHARD; sh++) { out->pairs_with_base += (int64_t)im->h_ctl[ctl_bq_base(sh)]; out->pairs_masked += (int64_t)im->h_ctl[ctl_bq_masked(sh)]; }
    return 0;
}

int engine_device(const xck_engine* e) { return e->n_impl > 0 && e->impls[0] ? e->impls[0]->device : -1; }

int engine_stats(const EngineImpl* im, xck_stats* out) {
    *out = im->st; out->key_bits = im->key_bits; out->umi_bits = im->ubits;
    out->n_join_launches = im->n_join_launches;
    out->fold_path = im->fold_path; out->fold_fallbacks = im->fold_fallbacks; out->pileup_sort_path = im->pileup_sort_path; out->fold_refinements = im->fold_refinements;
    out->pileup_sort2_path = im->pileup_sort2_path; out->gpu_inflate_chunks = (int32_t)std::min<int64_t>(im->eng->gpu_inflate_chunks.load(), INT32_MAX);
    return 0;
}

int engine_numa_node(const xck_engine* e) {
    const EngineImpl* im = e && e->n_impl > 0 ? e->impls[0] : nullptr;
    if (!im) return -1;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, im->device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char* p = bus; *p; p++) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');
    char path[160]; snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE* f = fopen(path, "r"); if (!f) return -1;
    int node = -1; if (fscanf(f, "%d", &node) != 1) node = -1; fclose(f);
    return node;
}

int engine_create(const xck_config* cfg, xck_engine* e, EngineImpl** out) {
    EngineImpl* im = new EngineImpl();
    im->eng = e; *out = im;
    im->mode = cfg->mode; im->device = cfg->device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { e->err = "no HIP device available (the engine has no CPU fallback)"; return XCK_E_DEVICE; }
    if (cfg->device < 0 || cfg->device >= ndev) { e->err = "device ordinal out of range"; return XCK_E_ARG; }
    HIP_TRY(hipSetDevice(im->device));
    // filters (double-typed thresholds become exact integer thresholds: x < v  <=>  x < ceil(v) for integer x)
    im->rf.min_mapq = (int32_t)std::min(256.0, std::max(0.0, std::ceil(cfg->min_mapq)));
    im->rf.min_len = cfg->min_len;
    im->rf.incl_flag = cfg->incl_flag; im->rf.excl_flag = cfg->excl_flag; im->rf.no_orphan = cfg->no_orphan;
    im->rf.frac_mode = (cfg->min_include > 0.0 && cfg->min_include < 1.0) ? 1 : 0;
    im->rf.min_inc_frac = cfg->min_include;
    im->rf.min_inc_len = cfg->min_include <= 0.0 ? 0 : (int32_t)std::min(2147483647.0, std::ceil(cfg->min_include));
    im->sf.min_count = cfg->min_count <= 0.0 ? 0 : (int32_t)std::min(2147483647.0, std::ceil(cfg->min_count));
    im->sf.min_maf = cfg->min_maf;
    im->no_dup_hap = cfg->no_dup_hap;
    im->min_baseq = im->mode == XCK_MODE_BAF ? cfg->min_baseq : 0;       // (xck_create: checked, the knob folded in; the basefc half of a fused handle has none)
    im->n_cells = cfg->n_cells; im->n_regions = cfg->n_regions;
    { KeyBits kb = key_layout(cfg); im->key_bits = kb.key_bits; im->ubits = kb.ubits; im->cbits = kb.cbits; im->rbits = kb.rbits; }
    im->st.key_bits = im->key_bits; im->st.umi_bits = im->ubits;
    im->max_batch_reads = cfg->max_batch_reads > 0 ? cfg->max_batch_reads : (int64_t)1 << 21;
    int rc = build_tables(im, cfg); if (rc) return rc;
    rc = finish_init(im); if (rc) return rc;
    HIP_TRY(hipStreamCreateWithFlags(&im->s_copy, hipStreamNonBlocking));
    { int lo = 0, hi = 0;                                   // numerically lowest value = highest priority
      HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
      HIP_TRY(hipStreamCreateWithPriority(&im->s_comp, hipStreamNonBlocking, (cfg->flags & XCK_F_LOW_PRIORITY) ? lo : hi)); }
    HIP_TRY(hipEventCreate(&im->ev0)); HIP_TRY(hipEventCreate(&im->ev1));
    HIP_TRY(hipEventCreate(&im->ev_res)); HIP_TRY(hipEventCreate(&im->ev_c0)); HIP_TRY(hipEventCreate(&im->ev_c1));
    rc = dev_zeroed(im, (void**)&im->d_ctl, CTL_WORDS * sizeof(unsigned long long)); if (rc) return rc;
    HIP_TRY(hipHostMalloc((void**)&im->h_ctl, CTL_WORDS * sizeof(unsigned long long), hipHostMallocMapped));
    memset(im->h_ctl, 0, CTL_WORDS * sizeof(unsigned long long));
    HIP_TRY(hipHostGetDevicePointer((void**)&im->d_hctl, im->h_ctl, 0));
    rc = ensure_hits(im, (size_t)e->knobs.hit_cap0); if (rc) return rc;   // (XCK_HIT_CAP0: test knob)
    if ((cfg->flags & XCK_F_UMI_CONSENSUS) && im->mode == XCK_MODE_BAF) { rc = molecule_stats_init(im); if (rc) return rc; }
    if ((cfg->flags & XCK_F_UNIQUE_FEATURE) && im->mode == XCK_MODE_BASEFC) { rc = unique_feature_init(im, cfg); if (rc) return rc; }
    im->umi_collapse = (cfg->flags & XCK_F_UMI_COLLAPSE) && im->mode == XCK_MODE_BASEFC;
    return summaries_init(im, cfg->flags);
}

void engine_destroy(EngineImpl* im) {
    if (!im) return;
    hipSetDevice(im->device);
    if (im->s_comp) hipStreamSynchronize(im->s_comp);
    void* ptrs[] = { im->d_reg_s0, im->d_reg_e0, im->d_reg_row, im->d_reg_pmax, im->d_snp_p0, im->d_snp_win,
                     im->d_csr_off, im->d_csr_reg, im->d_snp_info, im->d_tally, im->d_keys, im->d_vals, im->d_nkeys, im->d_nvals, im->d_ctl, im->d_meta, im->d_fate, im->d_cell, im->d_cmat, im->d_feat, im->d_fmat, im->d_kept, im->d_mol, im->d_uf_rank, im->d_uf_span,
                     im->d_csr_alt, im->d_rf, im->d_cm, im->d_sc_perm, im->ws1.base, im->ws2.base };
    for (void* p : ptrs) if (p) hipFree(p);
    for (auto& s : im->slot) { void* q[] = { s.pos, s.flag, s.mapq, s.cell, s.umi, s.cig_off, s.cigar, s.seq_off, s.seq, s.qual }; for (void* p : q) if (p) hipFree(p); }
    for (int m = 0; m < 4; m++) if (im->h_res[m]) hipHostFree(im->h_res[m]);
    coo_call_free(im->sc); coo_call_free(im->gc);
    base_tally_free(im);
    if (im->h_ctl) hipHostFree(im->h_ctl);
    if (im->ev0) hipEventDestroy(im->ev0);
    if (im->ev1) hipEventDestroy(im->ev1);
    if (im->ev_res) hipEventDestroy(im->ev_res);
    if (im->ev_c0) hipEventDestroy(im->ev_c0);
    if (im->ev_c1) hipEventDestroy(im->ev_c1);
    if (im->ev_f1) hipEventDestroy(im->ev_f1);
    if (im->ev_f2) hipEventDestroy(im->ev_f2);
    for (hipEvent_t ev : { im->ev_r0, im->ev_r1, im->ev_r2, im->ev_r3, im->ev_m0, im->ev_m1 }) if (ev) hipEventDestroy(ev);
    if (im->s_copy) hipStreamDestroy(im->s_copy);
    if (im->s_comp) hipStreamDestroy(im->s_comp);
    delete im;
}

void* pinned_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) return p;
    return nullptr;
}
void pinned_free(void* p) { if (p) hipHostFree(p); }

}  // namespace xck
