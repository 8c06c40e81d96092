// intern_dev.hip - the device intern table's kernels and its host side (see intern_dev.h).
//
//   k_intern_recs   one lane per record of a chunk the device walked (the grid of k_parse): the record's read name -> its key, into
//                   the umi column of the chunk's SoA block.  Runs behind k_parse on the same stream.
//   k_intern_items  one lane per kept record of a chunk the host parsed: the names the parse tasks packed behind the SoA block.
//   k_di_rehash     one lane per slot of the old table: its word goes into the table of twice the size (growth).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include "intern_dev.h"
#include "parse_dev.h"

namespace xck {

__global__ __launch_bounds__(64) void k_intern_recs(const uint8_t* __restrict__ u, const DpRec* __restrict__ rec, const DpCnt* __restrict__ cnt, const DpBase* __restrict__ base,
                                                    DiView v, uint64_t* __restrict__ umi, uint32_t n_out_total) {
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const DpCnt c = cnt[b]; const DpBase bs = base[b];
    const uint32_t r0 = blockIdx.y * 64u;
    if (r0 >= c.n_rec) return;                                             // (the whole wave)
    const uint32_t ri = r0 + (uint32_t)lane;
    const bool have = ri < c.n_rec;
    const DpRec rr = have ? rec[c.rec_at + ri] : DpRec{0, DP_DROPPED, 0, 0};
    const size_t o = (size_t)bs.out + rr.slot;
    const bool kept = have && rr.slot != DP_DROPPED && o < n_out_total;
    const uint8_t* r = u + rr.off;
    const uint32_t l_name = kept ? r[8] : 0u;                              // (the walk checked that the name lies inside the record)
    const uint64_t key = di_key_wave(v, r + 32, l_name ? l_name - 1 : 0u, kept, lane);
    if (kept) umi[o] = key;
}

__global__ __launch_bounds__(64) void k_intern_items(const DiItem* __restrict__ items, const uint8_t* __restrict__ bytes, uint32_t n_bytes, DiView v, uint64_t* __restrict__ umi, uint32_t n_out) {
    const int lane = (int)threadIdx.x;
    const uint32_t o = blockIdx.x * 64u + (uint32_t)lane;
    const DiItem it = o < n_out ? items[o] : DiItem{0, 0};
    const bool want = it.len != 0 && (uint64_t)it.off + it.len <= n_bytes;
    const uint64_t key = di_key_wave(v, bytes + (want ? it.off : 0u), want ? it.len : 0u, want, lane);
    if (want) umi[o] = key;
}

__global__ __launch_bounds__(256) void k_di_rehash(const unsigned long long* __restrict__ old, uint64_t n_old, DiView nv) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_old) return;
    const unsigned long long w = old[i];
    if (w == 0) return;
    const uint32_t at = (uint32_t)w, n = (uint32_t)(w >> 32) & 0xffu;
    if ((uint64_t)at + di_entry_words(n) > nv.arena_cap) return;
    uint64_t pos = (dp_hash_bytes((const uint8_t*)(nv.arena + at + 1), n) & nv.hash_keep) & nv.mask;   // (the arena was copied on this stream before this kernel)
    for (uint64_t steps = 0; steps <= nv.mask; steps++) {
        if (atomicCAS(nv.slots + pos, 0ull, w) == 0ull) return;           // all entries are distinct: the first empty slot
        pos = (pos + 1) & nv.mask;
    }
    atomicOr(&nv.ctl->flags, DI_F_FULL);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static inline bool ok(hipError_t e) { if (e != hipSuccess) { (void)hipGetLastError(); return false; } return true; }

DevIntern* dev_intern_create(int device, size_t slots0, size_t arena0_bytes, int hash_bits, bool timing) {
    DevIntern* t = new DevIntern();
    t->device = device; t->timing = timing;
    size_t s = 64; while (s < slots0) s <<= 1;
    t->slots0 = s; t->arena0 = std::max<size_t>(arena0_bytes, 1024) / 4;
    t->hash_keep = hash_bits > 0 && hash_bits < 64 ? (1ull << hash_bits) - 1 : ~0ull;
    return t;
}

void dev_intern_destroy(DevIntern* t) {
    if (!t) return;
    if (t->device >= 0 && hipSetDevice(t->device) == hipSuccess) {
        if (t->d_slots) (void)hipFree(t->d_slots);
        if (t->d_arena) (void)hipFree(t->d_arena);
        if (t->d_ctl) (void)hipFree(t->d_ctl);
        if (t->h_ctl) (void)hipHostFree(t->h_ctl);
        if (t->h_init) (void)hipHostFree(t->h_init);
        if (t->ev0) (void)hipEventDestroy(t->ev0);
        if (t->ev1) (void)hipEventDestroy(t->ev1);
    }
    delete t;
}

static int di_first_alloc(DevIntern* t, hipStream_t stream) {
    if (!ok(hipSetDevice(t->device))) return XCK_E_DEVICE;
    if (!ok(hipMalloc((void**)&t->d_ctl, sizeof(DiCtl))) || !ok(hipHostMalloc((void**)&t->h_ctl, sizeof(DiCtl))) || !ok(hipHostMalloc((void**)&t->h_init, sizeof(DiCtl)))) return XCK_E_NOMEM;
    if (!ok(hipMalloc((void**)&t->d_slots, t->slots0 * 8))) return XCK_E_NOMEM;
    t->n_slots = t->slots0;
    if (!ok(hipMalloc((void**)&t->d_arena, t->arena0 * 4))) return XCK_E_NOMEM;
    t->cap_words = t->arena0;
    if (t->timing && (!ok(hipEventCreate(&t->ev0)) || !ok(hipEventCreate(&t->ev1)))) return XCK_E_DEVICE;
    memset(t->h_init, 0, sizeof(DiCtl)); t->h_init->arena_words = 1;
    *t->h_ctl = *t->h_init;
    if (!ok(hipMemsetAsync(t->d_slots, 0, t->n_slots * 8, stream)) || !ok(hipMemcpyAsync(t->d_ctl, t->h_init, sizeof(DiCtl), hipMemcpyHostToDevice, stream))) return XCK_E_DEVICE;
    return 0;
}

DiView dev_intern_view(const DevIntern* t, int umi_bits, uint64_t id_limit) {
    DiView v; memset(&v, 0, sizeof v);
    v.slots = t->d_slots; v.mask = t->n_slots - 1; v.arena = t->d_arena; v.arena_cap = (uint32_t)std::min<size_t>(t->cap_words, 0xffffffffu); v.ctl = t->d_ctl;
    v.hash_keep = t->hash_keep; v.id_limit = std::min<uint64_t>(id_limit, 0xffffffffull); v.umi_bits = umi_bits;
    return v;
}

static void di_close_timing(DevIntern* t) {
    if (!t->ev_open) return;
    float ms = 0; if (hipEventElapsedTime(&ms, t->ev0, t->ev1) == hipSuccess) t->kernel_ms += ms; else (void)hipGetLastError();
    t->ev_open = false;
}

uint32_t dev_intern_synced(DevIntern* t) {
    if (!t->h_ctl) return 0;
    di_close_timing(t);
    t->exact_entries = t->h_ctl->n_entries; t->exact_words = t->h_ctl->arena_words; t->exact_ids = t->h_ctl->next_id;
    t->pend_names = 0; t->pend_words = 0;
    return t->h_ctl->flags;
}

// the words n names of `bytes` bytes can take: an id each, and up to 3 bytes of padding each
static inline uint64_t di_words_bound(size_t n, size_t bytes) { return (uint64_t)n + ((uint64_t)bytes + 3 * (uint64_t)n) / 4; }

static int di_grow(DevIntern* t, hipStream_t stream, uint64_t need_entries, uint64_t need_words) {
    size_t ns = t->n_slots; while ((uint64_t)ns < need_entries * 2) ns <<= 1;
    size_t nw = t->cap_words; while ((uint64_t)nw < need_words) nw <<= 1;
    if (nw > 0xffffffffull) return XCK_E_NOMEM;                            // (a slot word holds 32 bits of arena offset)
    unsigned long long* old_slots = nullptr; uint32_t* old_arena = nullptr;
    if (nw != t->cap_words) {
        uint32_t* a = nullptr;
        if (!ok(hipMalloc((void**)&a, nw * 4))) return XCK_E_NOMEM;
        if (!ok(hipMemcpyAsync(a, t->d_arena, (size_t)t->exact_words * 4, hipMemcpyDeviceToDevice, stream))) { (void)hipFree(a); return XCK_E_DEVICE; }
        old_arena = t->d_arena; t->d_arena = a; t->cap_words = nw;
    }
    if (ns != t->n_slots) {
        unsigned long long* s = nullptr;
        if (!ok(hipMalloc((void**)&s, ns * 8))) { if (old_arena) { (void)hipStreamSynchronize(stream); (void)hipFree(old_arena); } return XCK_E_NOMEM; }
        const size_t n_old = t->n_slots;
        old_slots = t->d_slots; t->d_slots = s; t->n_slots = ns;
        const DiView nv = dev_intern_view(t, 64, ~0ull);
        if (!ok(hipMemsetAsync(s, 0, ns * 8, stream))) return XCK_E_DEVICE;
        hipLaunchKernelGGL(k_di_rehash, dim3((unsigned)((n_old + 255) / 256)), dim3(256), 0, stream, (const unsigned long long*)old_slots, (uint64_t)n_old, nv);
        if (!ok(hipGetLastError())) return XCK_E_DEVICE;
    }
    t->growths++;
    // the old buffers go once the stream has passed them
    if (!ok(hipStreamSynchronize(stream))) return XCK_E_DEVICE;
    if (old_slots) (void)hipFree(old_slots);
    if (old_arena) (void)hipFree(old_arena);
    return 0;
}

int dev_intern_reserve(DevIntern* t, hipStream_t stream, size_t n, size_t bytes) {
    if (!t->d_ctl) { if (int rc = di_first_alloc(t, stream)) return rc; }
    const uint64_t add_w = di_words_bound(n, bytes);
    auto fits = [&] { return (t->exact_entries + t->pend_names + n) * 2 <= (uint64_t)t->n_slots && t->exact_words + t->pend_words + add_w <= (uint64_t)t->cap_words; };
    if (!fits()) {
        if (!ok(hipSetDevice(t->device)) || !ok(hipStreamSynchronize(stream))) return XCK_E_DEVICE;   // the exact counters instead of the bound
        dev_intern_synced(t);
        if (!fits()) { if (int rc = di_grow(t, stream, t->exact_entries + n, t->exact_words + add_w)) return rc; }
    }
    t->pend_names += n; t->pend_words += add_w;
    return 0;
}

static int di_after_launch(DevIntern* t, hipStream_t stream) {
    if (!ok(hipGetLastError())) return XCK_E_DEVICE;
    if (t->timing && !t->ev_open) { if (ok(hipEventRecord(t->ev1, stream))) t->ev_open = true; }
    return ok(hipMemcpyAsync(t->h_ctl, t->d_ctl, sizeof(DiCtl), hipMemcpyDeviceToHost, stream)) ? 0 : XCK_E_DEVICE;
}
static void di_before_launch(DevIntern* t, hipStream_t stream) {
    // (one pair of events: a launch whose predecessor's time was not read yet - no wait in between - goes untimed)
    if (t->timing && !t->ev_open) (void)ok(hipEventRecord(t->ev0, stream));
}

int dev_intern_launch_items(DevIntern* t, hipStream_t stream, const DiItem* items, const uint8_t* bytes, size_t n_bytes, uint64_t* umi, size_t n_out, int umi_bits, uint64_t id_limit) {
    if (n_out == 0) return 0;
    if (n_out > 0xffffffffull || n_bytes > 0xffffffffull) return XCK_E_ARG;
    di_before_launch(t, stream);
    hipLaunchKernelGGL(k_intern_items, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, stream, items, bytes, (uint32_t)n_bytes, dev_intern_view(t, umi_bits, id_limit), umi, (uint32_t)n_out);
    return di_after_launch(t, stream);
}

int dev_intern_launch_recs(DevIntern* t, hipStream_t stream, const GpuInflateSlot* s, size_t n_blocks, size_t max_rec, uint64_t* umi, size_t n_out, int umi_bits, uint64_t id_limit) {
    if (n_blocks == 0 || n_out == 0) return 0;
    const unsigned rounds = (unsigned)std::min<size_t>(std::max<size_t>((max_rec + 63) / 64, 1), 65535);   // (as dev_parse_launch)
    di_before_launch(t, stream);
    hipLaunchKernelGGL(k_intern_recs, dim3((unsigned)n_blocks, rounds), dim3(64), 0, stream, (const uint8_t*)s->d_out, (const DpRec*)s->d_rec, (const DpCnt*)s->d_cnt, (const DpBase*)s->d_base,
                       dev_intern_view(t, umi_bits, id_limit), umi, (uint32_t)n_out);
    return di_after_launch(t, stream);
}

int dev_intern_clear(DevIntern* t, hipStream_t stream) {
    if (!t->d_ctl) return 0;
    if (!ok(hipSetDevice(t->device)) || !ok(hipStreamSynchronize(stream))) return XCK_E_DEVICE;
    dev_intern_synced(t);
    t->base_lookups += t->h_ctl->n_lookups; t->base_entries += t->h_ctl->n_entries;
    *t->h_ctl = *t->h_init;
    t->exact_entries = 0; t->exact_words = 1; t->exact_ids = 0;
    if (!ok(hipMemsetAsync(t->d_slots, 0, t->n_slots * 8, stream)) || !ok(hipMemcpyAsync(t->d_ctl, t->h_init, sizeof(DiCtl), hipMemcpyHostToDevice, stream))) return XCK_E_DEVICE;
    return 0;
}

void dev_intern_stats(const DevIntern* t, int64_t* lookups, int64_t* distinct) {
    *lookups = (int64_t)(t->base_lookups + (t->h_ctl ? t->h_ctl->n_lookups : 0));
    *distinct = (int64_t)(t->base_entries + (t->h_ctl ? t->h_ctl->n_entries : 0));
}
void dev_intern_zero_stats(DevIntern* t) {
    // (what the live table holds stays counted: xck_reset clears the table as well)
    t->base_lookups = 0; t->base_entries = 0;
}

}  // namespace xck
