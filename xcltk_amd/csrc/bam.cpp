// bam.cpp - host ingest: multithreaded BGZF inflate + BAM record parse into pinned SoA batches.
//
// Replaces pysam.AlignmentFile / fetch() of the reference (xcltk/rdr/fc/core.py:73-76,
// xcltk/utils/sam.py:85-118): instead of one indexed fetch per region / SNP (every read
// overlapping k features is decompressed k times) the file is decoded ONCE,
// in file order, and handed to the GPU as structure-of-arrays batches (include/xck.h xck_batch).
//
// Written from the SAM/BAM specification (SAMv1 section 4); htslib is not available here.
// Pipeline per chunk of BGZF blocks:  inflate (parallel over blocks) -> record walk (serial,
// touches 24 B per record) -> field/tag parse into SoA (parallel over records).  The inflate of
// chunk i+1 runs while chunk i is walked and parsed.
//
// This unit is the READER: xck_bam with its chunk ring, the scanner and the index ranges, the GPU share of the inflate and the device
// walk / parse fallbacks, ChunkJob / Pusher, the coordinator's stages, the NUMA binding and the C entry points.  The work on one chunk
// that knows nothing of a reader (inflate, walk, parse, layout, keys) is bam_records.cpp; the types both share are bam_decode.h.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <stdexcept>
#include "bam_decode.h"

namespace xck {

// ---------------------------------------------------------------------------------------------
// small utilities
// ---------------------------------------------------------------------------------------------
static thread_local std::string t_err;
void set_thread_error(const std::string& s) { t_err = s; }
const char* get_thread_error() { return t_err.c_str(); }

int default_threads() {
    static const int cached = [] {
        long n = (long)std::thread::hardware_concurrency(); if (n <= 0) n = 4;
        cpu_set_t set; CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof set, &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0 && c < n) n = c; }
        long long quota = -1, period = 100000;
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {                                  // cgroup v2: "<quota|max> <period>"
            char q[32] = {0}; if (fscanf(f, "%31s %lld", q, &period) >= 1 && strcmp(q, "max") != 0) quota = atoll(q); fclose(f);
        } else if (FILE* f1 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {              // cgroup v1
            if (fscanf(f1, "%lld", &quota) != 1) quota = -1; fclose(f1);
            if (FILE* f2 = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (fscanf(f2, "%lld", &period) != 1) period = 100000; fclose(f2); }
        }
        // Behind a CPU-time quota smaller than the CPUs the scheduler may use (a GPU box: 256 hardware threads, 16 CPUs' worth of
        // time), 1.5 threads per quota CPU keep the quota spent while the coordinator, the scanner and the GPU runtime's own
        // threads take their turns: fused ingest 36 -> 40-42 M reads/s at 24 threads, no further gain at 32
        // (profiles/r02_b_ingest_thread_scaling_100m.log, r02_d_ingest_thread_scaling_500m.log).
        if (quota > 0 && period > 0) { const long c = (long)((quota + period - 1) / period); if (c > 0 && c < n) n = std::min(n, c + c / 2); }
        if (const char* e = getenv("XCK_THREADS")) { const int v = atoi(e); if (v > 0) n = v; }
        return (int)std::max(1l, n);
    }();
    return cached;
}

}  // namespace xck

// sequential reader used only for the header
struct SeqReader {
    xck_bam* b; uint64_t coff = 0; std::vector<uint8_t> buf; size_t pos = 0; uint64_t blk_coff = 0; size_t blk_start = 0; std::string err;
    bool fill(size_t need) {
        while (buf.size() - pos < need) {
            BlockRef br;
            if (!bgzf_peek(b->map, b->fsize, coff, &br, &err)) { if (err.empty()) err = "unexpected end of file in BAM header"; return false; }
            size_t old = buf.size();
            buf.resize(old + br.isize);
            if (!bgzf_inflate(b->map, br, buf.data() + old, false, &err)) { if (err.empty()) err = "inflate init failed"; return false; }
            blk_coff = coff; blk_start = old; coff += br.clen;
        }
        return true;
    }
};

// A multi-BAM run (one file per cell, hundreds of files) opens and closes a reader per file.  The big buffers of a reader -
// pinned SoA arrays (hipHostMalloc pins page by page), the two inflate buffers, the record index, the thread pool - cost
// ~30 ms to set up, twice the decode time of a 500 k-read file: closed readers park them here for the next open.
struct BamScratch {
    HostSoA soa[N_JOB]; std::vector<uint8_t> ubuf[N_CHUNK];
    Pool* pool = nullptr; int n_threads = 0;
};
static std::mutex g_scratch_mu;
static std::vector<BamScratch*> g_scratch;                            // at most 4 parked sets; kept until the process ends
// ... and so are the GPU-inflate slots of closed readers: a slot is ~70 MB of pinned + 50 MB of device memory, and pinning it anew
// for every file cost 0.2 s per open (a 20 M-record file decodes in 0.45 s)
static std::vector<GpuInflateSlot*> g_gpu_slots;                      // at most 16; kept until the process ends
// ... and the contig tables of the device walk (device_parse_now), by content: at most 8, kept until the process ends
struct CmShared { int device; bool tend; std::vector<int32_t> host; void* d; };
static std::vector<CmShared> g_cm_shared;
static GpuInflateSlot* take_gpu_slot(int device, int free_cus, bool verbose) {
    { std::lock_guard<std::mutex> lk(g_scratch_mu);
      for (size_t i = 0; i < g_gpu_slots.size(); i++) if (g_gpu_slots[i]->device == device) { GpuInflateSlot* s = g_gpu_slots[i]; g_gpu_slots.erase(g_gpu_slots.begin() + (long)i); return s; } }
    return gpu_inflate_slot_create(device, free_cus, verbose);
}
// (parked slots are destroyed at exit, BEFORE the HIP runtime's own teardown - this handler is registered after the runtime came up, so
// it runs first: streams with a CU mask and mapped host blocks left alive made the process crash at exit under rocprofv3)
static void destroy_parked_gpu_slots() {
    std::vector<GpuInflateSlot*> v;
    { std::lock_guard<std::mutex> lk(g_scratch_mu); v.swap(g_gpu_slots); }
    for (GpuInflateSlot* s : v) gpu_inflate_slot_destroy(s);
}
static void park_gpu_slot(GpuInflateSlot* s) {
    if (!s) return;
    gpu_inflate_slot_wait(s);                                          // nothing in flight on a parked slot
    { std::lock_guard<std::mutex> lk(g_scratch_mu);
      static bool at_exit = false;
      if (!at_exit) { at_exit = true; std::atexit(destroy_parked_gpu_slots); }
      if (g_gpu_slots.size() < 16) { g_gpu_slots.push_back(s); return; } }
    gpu_inflate_slot_destroy(s);
}

extern "C" {

static int bam_open_impl(const char* path, int n_threads, xck_bam** out, char* err, size_t errlen) {
    auto fail = [&](const std::string& m, xck_bam* b) { if (err && errlen) { snprintf(err, errlen, "%s: %s", path ? path : "(null)", m.c_str()); } set_thread_error(m); if (b) xck_bam_close(b); return XCK_E_IO; };
    if (!path || !out) return fail("null argument", nullptr);
    xck_bam* b = new xck_bam();
    b->path = path;
    b->fd = open(path, O_RDONLY);
    if (b->fd < 0) return fail("cannot open file", b);
    struct stat st; if (fstat(b->fd, &st) != 0 || st.st_size < 28) return fail("cannot stat file / file too small", b);
    b->fsize = (uint64_t)st.st_size;
    void* m = mmap(nullptr, b->fsize, PROT_READ, MAP_PRIVATE, b->fd, 0);
    if (m == MAP_FAILED) return fail("mmap failed", b);
    b->map = (const uint8_t*)m;
    madvise(m, b->fsize, MADV_SEQUENTIAL);
    // the reference lets pysam detect SAM / BAM / CRAM; this decoder reads BAM only and says so up front
    if (memcmp(b->map, "CRAM", 4) == 0) return fail("CRAM input is not supported: this decoder reads BAM only (samtools view -b)", b);
    if (b->map[0] == '@' && b->map[3] == '\t') return fail("SAM text input is not supported: this decoder reads BAM only (samtools view -b)", b);
    SeqReader r; r.b = b;
    if (!r.fill(12)) return fail(r.err, b);
    if (memcmp(r.buf.data(), "BAM\1", 4) != 0) return fail("not a BAM file (bad magic)", b);
    uint32_t l_text = le32(r.buf.data() + 4);
    if (!r.fill(12 + (size_t)l_text)) return fail(r.err, b);
    r.pos = 8 + l_text;
    uint32_t n_ref = le32(r.buf.data() + r.pos); r.pos += 4;
    for (uint32_t i = 0; i < n_ref; i++) {
        if (!r.fill(4)) return fail(r.err, b);
        uint32_t l_name = le32(r.buf.data() + r.pos); r.pos += 4;
        if (!r.fill((size_t)l_name + 4)) return fail(r.err, b);
        b->ref_names.emplace_back((const char*)r.buf.data() + r.pos, l_name ? l_name - 1 : 0); r.pos += l_name;
        b->ref_lens.push_back((int64_t)le32(r.buf.data() + r.pos)); r.pos += 4;
    }
    // first alignment record: inside the last inflated block at offset (r.pos - r.blk_start), or at the next block
    if (r.pos == r.buf.size()) { b->next_coff = r.coff; b->first_skip = 0; }
    else { b->next_coff = r.blk_coff; b->first_skip = (uint32_t)(r.pos - r.blk_start); }
    b->threads_auto = n_threads <= 0;
    if (n_threads <= 0) n_threads = default_threads();
    b->n_threads = n_threads;
    b->tm.t_open = std::chrono::steady_clock::now();
    { BamScratch* sc = nullptr;
      { std::lock_guard<std::mutex> lk(g_scratch_mu); if (!g_scratch.empty()) { sc = g_scratch.back(); g_scratch.pop_back(); } }
      if (sc) {
          for (int i = 0; i < N_JOB; i++) b->jobs[i].soa = sc->soa[i];
          for (int i = 0; i < N_CHUNK; i++) b->ch[i].ubuf.swap(sc->ubuf[i]);
          if (sc->pool && sc->n_threads == n_threads) b->pool = sc->pool; else delete sc->pool;
          delete sc;
      } }
    if (!b->pool) b->pool = new Pool(n_threads);
    if (const char* cb = getenv("XCK_CHUNK_BYTES")) { long long v = atoll(cb); if (v >= 1024) b->chunk_target = (size_t)v; }   // tests: force many chunks
    *out = b;
    return XCK_OK;
}

void xck_bam_close(xck_bam* b) {
    if (!b) return;
    if (b->pusher) { b->pusher->wait_idle(); b->tm.push += b->pusher->push_ns; b->tm.wait_parse += b->pusher->parse_wait_ns; b->tm.push_parsed += b->pusher->push_parsed_ns; delete b->pusher; b->pusher = nullptr; }
    for (auto& j : b->jobs) j.tg.wait();
    delete b->scanner; b->scanner = nullptr;
    for (auto& c : b->ch) c.tg.wait();
    // no H2D copy may still read a block that is parked or freed - and a parked block must not keep its event: the copy stream
    // it was recorded on dies with the engine's staging, and waiting on such an event later fails (hipErrorStreamCaptureUnsupported
    // on ROCm 7: the next reader's first launch check then reported that stale error; tests/test_gpu_random_e2e.py seed 9)
    for (auto& j : b->jobs) if (j.soa.fence) { fence_wait(j.soa.fence); fence_destroy(j.soa.fence); j.soa.fence = nullptr; }
    if (getenv("XCK_DEBUG_TIMING") && b->gi.chunks)
        fprintf(stderr, "[xck] ingest %s: GPU share of the inflate: %llu chunks / %llu blocks on the device (%llu of them finished by the host), gather %.0f ms of pool time, coordinator waited %.0f ms%s\n",
                b->path.c_str(), (unsigned long long)b->gi.chunks, (unsigned long long)b->gi.blocks, (unsigned long long)b->gi.left_blocks, b->gi.copy_ns * 1e-6, b->gi.wait_ns * 1e-6,
                b->gi.broken ? "; the device path was given up (runtime error / no memory)" : "");
    if (getenv("XCK_DEBUG_TIMING") && (b->dstat[DS_PARSE_CHUNKS].load() || b->dstat[DS_PARSE_FALLBACKS].load()))
        fprintf(stderr, "[xck] ingest %s: device walk + parse: %lld chunks, %lld fallbacks to the host path%s | coordinator ms: summaries -> batches %.0f | push thread ms: parse kernel + launches %.0f | fallback copies ms: %.0f\n",
                b->path.c_str(), (long long)b->dstat[DS_PARSE_CHUNKS].load(), (long long)b->dstat[DS_PARSE_FALLBACKS].load(), b->gi.parse_off.load() ? " (given up for this file)" : "",
                b->tm.dp_layout * 1e-6, b->tm.push_parsed * 1e-6, b->tm.dp_copy_out * 1e-6);
    for (auto& gs : b->gi.slot) { park_gpu_slot(gs); gs = nullptr; }
    for (auto& gs : b->gi.free_slots) park_gpu_slot(gs);
    b->gi.free_slots.clear();
    for (void* p : b->gi.d_cm_all) dev_parse_free(b->gi.device, p);   // (after the slots were waited for: no walk reads the tables any more)
    b->gi.d_cm_all.clear();
    if (b->numa_bound && b->pool) b->pool->set_affinity(b->old_affinity);   // a parked pool goes back to the full mask
    if (getenv("XCK_DEBUG_TIMING") && b->tm.chunks) {
        const DecodeTimes& t = b->tm; const double ms = 1e-6;
        fprintf(stderr, "[xck] ingest %s: %lld records, %llu chunks (%llu stitched serially), %.0f ms since open, %d threads | pool CPU ms: inflate %.0f walk %.0f parse %.0f | "
                        "coordinator ms: wait_inflate %.0f schedule %.0f stitch %.0f layout %.0f wait_parse %.0f wait_push %.0f | push thread ms: %.0f\n",
                b->path.c_str(), (long long)b->n_records, (unsigned long long)t.chunks, (unsigned long long)t.slow_chunks, ns_since(t.t_open) * ms, b->n_threads,
                t.inflate.load() * ms, t.walk.load() * ms, t.parse.load() * ms,
                t.wait_inflate * ms, t.sched * ms, t.stitch * ms, t.layout * ms, t.wait_parse * ms, t.wait_push * ms, t.push * ms);
    }
    { BamScratch* sc = new BamScratch();
      for (int i = 0; i < N_JOB; i++) { sc->soa[i] = b->jobs[i].soa; b->jobs[i].soa = HostSoA(); }
      for (int i = 0; i < N_CHUNK; i++) sc->ubuf[i].swap(b->ch[i].ubuf);
      sc->pool = b->pool; sc->n_threads = b->n_threads; b->pool = nullptr;
      std::lock_guard<std::mutex> lk(g_scratch_mu);
      if (g_scratch.size() < 4) g_scratch.push_back(sc);
      else { delete sc->pool; for (auto& so : sc->soa) soa_free(so); delete sc; } }
    if (b->map) munmap((void*)b->map, b->fsize);
    if (b->fd >= 0) close(b->fd);
    delete b;
}

int xck_bam_n_refs(const xck_bam* b) { return b ? (int)b->ref_names.size() : 0; }
const char* xck_bam_ref_name(const xck_bam* b, int tid) { return (b && tid >= 0 && tid < (int)b->ref_names.size()) ? b->ref_names[tid].c_str() : nullptr; }
int64_t xck_bam_ref_len(const xck_bam* b, int tid) { return (b && tid >= 0 && tid < (int)b->ref_lens.size()) ? b->ref_lens[tid] : -1; }

}  // extern "C"

// ---- .bai (SAMv1 section 5.2): only what contig sharding needs: where each reference starts / ends ----
static void load_index(xck_bam* b) {
    if (b->idx_loaded) return;
    b->idx_loaded = true;
    std::string cand[2] = { b->path + ".bai", b->path.size() > 4 ? b->path.substr(0, b->path.size() - 4) + ".bai" : std::string() };
    std::vector<uint8_t> d;
    for (auto& fn : cand) { if (fn.empty()) continue; FILE* fp = fopen(fn.c_str(), "rb"); if (!fp) continue;
        fseek(fp, 0, SEEK_END); long n = ftell(fp); fseek(fp, 0, SEEK_SET); d.resize(n > 0 ? (size_t)n : 0);
        size_t got = d.empty() ? 0 : fread(d.data(), 1, d.size(), fp); fclose(fp); if (got == d.size() && got >= 8) break; d.clear(); }
    if (d.size() < 8 || memcmp(d.data(), "BAI\1", 4) != 0) return;
    size_t o = 4; auto need = [&](size_t k) { return o + k <= d.size(); };
    uint32_t n_ref = le32(d.data() + o); o += 4;
    if (n_ref != b->ref_names.size()) return;
    b->idx_beg.assign(n_ref, ~0ull); b->idx_end.assign(n_ref, 0); b->idx_mapped.assign(n_ref, 0); b->idx_unmapped.assign(n_ref, 0); b->idx_lin.assign(n_ref, {});
    auto le64 = [&](size_t at) { return (uint64_t)le32(d.data() + at) | ((uint64_t)le32(d.data() + at + 4) << 32); };
    for (uint32_t r = 0; r < n_ref; r++) {
        if (!need(4)) return;
        uint32_t n_bin = le32(d.data() + o); o += 4;
        for (uint32_t k = 0; k < n_bin; k++) {
            if (!need(8)) return;
            uint32_t bin = le32(d.data() + o), n_chunk = le32(d.data() + o + 4); o += 8;
            if (!need((size_t)n_chunk * 16)) return;
            if (bin == 37450 && n_chunk == 2) { b->idx_mapped[r] = (int64_t)le64(o + 16); b->idx_unmapped[r] = (int64_t)le64(o + 24); }
            else for (uint32_t c = 0; c < n_chunk; c++) { uint64_t cb = le64(o + c * 16), ce = le64(o + c * 16 + 8);
                if (cb < b->idx_beg[r]) b->idx_beg[r] = cb; if (ce > b->idx_end[r]) b->idx_end[r] = ce; }
            o += (size_t)n_chunk * 16;
        }
        if (!need(4)) return;
        uint32_t n_intv = le32(d.data() + o); o += 4;
        if (!need((size_t)n_intv * 8)) return;
        b->idx_lin[r].resize(n_intv);
        for (uint32_t w = 0; w < n_intv; w++) b->idx_lin[r][w] = le64(o + (size_t)w * 8);
        o += (size_t)n_intv * 8;
    }
    b->idx_ok = true;
}

// restrict decoding to the references wanted by tid_to_contig (virtual-offset ranges from the index)
static void set_ranges(xck_bam* b, const xck_ingest_opts* o) {
    b->ranges_set = true; b->use_ranges = false;
    if (!o->use_index || !o->tid_to_contig) return;
    load_index(b);
    if (!b->idx_ok) return;                                            // no usable index: decode everything
    const bool has_win = o->struct_size >= offsetof(xck_ingest_opts, tid_end) + sizeof(void*) && (o->tid_beg || o->tid_end);
    struct Rg { uint64_t first, second; int32_t tid; bool operator<(const Rg& o) const { return first != o.first ? first < o.first : second < o.second; } };
    std::vector<Rg> rg;
    for (size_t t = 0; t < b->ref_names.size(); t++) {
        if (!(o->tid_to_contig[t] >= 0 && b->idx_beg[t] != ~0ull && b->idx_end[t] > b->idx_beg[t])) continue;
        uint64_t beg = b->idx_beg[t];
        if (has_win && o->tid_beg && o->tid_beg[t] > 0) {                  // first record overlapping the window's first position: linear index
            const std::vector<uint64_t>& lin = b->idx_lin[t];
            const size_t w = (size_t)o->tid_beg[t] >> 14;
            if (w >= lin.size()) continue;                               // nothing overlaps that far right
            if (lin[w] > beg) beg = lin[w];
        }
        if (beg < b->idx_end[t]) rg.push_back({beg, b->idx_end[t], (int32_t)t});
    }
    std::sort(rg.begin(), rg.end());
    b->per_tid_ranges = has_win;
    for (auto& x : rg) { if (!has_win && !b->ranges.empty() && (x.first >> 16) <= (b->ranges.back().second >> 16) + 1) b->ranges.back().second = std::max(b->ranges.back().second, x.second);
                         else { b->ranges.push_back({x.first, x.second}); b->range_tid.push_back(x.tid); } }
    b->use_ranges = true;
}

// position windows: the reference whose index range the chunk belongs to (ContigMap::only_tid), -1 without windows
static int32_t range_only_tid(const xck_bam* b, const Chunk& c) { return b->per_tid_ranges && (size_t)c.range_id < b->range_tid.size() ? b->range_tid[c.range_id] : -1; }

// XCK_GPU_PARSE: do the device chunks scheduled now get the walk behind their inflate?  begin_decode said whether the reader may at all
// (gi.parse); a record limit keeps this call's chunks on the host path; the contig tables the walk applies go to device memory here.
static bool device_parse_now(xck_bam* b, const ContigMap& cm, const xck_ingest_opts* o) {
    GpuShare& gi = b->gi;
    if (!gi.on || !gi.parse || gi.broken || gi.parse_off.load() || o->max_records > 0 || cm.n_refs <= 0 || !cm.t2c) return false;
    const size_t n = (size_t)cm.n_refs; const bool tend = cm.t_end != nullptr;
    const bool same = gi.d_cm && gi.cm_tend == tend && gi.cm_host.size() == n * (tend ? 2 : 1) && memcmp(gi.cm_host.data(), cm.t2c, n * 4) == 0 &&
                      (!tend || memcmp(gi.cm_host.data() + n, cm.t_end, n * 4) == 0);
    if (!same) {
        gi.cm_host.assign(cm.t2c, cm.t2c + n); if (tend) gi.cm_host.insert(gi.cm_host.end(), cm.t_end, cm.t_end + n);
        // the per-cell BAMs of a well-based run bring the same tables file after file: a table uploaded once is shared by the readers
        // that follow (an allocation and, at close, a free - which waits for the whole device, the next files' inflate kernels
        // included - per file otherwise).  The few shared tables live until the process ends, so no walk in flight outlives one.
        void* d = nullptr; bool shared = false;
        { std::lock_guard<std::mutex> lk(g_scratch_mu);
          for (const CmShared& c : g_cm_shared) if (c.device == gi.device && c.tend == tend && c.host == gi.cm_host) { d = c.d; shared = true; break; } }
        if (!d) {
            d = dev_parse_upload(gi.device, cm.t2c, n * 4, cm.t_end, tend ? n * 4 : 0);
            if (!d) { gi.parse_off = true; gi.cm_host.clear(); return false; }
            std::lock_guard<std::mutex> lk(g_scratch_mu);
            if (g_cm_shared.size() < 8) { g_cm_shared.push_back(CmShared{gi.device, tend, gi.cm_host, d}); shared = true; }
        }
        gi.d_cm = (int32_t*)d; gi.cm_tend = tend; if (!shared) gi.d_cm_all.push_back(d);
    }
    return true;
}
// a device-walked chunk goes down the host path after all: counted, and after four in a row the reader stops asking for the walk (a
// file of unaligned blocks, or of UMIs the device cannot code, must not pay for both paths chunk after chunk)
static void count_parse_fallback(xck_bam* b) {
    b->dstat[DS_PARSE_FALLBACKS].fetch_add(1, std::memory_order_relaxed);
    if (b->gi.fb_row.fetch_add(1) + 1 >= 4) b->gi.parse_off.store(true);
}
// ... for which its inflated bytes, so far in HBM only, are copied to the slot's host block: from there on it is a device chunk of old
static bool fallback_copy_out(xck_bam* b, Chunk& c, GpuInflateSlot* gs) {
    const auto t0 = std::chrono::steady_clock::now();
    const bool ok = dev_parse_copy_out(gs, c.usize) == 0;
    __atomic_fetch_add(&b->tm.dp_copy_out, ns_since(t0), __ATOMIC_RELAXED);
    c.dparse = false; c.dp_ok = false;
    return ok;
}

// take the next plan from the scanner and start inflating it into c (asynchronous); the contig map lets the walk tasks
// prepare the output layout of their own records
static void schedule_chunk(xck_bam* b, Chunk& c, int ci, bool verify_crc, bool crc_on_device, const ContigMap cm_in, bool want_seq, bool dev_parse) {
    c.blocks.clear(); c.usize = 0; c.valid = false; c.failed = false; c.err.clear(); c.new_range = false; c.first_skip = 0; c.gpu = false; c.gpu_rc = 0; c.launched = 0; c.stage2 = false;
    c.dparse = false; c.dp_ok = false;
    if (b->scan_end) return;
    ChunkPlan pl = b->scanner->next();
    if (pl.end) { b->scan_end = true; return; }
    c.blocks.swap(pl.blocks); c.new_range = pl.new_range; c.first_skip = pl.first_skip; c.range_id = pl.range_id;
    if (pl.failed) { c.failed = true; c.err = pl.err; }
    if (c.blocks.empty() && !c.failed) return;
    c.valid = true; c.usize = pl.usize;
    const size_t usz = pl.usize;
    const size_t nb = c.blocks.size();
    // ---- does this chunk go to the GPU?  (a fixed share of the chunks; small chunks - the tail of a range - stay on the host)
    GpuShare& gi = b->gi;
    GpuInflateSlot* gs = nullptr;
    if (gi.on && !gi.broken && (!verify_crc || crc_on_device) && nb >= 64 && usz < (size_t(1) << 31)) {
        bool want;
        if (gi.pct > 0) { gi.acc += gi.pct; want = gi.acc >= 100; if (want) gi.acc -= 100; }       // a fixed share
        else {                                                            // auto: keep gi.depth chunks on the device, the pool takes the rest -
            int busy = 0;                                                 // the shares then follow the two sides' speeds on this file and this box
            int held = 0;
            for (int k = 0; k < b->n_ring; k++) { if (!gi.slot[k]) continue; held++; if (gi.inflight[k] && !gpu_inflate_slot_done(gi.slot[k])) busy++; }
            // ... but never the chunk the coordinator needs next or the one after (a device chunk takes tens of milliseconds, the pool
            // delivers in three: the first chunks of a file, and whatever follows a drained ring, stay on the host)
            want = busy < gi.depth && held < gi.max_held && (b->n_sched >= 2 || b->prefetching);   // (reading ahead: nobody waits for these chunks yet)
        }
        if (want) {
            size_t tin = 0; for (size_t i = 0; i < nb; i++) tin += ((size_t)c.blocks[i].data_len + 3) & ~size_t(3);
            if (!gi.slot[ci]) {
                if (!gi.free_slots.empty()) { gi.slot[ci] = gi.free_slots.back(); gi.free_slots.pop_back(); }
                else gi.slot[ci] = take_gpu_slot(gi.device, gi.free_cus, gi.verbose && !gi.chunks);
            }
            gs = gi.slot[ci];
            if (gs && dev_parse) gs->parse = true;                          // (the slot then holds the walk's buffers too, from here on)
            if (gs && gi.inflight[ci]) { gpu_inflate_slot_wait(gs); gi.inflight[ci] = false; }   // (a chunk that was dropped unconsumed)
            if (!gs || !gpu_inflate_slot_reserve(gs, tin + 8, usz + 8, nb)) { gi.broken = true; gs = nullptr; }   // no device memory: the host does it all from here on
            else c.in_total = tin;
        }
    }
    if (gs) { c.gpu = true; c.ubase = gs->h_out; gi.inflight[ci] = true; c.dparse = dev_parse; }
    else { if (c.ubuf.size() < usz + 8) c.ubuf.resize(usz + 8); c.ubase = c.ubuf.data(); }
    const size_t per = std::max<size_t>(1, (nb + (size_t)b->n_threads * 4 - 1) / ((size_t)b->n_threads * 4));
    const size_t n_parts = (nb + per - 1) / per;
    c.parts.resize(n_parts);
    const size_t skip0 = c.first_skip;             // bytes before the first record (first chunk of the file / of an index range)
    ContigMap cm = cm_in; cm.only_tid = range_only_tid(b, c);
    if (gs) {                                       // block table: where every block's stream sits in the gathered input, where its bytes go
        size_t at = 0;
        for (size_t i = 0; i < nb; i++) {
            const BlockRef& br = c.blocks[i];                            // (crc: the footer's, the bytes bgzf_inflate checks)
            gs->h_bl[i] = DevBlock{(uint32_t)at, br.data_len, (uint32_t)br.uoff, br.isize, crc_on_device ? le32(b->map + br.coff + br.clen - 8) : 0u};
            at += ((size_t)br.data_len + 3) & ~size_t(3);
        }
        c.copy_left = (int)n_parts; gi.chunks++; gi.blocks += nb;
    }
    for (size_t pi = 0; pi < n_parts; pi++) {
        size_t i0 = pi * per, i1 = std::min(nb, i0 + per);
        WalkPart& wp = c.parts[pi];
        wp.i0 = i0; wp.i1 = i1;
        wp.u_begin = c.blocks[i0].uoff; wp.u_end = c.blocks[i1 - 1].uoff + c.blocks[i1 - 1].isize;
        wp.spec_start = wp.u_begin + (pi == 0 ? skip0 : 0); wp.stop = wp.spec_start; wp.recs.clear();
        wp.n_out = wp.n_cig = wp.n_seq = wp.n_name = 0; wp.runs.clear();
        Chunk* cp = &c; const uint8_t* map = b->map; WalkPart* wpp = &wp; DecodeTimes* tmp_ = &b->tm; std::atomic<int64_t>* ds = b->dstat;
        if (!gs) { c.tg.later([cp, map, verify_crc, wpp, tmp_, cm, want_seq, ds] { run_part(cp, map, verify_crc, wpp, tmp_, cm, want_seq, nullptr, ds); }); continue; }
        GpuShare* gip = &gi; const size_t nb_ = nb, usz_ = usz;
        // (device walk behind the inflate: the contig map as run_part applies it, its tables in device memory)
        const bool walk = c.dparse;
        const DpWalk dw{(uint32_t)skip0, DpContigMap{gi.d_cm, gi.cm_tend && gi.d_cm ? gi.d_cm + cm.n_refs : nullptr, cm.n_refs, cm.only_tid}, want_seq};
        c.tg.later([cp, map, i0, i1, gs, gip, nb_, usz_, crc_on_device, walk, dw] {
            const auto t_a = std::chrono::steady_clock::now();
            for (size_t i = i0; i < i1; i++) memcpy(gs->h_in + gs->h_bl[i].in_off, map + cp->blocks[i].coff + cp->blocks[i].data_off, cp->blocks[i].data_len);
            __atomic_fetch_add(&gip->copy_ns, ns_since(t_a), __ATOMIC_RELAXED);
            if (cp->copy_left.fetch_sub(1) == 1) {                         // the chunk's compressed bytes are gathered: hand it to the device
                const int rc = gpu_inflate_slot_launch(gs, cp->in_total, usz_, nb_, crc_on_device, walk ? &dw : nullptr);
                cp->gpu_rc = rc; cp->launched.store(1, std::memory_order_release);
            }
        });
    }
    c.tg.flush(*b->pool);
}

// ---- NUMA: the decoder stays on ONE socket ---------------------------------------------------------------------------
// A GPU box has two sockets behind a CPU-time quota; left alone, the scheduler spreads the pool over both and every chunk's
// inflated bytes, records and SoA block cross the socket link: 35 M reads/s unpinned against 40.5-41.8 M with the process held
// on either socket (24 threads, same box, same call: profiles/r02_v_numa_affinity.log).  At the first decode call the pool, the
// scanner and the calling thread (whose first touch places the inflate buffers) are bound to the CPUs of the GPU's NUMA node
// (decode-only handle: the node the caller runs on); the caller's mask is restored by xck_bam_close.  XCK_NUMA=0 turns it off.
static bool read_cpulist(const char* path, cpu_set_t* out) {
    FILE* f = fopen(path, "r"); if (!f) return false;
    char buf[4096]; const size_t n = fread(buf, 1, sizeof buf - 1, f); fclose(f); buf[n] = 0;
    CPU_ZERO(out); int any = 0;
    for (char* p = buf; *p;) {
        while (*p == ',' || *p == ' ' || *p == '\n') p++;
        if (!*p) break;
        char* q; long a = strtol(p, &q, 10); if (q == p) break; long z = a; p = q;
        if (*p == '-') { p++; z = strtol(p, &q, 10); if (q == p) break; p = q; }
        for (long c = a; c <= z && c < CPU_SETSIZE; c++) { CPU_SET((int)c, out); any = 1; }
    }
    return any != 0;
}
static int node_of_cpu(int cpu, cpu_set_t* node_set) {
    for (int node = 0; node < 64; node++) {
        char path[96]; snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
        cpu_set_t s; if (!read_cpulist(path, &s)) { if (node > 8) break; continue; }
        if (cpu >= 0 && CPU_ISSET(cpu, &s)) { *node_set = s; return node; }
    }
    return -1;
}
struct CallerBinding {
    xck_bam* b; cpu_set_t saved; bool active = false;
    explicit CallerBinding(xck_bam* b_) : b(b_) { if (b) { b->cur_binding = this; enter(); } }
    void enter() {
        if (!b || !b->numa_bound || active) return;
        if (sched_getaffinity(0, sizeof saved, &saved) != 0) return;
        if (pthread_setaffinity_np(pthread_self(), sizeof b->numa_set, &b->numa_set) == 0) active = true;
    }
    ~CallerBinding() { if (active) pthread_setaffinity_np(pthread_self(), sizeof saved, &saved); if (b) b->cur_binding = nullptr; }
};
static void bind_to_numa_node(xck_engine* e, xck_bam* b) {
    if (const char* v = getenv("XCK_NUMA")) if (atoi(v) == 0) return;
    if (!b->pool || b->n_threads < 2) return;
    cpu_set_t node_set; CPU_ZERO(&node_set);
    int node = e && e->n_impl > 0 ? xck::engine_numa_node(e) : -1;
    if (node >= 0) { char path[96]; snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node); if (!read_cpulist(path, &node_set)) node = -1; }
    if (node < 0) node = node_of_cpu(sched_getcpu(), &node_set);
    if (node < 0) return;
    cpu_set_t cur; CPU_ZERO(&cur);
    if (sched_getaffinity(0, sizeof cur, &cur) != 0) return;
    cpu_set_t both; CPU_AND(&both, &cur, &node_set);
    if (CPU_COUNT(&both) < 2 || CPU_COUNT(&both) == CPU_COUNT(&cur)) return;     // not allowed there, or there is only this node
    // a thread count that was derived from the CPUs of the WHOLE machine (no quota, two sockets) is cut to the node's CPUs
    if (b->threads_auto && b->n_threads > CPU_COUNT(&both)) { delete b->pool; b->n_threads = CPU_COUNT(&both); b->pool = new Pool(b->n_threads); }
    b->old_affinity = cur; b->numa_set = both; b->numa_bound = true;
    b->pool->set_affinity(both);
    if (b->cur_binding) b->cur_binding->enter();                     // the rest of this decode call (the scanner thread made next inherits it)
}

// ---- a decoded chunk's way out: jobs, the push thread ------------------------------------------------------------------
// the chunk at the head of the ring is consumed (or dropped): its slot, if it had one and nothing is in flight on it, serves the next device chunk
static void release_chunk(xck_bam* b, int ci) {
    GpuShare& gi = b->gi;
    if (gi.slot[ci] && !gi.inflight[ci]) { gi.free_slots.push_back(gi.slot[ci]); gi.slot[ci] = nullptr; }
}
static void advance_head(xck_bam* b, ChunkJob* hold = nullptr) {      // hold: that job's parse still reads the chunk (reap_jobs takes it back)
    if (hold) { hold->ring_idx = b->head; hold->released = false; } else release_chunk(b, b->head);
    b->head = (b->head + 1) % b->n_ring; b->n_sched--;
}
// ring chunks whose parse has ended go back to the ring (coordinator only)
static void reap_jobs(xck_bam* b) {
    for (auto& j : b->jobs) if (!j.released && j.parsed.load(std::memory_order_acquire)) { release_chunk(b, j.ring_idx); j.released = true; }
}
// The job of the chunk that is decoded now.  The push thread is never more than N_JOB - 1 jobs behind (Pusher::submit), so the slot's last
// user is done with it; should that ever fail to hold the decode ends here rather than write into a block that is still parsed into or copied.
static ChunkJob* take_job(xck_engine* e, xck_bam* b) {
    ChunkJob& j = b->jobs[b->n_jobs % N_JOB];
    reap_jobs(b);
    if (j.queued.load(std::memory_order_acquire) || !j.released) { b->err = "internal: the job slot of this chunk is still in use"; return nullptr; }
    b->n_jobs++; b->cur = &j;
    if (j.soa.fence) fence_wait(j.soa.fence);                           // the H2D copy that last read this block has completed
    j.e = e; j.flags.store(0); j.parsed.store(0); j.ring_idx = -1; j.batches.clear(); j.dev = false;
    j.b = b; j.names = e->names_mode && b->defer_parse;                          // (xck_ingest_bam on a handle in device-names mode)
    j.qual = e->dec.want_qual;
    return &j;
}
// what a chunk's parse tasks reported (flags 1 / 2: parse_record; a task that threw) -> error code and text, 0 if nothing.  Call after tg.wait().
static int parse_error(ChunkJob& j, std::string* msg) {
    int fl = j.flags.load();
    if (const int th = j.tg.take_thrown()) fl |= th == 1 ? 4 : 8;
    if (fl & 4) { *msg = "out of host memory (record parse)"; return XCK_E_NOMEM; }
    if (fl & 8) { *msg = "C++ exception in a parse task"; return XCK_E_IO; }
    if (fl & 1) { *msg = "corrupt BAM record (fields exceed block_size)"; return XCK_E_IO; }
    if (fl & 2) { *msg = "too many distinct non-ACGT keys for the key width"; return XCK_E_CAPACITY; }
    return 0;
}

static int redo_on_host(ChunkJob* j, std::string* msg);
void Pusher::run() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
        cv.wait(lk, [this] { return stop || qn > 0; });
        if (qn == 0) return;
        ChunkJob* j = q[qh];
        const bool failed = rc != 0;
        lk.unlock();
        std::string msg;
        auto t0 = std::chrono::steady_clock::now();
        int r = 0; bool host_chunk = !j->dev;
        if (j->dev && !failed) {
            // a chunk the device walked: the parse kernel writes its SoA block into the engine's staging slot and the batches follow - no
            // parse task, no copy.  A chunk that kernel flags (1) takes the host path here, late but in file order.
            xck_bam* b = j->b; GpuInflateSlot* gs = b->gi.slot[j->ring_idx];
            try { r = xck::engine_push_parsed(j->e, gs, b->ch[j->ring_idx].blocks.size(), j->lay.max_rec, j->lay.n_out, j->lay.n_cig, j->lay.n_seq, j->opts.sample, j->lay.batches.data(), (int)j->lay.batches.size(), b->ch[j->ring_idx].usize); }
            catch (const std::bad_alloc&) { r = XCK_E_NOMEM; } catch (...) { r = XCK_E_IO; }
            push_parsed_ns += ns_since(t0); push_ns += ns_since(t0);
            if (r == 1) { count_parse_fallback(b); r = redo_on_host(j, &msg); host_chunk = r == 0; }
            else if (r) msg = j->e->err;
            else {
                b->dstat[DS_PARSE_CHUNKS].fetch_add(1, std::memory_order_relaxed); b->gi.fb_row.store(0);
                // (the tag filter: what k_parse counted, read behind the event engine_push_parsed waited for; a chunk that fell back is counted by its host parse alone)
                if (j->e->dec.filter_on) b->dstat[DS_TAG_FILTERED].fetch_add((int64_t)gs->h_head->n_filtered, std::memory_order_relaxed);
            }
            t0 = std::chrono::steady_clock::now();
        }
        if (host_chunk) {
            j->tg.wait();
            parse_wait_ns += ns_since(t0);
            r = parse_error(*j, &msg);
        }
        j->parsed.store(1, std::memory_order_release);
        if (host_chunk && !failed && !r && !j->batches.empty()) {
            // the whole chunk crosses PCIe as ONE block; its batches are slices of the block (fused handles: both pipelines read the same copy)
            t0 = std::chrono::steady_clock::now();
            xck_engine* e = j->e; HostSoA& s = j->soa;
            std::vector<xck_batch> bts(j->batches.size());
            for (size_t i = 0; i < bts.size(); i++) fill_batch(s, j->batches[i], e->dec.want_seq, &bts[i]);
            const bool names = j->names && s.has_names && s.nt.n_out > 0;
            if (names && j->b) j->b->dstat[DS_NAMES_HOST_CHUNKS].fetch_add(1, std::memory_order_relaxed);
            try { r = xck::engine_push_block(e, s.base, s.used, bts.data(), (int)bts.size(), &s.fence, names ? &s.nt : nullptr, s.qual); } catch (const std::bad_alloc&) { r = XCK_E_NOMEM; } catch (...) { r = XCK_E_IO; }
            if (r) msg = e->err;
            push_ns += ns_since(t0);
        }
        j->batches.clear();                                              // (handed over, or dropped behind a failure)
        lk.lock();
        if (r && !rc) { rc = r; err = msg; }
        qh = (qh + 1) % MAXQ; qn--;
        j->queued.store(0, std::memory_order_release);
        cv.notify_all();
    }
}

// the walk tasks of a device chunk (and the inflate of what the device left of it), ahead of the later chunks' inflate tasks
static void queue_host_walk(xck_engine* e, xck_bam* b, Chunk& c, ContigMap cm, const int32_t* st) {
    Chunk* cp = &c; const uint8_t* map = b->map; DecodeTimes* tmp_ = &b->tm; const bool want_seq = e->dec.want_seq, crc = e->dec.verify_crc; std::atomic<int64_t>* ds = b->dstat;
    for (WalkPart& wp : c.parts) { WalkPart* wpp = &wp; c.tg.later([cp, map, crc, wpp, tmp_, cm, want_seq, st, ds] { run_part(cp, map, crc, wpp, tmp_, cm, want_seq, st, ds); }); }
    c.tg.flush(*b->pool, true);
}

// A device chunk whose inflate is over: whatever the device did not inflate - single blocks with a non-zero status, or the whole chunk
// after a runtime error - the pool inflates now, and every part walks its records as on the host path.  Called for the chunk the
// coordinator has reached (wait = true: for the device if need be) and, without waiting, for the chunks behind it whose device part
// has already ended - their walk is then over by the time the coordinator gets there (it used to wait ~0.5 ms per chunk for it).
static void start_stage_two(xck_engine* e, xck_bam* b, int ci, ContigMap cm, bool wait) {
    Chunk& c = b->ch[ci];
    if (!c.gpu || c.stage2 || !c.valid || c.failed || (b->skip_range >= 0 && c.range_id == b->skip_range)) return;
    GpuInflateSlot* gs = b->gi.slot[ci];
    if (!wait && !(c.launched.load(std::memory_order_acquire) && (c.gpu_rc.load() != 0 || gpu_inflate_slot_done(gs)))) return;
    if (wait) c.tg.wait();                                               // (the gather tasks: the last of them launches)
    const auto t_w = std::chrono::steady_clock::now();
    const bool dev_ok = c.gpu_rc.load() == 0 && gpu_inflate_slot_wait(gs) == 0;
    b->gi.inflight[ci] = false;
    if (wait) b->gi.wait_ns += ns_since(t_w);
    if (!dev_ok) b->gi.broken = true;                                    // the device path stays off for the rest of this reader
    else e->gpu_inflate_chunks++;
    const int32_t* st = dev_ok ? gs->h_st : nullptr;
    bool walked = false;
    if (c.dparse && dev_ok) {                                            // walked on the device: clean summaries stand in for the walk tasks
        if (gs->h_head->walk_flags == 0) walked = true;
        else { count_parse_fallback(b); if (!fallback_copy_out(b, c, gs)) { b->gi.broken = true; st = nullptr; } }   // (no bytes on the host: the pool inflates the chunk)
    }
    c.dparse = false;
    const size_t nb = c.blocks.size(); size_t left = nb;
    if (dev_ok) {
        left = 0; size_t crc_ok = 0, crc_bad = 0;
        for (size_t i = 0; i < nb; i++) { left += st[i] != 0; crc_ok += st[i] == 0 && c.blocks[i].isize; crc_bad += st[i] == INFLATE_ST_CRC; }
        b->dstat[DS_GPU_CHUNKS] += 1; b->dstat[DS_GPU_BLOCKS] += (int64_t)nb;
        if (e->dec.crc_on_device) { b->dstat[DS_CRC_DEVICE] += (int64_t)crc_ok; b->dstat[DS_CRC_MISMATCH_DEVICE] += (int64_t)crc_bad; }
    }
    b->gi.left_blocks += left; b->dstat[DS_GPU_LEFT] += (int64_t)left;
    cm.only_tid = range_only_tid(b, c);
    c.stage2 = true;
    if (walked) { c.dp_ok = true; return; }
    queue_host_walk(e, b, c, cm, st);                                    // (what the device left - a CRC mismatch included - is checked on the host as every host block is)
}

// ---- decode_next_chunk and its stages ------------------------------------------------------------------------------------
// the phases of the coordinating thread (DecodeTimes): lap() books the time since the last lap
struct PhaseClock {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(uint64_t& acc) { acc += ns_since(t); t = std::chrono::steady_clock::now(); }
};

// Stage 1, at the first call of a reader (decode or prefetch): the index ranges to read, whether the GPU takes a share of the inflate,
// the NUMA binding, the scanner thread.
static int begin_decode(xck_engine* e, xck_bam* b, const xck_ingest_opts* o, bool schedule_only) {
    if (!schedule_only && !b->started) {
        b->started = true;
        // well mode without UMIs: the key is the read name and the column is the BAM itself, so names only have to be unique within one file -
        // restart the intern table per BAM (bounded memory for 384 x 2 M reads).  (At the first DECODE call, not at xck_bam_prefetch: the file
        // before this one may still be parsing.)
        if (!e->dec.use_barcodes && !e->dec.use_umi) {
            e->intern.clear();
            // (device-names mode: the device table with it, stream-ordered on the stream its kernels run on; both kinds of decode call may start over)
            if (e->names_mode) { if (const int rc = engine_names_clear(e)) { b->err = e->err; return rc; } e->names_calls = 0; }
        }
    }
    if (b->ranges_set) return 0;
    set_ranges(b, o);
    GpuShare& gi = b->gi;
    if (!gi.tried) {                                           // GPU share of the inflate: a handle with a device, XCK_GPU_INFLATE > 0, no host-only CRC checks asked for
        gi.tried = true;
        const int dev = engine_device(e), pct = e->knobs.gpu_inflate_pct;
        // (files of a few chunks - the per-cell BAMs of a well-based run - are done before the device has returned its first chunk)
        uint64_t span = b->fsize;
        if (b->use_ranges) { span = 0; for (auto& r : b->ranges) span += (r.second >> 16) - (r.first >> 16); }
        const bool big = span >= (uint64_t)e->knobs.gpu_inflate_min_mb << 20 || schedule_only;   // (a file that is read ahead has the time a device chunk takes, whatever its size)
        if (pct != 0 && dev >= 0 && (!e->dec.verify_crc || e->dec.crc_on_device) && (big || pct > 0)) {
            gi.on = true; gi.pct = pct < 0 ? 0 : std::min(pct, 100); gi.device = dev;
            gi.depth = e->knobs.gpu_inflate_depth; gi.max_held = std::min(gi.depth + 2, 12);
            gi.free_cus = e->knobs.gpu_inflate_free_cus; gi.verbose = e->knobs.debug_timing;
            b->n_ring = std::max(N_CHUNK + 1, std::min(N_CHUNK_GPU, e->knobs.gpu_inflate_ring));
            // XCK_GPU_PARSE: walk and parse these chunks on the device too - where the key is a UMI tag (read names are interned on the
            // host) and every barcode fits a slot of the barcode table, which the kernel probes as it is
            bool fits = true; for (const std::string& bc : e->dec.barcodes) fits = fits && bc.size() <= sizeof(DecodeCfg::BcSlot::key);
            // (... or, in device-names mode, the read name: the handle's device table interns it, csrc/intern_dev.hip)
            gi.parse = e->knobs.gpu_parse && (e->dec.use_umi || e->names_mode) && fits;
        }
    }
    bind_to_numa_node(e, b);                                   // (before the scanner thread is made: it inherits the mask)
    std::vector<ScanRange> rg;
    if (b->use_ranges) for (auto& r : b->ranges) rg.push_back({r.first >> 16, (uint32_t)(r.first & 0xffff), r.second >> 16});
    else rg.push_back({b->next_coff, b->first_skip, ~0ull});
    b->scanner = new Scanner(b->map, b->fsize, b->chunk_target, rg);
    return 0;
}

// Stage 2, keep the ring full: while the head chunk is stitched and parsed the pool inflates the next ones
static void fill_ring(xck_engine* e, xck_bam* b, const ContigMap& cm, const xck_ingest_opts* o) {
    reap_jobs(b);
    // (read-name keys come from the device only for xck_ingest_bam: a reader used through xck_bam_next_batch keeps the host's table and walk)
    const bool dev_parse = (e->dec.use_umi || b->defer_parse) && device_parse_now(b, cm, o);
    // (the chunks behind `head` that a parse in flight still reads must not be scheduled over: `back` = how far the oldest of them lies behind)
    int back = 0;
    for (auto& j : b->jobs) if (!j.released) back = std::max(back, (b->head - j.ring_idx + b->n_ring) % b->n_ring);
    while (b->n_sched + back < b->n_ring && !b->scan_end) {
        const int ci = (b->head + b->n_sched) % b->n_ring;
        schedule_chunk(b, b->ch[ci], ci, e->dec.verify_crc, e->dec.crc_on_device, cm, e->dec.want_seq, dev_parse);
        if (b->scan_end) break;
        b->n_sched++;
    }
}

// the chunk's pool tasks (inflate / gather, walk) have ended; one that threw ends the stream
static int wait_chunk_tasks(xck_bam* b, Chunk& c) {
    c.tg.wait();
    const int th = c.tg.take_thrown();
    if (th) b->err = th == 1 ? "out of host memory (BGZF inflate / record walk)" : "C++ exception in a decoder task";
    return !th ? 0 : th == 1 ? XCK_E_NOMEM : XCK_E_IO;
}

// Stage 3, wait for the chunk at the head of the ring: inflated and walked (a device chunk: stage two first), cm->only_tid set for it.
// Returns 1, 0 at the end of the stream, < 0 on error, or HEAD_SKIPPED: the chunk belonged to an abandoned range and was dropped.
constexpr int HEAD_SKIPPED = 2;
static int wait_head(xck_engine* e, xck_bam* b, ContigMap* cm, PhaseClock& clk) {
    if (b->n_sched == 0) {
        if (!b->use_ranges && !b->carry.empty()) { b->err = "truncated BAM file (partial record at end of file)"; return XCK_E_IO; }
        return 0;
    }
    if (b->gi.on) for (int k = 1; k < b->n_sched; k++) start_stage_two(e, b, (b->head + k) % b->n_ring, *cm, false);   // device chunks that are back already: walk them now
    Chunk& c = b->ch[b->head];
    cm->only_tid = range_only_tid(b, c);
    if (const int rc = wait_chunk_tasks(b, c)) return rc;
    if (c.gpu && !c.stage2) {
        start_stage_two(e, b, b->head, *cm, true);
        if (const int rc = wait_chunk_tasks(b, c)) return rc;
    }
    if (b->skip_range >= 0 && c.range_id == b->skip_range && !c.failed) {   // rest of a reference whose position window is behind us
        if (c.gpu && b->gi.inflight[b->head]) { gpu_inflate_slot_wait(b->gi.slot[b->head]); b->gi.inflight[b->head] = false; }
        advance_head(b); b->carry.clear();
        return HEAD_SKIPPED;
    }
    clk.lap(b->tm.wait_inflate); b->tm.chunks++;
    if (c.failed) { b->err = c.err.empty() ? "BGZF decode error" : c.err; return XCK_E_IO; }
    return 1;
}

// no carried-over bytes, no record limit, every part's speculative walk began where the previous one ended: the parts' lists are the chunk's
static bool speculation_held(const xck_bam* b, const Chunk& c, const xck_ingest_opts* o, size_t off) {
    if (!b->carry.empty() || o->max_records > 0) return false;
    size_t at = off;
    for (size_t pi = 0; pi < c.parts.size(); pi++) {
        const WalkPart& wp = c.parts[pi];
        if (wp.spec_start != at) return false;
        at = wp.stop;
        if (pi + 1 < c.parts.size() && wp.stop != wp.u_end) return false;       // a record straddles two parts
    }
    return !(at + 4 <= c.usize && le32(c.ubase + at) < 32);                     // not a straddling tail but a damaged record: the serial walk reports it
}

// The serial stitch: the boundary record from the carry, then the parts' lists where their speculation held and a re-walk where it did
// not, cut into c.stitched (pieces of a parse task's size) and ended at the record limit; what follows the last whole record is carried.
static int stitch_serially(xck_bam* b, Chunk& c, const ContigMap& cm, const xck_ingest_opts* o, bool want_seq, size_t off, bool* hit_limit) {
    const uint8_t* u = c.ubase; const size_t usz = c.usize;
    size_t est = 1; for (const WalkPart& wp : c.parts) est += wp.recs.size();
    const size_t per = std::max<size_t>(4096, (est + (size_t)b->n_threads * 4 - 1) / ((size_t)b->n_threads * 4));
    const int64_t limit = o->max_records > 0 ? std::max<int64_t>(0, o->max_records - b->n_records) : INT64_MAX;
    int64_t n_walked = 0; int32_t cur_c = INT32_MIN;
    c.stitched.clear();
    auto add = [&](const uint8_t* r, uint32_t len) {                    // (as the walk tasks note their records: run_part)
        if (n_walked++ >= limit) return;
        if (c.stitched.empty() || c.stitched.back().recs.size() >= per) { c.stitched.emplace_back(); cur_c = INT32_MIN; }
        WalkPart& wp = c.stitched.back();
        const RecRef rr{r, len, (int32_t)le32(r), le32(r + 16), le16(r + 12)};
        const int32_t ctg = cm(rr.tid, (int32_t)le32(r + 4));
        if (ctg != cur_c) { wp.runs.push_back({(uint32_t)wp.recs.size(), ctg}); cur_c = ctg; }
        if (ctg >= 0) { wp.n_out++; wp.n_cig += rr.n_cig; if (want_seq) wp.n_seq += (rr.l_seq + 1) / 2; wp.n_name += r[8]; }
        wp.recs.push_back(rr);
    };
    c.stitch.clear();
    if (!b->carry.empty()) {
        c.stitch.swap(b->carry);
        while (c.stitch.size() < 4 && off < usz) c.stitch.push_back(u[off++]);
        if (c.stitch.size() >= 4) {
            const uint32_t bs = le32(c.stitch.data());
            const size_t need = 4 + (size_t)bs - c.stitch.size();
            if (need <= usz - off) { c.stitch.insert(c.stitch.end(), u + off, u + off + need); off += need; }
            else { c.stitch.insert(c.stitch.end(), u + off, u + usz); off = usz; b->carry.swap(c.stitch); }   // record larger than a chunk
        } else { b->carry.swap(c.stitch); }
    }
    if (!c.stitch.empty()) {
        if (c.stitch.size() < 36) { b->err = "corrupt BAM record"; return XCK_E_IO; }
        add(c.stitch.data() + 4, (uint32_t)c.stitch.size() - 4);
    }
    size_t pi = 0; bool incomplete = false;
    while (!incomplete) {
        while (pi < c.parts.size() && c.parts[pi].u_end <= off) pi++;
        if (pi == c.parts.size()) break;
        const WalkPart& wp = c.parts[pi];
        if (off == wp.spec_start) {                                     // speculation held: take the task's list
            for (const RecRef& rr : wp.recs) add(rr.p, rr.len);
            off = wp.stop;
            if (off == wp.u_end) { pi++; continue; }
        }
        while (off < wp.u_end) {                                        // serial walk (record straddles ranges / mis-speculation)
            if (off + 4 > usz) { incomplete = true; break; }
            const uint32_t bs = le32(u + off);
            if (off + 4 + (size_t)bs > usz) { incomplete = true; break; }
            if (bs < 32) { b->err = "corrupt BAM record (block_size < 32)"; return XCK_E_IO; }
            add(u + off + 4, bs);
            off += 4 + (size_t)bs;
        }
        pi++;
    }
    if (off < usz) b->carry.insert(b->carry.end(), u + off, u + usz);
    *hit_limit = n_walked > limit;
    return 0;
}

// Stage 4, stitch: -> the chunk's records as a list of pieces (its walk parts, or what the serial stitch made), the reader's carry
static int stitch_chunk(xck_bam* b, Chunk& c, const ContigMap& cm, const xck_ingest_opts* o, bool want_seq, std::vector<WalkPart>** pieces, bool* hit_limit) {
    if (c.new_range) {                                                  // start of the file's records / of an index range
        if (!b->use_ranges && b->tm.chunks > 1 && !b->carry.empty()) { b->err = "internal: carry at a range start"; return XCK_E_IO; }
        b->carry.clear();
    }
    const size_t off = c.new_range ? c.first_skip : 0;                  // bytes of the range's first block that precede its first record
    if (off > c.usize) { b->err = "corrupt BAM header offset"; return XCK_E_IO; }
    *hit_limit = false;
    if (speculation_held(b, c, o, off)) {
        const size_t stop = c.parts.back().stop;
        if (stop < c.usize) b->carry.insert(b->carry.end(), c.ubase + stop, c.ubase + c.usize);
        *pieces = &c.parts;
        return 0;
    }
    b->tm.slow_chunks++;
    *pieces = &c.stitched;
    return stitch_serially(b, c, cm, o, want_seq, off, hit_limit);
}

// (Stage 5, layout: layout_chunk, bam_records.cpp)

// position windows: the chunk's last record (its tid and pos) starts beyond its reference's window - the rest of that reference's range is dropped
static void drop_range_past_window(xck_bam* b, const Chunk& c, const ContigMap& cm, int32_t last_tid, int32_t last_pos) {
    if (!b->per_tid_ranges || !cm.t_end) return;
    if (last_tid >= 0 && last_tid < cm.n_refs && cm.t_end[last_tid] > 0 && last_pos >= cm.t_end[last_tid]) {
        b->skip_range = c.range_id; b->scanner->abandon(c.range_id);
    }
}

static void queue_parse_tasks(xck_bam* b, ChunkJob& j, const std::vector<WalkPart>& pieces, const ContigMap& cm, int32_t sample) {
    xck_engine* e = j.e; HostSoA* sp = &j.soa; std::atomic<int>* fl = &j.flags; DecodeTimes* tm = &b->tm;
    std::atomic<int64_t>* nf = &b->dstat[DS_TAG_FILTERED];
    for (const WalkPart& wp : pieces) { if (!wp.n_out) continue; const WalkPart* wpp = &wp;
        j.tg.later([tm, e, sp, sample, wpp, cm, fl, nf] { parse_part(tm, e, sp, sample, wpp, cm, fl, nf); }); }
    j.tg.flush(*b->pool, true);                                         // (ahead of the later chunks' inflate tasks)
}

// the job goes to the push thread (made at the first one); waits while Pusher::MAXQ chunks are outstanding behind this one.
// Returns the push thread's first failure so far.
static int hand_to_pusher(xck_bam* b, ChunkJob& j, PhaseClock& clk) {
    if (!b->pusher) b->pusher = new Pusher();
    const int prc = b->pusher->submit(&j);
    clk.lap(b->tm.wait_push);
    if (prc) b->err = b->pusher->err;
    return prc;
}

// Stages 4 - 6 of a chunk the device walked (c.dp_ok): its summaries -> the batch list (parse_dev.h summaries_to_batches, what
// layout_chunk makes of the walk parts), no parse tasks; the job goes to the push thread, which launches the parse kernel.
static int layout_walked_chunk(xck_bam* b, Chunk& c, ChunkJob& j, const ContigMap& cm, const xck_ingest_opts* o, PhaseClock& clk) {
    GpuInflateSlot* gs = b->gi.slot[b->head];
    if (c.new_range) b->carry.clear();                                  // (a range start under use_index: see stitch_chunk)
    summaries_to_batches(gs->h_sum, c.blocks.size(), b->n_records, (uint64_t)(uint32_t)o->sample << ORD_REC_BITS, &j.lay);
    j.dev = true; j.b = b; j.cm = cm; j.rec_before = b->n_records;
    memset(&j.opts, 0, sizeof j.opts); memcpy(&j.opts, o, std::min<size_t>(o->struct_size, sizeof j.opts));
    clk.lap(b->tm.dp_layout);
    if (j.lay.has_last) drop_range_past_window(b, c, cm, j.lay.last_tid, j.lay.last_pos);   // (the last record the walk saw)
    b->n_records += (int64_t)j.lay.n_rec;
    advance_head(b, &j);
    return hand_to_pusher(b, j, clk);
}

// Stage 6, parse: one pool task per piece, record fields -> the job's SoA block.  The coordinator waits for them here, or
// (defer_parse) hands the job to the push thread, which does; the ring chunk goes with the job until its parse has ended.
static int parse_or_defer(xck_bam* b, Chunk& c, ChunkJob& j, const std::vector<WalkPart>& pieces, int64_t n_rec, const ContigMap& cm, int32_t sample, PhaseClock& clk) {
    queue_parse_tasks(b, j, pieces, cm, sample);
    if (!b->defer_parse) {
        j.tg.wait();
        clk.lap(b->tm.wait_parse);
        if (const int rc = parse_error(j, &b->err)) return rc;
    }
    const RecRef* last = nullptr;                                       // (the record lists are read, not what the parse tasks write)
    for (size_t pi = pieces.size(); pi-- > 0 && !last;) if (!pieces[pi].recs.empty()) last = &pieces[pi].recs.back();
    if (last) drop_range_past_window(b, c, cm, last->tid, (int32_t)le32(last->p + 4));
    b->n_records += n_rec;
    advance_head(b, b->defer_parse ? &j : nullptr);
    return b->defer_parse ? hand_to_pusher(b, j, clk) : 0;
}

// The push thread's way down the host path, for a chunk whose parse kernel met a record it leaves to the host (a UMI to intern): the
// chunk's bytes come over, the pool walks its parts and parses them into the job's own SoA block, exactly as the coordinator would have
// had them do; Pusher::run then waits for the parse tasks and pushes the block.  The ring chunk is still the job's (parsed is not set).
static int redo_on_host(ChunkJob* j, std::string* msg) {
    xck_bam* b = j->b; xck_engine* e = j->e; Chunk& c = b->ch[j->ring_idx]; GpuInflateSlot* gs = b->gi.slot[j->ring_idx];
    j->dev = false;
    if (!fallback_copy_out(b, c, gs)) { *msg = "device error while copying a chunk's inflated bytes to the host"; return XCK_E_DEVICE; }
    queue_host_walk(e, b, c, j->cm, gs->h_st);
    c.tg.wait();
    if (const int th = c.tg.take_thrown()) { *msg = th == 1 ? "out of host memory (BGZF inflate / record walk)" : "C++ exception in a decoder task"; return th == 1 ? XCK_E_NOMEM : XCK_E_IO; }
    // (the device's walk ended every block at its end and no bytes were carried in, so the parts' lists are the chunk's)
    size_t at = c.parts.empty() ? 0 : c.parts[0].spec_start;
    for (const WalkPart& wp : c.parts) { if (wp.spec_start != at || wp.stop != wp.u_end) { *msg = "internal: host and device walk disagree"; return XCK_E_IO; } at = wp.stop; }
    j->batches.clear();
    const int64_t n_rec = layout_chunk(*j, c.parts, &j->opts, e->dec.want_seq, j->rec_before, msg);
    if (n_rec < 0) return (int)n_rec;
    if ((size_t)n_rec != j->lay.n_rec) { *msg = "internal: host and device walk disagree"; return XCK_E_IO; }
    queue_parse_tasks(b, *j, c.parts, j->cm, j->opts.sample);
    return 0;
}

// decode the next chunk into the SoA block of its job (b->cur) and fill the job's batch list; returns 1 (decoded: parsed in place or,
// defer_parse, parse + push in flight), 0 (end of the stream), < 0 on error; schedule_only (xck_bam_prefetch): 1 once the pool is
// inflating the first chunks
static int decode_next_chunk(xck_engine* e, xck_bam* b, const xck_ingest_opts* o, bool schedule_only = false) {
    const bool has_win = o->struct_size >= offsetof(xck_ingest_opts, tid_end) + sizeof(void*);
    ContigMap cm; cm.t2c = o->tid_to_contig; cm.n_refs = (int)b->ref_names.size(); cm.t_end = has_win ? o->tid_end : nullptr;
    if (const int rc0 = begin_decode(e, b, o, schedule_only)) return rc0;
    PhaseClock clk;
    int rc;
    do {
        clk = PhaseClock();
        fill_ring(e, b, cm, o);
        clk.lap(b->tm.sched);
        if (schedule_only) return 1;
        rc = wait_head(e, b, &cm, clk);
    } while (rc == HEAD_SKIPPED);
    if (rc <= 0) return rc;
    Chunk& c = b->ch[b->head];
    ChunkJob* j = take_job(e, b);
    if (!j) return XCK_E_IO;
    if (c.dp_ok) {
        // a chunk the device walked stays on the device unless bytes are carried into it (the chunk before ended inside a record), the caller
        // wants its batches on the host (xck_bam_next_batch) or a record limit was set meanwhile: then its bytes come over and the pool walks it
        const bool carry_in = !b->carry.empty() && !(c.new_range && b->use_ranges);
        if (!carry_in && b->defer_parse && o->max_records <= 0) {
            if ((rc = layout_walked_chunk(b, c, *j, cm, o, clk)) < 0) return rc;
            return 1;
        }
        count_parse_fallback(b);
        GpuInflateSlot* gs = b->gi.slot[b->head];
        const bool copied = fallback_copy_out(b, c, gs);
        if (!copied) b->gi.broken = true;
        queue_host_walk(e, b, c, cm, copied ? gs->h_st : nullptr);
        if ((rc = wait_chunk_tasks(b, c))) return rc;
        if (c.failed) { b->err = c.err.empty() ? "BGZF decode error" : c.err; return XCK_E_IO; }
        clk.lap(b->tm.wait_inflate);
    }
    std::vector<WalkPart>* pieces = nullptr; bool hit_limit = false;
    if ((rc = stitch_chunk(b, c, cm, o, e->dec.want_seq, &pieces, &hit_limit)) < 0) return rc;
    clk.lap(b->tm.stitch);
    const int64_t n_rec = layout_chunk(*j, *pieces, o, e->dec.want_seq, b->n_records, &b->err);
    if (n_rec < 0) return (int)n_rec;
    clk.lap(b->tm.layout);
    if ((rc = parse_or_defer(b, c, *j, *pieces, n_rec, cm, o->sample, clk)) < 0) return rc;
    if (hit_limit) { b->done = true; for (auto& cc : b->ch) cc.tg.wait(); }
    return 1;
}

extern "C" {

int xck_bam_ref_records(xck_bam* b, int tid, int64_t* n_mapped, int64_t* n_unmapped) {
    if (!b || tid < 0 || tid >= (int)b->ref_names.size()) return XCK_E_ARG;
    load_index(b);
    if (!b->idx_ok) return XCK_E_IO;
    if (n_mapped) *n_mapped = b->idx_mapped[tid];
    if (n_unmapped) *n_unmapped = b->idx_unmapped[tid];
    return XCK_OK;
}

int xck_bam_linear_index(xck_bam* b, int tid, int64_t* n, const uint64_t** voffsets) {
    if (!b || !n || !voffsets || tid < 0 || tid >= (int)b->ref_names.size()) return XCK_E_ARG;
    load_index(b);
    if (!b->idx_ok) return XCK_E_IO;
    *n = (int64_t)b->idx_lin[tid].size(); *voffsets = b->idx_lin[tid].data();
    return XCK_OK;
}

// what the reader counted since the last decode call -> the handle's xck_decode_stats (at the end of every decode call)
struct FoldDecodeStats {
    xck_engine* e; xck_bam* b;
    ~FoldDecodeStats() {
        for (int k = 0; k < DS_N; k++) {
            const int64_t v = k == DS_GPU_GIVEN_UP ? (int64_t)b->gi.broken : b->dstat[k].load();   // (given up: once per reader)
            e->dstat[k] += v - b->dstat_folded[k]; b->dstat_folded[k] = v;
        }
    }
};

// Device-names mode (XCK_GPU_NAMES): xck_ingest_bam keys read names by the handle's device table, xck_bam_next_batch by the host's - ids
// of the two do not compare, so between two clears of the table a handle serves one kind of call (1 = ingest, 2 = next_batch) only.
static int names_state_check(xck_engine* e, xck_bam* b, int kind) {
    if (!e->names_mode) return 0;
    const bool clears = !b->started && !e->dec.use_barcodes && !e->dec.use_umi;   // (begin_decode empties both tables for this reader)
    if (clears || !(e->names_calls & (3 - kind))) return 0;
    e->err = kind == 2 ? "xck_bam_next_batch after xck_ingest_bam on a handle in device-names mode (XCK_GPU_NAMES): read names are keyed by the device table there and by the host table here; call xck_reset first"
                       : "xck_ingest_bam after xck_bam_next_batch on a handle in device-names mode (XCK_GPU_NAMES): read names are keyed by the host table there and by the device table here; call xck_reset first";
    return XCK_E_STATE;
}

static int next_batch_impl(xck_engine* e, xck_bam* b, const xck_ingest_opts* o, xck_batch* out) {
    if (!e || !b || !o || !out) return XCK_E_ARG;
    CallerBinding on_node(b);
    FoldDecodeStats fold{e, b};
    b->defer_parse = false;                                            // (this interface hands out finished batches: parse in place)
    if (e->dec.want_qual) { e->err = "xck_bam_next_batch on a handle with a base-quality floor (xck_config.min_baseq / XCK_MIN_BASEQ): the batches it hands out carry no qualities; use xck_ingest_bam"; return XCK_E_STATE; }
    if (const int src = names_state_check(e, b, 2)) return src;
    while (!b->cur || b->cur->batches.empty()) {
        if (b->done) return 0;
        int rc = decode_next_chunk(e, b, o);
        if (e->names_mode) e->names_calls |= 2;
        if (rc < 0) { e->err = b->path + ": " + b->err; return rc; }
        if (rc == 0) { b->done = true; return 0; }
    }
    fill_batch(b->cur->soa, b->cur->batches.front(), e->dec.want_seq, out);
    b->cur->batches.pop_front();
    return 1;
}

// nothing of this reader is in flight any more: parse tasks ended, their chunks pushed (unless something failed), push thread idle
static int drain_ingest(xck_bam* b, int rc) {
    if (b->pusher) { const int prc = b->pusher->wait_idle(); if (rc >= 0 && prc) { b->err = b->pusher->err; rc = prc; } }
    reap_jobs(b);
    return rc;
}

static int ingest_impl(xck_engine* e, xck_bam* b, const xck_ingest_opts* o, int64_t* n_records) {
    if (!e || !b || !o) return XCK_E_ARG;
    if (e->base_tally && !e->contig_len_set) { e->err = "xck_ingest_bam: the handle keeps base tallies (XCK_F_BASE_TALLY) and has no contig lengths; call xck_set_contig_lengths first"; return XCK_E_STATE; }
    CallerBinding on_node(b);
    FoldDecodeStats fold{e, b};
    const int64_t pause = o->struct_size >= offsetof(xck_ingest_opts, pause_records) + sizeof(int64_t) ? o->pause_records : 0;
    const int64_t start = b->n_records;
    b->defer_parse = e->n_impl > 0;                                    // (a decode-only handle decodes in place and discards: host-ingest benchmarks)
    if (const int src = names_state_check(e, b, 1)) return src;
    auto fail = [&](int rc) { rc = drain_ingest(b, rc); e->err = b->path + ": " + b->err; return rc; };
    try {
        while (!b->done) {
            const int rc = decode_next_chunk(e, b, o);
            if (e->names_mode) e->names_calls |= 1;
            if (rc < 0) return fail(rc);
            if (rc == 0) { b->done = true; break; }
            if (!b->defer_parse) b->cur->batches.clear();
            if (pause > 0 && !b->done && b->n_records - start >= pause) break;   // chunk boundary: the reader stays positioned
        }
    } catch (...) { drain_ingest(b, 0); throw; }                       // (XCK_GUARD makes an error code of it: no job may stay with the push thread)
    if (const int drc = drain_ingest(b, 0)) return fail(drc);          // (the caller may talk to the engine now: nothing is in flight)
    // device-names mode: the intern kernels behind the host-parsed chunks were not waited for - what they flagged (the id space used up) fails the call
    if (e->names_mode) { if (const int nrc = engine_names_check(e)) { b->err = e->err; return fail(nrc); } }
    if (n_records) *n_records = b->n_records;
    return b->done ? XCK_OK : 1;
}

// C++ exceptions (std::bad_alloc from a buffer that a damaged file made huge, ...) must not unwind through the C ABI into
// ctypes: they become error codes here.
#define XCK_GUARD(e_, expr)                                                                              \
    try { return (expr); }                                                                               \
    catch (const std::bad_alloc&) { if (e_) (e_)->err = "out of host memory"; set_thread_error("out of host memory"); return XCK_E_NOMEM; } \
    catch (const std::exception& x) { if (e_) (e_)->err = x.what(); set_thread_error(x.what()); return XCK_E_IO; }                        \
    catch (...) { if (e_) (e_)->err = "unknown C++ exception"; set_thread_error("unknown C++ exception"); return XCK_E_IO; }
int xck_bam_open(const char* path, int n_threads, xck_bam** out, char* err, size_t errlen) {
    xck_engine* none = nullptr;
    try { return bam_open_impl(path, n_threads, out, err, errlen); }
    catch (const std::bad_alloc&) { if (err && errlen) snprintf(err, errlen, "%s: out of host memory", path ? path : "(null)"); set_thread_error("out of host memory"); (void)none; return XCK_E_NOMEM; }
    catch (const std::exception& x) { if (err && errlen) snprintf(err, errlen, "%s: %s", path ? path : "(null)", x.what()); set_thread_error(x.what()); return XCK_E_IO; }
    catch (...) { if (err && errlen) snprintf(err, errlen, "%s: unknown C++ exception", path ? path : "(null)"); return XCK_E_IO; }
}
static int prefetch_impl(xck_engine* e, xck_bam* b, const xck_ingest_opts* o) {
    if (!e || !b || !o) return XCK_E_ARG;
    if (b->done || b->started) return XCK_OK;
    CallerBinding on_node(b);
    FoldDecodeStats fold{e, b};
    b->prefetching = true;
    if (e->names_mode) b->defer_parse = e->n_impl > 0;                 // (device-names mode: the chunks read ahead are walked on the device, as xck_ingest_bam will want them)
    const int rc = decode_next_chunk(e, b, o, true);
    b->prefetching = false;
    if (rc < 0) { e->err = b->path + ": " + b->err; return rc; }
    return XCK_OK;
}
int xck_bam_prefetch(xck_engine* e, xck_bam* b, const xck_ingest_opts* o) { XCK_GUARD(e, prefetch_impl(e, b, o)) }
int xck_bam_next_batch(xck_engine* e, xck_bam* b, const xck_ingest_opts* o, xck_batch* out) { XCK_GUARD(e, next_batch_impl(e, b, o, out)) }
int xck_ingest_bam(xck_engine* e, xck_bam* b, const xck_ingest_opts* o, int64_t* n_records) { XCK_GUARD(e, ingest_impl(e, b, o, n_records)) }

}  // extern "C"
