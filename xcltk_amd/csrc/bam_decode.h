// bam_decode.h - the BAM decoder's own types and the stage functions its two units share.  Private to the decoder: included by
// bam.cpp (the reader: ring, scanner, index, GPU share, jobs and push thread, C entry points), by bam_records.cpp (the work on one
// chunk that knows nothing of a reader: keys, barcodes, BGZF, SoA block, record walk, record parse, layout) and by the programs under
// tools/ that check either.
#pragma once
#include <pthread.h>
#include <sched.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <deque>
#include <functional>
#include <new>
#include <thread>
#include "xck_internal.h"
#include "inflate_dev.h"
#include "parse_dev.h"
#include "intern_dev.h"

namespace xck {

// ---------------------------------------------------------------------------------------------
// thread pool
// ---------------------------------------------------------------------------------------------
class Pool {
public:
    explicit Pool(int n) { for (int i = 0; i < n; i++) th_.emplace_back([this] { run(); }); }
    ~Pool() { { std::lock_guard<std::mutex> lk(mu_); stop_ = true; } cv_.notify_all(); for (auto& t : th_) t.join(); }
    // many tasks under ONE lock and one wake-up: a chunk hands ~100 part tasks to the pool three times (inflate / gather, walk, parse), and a
    // lock + futex wake per task cost the coordinator ~0.7 ms per chunk
    void submit_many(std::vector<std::function<void()>>& fs, bool front = false) {
        if (fs.empty()) return;
        { std::lock_guard<std::mutex> lk(mu_);
          if (front) for (size_t i = fs.size(); i-- > 0;) q_.push_front(std::move(fs[i])); else for (auto& f : fs) q_.push_back(std::move(f)); }
        if (fs.size() == 1) cv_.notify_one(); else cv_.notify_all();
        fs.clear();
    }
    int size() const { return (int)th_.size(); }
    void set_affinity(const cpu_set_t& set) { for (auto& t : th_) pthread_setaffinity_np(t.native_handle(), sizeof set, &set); }
private:
    void run() {
        for (;;) {
            std::function<void()> f;
            { std::unique_lock<std::mutex> lk(mu_); cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
              if (q_.empty()) return; f = std::move(q_.front()); q_.pop_front(); }
            f();
        }
    }
    std::vector<std::thread> th_; std::deque<std::function<void()>> q_; std::mutex mu_; std::condition_variable cv_; bool stop_ = false;
};

struct TaskGroup {
    std::mutex mu; std::condition_variable cv; int pending = 0;
    std::atomic<int> thrown{0};          // a task body threw: 1 = std::bad_alloc, 2 = anything else (checked by the waiter: an exception
                                         // that leaves a pool thread would otherwise end the process through std::terminate)
    int take_thrown() { return thrown.exchange(0); }
    // collect tasks with later(), hand them to the pool in one go with flush() (front: ahead of what is queued - work the coordinator
    // is waiting for).  The notify of a finished task happens UNDER the lock: a waiter may reuse or destroy the group as soon as wait()
    // returns, and wait() cannot return before the task has released the mutex - after which it touches the group no more.
    // (Notifying after the unlock let a waiter that saw pending == 0 leave first; the late pthread_cond_broadcast then wrote into
    // whatever the coordinator's stack held by then: "free(): invalid pointer", once per ~14 k chunks with more pool threads than
    // CPUs, tools/stress_e2e.py.)
    std::vector<std::function<void()>> batch;
    void later(std::function<void()> f) {
        batch.push_back([this, f] {
            try { f(); } catch (const std::bad_alloc&) { thrown.store(1); } catch (...) { thrown.store(2); }
            std::lock_guard<std::mutex> lk(mu); if (--pending == 0) cv.notify_all(); });
    }
    void flush(Pool& p, bool front = false) {
        if (batch.empty()) return;
        { std::lock_guard<std::mutex> lk(mu); pending += (int)batch.size(); }
        p.submit_many(batch, front);
    }
    void wait() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [this] { return pending == 0; }); }
};

static inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline uint16_t le16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }

struct BlockRef { uint64_t coff; uint32_t clen; uint32_t isize; uint32_t data_off; uint32_t data_len; uint64_t uoff; };
// (bam_records.cpp) parse one BGZF block header at file offset `coff`; returns false at EOF / on malformed data
bool bgzf_peek(const uint8_t* map, uint64_t fsize, uint64_t coff, BlockRef* out, std::string* err);
// (bam_records.cpp) inflate one block to dst (isize bytes) with the calling thread's own decoder state
bool bgzf_inflate(const uint8_t* map, const BlockRef& b, uint8_t* dst, bool verify_crc, std::string* err);

}  // namespace xck

using namespace xck;   // (the reader's own types are global, as the C handle xck_bam has to be; only the decoder's units and its checkers include this)

// One decoded chunk as structure-of-arrays, all columns carved out of ONE pinned block: the whole chunk crosses PCIe in a
// single hipMemcpyAsync (engine_push_block) and the batches of the chunk are slices of it.  Every ChunkJob (below) has one,
// so the decoder fills the next job's block while this one is still being copied; `fence` (an event owned by this block,
// recorded by the engine behind the copy) is waited for before the block is overwritten.
struct HostSoA {
    uint8_t* base = nullptr; size_t cap = 0, used = 0; bool pinned = false; void* fence = nullptr;
    int32_t* pos = nullptr; uint16_t* flag = nullptr; uint8_t* mapq = nullptr; int32_t* cell = nullptr; uint64_t* umi = nullptr;
    uint32_t* cig_off = nullptr; uint32_t* cigar = nullptr; uint32_t* seq_off = nullptr; uint8_t* seq = nullptr;
    // device-names mode: behind the columns (SoaLayout::total) one DiItem per kept record and the packed bytes of the names that have
    // to be interned - the parse tasks fill them, the block's copy takes them along (engine_push_block)
    bool has_names = false; xck::NameTrailer nt{0, 0, 0, 0}; xck::DiItem* items = nullptr; uint8_t* name_bytes = nullptr;
    // a handle with a base-quality floor: the quality region (parse_dev.h soa_qual_bytes) between the columns and the name trailer, else null
    uint8_t* qual = nullptr;
};

struct RecRef { const uint8_t* p; uint32_t len; int32_t tid; uint32_t l_seq; uint16_t n_cig; };

// Records found by one inflate task in its own byte range, walked right after inflating (data
// still hot in that core's cache) under the SPECULATION that a record starts at the first byte of
// the range - true for BGZF writers that flush a block before a record that would not fit (htslib,
// samtools, this repo's writers).  The task also sums up what its records need in the SoA (kept records, CIGAR words,
// sequence bytes) and notes where the contig changes: the output layout is a prefix sum over the parts and each part is
// parsed by its own task.  When a speculation of the chunk failed the stitch re-walks serially and cuts its record list
// into pieces of the same shape (Chunk::stitched), so layout and parse know one kind of input.
struct ContigRun { uint32_t first; int32_t contig; };                    // records [first, next run's first) of the part are on `contig` (-1: unused)
struct WalkPart {
    size_t u_begin = 0, u_end = 0, spec_start = 0, stop = 0; std::vector<RecRef> recs;
    size_t n_out = 0, n_cig = 0, n_seq = 0; std::vector<ContigRun> runs;
    size_t n_name = 0;                                                    // l_name summed over the kept records: the room their names can take (device-names mode)
    size_t out_base = 0, cig_base = 0, seq_base = 0, name_base = 0;       // filled by the coordinator (layout_chunk)
    size_t i0 = 0, i1 = 0;                                                // the part's blocks: [i0, i1) of the chunk
};

struct Chunk {
    std::vector<BlockRef> blocks;
    std::vector<uint8_t> ubuf; size_t usize = 0;
    uint8_t* ubase = nullptr;          // where the chunk's inflated bytes live: ubuf, or the pinned output block of its GPU slot
    std::vector<WalkPart> parts;
    // a chunk that was stitched serially: its records in pieces of a parse task's size (only recs, runs and the n_* / *_base fields are
    // used), and the record that straddles the boundary to the previous chunk, assembled from the reader's carry.  Both are read by the
    // chunk's parse tasks, which may run behind the coordinator: they live here, with the inflated bytes, until the chunk is released.
    std::vector<WalkPart> stitched; std::vector<uint8_t> stitch;
    TaskGroup tg; std::atomic<bool> failed{false}; std::string err; std::mutex emu;
    bool valid = false, new_range = false; uint32_t first_skip = 0; int range_id = 0;
    // GPU share of the inflate (csrc/inflate_dev.hip): the pool only gathers the compressed bytes into the slot's pinned block, the task
    // that finishes last enqueues copy-in, kernel and copy-out; walk (and the blocks the kernel left) follow when the chunk is consumed
    bool gpu = false; std::atomic<int> copy_left{0}; std::atomic<int> gpu_rc{0}; size_t in_total = 0;
    std::atomic<int> launched{0};      // the last gather task has handed the chunk to the device (gpu_rc says how that went)
    bool stage2 = false;               // the walk tasks that follow the device's inflate have been queued
    // device walk + parse (csrc/parse_dev.hip): the chunk was launched with the walk behind its inflate and nothing stored to the host
    // (dparse); its summaries came back clean, so no walk task was queued (dp_ok) - until something sends it down the host path after all
    bool dparse = false, dp_ok = false;
};

struct PendingBatch { int32_t contig; int64_t r0, r1; uint64_t ordinal_base; };

// BAM tid (+ record position) -> engine contig: -1 for references that are not wanted and for records that start at or
// beyond the end of the position window of their reference (xck_ingest_opts.tid_end)
struct ContigMap {
    const int32_t* t2c = nullptr; const int32_t* t_end = nullptr; int n_refs = 0;
    int32_t only_tid = -1;               // position windows: the chunk belongs to the index range of ONE reference; the tail block of that
                                         // range also holds the first records of the next reference, which that reference's own range
                                         // delivers again - they are dropped here, so no record reaches the consumer twice
    inline int32_t operator()(int32_t tid, int32_t pos) const {
        if (tid < 0 || tid >= n_refs || !t2c) return -1;
        if (only_tid >= 0 && tid != only_tid) return -1;
        if (t_end && t_end[tid] > 0 && pos >= t_end[tid]) return -1;
        return t2c[tid];
    }
};

// where the ingest time goes (XCK_DEBUG_TIMING=1 prints it when the reader is closed): pool-side CPU time summed over
// threads, and the phases of the coordinating thread
struct DecodeTimes {
    std::atomic<uint64_t> inflate{0}, walk{0}, parse{0};                 // ns, summed over pool threads
    uint64_t wait_inflate = 0, sched = 0, stitch = 0, layout = 0, wait_parse = 0, wait_push = 0;   // ns, coordinating thread
    uint64_t push = 0;                                                   // ns, push thread (engine_push_block, engine_push_parsed)
    uint64_t push_parsed = 0, dp_layout = 0, dp_copy_out = 0;            // ns: engine_push_parsed alone (push thread); summaries -> batches (coordinator); fallback copies d_out -> h_out
    uint64_t chunks = 0, slow_chunks = 0; std::chrono::steady_clock::time_point t_open;
};
static inline uint64_t ns_since(std::chrono::steady_clock::time_point t0) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }

// The BGZF block headers form a chain (every header gives the offset of the next one): a scanner thread walks it ahead of
// the decoder - it also takes the page faults of the mapping - and hands over one plan per chunk.
struct ChunkPlan { std::vector<BlockRef> blocks; size_t usize = 0; uint32_t first_skip = 0; int range_id = 0; bool new_range = false, failed = false, end = false; std::string err; };
struct ScanRange { uint64_t coff; uint32_t skip; uint64_t stop; };
class Scanner {
public:
    Scanner(const uint8_t* map, uint64_t fsize, size_t chunk_target, std::vector<ScanRange> ranges)
        : map_(map), fsize_(fsize), target_(chunk_target), ranges_(std::move(ranges)) { th_ = std::thread([this] { run(); }); }
    ~Scanner() { { std::lock_guard<std::mutex> lk(mu_); stop_ = true; } cv_.notify_all(); if (th_.joinable()) th_.join(); }
    void abandon(int range_id) { abandoned_.store(range_id); }          // the decoder has seen everything it wants of that range
    ChunkPlan next() {                                                  // blocks until a plan is ready; `end` after the last chunk
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return !q_.empty(); });
        ChunkPlan p = std::move(q_.front()); q_.pop_front();
        lk.unlock(); cv_.notify_all();
        return p;
    }
private:
    bool put(ChunkPlan&& p) {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [this] { return stop_ || q_.size() < 3; });
        if (stop_) return false;
        q_.push_back(std::move(p)); lk.unlock(); cv_.notify_all();
        return true;
    }
    void run() {
        // (the scanner's only allocations are the block lists: out of memory ends the stream with a failed plan, not the process)
        try { scan(); }
        catch (...) { ChunkPlan f; f.failed = true; f.err = "out of host memory (BGZF scanner)"; f.blocks.clear(); if (put(std::move(f))) { ChunkPlan z; z.end = true; put(std::move(z)); } }
    }
    void scan() {
        for (size_t ri = 0; ri < ranges_.size(); ri++) {
            const ScanRange& rg = ranges_[ri];
            uint64_t coff = rg.coff; bool first = true, ended = false;
            while (!ended) {
                if (abandoned_.load() == (int)ri) break;
                ChunkPlan p; p.new_range = first; p.first_skip = first ? rg.skip : 0; p.range_id = (int)ri; first = false;
                size_t usz = 0;
                while (usz < target_) {
                    if (coff > rg.stop) { ended = true; break; }          // end of the indexed range
                    BlockRef br; std::string e;
                    if (!bgzf_peek(map_, fsize_, coff, &br, &e)) { ended = true; if (!e.empty()) { p.failed = true; p.err = e; } break; }
                    br.uoff = usz; usz += br.isize; coff += br.clen;
                    p.blocks.push_back(br);
                }
                p.usize = usz;
                if (p.blocks.empty() && !p.failed) { if (p.new_range) { /* an empty range: nothing to hand over */ } break; }
                const bool failed = p.failed;
                if (!put(std::move(p))) return;
                if (failed) { ChunkPlan z; z.end = true; put(std::move(z)); return; }
            }
        }
        ChunkPlan z; z.end = true; put(std::move(z));
    }
    const uint8_t* map_; uint64_t fsize_; size_t target_; std::vector<ScanRange> ranges_;
    std::thread th_; std::mutex mu_; std::condition_variable cv_; std::deque<ChunkPlan> q_; bool stop_ = false;
    std::atomic<int> abandoned_{-1};
};

#ifndef XCK_PUSH_Q
#define XCK_PUSH_Q 2
#endif
constexpr int PUSH_Q = XCK_PUSH_Q;      // chunks the coordinator may run ahead of the push thread (Pusher)
constexpr int N_CHUNK = 3 + PUSH_Q, N_JOB = PUSH_Q + 1;
// One decoded chunk in flight, from its layout to the end of its push: the SoA block, the batch list (slices of the block), the parse
// tasks and their flags, the ring chunk the parse still reads (inflated bytes + record lists, until `parsed`) and the engine the chunk
// goes to.  The k-th chunk a reader decodes takes jobs[k % N_JOB], whoever consumes it.  xck_bam_next_batch and a decode-only
// xck_ingest_bam wait for the parse themselves.  On a GPU-backed handle EVERY chunk's job - one without batches too - goes to the push
// thread (Pusher), which waits for the parse tasks and pushes the block (engine_push_block: one H2D copy + the join launches) in file
// order while the coordinator schedules, waits for and lays out the next chunks (with the GPU share of the inflate the coordinator had
// become the limiter: schedule + wait for parse + push = 4.5 ms per chunk, the pool a third idle).  At most Pusher::MAXQ = N_JOB - 1
// jobs are with the push thread, so the slot of chunk k is free again when chunk k + N_JOB is laid out (take_job checks it).
struct ChunkJob {
    HostSoA soa; std::deque<PendingBatch> batches;
    TaskGroup tg; std::atomic<int> flags{0};   // the parse tasks; what they found (parse_error)
    xck_engine* e = nullptr;           // the handle of the call that decoded the chunk: where the push thread pushes it
    int ring_idx = -1;                 // the ring chunk the parse tasks read, while the job holds it
    std::atomic<int> parsed{0};        // set by the push thread once the parse tasks have ended: the coordinator may take the ring chunk back
    bool released = true;              // (coordinator) the ring chunk was taken back, or was never held
    std::atomic<int> queued{0};        // with the push thread: set by Pusher::submit, cleared when the job's push has ended
    // a chunk walked on the device: no parse tasks, the push thread launches the parse kernel (engine_push_parsed) - or, if that kernel
    // flags the chunk, takes it down the host path itself (redo_on_host), for which it needs what the coordinator knew
    bool dev = false; xck_bam* b = nullptr; DpChunkLayout lay; ContigMap cm; xck_ingest_opts opts; int64_t rec_before = 0;
    bool names = false;                // device-names mode: the chunk's names are keyed by the handle's device table (take_job)
    bool qual = false;                 // the handle has a base-quality floor: the block carries the records' qualities (take_job)
};
struct Pusher {
    static constexpr int MAXQ = PUSH_Q; // jobs the coordinator may run ahead
    std::thread th; std::mutex mu; std::condition_variable cv;
    bool stop = false; ChunkJob* q[MAXQ] = {}; int qh = 0, qn = 0;
    int rc = 0; std::string err;       // first failure (parse flags or push); later jobs are waited for, not pushed
    uint64_t push_ns = 0, parse_wait_ns = 0, push_parsed_ns = 0;
    void run();
    Pusher() { th = std::thread([this] { run(); }); }
    // blocks while MAXQ jobs are outstanding; returns the first failure so far (the job is queued regardless: its parse must be waited for)
    int submit(ChunkJob* j) {
        std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [this] { return qn < MAXQ; });
        j->queued.store(1); q[(qh + qn) % MAXQ] = j; qn++; cv.notify_all(); return rc;
    }
    int wait_idle() { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [this] { return qn == 0; }); return rc; }
    ~Pusher() { { std::lock_guard<std::mutex> lk(mu); stop = true; cv.notify_all(); } if (th.joinable()) th.join(); }
};
constexpr int N_CHUNK_GPU = 16;        // ring depth with the GPU share on: its chunks need several in flight on the device (one wave per block)
// XCK_GPU_INFLATE=<percent>: that share of the chunks is inflated on the handle's GPU (0 = off).  State of one reader:
struct GpuShare {
    bool tried = false, on = false, broken = false, verbose = false; int pct = 0, acc = 0, device = -1, free_cus = 32, depth = 4;
    GpuInflateSlot* slot[N_CHUNK_GPU] = {nullptr}; bool inflight[N_CHUNK_GPU] = {false};   // slot[k]: the slot that holds ring chunk k (its inflated bytes live there until the chunk is consumed)
    std::vector<GpuInflateSlot*> free_slots;                             // slots of consumed chunks, reused before a new one is made
    int max_held = 10;                                                   // device chunks in the ring at a time (in flight + inflated, not yet consumed) = slots this reader ever holds
    uint64_t chunks = 0, blocks = 0, left_blocks = 0, wait_ns = 0, copy_ns = 0;
    // device walk + parse of the device chunks (XCK_GPU_PARSE): whether the handle and its barcode list allow it, the contig tables in
    // device memory (uploaded anew when a call brings other tables; the old ones live until the reader closes: walks in flight read them)
    bool parse = false; std::atomic<bool> parse_off{false}; std::atomic<int> fb_row{0};
    std::vector<int32_t> cm_host; int32_t* d_cm = nullptr; bool cm_tend = false; std::vector<void*> d_cm_all;
};
struct CallerBinding;
struct xck_bam {
    std::string path; int fd = -1; const uint8_t* map = nullptr; uint64_t fsize = 0;
    std::vector<std::string> ref_names; std::vector<int64_t> ref_lens;
    uint64_t next_coff = 0;            // first BGZF block with alignment records
    // .bai: per reference [beg, end) virtual offsets + record counts (samtools pseudo-bin 37450 or bin chunks)
    bool idx_loaded = false, idx_ok = false;
    std::vector<uint64_t> idx_beg, idx_end; std::vector<int64_t> idx_mapped, idx_unmapped; std::vector<std::vector<uint64_t>> idx_lin;
    std::vector<std::pair<uint64_t, uint64_t>> ranges; bool use_ranges = false, ranges_set = false;
    uint32_t first_skip = 0;           // bytes of the first block that precede the first record
    Scanner* scanner = nullptr; bool scan_end = false;
    std::vector<int32_t> range_tid;                       // per_tid_ranges: reference of every range
    bool per_tid_ranges = false; int skip_range = -1;   // position windows: one range per reference; a range is dropped once a record starts beyond its window
    Pool* pool = nullptr; int n_threads = 1;
    Chunk ch[N_CHUNK_GPU]; int n_ring = N_CHUNK, head = 0, n_sched = 0;      // ring of n_ring chunks: ch[head] is decoded next, n_sched chunks are inflating / inflated
    GpuShare gi;
    bool started = false;              // a decode call has been made (xck_bam_prefetch alone does not count)
    bool prefetching = false;          // inside xck_bam_prefetch
    Pusher* pusher = nullptr;          // made at the first chunk of a GPU-backed ingest
    ChunkJob jobs[N_JOB]; uint64_t n_jobs = 0;   // jobs[k % N_JOB] belongs to the k-th chunk decoded (take_job)
    ChunkJob* cur = nullptr;           // the job of the chunk decoded last: xck_bam_next_batch hands its batches out
    bool defer_parse = false;          // set by xck_ingest_bam for GPU-backed handles: parse and push run behind the coordinator
    std::vector<uint8_t> carry;        // partial record from the previous chunk
    int64_t n_records = 0;             // records walked so far (all, including unused contigs)
    bool done = false;
    size_t chunk_target = 48u << 20;   // uncompressed bytes per chunk
    // NUMA binding (bind_to_numa_node): the pool and the scanner sit on the node of the handle's GPU while the reader is open; the
    // CALLING thread (it runs the coordinator, and its first touch places the inflate buffers) only for the duration of a decode
    // call (CallerBinding) - between calls, and on whatever thread closes the reader, the caller's own mask is untouched
    bool numa_bound = false, threads_auto = false; cpu_set_t numa_set, old_affinity;
    struct CallerBinding* cur_binding = nullptr;
    DecodeTimes tm;
    std::atomic<int64_t> dstat[DS_N] = {}; int64_t dstat_folded[DS_N] = {};   // xck_decode_stats of this reader; the part already added to a handle's
    std::string err;
};

// ---------------------------------------------------------------------------------------------
// the stages of one chunk (bam_records.cpp): none of them knows the reader
// ---------------------------------------------------------------------------------------------
namespace xck {
// the part of encode_key() that needs no table: empty string -> NONE, short ACGT string -> 2-bit code
bool encode_key_direct(const char* s, size_t n, int umi_bits, uint64_t* out);
// carve the columns of a chunk with n_reads kept records out of the block (growing it if needed)
bool soa_reserve(HostSoA& s, size_t n_reads, size_t n_cig, size_t n_seq, size_t name_items = 0, size_t name_bytes = 0, bool names = false, bool qual = false);
void soa_free(HostSoA& s);
// a batch = a slice of the chunk's SoA block
void fill_batch(const HostSoA& s, const PendingBatch& pb, bool want_seq, xck_batch* bt);
// pool task: inflate the part's blocks (st given: only those the GPU kernel left), then walk the records of its byte range speculatively
void run_part(Chunk* cp, const uint8_t* map, bool verify_crc, WalkPart* wpp, DecodeTimes* tm, const ContigMap cm, bool want_seq, const int32_t* st,
              std::atomic<int64_t>* dstat);
// pool task: the records of one piece of a chunk -> the SoA block, at the piece's bases (layout_chunk)
// (n_filtered: where the piece adds the records the handle's tag filter rejected - the reader's DS_TAG_FILTERED counter)
void parse_part(DecodeTimes* tm, xck_engine* e, HostSoA* sp, int32_t sample, const WalkPart* wp, const ContigMap cm, std::atomic<int>* flags,
                std::atomic<int64_t>* n_filtered = nullptr);
// where every piece's records go in the job's SoA block, and the job's batches; returns the chunk's record count, < 0 on error
int64_t layout_chunk(ChunkJob& j, std::vector<WalkPart>& pieces, const xck_ingest_opts* o, bool want_seq, int64_t records_before, std::string* err);
}  // namespace xck
