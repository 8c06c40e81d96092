// xck_internal.h - shared declarations between the HIP engine, the BAM decoder and the C-ABI.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include <unordered_map>
#include <mutex>
#include <atomic>
#include "../../include/xck.h"

#define XCK_VERSION_STR "0.1.0 (gfx950)"

namespace xck {

// BAM flag bits used by check_read (reference xcltk/utils/sam.py:120-121)
constexpr uint32_t BAM_FPAIRED = 1, BAM_FPROPER_PAIR = 2, BAM_FUNMAP = 4;

// ordinal layout: (bam_index << 40) | record number ; value word of a pileup hit:
// (ordinal << 5) | (allele nibble + 1), 0 in the low 5 bits = "read has no base at the SNP"
constexpr int ORD_REC_BITS = 40;
constexpr int ALLELE_BITS = 5;

// Host-side string -> dense id table for keys that cannot be 2-bit coded (IUPAC UMIs,
// read names in UMI-less mode).  Sharded so decoder threads can intern concurrently.
class InternTable {
public:
    static constexpr int NSHARD = 64;
    uint64_t intern(const char* s, size_t n);
    // many strings at once: grouped by shard, so that a shard's lock is taken once and its slots stay in the cache
    struct Item { uint64_t h; const char* s; uint32_t n; uint32_t pad; uint64_t* out; int umi_bits; };
    void intern_batch(std::vector<Item>& items, bool* overflow);
    static uint64_t hash(const char* s, size_t n);
    uint64_t size() const;
    void clear();
private:
    // open addressing over (hash, bytes in a per-shard arena): no allocation per lookup (a std::unordered_map<std::string>
    // cost ~4 us per read name in UMI-less mode and made the well-based ingest 10x slower than the 10x one)
    struct Slot { uint64_t h; uint32_t off; uint32_t len1; uint32_t idx; uint32_t epoch; };   // live iff epoch == the shard's (clear() is O(1))
    struct Shard {
        std::mutex mu; std::vector<Slot> slots; std::vector<char> arena; uint32_t count = 0, epoch = 1;
        void grow();
    };
    Shard shards_[NSHARD];
    // id = (local index << 6) | shard  -> unique without a global counter
    static uint64_t probe_or_insert(Shard& sh, uint64_t h, const char* s, uint32_t n);   // (bam_records.cpp: intern and intern_batch)
};

// Decoder settings derived from xck_config at xck_create()
struct DecodeCfg {
    bool use_barcodes = false;
    bool use_umi = false;
    char cell_tag[2] = {0, 0};
    char umi_tag[2] = {0, 0};
    int  umi_bits = 64;
    bool want_seq = false;
    bool want_qual = false;              // the handle's pileup has a base-quality floor (xck_config.min_baseq): the records' quality bytes are kept
    bool verify_crc = false;             // check the CRC32 of every block the record decoder inflates (XCK_F_VERIFY_CRC, XCK_F_DEVICE_CRC)
    bool crc_on_device = false;          // ... and keep the GPU share of the inflate: the kernel checks its blocks (XCK_F_DEVICE_CRC)
    // the tag filter (xck_config.filter_tag / XCK_TAG_FILTER): a record whose first filter_tag is not an integer v in 0 .. 2^32 - 1 with
    // (v & filter_mask) == filter_value gets cell = XCK_CELL_FILTERED (parse_dev.h tag_filter_pass: one rule for host and device)
    bool filter_on = false;
    char filter_tag[2] = {0, 0};
    uint32_t filter_mask = 0, filter_value = 0;
    int  n_threads = 0;
    int64_t max_batch_reads = 0;
    // barcode hash (open addressing over the barcode strings)
    struct BcSlot { uint64_t h; int32_t idx; uint16_t len; char key[18]; };   // 32 bytes: hash, column (-1 = empty), the barcode itself
    std::vector<std::string> barcodes;
    std::vector<BcSlot> bc_slots;        // size pow2
    uint64_t bc_mask = 0;
    int32_t lookup_cell(const char* s, size_t n) const;
    void build_barcodes(const char* const* names, int n);
};

uint64_t hash_bytes(const char* s, size_t n);
// 2-bit / interned key code, see include/xck.h xck_umi_bits()
uint64_t encode_key(const char* s, size_t n, int umi_bits, InternTable& tab, bool* overflow);

constexpr int XCK_F_LAYOUT_BOTH = 1 << 16;   // internal: size the row field for regions AND SNPs (fused handle)
// key layout rule shared by engine and decoder: 64-bit keys (row | cell | umi) when the UMI code
// gets >= 26 bits, otherwise 128-bit keys with a 64-bit UMI code.
struct KeyBits { int key_bits, ubits, cbits, rbits; };
inline int bits_for_count(int64_t n) { int b = 1; while ((int64_t(1) << b) < n) b++; return b; }
inline KeyBits key_layout(const xck_config* cfg) {
    KeyBits k;
    k.cbits = bits_for_count(cfg->n_cells > 2 ? cfg->n_cells : 2);
    // (rows are sized for one more than there are: the row field is then never all ones, so no key equals ~0 - the "empty" word of the
    // LDS hash sets of the folds - whatever the cell and UMI fields hold)
    k.rbits = bits_for_count((int64_t)(cfg->n_regions > 2 ? cfg->n_regions : 2) + 1);
    if ((cfg->mode & XCK_MODE_BAF) || (cfg->flags & XCK_F_LAYOUT_BOTH)) { int sb = bits_for_count((int64_t)(cfg->n_snps > 2 ? cfg->n_snps : 2) + 1); if (sb > k.rbits) k.rbits = sb; }
    int ub = 64 - k.rbits - k.cbits;
    if ((cfg->flags & XCK_F_FORCE_KEY128) || ub < 26) { k.key_bits = 128; k.ubits = 64; }
    else { k.key_bits = 64; k.ubits = ub; }
    return k;
}

// Tuning / test knobs of a handle, read from the environment ONCE, at xck_create (include/xck.h lists them with their meaning):
// the host path of push / finish never calls getenv().
struct Knobs {
    bool debug_timing = false;           // XCK_DEBUG_TIMING
    bool fold_sort = false;              // XCK_FOLD=sort
    int  fold_c = 0;                     // XCK_FOLD_C (0 = the built-in page size)
    int  fold_lgg = -1;                  // XCK_FOLD_LGG (-1 = by the number of cells)
    int  fold_copies_lg = 4;             // XCK_FOLD_COPIES_LG
    int  fold_bucket_blocks = 2048;      // XCK_FOLD_BUCKET_BLOCKS
    int  fold_overlap = 1;               // XCK_FOLD_OVERLAP
    int  fold_overlap_blocks = 512;      // XCK_FOLD_OVERLAP_BLOCKS
    bool full_sort = false;              // XCK_FULL_SORT
    bool pileup_radix = false;           // XCK_PILEUP_SORT=radix
    int  pileup_hap = 0;                 // XCK_PILEUP_HAP: 0 = packed class bits, 1 = sorted, 2 = values
    int  pileup_lgg = 10;                // XCK_PILEUP_LGG
    long long hit_slack = 65536;         // XCK_HIT_SLACK
    long long hit_cap0 = 1 << 20;        // XCK_HIT_CAP0
    int  push_stage = -1;                // XCK_PUSH_STAGE (-1 = by size)
    long long push_stage_bytes = 2 << 20;   // XCK_PUSH_STAGE_BYTES
    int  gpu_inflate_pct = -1;           // XCK_GPU_INFLATE: share (percent) of the BGZF chunks inflated on the handle's GPU; -1 = auto (keep gpu_inflate_depth chunks on the device)
    int  gpu_inflate_depth = 10;         // XCK_GPU_INFLATE_DEPTH
    int  gpu_inflate_ring = 12;          // XCK_GPU_INFLATE_RING: chunks in flight (host + device) while the GPU share is on
    int  gpu_inflate_min_mb = 96;        // XCK_GPU_INFLATE_MIN_MB: auto mode only for files (index ranges) of at least this many compressed MB
    int  gpu_inflate_free_cus = 32;      // XCK_GPU_INFLATE_FREE_CUS: CUs the inflate streams never use (they stay free for the join kernels)
    bool read_fate = false;              // XCK_READ_FATE=1: XCK_F_READ_FATE ORed into the flags of every handle that drives a GPU
    bool cell_summary = false;           // XCK_CELL_SUMMARY=1: XCK_F_CELL_SUMMARY ORed into the flags of every handle that drives a GPU
    int  cell_summary_slots = 0;         // XCK_CELL_SUMMARY_SLOTS: rows of the per-block LDS tables (0 = the built-in 512 per-cell, 1024 per-feature / per-SNP; tests: small tables reach the no-fit path)
    bool feature_summary = false;        // XCK_FEATURE_SUMMARY=1: XCK_F_FEATURE_SUMMARY ORed into the flags of every handle that drives a GPU
    bool umi_consensus = false;          // XCK_UMI_CONSENSUS=1: XCK_F_UMI_CONSENSUS ORed into the flags of every handle with a BAF pipeline that drives a GPU
    int  umi_feature = 0; std::string umi_feature_text;   // XCK_UMI_FEATURE=unique: XCK_F_UNIQUE_FEATURE ORed into the flags of every handle with a basefc pipeline that drives a GPU; -1 = a value that is neither `unique` nor `all` nor empty (xck_create fails and quotes the text)
    int  umi_dedup = 0; std::string umi_dedup_text;   // XCK_UMI_DEDUP=1mm_all: XCK_F_UMI_COLLAPSE ORed into the flags of every handle with a basefc pipeline that drives a GPU; -1 = a value that is neither `1mm_all` nor `exact` nor empty (xck_create fails and quotes the text)
    int  min_baseq = 0; std::string min_baseq_text;   // XCK_MIN_BASEQ=<0 .. 93>: xck_config.min_baseq of every handle with a BAF pipeline that drives a GPU and sets none; -1 = malformed (xck_create fails and quotes the text)
    long long ref_chunk_bytes = 32ll << 20;   // XCK_REF_CHUNK_BYTES: raw FASTA bytes per staging chunk of xck_set_contig_ref (64 .. 2^30; tests: 64 cuts a tiny contig into many chunks)
    int  group_long_row = 64;            // XCK_GROUP_LONG_ROW: rows of xck_group_counts with at least this many entries take one block each (1 .. 64; tests: a small value reaches that shape with small inputs)
    bool gpu_parse = true;               // XCK_GPU_PARSE=auto|0: walk and parse the GPU-inflated chunks on the device where that applies (bam.cpp device_parse_now)
    bool gpu_names = false;              // XCK_GPU_NAMES=1: read names of a UMI-less handle are interned on the device (intern_dev.h; the conditions: api.cpp xck_create)
    long long gpu_names_slots0 = 1 << 21;   // XCK_GPU_NAMES_SLOTS0: first size of the device table (slots; tests: 64 makes a small file grow it several times)
    long long gpu_names_arena0 = 64 << 20;  // XCK_GPU_NAMES_ARENA0: first size of its arena (bytes)
    int  names_hash_bits = 0;            // XCK_TEST_NAMES_HASH_BITS: the device table keeps only that many low hash bits (0 = all)
    int  verify_crc = 0;                 // XCK_VERIFY_CRC: 0 = as the flags say, 1 = host (XCK_F_VERIFY_CRC ORed in), 2 = device (XCK_F_DEVICE_CRC)
    // XCK_TAG_FILTER=TAG:VALUE[/MASK]: 0 = unset, 1 = parsed into the three fields, -1 = malformed (xck_create fails and quotes tag_filter_text)
    int  tag_filter = 0; char tag_filter_tag[2] = {0, 0}; uint32_t tag_filter_mask = 0, tag_filter_value = 0; std::string tag_filter_text;
    static Knobs from_env();             // api.cpp
};

// xck_decode_stats counters (include/xck.h), in this order.  A reader counts in its own set; every decode call adds what it counted
// since the last call to its handle's (bam.cpp fold_decode_stats).
enum DecodeStat { DS_GPU_CHUNKS, DS_GPU_BLOCKS, DS_GPU_LEFT, DS_CRC_DEVICE, DS_CRC_HOST, DS_CRC_MISMATCH_DEVICE, DS_CRC_DISAGREE, DS_GPU_GIVEN_UP, DS_PARSE_CHUNKS, DS_PARSE_FALLBACKS, DS_NAMES_INTERNED, DS_NAMES_DISTINCT, DS_NAMES_HOST_CHUNKS, DS_TAG_FILTERED, DS_N };
// (DS_NAMES_INTERNED / DS_NAMES_DISTINCT are the device table's own counters: xck_get_decode_stats asks the table)

struct EngineImpl;                       // one GPU pipeline of a handle (engine_impl.h)
struct Stager;                           // device staging slots of engine_push_block (pipeline.hip)
struct DevIntern;                        // the handle's intern table in HBM (intern_dev.h)
uint64_t intern_id_limit(int umi_bits);  // ids an intern table may hand out for that key width (bam_records.cpp; XCK_TEST_INTERN_LIMIT)
// the names a host-parsed chunk hands to the device table: DiItem[n_out] at items_off of its block, the packed bytes behind them
struct NameTrailer { size_t items_off, bytes_off, n_bytes, n_out; };

// the decoder's own batches are valid by construction and skip the O(n) check of xck_push_batch()
int push_trusted(xck_engine* e, const xck_batch* b, const uint8_t* qual = nullptr);
// host threads this process may really use: min(hardware threads, CPU affinity, cgroup CPU quota) - a container with a
// 16-CPU quota on a 256-thread host must not start 256 decoder threads
int  default_threads();
void set_thread_error(const std::string& s);
const char* get_thread_error();

}  // namespace xck

// The engine object behind the opaque C handle.
struct xck_engine {
    std::string err;
    xck::DecodeCfg dec;
    xck::InternTable intern;
    xck::EngineImpl* impls[2] = {nullptr, nullptr};   // the handle's pipelines; fused handle (XCK_MODE_BOTH): [0] basefc, [1] pileup
    int n_impl = 0;                      // 0: decode-only handle, no GPU engine behind it
    xck::Stager* stager = nullptr;       // device staging slots of engine_push_block
    struct PushRing { void* blk[3] = {nullptr, nullptr, nullptr}; size_t cap[3] = {0, 0, 0}; void* fence[3] = {nullptr, nullptr, nullptr}; int next = 0; } push_ring;   // pinned blocks of xck_push_batch's one-copy form (api.cpp)
    xck::Knobs knobs;                    // the environment, read once at xck_create
    // device-names mode (XCK_GPU_NAMES, include/xck.h): set at xck_create for the handle's life.  names_calls: which decode calls the
    // handle has seen since the table was last cleared (1 = xck_ingest_bam, 2 = xck_bam_next_batch): the two do not mix
    bool names_mode = false; int names_calls = 0; xck::DevIntern* dnames = nullptr;
    std::atomic<int64_t> gpu_inflate_chunks{0};   // chunks inflated on the device by the readers that fed this handle (xck_stats)
    std::atomic<int64_t> dstat[xck::DS_N] = {};   // xck_decode_stats, summed over the readers that fed this handle since the last xck_reset
    int mode = 0;
    bool read_fate = false;              // made with XCK_F_READ_FATE (or XCK_READ_FATE=1), or with the flag below, which implies it
    bool cell_summary = false;           // made with XCK_F_CELL_SUMMARY (or XCK_CELL_SUMMARY=1)
    bool feature_summary = false;        // made with XCK_F_FEATURE_SUMMARY (or XCK_FEATURE_SUMMARY=1)
    bool umi_consensus = false;          // made with XCK_F_UMI_CONSENSUS (or XCK_UMI_CONSENSUS=1) and a BAF pipeline: its molecule stage votes (umi_consensus.h)
    bool unique_feature = false;         // made with XCK_F_UNIQUE_FEATURE (or XCK_UMI_FEATURE=unique) and a basefc pipeline: its fold counts unique-feature molecules only (umi_feature.h)
    bool umi_collapse = false;           // made with XCK_F_UMI_COLLAPSE (or XCK_UMI_DEDUP=1mm_all) and a basefc pipeline: its fold counts the components of the 1-mismatch graph (umi_collapse.h)
    bool base_tally = false;             // made with XCK_F_BASE_TALLY and a BAF pipeline: its pileup pipeline keeps base tallies (base_tally.h)
    bool contig_len_set = false;         // ... and xck_set_contig_lengths has been called
    int  min_baseq = 0;                  // base-quality floor of the pileup pipeline's join (xck_config.min_baseq or XCK_MIN_BASEQ), 0 = off
    int umi_bits = 64;
    int32_t n_cells = 0, n_contigs = 0;  // bounds that caller-supplied batches are checked against (xck_push_batch)
    // host pinned batch staging used by xck_ingest_bam lives in the xck_bam
};

// implemented in pipeline.hip (the summaries: the headers engine.hip includes; engine_finish and what follows it: finish.hip).  A per-pipeline call takes the
// pipeline it works on; nothing in the handle says which one is "current", so calls from several threads do not meet there.
namespace xck {
int  engine_create(const xck_config* cfg, xck_engine* e, EngineImpl** out);   // *out is set as soon as it exists: a failed create still has to be destroyed
void engine_destroy(EngineImpl* im);
int  engine_push(EngineImpl* im, const xck_batch* b, bool device_resident, const uint8_t* qual = nullptr);   // qual (a pileup pipeline with a floor, host arrays): 2 * (seq_off[n] - seq_off[0]) bytes
int  engine_baseq_stats(EngineImpl* im, xck_baseq_stats* out);     // pipeline.hip: the join's pair counters since the last reset
int  engine_flush(EngineImpl* im);
int  engine_finish(EngineImpl* im, xck_result* out);
int  engine_finish_async(EngineImpl* im);
int  engine_result_device(EngineImpl* im, xck_result* out);
int  engine_refold(EngineImpl* im, const xck_refold_config* cfg, xck_result* out);   // refold.h (finish.hip): the pileup pipeline's region stage under new tables
int  engine_snp_counts(EngineImpl* im, xck_result* out);           // snp_counts.h (finish.hip): SNP x cell AD / DP / OTH of the finished pileup
// what one xck_group_counts spent, summed over the handle's pipelines (XCK_DEBUG_TIMING, tools/group_counts_time.py)
struct GroupTimes { double ms_total = 0, ms_ptr = 0, ms_count = 0, ms_emit = 0, ms_copy = 0; long long entries = 0, nnz[4] = {0, 0, 0, 0}; };
int  engine_group_counts(EngineImpl* im, int source, int n_groups, const int32_t* cell_group, xck_result* out, GroupTimes* gt);   // group_counts.h (finish.hip): one pipeline's matrices summed per cell group
int  engine_reset(EngineImpl* im);
int  engine_stats(const EngineImpl* im, xck_stats* out);
int  engine_read_fate(EngineImpl* im, xck_read_fate* out);         // read_fate.h
int  engine_cell_summary(EngineImpl* im, xck_cell_summary* out);   // cell_summary.h
int  engine_feature_summary(EngineImpl* im, xck_feature_summary* out);   // feature_summary.h
int  engine_molecule_stats(EngineImpl* im, xck_molecule_stats* out);   // umi_consensus.h (finish.hip)
int  engine_umi_feature_stats(EngineImpl* im, xck_umi_feature_stats* out);   // umi_feature.h (finish.hip)
int  engine_umi_dedup_stats(EngineImpl* im, xck_umi_dedup_stats* out);   // umi_collapse.h (finish.hip)
int  base_tally_set_lengths(EngineImpl* im, const int64_t* len, int32_t n);   // base_tally.h (engine.hip)
int  engine_base_tally(EngineImpl* im, int32_t contig, int32_t pos0, int32_t n, uint32_t* out);
int  engine_base_tally_stats(EngineImpl* im, xck_base_tally_stats* out);
int  engine_find_candidates(EngineImpl* im, const xck_candidate_config* cfg, xck_candidates* out);
int  engine_find_candidates_ref(EngineImpl* im, const xck_candidate_config* cfg, xck_candidates* out, xck_candidate_ref_stats* st);
int  engine_set_contig_ref(EngineImpl* im, int32_t contig, const char* raw, int64_t n_raw, int32_t line_bases, int32_t line_width);   // ref_seq.h (engine.hip)
int  engine_get_contig_ref(EngineImpl* im, int32_t contig, int32_t pos0, int32_t n, char* out);
int  engine_base_tally_contigs(EngineImpl* im, uint8_t* has_table, int32_t n);
int  engine_device(const xck_engine* e);      // HIP device of the handle (-1: decode-only handle)
int  engine_numa_node(const xck_engine* e);   // NUMA node of the handle's GPU (sysfs, by PCI bus id); -1 = unknown
// One decoded chunk (all SoA columns in one pinned host block of `bytes` bytes at host_base; the batches point into it): ONE
// asynchronous H2D copy into a device staging slot shared by the handle's pipelines, then the join kernel(s) on the batches.
// *fence (created on first use) is recorded behind the copy: fence_wait() before the host block is overwritten.
// names (device-names mode): the chunk's packed read names lie in the block too; their keys are written into the staged umi column
// by the intern kernel, on the copy stream, before the batches are queued.
// qual (a handle with a base-quality floor): the block's quality column, inside the block, indexed by 2 * seq_off + query offset with the
// same offsets the batches' seq pointers are indexed by
int  engine_push_block(xck_engine* e, const void* host_base, size_t bytes, const xck_batch* batches, int n, void** fence, const NameTrailer* names = nullptr, const uint8_t* qual = nullptr);
// One chunk the device inflated and walked (parse_dev.h): the parse kernel writes the chunk's SoA block into the staging slot - no copy -
// and the batches follow as in engine_push_block.  1 = the kernel flagged the chunk and nothing was queued: the host path takes it.
struct GpuInflateSlot; struct DpBatch;
// chunk_bytes: the chunk's inflated size (device-names mode: a bound on its name bytes)
int  engine_push_parsed(xck_engine* e, const GpuInflateSlot* gs, size_t n_blocks, size_t max_rec, size_t n_out, size_t n_cig, size_t n_seq, int32_t sample, const DpBatch* batches, int n, size_t chunk_bytes);
// device-names mode: empty the handle's table (stream-ordered on the copy stream; waits for what is in flight there first);
// zero_stats (xck_reset): its counters start over too
int  engine_names_clear(xck_engine* e, bool zero_stats = false);
// ... wait for the intern kernels in flight and report what they flagged: 0, XCK_E_CAPACITY or XCK_E_DEVICE with e->err set
int  engine_names_check(xck_engine* e);
void engine_names_stats(const xck_engine* e, int64_t* interned, int64_t* distinct);
void engine_release_staging(xck_engine* e);   // frees the staging slots (xck_destroy)
void fence_wait(void* fence);
void fence_destroy(void* fence);
// xck_local_phase (local_phase.hip): api.cpp checks the problem and levels the regions, local_phase_run drives the device
struct PhasePlan {
    std::vector<int32_t> order;          // regions sorted by (level, index)
    std::vector<int32_t> level_beg;      // [n_levels + 1] into order
    int max_n = 0;                       // most slots of a region
    int max_e = 0;                       // most pileup entries under the slots of a region
};
int  local_phase_run(const xck_phase_problem* p, const PhasePlan& plan, double ms_prepare, xck_phase_result** out);
void local_phase_free(xck_phase_result* r);
void* pinned_alloc(size_t bytes);        // hipHostMalloc, falls back to malloc when no device
void  pinned_free(void* p);
}
