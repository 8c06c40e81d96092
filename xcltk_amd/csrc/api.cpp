// api.cpp - C-ABI entry points of libxck.so (include/xck.h) except the BAM functions (bam.cpp).
#include <hip/hip_runtime_api.h>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>
#include "xck_internal.h"
#include "mtx_writer.h"

using namespace xck;

extern "C" {

const char* xck_version(void) { return XCK_VERSION_STR; }
int xck_abi_version(void) { return XCK_ABI_VERSION; }

int xck_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* xck_last_error(const xck_engine* e) { return e ? e->err.c_str() : get_thread_error(); }

// the environment knobs of a handle (include/xck.h "Environment"), read here and nowhere on the push / finish path
Knobs xck::Knobs::from_env() {
    Knobs k;
    auto str = [](const char* n) { const char* e = getenv(n); return e ? e : ""; };
    auto num = [](const char* n, long long d) { const char* e = getenv(n); return e && *e ? atoll(e) : d; };
    k.debug_timing = getenv("XCK_DEBUG_TIMING") != nullptr;
    k.fold_sort = !strcmp(str("XCK_FOLD"), "sort");
    k.fold_c = (int)num("XCK_FOLD_C", 0);
    k.fold_lgg = (int)num("XCK_FOLD_LGG", -1);
    k.fold_copies_lg = (int)num("XCK_FOLD_COPIES_LG", 4);
    k.fold_bucket_blocks = (int)num("XCK_FOLD_BUCKET_BLOCKS", 256 * 4 * 2);
    k.fold_overlap = (int)num("XCK_FOLD_OVERLAP", 1);
    k.fold_overlap_blocks = (int)num("XCK_FOLD_OVERLAP_BLOCKS", 512);
    k.full_sort = num("XCK_FULL_SORT", 0) != 0;
    k.pileup_radix = !strcmp(str("XCK_PILEUP_SORT"), "radix");
    k.pileup_hap = !strcmp(str("XCK_PILEUP_HAP"), "sorted") ? 1 : !strcmp(str("XCK_PILEUP_HAP"), "values") ? 2 : 0;
    k.pileup_lgg = (int)num("XCK_PILEUP_LGG", 10);
    k.hit_slack = std::max(0ll, num("XCK_HIT_SLACK", 65536));
    k.hit_cap0 = std::max(64ll, num("XCK_HIT_CAP0", 1ll << 20));
    k.push_stage = (int)num("XCK_PUSH_STAGE", -1);
    k.push_stage_bytes = num("XCK_PUSH_STAGE_BYTES", 2ll << 20);
    k.gpu_inflate_pct = (!*str("XCK_GPU_INFLATE") || !strcmp(str("XCK_GPU_INFLATE"), "auto")) ? -1 : (int)std::max(0ll, std::min(100ll, num("XCK_GPU_INFLATE", 0)));
    k.gpu_parse = strcmp(str("XCK_GPU_PARSE"), "0") != 0;
    k.gpu_names = num("XCK_GPU_NAMES", 0) != 0;
    k.gpu_names_slots0 = std::max(64ll, std::min(1ll << 30, num("XCK_GPU_NAMES_SLOTS0", 1ll << 21)));
    k.gpu_names_arena0 = std::max(1024ll, std::min(8ll << 30, num("XCK_GPU_NAMES_ARENA0", 64ll << 20)));
    k.names_hash_bits = (int)std::max(0ll, std::min(63ll, num("XCK_TEST_NAMES_HASH_BITS", 0)));
    k.gpu_inflate_depth = (int)std::max(1ll, std::min(10ll, num("XCK_GPU_INFLATE_DEPTH", 10)));
    k.gpu_inflate_ring = (int)num("XCK_GPU_INFLATE_RING", 12);
    k.gpu_inflate_min_mb = (int)std::max(0ll, num("XCK_GPU_INFLATE_MIN_MB", 96));
    k.gpu_inflate_free_cus = (int)num("XCK_GPU_INFLATE_FREE_CUS", 32);
    k.verify_crc = !strcmp(str("XCK_VERIFY_CRC"), "device") ? 2 : (!*str("XCK_VERIFY_CRC") || !strcmp(str("XCK_VERIFY_CRC"), "0")) ? 0 : 1;   // (any other value: host)
    k.read_fate = num("XCK_READ_FATE", 0) != 0;
    k.cell_summary = num("XCK_CELL_SUMMARY", 0) != 0;
    k.feature_summary = num("XCK_FEATURE_SUMMARY", 0) != 0;
    k.umi_consensus = num("XCK_UMI_CONSENSUS", 0) != 0;
    if (*str("XCK_UMI_FEATURE")) {                                       // unique | all; anything else: -1, and xck_create quotes the text
        k.umi_feature_text = str("XCK_UMI_FEATURE");
        k.umi_feature = k.umi_feature_text == "unique" ? 1 : k.umi_feature_text == "all" ? 0 : -1;
    }
    if (*str("XCK_UMI_DEDUP")) {                                         // 1mm_all | exact; anything else: -1, and xck_create quotes the text
        k.umi_dedup_text = str("XCK_UMI_DEDUP");
        k.umi_dedup = k.umi_dedup_text == "1mm_all" ? 1 : k.umi_dedup_text == "exact" ? 0 : -1;
    }
    if (*str("XCK_MIN_BASEQ")) {                                         // decimal digits only, 0 .. 93; anything else: -1, and xck_create quotes the text
        k.min_baseq_text = str("XCK_MIN_BASEQ");
        const std::string& t = k.min_baseq_text;
        long long v = 0;
        bool ok = t.size() <= 3;
        for (char c : t) { ok = ok && c >= '0' && c <= '9'; v = v * 10 + (c - '0'); }
        k.min_baseq = ok && v <= 93 ? (int)v : -1;
    }
    k.ref_chunk_bytes = std::max(64ll, std::min(1ll << 30, num("XCK_REF_CHUNK_BYTES", 32ll << 20)));
    k.group_long_row = (int)std::max(1ll, std::min(64ll, num("XCK_GROUP_LONG_ROW", 64)));
    k.cell_summary_slots = (int)std::max(0ll, std::min(1ll << 20, num("XCK_CELL_SUMMARY_SLOTS", 0)));
    if (*str("XCK_TAG_FILTER")) {                                        // TAG:VALUE[/MASK], numbers decimal or 0x hex, MASK defaults to all ones
        k.tag_filter_text = str("XCK_TAG_FILTER");
        const char* s = k.tag_filter_text.c_str();
        // a number that fills its field up to `stop` (':' '/' or the end) and fits 32 bits
        auto u32 = [](const char* p, const char* stop, uint32_t* out) {
            const bool hex = stop - p > 2 && p[0] == '0' && (p[1] == 'x' || p[1] == 'X');
            if (hex) p += 2;
            if (p == stop || stop - p > 10) return false;
            uint64_t v = 0;
            for (; p < stop; p++) {
                const int d = *p >= '0' && *p <= '9' ? *p - '0' : hex && *p >= 'a' && *p <= 'f' ? *p - 'a' + 10 : hex && *p >= 'A' && *p <= 'F' ? *p - 'A' + 10 : -1;
                if (d < 0) return false;
                v = v * (hex ? 16 : 10) + (uint64_t)d;
            }
            if (v > 0xFFFFFFFFull) return false;
            *out = (uint32_t)v; return true;
        };
        const size_t len = k.tag_filter_text.size();
        const char* slash = strchr(s, '/'); const char* end = s + len;
        k.tag_filter_mask = 0xFFFFFFFFu;
        const bool ok = len >= 4 && s[2] == ':' && u32(s + 3, slash ? slash : end, &k.tag_filter_value) && (!slash || u32(slash + 1, end, &k.tag_filter_mask));
        k.tag_filter = ok ? 1 : -1;
        if (ok) { k.tag_filter_tag[0] = s[0]; k.tag_filter_tag[1] = s[1]; }
    }
    return k;
}

int xck_create(const xck_config* cfg_in, xck_engine** out) {
    if (!cfg_in || !out) { set_thread_error("null argument"); return XCK_E_ARG; }
    *out = nullptr;
    // ABI 1 structs (without the exclusion pairs) are accepted: the missing tail reads as zero
    // ... and so are those without the tag filter (they end where filter_tag begins): no filter from the struct
    // (min_baseq sits in what was the tail padding: the size did not change, and sizeof - 4 - where the field begins - is no accepted size)
    static_assert(offsetof(xck_config, min_baseq) == 172 && sizeof(xck_config) == 176, "min_baseq fills the old tail padding");
    if (cfg_in->struct_size != offsetof(xck_config, n_excl_pairs) && cfg_in->struct_size != offsetof(xck_config, filter_tag) && cfg_in->struct_size != sizeof(xck_config)) { set_thread_error("xck_config.struct_size mismatch (ABI)"); return XCK_E_ARG; }
    xck_config cfg_full; memset(&cfg_full, 0, sizeof cfg_full); memcpy(&cfg_full, cfg_in, cfg_in->struct_size); cfg_full.struct_size = sizeof(xck_config);
    // the bytes of min_baseq are a caller's padding unless it says otherwise (XCK_F_MIN_BASEQ); a struct that ends before the field cannot
    // say so - refused, not ignored: the caller asked for a floor and would get none
    if (cfg_in->struct_size > offsetof(xck_config, flags) && (cfg_full.flags & XCK_F_MIN_BASEQ) && cfg_in->struct_size != sizeof(xck_config)) {
        set_thread_error("XCK_F_MIN_BASEQ on an xck_config whose struct_size ends before min_baseq"); return XCK_E_ARG; }
    if (!(cfg_full.flags & XCK_F_MIN_BASEQ)) cfg_full.min_baseq = 0;
    const xck_config* cfg = &cfg_full;
    if (cfg->n_excl_pairs < 0 || (cfg->n_excl_pairs > 0 && (!cfg->excl_region || !cfg->excl_snp))) { set_thread_error("invalid exclusion pairs"); return XCK_E_ARG; }
    if (cfg->mode != XCK_MODE_BASEFC && cfg->mode != XCK_MODE_BAF && cfg->mode != XCK_MODE_BOTH) { set_thread_error("invalid mode"); return XCK_E_ARG; }
    if (cfg->n_cells <= 0 || cfg->n_contigs < 0 || cfg->n_regions < 0 || cfg->n_snps < 0) { set_thread_error("invalid table sizes"); return XCK_E_ARG; }
    if ((cfg->n_regions > 0 && !cfg->regions) || (cfg->n_snps > 0 && !cfg->snps)) { set_thread_error("null table pointer"); return XCK_E_ARG; }
    const struct { int flag; const char* name; } gpu_only[] = { { XCK_F_READ_FATE, "XCK_F_READ_FATE" }, { XCK_F_CELL_SUMMARY, "XCK_F_CELL_SUMMARY" }, { XCK_F_FEATURE_SUMMARY, "XCK_F_FEATURE_SUMMARY" } };
    for (const auto& g : gpu_only)
        if ((cfg->flags & g.flag) && (cfg->flags & XCK_F_DECODE_ONLY)) { set_thread_error(std::string(g.name) + " needs a GPU engine: not with XCK_F_DECODE_ONLY"); return XCK_E_ARG; }
    if (cfg->flags & XCK_F_UMI_CONSENSUS) {
        if (cfg->flags & XCK_F_DECODE_ONLY) { set_thread_error("XCK_F_UMI_CONSENSUS needs a GPU engine: not with XCK_F_DECODE_ONLY"); return XCK_E_ARG; }
        if (!(cfg->mode & XCK_MODE_BAF)) { set_thread_error("XCK_F_UMI_CONSENSUS: the handle has no BAF pipeline"); return XCK_E_ARG; }
    }
    if (cfg->flags & XCK_F_UNIQUE_FEATURE) {
        if (cfg->flags & XCK_F_DECODE_ONLY) { set_thread_error("XCK_F_UNIQUE_FEATURE needs a GPU engine: not with XCK_F_DECODE_ONLY"); return XCK_E_ARG; }
        if (!(cfg->mode & XCK_MODE_BASEFC)) { set_thread_error("XCK_F_UNIQUE_FEATURE: the handle has no basefc pipeline"); return XCK_E_ARG; }
    }
    if (cfg->flags & XCK_F_UMI_COLLAPSE) {
        if (cfg->flags & XCK_F_DECODE_ONLY) { set_thread_error("XCK_F_UMI_COLLAPSE needs a GPU engine: not with XCK_F_DECODE_ONLY"); return XCK_E_ARG; }
        if (!(cfg->mode & XCK_MODE_BASEFC)) { set_thread_error("XCK_F_UMI_COLLAPSE: the handle has no basefc pipeline"); return XCK_E_ARG; }
    }
    if (cfg->flags & XCK_F_BASE_TALLY) {
        if (cfg->flags & XCK_F_DECODE_ONLY) { set_thread_error("XCK_F_BASE_TALLY needs a GPU engine: not with XCK_F_DECODE_ONLY"); return XCK_E_ARG; }
        if (!(cfg->mode & XCK_MODE_BAF)) { set_thread_error("XCK_F_BASE_TALLY: the handle has no BAF pipeline"); return XCK_E_ARG; }
    }
    if (cfg->min_baseq) {
        if (cfg->min_baseq < 0 || cfg->min_baseq > 93) { set_thread_error("xck_config.min_baseq outside 0 .. 93"); return XCK_E_ARG; }
        if (cfg->flags & XCK_F_DECODE_ONLY) { set_thread_error("xck_config.min_baseq needs a GPU engine: not with XCK_F_DECODE_ONLY"); return XCK_E_ARG; }
        if (!(cfg->mode & XCK_MODE_BAF)) { set_thread_error("xck_config.min_baseq: the handle has no BAF pipeline"); return XCK_E_ARG; }
    }
    xck_engine* e = new xck_engine();
    e->knobs = Knobs::from_env();
    if (e->knobs.min_baseq < 0) { set_thread_error("malformed XCK_MIN_BASEQ \"" + e->knobs.min_baseq_text + "\": expected a number in 0 .. 93"); delete e; return XCK_E_ARG; }
    if (e->knobs.umi_feature < 0) { set_thread_error("malformed XCK_UMI_FEATURE \"" + e->knobs.umi_feature_text + "\": expected unique or all"); delete e; return XCK_E_ARG; }
    if (e->knobs.umi_dedup < 0) { set_thread_error("malformed XCK_UMI_DEDUP \"" + e->knobs.umi_dedup_text + "\": expected 1mm_all or exact"); delete e; return XCK_E_ARG; }
    // the tag filter: the struct's fields, or - where the struct carries none - the knob; checked before a device is touched
    {
        DecodeCfg& d = e->dec;
        auto bad = [&](const std::string& s) { set_thread_error(s); delete e; return XCK_E_ARG; };
        if (e->knobs.tag_filter < 0) return bad("malformed XCK_TAG_FILTER \"" + e->knobs.tag_filter_text + "\": expected TAG:VALUE[/MASK], e.g. xf:25 or xf:8/8");
        if (cfg->filter_tag[0]) { d.filter_on = true; d.filter_tag[0] = cfg->filter_tag[0]; d.filter_tag[1] = cfg->filter_tag[1]; d.filter_mask = cfg->filter_mask; d.filter_value = cfg->filter_value; }
        else if (e->knobs.tag_filter > 0) { d.filter_on = true; memcpy(d.filter_tag, e->knobs.tag_filter_tag, 2); d.filter_mask = e->knobs.tag_filter_mask; d.filter_value = e->knobs.tag_filter_value; }
        if (d.filter_on) {
            const char* src = cfg->filter_tag[0] ? "xck_config.filter_tag" : "XCK_TAG_FILTER";
            auto printable = [](char c) { return c > 0x20 && c < 0x7f; };
            if (!printable(d.filter_tag[0]) || !printable(d.filter_tag[1]) || (cfg->filter_tag[0] && cfg->filter_tag[2])) return bad(std::string(src) + ": the tag must be two printable characters");
            if ((cfg->barcodes && !memcmp(d.filter_tag, cfg->cell_tag, 2)) || (cfg->umi_tag[0] && !memcmp(d.filter_tag, cfg->umi_tag, 2)))
                return bad(std::string(src) + ": the filter tag is the handle's cell or UMI tag");
            if (d.filter_value & ~d.filter_mask) return bad(std::string(src) + ": value has bits outside the mask (no record could pass)");
        }
    }
    e->cell_summary = !(cfg->flags & XCK_F_DECODE_ONLY) && ((cfg->flags & XCK_F_CELL_SUMMARY) || e->knobs.cell_summary);
    e->feature_summary = !(cfg->flags & XCK_F_DECODE_ONLY) && ((cfg->flags & XCK_F_FEATURE_SUMMARY) || e->knobs.feature_summary);   // (does not imply the read summary)
    e->read_fate = !(cfg->flags & XCK_F_DECODE_ONLY) && ((cfg->flags & XCK_F_READ_FATE) || e->knobs.read_fate || e->cell_summary);
    e->umi_consensus = !(cfg->flags & XCK_F_DECODE_ONLY) && (cfg->mode & XCK_MODE_BAF) && ((cfg->flags & XCK_F_UMI_CONSENSUS) || e->knobs.umi_consensus);   // (the knob: ignored by the other handles)
    e->unique_feature = !(cfg->flags & XCK_F_DECODE_ONLY) && (cfg->mode & XCK_MODE_BASEFC) && ((cfg->flags & XCK_F_UNIQUE_FEATURE) || e->knobs.umi_feature > 0);   // (the knob: ignored by the other handles)
    e->umi_collapse = !(cfg->flags & XCK_F_DECODE_ONLY) && (cfg->mode & XCK_MODE_BASEFC) && ((cfg->flags & XCK_F_UMI_COLLAPSE) || e->knobs.umi_dedup > 0);   // (the knob: ignored by the other handles)
    e->min_baseq = cfg->min_baseq ? cfg->min_baseq : (!(cfg->flags & XCK_F_DECODE_ONLY) && (cfg->mode & XCK_MODE_BAF)) ? e->knobs.min_baseq : 0;   // (the knob: ignored by the other handles)
    e->base_tally = (cfg->flags & XCK_F_BASE_TALLY) != 0;              // (checked above: a BAF pipeline, a GPU engine; no knob)
    e->umi_bits = key_layout(cfg).ubits;
    e->mode = cfg->mode;
    e->n_cells = cfg->n_cells; e->n_contigs = cfg->n_contigs;
    if (!(cfg->flags & XCK_F_DECODE_ONLY)) {
        const int modes[2] = { cfg->mode == XCK_MODE_BOTH ? XCK_MODE_BASEFC : cfg->mode, XCK_MODE_BAF };
        const int n = cfg->mode == XCK_MODE_BOTH ? 2 : 1;
        for (int k = 0; k < n; k++) {
            xck_config c = *cfg;
            c.mode = modes[k];
            if (n == 2) c.flags |= XCK_F_LAYOUT_BOTH;          // one key layout -> one decode serves both pipelines
            if (e->read_fate) c.flags |= XCK_F_READ_FATE;      // (XCK_READ_FATE=1, or implied by the per-cell table)
            if (e->cell_summary) c.flags |= XCK_F_CELL_SUMMARY;  // (XCK_CELL_SUMMARY=1)
            if (e->feature_summary) c.flags |= XCK_F_FEATURE_SUMMARY;  // (XCK_FEATURE_SUMMARY=1)
            c.flags &= ~XCK_F_UMI_CONSENSUS;                   // the pileup pipeline's rule alone (XCK_UMI_CONSENSUS=1)
            if (e->umi_consensus && modes[k] == XCK_MODE_BAF) c.flags |= XCK_F_UMI_CONSENSUS;
            c.flags &= ~XCK_F_UNIQUE_FEATURE;                  // the basefc pipeline's rule alone (XCK_UMI_FEATURE=unique)
            if (e->unique_feature && modes[k] == XCK_MODE_BASEFC) c.flags |= XCK_F_UNIQUE_FEATURE;
            c.flags &= ~XCK_F_UMI_COLLAPSE;                    // the basefc pipeline's rule alone (XCK_UMI_DEDUP=1mm_all)
            if (e->umi_collapse && modes[k] == XCK_MODE_BASEFC) c.flags |= XCK_F_UMI_COLLAPSE;
            c.min_baseq = modes[k] == XCK_MODE_BAF ? e->min_baseq : 0;   // (XCK_MIN_BASEQ folded in)
            const int rc = engine_create(&c, e, &e->impls[k]);
            e->n_impl = k + 1;                                 // (a pipeline that failed half-way is destroyed with the rest)
            if (rc) { set_thread_error(e->err); xck_destroy(e); return rc; }
        }
    }
    // decoder settings
    DecodeCfg& d = e->dec;
    d.use_barcodes = cfg->barcodes != nullptr;
    if (d.use_barcodes) { d.build_barcodes(cfg->barcodes, cfg->n_cells); d.cell_tag[0] = cfg->cell_tag[0]; d.cell_tag[1] = cfg->cell_tag[1]; }
    d.use_umi = cfg->umi_tag[0] != 0;
    if (d.use_umi) { d.umi_tag[0] = cfg->umi_tag[0]; d.umi_tag[1] = cfg->umi_tag[1]; }
    d.umi_bits = e->umi_bits;
    d.want_seq = (cfg->mode & XCK_MODE_BAF) != 0;
    d.want_qual = e->min_baseq > 0;
    const int crc_flags = cfg->flags | (e->knobs.verify_crc == 2 ? XCK_F_DEVICE_CRC : e->knobs.verify_crc == 1 ? XCK_F_VERIFY_CRC : 0);
    d.verify_crc = (crc_flags & (XCK_F_VERIFY_CRC | XCK_F_DEVICE_CRC)) != 0;
    d.crc_on_device = (crc_flags & XCK_F_DEVICE_CRC) != 0;
    d.n_threads = cfg->n_threads;
    d.max_batch_reads = cfg->max_batch_reads;
    // device-names mode (XCK_GPU_NAMES=1): a handle with a GPU whose key is the read name, whose device chunks may be parsed on the
    // device (XCK_GPU_PARSE), for which the GPU share of the inflate is not off and whose barcodes all fit the device's table
    { bool fits = true; for (const std::string& bc : d.barcodes) fits = fits && bc.size() <= sizeof(DecodeCfg::BcSlot::key);
      e->names_mode = e->knobs.gpu_names && e->n_impl > 0 && !d.use_umi && e->knobs.gpu_parse && e->knobs.gpu_inflate_pct != 0 && (!d.verify_crc || d.crc_on_device) && fits; }
    *out = e;
    return XCK_OK;
}

// the one answer of every call that needs a pipeline to a handle that has none
static int no_engine(xck_engine* e) { e->err = "decode-only handle: no GPU engine behind it"; return XCK_E_STATE; }
// fn(pipeline) on every pipeline of the handle, up to the first error
static int for_pipelines(xck_engine* e, const std::function<int(EngineImpl*)>& fn) {
    if (e->n_impl <= 0) return no_engine(e);
    for (int k = 0; k < e->n_impl; k++) if (int rc = fn(e->impls[k])) return rc;
    return XCK_OK;
}
// the pipeline that xck_get_read_fate / xck_get_cell_summary / xck_get_feature_summary ask about, or null with e->err set
static EngineImpl* pipeline_of(xck_engine* e, int mode, const char* who) {
    if ((mode != XCK_MODE_BASEFC && mode != XCK_MODE_BAF) || !(e->mode & mode)) { e->err = std::string(who) + ": the handle has no such pipeline"; return nullptr; }
    return e->impls[e->mode == XCK_MODE_BOTH && mode == XCK_MODE_BAF ? 1 : 0];
}

void xck_destroy(xck_engine* e) {
    if (!e) return;
    for (int k = 0; k < 3; k++) {                                        // staging ring of xck_push_batch
        if (e->push_ring.fence[k]) { fence_wait(e->push_ring.fence[k]); fence_destroy(e->push_ring.fence[k]); }
        if (e->push_ring.blk[k]) pinned_free(e->push_ring.blk[k]);
    }
    for (int k = 0; k < e->n_impl; k++) engine_destroy(e->impls[k]);
    if (e->stager) engine_release_staging(e);
    delete e;
}
int xck_umi_bits(const xck_engine* e) { return e ? e->umi_bits : 0; }

// Host arrays handed in through the ABI are checked before any kernel sees them: an offset table that runs backwards or a
// column index outside the cell table would otherwise become an out-of-bounds access on the device or a row outside the
// result.  One linear pass over three of the columns; device-resident batches (xck_push_batch_device) are the caller's word.
static int check_host_batch(xck_engine* e, const xck_batch* b) {
    if (b->n_reads < 0) { e->err = "batch: negative n_reads"; return XCK_E_ARG; }
    if (b->contig < 0 || b->n_reads == 0) return XCK_OK;                       // skipped by the engine
    if (b->contig >= e->n_contigs) { e->err = "batch: contig id outside the configured contigs"; return XCK_E_ARG; }
    const bool seq = (e->mode & XCK_MODE_BAF) != 0;
    if (!b->pos || !b->flag || !b->mapq || !b->cell || !b->umi || !b->cig_off || (!b->cigar && b->cig_off[b->n_reads] != b->cig_off[0]) ||
        (seq && (!b->seq_off || (!b->seq && b->seq_off[b->n_reads] != b->seq_off[0])))) { e->err = "batch: null column"; return XCK_E_ARG; }
    const int64_t n = b->n_reads;
    uint32_t bad = 0;
    for (int64_t i = 0; i < n; i++) bad |= (uint32_t)(b->cig_off[i + 1] < b->cig_off[i]) | (uint32_t)(b->cell[i] >= e->n_cells);
    if (seq) for (int64_t i = 0; i < n; i++) bad |= (uint32_t)(b->seq_off[i + 1] < b->seq_off[i]);
    if (bad) { e->err = "batch: offsets run backwards or a cell index is outside the cell table"; return XCK_E_ARG; }
    return XCK_OK;
}
extern "C++" { namespace xck { int push_trusted(xck_engine* e, const xck_batch* b, const uint8_t* qual) { return for_pipelines(e, [&](EngineImpl* im) { return engine_push(im, b, false, qual); }); } } }
// what a push answers on a handle that keeps base tallies and has not been told its contigs' lengths
static int needs_lengths(xck_engine* e, const char* who) {
    e->err = std::string(who) + ": the handle keeps base tallies (XCK_F_BASE_TALLY) and has no contig lengths; call xck_set_contig_lengths first";
    return XCK_E_STATE;
}
// what the calls that carry no qualities answer on a handle whose pileup needs them
static int needs_qualities(xck_engine* e, const char* who) {
    e->err = std::string(who) + ": the handle has a base-quality floor (xck_config.min_baseq / XCK_MIN_BASEQ = " + std::to_string(e->min_baseq) + ") and this call carries no qualities; use xck_push_batch_q or xck_ingest_bam";
    return XCK_E_STATE;
}

// xck_push_batch, one-copy form for SMALL batches: the caller's nine arrays are packed into ONE engine-owned pinned block (ring of
// three), which crosses PCIe with ONE hipMemcpyAsync into a device staging slot shared by the handle's pipelines
// (engine_push_block - the path the BAM decoder uses).  The call returns as soon as the arrays are packed: the caller may reuse
// them, and the DMA of this batch overlaps the packing of the next one (the block's fence, an event, is waited for only when
// the ring comes round).  Measured on the MI355X box (tools/h2d_bench.py, profiles/r03_a_h2d_*): for batches of 4 M reads the
// direct form (engine_push: nine DMA copies straight from the caller's arrays + one wait) moves 0.86-1.05 G reads/s whether the
// arrays are pinned or plain numpy memory, the packed form 0.6 G reads/s (a host memcpy is slower than the DMA it saves) - so
// the packed form is used where the nine calls and the wait dominate: below XCK_PUSH_STAGE_BYTES (default 2 MB) per batch.
// XCK_PUSH_STAGE=0 / 1 forces one form.
static int push_staged(xck_engine* e, const xck_batch* b, const uint8_t* qual) {
    const bool seq = (e->mode & XCK_MODE_BAF) != 0;
    const size_t n = (size_t)b->n_reads;
    const uint32_t c_lo = b->cig_off[0], s_lo = seq ? b->seq_off[0] : 0;
    const size_t n_cig = b->cig_off[n] - c_lo, n_seq = seq ? b->seq_off[n] - s_lo : 0;
    struct Seg { const void* src; size_t bytes, off; } seg[10] = {
        { b->pos, n * 4, 0 }, { b->flag, n * 2, 0 }, { b->mapq, n, 0 }, { b->cell, n * 4, 0 }, { b->umi, n * 8, 0 }, { b->cig_off, (n + 1) * 4, 0 },
        { b->cigar ? b->cigar + c_lo : nullptr, n_cig * 4, 0 }, { seq ? b->seq_off : nullptr, seq ? (n + 1) * 4 : 0, 0 }, { seq && b->seq ? b->seq + s_lo : nullptr, n_seq, 0 },
        { qual, qual ? 2 * n_seq : 0, 0 } };                               // (a handle with a base-quality floor: the tenth column)
    size_t total = 0;
    for (auto& g : seg) { g.off = total; total += (g.bytes + 255) & ~size_t(255); }
    xck_engine::PushRing& ring = e->push_ring;
    const int k = ring.next; ring.next = (ring.next + 1) % 3;
    if (ring.fence[k]) fence_wait(ring.fence[k]);                        // the DMA that last read this block
    if (total > ring.cap[k]) {
        if (ring.blk[k]) pinned_free(ring.blk[k]);
        ring.cap[k] = 0;
        const size_t c = total + total / 4 + (1 << 16);
        ring.blk[k] = pinned_alloc(c);
        if (!ring.blk[k]) { e->err = "out of pinned host memory (xck_push_batch staging)"; return XCK_E_NOMEM; }
        ring.cap[k] = c;
    }
    char* base = (char*)ring.blk[k];
    // pack: the byte range [0, total) of the block is cut into equal parts, one per thread
    auto pack = [&](size_t lo, size_t hi) {
        for (const auto& g : seg) {
            if (!g.bytes || !g.src) continue;
            const size_t a = std::max(lo, g.off), z = std::min(hi, g.off + g.bytes);
            if (a < z) memcpy(base + a, (const char*)g.src + (a - g.off), z - a);
        }
    };
    const int nt = total < (size_t(4) << 20) ? 1 : std::min(4, std::max(1, default_threads()));
    if (nt == 1) pack(0, total);
    else {
        std::vector<std::thread> th;
        const size_t step = ((total + nt - 1) / nt + 63) & ~size_t(63);
        for (int t = 1; t < nt; t++) th.emplace_back(pack, std::min(total, step * t), std::min(total, step * (t + 1)));
        pack(0, std::min(total, step));
        for (auto& t : th) t.join();
    }
    xck_batch sb = *b;
    sb.pos = (const int32_t*)(base + seg[0].off); sb.flag = (const uint16_t*)(base + seg[1].off); sb.mapq = (const uint8_t*)(base + seg[2].off);
    sb.cell = (const int32_t*)(base + seg[3].off); sb.umi = (const uint64_t*)(base + seg[4].off); sb.cig_off = (const uint32_t*)(base + seg[5].off);
    sb.cigar = (const uint32_t*)(base + seg[6].off) - c_lo;               // rebased: never read below c_lo
    sb.seq_off = seq ? (const uint32_t*)(base + seg[7].off) : nullptr;
    sb.seq = seq ? (const uint8_t*)(base + seg[8].off) - s_lo : nullptr;
    return engine_push_block(e, base, total, &sb, 1, &ring.fence[k], nullptr, qual ? (const uint8_t*)(base + seg[9].off) - 2 * (size_t)s_lo : nullptr);
}
static int push_host_batch(xck_engine* e, const xck_batch* b, const uint8_t* qual) {
    if (int rc = check_host_batch(e, b)) return rc;
    if (b->n_reads <= 0 || b->contig < 0 || e->n_impl <= 0) return push_trusted(e, b, qual);     // nothing to copy / decode-only: reported there
    const int force = e->knobs.push_stage;
    const long long small = e->knobs.push_stage_bytes;
    const size_t n = (size_t)b->n_reads;
    // (the join addresses a quality byte as 2 * sequence offset + query offset in 32 bits)
    if (qual && (e->mode & XCK_MODE_BAF) && b->seq_off[n] >= (1u << 31)) { e->err = "xck_push_batch_q: sequence offsets of 2^31 and above"; return XCK_E_ARG; }
    const size_t bytes = n * 27 + (size_t)(b->cig_off[n] - b->cig_off[0]) * 4 + ((e->mode & XCK_MODE_BAF) ? n * 4 + (b->seq_off[n] - b->seq_off[0]) : 0);
    const bool stage = force >= 0 ? force != 0 : (long long)bytes < small;
    return stage ? push_staged(e, b, qual) : push_trusted(e, b, qual);
}
int xck_push_batch(xck_engine* e, const xck_batch* b) {
    if (!e || !b) return XCK_E_ARG;
    if (e->base_tally && !e->contig_len_set) return needs_lengths(e, "xck_push_batch");
    if (e->min_baseq > 0) return needs_qualities(e, "xck_push_batch");
    return push_host_batch(e, b, nullptr);
}
int xck_push_batch_q(xck_engine* e, const xck_batch* b, const uint8_t* qual) {
    if (!e || !b) return XCK_E_ARG;
    if (e->base_tally && !e->contig_len_set) return needs_lengths(e, "xck_push_batch_q");
    if (e->min_baseq <= 0) return push_host_batch(e, b, nullptr);        // no floor: qual is ignored
    if (!qual) {                                                         // (only a batch without sequence bytes needs none: a byte that is never read stands in)
        static const uint8_t none = 0xff;
        const bool empty = b->n_reads <= 0 || b->contig < 0 || (b->seq_off && b->seq_off[b->n_reads] == b->seq_off[0]);
        if (!empty) { e->err = "xck_push_batch_q: null qual on a handle with a base-quality floor"; return XCK_E_ARG; }
        qual = &none;
    }
    return push_host_batch(e, b, qual);
}
int xck_push_batch_device(xck_engine* e, const xck_batch* b) {
    if (!e || !b) return XCK_E_ARG;
    if (e->base_tally && !e->contig_len_set) return needs_lengths(e, "xck_push_batch_device");
    if (e->min_baseq > 0) return needs_qualities(e, "xck_push_batch_device");
    return for_pipelines(e, [&](EngineImpl* im) { return engine_push(im, b, true); });
}
int xck_flush(xck_engine* e) { if (!e) return XCK_E_ARG; return for_pipelines(e, engine_flush); }
int xck_reset(xck_engine* e) {
    if (!e) return XCK_E_ARG;
    for (auto& v : e->dstat) v = 0;
    if (int rc = for_pipelines(e, engine_reset)) return rc;
    e->gpu_inflate_chunks = 0;
    if (e->names_mode) {                                                 // the device table is cleared where the host's is; the two kinds of decode call may start over
        if (int rc = engine_names_clear(e, true)) return rc;
        e->names_calls = 0;
    }
    return XCK_OK;
}

int xck_get_decode_stats(const xck_engine* e, xck_decode_stats* out) {
    if (!e || !out) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (out->struct_size < offsetof(xck_decode_stats, gpu_parse_chunks)) { set_thread_error("xck_decode_stats.struct_size mismatch (ABI)"); return XCK_E_ARG; }
    int64_t* f[DS_N] = { &out->gpu_inflate_chunks, &out->gpu_inflate_blocks, &out->gpu_blocks_left_to_host, &out->crc_blocks_device, &out->crc_blocks_host,
                         &out->crc_mismatch_device, &out->crc_device_host_disagree, &out->gpu_path_given_up, &out->gpu_parse_chunks, &out->gpu_parse_fallbacks,
                         &out->gpu_names_interned, &out->gpu_names_distinct, &out->gpu_names_host_chunks, &out->tag_filtered };
    // (gpu_parse_*, then gpu_names_*, then tag_filtered were appended: a caller built before them passes the shorter struct and gets what it knows)
    const int n = out->struct_size >= sizeof(xck_decode_stats) ? DS_N : out->struct_size >= offsetof(xck_decode_stats, tag_filtered) ? DS_TAG_FILTERED
                : out->struct_size >= offsetof(xck_decode_stats, gpu_names_interned) ? DS_NAMES_INTERNED : DS_PARSE_CHUNKS;
    for (int k = 0; k < n; k++) *f[k] = e->dstat[k].load();
    if (n > DS_NAMES_INTERNED) engine_names_stats(e, &out->gpu_names_interned, &out->gpu_names_distinct);   // (the table's own counters)
    return XCK_OK;
}

// xck_get_read_fate / xck_get_cell_summary / xck_get_feature_summary: T the struct ("xck_<what>"), kept the handle's switch ("XCK_F_<FLAG>")
extern "C++" {                                            // (a template cannot have C linkage)
template <class T>
static int get_summary(xck_engine* e, int mode, T* out, bool xck_engine::*kept, const char* what, const char* flag, int (*get)(EngineImpl*, T*)) {
    if (!e || !out) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (out->struct_size < sizeof(T)) { e->err = std::string("xck_") + what + ".struct_size mismatch (ABI)"; return XCK_E_ARG; }
    if (!(e->*kept) || e->n_impl <= 0) { e->err = std::string("handle made without XCK_F_") + flag; return XCK_E_STATE; }
    EngineImpl* im = pipeline_of(e, mode, (std::string("xck_get_") + what).c_str());
    if (!im) return XCK_E_ARG;
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out); out->struct_size = sz;
    return get(im, out);
}
}
int xck_get_read_fate(xck_engine* e, int mode, xck_read_fate* out) { return get_summary(e, mode, out, &xck_engine::read_fate, "read_fate", "READ_FATE", engine_read_fate); }
int xck_get_cell_summary(xck_engine* e, int mode, xck_cell_summary* out) { return get_summary(e, mode, out, &xck_engine::cell_summary, "cell_summary", "CELL_SUMMARY", engine_cell_summary); }
int xck_get_feature_summary(xck_engine* e, int mode, xck_feature_summary* out) { return get_summary(e, mode, out, &xck_engine::feature_summary, "feature_summary", "FEATURE_SUMMARY", engine_feature_summary); }

int xck_get_umi_feature_stats(xck_engine* e, xck_umi_feature_stats* out) {
    if (!e || !out) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (out->struct_size < sizeof(xck_umi_feature_stats)) { e->err = "xck_umi_feature_stats.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    if (!e->unique_feature || e->n_impl <= 0) { e->err = "handle made without XCK_F_UNIQUE_FEATURE"; return XCK_E_STATE; }
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out); out->struct_size = sz;
    return engine_umi_feature_stats(e->impls[0], out);                  // (a fused handle answers from its basefc pipeline)
}

int xck_get_umi_dedup_stats(xck_engine* e, xck_umi_dedup_stats* out) {
    if (!e || !out) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (out->struct_size < sizeof(xck_umi_dedup_stats)) { e->err = "xck_umi_dedup_stats.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    if (!e->umi_collapse || e->n_impl <= 0) { e->err = "handle made without XCK_F_UMI_COLLAPSE"; return XCK_E_STATE; }
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out); out->struct_size = sz;
    return engine_umi_dedup_stats(e->impls[0], out);                    // (a fused handle answers from its basefc pipeline)
}

int xck_get_molecule_stats(xck_engine* e, xck_molecule_stats* out) {
    if (!e || !out) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (out->struct_size < sizeof(xck_molecule_stats)) { e->err = "xck_molecule_stats.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    if (!e->umi_consensus || e->n_impl <= 0) { e->err = "handle made without XCK_F_UMI_CONSENSUS"; return XCK_E_STATE; }
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out); out->struct_size = sz;
    return engine_molecule_stats(e->impls[e->n_impl - 1], out);         // (a fused handle answers from its pileup pipeline)
}

int xck_get_baseq_stats(xck_engine* e, xck_baseq_stats* out) {
    if (!e || !out) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (out->struct_size < sizeof(xck_baseq_stats)) { e->err = "xck_baseq_stats.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    if (e->min_baseq <= 0 || e->n_impl <= 0) { e->err = "handle made without a base-quality floor (xck_config.min_baseq / XCK_MIN_BASEQ)"; return XCK_E_STATE; }
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out); out->struct_size = sz;
    return engine_baseq_stats(e->impls[e->n_impl - 1], out);            // (a fused handle answers from its pileup pipeline)
}

// ---- pseudo-bulk base tallies (XCK_F_BASE_TALLY, base_tally.h): the handle's pileup pipeline keeps them ----
static EngineImpl* tally_pipeline(xck_engine* e) {
    if (!e->base_tally || e->n_impl <= 0) { e->err = "handle made without XCK_F_BASE_TALLY"; return nullptr; }
    return e->impls[e->n_impl - 1];                                      // (a fused handle answers from its pileup pipeline)
}
int xck_set_contig_lengths(xck_engine* e, const int64_t* len, int32_t n) {
    if (!e) { set_thread_error("null argument"); return XCK_E_ARG; }
    EngineImpl* im = tally_pipeline(e);
    if (!im) return XCK_E_STATE;
    // (the handle's first pipeline sees every push the pileup pipeline sees: "after the first push" is asked of the tally's own)
    if (int rc = base_tally_set_lengths(im, len, n)) return rc;
    e->contig_len_set = true;
    return XCK_OK;
}
int xck_get_base_tally(xck_engine* e, int32_t contig, int32_t pos0, int32_t n, uint32_t* out) {
    if (!e) { set_thread_error("null argument"); return XCK_E_ARG; }
    EngineImpl* im = tally_pipeline(e);
    return im ? engine_base_tally(im, contig, pos0, n, out) : XCK_E_STATE;
}
int xck_get_base_tally_stats(xck_engine* e, xck_base_tally_stats* out) {
    if (!e || !out) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (out->struct_size < sizeof(xck_base_tally_stats)) { e->err = "xck_base_tally_stats.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    EngineImpl* im = tally_pipeline(e);
    if (!im) return XCK_E_STATE;
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out); out->struct_size = sz;
    return engine_base_tally_stats(im, out);
}
int xck_find_candidates(xck_engine* e, const xck_candidate_config* cfg, xck_candidates* out) {
    if (!e) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (!cfg || !out) { e->err = "xck_find_candidates: null argument"; return XCK_E_ARG; }
    if (cfg->struct_size < sizeof(xck_candidate_config)) { e->err = "xck_candidate_config.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    EngineImpl* im = tally_pipeline(e);
    if (!im) return XCK_E_STATE;
    memset(out, 0, sizeof *out);
    return engine_find_candidates(im, cfg, out);
}
int xck_find_candidates_ref(xck_engine* e, const xck_candidate_config* cfg, xck_candidates* out, xck_candidate_ref_stats* st) {
    if (!e) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (!cfg || !out || !st) { e->err = "xck_find_candidates_ref: null argument"; return XCK_E_ARG; }
    if (cfg->struct_size < sizeof(xck_candidate_config)) { e->err = "xck_candidate_config.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    if (st->struct_size < sizeof(xck_candidate_ref_stats)) { e->err = "xck_candidate_ref_stats.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    EngineImpl* im = tally_pipeline(e);
    if (!im) return XCK_E_STATE;
    const uint32_t sz = st->struct_size;
    memset(out, 0, sizeof *out); memset(st, 0, sizeof *st); st->struct_size = sz;
    return engine_find_candidates_ref(im, cfg, out, st);
}
int xck_set_contig_ref(xck_engine* e, int32_t contig, const char* raw, int64_t n_raw, int32_t line_bases, int32_t line_width) {
    if (!e) { set_thread_error("null argument"); return XCK_E_ARG; }
    EngineImpl* im = tally_pipeline(e);
    return im ? engine_set_contig_ref(im, contig, raw, n_raw, line_bases, line_width) : XCK_E_STATE;
}
int xck_get_contig_ref(xck_engine* e, int32_t contig, int32_t pos0, int32_t n, char* out) {
    if (!e) { set_thread_error("null argument"); return XCK_E_ARG; }
    EngineImpl* im = tally_pipeline(e);
    return im ? engine_get_contig_ref(im, contig, pos0, n, out) : XCK_E_STATE;
}
int xck_get_base_tally_contigs(xck_engine* e, uint8_t* has_table, int32_t n) {
    if (!e) { set_thread_error("null argument"); return XCK_E_ARG; }
    EngineImpl* im = tally_pipeline(e);
    return im ? engine_base_tally_contigs(im, has_table, n) : XCK_E_STATE;
}

int xck_finish_async(xck_engine* e) { if (!e) return XCK_E_ARG; return for_pipelines(e, engine_finish_async); }

// the handle's result from those of its pipelines (get: engine_finish or engine_result_device): a fused handle takes the count matrix
// of its basefc pipeline and the three allele matrices of its pileup pipeline
static int merged_result(xck_engine* e, xck_result* out, int (*get)(EngineImpl*, xck_result*)) {
    memset(out, 0, sizeof *out);
    int k = 0;
    return for_pipelines(e, [&](EngineImpl* im) -> int {
        xck_result r;
        if (int rc = get(im, &r)) return rc;
        if (e->mode != XCK_MODE_BOTH) *out = r;
        else if (k++ == 0) out->count = r.count;
        else { out->ad = r.ad; out->dp = r.dp; out->oth = r.oth; }
        return XCK_OK;
    });
}
int xck_finish(xck_engine* e, xck_result* out) { if (!e || !out) return XCK_E_ARG; return merged_result(e, out, engine_finish); }
int xck_get_result_device(xck_engine* e, xck_result* out) { if (!e || !out) return XCK_E_ARG; return merged_result(e, out, engine_result_device); }

int xck_refold(xck_engine* e, const xck_refold_config* cfg, xck_result* out) {
    if (!e || !cfg || !out) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (e->n_impl <= 0) return no_engine(e);
    if (!(e->mode & XCK_MODE_BAF)) { e->err = "xck_refold: the handle has no BAF pipeline (a basefc recount needs the reads)"; return XCK_E_ARG; }
    if (cfg->struct_size < XCK_REFOLD_CONFIG_SIZE_V1) { e->err = "xck_refold_config.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    xck_refold_config full;                                // the fields the caller's struct_size covers; the appended ones NULL
    memset(&full, 0, sizeof full);
    memcpy(&full, cfg, std::min<size_t>(cfg->struct_size, sizeof full));
    xck_result r;
    if (int rc = engine_refold(e->impls[e->n_impl - 1], &full, &r)) return rc;
    if (e->mode == XCK_MODE_BOTH) {                        // the count matrix is the last finish's, untouched
        xck_result c;
        if (int rc = engine_finish(e->impls[0], &c)) return rc;
        r.count = c.count;
    }
    *out = r;
    return XCK_OK;
}

int xck_snp_counts(xck_engine* e, xck_result* out) {
    if (!e) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (!out) { e->err = "xck_snp_counts: null result"; return XCK_E_ARG; }
    if (e->n_impl <= 0) return no_engine(e);
    if (!(e->mode & XCK_MODE_BAF)) { e->err = "xck_snp_counts: the handle has no BAF pipeline"; return XCK_E_ARG; }
    return engine_snp_counts(e->impls[e->n_impl - 1], out);              // (a fused handle answers from its pileup pipeline)
}

// The handle's matrices summed per cell group (group_counts.h).  Everything that can be wrong with the arguments is found here, before the
// device is touched; a fused handle answers from both pipelines, each with buffers of its own.
int xck_group_counts(xck_engine* e, const xck_group_config* cfg, xck_result* out) {
    if (!e) { set_thread_error("null argument"); return XCK_E_ARG; }
    if (!cfg || !out) { e->err = "xck_group_counts: null argument"; return XCK_E_ARG; }
    if (cfg->struct_size < sizeof(xck_group_config)) { e->err = "xck_group_config.struct_size mismatch (ABI)"; return XCK_E_ARG; }
    if (e->n_impl <= 0) return no_engine(e);
    if (cfg->source != XCK_GROUP_SRC_RESULT && cfg->source != XCK_GROUP_SRC_SNP) { e->err = "xck_group_counts: unknown source"; return XCK_E_ARG; }
    if (cfg->source == XCK_GROUP_SRC_SNP && !(e->mode & XCK_MODE_BAF)) { e->err = "xck_group_counts: source SNP on a handle without a BAF pipeline"; return XCK_E_ARG; }
    if (cfg->n_groups < 1 || cfg->n_groups > XCK_GROUP_MAX) { e->err = "xck_group_counts: n_groups outside 1 .. XCK_GROUP_MAX"; return XCK_E_ARG; }
    if (!cfg->cell_group) { e->err = "xck_group_counts: null cell_group"; return XCK_E_ARG; }
    { uint32_t bad = 0;
      for (int32_t c = 0; c < e->n_cells; c++) bad |= (uint32_t)(cfg->cell_group[c] < -1) | (uint32_t)(cfg->cell_group[c] >= cfg->n_groups);
      if (bad) { e->err = "xck_group_counts: a cell_group entry outside -1 .. n_groups - 1"; return XCK_E_ARG; } }
    xck_result r; memset(&r, 0, sizeof r);
    GroupTimes gt;
    const int k0 = cfg->source == XCK_GROUP_SRC_SNP ? e->n_impl - 1 : 0;  // (the SNP x cell blocks are the pileup pipeline's)
    for (int k = k0; k < e->n_impl; k++)
        if (int rc = engine_group_counts(e->impls[k], cfg->source, cfg->n_groups, cfg->cell_group, &r, &gt)) return rc;
    if (e->knobs.debug_timing)
        fprintf(stderr, "[xck] group_counts: source %s, %d groups: total %.3f ms (host clock to the stream synchronise): row pointers %.3f, count + scans %.3f, emit %.3f; "
                        "wait for the copy-out %.3f; %lld entries, nnz %lld / %lld / %lld / %lld\n", cfg->source == XCK_GROUP_SRC_SNP ? "snp" : "result", cfg->n_groups,
                gt.ms_total, gt.ms_ptr, gt.ms_count, gt.ms_emit, gt.ms_copy, gt.entries, gt.nnz[0], gt.nnz[1], gt.nnz[2], gt.nnz[3]);
    *out = r;
    return XCK_OK;
}

// Region-wise local phasing on the device (local_phase.hip).  Everything that can be wrong with the arguments is found here, before
// the device is touched; the levels are made here too: a region reads the SNP state that the earlier regions sharing a SNP left.
int xck_local_phase(const xck_phase_problem* p, xck_phase_result** out) {
    if (out) *out = nullptr;
    if (!p || !out) { set_thread_error("xck_local_phase: null argument"); return XCK_E_ARG; }
    const auto t0 = std::chrono::steady_clock::now();
    auto bad = [](const std::string& s) { set_thread_error("xck_local_phase: " + s); return XCK_E_ARG; };
    if (p->struct_size < sizeof(xck_phase_problem)) return bad("xck_phase_problem.struct_size mismatch (ABI)");
    if (p->n_cells <= 0 || p->n_cols < 0 || p->n_snps < 0 || p->n_regions < 0) return bad("invalid table sizes");
    if (!p->col_ptr || !p->reg_ptr) return bad("null pointer array");
    if (p->col_ptr[0] != 0 || p->reg_ptr[0] != 0) return bad("pointer arrays must start at 0");
    for (int32_t c = 0; c < p->n_cols; c++) if (p->col_ptr[c + 1] < p->col_ptr[c]) return bad("col_ptr runs backwards");
    for (int32_t r = 0; r < p->n_regions; r++) if (p->reg_ptr[r + 1] < p->reg_ptr[r]) return bad("reg_ptr runs backwards");
    const int64_t nnz = p->col_ptr[p->n_cols], n_slots = p->reg_ptr[p->n_regions];
    if ((nnz > 0 && (!p->cell || !p->ad || !p->dp)) || (n_slots > 0 && (!p->slot_col || !p->slot_snp || !p->slot_pos)) || (p->n_snps > 0 && (!p->ref_hap || !p->alt_hap)))
        return bad("null table pointer");
    for (int32_t c = 0; c < p->n_cols; c++)
        for (int64_t i = p->col_ptr[c]; i < p->col_ptr[c + 1]; i++) {
            if (p->cell[i] < 0 || p->cell[i] >= p->n_cells) return bad("cell index outside the table");
            if (i > p->col_ptr[c] && p->cell[i] <= p->cell[i - 1]) return bad("cells of a column are not strictly ascending");
            if (p->ad[i] < 0 || p->ad[i] > p->dp[i]) return bad("ad outside [0, dp]");
        }
    for (int32_t s = 0; s < p->n_snps; s++) if ((p->ref_hap[s] | p->alt_hap[s]) & ~1) return bad("haplotype index other than 0 / 1");
    PhasePlan plan;
    std::vector<int32_t> snp_level(p->n_snps, -1), snp_region(p->n_snps, -1), level(p->n_regions, 0);
    int n_levels = 0;
    for (int32_t r = 0; r < p->n_regions; r++) {
        int64_t entries = 0;
        int lv = 0;
        for (int64_t s = p->reg_ptr[r]; s < p->reg_ptr[r + 1]; s++) {
            const int32_t col = p->slot_col[s], snp = p->slot_snp[s];
            if (col < -1 || col >= p->n_cols) return bad("slot column outside the pileup");
            if (snp < 0 || snp >= p->n_snps) return bad("slot SNP outside the list");
            if (snp_region[snp] == r) return bad("a SNP twice in one region");
            snp_region[snp] = r;
            lv = std::max(lv, snp_level[snp] + 1);
            if (col >= 0) entries += p->col_ptr[col + 1] - p->col_ptr[col];
        }
        if (p->reg_ptr[r + 1] - p->reg_ptr[r] > INT32_MAX || entries > INT32_MAX) return bad("region too large");
        for (int64_t s = p->reg_ptr[r]; s < p->reg_ptr[r + 1]; s++) snp_level[p->slot_snp[s]] = lv;
        level[r] = lv;
        n_levels = std::max(n_levels, lv + 1);
        plan.max_n = std::max(plan.max_n, (int)(p->reg_ptr[r + 1] - p->reg_ptr[r]));
        plan.max_e = std::max(plan.max_e, (int)entries);
    }
    plan.level_beg.assign(n_levels + 1, 0);
    for (int32_t r = 0; r < p->n_regions; r++) plan.level_beg[level[r] + 1]++;
    for (int l = 0; l < n_levels; l++) plan.level_beg[l + 1] += plan.level_beg[l];
    plan.order.resize(p->n_regions);
    { std::vector<int32_t> cur(plan.level_beg.begin(), plan.level_beg.end() - 1); for (int32_t r = 0; r < p->n_regions; r++) plan.order[cur[level[r]]++] = r; }
    const double ms_prepare = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return local_phase_run(p, plan, ms_prepare, out);
}

void xck_free_phase_result(xck_phase_result* r) { local_phase_free(r); }

int xck_get_stats(const xck_engine* e, xck_stats* out) {
    if (!e || !out) return XCK_E_ARG;
    if (e->n_impl == 0) return XCK_E_STATE;
    memset(out, 0, sizeof *out);
    for (int k = 0; k < e->n_impl; k++) {
        xck_stats s;
        if (int rc = engine_stats(e->impls[k], &s)) return rc;
        if (k == 0) *out = s;
        else { out->n_hits += s.n_hits; out->n_hits_unique += s.n_hits_unique; out->ms_h2d += s.ms_h2d; out->ms_device += s.ms_device;
               out->ms_join += s.ms_join; out->ms_sort += s.ms_sort; out->ms_d2h += s.ms_d2h; out->algo_bytes_join += s.algo_bytes_join; out->n_join_launches += s.n_join_launches; }
    }
    return XCK_OK;
}

// ---- MatrixMarket text (merge_mtx(), rdr/fc/utils.py:54-93: byte-identical): csrc/mtx_writer.cpp ----
int xck_write_mtx(const char* path, const xck_coo* m, const int32_t* row_map, int32_t n_rows_out, int32_t n_cols) {
    if (!path || !m || !row_map) return XCK_E_ARG;
    std::string err;
    const int rc = mtx_write_file(path, m, row_map, n_rows_out, n_cols, default_threads(), &err);
    if (rc) set_thread_error(err);
    return rc;
}

// One process's piece of a file that several processes write together (multi-GPU run on one node: every rank owns rows and
// writes their lines itself; sizes are exchanged first, so every piece knows its offset).
int xck_mtx_part_size(const xck_coo* m, const int32_t* row_map, int64_t* n_bytes, int64_t* n_lines) {
    if (!m || !row_map || !n_bytes || !n_lines) return XCK_E_ARG;
    const int64_t ch = mtx_chunk_entries();
    mtx_measure(m, row_map, ch, mtx_threads(default_threads(), (m->nnz + ch - 1) / ch), n_lines, n_bytes);
    return XCK_OK;
}
int xck_write_mtx_part(const char* path, int64_t offset, const xck_coo* m, const int32_t* row_map) {
    if (!path || !m || !row_map || offset < 0) return XCK_E_ARG;
    std::string err;
    const int rc = mtx_write_part(path, offset, m, row_map, default_threads(), &err);
    if (rc) set_thread_error(err);
    return rc;
}

}  // extern "C"
