// Stand-ins for the engine, for programs that link the BAM decoder (csrc/bam.cpp, csrc/bam_records.cpp) or the C entry points
// (csrc/api.cpp) without it: a decode-only handle never reaches any of them, except the pinned block of a chunk's SoA (plain heap here,
// so that a sanitizer sees every overrun) and its fence.  Grouped by the unit that provides the real thing; a new engine_* call of the
// decoder gets its stand-in here and nowhere else.  (The device decoder's stand-ins: device_stubs.cpp.)
#include <cstdlib>
#include "../../xcltk_amd/csrc/xck_internal.h"

namespace xck {
// ---- csrc/engine.hip (the summary headers it includes) ----
int  engine_read_fate(EngineImpl*, xck_read_fate*) { return XCK_E_ARG; }
int  engine_cell_summary(EngineImpl*, xck_cell_summary*) { return XCK_E_ARG; }
int  engine_feature_summary(EngineImpl*, xck_feature_summary*) { return XCK_E_ARG; }
// ---- csrc/pipeline.hip ----
int  engine_create(const xck_config*, xck_engine*, EngineImpl**) { return XCK_E_ARG; }
void engine_destroy(EngineImpl*) {}
int  engine_push(EngineImpl*, const xck_batch*, bool, const uint8_t*) { return XCK_E_ARG; }
int  engine_baseq_stats(EngineImpl*, xck_baseq_stats*) { return XCK_E_ARG; }
int  engine_flush(EngineImpl*) { return XCK_E_ARG; }
int  engine_reset(EngineImpl*) { return XCK_E_ARG; }
int  engine_stats(const EngineImpl*, xck_stats*) { return XCK_E_ARG; }
int  engine_device(const xck_engine*) { return -1; }                          // no device: the decoder's GPU share of the inflate never starts
int  engine_numa_node(const xck_engine*) { return -1; }
// (weak: a program that wants to see the chunks a GPU-backed handle would get brings its own, tools/asan/decoder_asan.cpp)
__attribute__((weak)) int engine_push_block(xck_engine*, const void*, size_t, const xck_batch*, int, void**, const NameTrailer*, const uint8_t*) { return XCK_E_ARG; }
int  engine_push_parsed(xck_engine*, const GpuInflateSlot*, size_t, size_t, size_t, size_t, size_t, int32_t, const DpBatch*, int, size_t) { return XCK_E_ARG; }
int  engine_names_clear(xck_engine*, bool) { return 0; }
int  engine_names_check(xck_engine*) { return 0; }
void engine_names_stats(const xck_engine*, int64_t* interned, int64_t* distinct) { *interned = 0; *distinct = 0; }
void engine_release_staging(xck_engine*) {}
void fence_wait(void*) {}
void fence_destroy(void*) {}
void* pinned_alloc(size_t bytes) { return malloc(bytes ? bytes : 1); }
void  pinned_free(void* p) { free(p); }
// ---- csrc/finish.hip ----
int  engine_finish(EngineImpl*, xck_result*) { return XCK_E_ARG; }
int  engine_finish_async(EngineImpl*) { return XCK_E_ARG; }
int  engine_result_device(EngineImpl*, xck_result*) { return XCK_E_ARG; }
int  engine_refold(EngineImpl*, const xck_refold_config*, xck_result*) { return XCK_E_ARG; }
int  engine_snp_counts(EngineImpl*, xck_result*) { return XCK_E_ARG; }
int  engine_group_counts(EngineImpl*, int, int, const int32_t*, xck_result*, GroupTimes*) { return XCK_E_ARG; }
int  engine_molecule_stats(EngineImpl*, xck_molecule_stats*) { return XCK_E_ARG; }
int  engine_umi_feature_stats(EngineImpl*, xck_umi_feature_stats*) { return XCK_E_ARG; }
int  engine_umi_dedup_stats(EngineImpl*, xck_umi_dedup_stats*) { return XCK_E_ARG; }
int  base_tally_set_lengths(EngineImpl*, const int64_t*, int32_t) { return XCK_E_ARG; }
int  engine_base_tally(EngineImpl*, int32_t, int32_t, int32_t, uint32_t*) { return XCK_E_ARG; }
int  engine_base_tally_stats(EngineImpl*, xck_base_tally_stats*) { return XCK_E_ARG; }
int  engine_find_candidates(EngineImpl*, const xck_candidate_config*, xck_candidates*) { return XCK_E_ARG; }
int  engine_find_candidates_ref(EngineImpl*, const xck_candidate_config*, xck_candidates*, xck_candidate_ref_stats*) { return XCK_E_ARG; }
int  engine_set_contig_ref(EngineImpl*, int32_t, const char*, int64_t, int32_t, int32_t) { return XCK_E_ARG; }
int  engine_get_contig_ref(EngineImpl*, int32_t, int32_t, int32_t, char*) { return XCK_E_ARG; }
int  engine_base_tally_contigs(EngineImpl*, uint8_t*, int32_t) { return XCK_E_ARG; }
// ---- csrc/local_phase.hip ----
int  local_phase_run(const xck_phase_problem*, const PhasePlan&, double, xck_phase_result**) { return XCK_E_DEVICE; }
void local_phase_free(xck_phase_result*) {}
}
