// Stand-ins for the device decoder, for programs that link the BAM reader (csrc/bam.cpp) on a machine without a GPU: no slot is ever
// made, so no chunk goes to the device and nothing else here is reached.  Grouped by the unit that provides the real thing.
// (The engine's stand-ins: engine_stubs.cpp.)
#include "../../xcltk_amd/csrc/inflate_dev.h"
#include "../../xcltk_amd/csrc/parse_dev.h"

namespace xck {
// ---- csrc/inflate_dev.hip ----
GpuInflateSlot* gpu_inflate_slot_create(int, int, bool) { return nullptr; }
void gpu_inflate_slot_destroy(GpuInflateSlot*) {}
bool gpu_inflate_slot_reserve(GpuInflateSlot*, size_t, size_t, size_t) { return false; }
int  gpu_inflate_slot_launch(GpuInflateSlot*, size_t, size_t, size_t, bool, const DpWalk*) { return -1; }
int  gpu_inflate_slot_wait(GpuInflateSlot*) { return -1; }
bool gpu_inflate_slot_done(GpuInflateSlot*) { return true; }
// ---- csrc/parse_dev.hip ----
int  dev_parse_copy_out(GpuInflateSlot*, size_t) { return -1; }
void* dev_parse_upload(int, const void*, size_t, const void*, size_t) { return nullptr; }
void dev_parse_free(int, void*) {}
}
