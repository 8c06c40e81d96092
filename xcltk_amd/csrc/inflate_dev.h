// inflate_dev.h - GPU raw-DEFLATE decoder for BGZF blocks (csrc/inflate_dev.hip): one wave per block.
#pragma once
#include <cstdint>
#include <hip/hip_runtime_api.h>

namespace xck {

struct DpRec; struct DpCnt; struct DpBase; struct DpBlockSum; struct DpHead;   // parse_dev.h

// byte ranges of one block's deflate stream / inflated data inside the chunk buffers; crc: the CRC-32 of the BGZF footer (read with check_crc only)
struct DevBlock { uint32_t in_off, in_len, out_off, out_len; uint32_t crc; };
constexpr int32_t INFLATE_ST_CRC = 50;   // status: the block was inflated to out_len bytes, but their CRC-32 is not DevBlock.crc (check_crc)

// Enqueue the inflate of n_blocks blocks: d_in (compressed bytes of the chunk), d_out (inflated bytes), d_status[b] = 0 when block b
// was inflated to exactly out_len bytes, non-zero when the block is left to the host decoder.  Returns 0 / -1 (launch error).
void dev_inflate_read_prof(unsigned long long out[8]);   // variant 10 (phase clocks): cycles per phase, summed over the blocks
int dev_inflate_launch(hipStream_t stream, const uint8_t* d_in, const DevBlock* d_blocks, int n_blocks, uint8_t* d_out, int32_t* d_status, uint8_t* host_out = nullptr, int variant = 0,
                       bool check_crc = false);
// host_out: device alias of a mapped host block that receives every finished block's bytes too; variant: 0 = the kernel, 10 = the same with
// phase clocks (bench harness only, dev_inflate_read_prof); check_crc: every inflated non-empty block's CRC-32 (zlib's crc32) is compared with
// DevBlock.crc - status INFLATE_ST_CRC when they differ (empty blocks are not checked, as on the host)

// workgroups (of one wave) of that instantiation the runtime fits on a CU (hipOccupancyMaxActiveBlocksPerMultiprocessor); -1 = no answer
int dev_inflate_occupancy(int variant = 0, bool check_crc = false);

// One chunk of BGZF blocks in flight on the GPU (the host decoder keeps a ring of these, csrc/bam.cpp): pinned host buffers for the
// compressed bytes, the block table, the inflated bytes and the per-block status; device twins; a stream and an event of its own,
// so that the chunks of a ring overlap on the device (the decoder needs thousands of blocks in flight to pay: one wave per block).
struct GpuInflateSlot {
    int device = -1; hipStream_t stream = nullptr; hipEvent_t done = nullptr; int variant = 0;   // (see dev_inflate_launch)
    // pinned + mapped host blocks (h_*) with their device aliases (a_*): the kernel reads the compressed bytes and the block table
    // straight from host memory and writes the statuses there; the inflated bytes are produced in HBM (d_out: match copies read
    // them back) and stored to h_out by the wave that made them, block by block - no DMA engine is involved (see gpu_inflate_slot_launch)
    uint8_t *h_in = nullptr, *a_in = nullptr, *h_out = nullptr, *a_out = nullptr, *d_out = nullptr; DevBlock *h_bl = nullptr, *a_bl = nullptr; int32_t *h_st = nullptr, *a_st = nullptr;
    size_t cap_in = 0, cap_out = 0, cap_bl = 0;
    // device walk + parse (csrc/parse_dev.hip): the chunk's record list, per-block counts and bases in device memory; the per-block
    // summaries and the chunk's head in mapped host memory, visible with `done`
    DpRec* d_rec = nullptr; DpCnt* d_cnt = nullptr; DpBase* d_base = nullptr; DpBlockSum *h_sum = nullptr, *a_sum = nullptr; DpHead *h_head = nullptr, *a_head = nullptr;
    uint32_t* d_nfilt = nullptr;         // device counter of the parse kernel: records the handle's tag filter rejected (zero between two parses: k_filtered_out)
    bool parse = false;                  // reserve the buffers above as well, and leave h_out unwritten (gpu_inflate_slot_launch)
};
GpuInflateSlot* gpu_inflate_slot_create(int device, int free_cus, bool verbose);           // nullptr when the device cannot be used; free_cus: CUs its stream never uses
void gpu_inflate_slot_destroy(GpuInflateSlot* s);                                          // waits for whatever is in flight
bool gpu_inflate_slot_reserve(GpuInflateSlot* s, size_t in_bytes, size_t out_bytes, size_t n_blocks);   // (re)allocates; false = out of memory
struct DpWalk;                                                                             // parse_dev.h: what the walk behind the inflate needs
int  gpu_inflate_slot_launch(GpuInflateSlot* s, size_t in_bytes, size_t out_bytes, size_t n_blocks, bool check_crc = false, const DpWalk* walk = nullptr);   // inflate kernel (every wave also stores its finished block to h_out; with `walk`: nothing goes to h_out, walk and scan follow) + event, asynchronous; 0 = enqueued
bool gpu_inflate_slot_done(GpuInflateSlot* s);                                            // non-blocking: has the last launch finished?
int  gpu_inflate_slot_wait(GpuInflateSlot* s);                                             // 0 = the chunk's bytes and statuses are in h_out / h_st

}  // namespace xck
