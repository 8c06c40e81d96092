// mtx_writer.h - MatrixMarket text of a COO result (merge_mtx(), rdr/fc/utils.py:54-93: byte-identical), behind xck_write_mtx,
// xck_mtx_part_size and xck_write_mtx_part (api.cpp).  Host code only, nothing of the engine: tools/asan/mtx_writer_check.cpp
// builds this unit alone.
//
// Two ways into the file:
//   pipeline   threads format ahead into a small ring of buffers, the calling thread drains them in file order with pwrite (write on a
//              descriptor that cannot seek): the bound is the one copy into the page cache, which an inode takes from one thread at a
//              time anyway.  The default, and the only way for what is not a regular file and for xck_write_mtx_part (ranks share
//              the first and last page of their ranges).
//   mapped     XCK_WRITE_MAP=1: sizes first (mtx_layout: per chunk the kept lines and the exact bytes of their text, prefix-summed into
//              file offsets), the file allocated at its final size (fallocate), mapped MAP_SHARED, and every thread formats its
//              chunks straight at base + off[chunk] (mtx_fill): no buffers, no write calls.  Faster on tmpfs; on a disk file system
//              the write faults of sixteen threads on one file cost several times the copy they save (measured on overlayfs:
//              profiles/r30_mtx_mapped_writer.txt), hence opt-in.
//              Regular files only; where the allocation fails the pipeline takes over.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include <sys/types.h>
#include "../../include/xck.h"

namespace xck {

// the text of one matrix laid out in its file: chunks of `ch` entries, off[c] = file offset of chunk c's first byte
struct MtxLayout {
    int64_t ch = 0, n_chunks = 0;
    int64_t lines = 0;                   // kept entries (row_map > 0): the header's nnz
    std::vector<int64_t> off;            // [n_chunks + 1]; off[0] = header_len, off[n_chunks] = the file's size
    char header[96]; int header_len = 0;
    int64_t size() const { return off.empty() ? header_len : off.back(); }
};

struct MtxTimes { double ms_open = 0, ms_sizes = 0, ms_alloc = 0, ms_fill = 0, ms_format_cpu = 0, ms_pwrite = 0, ms_drain_wait = 0; };

int64_t  mtx_chunk_entries();                                          // XCK_WRITE_CHUNK_ENTRIES (default 256 k)
unsigned mtx_threads(int default_threads, int64_t n_chunks);           // XCK_WRITE_THREADS (default: default_threads, at most 16)

// lines and bytes of the "row\tcol\tval\n" text of m (no header)
void mtx_measure(const xck_coo* m, const int32_t* row_map, int64_t ch, unsigned nt, int64_t* lines, int64_t* bytes);
// header + per-chunk offsets
void mtx_layout(const xck_coo* m, const int32_t* row_map, int32_t n_rows_out, int32_t n_cols, int64_t ch, unsigned nt, MtxLayout* L);
// header and text into [base, base + L.size()), nothing outside it; false (and *err) if a chunk did not end where the next one starts
bool mtx_fill(char* base, const xck_coo* m, const int32_t* row_map, const MtxLayout& L, unsigned nt, std::string* err);
// the text of m (no header) into fd from file_off on through the ring; the offset past the last byte, or -1
off_t mtx_write_stream(int fd, off_t file_off, bool seekable, const xck_coo* m, const int32_t* row_map, int64_t ch, unsigned nt, MtxTimes* tm);

// xck_write_mtx / xck_write_mtx_part without their argument checks: XCK_OK or XCK_E_IO (+ *err)
int mtx_write_file(const char* path, const xck_coo* m, const int32_t* row_map, int32_t n_rows_out, int32_t n_cols, int default_threads, std::string* err);
int mtx_write_part(const char* path, int64_t offset, const xck_coo* m, const int32_t* row_map, int default_threads, std::string* err);

}  // namespace xck
