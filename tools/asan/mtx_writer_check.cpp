// Host-only check of the .mtx writer (csrc/mtx_writer.cpp) under AddressSanitizer / UBSan, and under ThreadSanitizer: random matrices,
// chunk sizes and thread counts, each written three ways - xck_write_mtx's pipeline (the default), its mapped path (XCK_WRITE_MAP=1), and snprintf
// line by line here - and the three texts must be the same bytes.  Then the fill alone (mtx_fill) runs on a mapping made here: a file of a
// whole number of pages with a PROT_NONE page behind it and the text placed so that its last byte is the last byte of the last page, so
// one store past the end of the text is a fault, and the bytes in front of the text must still be the zeros they were.  No device, no HIP
// call: the program links csrc/mtx_writer.cpp alone.
//   make -C tools/asan mtx_writer_check mtx_writer_check_tsan && tools/asan/mtx_writer_check && tools/asan/mtx_writer_check_tsan
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <fcntl.h>
#include <unistd.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include "../../xcltk_amd/csrc/mtx_writer.h"

using namespace xck;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)((g_rng >> 11) % n); }
// a number of 1 to 10 digits, every length as likely as the next, INT32_MAX among them
static int32_t rnd_digits() {
    static const int64_t p10[11] = {1, 10, 100, 1000, 10000, 100000, 1000000, 10000000, 100000000, 1000000000, (int64_t)INT32_MAX + 1};
    const int d = 1 + (int)rnd(10);
    if (rnd(50) == 0) return INT32_MAX;
    return (int32_t)(p10[d - 1] + rnd((uint32_t)(p10[d] - p10[d - 1])));
}

static bool slurp(const std::string& fn, std::string* out) {
    FILE* f = fopen(fn.c_str(), "rb"); if (!f) return false;
    out->clear(); char buf[65536]; size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) out->append(buf, k);
    fclose(f); return true;
}

int main() {
    char dir_t[] = "/tmp/xck_mtx_check_XXXXXX";
    if (!mkdtemp(dir_t)) { perror("mkdtemp"); return 2; }
    const std::string dir = dir_t, fn_map = dir + "/map.mtx", fn_pipe = dir + "/pipe.mtx", fn_guard = dir + "/guard.bin";
    const size_t page = (size_t)sysconf(_SC_PAGESIZE);
    long rounds = 0, lines = 0, many_chunks = 0;
    int rc = 0;
    for (int round = 0; round < 400 && rc == 0; round++) {
        // ---- a matrix: rows sorted, a row map that drops some rows and sends the others to numbers of every width ----
        const int64_t n = round < 4 ? round : round % 9 == 0 ? 2000 + (int64_t)rnd(8000) : (int64_t)rnd(600);
        const int32_t n_rows = 1 + (int32_t)rnd(40);
        std::vector<int32_t> rm((size_t)n_rows), row((size_t)n), col((size_t)n), val((size_t)n);
        const uint32_t drop = rnd(4);                                // 0: none dropped; 3 of 4 matrices lose rows
        for (auto& r : rm) r = drop && rnd(4) < drop ? (rnd(2) ? 0 : -(int32_t)rnd(5)) : rnd_digits();
        if (round % 17 == 5) for (auto& r : rm) r = 0;               // everything dropped
        for (auto& r : row) r = (int32_t)rnd((uint32_t)n_rows);
        std::sort(row.begin(), row.end());
        for (auto& c : col) c = rnd_digits() - 1;
        for (auto& v : val) v = rnd(8) == 0 ? -rnd_digits() : rnd(200) == 0 ? INT32_MIN : rnd_digits();
        const xck_coo m = {n, row.data(), col.data(), val.data()};
        const int64_t ch = 1 + (int64_t)rnd(round % 3 == 0 ? 8 : 300);
        const unsigned nt = 1 + rnd(6);
        setenv("XCK_WRITE_CHUNK_ENTRIES", std::to_string(ch).c_str(), 1);
        setenv("XCK_WRITE_THREADS", std::to_string(nt).c_str(), 1);
        const int32_t n_rows_out = rnd_digits(), n_cols = rnd_digits();

        // ---- the text, line by line ----
        std::string ref; int64_t kept = 0;
        for (int64_t i = 0; i < n; i++) if (rm[(size_t)row[(size_t)i]] > 0) {
            char line[64]; kept++;
            ref.append(line, (size_t)snprintf(line, sizeof line, "%d\t%lld\t%d\n", rm[(size_t)row[(size_t)i]], (long long)col[(size_t)i] + 1, val[(size_t)i]));
        }
        { char head[96]; ref.insert(0, head, (size_t)snprintf(head, sizeof head, "%%%%MatrixMarket matrix coordinate integer general\n%%%%\n%d\t%d\t%lld\n", n_rows_out, n_cols, (long long)kept)); }

        // ---- both paths of xck_write_mtx; now and then over a longer file that is already there ----
        std::string err, got;
        if (round % 5 == 0) for (const std::string* f : {&fn_map, &fn_pipe}) { FILE* o = fopen(f->c_str(), "wb"); std::string junk(ref.size() + 1 + rnd(10000), 'x'); fwrite(junk.data(), 1, junk.size(), o); fclose(o); }
        setenv("XCK_WRITE_MAP", "1", 1);
        if (mtx_write_file(fn_map.c_str(), &m, rm.data(), n_rows_out, n_cols, 4, &err) != XCK_OK) { fprintf(stderr, "round %d: mapped path: %s\n", round, err.c_str()); rc = 1; break; }
        if (!slurp(fn_map, &got) || got != ref) { fprintf(stderr, "round %d: mapped path: %zu bytes, not the %zu expected ones (n %lld, chunk %lld, %u threads)\n", round, got.size(), ref.size(), (long long)n, (long long)ch, nt); rc = 1; break; }
        if (round & 1) unsetenv("XCK_WRITE_MAP"); else setenv("XCK_WRITE_MAP", "0", 1);
        if (mtx_write_file(fn_pipe.c_str(), &m, rm.data(), n_rows_out, n_cols, 4, &err) != XCK_OK) { fprintf(stderr, "round %d: pipeline: %s\n", round, err.c_str()); rc = 1; break; }
        if (!slurp(fn_pipe, &got) || got != ref) { fprintf(stderr, "round %d: pipeline: %zu bytes, not the %zu expected ones (n %lld, chunk %lld, %u threads)\n", round, got.size(), ref.size(), (long long)n, (long long)ch, nt); rc = 1; break; }
        int64_t part_lines = 0, part_bytes = 0;
        mtx_measure(&m, rm.data(), ch, nt, &part_lines, &part_bytes);
        if (part_lines != kept) { fprintf(stderr, "round %d: mtx_measure counts %lld lines, not %lld\n", round, (long long)part_lines, (long long)kept); rc = 1; break; }

        // ---- the fill alone, its end against a guard page ----
        MtxLayout L;
        mtx_layout(&m, rm.data(), n_rows_out, n_cols, ch, nt, &L);
        if ((size_t)L.size() != ref.size() || L.lines != kept || L.off[0] + part_bytes != L.size()) { fprintf(stderr, "round %d: mtx_layout: %lld bytes, %lld lines, expected %zu, %lld\n", round, (long long)L.size(), (long long)L.lines, ref.size(), (long long)kept); rc = 1; break; }
        const size_t size = (size_t)L.size(), whole = (size + page - 1) / page * page, lead = whole - size;
        const int fd = open(fn_guard.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0666);
        if (fd < 0 || ftruncate(fd, (off_t)whole) != 0) { perror("guard file"); rc = 2; break; }
        char* area = (char*)mmap(nullptr, whole + page, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (area == MAP_FAILED || mmap(area, whole, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_FIXED, fd, 0) != area) { perror("guard mapping"); rc = 2; break; }
        const bool ok = mtx_fill(area + lead, &m, rm.data(), L, nt, &err);       // a store behind the text dies here
        bool clean = true; for (size_t i = 0; i < lead; i++) clean &= area[i] == 0;
        const bool same = memcmp(area + lead, ref.data(), size) == 0;
        munmap(area, whole + page); close(fd);
        if (!ok || !clean || !same) { fprintf(stderr, "round %d: mtx_fill: %s%s%s\n", round, ok ? "" : err.c_str(), clean ? "" : " bytes in front of the text were written", same ? "" : " the text differs"); rc = 1; break; }
        rounds++; lines += kept; many_chunks += L.n_chunks > 8;
    }
    unlink(fn_map.c_str()); unlink(fn_pipe.c_str()); unlink(fn_guard.c_str()); rmdir(dir.c_str());
    if (rc) return rc;
    printf("%ld matrices, %ld lines: three texts identical, guard page untouched (%ld of them in more than 8 chunks)\n", rounds, lines, many_chunks);
    return rounds == 400 && many_chunks > 100 ? 0 : 1;
}
