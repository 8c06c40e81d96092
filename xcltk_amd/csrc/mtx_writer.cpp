// mtx_writer.cpp - see mtx_writer.h.  A 500 M-read run writes ~1.3 * 10^8 lines, 1.6 GB of text in four files, and nothing
// overlaps it: a run ends when the files are there.
#include "mtx_writer.h"
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <fcntl.h>
#include <unistd.h>
#include <sys/mman.h>
#include <sys/stat.h>

namespace xck {
namespace {

typedef std::chrono::steady_clock::time_point tp;
inline tp now() { return std::chrono::steady_clock::now(); }
inline double ms_between(tp a, tp b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

const char* const kDigits2 =
    "0001020304050607080910111213141516171819202122232425262728293031323334353637383940414243444546474849"
    "5051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
// decimal digits of v without a divide: floor(log10) estimated from the bit length (1233 / 4096 ~ log10 2), corrected by one compare
const uint32_t kPow10[10] = {0, 10, 100, 1000, 10000, 100000, 1000000, 10000000, 100000000, 1000000000};
inline int n_digits_u32(uint32_t v) {
    const int t = ((32 - __builtin_clz(v | 1)) * 1233) >> 12;
    return t + 1 - (v < kPow10[t]);
}
// the numbers of a line are int32 values or an int32 + 1: their magnitude fits 32 bits
inline int n_chars(int64_t v) { return v < 0 ? 1 + n_digits_u32((uint32_t)-v) : n_digits_u32((uint32_t)v); }
// decimal text of such a number, two digits per step from a table; stores its own characters and nothing else
inline void put_int(char*& p, int64_t v64) {
    if (v64 < 0) { *p++ = '-'; v64 = -v64; }
    uint32_t v = (uint32_t)v64;
    const int d = n_digits_u32(v);
    char* q = p + d;
    while (v >= 100) { const uint32_t r = v % 100; v /= 100; q -= 2; memcpy(q, kDigits2 + 2 * r, 2); }
    if (v >= 10) memcpy(q - 2, kDigits2 + 2 * v, 2); else q[-1] = char('0' + v);
    p += d;
}

template <class F> void for_chunks(int64_t n_chunks, unsigned nt, F fn) {
    if (nt <= 1 || n_chunks <= 1) { for (int64_t c = 0; c < n_chunks; c++) fn(c); return; }
    std::atomic<int64_t> next(0);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back([&]() { for (int64_t c; (c = next.fetch_add(1)) < n_chunks;) fn(c); });
    for (auto& x : th) x.join();
}

// kept lines of entries [i0, i1) and, if asked, the bytes of their text (entries are sorted by row: its width once per run)
inline void chunk_sizes(const xck_coo* m, const int32_t* row_map, int64_t i0, int64_t i1, int64_t* lines, int64_t* bytes) {
    int64_t k = 0, by = 0; int32_t r_prev = -1; int rw = 0;
    if (!bytes) { for (int64_t i = i0; i < i1; i++) k += row_map[m->row[i]] > 0; *lines = k; return; }
    for (int64_t i = i0; i < i1; i++) {
        const int32_t r = row_map[m->row[i]];
        if (r <= 0) continue;
        if (r != r_prev) { rw = n_digits_u32((uint32_t)r) + 3; r_prev = r; }     // + two tabs and the newline
        k++; by += rw + n_chars((int64_t)m->col[i] + 1) + n_chars(m->val[i]);
    }
    *lines = k; *bytes = by;
}

// "row\tcol\tval\n" lines of entries [i0, i1) from p on; returns the end of the text.  No store reaches `end` or beyond: the
// row text is copied as a fixed 16 bytes (rlen <= 11 of them kept, the rest overwritten by what follows) only where 16 bytes
// are left before `end`, exactly otherwise - in a mapped file the bytes behind a chunk belong to another thread, or to no one.
inline char* format_chunk(char* p, const char* end, const xck_coo* m, const int32_t* row_map, int64_t i0, int64_t i1) {
    char rtxt[16] = {0}; int rlen = 0; int32_t r_prev = -1;
    for (int64_t i = i0; i < i1; i++) {
        const int32_t r = row_map[m->row[i]];
        if (r <= 0) continue;
        if (r != r_prev) { char* q = rtxt; put_int(q, r); *q++ = '\t'; rlen = (int)(q - rtxt); r_prev = r; }
        if (end - p >= 16) memcpy(p, rtxt, 16); else memcpy(p, rtxt, (size_t)rlen);
        p += rlen;
        put_int(p, (int64_t)m->col[i] + 1); *p++ = '\t'; put_int(p, m->val[i]); *p++ = '\n';
    }
    return p;
}
constexpr size_t kLineMax = 36;          // 3 numbers of <= 11 characters + 3 separators

int header_text(char* line, size_t cap, int32_t n_rows_out, int32_t n_cols, int64_t nnz) {
    return snprintf(line, cap, "%%%%MatrixMarket matrix coordinate integer general\n%%%%\n%d\t%d\t%lld\n", n_rows_out, n_cols, (long long)nnz);
}

bool put_all(int fd, const char* p, size_t len, off_t at, bool seekable) {
    while (len) {
        const ssize_t w = seekable ? pwrite(fd, p, len, at) : write(fd, p, len);
        if (w < 0) { if (errno == EINTR) continue; return false; }
        p += w; len -= (size_t)w; at += w;
    }
    return true;
}

}  // namespace

int64_t mtx_chunk_entries() {
    if (const char* e = getenv("XCK_WRITE_CHUNK_ENTRIES")) { const long long v = atoll(e); if (v > 0) return (int64_t)std::min<long long>(v, 1ll << 24); }
    return 1 << 18;
}

unsigned mtx_threads(int default_threads, int64_t n_chunks) {
    unsigned nt = (unsigned)std::max(1, default_threads); if (nt > 16) nt = 16;
    if (const char* e = getenv("XCK_WRITE_THREADS")) nt = (unsigned)std::max(1, std::min(256, atoi(e)));
    if ((int64_t)nt > n_chunks) nt = (unsigned)std::max<int64_t>(n_chunks, 1);
    return nt;
}

void mtx_measure(const xck_coo* m, const int32_t* row_map, int64_t ch, unsigned nt, int64_t* lines, int64_t* bytes) {
    const int64_t n = m->nnz, n_chunks = (n + ch - 1) / ch;
    std::vector<int64_t> kl((size_t)n_chunks, 0), kb((size_t)n_chunks, 0);
    for_chunks(n_chunks, nt, [&](int64_t c) { chunk_sizes(m, row_map, c * ch, std::min(n, (c + 1) * ch), &kl[(size_t)c], bytes ? &kb[(size_t)c] : nullptr); });
    int64_t L = 0, B = 0; for (int64_t c = 0; c < n_chunks; c++) { L += kl[(size_t)c]; B += kb[(size_t)c]; }
    *lines = L; if (bytes) *bytes = B;
}

void mtx_layout(const xck_coo* m, const int32_t* row_map, int32_t n_rows_out, int32_t n_cols, int64_t ch, unsigned nt, MtxLayout* L) {
    const int64_t n = m->nnz;
    L->ch = ch; L->n_chunks = (n + ch - 1) / ch;
    std::vector<int64_t> kl((size_t)L->n_chunks, 0);
    L->off.assign((size_t)L->n_chunks + 1, 0);
    for_chunks(L->n_chunks, nt, [&](int64_t c) { chunk_sizes(m, row_map, c * ch, std::min(n, (c + 1) * ch), &kl[(size_t)c], &L->off[(size_t)c + 1]); });
    L->lines = 0; for (int64_t k : kl) L->lines += k;
    L->header_len = header_text(L->header, sizeof L->header, n_rows_out, n_cols, L->lines);
    L->off[0] = L->header_len;
    for (int64_t c = 0; c < L->n_chunks; c++) L->off[(size_t)c + 1] += L->off[(size_t)c];       // sizes -> offsets
}

bool mtx_fill(char* base, const xck_coo* m, const int32_t* row_map, const MtxLayout& L, unsigned nt, std::string* err) {
    const int64_t n = m->nnz;
    std::atomic<int64_t> bad(-1);
    if (L.n_chunks == 0) memcpy(base, L.header, (size_t)L.header_len);
    for_chunks(L.n_chunks, nt, [&](int64_t c) {
        if (c == 0) memcpy(base, L.header, (size_t)L.header_len);
        const char* end = base + L.off[(size_t)c + 1];
        if (format_chunk(base + L.off[(size_t)c], end, m, row_map, c * L.ch, std::min(n, (c + 1) * L.ch)) != end) bad = c;
    });
    if (bad.load() >= 0 && err) *err = "mtx writer: the text of chunk " + std::to_string(bad.load()) + " does not have its measured size";
    return bad.load() < 0;
}

off_t mtx_write_stream(int fd, off_t file_off, bool seekable, const xck_coo* m, const int32_t* row_map, int64_t ch, unsigned nt, MtxTimes* tm) {
    const int64_t n = m->nnz, n_chunks = (n + ch - 1) / ch;
    const size_t cap = (size_t)ch * kLineMax + 64;
    if (n_chunks == 0) return file_off;
    if (nt <= 1 || n_chunks == 1) {                                    // one buffer, no thread
        std::unique_ptr<char[]> b(new char[cap]);
        for (int64_t c = 0; c < n_chunks; c++) {
            const tp t0 = now();
            const size_t used = (size_t)(format_chunk(b.get(), b.get() + cap, m, row_map, c * ch, std::min(n, (c + 1) * ch)) - b.get());
            const tp t1 = now();
            if (used && !put_all(fd, b.get(), used, file_off, seekable)) return (off_t)-1;
            file_off += (off_t)used;
            if (tm) { tm->ms_format_cpu += ms_between(t0, t1); tm->ms_pwrite += ms_between(t1, now()); }
        }
        return file_off;
    }
    // the ring: slot c % R holds chunk c from the moment its formatter is done until the drain has written it; a formatter
    // takes the next chunk number and waits for that chunk's slot, so the chunk the drain waits for is never held up
    const int64_t R = std::min<int64_t>(n_chunks, (int64_t)nt + 2);
    std::vector<std::unique_ptr<char[]>> bufs((size_t)R);              // uninitialised, allocated on first use
    std::vector<size_t> used((size_t)R, 0);
    std::vector<int64_t> holds((size_t)R, -1);
    std::mutex mu; std::condition_variable cv_ready, cv_free;
    int64_t drained = 0; bool stop = false;
    std::atomic<int64_t> next(0);
    double fmt_ms = 0;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++) th.emplace_back([&]() {
        double my_ms = 0;
        for (int64_t c; (c = next.fetch_add(1)) < n_chunks;) {
            const size_t s = (size_t)(c % R);
            { std::unique_lock<std::mutex> lk(mu); cv_free.wait(lk, [&] { return stop || c < drained + R; }); if (stop) break; }
            const tp t0 = now();
            if (!bufs[s]) bufs[s].reset(new char[cap]);
            const size_t u = (size_t)(format_chunk(bufs[s].get(), bufs[s].get() + cap, m, row_map, c * ch, std::min(n, (c + 1) * ch)) - bufs[s].get());
            my_ms += ms_between(t0, now());
            { std::lock_guard<std::mutex> lk(mu); used[s] = u; holds[s] = c; }
            cv_ready.notify_one();
        }
        std::lock_guard<std::mutex> lk(mu); fmt_ms += my_ms;
    });
    bool ok = true;
    for (int64_t c = 0; c < n_chunks; c++) {
        const size_t s = (size_t)(c % R);
        const tp t0 = now();
        { std::unique_lock<std::mutex> lk(mu); cv_ready.wait(lk, [&] { return holds[s] == c; }); }
        const tp t1 = now();
        ok = !used[s] || put_all(fd, bufs[s].get(), used[s], file_off, seekable);
        file_off += (off_t)used[s];
        if (tm) { tm->ms_drain_wait += ms_between(t0, t1); tm->ms_pwrite += ms_between(t1, now()); }
        { std::lock_guard<std::mutex> lk(mu); if (ok) drained = c + 1; else stop = true; }
        cv_free.notify_all();
        if (!ok) break;
    }
    for (auto& x : th) x.join();
    if (tm) tm->ms_format_cpu += fmt_ms;
    return ok ? file_off : (off_t)-1;
}

int mtx_write_file(const char* path, const xck_coo* m, const int32_t* row_map, int32_t n_rows_out, int32_t n_cols, int default_threads, std::string* err) {
    const bool dbg = getenv("XCK_DEBUG_TIMING") != nullptr;
    auto fail = [&](int fd, const std::string& what) { const int e = errno; if (fd >= 0) close(fd); if (err) *err = what + " " + path + (e ? std::string(": ") + strerror(e) : std::string()); return XCK_E_IO; };
    MtxTimes tm;
    const tp t0 = now();
    // a pipe or a device is opened for writing only, as ever (a FIFO opened for both directions would never notice that its reader left).
    // A regular file that is already there is NOT emptied: its pages are overwritten in place and what is left of it behind the new
    // text is cut off at the end.  Emptying the last run's matrix.mtx (1.2 GB in the page cache) costs 80 - 100 ms on ext4, and a file
    // emptied and rewritten is what ext4's auto_da_alloc looks for: close then starts the write-back of the new text, 125 - 140 ms more
    // (profiles/r30_mtx_mapped_writer.txt).  Neither way promises anything about the file before the call has returned.
    struct stat st;
    const bool special = stat(path, &st) == 0 && !S_ISREG(st.st_mode);
    errno = 0;
    const int fd = open(path, special ? O_WRONLY : O_RDWR | O_CREAT, 0666);
    if (fd < 0) return fail(-1, "cannot open");
    const bool regular = fstat(fd, &st) == 0 && S_ISREG(st.st_mode);
    const bool seekable = regular || lseek(fd, 0, SEEK_CUR) != (off_t)-1;
    const int64_t ch = mtx_chunk_entries(), n_chunks = (m->nnz + ch - 1) / ch;
    const unsigned nt = mtx_threads(default_threads, n_chunks);
    const char* knob = getenv("XCK_WRITE_MAP");
    const bool want_map = knob && !strcmp(knob, "1");
    const char* why = !want_map ? nullptr : !regular ? "not a regular file" : nullptr;      // why a wanted mapping was not made
    const tp t1 = now();
    tm.ms_open = ms_between(t0, t1);

    MtxLayout L;
    if (want_map && !why) {                                            // sizes first
        mtx_layout(m, row_map, n_rows_out, n_cols, ch, nt, &L);
    } else {
        mtx_measure(m, row_map, ch, nt, &L.lines, nullptr);
        L.header_len = header_text(L.header, sizeof L.header, n_rows_out, n_cols, L.lines);
    }
    const tp t2 = now();
    tm.ms_sizes = ms_between(t1, t2);

    if (want_map && !why && L.lines > 0) {
        // the file at its final size with its blocks allocated: a full disk is an error code here, not a SIGBUS in the fill
        // (glibc's posix_fallocate would write zeros where the file system has no fallocate: the pipeline is the better fallback)
        if (st.st_size > (off_t)L.size() && ftruncate(fd, (off_t)L.size()) != 0) why = "ftruncate failed";
        else if (fallocate(fd, 0, 0, (off_t)L.size()) != 0) why = "fallocate failed";
        else {
            const tp t3 = now();
            tm.ms_alloc = ms_between(t2, t3);
            void* base = mmap(nullptr, (size_t)L.size(), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
            if (base == MAP_FAILED) why = "mmap failed";
            else {
                std::string ferr;
                const bool ok = mtx_fill((char*)base, m, row_map, L, nt, &ferr);
                const tp t4 = now();
                tm.ms_fill = ms_between(t3, t4);
                errno = 0;
                const bool unmapped = munmap(base, (size_t)L.size()) == 0;       // no msync: pwrite promised no durability either
                if (!ok) { errno = 0; return fail(fd, ferr + ":"); }
                if (!unmapped || close(fd) != 0) return fail(unmapped ? -1 : fd, "cannot finish");
                if (dbg) fprintf(stderr, "[xck] write_mtx %s: mapped: %lld lines, %lld bytes, %lld chunks of %lld entries, %u threads | ms: open %.1f sizes %.1f fallocate %.1f fill %.1f unmap+close %.1f total %.1f\n",
                                 path, (long long)L.lines, (long long)L.size(), (long long)L.n_chunks, (long long)ch, nt, tm.ms_open, tm.ms_sizes, tm.ms_alloc, tm.ms_fill, ms_between(t4, now()), ms_between(t0, now()));
                return XCK_OK;
            }
        }
    }

    // header only, or the pipeline
    errno = 0;
    if (!put_all(fd, L.header, (size_t)L.header_len, 0, seekable)) return fail(fd, "cannot write");
    off_t end = (off_t)L.header_len;
    if (L.lines > 0) end = mtx_write_stream(fd, end, seekable, m, row_map, ch, nt, &tm);
    if (end < 0) return fail(fd, "cannot write");
    const tp t5 = now();
    if (regular && st.st_size > end && ftruncate(fd, end) != 0) return fail(fd, "cannot truncate");       // the rest of an older, longer file
    const tp t6 = now();
    if (close(fd) != 0) return fail(-1, "cannot finish");
    if (dbg) fprintf(stderr, "[xck] write_mtx %s: %s: %lld lines, %lld bytes, chunks of %lld entries, %u threads | ms: open %.1f %s %.1f drain: waited %.1f pwrite %.1f (formatting, CPU ms of all threads: %.1f) cut %.1f close %.1f total %.1f\n",
                     path, L.lines == 0 ? "header only" : why ? (std::string("pipeline (") + why + ")").c_str() : "pipeline", (long long)L.lines, (long long)end, (long long)ch, nt, tm.ms_open,
                     L.off.empty() ? "measure" : "sizes", tm.ms_sizes, tm.ms_drain_wait, tm.ms_pwrite, tm.ms_format_cpu, ms_between(t5, t6), ms_between(t6, now()), ms_between(t0, now()));
    return XCK_OK;
}

int mtx_write_part(const char* path, int64_t offset, const xck_coo* m, const int32_t* row_map, int default_threads, std::string* err) {
    errno = 0;
    const int fd = open(path, O_WRONLY | O_CREAT, 0666);               // never truncated: other pieces may be there already
    if (fd < 0) { if (err) *err = std::string("cannot open ") + path + ": " + strerror(errno); return XCK_E_IO; }
    const int64_t ch = mtx_chunk_entries();
    const off_t end = mtx_write_stream(fd, (off_t)offset, true, m, row_map, ch, mtx_threads(default_threads, (m->nnz + ch - 1) / ch), nullptr);
    if (close(fd) != 0 || end < 0) { if (err) *err = std::string("cannot write ") + path; return XCK_E_IO; }
    return XCK_OK;
}

}  // namespace xck
