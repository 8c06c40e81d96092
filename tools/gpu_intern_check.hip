// xck_gpu_intern_check - the device intern table (csrc/intern_dev.hip, XCK_GPU_NAMES) alone: name lists go through its insert routine
// (di_key_wave, the one both kernels of the ingest use) in several launches, and the host checks
//   - keys are equal exactly where the names are (lengths and bytes),
//   - ids are smaller than the distinct names plus the lanes the launches had (an insert race may waste an id, never more than one per lane),
//   - the table counted as many entries as there are distinct interned names,
//   - a table grown from 64 slots and a 1 KB arena gives the same partition as one sized in advance.
// The lists: 64 copies of one name in one wave; 32 names twice in one wave; names of 1, 7, 8, 9, 15, 16, 17, 253 and 254 bytes; names
// equal in their first 8 / 16 bytes that differ in the last byte or only in length; names with high and zero bytes; directly codable
// names among the others; 20,000 random names with the table keeping 4 hash bits (every probe chain holds thousands of names).
// Prints one line per list and run; exit status 0 iff every check held.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>
#include "../xcltk_amd/csrc/intern_dev.h"

using namespace xck;

__global__ __launch_bounds__(64) void k_check(const uint32_t* __restrict__ off, const uint32_t* __restrict__ len, const uint8_t* __restrict__ bytes, uint32_t n, DiView v, uint64_t* __restrict__ keys) {
    const int lane = (int)threadIdx.x;
    const uint32_t i = blockIdx.x * 64u + (uint32_t)lane;
    const bool have = i < n;
    const uint64_t key = di_key_wave(v, bytes + (have ? off[i] : 0u), have ? len[i] : 0u, have, lane);
    if (have) keys[i] = key;
}

#define CK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "HIP error at %s:%d\n", __FILE__, __LINE__); return false; } } while (0)
constexpr int UMI_BITS = 38;

struct Run { std::vector<uint64_t> keys; uint32_t entries = 0, ids = 0, flags = 0; int growths = 0; size_t lanes = 0; };

// the names in `launches` launches through a table of the given first sizes
static bool run_list(const std::vector<std::string>& names, int launches, size_t slots0, size_t arena0, int hash_bits, Run* out) {
    hipStream_t st; CK(hipStreamCreate(&st));
    DevIntern* t = dev_intern_create(0, slots0, arena0, hash_bits, false);
    const size_t n = names.size();
    std::vector<uint32_t> off(n), len(n); std::vector<uint8_t> bytes;
    for (size_t i = 0; i < n; i++) { off[i] = (uint32_t)bytes.size(); len[i] = (uint32_t)names[i].size(); bytes.insert(bytes.end(), names[i].begin(), names[i].end()); }
    bytes.resize(bytes.size() + 8);
    uint32_t *d_off, *d_len; uint8_t* d_bytes; uint64_t* d_keys;
    CK(hipMalloc((void**)&d_off, n * 4)); CK(hipMalloc((void**)&d_len, n * 4)); CK(hipMalloc((void**)&d_bytes, bytes.size())); CK(hipMalloc((void**)&d_keys, n * 8));
    CK(hipMemcpy(d_off, off.data(), n * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(d_len, len.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice)); CK(hipMemset(d_keys, 0xee, n * 8));
    const size_t per = (n + (size_t)launches - 1) / (size_t)launches;
    out->lanes = 0;
    for (size_t i0 = 0; i0 < n; i0 += per) {
        const size_t k = std::min(per, n - i0); size_t nb = 0; for (size_t i = i0; i < i0 + k; i++) nb += len[i];
        if (dev_intern_reserve(t, st, k, nb) != 0) { fprintf(stderr, "reserve failed\n"); return false; }
        const unsigned g = (unsigned)((k + 63) / 64);
        hipLaunchKernelGGL(k_check, dim3(g), dim3(64), 0, st, d_off + i0, d_len + i0, d_bytes, (uint32_t)k, dev_intern_view(t, UMI_BITS, (1ull << (UMI_BITS - 1)) - 1), d_keys + i0);
        CK(hipGetLastError());
        CK(hipMemcpyAsync(t->h_ctl, t->d_ctl, sizeof(DiCtl), hipMemcpyDeviceToHost, st));
        if (i0 / per % 2 == 0) { CK(hipStreamSynchronize(st)); (void)dev_intern_synced(t); }   // (every other launch leaves the host with its bound only)
        out->lanes += (size_t)g * 64;
    }
    CK(hipStreamSynchronize(st));
    out->flags = dev_intern_synced(t); out->entries = t->h_ctl->n_entries; out->ids = t->h_ctl->next_id; out->growths = t->growths;
    out->keys.resize(n); CK(hipMemcpy(out->keys.data(), d_keys, n * 8, hipMemcpyDeviceToHost));
    (void)hipFree(d_off); (void)hipFree(d_len); (void)hipFree(d_bytes); (void)hipFree(d_keys);
    dev_intern_destroy(t); (void)hipStreamDestroy(st);
    return true;
}

// the host's rule for what needs no table (bam_records.cpp encode_key_direct)
static bool direct_key(const std::string& s, uint64_t* out) {
    if (s.empty()) { *out = XCK_UMI_NONE; return true; }
    if (2 * (int)s.size() + 1 > UMI_BITS - 1) return false;
    uint64_t v = 1;
    for (char c : s) { const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; if (code == 4) return false; v = (v << 2) | (uint64_t)code; }
    *out = v; return true;
}

static int check_run(const char* what, const std::vector<std::string>& names, const Run& r) {
    int bad = 0;
    if (r.flags) { printf("  %s: table flags %u\n", what, r.flags); bad++; }
    std::map<std::string, uint64_t> by_name; std::map<uint64_t, std::string> by_key; size_t distinct_interned = 0; uint64_t max_id = 0;
    const uint64_t top = 1ull << (UMI_BITS - 1);
    for (size_t i = 0; i < names.size() && bad < 10; i++) {
        const uint64_t k = r.keys[i]; uint64_t d;
        if (direct_key(names[i], &d)) { if (k != d) { printf("  %s: name %zu is directly codable, key %llx != %llx\n", what, i, (unsigned long long)k, (unsigned long long)d); bad++; } continue; }
        if (!(k & top) || k == XCK_UMI_NONE) { printf("  %s: name %zu got no interned key (%llx)\n", what, i, (unsigned long long)k); bad++; continue; }
        auto a = by_name.find(names[i]);
        if (a == by_name.end()) { by_name[names[i]] = k; distinct_interned++; } else if (a->second != k) { printf("  %s: name %zu has two keys\n", what, i); bad++; }
        auto b = by_key.find(k);
        if (b == by_key.end()) by_key[k] = names[i]; else if (b->second != names[i]) { printf("  %s: key %llx serves two names (lengths %zu, %zu)\n", what, (unsigned long long)k, b->second.size(), names[i].size()); bad++; }
        max_id = std::max<uint64_t>(max_id, k & (top - 1));
    }
    if (distinct_interned && max_id >= distinct_interned + r.lanes) { printf("  %s: id %llu is not below distinct names + lanes (%zu + %zu)\n", what, (unsigned long long)max_id, distinct_interned, r.lanes); bad++; }
    if (r.entries != distinct_interned) { printf("  %s: the table counted %u entries, the list has %zu distinct interned names\n", what, r.entries, distinct_interned); bad++; }
    if (r.ids < r.entries || r.ids > distinct_interned + r.lanes) { printf("  %s: %u ids reserved for %u entries\n", what, r.ids, r.entries); bad++; }
    return bad;
}

// where keys are equal in one run they are in the other
static int same_partition(const char* what, const Run& a, const Run& b) {
    std::map<uint64_t, uint64_t> ab, ba; int bad = 0;
    for (size_t i = 0; i < a.keys.size(); i++) {
        auto x = ab.emplace(a.keys[i], b.keys[i]); auto y = ba.emplace(b.keys[i], a.keys[i]);
        if (x.first->second != b.keys[i] || y.first->second != a.keys[i]) { if (bad < 5) printf("  %s: the partitions differ at name %zu\n", what, i); bad++; }
    }
    return bad;
}

int main() {
    int n_dev = 0; if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || hipSetDevice(0) != hipSuccess) { fprintf(stderr, "no device\n"); return 2; }
    struct List { const char* what; std::vector<std::string> names; int launches, hash_bits; };
    std::vector<List> lists;
    { List l{"64 copies of one name in one wave", {}, 1, 0}; for (int i = 0; i < 64; i++) l.names.push_back("read/one-name:1234"); lists.push_back(l); }
    { List l{"32 names twice in one wave", {}, 1, 0}; for (int i = 0; i < 64; i++) l.names.push_back("pair" + std::to_string(1000 + i % 32)); lists.push_back(l); }
    { List l{"lengths 1 .. 254", {}, 2, 0};
      for (int rep = 0; rep < 3; rep++) for (int n : {1, 7, 8, 9, 15, 16, 17, 253, 254}) { std::string s((size_t)n, 'x'); s[(size_t)n / 2] = 'y'; l.names.push_back(s); l.names.push_back(std::string((size_t)n, 'x')); }
      lists.push_back(l); }
    { List l{"equal prefixes, last byte or length differs", {}, 2, 0};
      const std::string p8 = "abcdefgh", p16 = "abcdefghijklmnop";
      for (int rep = 0; rep < 2; rep++)
          for (const std::string& s : {p8, p8 + "i", p8 + "j", p8.substr(0, 7), p8.substr(0, 7) + "x", p16, p16 + "q", p16 + "r", p16.substr(0, 15), p16.substr(0, 15) + "x", p16 + "qr", p16 + "qs"}) l.names.push_back(s);
      lists.push_back(l); }
    { List l{"high and zero bytes, directly codable names", {}, 2, 0};
      for (int rep = 0; rep < 2; rep++) {
          l.names.push_back(std::string("\xff\x80" "abc", 5)); l.names.push_back(std::string("\xff\x80" "abd", 5)); l.names.push_back(std::string("\xff\x81" "abc", 5));
          l.names.push_back(std::string("a\0b", 3)); l.names.push_back(std::string("a\0c", 3)); l.names.push_back(std::string("a\0", 2)); l.names.push_back(std::string("a", 1));
          l.names.push_back(std::string(9, '\xfe')); l.names.push_back(std::string(8, '\xfe') + "\xfd");
          l.names.push_back("ACGT"); l.names.push_back("ACGTACGTACGTACGTAC"); l.names.push_back("ACGTACGTACGTACGTACG"); l.names.push_back("ACGN"); l.names.push_back(""); }
      lists.push_back(l); }
    { List l{"20,000 random names, 4 hash bits", {}, 5, 4};
      std::mt19937_64 rng(12345); std::vector<std::string> pool;
      for (int i = 0; i < 12000; i++) { const size_t n = 18 + rng() % 20; std::string s(n, ' '); for (char& c : s) c = (char)(33 + rng() % 90); pool.push_back(s); }
      for (int i = 0; i < 20000; i++) l.names.push_back(i < 12000 ? pool[(size_t)i] : pool[rng() % pool.size()]);
      lists.push_back(l); }
    int bad = 0;
    for (const List& l : lists) {
        Run sized, grown;
        if (!run_list(l.names, l.launches, 1 << 16, 4 << 20, l.hash_bits, &sized) || !run_list(l.names, l.launches + 2, 64, 1024, l.hash_bits, &grown)) return 2;
        int b = check_run("sized in advance", l.names, sized) + check_run("grown from 64 slots", l.names, grown) + same_partition("sized vs grown", sized, grown);
        if (sized.growths != 0) { printf("  the table sized in advance grew\n"); b++; }
        if (l.names.size() > 64 && grown.growths == 0) { printf("  the small table never grew\n"); b++; }
        printf("%s: %zu names, %u entries, ids %u / %u, growths %d / %d: %s\n", l.what, l.names.size(), sized.entries, sized.ids, grown.ids, sized.growths, grown.growths, b ? "FAILED" : "ok");
        bad += b;
    }
    printf("%s\n", bad ? "xck_gpu_intern_check: FAILED" : "xck_gpu_intern_check: all checks held");
    return bad ? 1 : 0;
}
