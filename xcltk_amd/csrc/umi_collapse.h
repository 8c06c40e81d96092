// umi_collapse.h - opt-in 1-mismatch UMI collapsing of the basefc fold (XCK_F_UMI_COLLAPSE / XCK_UMI_DEDUP=1mm_all;
// xck_get_umi_dedup_stats, include/xck.h).  Included by finish.hip inside namespace xck, behind umi_feature.h: it uses KeyLayout,
// ShardSpan, block_excl_scan, uf_block_sum, k_uf_heads / k_uf_distinct, k_cp_scan, read_ctl_words, Timer, sort_run / sort_tmp_bytes,
// pf_carve, fold_coo and HIP_TRY.  DESIGN.md section 3.14.
//
// The default fold counts R, the distinct (row, cell, UMI) keys the join accepted.  Under the flag the keys of one (row, cell) - a
// group - are the nodes of a graph: two keys are adjacent when both UMI codes are direct 2-bit codes of the same length that differ in
// exactly one base (uc_adjacent), and the matrix value is the number of connected components (STARsolo's 1MM_All, UMI-tools' cluster).
// Interned codes are adjacent to nothing.
//   k_uc_pack      shard slices -> one array, the UMI field narrowed to its used bits (64-bit keys, as k_pack_squeeze does)
//   sort           rocPRIM over all key bits from bit 0 (sort_run)
//   k_uf_heads / k_uf_distinct   the distinct keys D in (row, cell, UMI) order (umi_feature.h)
//   k_uc_small     tiles of UC_TILE keys of D through LDS with a halo of UC_SMALL keys on either side, so that every group of at most
//                  UC_SMALL keys that touches the tile lies in it whole.  Every key finds its group's bounds by walking its neighbours,
//                  tests its code against the other members once (a 64-bit adjacency mask in registers) and then lowers its label to
//                  the least label among its adjacent members until a block-wide vote says nothing changed; a key is its component's
//                  root when it kept its own label.  A group of one key does nothing.  Per tile: groups, changed groups, opaque keys,
//                  heads of larger groups, the largest small group - words that k_cp_scan sums (k_uc_max for the largest); no atomics
//                  on global memory
//   k_uc_big_list  the first keys of the groups of more than UC_SMALL keys, in order
//   k_uc_big       one workgroup per such group: its end by bisection; every key generates its 3L substitution neighbours, bisects the
//                  group's sorted codes for each, and joins what it finds in a union-find forest (compare-and-swap on the root, path
//                  halving).  Up to UC_MEDIUM keys the codes and the parents sit in LDS, beyond that the codes stay in D and the
//                  parents in the workspace - the same code over another accessor
//   k_uc_count / k_uc_emit   the roots, in the order of D and in the handle's key layout, packed at the front of the hit buffer
// The roots are distinct and sorted, so fold_coo() counts them as they are (sorted_from = 0; fold_path = 2).
//
// Count-directed rules (UMI-tools' directional, Cell Ranger's "correct to the more abundant neighbour") are not possible here: the
// join removes duplicate keys in its LDS set before they reach HBM, so the fold never sees read multiplicities.
#pragma once

constexpr int UC_BLOCK = 256, UC_ITEMS = 8, UC_TILE = UC_BLOCK * UC_ITEMS;
constexpr int UC_SMALL = 64;                                          // largest group of the tile path: one wave of keys, one 64-bit adjacency mask per key
constexpr int UC_MEDIUM = 5120;                                       // largest group whose codes (8 bytes) and parents (4 bytes) fit one workgroup's 64 KB of LDS
constexpr int UC_SPAN = UC_TILE + 2 * UC_SMALL, UC_STRIPS = (UC_SPAN + UC_BLOCK - 1) / UC_BLOCK;
constexpr int UC_BIG_BLOCK = 512;
static_assert(UC_TILE == (int)WS_TILE && UC_BLOCK == JOIN_BLOCK && UC_TILE == UF_TILE, "fold_ws.h sizes the per-tile words by this; block_excl_scan scans JOIN_BLOCK threads");
static_assert(UC_SMALL == (int)WS_UC_SMALL, "fold_ws.h sizes the list of larger groups by this");
static_assert(UC_MEDIUM * 12 + 256 <= 65536 && UC_SPAN < 65536, "LDS of k_uc_big; 16-bit labels of k_uc_small");
enum { UC_KEYS, UC_MOLECULES, UC_GROUPS, UC_CHANGED, UC_OPAQUE, UC_MAX_GROUP, UC_N_STATS };   // EngineImpl::uc_stats
enum { UCW_GROUPS, UCW_CHANGED, UCW_OPAQUE, UCW_BIG, UCW_MAX, UCW_ROWS };                      // rows of per-tile words of k_uc_small

template <class K> struct UcLayout {
    int ubits, used;                                                  // UMI field of the handle's keys; of the packed keys (<= ubits)
    unsigned long long imask;                                         // the bit that marks an interned code
    __device__ __forceinline__ K rc(K k) const { return k >> used; }
    __device__ __forceinline__ unsigned long long umi(K k) const { return (unsigned long long)(k & ((K(1) << used) - 1)); }
    __device__ __forceinline__ K widen(K k) const { return ((k >> used) << ubits) | (k & ((K(1) << used) - 1)); }
};

// two UMI codes of one group: direct codes of the same length that differ in exactly one base
__device__ __forceinline__ bool uc_adjacent(unsigned long long a, unsigned long long b, unsigned long long imask) {
    if (((a | b) & imask) || a == 0 || b == 0) return false;
    if (__clzll((long long)a) != __clzll((long long)b)) return false;
    const unsigned long long x = a ^ b;
    return __popcll((x | (x >> 1)) & 0x5555555555555555ull) == 1;
}

template <class K>
__global__ void __launch_bounds__(256) k_uc_pack(const K* __restrict__ src, unsigned long long cap, ShardSpan sp, UcLayout<K> ly, K* __restrict__ dst) {
    const unsigned long long n = sp.start[NSHARD];
    const K lowmask = (K(1) << ly.used) - 1;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        int sh = 0;
#pragma unroll
        for (int q = 1; q < NSHARD; q++) sh += (i >= sp.start[q]) ? 1 : 0;
        const K k = src[(unsigned long long)sh * cap + (i - sp.start[sh])];
        dst[i] = ((k >> ly.ubits) << ly.used) | (k & lowmask);
    }
}

__device__ __forceinline__ uint32_t uc_block_max(uint32_t c, uint32_t* s_wave) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c = max(c, (uint32_t)__shfl_xor(c, d, 64));
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    const uint32_t t = max(max(s_wave[0], s_wave[1]), max(s_wave[2], s_wave[3]));
    __syncthreads();
    return t;
}

// the groups of at most UC_SMALL keys; blk: UCW_ROWS rows of nb words
template <class K>
__global__ __launch_bounds__(UC_BLOCK) void k_uc_small(const K* __restrict__ d, long long nd, UcLayout<K> ly, uint8_t* __restrict__ root, uint32_t* __restrict__ blk, long long nb) {
    __shared__ K tile[UC_SPAN];
    __shared__ uint16_t s_lab[UC_SPAN];
    __shared__ uint32_t s_wave[UC_BLOCK / 64];
    volatile uint16_t* lab = s_lab;
    const long long base = (long long)blockIdx.x * UC_TILE - UC_SMALL;    // key of D at place 0 of the tile
    const int lo = base < 0 ? (int)-base : 0, hi = (int)min((long long)UC_SPAN, nd - base);
#pragma unroll
    for (int t = 0; t < UC_STRIPS; t++) {
        const int e = t * UC_BLOCK + threadIdx.x;
        if (e >= lo && e < hi) tile[e] = d[base + e];
        if (e < UC_SPAN) s_lab[e] = (uint16_t)e;
    }
    __syncthreads();
    unsigned long long adj[UC_STRIPS];                                    // per key: its adjacent members, bit j = member gs + j
    uint16_t gs[UC_STRIPS]; uint8_t gn[UC_STRIPS];                        // its group's first place and size (0: not a group of this path, or not whole in the tile)
    uint32_t groups = 0, changed = 0, opaque = 0, bigs = 0, mx = 0;
#pragma unroll
    for (int t = 0; t < UC_STRIPS; t++) {
        const int e = t * UC_BLOCK + threadIdx.x;
        adj[t] = 0; gs[t] = 0; gn[t] = 0;
        if (e < lo || e >= hi) continue;
        const K me = tile[e], myrc = ly.rc(me);
        const unsigned long long u = ly.umi(me);
        const bool own = e >= UC_SMALL && e < UC_SMALL + UC_TILE;
        if (own) {
            opaque += (u & ly.imask) ? 1u : 0u;
            const bool head = base + e == 0 || ly.rc(tile[e - 1]) != myrc;
            groups += head ? 1u : 0u;
            if (head && base + e + UC_SMALL < nd && ly.rc(tile[e + UC_SMALL]) == myrc) bigs++;
        }
        // the group's bounds [s, en): exact, or the key is left alone (a larger group, or a group of another tile that the halo cuts)
        int s = e, en = e + 1; bool ok = true;
        for (;;) {
            if (s == lo) { ok = base + s == 0; break; }
            if (ly.rc(tile[s - 1]) != myrc) break;
            s--;
            if (e - s >= UC_SMALL) { ok = false; break; }
        }
        while (ok) {
            if (en == hi) { ok = base + en == nd; break; }
            if (ly.rc(tile[en]) != myrc) break;
            en++;
            if (en - s > UC_SMALL) ok = false;
        }
        if (!ok) continue;
        gs[t] = (uint16_t)s; gn[t] = (uint8_t)(en - s);
        if (own && s == e) mx = max(mx, (uint32_t)(en - s));
        unsigned long long m = 0;
        for (int j = s; j < en; j++) if (j != e && uc_adjacent(u, ly.umi(tile[j]), ly.imask)) m |= 1ull << (j - s);
        adj[t] = m;
    }
    __syncthreads();
    // labels: every key takes the least label among its adjacent members, then that label's label, until no key of the block moved
    for (;;) {
        int moved = 0;
#pragma unroll
        for (int t = 0; t < UC_STRIPS; t++) {
            unsigned long long mm = adj[t];
            if (!mm) continue;
            const int e = t * UC_BLOCK + threadIdx.x;
            const uint16_t mine = lab[e];
            uint16_t m = mine;
            while (mm) { const int j = gs[t] + __builtin_ctzll(mm); mm &= mm - 1; const uint16_t l = lab[j]; if (l < m) m = l; }
            m = lab[m];                                                   // (labels only fall: lab[x] <= x)
            if (m < mine) { lab[e] = m; moved = 1; }
        }
        if (!__syncthreads_or(moved)) break;
    }
#pragma unroll
    for (int t = 0; t < UC_STRIPS; t++) {
        const int e = t * UC_BLOCK + threadIdx.x;
        if (!gn[t] || e < UC_SMALL || e >= UC_SMALL + UC_TILE) continue;
        root[base + e] = lab[e] == e ? 1 : 0;
        if (gs[t] == e && gn[t] >= 2) {                                   // the head counts its group's roots
            uint32_t r = 0;
            for (int j = e; j < e + gn[t]; j++) r += lab[j] == j ? 1u : 0u;
            changed += r < gn[t] ? 1u : 0u;
        }
    }
    const uint32_t tg = uf_block_sum(groups, s_wave), tc = uf_block_sum(changed, s_wave), to = uf_block_sum(opaque, s_wave), tb = uf_block_sum(bigs, s_wave),
                   tx = uc_block_max(mx, s_wave);
    if (threadIdx.x == 0) {
        blk[UCW_GROUPS * nb + blockIdx.x] = tg; blk[UCW_CHANGED * nb + blockIdx.x] = tc; blk[UCW_OPAQUE * nb + blockIdx.x] = to;
        blk[UCW_BIG * nb + blockIdx.x] = tb; blk[UCW_MAX * nb + blockIdx.x] = tx;
    }
}

// the first keys of the groups of more than UC_SMALL keys, in order: start[off[tile] ..) (the test k_uc_small counted with)
template <class K>
__global__ __launch_bounds__(UC_BLOCK) void k_uc_big_list(const K* __restrict__ d, long long nd, UcLayout<K> ly, const unsigned long long* __restrict__ off,
                                                          unsigned long long* __restrict__ start) {
    __shared__ uint32_t s_wave[UC_BLOCK / 64];
    const long long base = (long long)blockIdx.x * UC_TILE;
    unsigned long long at = off[blockIdx.x];
    for (int t = 0; t < UC_ITEMS; t++) {
        const long long i = base + t * UC_BLOCK + threadIdx.x;
        bool big = false;
        if (i + UC_SMALL < nd) {
            const K myrc = ly.rc(d[i]);
            big = (i == 0 || ly.rc(d[i - 1]) != myrc) && ly.rc(d[i + UC_SMALL]) == myrc;
        }
        uint32_t total;
        const uint32_t x = block_excl_scan(big ? 1u : 0u, s_wave, total);
        if (big) start[at + x] = (unsigned long long)i;
        at += total;
    }
}

// the codes and parents of one larger group: in LDS, or the codes in D and the parents in the workspace
struct UcLds {
    const unsigned long long* u; uint32_t* p;
    __device__ __forceinline__ unsigned long long key(uint32_t i) const { return u[i]; }
    __device__ __forceinline__ uint32_t ld(uint32_t i) const { return __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ void st(uint32_t i, uint32_t v) const { __hip_atomic_store(&p[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ uint32_t cas(uint32_t i, uint32_t expect, uint32_t v) const { return atomicCAS(&p[i], expect, v); }
};
template <class K> struct UcGlobal {
    const K* d; UcLayout<K> ly; uint32_t* p;
    __device__ __forceinline__ unsigned long long key(uint32_t i) const { return ly.umi(d[i]); }
    __device__ __forceinline__ uint32_t ld(uint32_t i) const { return __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void st(uint32_t i, uint32_t v) const { __hip_atomic_store(&p[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint32_t cas(uint32_t i, uint32_t expect, uint32_t v) const { return atomicCAS(&p[i], expect, v); }
};
// parents only fall (p[x] <= x), a root is linked by compare-and-swap alone, and path halving writes an ancestor over a parent of a
// key that is no root: every interleaving leaves a forest of the same components
template <class A> __device__ __forceinline__ uint32_t uc_find(const A& a, uint32_t x) {
    uint32_t p = a.ld(x);
    while (p != x) { const uint32_t gp = a.ld(p); if (gp != p) a.st(x, gp); x = p; p = gp; }
    return x;
}
template <class A> __device__ __forceinline__ void uc_unite(const A& a, uint32_t x, uint32_t y) {
    for (;;) {
        x = uc_find(a, x); y = uc_find(a, y);
        if (x == y) return;
        if (x < y) { const uint32_t t = x; x = y; y = t; }                // the larger root goes under the smaller
        if (a.cas(x, x, y) == x) return;
    }
}
// every key of the group [0, m) against its substitution neighbours with a smaller code (each edge from its upper end)
template <class A> __device__ __forceinline__ void uc_links(const A& a, uint32_t m, unsigned long long imask) {
    for (uint32_t i = threadIdx.x; i < m; i += UC_BIG_BLOCK) {
        const unsigned long long u = a.key(i);
        if ((u & imask) || u == 0) continue;
        const int lz = __clzll((long long)u), lead = 63 - lz;
        for (int b = 0; 2 * b < lead; b++)
            for (unsigned long long s = 1; s < 4; s++) {
                const unsigned long long v = u ^ (s << (2 * b));
                if (v >= u || v == 0 || __clzll((long long)v) != lz) continue;
                uint32_t lo = 0, hi = i;                                  // the codes are sorted: v < u lies before i
                while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a.key(mid) < v) lo = mid + 1; else hi = mid; }
                if (lo < i && a.key(lo) == v) uc_unite(a, i, lo);
            }
    }
}

// one workgroup per group of more than UC_SMALL keys; bw: three rows of nbig words [changed | keys of a medium group | keys of a giant group]
template <class K>
__global__ __launch_bounds__(UC_BIG_BLOCK) void k_uc_big(const K* __restrict__ d, long long nd, UcLayout<K> ly, const unsigned long long* __restrict__ start,
                                                         uint32_t* __restrict__ parent, uint8_t* __restrict__ root, uint32_t* __restrict__ size, uint32_t* __restrict__ bw, long long nbig) {
    __shared__ unsigned long long s_u[UC_MEDIUM];
    __shared__ uint32_t s_p[UC_MEDIUM];
    __shared__ uint32_t s_cnt[UC_BIG_BLOCK / 64];
    __shared__ unsigned long long s_end;
    const unsigned long long s = start[blockIdx.x];
    if (threadIdx.x == 0) {                                               // the group's end: the first key behind s + UC_SMALL with another (row, cell)
        const K myrc = ly.rc(d[s]);
        unsigned long long lo = s + UC_SMALL + 1, hi = (unsigned long long)nd;
        while (lo < hi) { const unsigned long long mid = (lo + hi) >> 1; if (ly.rc(d[mid]) == myrc) lo = mid + 1; else hi = mid; }
        s_end = lo;
    }
    __syncthreads();
    const uint32_t m = (uint32_t)(s_end - s);
    uint32_t r = 0;
    if (m <= (uint32_t)UC_MEDIUM) {
        for (uint32_t i = threadIdx.x; i < m; i += UC_BIG_BLOCK) { s_u[i] = ly.umi(d[s + i]); s_p[i] = i; }
        __syncthreads();
        const UcLds a{s_u, s_p};
        uc_links(a, m, ly.imask);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < m; i += UC_BIG_BLOCK) { const bool is_root = a.ld(i) == i; root[s + i] = is_root ? 1 : 0; r += is_root ? 1u : 0u; }
    } else {
        const UcGlobal<K> a{d + s, ly, parent + s};
        for (uint32_t i = threadIdx.x; i < m; i += UC_BIG_BLOCK) a.st(i, i);
        __threadfence(); __syncthreads();
        uc_links(a, m, ly.imask);
        __threadfence(); __syncthreads();
        for (uint32_t i = threadIdx.x; i < m; i += UC_BIG_BLOCK) { const bool is_root = a.ld(i) == i; root[s + i] = is_root ? 1 : 0; r += is_root ? 1u : 0u; }
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) r += __shfl_xor(r, x, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t roots = 0;
        for (int w = 0; w < UC_BIG_BLOCK / 64; w++) roots += s_cnt[w];
        size[blockIdx.x] = m;
        bw[blockIdx.x] = roots < m ? 1u : 0u;
        bw[nbig + blockIdx.x] = m <= (uint32_t)UC_MEDIUM ? m : 0u;
        bw[2 * nbig + blockIdx.x] = m <= (uint32_t)UC_MEDIUM ? 0u : m;
    }
}

// the largest of the per-tile maxima of k_uc_small and the sizes of the larger groups
__global__ __launch_bounds__(1024) void k_uc_max(const uint32_t* __restrict__ a, long long na, const uint32_t* __restrict__ b, long long nb, unsigned long long* __restrict__ out) {
    __shared__ uint32_t s_w[16];
    uint32_t c = 0;
    for (long long i = threadIdx.x; i < na; i += 1024) c = max(c, a[i]);
    for (long long i = threadIdx.x; i < nb; i += 1024) c = max(c, b[i]);
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) c = max(c, (uint32_t)__shfl_xor(c, x, 64));
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t t = 0; for (int w = 0; w < 16; w++) t = max(t, s_w[w]); *out = t; }
}

// roots per tile of D
__global__ __launch_bounds__(UC_BLOCK) void k_uc_count(const uint8_t* __restrict__ root, long long nd, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_wave[UC_BLOCK / 64];
    const long long base = (long long)blockIdx.x * UC_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int t = 0; t < UC_ITEMS; t++) { const long long i = base + t * UC_BLOCK + threadIdx.x; if (i < nd && root[i]) c++; }
    const uint32_t total = uf_block_sum(c, s_wave);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}
// ... written in the order of D, in the handle's key layout, to dst[off[tile] ..)
template <class K>
__global__ __launch_bounds__(UC_BLOCK) void k_uc_emit(const K* __restrict__ d, long long nd, const uint8_t* __restrict__ root, const unsigned long long* __restrict__ off,
                                                      UcLayout<K> ly, K* __restrict__ dst) {
    __shared__ uint32_t s_wave[UC_BLOCK / 64];
    const long long base = (long long)blockIdx.x * UC_TILE;
    unsigned long long at = off[blockIdx.x];
    for (int t = 0; t < UC_ITEMS; t++) {
        const long long i = base + t * UC_BLOCK + threadIdx.x;
        const bool keep = i < nd && root[i];
        uint32_t total;
        const uint32_t x = block_excl_scan(keep ? 1u : 0u, s_wave, total);
        if (keep) dst[at + x] = ly.widen(d[i]);
        at += total;
    }
}

static const char* const WS_UC_FULL = "workspace exhausted (UMI collapsing)";
// The keys of the shard slices (n of them, n > 0) -> one key per connected component, packed at the front of the hit buffer (cur[] /
// cursor say where they are), and counted into matrix 0.
template <class K>
static int umi_collapse_fold(EngineImpl* im, size_t n) {
    Timer tm{im, im->ev0, im->ev1};
    int rc;
    UcLayout<K> ly; ly.ubits = im->ubits; ly.used = im->ubits; ly.imask = 1ull << (std::min(im->ubits, 64) - 1);
    if (sizeof(K) == 8) { unsigned long long uor = 0; for (int sh = 0; sh < NSHARD; sh++) uor |= im->h_ctl[ctl_umi_or(sh)]; ly.used = std::min(im->ubits, uor ? 64 - __builtin_clzll(uor) : 1); }
    if (n >= (size_t(1) << 32)) { im->eng->err = "UMI collapsing: more than 2^32 keys on one handle"; return XCK_E_CAPACITY; }
    const int top = ly.used + im->cbits + im->rbits;
    const size_t tmpb = sort_tmp_bytes<K, rocprim::empty_type>(n, top);
    UmiCollapseWs w;
    if ((rc = pf_carve(im, im->ws1, true, [&](Arena& ar) { umi_collapse_carve(ar, n, sizeof(K), tmpb, w); }, WS_UC_FULL))) return rc;
    K* A = (K*)w.a; K* B = (K*)w.b;
    if ((rc = tm.start())) return rc;
    hipLaunchKernelGGL((k_uc_pack<K>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, im->s_comp,
                       (const K*)im->d_keys, (unsigned long long)im->hit_cap, shard_span(im->cur), ly, A);
    HIP_TRY(hipGetLastError());
    if ((rc = sort_run<K, rocprim::empty_type>(im, w.tmp, tmpb, A, B, nullptr, nullptr, n, top))) return rc;
    // the distinct keys D: B -> A
    const size_t nb = (n + UC_TILE - 1) / UC_TILE;
    const unsigned long long* h;
    hipLaunchKernelGGL((k_uf_heads<K>), dim3((unsigned)nb), dim3(UF_BLOCK), 0, im->s_comp, (const K*)B, (long long)n, w.d_blk);
    hipLaunchKernelGGL(k_cp_scan, dim3(1), dim3(1024), 0, im->s_comp, (const uint32_t*)w.d_blk, (long long)nb, w.d_off, im->d_ctl + CTL_SCRATCH);
    if ((rc = read_ctl_words(im, CTL_SCRATCH, 1, h))) return rc;
    const size_t nd = h[0];
    if (nd == 0 || nd > n) { im->eng->err = "internal: distinct keys of the UMI collapsing stage out of range"; return XCK_E_STATE; }
    hipLaunchKernelGGL((k_uf_distinct<K>), dim3((unsigned)nb), dim3(UF_BLOCK), 0, im->s_comp, (const K*)B, (long long)n, (const unsigned long long*)w.d_off, A);
    // the groups of the tile path, and the sums (the k_expand words are the pileup pipeline's: free on this one)
    const size_t nbd = (nd + UC_TILE - 1) / UC_TILE;
    hipLaunchKernelGGL((k_uc_small<K>), dim3((unsigned)nbd), dim3(UC_BLOCK), 0, im->s_comp, (const K*)A, (long long)nd, ly, w.root, w.d_blk, (long long)nbd);
    hipLaunchKernelGGL(k_cp_scan, dim3(UCW_MAX), dim3(1024), 0, im->s_comp, (const uint32_t*)w.d_blk, (long long)nbd, w.d_off, im->d_ctl + CTL_X0);
    if ((rc = read_ctl_words(im, CTL_X0, UCW_MAX, h))) return rc;
    const size_t groups = h[UCW_GROUPS], opaque = h[UCW_OPAQUE], nbig = h[UCW_BIG];
    size_t changed = h[UCW_CHANGED];
    if (groups == 0 || groups > nd || opaque > nd || changed > groups || nbig > w.big_cap) { im->eng->err = "internal: counters of the UMI collapsing stage out of range"; return XCK_E_STATE; }
    // the larger groups (B is free: the parents of the groups beyond UC_MEDIUM keys lie in it, one word per key of D)
    if (nbig) {
        hipLaunchKernelGGL((k_uc_big_list<K>), dim3((unsigned)nbd), dim3(UC_BLOCK), 0, im->s_comp, (const K*)A, (long long)nd, ly,
                           (const unsigned long long*)(w.d_off + UCW_BIG * nbd), w.big_start);
        hipLaunchKernelGGL((k_uc_big<K>), dim3((unsigned)nbig), dim3(UC_BIG_BLOCK), 0, im->s_comp, (const K*)A, (long long)nd, ly, (const unsigned long long*)w.big_start,
                           (uint32_t*)w.b, w.root, w.big_size, w.big_words, (long long)nbig);
        hipLaunchKernelGGL(k_cp_scan, dim3(3), dim3(1024), 0, im->s_comp, (const uint32_t*)w.big_words, (long long)nbig, w.big_off, im->d_ctl + CTL_X0 + 2);
    } else
        HIP_TRY(hipMemsetAsync(im->d_ctl + CTL_X0 + 2, 0, 3 * sizeof(unsigned long long), im->s_comp));
    hipLaunchKernelGGL(k_uc_max, dim3(1), dim3(1024), 0, im->s_comp, (const uint32_t*)(w.d_blk + UCW_MAX * nbd), (long long)nbd, (const uint32_t*)w.big_size, (long long)nbig, im->d_ctl + CTL_X0 + 1);
    hipLaunchKernelGGL(k_uc_count, dim3((unsigned)nbd), dim3(UC_BLOCK), 0, im->s_comp, (const uint8_t*)w.root, (long long)nd, w.d_blk);
    hipLaunchKernelGGL(k_cp_scan, dim3(1), dim3(1024), 0, im->s_comp, (const uint32_t*)w.d_blk, (long long)nbd, w.d_off, im->d_ctl + CTL_X0);
    if ((rc = read_ctl_words(im, CTL_X0, 5, h))) return rc;
    const size_t nr = h[0], max_group = h[1], keys_medium = h[3], keys_giant = h[4];
    changed += h[2];
    if (nr == 0 || nr > nd || nr < groups || changed > groups || max_group > nd || keys_medium + keys_giant > nd) { im->eng->err = "internal: components of the UMI collapsing stage out of range"; return XCK_E_STATE; }
    im->uc_stats[UC_KEYS] = (long long)nd; im->uc_stats[UC_MOLECULES] = (long long)nr; im->uc_stats[UC_GROUPS] = (long long)groups;
    im->uc_stats[UC_CHANGED] = (long long)changed; im->uc_stats[UC_OPAQUE] = (long long)opaque; im->uc_stats[UC_MAX_GROUP] = (long long)max_group;
    hipLaunchKernelGGL((k_uc_emit<K>), dim3((unsigned)nbd), dim3(UC_BLOCK), 0, im->s_comp, (const K*)A, (long long)nd, (const uint8_t*)w.root, (const unsigned long long*)w.d_off, ly, (K*)im->d_keys);
    HIP_TRY(hipGetLastError());
    im->cursor = nr;
    for (int sh = 0; sh < NSHARD; sh++) { const size_t lo = (size_t)sh * im->hit_cap; im->cur[sh] = nr > lo ? std::min(nr - lo, im->hit_cap) : 0; }
    if (im->eng->knobs.debug_timing)
        fprintf(stderr, "[xck] UMI collapsing: n=%zu distinct=%zu components=%zu groups=%zu changed=%zu opaque=%zu max group=%zu larger groups=%zu keys medium=%zu giant=%zu sort bits=%d\n",
                n, nd, nr, groups, changed, opaque, max_group, nbig, keys_medium, keys_giant, top);
    // the roots are distinct and in (row, cell, UMI) order: counted as they are
    RadixFoldWs fw; fw.alt = nullptr; fw.tmp = nullptr; fw.d_blk = w.d_blk; fw.d_off = w.d_off; fw.coo_at = w.coo_at;
    if ((rc = fold_coo<K>(im, im->ws1, fw, (const K*)im->d_keys, nr, key_layout<K>(im), 0, 0))) return rc;
    return tm.stop(&im->st.ms_sort);
}

int umi_collapse_reset(EngineImpl* im) {
    im->uc_stats_valid = false;
    for (long long& v : im->uc_stats) v = 0;
    return 0;
}

// xck_get_umi_dedup_stats() for the basefc pipeline: the counters the last xck_finish left
int engine_umi_dedup_stats(EngineImpl* im, xck_umi_dedup_stats* out) {
    xck_engine* e = im->eng;
    if (!im->umi_collapse) { e->err = "handle made without XCK_F_UMI_COLLAPSE"; return XCK_E_STATE; }
    if (im->fold_failed || !im->finished || !im->uc_stats_valid) { e->err = "xck_get_umi_dedup_stats: valid between a successful xck_finish and the next xck_reset"; return XCK_E_STATE; }
    out->keys = im->uc_stats[UC_KEYS]; out->molecules = im->uc_stats[UC_MOLECULES]; out->groups = im->uc_stats[UC_GROUPS];
    out->groups_changed = im->uc_stats[UC_CHANGED]; out->opaque_keys = im->uc_stats[UC_OPAQUE]; out->max_group = im->uc_stats[UC_MAX_GROUP];
    return 0;
}
