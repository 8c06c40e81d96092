// umi_feature.h - opt-in unique-feature molecules of the basefc fold (XCK_F_UNIQUE_FEATURE / XCK_UMI_FEATURE=unique;
// xck_get_umi_feature_stats, include/xck.h).  Included by finish.hip inside namespace xck, behind the radix-sort fold's helpers and
// fold_partition.h: it uses KeyLayout, ShardSpan, block_excl_scan, k_cp_scan, read_ctl_words, Timer, sort_run / sort_tmp_bytes, pf_carve
// and HIP_TRY.  DESIGN.md section 3.13.
//
// The default fold counts R, the distinct (row, cell, UMI) keys the join accepted.  Under the flag a key of R counts only when its
// molecule - (contig of the row, cell, UMI) - has no other row in R on that contig.  The fold groups by (row, cell); this stage groups
// by molecule first, ahead of it, and hands the fold the surviving keys:
//   k_uf_rekey     shard slices -> one array of molecule-major keys  cell | umi | rank(row)  (64-bit keys: the UMI field narrowed to
//                  its used bits, as k_pack_squeeze does).  rank = the row's place in the join table's (contig, start, end, index)
//                  order: a permutation of the table's rows, so it fits the row field, and the ranks of a contig are one range.
//   sort           rocPRIM over all key bits from bit 0 (sort_run; finish.hip on begin_bit > 0 with end_bit = 64)
//   k_uf_heads / k_uf_distinct   the distinct keys D, in order (a key repeated across tiles and batches is the common case): after
//                  this a molecule's keys are its distinct rows, adjacent, ascending by rank and therefore contig by contig
//   k_uf_verdict   D[i] drops iff D[i - 1] or D[i + 1] has the same (cell, UMI) and a rank inside the range of D[i]'s contig.  Per
//                  tile: survivors, molecules (keys without such a predecessor) and multi-feature molecules (... that have such a
//                  successor) - three words per block that k_cp_scan sums; no atomics
//   k_uf_emit      the survivors as ordinary (row, cell, UMI) keys, packed at the front of the hit buffer: the shard slices lie back
//                  to back in it, so slice s then holds the keys [s * hit_cap, (s + 1) * hit_cap) of them
// The survivors arrive cell-major, which level 1 of the partition fold is not built for (it relies on few rows being active at any
// place of the stream): the radix-sort fold, which takes every input, counts them (fold_path = 2).
//
// A plurality rule (the molecule goes to the row with most reads) is not possible here: the join removes duplicate keys in its LDS
// set before they reach HBM, so the fold never sees read multiplicities.
#pragma once

constexpr int UF_BLOCK = 256, UF_ITEMS = 8, UF_TILE = UF_BLOCK * UF_ITEMS;
static_assert(UF_TILE == (int)WS_TILE && UF_BLOCK == JOIN_BLOCK, "fold_ws.h sizes the per-tile words by this; block_excl_scan scans JOIN_BLOCK threads");
enum { UF_MOLECULES, UF_MULTI, UF_KEYS, UF_DROPPED };              // EngineImpl::uf_stats

// molecule-major form of a key: cell | umi (used bits) | rank
template <class K> struct MolLayout {
    int ubits, cbits, rbits, used;                                   // the handle's key layout; UMI bits in use (<= ubits)
    __device__ __forceinline__ K umask() const { return (K(1) << used) - 1; }
    __device__ __forceinline__ K to_mol(K k, uint32_t rank) const {
        const K cell = (k >> ubits) & ((K(1) << cbits) - 1);
        return (cell << (used + rbits)) | ((k & umask()) << rbits) | K(rank);
    }
    __device__ __forceinline__ K from_mol(K m, uint32_t row) const {
        return (K(row) << (cbits + ubits)) | ((m >> (used + rbits)) << ubits) | ((m >> rbits) & umask());
    }
    __device__ __forceinline__ uint32_t row(K k) const { return uint32_t(k >> (cbits + ubits)); }
    __device__ __forceinline__ uint32_t rank(K m) const { return uint32_t(m) & uint32_t((1ull << rbits) - 1); }
    __device__ __forceinline__ K mol(K m) const { return m >> rbits; }
};

template <class K>
__global__ void __launch_bounds__(256) k_uf_rekey(const K* __restrict__ src, unsigned long long cap, ShardSpan sp, MolLayout<K> ml,
                                                    const uint32_t* __restrict__ rank_of, K* __restrict__ dst) {
    const unsigned long long n = sp.start[NSHARD];
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        int sh = 0;
#pragma unroll
        for (int q = 1; q < NSHARD; q++) sh += (i >= sp.start[q]) ? 1 : 0;
        const K k = src[(unsigned long long)sh * cap + (i - sp.start[sh])];
        dst[i] = ml.to_mol(k, rank_of[ml.row(k)]);
    }
}

// sum of one word per thread over the block -> thread 0 (s_wave: UF_BLOCK / 64 words)
__device__ __forceinline__ uint32_t uf_block_sum(uint32_t c, uint32_t* s_wave) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    const uint32_t t = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
    return t;
}

// distinct keys of every tile of the sorted stream (striped: lane-contiguous loads)
template <class K>
__global__ __launch_bounds__(UF_BLOCK) void k_uf_heads(const K* __restrict__ k, long long n, uint32_t* __restrict__ blk) {
    __shared__ uint32_t s_wave[UF_BLOCK / 64];
    const long long base = (long long)blockIdx.x * UF_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int t = 0; t < UF_ITEMS; t++) {
        const long long i = base + t * UF_BLOCK + threadIdx.x;
        if (i < n && (i == 0 || k[i] != k[i - 1])) c++;
    }
    const uint32_t total = uf_block_sum(c, s_wave);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// ... written in order to dst[off[tile] ..): one block scan per stripe of UF_BLOCK keys
template <class K>
__global__ __launch_bounds__(UF_BLOCK) void k_uf_distinct(const K* __restrict__ k, long long n, const unsigned long long* __restrict__ off, K* __restrict__ dst) {
    __shared__ uint32_t s_wave[UF_BLOCK / 64];
    const long long base = (long long)blockIdx.x * UF_TILE;
    unsigned long long at = off[blockIdx.x];
    for (int t = 0; t < UF_ITEMS; t++) {                                  // (every thread of the block takes every turn: the scan has barriers)
        const long long i = base + t * UF_BLOCK + threadIdx.x;
        K me = K(0); bool head = false;
        if (i < n) { me = k[i]; head = i == 0 || me != k[i - 1]; }
        uint32_t total;
        const uint32_t x = block_excl_scan(head ? 1u : 0u, s_wave, total);
        if (head) dst[at + x] = me;
        at += total;
    }
}

// the verdict over the distinct keys d[0, nd); blk: three rows of nb words [survivors | molecules | multi-feature molecules]
template <class K>
__global__ __launch_bounds__(UF_BLOCK) void k_uf_verdict(const K* __restrict__ d, long long nd, MolLayout<K> ml, const uint2* __restrict__ span,
                                                         uint8_t* __restrict__ drop, uint32_t* __restrict__ blk, long long nb) {
    __shared__ uint32_t s_wave[UF_BLOCK / 64];
    const long long base = (long long)blockIdx.x * UF_TILE;
    uint32_t keep = 0, mols = 0, multi = 0;
#pragma unroll
    for (int t = 0; t < UF_ITEMS; t++) {
        const long long i = base + t * UF_BLOCK + threadIdx.x;
        if (i < nd) {
            const K me = d[i];
            const uint2 sp = span[ml.rank(me)];                          // ranks of the contig of `me`: [x, y)
            bool with_prev = false, with_next = false;
            if (i > 0) { const K p = d[i - 1]; with_prev = ml.mol(p) == ml.mol(me) && ml.rank(p) >= sp.x; }
            if (i + 1 < nd) { const K q = d[i + 1]; with_next = ml.mol(q) == ml.mol(me) && ml.rank(q) < sp.y; }
            const bool dr = with_prev || with_next;
            drop[i] = dr ? 1 : 0;
            keep += dr ? 0u : 1u; mols += with_prev ? 0u : 1u; multi += (!with_prev && with_next) ? 1u : 0u;
        }
    }
    const uint32_t tk = uf_block_sum(keep, s_wave), tm = uf_block_sum(mols, s_wave), tx = uf_block_sum(multi, s_wave);
    if (threadIdx.x == 0) { blk[blockIdx.x] = tk; blk[nb + blockIdx.x] = tm; blk[2 * nb + blockIdx.x] = tx; }
}

// the survivors, in the order of d, as (row, cell, UMI) keys at dst[off[tile] ..)
template <class K>
__global__ __launch_bounds__(UF_BLOCK) void k_uf_emit(const K* __restrict__ d, long long nd, const uint8_t* __restrict__ drop, const unsigned long long* __restrict__ off,
                                                      MolLayout<K> ml, const int32_t* __restrict__ row_of, K* __restrict__ dst) {
    __shared__ uint32_t s_wave[UF_BLOCK / 64];
    const long long base = (long long)blockIdx.x * UF_TILE;
    unsigned long long at = off[blockIdx.x];
    for (int t = 0; t < UF_ITEMS; t++) {
        const long long i = base + t * UF_BLOCK + threadIdx.x;
        const bool keep = i < nd && !drop[i];
        uint32_t total;
        const uint32_t x = block_excl_scan(keep ? 1u : 0u, s_wave, total);
        if (keep) { const K me = d[i]; dst[at + x] = ml.from_mol(me, (uint32_t)row_of[ml.rank(me)]); }
        at += total;
    }
}

static const char* const WS_UF_FULL = "workspace exhausted (unique-feature molecules)";
// The keys of the shard slices (n of them, n > 0) -> the keys of the unique-feature molecules, packed at the front of the hit buffer;
// cur[] / cursor say where they are.  *n_out = their number.
template <class K>
static int unique_feature_keys(EngineImpl* im, size_t n, size_t* n_out) {
    Timer tm{im, im->ev0, im->ev1};
    int rc;
    MolLayout<K> ml; ml.ubits = im->ubits; ml.cbits = im->cbits; ml.rbits = im->rbits; ml.used = im->ubits;
    if (sizeof(K) == 8) { unsigned long long uor = 0; for (int sh = 0; sh < NSHARD; sh++) uor |= im->h_ctl[ctl_umi_or(sh)]; ml.used = std::min(im->ubits, uor ? 64 - __builtin_clzll(uor) : 1); }
    const int top = ml.cbits + ml.used + ml.rbits;
    const size_t tmpb = sort_tmp_bytes<K, rocprim::empty_type>(n, top);
    UniqueFeatureWs w;
    if ((rc = pf_carve(im, im->ws1, true, [&](Arena& ar) { unique_feature_carve(ar, n, sizeof(K), tmpb, w); }, WS_UF_FULL))) return rc;
    K* A = (K*)w.a; K* B = (K*)w.b;
    if ((rc = tm.start())) return rc;
    hipLaunchKernelGGL((k_uf_rekey<K>), dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, im->s_comp,
                       (const K*)im->d_keys, (unsigned long long)im->hit_cap, shard_span(im->cur), ml, (const uint32_t*)im->d_uf_rank, A);
    HIP_TRY(hipGetLastError());
    if ((rc = sort_run<K, rocprim::empty_type>(im, w.tmp, tmpb, A, B, nullptr, nullptr, n, top))) return rc;
    // the distinct keys D: B -> A
    const size_t nb = (n + UF_TILE - 1) / UF_TILE;
    const unsigned long long* h;
    hipLaunchKernelGGL((k_uf_heads<K>), dim3((unsigned)nb), dim3(UF_BLOCK), 0, im->s_comp, (const K*)B, (long long)n, w.d_blk);
    hipLaunchKernelGGL(k_cp_scan, dim3(1), dim3(1024), 0, im->s_comp, (const uint32_t*)w.d_blk, (long long)nb, w.d_off, im->d_ctl + CTL_SCRATCH);
    if ((rc = read_ctl_words(im, CTL_SCRATCH, 1, h))) return rc;
    const size_t nd = h[0];
    if (nd == 0 || nd > n) { im->eng->err = "internal: distinct keys of the unique-feature stage out of range"; return XCK_E_STATE; }
    hipLaunchKernelGGL((k_uf_distinct<K>), dim3((unsigned)nb), dim3(UF_BLOCK), 0, im->s_comp, (const K*)B, (long long)n, (const unsigned long long*)w.d_off, A);
    // the verdict, and the three sums (the k_expand words are the pileup pipeline's: free on this one)
    const size_t nbd = (nd + UF_TILE - 1) / UF_TILE;
    hipLaunchKernelGGL((k_uf_verdict<K>), dim3((unsigned)nbd), dim3(UF_BLOCK), 0, im->s_comp, (const K*)A, (long long)nd, ml, (const uint2*)im->d_uf_span, w.drop, w.d_blk, (long long)nbd);
    hipLaunchKernelGGL(k_cp_scan, dim3(3), dim3(1024), 0, im->s_comp, (const uint32_t*)w.d_blk, (long long)nbd, w.d_off, im->d_ctl + CTL_X0);
    if ((rc = read_ctl_words(im, CTL_X0, 3, h))) return rc;
    const size_t ns = h[0];
    if (ns > nd || h[1] > nd || h[2] > h[1]) { im->eng->err = "internal: counters of the unique-feature stage out of range"; return XCK_E_STATE; }
    im->uf_stats[UF_MOLECULES] = (long long)h[1]; im->uf_stats[UF_MULTI] = (long long)h[2]; im->uf_stats[UF_KEYS] = (long long)nd; im->uf_stats[UF_DROPPED] = (long long)(nd - ns);
    if (ns) {
        hipLaunchKernelGGL((k_uf_emit<K>), dim3((unsigned)nbd), dim3(UF_BLOCK), 0, im->s_comp, (const K*)A, (long long)nd, (const uint8_t*)w.drop, (const unsigned long long*)w.d_off,
                           ml, (const int32_t*)im->d_reg_row, (K*)im->d_keys);
        HIP_TRY(hipGetLastError());
    }
    im->cursor = ns;
    for (int sh = 0; sh < NSHARD; sh++) { const size_t lo = (size_t)sh * im->hit_cap; im->cur[sh] = ns > lo ? std::min(ns - lo, im->hit_cap) : 0; }
    if (im->eng->knobs.debug_timing) fprintf(stderr, "[xck] unique-feature molecules: n=%zu distinct=%zu kept=%zu molecules=%llu multi=%llu sort bits=%d\n", n, nd, ns, h[1], h[2], top);
    *n_out = ns;
    return tm.stop(&im->st.ms_sort);                                      // (waits: the emit is done before the fold begins workspace 1 anew)
}

// the rank tables (engine_create, with the flag only): the order build_tables() gave the join's region table
int unique_feature_init(EngineImpl* im, const xck_config* cfg) {
    const int nc = cfg->n_contigs;
    std::vector<int32_t> s0, e0, row, pmax, base, count;
    sort_regions_by_contig(cfg->regions, cfg->n_regions, nc, [](const xck_region& r) { return !(r.start < 1 || (int64_t)r.start - 1 > (int64_t)r.end); },
                           [](const xck_region& r) { return r.start - 1; }, s0, e0, row, pmax, base, count);
    std::vector<uint32_t> rank_of((size_t)std::max(cfg->n_regions, 1), 0u);
    std::vector<uint2> span(std::max<size_t>(row.size(), 1), make_uint2(0u, 0u));
    for (size_t r = 0; r < row.size(); r++) rank_of[(size_t)row[r]] = (uint32_t)r;
    for (int c = 0; c < nc; c++) for (int32_t r = base[c]; r < base[c] + count[c]; r++) span[(size_t)r] = make_uint2((uint32_t)base[c], (uint32_t)(base[c] + count[c]));
    HIP_TRY(hipMalloc((void**)&im->d_uf_rank, rank_of.size() * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(im->d_uf_rank, rank_of.data(), rank_of.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMalloc((void**)&im->d_uf_span, span.size() * sizeof(uint2)));
    HIP_TRY(hipMemcpy(im->d_uf_span, span.data(), span.size() * sizeof(uint2), hipMemcpyHostToDevice));
    return 0;
}
int unique_feature_reset(EngineImpl* im) {
    im->uf_stats_valid = false;
    for (long long& v : im->uf_stats) v = 0;
    return 0;
}

// xck_get_umi_feature_stats() for the basefc pipeline: the counters the last xck_finish left
int engine_umi_feature_stats(EngineImpl* im, xck_umi_feature_stats* out) {
    xck_engine* e = im->eng;
    if (!im->d_uf_rank) { e->err = "handle made without XCK_F_UNIQUE_FEATURE"; return XCK_E_STATE; }
    if (im->fold_failed || !im->finished || !im->uf_stats_valid) { e->err = "xck_get_umi_feature_stats: valid between a successful xck_finish and the next xck_reset"; return XCK_E_STATE; }
    out->molecules = im->uf_stats[UF_MOLECULES]; out->multi_feature = im->uf_stats[UF_MULTI]; out->keys = im->uf_stats[UF_KEYS]; out->keys_dropped = im->uf_stats[UF_DROPPED];
    return 0;
}
