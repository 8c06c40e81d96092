// umi_consensus.h - opt-in UMI consensus allele of the pileup fold (XCK_F_UMI_CONSENSUS / XCK_UMI_CONSENSUS=1; xck_get_molecule_stats,
// include/xck.h).  Included by finish.hip inside namespace xck, behind the first-read kernels and their launchers: it uses nib_bucket,
// RUN_WALK, KeyLayout, PileupFold, k_tally_rows / k_tally_long and HIP_TRY.  DESIGN.md section 3.11.
//
// The default fold keeps, per (SNP, cell, UMI) run of the sorted hits, the value of the read that comes first in fetch order
// (k_first_base / k_first_read), and a read that spans the SNP in a gap silences the run when it comes earlier still (k_claim).  Under
// the flag a run's allele is a plurality vote over its hits that show a base (allele code != 0):
//   buckets  A, C, G, T, N by nib_bucket(); c[b] = hits of bucket b, first[b] = its smallest value (ordinal << ALLELE_BITS | code)
//   winner   the bucket among A, C, G, T with the largest c; a tie goes to the tied bucket with the smallest first[b]; N only when
//            nothing else was seen.  The run head's allele byte is the code of first[winner] (an IUPAC nibble inside N survives).
// Hits without a base abstain and never claim: in split mode k_claim is not launched, and ordv and the filter table, which only it
// reads, are not filled; in plain mode the vote skips the code-0 hits of the stream, and a run of nothing else keeps al = 0.
//
//   k_consensus_base   split mode: k_first_base's up-front loads and its row_lo / row_hi (k_tally_rows needs them), the vote in registers
//   k_consensus_read   plain mode (128-bit keys, -DXCK_BAF_SPLIT=0): k_first_read with the vote and its tally atomics
//   k_consensus_long   runs longer than RUN_WALK: one block per run, count and minimum per bucket reduced across the block
// All three count the runs' agreement (MOL_* below): a block sums its lanes' flags by wave ballots and adds each non-zero sum with one
// atomic to one of the pipeline's copies of the five words (EngineImpl::d_mol).
#pragma once

enum { MOL_MOLECULES, MOL_MULTI_READ, MOL_DISCORDANT, MOL_TIED, MOL_CHANGED, MOL_WORDS };
// The counters are kept MOL_SLOTS times, one 64-byte line per copy, and a block adds to copy blockIdx.x % MOL_SLOTS; the getter sums the
// copies.  (One copy: 113 k blocks at configs[2] queue on five words, and k_consensus_base took 1.39 ms - the rate of atomics on one
// address - against 0.59 ms for k_first_base; profiles/r26_umi_consensus.txt.)
constexpr int MOL_SLOTS = 256, MOL_STRIDE = 8, MOL_BUF_WORDS = MOL_SLOTS * MOL_STRIDE;
static_assert(MOL_STRIDE >= MOL_WORDS && (MOL_SLOTS & (MOL_SLOTS - 1)) == 0, "a copy holds the five counters; the slot is a mask of the block index");

// the vote of one run (or of one lane's share of a long run)
struct Vote {
    uint32_t c[5]; uint64_t f[5];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int b = 0; b < 5; b++) { c[b] = 0; f[b] = ~0ull; }
    }
    __device__ __forceinline__ void add(uint64_t x) {
        const uint32_t code = uint32_t(x & ((1u << ALLELE_BITS) - 1));
        const int bk = code ? nib_bucket(int(code) - 1) : -1;            // (code 0: no base, abstains)
#pragma unroll
        for (int b = 0; b < 5; b++) if (bk == b) { c[b]++; if (x < f[b]) f[b] = x; }
    }
    __device__ __forceinline__ void merge(const uint32_t (&oc)[5], const uint64_t (&of)[5]) {
#pragma unroll
        for (int b = 0; b < 5; b++) { c[b] += oc[b]; if (of[b] < f[b]) f[b] = of[b]; }
    }
    // -> the head's allele code (0: no hit with a base); flags: bit MOL_* set where the run counts
    __device__ __forceinline__ uint32_t decide(uint32_t& flags) const {
        const uint32_t total = c[0] + c[1] + c[2] + c[3] + c[4];
        flags = 0;
        if (!total) return 0;
        int win = 4, first = 4; uint32_t best = 0, n_best = 0, n_bk = c[4] ? 1u : 0u;
        uint64_t fmin = f[4], fwin = f[4];                                // (~0 when no read shows N)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            if (!c[b]) continue;
            n_bk++;
            if (f[b] < fmin) { fmin = f[b]; first = b; }
            if (c[b] > best) { best = c[b]; n_best = 1; win = b; fwin = f[b]; }
            else if (c[b] == best) { n_best++; if (f[b] < fwin) { win = b; fwin = f[b]; } }
        }
        flags = 1u << MOL_MOLECULES;
        if (total >= 2) flags |= 1u << MOL_MULTI_READ;
        if (n_bk >= 2) flags |= 1u << MOL_DISCORDANT;
        if (n_best >= 2) flags |= 1u << MOL_TIED;
        if (win != first) flags |= 1u << MOL_CHANGED;
        return uint32_t(fwin & ((1u << ALLELE_BITS) - 1));
    }
};

// the flags of a 256-thread block's lanes -> the five counters: ballots per wave, one atomic per non-zero sum.  Every thread of the
// block calls it (no thread has returned).
__device__ __forceinline__ void mol_count_block(uint32_t flags, unsigned long long* __restrict__ mol) {
    __shared__ uint32_t s_m[4][MOL_WORDS];
#pragma unroll
    for (int q = 0; q < MOL_WORDS; q++) {
        const unsigned long long bal = __ballot((flags >> q) & 1u);
        if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6][q] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    if (threadIdx.x < MOL_WORDS) {
        const uint32_t v = s_m[0][threadIdx.x] + s_m[1][threadIdx.x] + s_m[2][threadIdx.x] + s_m[3][threadIdx.x];
        if (v) atomicAdd(&mol[(blockIdx.x & (MOL_SLOTS - 1)) * MOL_STRIDE + threadIdx.x], (unsigned long long)v);
    }
}

// split mode: per key run the voted allele code at the run head; first / one-past-last index of every SNP.  The loads are k_first_base's:
// neighbours' keys and the next two values up front, before any key is looked at (that kernel's cost is its dependent load stages).
template <class K>
__global__ void __launch_bounds__(256) k_consensus_base(const K* __restrict__ k, const uint64_t* __restrict__ v, long long n, KeyLayout<K> kl, uint8_t* __restrict__ al_out,
                                                        unsigned long long* __restrict__ row_lo, unsigned long long* __restrict__ row_hi,
                                                        unsigned long long* __restrict__ long_runs, unsigned long long* __restrict__ mol) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t flags = 0;
    if (i < n) {
        const long long ip = i > 0 ? i - 1 : 0, i1 = i + 1 < n ? i + 1 : n - 1, i2 = i + 2 < n ? i + 2 : n - 1;
        const K kp = k[ip], me = k[i], kn1 = k[i1], kn2 = k[i2];
        const uint64_t v0 = v[i], v1 = v[i1], v2 = v[i2];
        const uint32_t row = kl.row(me);
        if (i == 0 || kl.row(kp) != row) row_lo[row] = (unsigned long long)i;
        if (i + 1 == n || kl.row(kn1) != row) row_hi[row] = (unsigned long long)(i + 1);
        if (i > 0 && kp == me) al_out[i] = 0;
        else {
            Vote vt; vt.clear(); vt.add(v0);
            long long j = i + 1;
            if (j < n && kn1 == me) {
                vt.add(v1);
                j = i + 2;
                if (j < n && kn2 == me) {
                    vt.add(v2);
                    for (j = i + 3; j < n && j <= i + RUN_WALK && k[j] == me; j++) vt.add(v[j]);
                }
            }
            if (j < n && j > i + RUN_WALK && k[j] == me) long_runs[1 + atomicAdd(&long_runs[0], 1ull)] = (unsigned long long)i;   // al and counters of this head: k_consensus_long
            else al_out[i] = (uint8_t)vt.decide(flags);
        }
    }
    mol_count_block(flags, mol);
}

// plain mode: every hit, with a base or without, is in the stream; the head also adds its allele to the SNP's tallies
template <class K>
__global__ void __launch_bounds__(256) k_consensus_read(const K* __restrict__ k, const uint64_t* __restrict__ v, long long n, KeyLayout<K> kl, uint8_t* __restrict__ al_out,
                                                        uint32_t* __restrict__ tally, unsigned long long* __restrict__ long_runs, unsigned long long* __restrict__ mol) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t flags = 0;
    if (i < n) {
        const K me = k[i];
        if (i > 0 && k[i - 1] == me) al_out[i] = 0;
        else {
            Vote vt; vt.clear(); vt.add(v[i]);
            long long j = i + 1;
            for (; j < n && j <= i + RUN_WALK && k[j] == me; j++) vt.add(v[j]);
            if (j < n && j > i + RUN_WALK && k[j] == me) long_runs[1 + atomicAdd(&long_runs[0], 1ull)] = (unsigned long long)i;   // finished by k_consensus_long
            else {
                const uint32_t code = vt.decide(flags);
                al_out[i] = (uint8_t)code;
                if (code) atomicAdd(&tally[(size_t)kl.row(me) * 5 + nib_bucket(int(code) - 1)], 1u);
            }
        }
    }
    mol_count_block(flags, mol);
}

// a run longer than RUN_WALK: ONE BLOCK per run (k_first_long's bisection for the run's end), every lane votes over its stride, the
// five counts and five minima are put together by shuffles and through LDS.  SPLIT: the tallies are k_tally_rows', else added here.
template <class K, bool SPLIT>
__global__ void __launch_bounds__(256) k_consensus_long(const K* __restrict__ k, const uint64_t* __restrict__ v, long long n, KeyLayout<K> kl,
                                                        const unsigned long long* __restrict__ long_runs, uint8_t* __restrict__ al_out,
                                                        uint32_t* __restrict__ tally, unsigned long long* __restrict__ mol) {
    __shared__ uint32_t s_c[4][5];
    __shared__ unsigned long long s_f[4][5];
    const unsigned long long n_long = long_runs[0];
    uint32_t sum[MOL_WORDS] = {0, 0, 0, 0, 0};                            // (thread 0: over the runs of this block)
    for (unsigned long long r = blockIdx.x; r < n_long; r += gridDim.x) {
        const long long h = (long long)long_runs[1 + r];
        const K me = k[h];
        long long lo = h + 1, hi = n;                                     // first index past the run
        while (lo < hi) { const long long mid = lo + ((hi - lo) >> 1); if (k[mid] == me) lo = mid + 1; else hi = mid; }
        Vote vt; vt.clear();
        for (long long j = h + threadIdx.x; j < lo; j += blockDim.x) vt.add(v[j]);
#pragma unroll
        for (int b = 0; b < 5; b++)
            for (int d = 32; d; d >>= 1) {
                vt.c[b] += __shfl_xor(vt.c[b], d);
                const unsigned long long o = __shfl_xor((unsigned long long)vt.f[b], d);
                if (o < vt.f[b]) vt.f[b] = o;
            }
        if ((threadIdx.x & 63) == 0) { for (int b = 0; b < 5; b++) { s_c[threadIdx.x >> 6][b] = vt.c[b]; s_f[threadIdx.x >> 6][b] = vt.f[b]; } }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; w++) {
                uint32_t oc[5]; uint64_t of[5];
                for (int b = 0; b < 5; b++) { oc[b] = s_c[w][b]; of[b] = s_f[w][b]; }
                vt.merge(oc, of);
            }
            uint32_t flags;
            const uint32_t code = vt.decide(flags);
            al_out[h] = (uint8_t)code;
            if (!SPLIT && code) atomicAdd(&tally[(size_t)kl.row(me) * 5 + nib_bucket(int(code) - 1)], 1u);
            for (int q = 0; q < MOL_WORDS; q++) sum[q] += (flags >> q) & 1u;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { for (int q = 0; q < MOL_WORDS; q++) if (sum[q]) atomicAdd(&mol[(blockIdx.x & (MOL_SLOTS - 1)) * MOL_STRIDE + q], (unsigned long long)sum[q]); }
}

// the vote per key, split mode: no claims, so neither the ordinals nor the filter table are written; the tallies as in first_reads_split
template <class K>
static int consensus_split(EngineImpl* im, size_t n, const PileupFold<K>& pf) {
    static_assert(sizeof(K) == 8, "the join kernel splits the pileup hits for 64-bit keys only (split_mode())");
    const KeyLayout<K> kl = key_layout<K>(im);
    const unsigned gs = (unsigned)((n + 255) / 256);
    const MoleculeWs& w = pf.w1;
    const size_t ns = std::max<size_t>((size_t)im->n_snps_sorted, 1);
    HIP_TRY(hipMemsetAsync(w.row_lo, 0, 2 * ns * sizeof(unsigned long long), im->s_comp));
    hipLaunchKernelGGL((k_consensus_base<K>), dim3(gs), dim3(256), 0, im->s_comp, pf.keys, pf.vals, (long long)n, kl, w.al, w.row_lo, w.row_hi, w.long_runs, im->d_mol);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_consensus_long<K, true>), dim3(1024), dim3(256), 0, im->s_comp, pf.keys, pf.vals, (long long)n, kl, (const unsigned long long*)w.long_runs, w.al, im->d_tally, im->d_mol);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(w.long_runs, 0, sizeof(unsigned long long), im->s_comp));   // (k_consensus_long is done with the list: now the SNPs deeper than TALLY_LONG)
    hipLaunchKernelGGL(k_tally_rows, dim3((unsigned)((ns * 8 + 255) / 256)), dim3(256), 0, im->s_comp, (const uint8_t*)w.al, (const unsigned long long*)w.row_lo, (const unsigned long long*)w.row_hi,
                       (uint32_t)ns, im->d_tally, w.long_runs);
    hipLaunchKernelGGL(k_tally_long, dim3(1024), dim3(256), 0, im->s_comp, (const uint8_t*)w.al, (const unsigned long long*)w.row_lo, (const unsigned long long*)w.row_hi,
                       (const unsigned long long*)w.long_runs, im->d_tally);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ... and with every hit in the sorted stream
template <class K>
static int consensus_plain(EngineImpl* im, size_t n, const PileupFold<K>& pf) {
    const KeyLayout<K> kl = key_layout<K>(im);
    const unsigned gs = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL((k_consensus_read<K>), dim3(gs), dim3(256), 0, im->s_comp, pf.keys, pf.vals, (long long)n, kl, pf.w1.al, im->d_tally, pf.w1.long_runs, im->d_mol);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((k_consensus_long<K, false>), dim3(1024), dim3(256), 0, im->s_comp, pf.keys, pf.vals, (long long)n, kl, (const unsigned long long*)pf.w1.long_runs, pf.w1.al, im->d_tally, im->d_mol);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the counters' own memory (engine_create, with the flag only) and their zeroing on s_comp (engine_reset)
int molecule_stats_init(EngineImpl* im) { return dev_zeroed(im, (void**)&im->d_mol, MOL_BUF_WORDS * sizeof(unsigned long long)); }
int molecule_stats_reset(EngineImpl* im) {
    im->mol_stats_valid = false;
    if (im->d_mol) HIP_TRY(hipMemsetAsync(im->d_mol, 0, MOL_BUF_WORDS * sizeof(unsigned long long), im->s_comp));
    return 0;
}

// xck_get_molecule_stats() for the pileup pipeline: the counters the last xck_finish left
int engine_molecule_stats(EngineImpl* im, xck_molecule_stats* out) {
    xck_engine* e = im->eng;
    if (!im->d_mol) { e->err = "handle made without XCK_F_UMI_CONSENSUS"; return XCK_E_STATE; }
    if (im->fold_failed || !im->finished || !im->mol_stats_valid) { e->err = "xck_get_molecule_stats: valid between a successful xck_finish and the next xck_reset"; return XCK_E_STATE; }
    HIP_TRY(hipSetDevice(im->device));
    unsigned long long all[MOL_BUF_WORDS], h[MOL_WORDS] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(all, im->d_mol, sizeof all, hipMemcpyDeviceToHost));
    for (int sl = 0; sl < MOL_SLOTS; sl++) for (int q = 0; q < MOL_WORDS; q++) h[q] += all[sl * MOL_STRIDE + q];
    out->consensus = 1;
    out->molecules = (int64_t)h[MOL_MOLECULES]; out->multi_read = (int64_t)h[MOL_MULTI_READ]; out->discordant = (int64_t)h[MOL_DISCORDANT];
    out->tied = (int64_t)h[MOL_TIED]; out->changed = (int64_t)h[MOL_CHANGED];
    return 0;
}
