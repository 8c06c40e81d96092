// base_tally.h - opt-in pseudo-bulk base tallies and candidate SNP calls (XCK_F_BASE_TALLY; xck_set_contig_lengths, xck_get_base_tally,
// xck_get_base_tally_stats, xck_find_candidates, include/xck.h).
// Included by engine.hip inside namespace xck, behind read_fate.h: it uses the join's TILE, fill_batch_table and op_* helpers, rf_filter of
// read_fate.h, and from engine_impl.h BatchTable, JOIN_BLOCK, ReadFilter, BatchDesc, as_global, EngineImpl, grow_device, dev_zeroed, HIP_TRY.
//
// One more pass over the batches the join has just been launched on - the first one here whose unit of work is the aligned base, not the
// read or the (read, SNP) pair.  Per contig that received reads the handle keeps four 32-bit counters A, C, G, T per reference position
// (position-major: the 16 bytes of a position are one uint4).  A read that passes the read filter (rf_filter: regions and SNPs are not
// asked) is walked as utils/sam.py get_query_bases walks it - M, = and X are aligned, I and S consume the query, D and N the reference,
// H and P nothing - and every aligned base, at reference position p and query offset q, falls into the FIRST of these that applies:
//   p outside [0, contig length)                          bases_out_of_range
//   no sequence byte is stored for q (seq `*`, short seq)  bases_other
//   the handle has a floor Q, quality q is not 0xff, < Q   bases_masked
//   the 4-bit code is not 1, 2, 4 or 8 (N, IUPAC, pad 0)   bases_other
//   otherwise                                              + 1 on A, C, G or T of p (bases_tallied)
// Reads are counted, not molecules: a genome-wide molecule dedup would need a sort of every aligned base, and step 1 of the BAF path applies
// the molecule-level counts and filter_snps to the candidates afterwards anyway.
//
// k_base_tally: one block per join tile (TILE reads, the numbering of fill_batch_table).  Lane mapping: the filter and the CIGAR summary
// run one LANE per read, 64 reads of a wave at a time (their SoA columns load coalesced); the reads that pass are then walked one after
// the other by the whole WAVE, a lane per query base of the aligned operation - the packed bases of a read load coalesced, the 64 lanes of
// an LDS add hit 64 different positions (no same-address serialisation, which a lane per read over a deep pileup would meet on every add),
// and no lane waits for the longest CIGAR of its wave.  The block keeps a window of BT_WINDOW positions from the tile's least pos (a block
// reduction: sortedness is a speed assumption, never a correctness one) in LDS, base-major so that the lanes of an add fall on consecutive
// banks; bases outside it - a spliced read's far exon - go straight to the table with device-scope adds without return, and so do the
// non-zero window counters at the end, 64 consecutive dwords a wave instruction (other tiles overlap the same positions).
// The five counters are kept as d_mol is: BT_SLOTS copies, one per 64-byte line, summed by the getter.
#pragma once

constexpr int BT_WINDOW = 2048;           // positions of the LDS window (x 4 counters x 4 bytes = 32 KB a block); tests read it from here
constexpr int BT_READS = 0, BT_BASES = 1, BT_OTHER = 2, BT_MASKED = 3, BT_OOR = 4, BT_WORDS = 5;
constexpr int BT_SLOTS = 256, BT_STRIDE = 8, BT_BUF_WORDS = BT_SLOTS * BT_STRIDE;
constexpr int BT_CAND_BLOCK = 256;        // positions per block of the candidate passes
static_assert(BT_STRIDE >= BT_WORDS && (BT_SLOTS & (BT_SLOTS - 1)) == 0 && JOIN_BLOCK == 256 && TILE % 64 == 0, "a copy holds the five counters; four waves a block");

struct TallyArgs {
    BatchTable bt;                        // the batches of the join launch this pass follows (same tile numbering)
    ReadFilter f;
    uint32_t* tab[MAX_FUSE];              // per batch: the table of its contig, [len * 4]
    int32_t len[MAX_FUSE];                // ... and the contig's length
    unsigned long long* stats;            // [BT_BUF_WORDS]
    int32_t min_baseq;
};
static_assert(sizeof(TallyArgs) <= 4000, "kernel arguments must stay under the 4 KiB kernarg limit");

__global__ __launch_bounds__(JOIN_BLOCK) void k_base_tally(TallyArgs a) {
    __shared__ uint32_t s_win[4 * BT_WINDOW];                         // [base][position - w0]
    __shared__ int32_t s_min[JOIN_BLOCK / 64];
    __shared__ unsigned long long s_cnt[BT_WORDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x;
    int lo = 0, hi = a.bt.n_batches - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.bt.desc[mid].tile0 <= t) lo = mid; else hi = mid - 1; }
    lo = __builtin_amdgcn_readfirstlane(lo);
    const BatchDesc& d = a.bt.desc[lo];
    uint32_t* const tab = a.tab[lo];
    const uint32_t len = (uint32_t)a.len[lo];
    const int32_t r0 = (t - d.tile0) * TILE;
    for (int k = tid; k < 4 * BT_WINDOW; k += JOIN_BLOCK) s_win[k] = 0u;
    if (tid < BT_WORDS) s_cnt[tid] = 0ull;
    // the tile's least pos (all its reads, whatever the filter says of them)
    int32_t mn = INT32_MAX;
#pragma unroll
    for (int j = 0; j < TILE / JOIN_BLOCK; j++) { const int32_t i = r0 + j * JOIN_BLOCK + tid; if (i < d.n) mn = min(mn, as_global(d.pos)[i]); }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) mn = min(mn, __shfl_xor(mn, dd, 64));
    if (lane == 0) s_min[wave] = mn;
    __syncthreads();
    const int32_t w0 = max(min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3])), 0);

    uint32_t n_reads = 0, n_base = 0, n_other = 0, n_masked = 0, n_oor = 0;
#pragma unroll 1
    for (int g = wave; g < TILE / 64; g += JOIN_BLOCK / 64) {
        const int32_t i = r0 + g * 64 + lane;
        RfSpan sp = {};
        uint32_t s0 = 0, sl = 0;
        bool ok = false;
        if (i < d.n) {
            ok = rf_filter(a.f, d, i, sp) < 0;
            if (ok) { s0 = as_global(d.seq_off)[i]; sl = as_global(d.seq_off)[i + 1] - s0; }
        }
        unsigned long long m = __ballot(ok);
        if (lane == 0) n_reads += (uint32_t)__popcll(m);
#pragma unroll 1
        while (m) {                                                   // wave-uniform: the reads that passed, one after the other
            const int src = __ffsll((long long)m) - 1;
            m &= m - 1;
            uint32_t rp = (uint32_t)__shfl(sp.pos, src, 64), q = 0;   // (unsigned: an absurd CIGAR wraps instead of overflowing; every use is bounds-checked)
            const uint32_t c0 = __shfl(sp.c0, src, 64), c1 = __shfl(sp.c1, src, 64);
            const uint32_t rs0 = __shfl(s0, src, 64), rsl = __shfl(sl, src, 64);
#pragma unroll 1
            for (uint32_t c = c0; c < c1; c++) {
                const uint32_t w = as_global(d.cigar)[c]; const uint32_t op = w & 15u, l = w >> 4;
                if (op_aligned(op)) {
#pragma unroll 1
                    for (uint32_t off = lane; off < l; off += 64) {
                        const uint32_t p = rp + off, qi = q + off;
                        if (p >= len) { n_oor++; continue; }          // (a negative position is a large unsigned one)
                        if ((qi >> 1) >= rsl) { n_other++; continue; }
                        const uint32_t by = as_global(d.seq)[rs0 + (qi >> 1)];
                        if (a.min_baseq > 0) {                        // (the quality byte of query offset qi: 2 * s0 + qi, as base_at_q of the join)
                            const int32_t qv = as_global(d.qual)[2u * rs0 + qi];
                            if (qv != 0xff && qv < a.min_baseq) { n_masked++; continue; }
                        }
                        const uint32_t nib = (qi & 1u) ? (by & 15u) : (by >> 4);
                        const int b = nib == 1u ? 0 : nib == 2u ? 1 : nib == 4u ? 2 : nib == 8u ? 3 : -1;
                        if (b < 0) { n_other++; continue; }
                        n_base++;
                        const uint32_t rel = p - (uint32_t)w0;
                        if (rel < (uint32_t)BT_WINDOW) atomicAdd(&s_win[b * BT_WINDOW + (int)rel], 1u);
                        else atomicAdd(&tab[(size_t)p * 4 + b], 1u);  // p < len: inside the table
                    }
                    rp += l; q += l;
                } else if (op_ref(op)) rp += l;
                else if (op == 1u || op == 4u) q += l;
            }
        }
    }
    uint32_t cnt[BT_WORDS] = { n_reads, n_base, n_other, n_masked, n_oor };
#pragma unroll
    for (int k = 0; k < BT_WORDS; k++) {
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) cnt[k] += __shfl_xor(cnt[k], dd, 64);
        if (lane == 0 && cnt[k]) atomicAdd(&s_cnt[k], (unsigned long long)cnt[k]);
    }
    __syncthreads();
    // the window's non-zero counters, in the table's order: a wave instruction covers 64 consecutive dwords (w0 + rel < len: only such bases were added)
    for (int k = tid; k < 4 * BT_WINDOW; k += JOIN_BLOCK) {
        const uint32_t v = s_win[(k & 3) * BT_WINDOW + (k >> 2)];
        if (v) atomicAdd(&tab[(size_t)w0 * 4 + (size_t)k], v);
    }
    if (tid < BT_WORDS) { const unsigned long long v = s_cnt[tid]; if (v) atomicAdd(&a.stats[(blockIdx.x & (BT_SLOTS - 1)) * BT_STRIDE + tid], v); }
}

// ---- candidates: ref / alt of one position and the verdict, stated once (tests/base_tally_cases.py states it again in Python) ----
// c: A C G T.  ref: the largest count, the earliest of equals; alt: the largest of the other three, same tie rule, m its count.  The
// arithmetic is snp_passes() of finish.hip with the alt count as the minor count.
__host__ __device__ inline bool bt_candidate(const uint32_t c[4], double min_count, double min_maf, int& ref, int& alt, bool& covered) {
    const unsigned long long n = (unsigned long long)c[0] + c[1] + c[2] + c[3];
    covered = n > 0;
    ref = 0;
    for (int b = 1; b < 4; b++) if (c[b] > c[ref]) ref = b;
    alt = ref == 0 ? 1 : 0;
    for (int b = alt + 1; b < 4; b++) if (b != ref && c[b] > c[alt]) alt = b;
    const uint32_t m = c[alt];
    return m > 0 && !((double)n < min_count) && !((double)m < (double)n * min_maf);
}

// ... and oriented by the genome's 4-bit code g of the position (xck_find_candidates_ref, include/xck.h; tests/refseq_cases.py states it
// again): ref = g, alt the largest of the other three, m the smaller of the two counts, the same arithmetic.  Returns the position's class;
// BT_REF_MAJOR and BT_REF_MINOR are written (ref is, or is not, the base bt_candidate makes ref), the other two count what bt_candidate
// accepts and this rule does not: a genome base the reads do not support, a genome code that is not one of A C G T.
constexpr int BT_REF_NONE = 0, BT_REF_MAJOR = 1, BT_REF_MINOR = 2, BT_REF_UNSUPPORTED = 3, BT_REF_UNKNOWN = 4;
__host__ __device__ inline int bt_candidate_ref(const uint32_t c[4], uint32_t g, double min_count, double min_maf, int& ref, int& alt, bool& covered) {
    int pref, palt;
    const bool parent = bt_candidate(c, min_count, min_maf, pref, palt, covered);
    const int gi = g == 1u ? 0 : g == 2u ? 1 : g == 4u ? 2 : g == 8u ? 3 : -1;
    ref = pref; alt = palt;
    if (gi < 0) return parent ? BT_REF_UNKNOWN : BT_REF_NONE;
    ref = gi;
    alt = ref == 0 ? 1 : 0;
    for (int b = alt + 1; b < 4; b++) if (b != ref && c[b] > c[alt]) alt = b;
    const unsigned long long n = (unsigned long long)c[0] + c[1] + c[2] + c[3];
    const uint32_t m = c[ref] < c[alt] ? c[ref] : c[alt];
    if (m > 0 && !((double)n < min_count) && !((double)m < (double)n * min_maf)) return ref == pref ? BT_REF_MAJOR : BT_REF_MINOR;
    return parent ? BT_REF_UNSUPPORTED : BT_REF_NONE;
}

// count pass (EMIT = false): candidates and covered positions per block of BT_CAND_BLOCK positions.  Emit pass: the same verdicts again,
// every candidate written at the block's scanned offset + its rank inside the block, i.e. in position order.
// REF: the verdict is bt_candidate_ref's under the position's nibble of the contig's packed sequence (ref_seq.h; half a byte more a
// position, two lanes a byte; null: no sequence, every position N), and the count pass leaves the block's four class counts in blk_st.
// Without REF the two trailing arguments are not read.
template <bool EMIT, bool REF = false>
__global__ __launch_bounds__(BT_CAND_BLOCK) void k_bt_candidates(const uint32_t* __restrict__ tab, uint32_t len, double min_count, double min_maf,
                                                                 uint32_t* __restrict__ blk_cand, uint32_t* __restrict__ blk_cov,
                                                                 int32_t* __restrict__ o_pos, uint32_t* __restrict__ o_cnt, char* __restrict__ o_ref, char* __restrict__ o_alt,
                                                                 const uint8_t* __restrict__ seq, uint32_t* __restrict__ blk_st) {
    __shared__ uint32_t s_c[BT_CAND_BLOCK / 64], s_v[BT_CAND_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t p = blockIdx.x * (uint32_t)BT_CAND_BLOCK + tid;
    uint32_t c[4] = { 0, 0, 0, 0 };
    if (p < len) { const uint4 v = *reinterpret_cast<const uint4*>(tab + (size_t)p * 4); c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w; }
    int ref = 0, alt = 1; bool cov = false;
    bool cand;
    if (REF) {
        __shared__ uint32_t s_k[BT_CAND_BLOCK / 64][4];
        uint32_t g = 15u;
        if (seq && p < len) { const uint32_t by = seq[p >> 1]; g = (p & 1u) ? (by & 15u) : (by >> 4); }   // (p < len: inside the (len + 7) / 8 dwords)
        const int cls = bt_candidate_ref(c, g, min_count, min_maf, ref, alt, cov);
        cand = cls == BT_REF_MAJOR || cls == BT_REF_MINOR;
        if (!EMIT) {
#pragma unroll
            for (int k = 0; k < 4; k++) { const unsigned long long mk = __ballot(cls == k + 1); if (lane == 0) s_k[wave][k] = (uint32_t)__popcll(mk); }
            __syncthreads();
            if (tid < 4) { uint32_t a = 0; for (int w = 0; w < BT_CAND_BLOCK / 64; w++) a += s_k[w][tid]; blk_st[(size_t)blockIdx.x * 4 + tid] = a; }
        }
    } else cand = bt_candidate(c, min_count, min_maf, ref, alt, cov);
    const unsigned long long mc = __ballot(cand), mv = __ballot(cov);
    if (lane == 0) { s_c[wave] = (uint32_t)__popcll(mc); s_v[wave] = (uint32_t)__popcll(mv); }
    __syncthreads();
    if (!EMIT) {
        if (tid == 0) { uint32_t a = 0, b = 0; for (int w = 0; w < BT_CAND_BLOCK / 64; w++) { a += s_c[w]; b += s_v[w]; } blk_cand[blockIdx.x] = a; blk_cov[blockIdx.x] = b; }
    } else if (cand) {
        uint32_t at = blk_cand[blockIdx.x];                           // (scanned: the block's first candidate)
        for (int w = 0; w < wave; w++) at += s_c[w];
        at += (uint32_t)__popcll(mc & ((1ull << lane) - 1ull));
        o_pos[at] = (int32_t)p + 1;
        *reinterpret_cast<uint4*>(o_cnt + (size_t)at * 4) = make_uint4(c[0], c[1], c[2], c[3]);
        o_ref[at] = "ACGT"[ref]; o_alt[at] = "ACGT"[alt];
    }
}

// one block: the four class counts of blk_st[0, nb) summed into tot[0 .. 4) (xck_find_candidates_ref, behind the count pass)
__global__ __launch_bounds__(1024) void k_bt_ref_sum(const uint32_t* __restrict__ blk_st, long long nb, unsigned long long* __restrict__ tot) {
    __shared__ unsigned long long s_w[16][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned long long a[4] = { 0, 0, 0, 0 };
    for (long long i = tid; i < nb; i += 1024) { const uint4 v = *reinterpret_cast<const uint4*>(blk_st + i * 4); a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w; }
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int dd = 32; dd >= 1; dd >>= 1) a[k] += __shfl_xor(a[k], dd, 64);
        if (lane == 0) s_w[wave][k] = a[k];
    }
    __syncthreads();
    if (tid < 4) { unsigned long long t = 0; for (int w = 0; w < 16; w++) t += s_w[w][tid]; tot[tid] = t; }
}

// one block: blk[0, nb) -> its exclusive prefix sums in place; tot[0] = their total, tot[1] = the sum of cov[0, nb)
__global__ __launch_bounds__(1024) void k_bt_scan(uint32_t* __restrict__ blk, const uint32_t* __restrict__ cov, long long nb, unsigned long long* __restrict__ tot) {
    __shared__ uint32_t s_w[16];
    __shared__ unsigned long long s_cov;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_cov = 0ull;
    unsigned long long carry = 0, my_cov = 0;
    for (long long base = 0; base < nb; base += 1024) {
        const long long i = base + tid;
        const uint32_t v = i < nb ? blk[i] : 0u;
        if (i < nb) my_cov += cov[i];
        uint32_t inc = v;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) { const uint32_t y = __shfl_up(inc, dd, 64); if (lane >= dd) inc += y; }
        __syncthreads();                                              // (the previous round's s_w has been read)
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < 16; w++) { const uint32_t x = s_w[w]; if (w < wave) before += x; all += x; }
        if (i < nb) blk[i] = (uint32_t)(carry + before + inc - v);
        carry += all;
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) my_cov += __shfl_xor(my_cov, dd, 64);
    __syncthreads();
    if (lane == 0 && my_cov) atomicAdd(&s_cov, my_cov);
    __syncthreads();
    if (tid == 0) { tot[0] = carry; tot[1] = s_cov; }
}

// ---- host side ----
// the counters' memory and the (still empty) table of tables (summaries_init, only with the flag)
static int base_tally_init(EngineImpl* im) {
    im->base_tally = true;
    im->bt_tab.assign(std::max(im->eng->n_contigs, 1), nullptr);
    im->rs_tab.assign(std::max(im->eng->n_contigs, 1), nullptr);
    return dev_zeroed(im, (void**)&im->d_bt_stats, BT_BUF_WORDS * sizeof(unsigned long long));
}
// xck_reset: the tables that exist and the counters zeroed on s_comp (the caller synchronises); the lengths and the packed sequences stay
static int base_tally_reset(EngineImpl* im) {
    for (size_t c = 0; c < im->bt_tab.size(); c++)
        if (im->bt_tab[c]) HIP_TRY(hipMemsetAsync(im->bt_tab[c], 0, (size_t)im->bt_len[c] * 16, im->s_comp));
    HIP_TRY(hipMemsetAsync(im->d_bt_stats, 0, BT_BUF_WORDS * sizeof(unsigned long long), im->s_comp));
    return 0;
}
void base_tally_free(EngineImpl* im) {
    for (uint32_t* p : im->bt_tab) if (p) hipFree(p);
    ref_seq_free(im);
    for (void* p : { (void*)im->d_bt_stats, (void*)im->d_bt_blk, (void*)im->d_bt_out, (void*)im->d_bt_tot }) if (p) hipFree(p);
}

int base_tally_set_lengths(EngineImpl* im, const int64_t* len, int32_t n) {
    if (!im->base_tally) { im->eng->err = "handle made without XCK_F_BASE_TALLY"; return XCK_E_STATE; }
    if (im->st.n_batches > 0) { im->eng->err = "xck_set_contig_lengths: after the first push (call it right after xck_create or xck_reset)"; return XCK_E_STATE; }
    if (!len || n != im->eng->n_contigs) { im->eng->err = "xck_set_contig_lengths: one length per contig of the handle"; return XCK_E_ARG; }
    for (int32_t c = 0; c < n; c++) if (len[c] < 1 || len[c] > (int64_t)INT32_MAX) { im->eng->err = "xck_set_contig_lengths: a length outside 1 .. 2^31 - 1"; return XCK_E_ARG; }
    for (int32_t c = 0; c < n; c++)
        if (im->bt_tab[c] && (im->bt_len.size() != (size_t)n || im->bt_len[c] != len[c])) {   // (after a reset: a table that exists keeps its size)
            HIP_TRY(hipSetDevice(im->device));
            HIP_TRY(hipFree(im->bt_tab[c])); im->bt_tab[c] = nullptr;
        }
    for (int32_t c = 0; c < n; c++)
        if (im->rs_tab[c] && im->bt_len[c] != len[c]) {                  // (a packed sequence is as long as its contig: ref_seq.h)
            HIP_TRY(hipSetDevice(im->device));
            HIP_TRY(hipFree(im->rs_tab[c])); im->rs_tab[c] = nullptr;
        }
    im->bt_len.assign(len, len + n);
    return 0;
}

// describe_batch, a batch of contig c is about to be queued: the contig's table exists from here on, zeroed on s_comp in front of the
// pass that first adds to it
int base_tally_touch(EngineImpl* im, int32_t c) {
    if (im->bt_len.empty()) { im->eng->err = "XCK_F_BASE_TALLY: no contig lengths (call xck_set_contig_lengths before the first push)"; return XCK_E_STATE; }
    if (im->bt_tab[c]) return 0;
    const size_t bytes = (size_t)im->bt_len[c] * 16;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        char b[200]; snprintf(b, sizeof b, "out of device memory for the base tally table of contig %d (%lld positions, %.2f GB)", (int)c, (long long)im->bt_len[c], bytes * 1e-9);
        im->eng->err = b; return e == hipErrorOutOfMemory ? XCK_E_NOMEM : XCK_E_DEVICE;
    }
    im->bt_tab[c] = (uint32_t*)p;
    HIP_TRY(hipMemsetAsync(p, 0, bytes, im->s_comp));
    return 0;
}

// Runs once per batch: called by launch_queue() (launch_summaries) behind the FIRST join launch of the batches in im->inflight, on the
// same stream, and never by the overflow replay - as launch_read_fate.
static int launch_base_tally(EngineImpl* im) {
    if (!im->base_tally || im->inflight.empty()) return 0;
    TallyArgs a;
    const int32_t tiles = fill_batch_table(im, a.bt);
    a.f = im->rf; a.stats = im->d_bt_stats; a.min_baseq = im->min_baseq;
    for (int b = 0; b < MAX_FUSE; b++) { a.tab[b] = nullptr; a.len[b] = 0; }
    for (int b = 0; b < a.bt.n_batches; b++) {
        const int32_t c = a.bt.desc[b].contig;
        if (c < 0 || (size_t)c >= im->bt_tab.size() || !im->bt_tab[c]) { im->eng->err = "internal: a queued batch without a base tally table"; return XCK_E_STATE; }
        a.tab[b] = im->bt_tab[c]; a.len[b] = (int32_t)im->bt_len[c];
    }
    hipLaunchKernelGGL(k_base_tally, dim3(tiles), dim3(JOIN_BLOCK), 0, im->s_comp, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// xck_get_base_tally for the pileup pipeline: waits for the queued work, copies the counters of [pos0, pos0 + n)
int engine_base_tally(EngineImpl* im, int32_t contig, int32_t pos0, int32_t n, uint32_t* out) {
    if (!im->base_tally) { im->eng->err = "handle made without XCK_F_BASE_TALLY"; return XCK_E_STATE; }
    if (im->bt_len.empty()) { im->eng->err = "xck_get_base_tally: no contig lengths (xck_set_contig_lengths)"; return XCK_E_STATE; }
    if (contig < 0 || contig >= (int32_t)im->bt_len.size() || pos0 < 0 || n < 0 || (int64_t)pos0 + n > im->bt_len[contig] || (n > 0 && !out)) {
        im->eng->err = "xck_get_base_tally: contig or position range outside the handle's contigs"; return XCK_E_ARG; }
    if (const int rc = engine_flush(im)) return rc;
    if (n == 0) return 0;
    if (!im->bt_tab[contig]) { memset(out, 0, (size_t)n * 16); return 0; }
    HIP_TRY(hipMemcpy(out, im->bt_tab[contig] + (size_t)pos0 * 4, (size_t)n * 16, hipMemcpyDeviceToHost));
    return 0;
}

int engine_base_tally_stats(EngineImpl* im, xck_base_tally_stats* out) {
    if (!im->base_tally) { im->eng->err = "handle made without XCK_F_BASE_TALLY"; return XCK_E_STATE; }
    if (const int rc = engine_flush(im)) return rc;
    std::vector<unsigned long long> all(BT_BUF_WORDS);
    HIP_TRY(hipMemcpy(all.data(), im->d_bt_stats, BT_BUF_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long h[BT_WORDS] = { 0, 0, 0, 0, 0 };
    for (int sl = 0; sl < BT_SLOTS; sl++) for (int q = 0; q < BT_WORDS; q++) h[q] += all[sl * BT_STRIDE + q];
    out->reads_tallied = (int64_t)h[BT_READS]; out->bases_tallied = (int64_t)h[BT_BASES]; out->bases_other = (int64_t)h[BT_OTHER];
    out->bases_masked = (int64_t)h[BT_MASKED]; out->bases_out_of_range = (int64_t)h[BT_OOR];
    return 0;
}

// xck_find_candidates for the pileup pipeline: per allocated table, in contig order, a count pass, a scan and an emit pass; the contig's
// candidates are copied behind those of the contigs before it, so the arrays are in (contig, pos) order.
// st (xck_find_candidates_ref): the REF instantiation under the contig's packed sequence (ref_seq.h), its class counts summed per contig
static int find_candidates(EngineImpl* im, const xck_candidate_config* cfg, xck_candidates* out, xck_candidate_ref_stats* st) {
    if (!im->base_tally) { im->eng->err = "handle made without XCK_F_BASE_TALLY"; return XCK_E_STATE; }
    if (!im->finished || im->fold_failed) {
        im->eng->err = std::string(st ? "xck_find_candidates_ref" : "xck_find_candidates") + ": valid between a successful xck_finish and the next xck_reset"; return XCK_E_STATE; }
    HIP_TRY(hipSetDevice(im->device));
    const auto t0 = std::chrono::steady_clock::now();
    im->h_bt_contig.clear(); im->h_bt_pos.clear(); im->h_bt_ref.clear(); im->h_bt_alt.clear(); im->h_bt_cnt.clear();
    long long covered = 0;
    if (!im->d_bt_tot) HIP_TRY(hipMalloc((void**)&im->d_bt_tot, 6 * sizeof(unsigned long long)));   // the scan's two totals, the four class counts
    long long cls[4] = { 0, 0, 0, 0 };
    for (size_t c = 0; c < im->bt_tab.size(); c++) {
        const uint32_t* tab = im->bt_tab[c];
        if (!tab) continue;
        const uint32_t len = (uint32_t)im->bt_len[c];
        const size_t nb = ((size_t)len + BT_CAND_BLOCK - 1) / BT_CAND_BLOCK;
        if (const int rc = grow_device(im, (void**)&im->d_bt_blk, &im->bt_blk_cap, (st ? 6 : 2) * nb * sizeof(uint32_t), 0)) return rc;
        uint32_t* blk_st = (uint32_t*)im->d_bt_blk;                     // (in front: its rows are read as uint4)
        uint32_t* blk_cand = blk_st + (st ? 4 * nb : 0); uint32_t* blk_cov = blk_cand + nb;
        const uint8_t* seq = st ? (const uint8_t*)im->rs_tab[c] : nullptr;
        if (st) hipLaunchKernelGGL((k_bt_candidates<false, true>), dim3((unsigned)nb), dim3(BT_CAND_BLOCK), 0, im->s_comp, tab, len, cfg->min_count, cfg->min_maf, blk_cand, blk_cov,
                                   (int32_t*)nullptr, (uint32_t*)nullptr, (char*)nullptr, (char*)nullptr, seq, blk_st);
        else hipLaunchKernelGGL((k_bt_candidates<false>), dim3((unsigned)nb), dim3(BT_CAND_BLOCK), 0, im->s_comp, tab, len, cfg->min_count, cfg->min_maf, blk_cand, blk_cov,
                                (int32_t*)nullptr, (uint32_t*)nullptr, (char*)nullptr, (char*)nullptr, (const uint8_t*)nullptr, (uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_bt_scan, dim3(1), dim3(1024), 0, im->s_comp, blk_cand, (const uint32_t*)blk_cov, (long long)nb, im->d_bt_tot);
        HIP_TRY(hipGetLastError());
        if (st) { hipLaunchKernelGGL(k_bt_ref_sum, dim3(1), dim3(1024), 0, im->s_comp, (const uint32_t*)blk_st, (long long)nb, im->d_bt_tot + 2); HIP_TRY(hipGetLastError()); }
        unsigned long long tot[6] = { 0, 0, 0, 0, 0, 0 };
        HIP_TRY(hipMemcpyAsync(tot, im->d_bt_tot, (st ? 6 : 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, im->s_comp));
        HIP_TRY(hipStreamSynchronize(im->s_comp));
        covered += (long long)tot[1];
        for (int k = 0; k < 4; k++) cls[k] += (long long)tot[2 + k];
        const size_t n = (size_t)tot[0];
        if (!n) continue;
        // the contig's output: [counts n * 16 | pos n * 4 | ref n | alt n]
        if (const int rc = grow_device(im, (void**)&im->d_bt_out, &im->bt_out_cap, n * 22, n * 22 / 4 + 4096)) return rc;
        uint32_t* o_cnt = (uint32_t*)im->d_bt_out; int32_t* o_pos = (int32_t*)(im->d_bt_out + n * 16); char* o_ref = im->d_bt_out + n * 20; char* o_alt = o_ref + n;
        if (st) hipLaunchKernelGGL((k_bt_candidates<true, true>), dim3((unsigned)nb), dim3(BT_CAND_BLOCK), 0, im->s_comp, tab, len, cfg->min_count, cfg->min_maf, blk_cand, blk_cov, o_pos, o_cnt, o_ref, o_alt, seq, blk_st);
        else hipLaunchKernelGGL((k_bt_candidates<true>), dim3((unsigned)nb), dim3(BT_CAND_BLOCK), 0, im->s_comp, tab, len, cfg->min_count, cfg->min_maf, blk_cand, blk_cov, o_pos, o_cnt, o_ref, o_alt,
                                (const uint8_t*)nullptr, (uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
        const size_t at = im->h_bt_pos.size();
        im->h_bt_contig.resize(at + n, (int32_t)c); im->h_bt_pos.resize(at + n); im->h_bt_ref.resize(at + n); im->h_bt_alt.resize(at + n); im->h_bt_cnt.resize((at + n) * 4);
        HIP_TRY(hipMemcpyAsync(im->h_bt_cnt.data() + at * 4, o_cnt, n * 16, hipMemcpyDeviceToHost, im->s_comp));
        HIP_TRY(hipMemcpyAsync(im->h_bt_pos.data() + at, o_pos, n * 4, hipMemcpyDeviceToHost, im->s_comp));
        HIP_TRY(hipMemcpyAsync(im->h_bt_ref.data() + at, o_ref, n, hipMemcpyDeviceToHost, im->s_comp));
        HIP_TRY(hipMemcpyAsync(im->h_bt_alt.data() + at, o_alt, n, hipMemcpyDeviceToHost, im->s_comp));
        HIP_TRY(hipStreamSynchronize(im->s_comp));
    }
    out->n = (int64_t)im->h_bt_pos.size();
    out->contig = im->h_bt_contig.data(); out->pos = im->h_bt_pos.data(); out->ref = im->h_bt_ref.data(); out->alt = im->h_bt_alt.data(); out->count = im->h_bt_cnt.data();
    out->positions_covered = covered;
    if (st) { st->ref_major = cls[0]; st->ref_minor = cls[1]; st->ref_unsupported = cls[2]; st->ref_unknown = cls[3]; }
    if (im->eng->knobs.debug_timing)
        fprintf(stderr, "[xck] find_candidates%s: %.3f ms (host clock), %lld candidates of %lld covered positions\n", st ? "_ref" : "",
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), (long long)out->n, covered);
    return 0;
}
int engine_find_candidates(EngineImpl* im, const xck_candidate_config* cfg, xck_candidates* out) { return find_candidates(im, cfg, out, nullptr); }
int engine_find_candidates_ref(EngineImpl* im, const xck_candidate_config* cfg, xck_candidates* out, xck_candidate_ref_stats* st) { return find_candidates(im, cfg, out, st); }
