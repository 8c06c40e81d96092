// cell_summary.h - opt-in per-cell table (XCK_F_CELL_SUMMARY / XCK_CELL_SUMMARY=1; xck_get_cell_summary, include/xck.h).
// Included by engine.hip inside namespace xck, in front of read_fate.h: the grouped accumulation below is what the per-cell
// instantiation of the read-fate pass (k_read_fate_cell, read_fate.h) and the column marginals of the result blocks
// (k_cell_marginals, here) share; launch_marginals() is the one host loop over the result blocks, for the column marginals here and
// the row marginals of feature_summary.h.  Uses JOIN_BLOCK, as_global, EngineImpl and HIP_TRY from engine_impl.h.
//
// The table in HBM: one row per cell plus one for the reads without a listed cell, CS_ROW_WORDS = 16 64-bit words = 128 B a row
// (the 12 columns of xck_read_fate from low_mapq on, 4 words of padding), so that a row is one aligned line and its columns are
// contiguous bytes for the atomics that reach it.
//
// Two regimes, one kernel.  A 10x file in coordinate order gives a block of 1024 reads about 1024 different rows:
// there is nothing to combine, and what matters is that the pass adds little to the classification.  A well / bulk file gives
// every read of a launch the same row: one atomic per read would send all of them to twelve addresses.  So every contribution
// is combined on chip first, in three steps:
//   1. wave: the lanes that share (row, column) are found with ballots (a leader loop over the distinct pairs: one round per
//      pair, register work only) and add ONCE - the group's popcount, and the sum of its pair counts;
//   2. block: the leaders add into an LDS table keyed by row (open addressing, CS_PROBES probes, CS_SLOTS rows fixed at compile
//      time; XCK_CELL_SUMMARY_SLOTS lowers the capacity for tests).  A leader that finds no slot sends its sums straight to HBM:
//      a tile of 1024 reads can touch 1024 rows, and rows that do not fit have nothing to combine with anyway;
//   3. HBM: the occupied slots are flushed 16 lanes a row, four rows a wave instruction - one 64-bit atomic per non-zero
//      (row, column) of the block, neighbouring lanes on neighbouring words of one 128-B line.
// With one cell a block of 1024 reads ends in at most 12 global atomics.
#pragma once

constexpr int CS_ROW_WORDS = 16;          // 64-bit words of a table row in HBM
constexpr int CS_COLS = 12;               // ... of which xck_cell_summary.fate hands out the first 12
constexpr int CS_MATRIX_COLS = 4;         // columns of the matrix half (BAF; basefc uses 2)
constexpr int CS_SLOTS = 512;             // rows of the LDS table: 512 * 56 B + list = 29.7 KB, five blocks a CU
constexpr int CS_PROBES = 8;
constexpr int CS_C32 = 11;                // 32-bit counters of an LDS row (a block adds at most its read count to each); word 11 is the row's key
constexpr uint32_t CS_EMPTY = 0xFFFFFFFFu;
constexpr int MG_ITEMS = 8;               // k_cell_marginals: entries per thread

// where the sums of a block go
struct CellArgs {
    unsigned long long* tab;              // [rows * stride]
    int32_t  n_rows;                      // rows of the table (the callers hand in row < n_rows)
    uint32_t slot_mask;                   // LDS rows in use - 1 (a power of two <= CS_SLOTS)
    int32_t  stride;                      // words of a table row
    int32_t  c32_base;                    // table column of the 32-bit counter 0 (< 0: the 32-bit counters are dropped)
    int32_t  wide_col;                    // table column of the 64-bit sum
};

// The LDS table of a block: SLOTS rows of C32 32-bit counters and the row's key, a 64-bit sum per row when WIDE.  The per-cell
// table is CellLds; the per-feature and per-SNP tables (feature_summary.h) carry three counters and one, no sum, and so twice the rows.
template <int C32, int SLOTS, bool WIDE>
struct SumLds {
    uint32_t cnt[SLOTS * (C32 + 1)];            // per row: C32 counters, then the key
    unsigned long long wide[WIDE ? SLOTS : 1];  // per row: the 64-bit sum
    uint16_t list[SLOTS];                       // the occupied rows, in the order they were claimed
    uint32_t n_list;
};
typedef SumLds<CS_C32, CS_SLOTS, true> CellLds;

// the block's table (ON = false: no LDS at all)
template <bool ON> __device__ __forceinline__ CellLds* cs_lds() {
    if constexpr (ON) { __shared__ CellLds s; return &s; } else return nullptr;
}

template <int C32, int SLOTS, bool WIDE>
__device__ __forceinline__ void cs_init(SumLds<C32, SLOTS, WIDE>& s, const CellArgs& ca, const int tid) {
    const uint32_t slots = ca.slot_mask + 1u;
    for (uint32_t k = tid; k < slots * (C32 + 1); k += JOIN_BLOCK) s.cnt[k] = (k % (C32 + 1)) == C32 ? CS_EMPTY : 0u;
    if constexpr (WIDE) for (uint32_t k = tid; k < slots; k += JOIN_BLOCK) s.wide[k] = 0ull;
    if (tid == 0) s.n_list = 0u;
}

// One contribution per valid lane: +1 in the 32-bit column c32 of `row`, +wv in its 64-bit sum, +1 in column xcol when `extra`.
// Every lane of the wave calls it (wave-uniform control flow).
template <int C32, int SLOTS, bool WIDE>
__device__ __forceinline__ void cs_add(SumLds<C32, SLOTS, WIDE>& s, const CellArgs& ca, const int lane, const bool valid, const int32_t row, const int c32,
                                       const uint32_t wv, const bool extra, const int xcol) {
    // step 1: one round per distinct (row, c32) of the wave; the lowest lane of a group keeps the group's sums
    unsigned long long todo = __ballot(valid);
    uint32_t g_n = 0, g_x = 0; unsigned long long g_w = 0;
    while (todo) {
        const int ld = __ffsll(todo) - 1;
        const int32_t r = __builtin_amdgcn_readlane(row, ld); const int c = __builtin_amdgcn_readlane(c32, ld);
        const bool in = valid && row == r && c32 == c;
        const unsigned long long same = __ballot(in);
        unsigned long long w = 0;
        if (WIDE && __ballot(in && wv != 0u)) {
            if (!(same & (same - 1))) w = (uint32_t)__builtin_amdgcn_readlane((int)wv, ld);      // a group of one
            else {
                w = in ? wv : 0u;
#pragma unroll
                for (int dd = 32; dd >= 1; dd >>= 1) w += __shfl_xor(w, dd, 64);
            }
        }
        const uint32_t x = (uint32_t)__popcll(__ballot(in && extra));
        if (lane == ld) { g_n = (uint32_t)__popcll(same); g_x = x; g_w = w; }
        todo &= ~same;
    }
    if (!g_n) return;
    // step 2: the row's slot of the LDS table
    uint32_t h = (((uint32_t)row * 0x9E3779B1u) >> 16) & ca.slot_mask;
    int slot = -1;
    for (int q = 0; q < CS_PROBES; q++) {
        const uint32_t old = atomicCAS(&s.cnt[h * (C32 + 1) + C32], CS_EMPTY, (uint32_t)row);
        if (old == CS_EMPTY) { s.list[atomicAdd(&s.n_list, 1u)] = (uint16_t)h; slot = (int)h; break; }
        if (old == (uint32_t)row) { slot = (int)h; break; }
        h = (h + 1u) & ca.slot_mask;
    }
    if (slot >= 0) {
        atomicAdd(&s.cnt[slot * (C32 + 1) + c32], g_n);
        if (g_x) atomicAdd(&s.cnt[slot * (C32 + 1) + xcol], g_x);
        if (WIDE && g_w) atomicAdd(&s.wide[slot], g_w);
    } else {                                                   // no slot within CS_PROBES: straight to HBM
        unsigned long long* t = ca.tab + (size_t)row * ca.stride;
        if (ca.c32_base >= 0) { atomicAdd(&t[ca.c32_base + c32], (unsigned long long)g_n); if (g_x) atomicAdd(&t[ca.c32_base + xcol], (unsigned long long)g_x); }
        if (g_w) atomicAdd(&t[ca.wide_col], g_w);
    }
}

// step 3, behind a __syncthreads(): LPR lanes per occupied row (16 for the twelve columns of the per-cell table)
template <int C32, int SLOTS, bool WIDE>
__device__ __forceinline__ void cs_flush(SumLds<C32, SLOTS, WIDE>& s, const CellArgs& ca, const int tid) {
    constexpr int COLS = C32 + (WIDE ? 1 : 0), LPR = COLS <= 1 ? 1 : COLS <= 4 ? 4 : 16;
    static_assert(COLS <= 16, "a row is flushed by at most 16 lanes");
    const uint32_t n = s.n_list;
    const int j = tid & (LPR - 1);
    for (uint32_t k = tid / LPR; k < n; k += JOIN_BLOCK / LPR) {
        const uint32_t slot = s.list[k];
        const uint32_t row = s.cnt[slot * (C32 + 1) + C32];
        unsigned long long v = 0; int col = -1;
        if (j < C32) { v = s.cnt[slot * (C32 + 1) + j]; col = ca.c32_base >= 0 ? ca.c32_base + j : -1; }
        else if (WIDE && j == C32) { v = s.wide[slot]; col = ca.wide_col; }
        if (v && col >= 0) atomicAdd(&ca.tab[(size_t)row * ca.stride + col], v);
    }
}

// ---- matrix half: column marginals of one result block [row | col | val] ----
struct MargArgs { const int32_t* col; const int32_t* val; long long n; CellArgs ca; };

// Per column of the matrix the sum of val (64-bit) and the number of entries.  The entries are sorted by (row, col): a wave sees
// 64 neighbouring columns of one row, or - few cells - the same few columns again and again; same shape as the per-read half.
__global__ __launch_bounds__(JOIN_BLOCK) void k_cell_marginals(MargArgs a) {
    __shared__ CellLds s;
    const int tid = threadIdx.x, lane = tid & 63;
    cs_init(s, a.ca, tid);
    __syncthreads();
    const long long base = (long long)blockIdx.x * (JOIN_BLOCK * MG_ITEMS);
#pragma unroll 1
    for (int j = 0; j < MG_ITEMS; j++) {
        const long long i = base + (long long)j * JOIN_BLOCK + tid;
        int32_t c = 0, v = 0;
        if (i < a.n) { c = as_global(a.col)[i]; v = as_global(a.val)[i]; }
        const bool valid = i < a.n && (uint32_t)c < (uint32_t)a.ca.n_rows;
        cs_add(s, a.ca, lane, valid, c, 0, (uint32_t)v, false, 0);
    }
    __syncthreads();
    cs_flush(s, a.ca, tid);
}

static uint32_t cs_slot_mask(const EngineImpl* im, const int slots = CS_SLOTS) {
    long long want = im->eng->knobs.cell_summary_slots;
    if (want <= 0 || want > slots) want = slots;
    uint32_t p = 1; while ((long long)p * 2 <= want) p *= 2;
    return p - 1u;
}

// the table's own memory (summaries_init; off: nothing), and its zeroing on s_comp (summaries_reset; off: only the flag)
static int cell_summary_init(EngineImpl* im) {
    if (const int rc = dev_zeroed(im, (void**)&im->d_cell, ((size_t)im->n_cells + 1) * CS_ROW_WORDS * sizeof(unsigned long long))) return rc;
    HIP_TRY(hipMalloc((void**)&im->d_cmat, (size_t)im->n_cells * CS_MATRIX_COLS * sizeof(unsigned long long)));
    return 0;
}
static int cell_summary_reset(EngineImpl* im) {
    if (im->d_cell) HIP_TRY(hipMemsetAsync(im->d_cell, 0, ((size_t)im->n_cells + 1) * CS_ROW_WORDS * sizeof(unsigned long long), im->s_comp));
    im->cmat_valid = false;
    return 0;
}

// One k_cell_marginals launch per job: result block m of the last finish, summed by its column array (by_row: by its row array) into
// `tab` ([n_rows * stride] words): the sum of val goes to wide_col, the number of entries to c32_base (< 0: not counted).
struct MargJob { int m, wide_col, c32_base; };
static int launch_marginals(EngineImpl* im, const MargJob* job, const int n_job, const bool by_row, unsigned long long* tab, const int n_rows, const int stride) {
    for (int q = 0; q < n_job; q++) {
        const size_t z = im->res_nnz[job[q].m];
        if (!z) continue;
        const int32_t* d = im->d_res[job[q].m];
        if (!d) { im->eng->err = "internal: result block without a device copy"; return XCK_E_STATE; }
        MargArgs a;
        a.col = by_row ? d : d + z; a.val = d + 2 * z; a.n = (long long)z;
        a.ca.tab = tab; a.ca.n_rows = n_rows; a.ca.slot_mask = cs_slot_mask(im); a.ca.stride = stride;
        a.ca.c32_base = job[q].c32_base; a.ca.wide_col = job[q].wide_col;
        const size_t per = (size_t)JOIN_BLOCK * MG_ITEMS;
        hipLaunchKernelGGL(k_cell_marginals, dim3((unsigned)((z + per - 1) / per)), dim3(JOIN_BLOCK), 0, im->s_comp, a);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// column marginals of the matrices of the last finish -> im->h_cmat ([n_cells * k]); once per finish
static int cell_marginals(EngineImpl* im, const int k) {
    HIP_TRY(hipMemsetAsync(im->d_cmat, 0, (size_t)im->n_cells * k * sizeof(unsigned long long), im->s_comp));
    // basefc: umis = column sums of count, features = its entries; BAF: ad, dp, oth sums, features = entries of DP
    const MargJob fc[1] = { {0, 0, 1} }, baf[3] = { {1, 0, -1}, {2, 1, 3}, {3, 2, -1} };
    const bool is_fc = im->mode == XCK_MODE_BASEFC;
    if (int rc = launch_marginals(im, is_fc ? fc : baf, is_fc ? 1 : 3, false, im->d_cmat, im->n_cells, k)) return rc;
    im->h_cmat.resize((size_t)im->n_cells * k);
    HIP_TRY(hipMemcpyAsync(im->h_cmat.data(), im->d_cmat, im->h_cmat.size() * sizeof(int64_t), hipMemcpyDeviceToHost, im->s_comp));
    HIP_TRY(hipStreamSynchronize(im->s_comp));
    return 0;
}

// xck_get_cell_summary() for one pipeline: waits for the queued work, copies the table; the matrix half runs the first
// time after a finish and is kept until the next reset (a finished handle takes no more reads)
int engine_cell_summary(EngineImpl* im, xck_cell_summary* out) {
    if (!im->d_cell) { im->eng->err = "handle made without XCK_F_CELL_SUMMARY"; return XCK_E_STATE; }
    int rc = engine_flush(im); if (rc) return rc;
    const size_t rows = (size_t)im->n_cells + 1;
    im->h_cell_raw.resize(rows * CS_ROW_WORDS);
    HIP_TRY(hipMemcpy(im->h_cell_raw.data(), im->d_cell, im->h_cell_raw.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    im->h_cell.resize(rows * CS_COLS);
    for (size_t r = 0; r < rows; r++) for (int c = 0; c < CS_COLS; c++) im->h_cell[r * CS_COLS + c] = im->h_cell_raw[r * CS_ROW_WORDS + c];
    out->mode = im->mode; out->n_cells = im->n_cells; out->n_fate_cols = CS_COLS; out->fate = im->h_cell.data();
    out->n_matrix_cols = im->mode == XCK_MODE_BASEFC ? 2 : CS_MATRIX_COLS;
    out->has_matrix = im->finished ? 1 : 0; out->matrix = nullptr;
    if (im->finished) {
        if (!im->cmat_valid) { rc = cell_marginals(im, out->n_matrix_cols); if (rc) return rc; im->cmat_valid = true; }
        out->matrix = im->h_cmat.data();
    }
    return 0;
}
