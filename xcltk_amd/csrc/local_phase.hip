// local_phase.hip - region-wise local phasing on the device (xck_local_phase, include/xck.h).
//
// Restates reg_local_phasing (xcltk_amd/baf/fc/phasing.py) and snp_local_phasing / em_two_haplotypes / gaussian_smooth
// (xcltk_amd/baf/localphase.py) in fp64: same constants, same decisions, sums in a fixed order of this file's own.
// One workgroup of 256 threads owns one region at a time and walks the regions of its launch (one level, api.cpp) in a grid-stride
// loop; every resident workgroup has a slice of one HBM scratch block for what does not fit in LDS:
//   per cell     the map global cell -> local cell, the cell-major (transposed) entry lists, alive flags, the four logs of the M-step
//   per SNP      where its column lies, its position, log-sum-exp terms; z and orientation too when the region is too large for LDS
//   per region   the normalised smoothing weights, where they fit
// Work inside the region goes to GROUPS of G lanes (G a power of two up to 64, chosen from the number of SNPs / cells so that about
// 256 lanes are busy): a group owns one SNP or one cell, its lanes stride over the entries in a fixed order and a xor butterfly adds
// the partial sums, which gives every lane of the group the same bits.  No floating-point atomic, no order that depends on timing.
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include "xck_internal.h"

#pragma clang fp contract(off)   // a * b + c stays two roundings, as in the numpy statement

namespace {

constexpr int BT = 256;                  // threads of a workgroup
constexpr int NS_LDS = 1024;             // SNPs whose z / orientation fit in LDS
constexpr int W_CAP = 512;               // SNPs whose weight matrix fits in the slice
constexpr double LOW_BAF = 0.45, UP_BAF = 0.55, EPS_THETA = 1e-6, TOL = 1e-3;
constexpr int EM_MIN_ITER = 10, EM_MAX_ITER = 1000, RND_MIN_ITER = 5, RND_MAX_ITER = 50;
constexpr double KERNEL_B2 = 20000.0 * 20000.0;

// offsets (bytes) of the arrays of one scratch slice; the same function sizes the block on the host
struct Slice {
    size_t cloc, cptr, ccur, alive, lt, t_k, t_ad, t_dp, e_lc, kslot, kbeg, klen, kent, kpos, lse, wsum, gz0, gzr, gor, gff, wn, bytes;
    __host__ __device__ Slice(int n_cells, int max_n, int max_e, int m_cap, int w_cap) {
        size_t o = 0;
        auto take = [&o](size_t n) { size_t at = o; o += (n + 15) & ~size_t(15); return at; };
        cloc = take(sizeof(int) * (size_t)n_cells);
        cptr = take(sizeof(int) * ((size_t)m_cap + 1));
        ccur = take(sizeof(int) * (size_t)m_cap);
        alive = take((size_t)m_cap);
        lt = take(sizeof(double) * 4 * (size_t)m_cap);
        t_k = take(sizeof(int) * (size_t)max_e);
        t_ad = take(sizeof(int) * (size_t)max_e);
        t_dp = take(sizeof(int) * (size_t)max_e);
        e_lc = take(sizeof(int) * (size_t)max_e);
        kslot = take(sizeof(int) * (size_t)max_n);
        kbeg = take(sizeof(long long) * (size_t)max_n);
        klen = take(sizeof(int) * (size_t)max_n);
        kent = take(sizeof(int) * (size_t)max_n);
        kpos = take(sizeof(long long) * (size_t)max_n);
        lse = take(sizeof(double) * (size_t)max_n);
        wsum = take(sizeof(double) * (size_t)max_n);
        gz0 = take(sizeof(double) * (size_t)max_n);
        gzr = take(sizeof(double) * (size_t)max_n);
        gor = take((size_t)max_n);
        gff = take((size_t)max_n);
        wn = take(sizeof(double) * (size_t)w_cap * (size_t)w_cap);
        bytes = o;
    }
};

struct PhaseArgs {
    const long long* col_ptr; const int* cell; const int* ad; const int* dp; const unsigned char* cell_enabled; int n_cells;
    const long long* reg_ptr; const int* slot_col; const int* slot_snp; const long long* slot_pos;
    const int* regs; int n_regs;                       // the regions of this launch
    signed char* ref_hap; signed char* alt_hap;        // SNP state: read at entry, flipped at the end
    unsigned char* kept; unsigned char* flip; unsigned char* status;
    char* scratch; int max_n, max_e, m_cap, w_cap, lds_snps;
};

__device__ __forceinline__ int pow2_group(int n) {     // lanes per item so that about BT lanes are busy with n items
    int g = 1;
    while (g < 64 && (long long)n * (g * 2) <= BT) g *= 2;
    return g;
}
__device__ __forceinline__ double gsum(double v, int G) { for (int o = G >> 1; o; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ long long gsum(long long v, int G) { for (int o = G >> 1; o; o >>= 1) v += __shfl_xor(v, o); return v; }

// exclusive scan of two ints per item over n items: thread t owns the items [t * per, (t + 1) * per); get(i, a, b) reads item i,
// put(i, ea, eb, a, b) receives its exclusive prefixes.  Returns the totals through s_tot.  Every thread of the block calls it.
template <class Get, class Put>
__device__ void block_scan2(int n, int* s_a, int* s_b, int* s_tot, Get get, Put put) {
    const int t = threadIdx.x;
    const int per = (n + BT - 1) / BT;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    int ta = 0, tb = 0;
    for (int i = lo; i < hi; i++) { int a, b; get(i, a, b); ta += a; tb += b; }
    s_a[t] = ta; s_b[t] = tb;
    __syncthreads();
    for (int o = 1; o < BT; o <<= 1) {                 // Hillis-Steele, inclusive
        int xa = t >= o ? s_a[t - o] : 0, xb = t >= o ? s_b[t - o] : 0;
        __syncthreads();
        s_a[t] += xa; s_b[t] += xb;
        __syncthreads();
    }
    int ea = s_a[t] - ta, eb = s_b[t] - tb;
    if (t == BT - 1) { s_tot[0] = s_a[t]; s_tot[1] = s_b[t]; }
    for (int i = lo; i < hi; i++) { int a, b; get(i, a, b); put(i, ea, eb, a, b); ea += a; eb += b; }
    __syncthreads();
}

__global__ __launch_bounds__(BT) void k_local_phase(PhaseArgs A) {
    __shared__ double s_z0[NS_LDS], s_zr[NS_LDS];
    __shared__ unsigned char s_or[NS_LDS], s_ff[NS_LDS];
    __shared__ int s_a[BT], s_b[BT], s_tot[2];
    __shared__ int s_cnt[2];
    __shared__ double s_ll;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const Slice L(A.n_cells, A.max_n, A.max_e, A.m_cap, A.w_cap);
    char* base = A.scratch + (size_t)blockIdx.x * L.bytes;
    int* cloc = (int*)(base + L.cloc); int* cptr = (int*)(base + L.cptr); int* ccur = (int*)(base + L.ccur);
    unsigned char* alive = (unsigned char*)(base + L.alive); double* lt = (double*)(base + L.lt);
    int* t_k = (int*)(base + L.t_k); int* t_ad = (int*)(base + L.t_ad); int* t_dp = (int*)(base + L.t_dp); int* e_lc = (int*)(base + L.e_lc);
    int* kslot = (int*)(base + L.kslot); long long* kbeg = (long long*)(base + L.kbeg); int* klen = (int*)(base + L.klen);
    int* kent = (int*)(base + L.kent); long long* kpos = (long long*)(base + L.kpos); double* lse = (double*)(base + L.lse);
    double* wsum = (double*)(base + L.wsum); double* wn = (double*)(base + L.wn);

    for (int ri = blockIdx.x; ri < A.n_regs; ri += gridDim.x) {
        const int r = A.regs[ri];
        const long long s0 = A.reg_ptr[r];
        const int n = (int)(A.reg_ptr[r + 1] - s0);
        // ---- 1. masks: which slots have depth in the enabled cells, how many entries every cell has
        for (int c = t; c < A.n_cells; c += BT) cloc[c] = 0;
        __syncthreads();
        for (int j = wave; j < n; j += BT / 64) {
            const int col = A.slot_col[s0 + j];
            bool has = false;
            if (col >= 0) {
                const long long b = A.col_ptr[col], e = A.col_ptr[col + 1];
                for (long long p = b + lane; p < e; p += 64) {
                    const int c = A.cell[p];
                    if (A.dp[p] > 0 && (!A.cell_enabled || A.cell_enabled[c])) { has = true; atomicAdd(&cloc[c], 1); }
                }
            }
            has = __any(has);
            if (lane == 0) { A.kept[s0 + j] = has; A.flip[s0 + j] = 0; }
        }
        __syncthreads();
        // ---- 2. kept SNPs in slot order (k), their columns; cells with depth in ascending order (local id), their entry ranges
        block_scan2(n, s_a, s_b, s_tot,
            [&](int j, int& a, int& b) { a = A.kept[s0 + j]; const int col = A.slot_col[s0 + j]; b = a ? (int)(A.col_ptr[col + 1] - A.col_ptr[col]) : 0; },
            [&](int j, int ea, int eb, int a, int b) { if (a) { kslot[ea] = j; kent[ea] = eb; klen[ea] = b; kbeg[ea] = A.col_ptr[A.slot_col[s0 + j]]; kpos[ea] = A.slot_pos[s0 + j]; } });
        const int N = s_tot[0];
        __syncthreads();
        block_scan2(A.n_cells, s_a, s_b, s_tot,
            [&](int c, int& a, int& b) { b = cloc[c]; a = b > 0; },
            [&](int c, int ea, int eb, int a, int b) { if (a) { cloc[c] = ea; cptr[ea] = eb; ccur[ea] = eb; alive[ea] = 1; } else cloc[c] = -1; });
        const int M = s_tot[0], E = s_tot[1];
        __syncthreads();
        if (M == 0) {                                  // no cell with depth: the host returns None before the first round
            if (t == 0) A.status[r] = XCK_PHASE_FAILED;
            continue;
        }
        if (t == 0) cptr[M] = E;
        const bool in_lds = N <= A.lds_snps;
        double* z0 = in_lds ? s_z0 : (double*)(base + L.gz0);
        double* zr = in_lds ? s_zr : (double*)(base + L.gzr);
        unsigned char* orient = in_lds ? s_or : (unsigned char*)(base + L.gor);
        unsigned char* ff = in_lds ? s_ff : (unsigned char*)(base + L.gff);
        for (int k = t; k < N; k += BT) {              // entry orientation: AD counts the REF haplotype as it is now
            orient[k] = A.ref_hap[A.slot_snp[s0 + kslot[k]]] == 1;
            ff[k] = 0;
        }
        __syncthreads();
        // ---- 3. transpose to cell-major, SNP after SNP so that every cell's list is in SNP order
        for (int k = 0; k < N; k++) {
            const long long b = kbeg[k];
            const int len = klen[k], eo = kent[k];
            for (int i = t; i < len; i += BT) {
                const int c = A.cell[b + i], d = A.dp[b + i];
                int lc = -1;
                if (d > 0 && (!A.cell_enabled || A.cell_enabled[c])) {
                    lc = cloc[c];
                    const int p = atomicAdd(&ccur[lc], 1);          // (one entry per cell and column: no two threads meet here)
                    t_k[p] = k; t_ad[p] = A.ad[b + i]; t_dp[p] = d;
                }
                e_lc[eo + i] = lc;
            }
            __syncthreads();
        }
        const int Gs = pow2_group(N), Gc = pow2_group(M);
        const int gs_id = t / Gs, gs_l = t % Gs, gs_n = BT / Gs;
        const int gc_id = t / Gc, gc_l = t % Gc, gc_n = BT / Gc;
        // ---- 4. smoothing weights: they depend on the positions alone
        const bool w_stored = N <= A.w_cap;
        auto weight = [&](int i, int j) { const long long dx = kpos[j] - kpos[i]; return exp(0.0 - (double)(dx * dx) / KERNEL_B2); };
        auto w_at = [&](int i, int j) -> double& { return Gs == 1 ? wn[(size_t)j * N + i] : wn[(size_t)i * N + j]; };
        for (int i0 = 0; i0 < N; i0 += gs_n) {
            const int i = i0 + gs_id;
            double s = 0.0;
            if (i < N) for (int j = gs_l; j < N; j += Gs) s += weight(i, j);
            s = gsum(s, Gs);
            if (i < N && gs_l == 0) wsum[i] = s;
            if (i < N && w_stored) for (int j = gs_l; j < N; j += Gs) w_at(i, j) = weight(i, j) / s;
        }
        __syncthreads();

        // the three passes of one EM iteration
        auto m_step = [&]() {                          // per cell: thetas of both components from the entries of the cell, then their logs
            for (int c0 = 0; c0 < M; c0 += gc_n) {
                const int c = c0 + gc_id;
                double s1 = 0, s2 = 0, s3 = 0, s4 = 0; long long sd = 0;
                const bool on = c < M && alive[c];
                if (on) for (int p = cptr[c] + gc_l, pe = cptr[c + 1]; p < pe; p += Gc) {
                    const int k = t_k[p], d = t_dp[p];
                    const int a = orient[k] ? d - t_ad[p] : t_ad[p];
                    const double za = z0[k], zb = 1.0 - za, zc = 1.0 - zb;
                    s1 += (double)a * za; s2 += (double)(d - a) * zb;           // AD.T @ Z[:, 0], BD.T @ (1 - Z)[:, 0]
                    s3 += (double)a * zb; s4 += (double)(d - a) * zc;           // ... [:, 1]
                    sd += d;
                }
                s1 = gsum(s1, Gc); s2 = gsum(s2, Gc); s3 = gsum(s3, Gc); s4 = gsum(s4, Gc); sd = gsum(sd, Gc);
                if (on && gc_l == 0) {
                    double th0 = (s1 + s2) / (double)sd, th1 = (s3 + s4) / (double)sd;
                    if (th0 <= 0) th0 = EPS_THETA; if (th0 >= 1) th0 = 1 - EPS_THETA;
                    if (th1 <= 0) th1 = EPS_THETA; if (th1 >= 1) th1 = 1 - EPS_THETA;
                    lt[4 * c + 0] = log(th0); lt[4 * c + 1] = log(1 - th0); lt[4 * c + 2] = log(th1); lt[4 * c + 3] = log(1 - th1);
                }
            }
            __syncthreads();
        };
        auto loglik = [&]() {                          // per SNP: log-likelihood under both components, its log-sum-exp, the E-step
            for (int k0 = 0; k0 < N; k0 += gs_n) {
                const int k = k0 + gs_id;
                double a0 = 0, b0 = 0, a1 = 0, b1 = 0;
                if (k < N) {
                    const long long b = kbeg[k]; const int eo = kent[k]; const bool sw = orient[k];
                    for (int i = gs_l, len = klen[k]; i < len; i += Gs) {
                        const int lc = e_lc[eo + i];
                        if (lc < 0 || !alive[lc]) continue;
                        const int d = A.dp[b + i], a = sw ? d - A.ad[b + i] : A.ad[b + i];
                        const double* q = lt + 4 * (size_t)lc;
                        a0 += (double)a * q[0]; b0 += (double)(d - a) * q[1];
                        a1 += (double)a * q[2]; b1 += (double)(d - a) * q[3];
                    }
                }
                a0 = gsum(a0, Gs); b0 = gsum(b0, Gs); a1 = gsum(a1, Gs); b1 = gsum(b1, Gs);
                if (k < N && gs_l == 0) {
                    const double m0 = a0 + b0, m1 = a1 + b1, mx = fmax(m0, m1);
                    const double e0 = exp(m0 - mx), e1 = exp(m1 - mx), s = e0 + e1;
                    lse[k] = log(s) + mx;
                    zr[k] = e0 / s;
                }
            }
            __syncthreads();
            if (wave == 0) {
                double s = 0;
                for (int k = lane; k < N; k += 64) s += lse[k];
                s = gsum(s, 64);
                if (lane == 0) s_ll = s;
            }
            __syncthreads();
        };
        auto smooth = [&]() {                          // z0[i] = sum_j zr[j] w_ij / sum_j w_ij over all SNPs of the region
            for (int i0 = 0; i0 < N; i0 += gs_n) {
                const int i = i0 + gs_id;
                double u = 0;
                if (i < N) {
                    if (w_stored) for (int j = gs_l; j < N; j += Gs) u += zr[j] * w_at(i, j);
                    else { const double ws = wsum[i]; for (int j = gs_l; j < N; j += Gs) u += zr[j] * (weight(i, j) / ws); }
                }
                u = gsum(u, Gs);
                if (i < N && gs_l == 0) z0[i] = u;
            }
            __syncthreads();
        };

        // ---- 5. rounds
        bool failed = false;
        for (int round = 0; round < RND_MAX_ITER; round++) {
            if (t < 2) s_cnt[t] = 0;
            __syncthreads();
            // cells: BAF from integer sums, one divide; cells in [0.45, 0.55] leave for good
            int n_alive = 0;
            for (int c0 = 0; c0 < M; c0 += gc_n) {
                const int c = c0 + gc_id;
                long long sa = 0, sd = 0;
                const bool on = c < M && alive[c];
                if (on) for (int p = cptr[c] + gc_l, pe = cptr[c + 1]; p < pe; p += Gc) {
                    const int d = t_dp[p];
                    sa += orient[t_k[p]] ? d - t_ad[p] : t_ad[p]; sd += d;
                }
                sa = gsum(sa, Gc); sd = gsum(sd, Gc);
                if (on && gc_l == 0) {
                    const double baf = (double)sa / (double)sd;
                    if (baf < LOW_BAF || baf > UP_BAF) n_alive++; else alive[c] = 0;
                }
            }
            if (n_alive) atomicAdd(&s_cnt[0], n_alive);
            __syncthreads();
            if (s_cnt[0] == 0) { failed = true; break; }                    // no informative cell left, in whichever round
            // SNPs: Z at the start of the EM from integer sums; a SNP that lost all its depth makes the round's Z NaN on the host
            for (int k0 = 0; k0 < N; k0 += gs_n) {
                const int k = k0 + gs_id;
                long long sa = 0, sd = 0;
                if (k < N) {
                    const long long b = kbeg[k]; const int eo = kent[k]; const bool sw = orient[k];
                    for (int i = gs_l, len = klen[k]; i < len; i += Gs) {
                        const int lc = e_lc[eo + i];
                        if (lc < 0 || !alive[lc]) continue;
                        const int d = A.dp[b + i];
                        sa += sw ? d - A.ad[b + i] : A.ad[b + i]; sd += d;
                    }
                }
                sa = gsum(sa, Gs); sd = gsum(sd, Gs);
                if (k < N && gs_l == 0) {
                    if (sd == 0) atomicOr(&s_cnt[1], 1); else z0[k] = (double)sa / (double)sd;
                }
            }
            __syncthreads();
            // NaN round: the host iterates 1000 times over NaN, flips nothing, changes nothing and so repeats the round until it may
            // stop (round 5): the flips XORed so far are the result
            if (s_cnt[1]) break;
            // EM (em_two_haplotypes): warm start, then E-step + smoothing + M-step until the log-likelihood gains less than TOL
            m_step();
            loglik();
            for (int it = 0; it < EM_MAX_ITER; it++) {
                const double ll_old = s_ll;
                __syncthreads();                                             // (everyone has read s_ll before loglik() writes it)
                smooth();
                m_step();
                loglik();
                if (it >= EM_MIN_ITER && s_ll - ll_old < TOL) break;
            }
            // flip = Z1 >= Z0, XOR into the running flip; stop when i >= 5 and the round flipped all or none
            int n_flip = 0;
            for (int k = t; k < N; k += BT) {
                const double za = z0[k], zb = 1.0 - za;
                const bool f = zb >= za;
                if (f) { n_flip++; ff[k] ^= 1; orient[k] ^= 1; }            // (re-orient AD by the flip: unused when the loop ends here)
            }
            __syncthreads();                                                 // (s_cnt[0] was read by all; now it counts the flips)
            if (t == 0) s_cnt[0] = 0;
            __syncthreads();
            if (n_flip) atomicAdd(&s_cnt[0], n_flip);
            __syncthreads();
            const int nf = s_cnt[0];
            __syncthreads();
            if (round >= RND_MIN_ITER && (nf == N || nf == 0)) break;
        }
        // ---- 6. majority rule, results, the SNP state for the regions that follow
        if (failed) {
            if (t == 0) A.status[r] = XCK_PHASE_FAILED;
        } else {
            if (t == 0) s_cnt[0] = 0;
            __syncthreads();
            int nf = 0;
            for (int k = t; k < N; k += BT) nf += ff[k];
            if (nf) atomicAdd(&s_cnt[0], nf);
            __syncthreads();
            const bool invert = (double)s_cnt[0] / (double)N > 0.5;
            for (int k = t; k < N; k += BT) {
                const int f = ff[k] ^ (invert ? 1 : 0);
                const int j = kslot[k];
                A.flip[s0 + j] = (unsigned char)f;
                if (f) { const int s = A.slot_snp[s0 + j]; A.ref_hap[s] = 1 - A.ref_hap[s]; A.alt_hap[s] = 1 - A.alt_hap[s]; }
            }
            if (t == 0) A.status[r] = XCK_PHASE_PHASED;
        }
        __syncthreads();
    }
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
};
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

namespace xck {

int local_phase_run(const xck_phase_problem* P, const PhasePlan& plan, double ms_prepare, xck_phase_result** out) {
    auto fail = [](hipError_t e, const char* what) {
        set_thread_error(std::string("xck_local_phase: ") + what + ": " + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? XCK_E_NOMEM : XCK_E_DEVICE;
    };
#define PH_TRY(expr, what) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(e_, what); } while (0)
    const double t0 = now_ms();
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { set_thread_error("xck_local_phase: no usable HIP device"); return XCK_E_DEVICE; }
    if (P->device < 0 || P->device >= n_dev) { set_thread_error("xck_local_phase: no such device"); return XCK_E_DEVICE; }
    PH_TRY(hipSetDevice(P->device), "hipSetDevice");
    auto knob = [](const char* name, int dflt) { const char* e = getenv(name); if (!e || !*e) return dflt; return (int)std::max(1ll, std::min((long long)dflt, atoll(e))); };
    const int w_knob = knob("XCK_PHASE_WCAP", W_CAP), lds_snps = knob("XCK_PHASE_LDS_SNPS", NS_LDS);

    const int64_t nnz = P->col_ptr[P->n_cols], n_slots = P->reg_ptr[P->n_regions];
    const int n_levels = (int)plan.level_beg.size() - 1;
    const int max_n = std::max(1, plan.max_n), max_e = std::max(1, plan.max_e);
    const int m_cap = std::max(1, std::min(P->n_cells, max_e)), w_cap = std::min(max_n, w_knob);
    const Slice L(P->n_cells, max_n, max_e, m_cap, w_cap);
    int widest = 1;
    for (int l = 0; l < n_levels; l++) widest = std::max(widest, plan.level_beg[l + 1] - plan.level_beg[l]);
    size_t free_b = 0, total_b = 0;
    PH_TRY(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
    const size_t budget = std::min<size_t>(free_b / 2, size_t(8) << 30);
    const int n_blocks = (int)std::max<size_t>(1, std::min<size_t>(std::min(widest, knob("XCK_PHASE_BLOCKS", 2048)), budget / L.bytes));

    xck_phase_result* R = (xck_phase_result*)calloc(1, sizeof(xck_phase_result));
    uint8_t* h_kept = (uint8_t*)malloc(std::max<int64_t>(1, n_slots)); uint8_t* h_flip = (uint8_t*)malloc(std::max<int64_t>(1, n_slots));
    uint8_t* h_status = (uint8_t*)malloc(std::max(1, P->n_regions));
    int8_t* h_ref = (int8_t*)malloc(std::max(1, P->n_snps)); int8_t* h_alt = (int8_t*)malloc(std::max(1, P->n_snps));
    struct HostGuard { xck_phase_result* r; void* a[5]; bool keep = false; ~HostGuard() { if (!keep) { for (void* p : a) free(p); free(r); } } } hg{R, {h_kept, h_flip, h_status, h_ref, h_alt}};
    if (!R || !h_kept || !h_flip || !h_status || !h_ref || !h_alt) { set_thread_error("xck_local_phase: out of host memory"); return XCK_E_NOMEM; }

    DevBuf d_col_ptr, d_cell, d_ad, d_dp, d_en, d_ref, d_alt, d_reg_ptr, d_scol, d_ssnp, d_spos, d_regs, d_kept, d_flip, d_status, d_scratch;
    auto up = [&](DevBuf& b, const void* src, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(&b.p, std::max<size_t>(bytes, 16));
        if (e != hipSuccess) return e;
        return bytes ? hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    PH_TRY(up(d_col_ptr, P->col_ptr, sizeof(int64_t) * ((size_t)P->n_cols + 1)), "pileup to the device");
    PH_TRY(up(d_cell, P->cell, sizeof(int32_t) * (size_t)nnz), "pileup to the device");
    PH_TRY(up(d_ad, P->ad, sizeof(int32_t) * (size_t)nnz), "pileup to the device");
    PH_TRY(up(d_dp, P->dp, sizeof(int32_t) * (size_t)nnz), "pileup to the device");
    if (P->cell_enabled) PH_TRY(up(d_en, P->cell_enabled, (size_t)P->n_cells), "cell mask to the device");
    PH_TRY(up(d_ref, P->ref_hap, (size_t)P->n_snps), "SNP state to the device");
    PH_TRY(up(d_alt, P->alt_hap, (size_t)P->n_snps), "SNP state to the device");
    PH_TRY(up(d_reg_ptr, P->reg_ptr, sizeof(int64_t) * ((size_t)P->n_regions + 1)), "regions to the device");
    PH_TRY(up(d_scol, P->slot_col, sizeof(int32_t) * (size_t)n_slots), "regions to the device");
    PH_TRY(up(d_ssnp, P->slot_snp, sizeof(int32_t) * (size_t)n_slots), "regions to the device");
    PH_TRY(up(d_spos, P->slot_pos, sizeof(int64_t) * (size_t)n_slots), "regions to the device");
    PH_TRY(up(d_regs, plan.order.data(), sizeof(int32_t) * plan.order.size()), "regions to the device");
    PH_TRY(hipMalloc(&d_kept.p, std::max<size_t>(16, (size_t)n_slots)), "result buffers");
    PH_TRY(hipMalloc(&d_flip.p, std::max<size_t>(16, (size_t)n_slots)), "result buffers");
    PH_TRY(hipMalloc(&d_status.p, std::max<size_t>(16, (size_t)P->n_regions)), "result buffers");
    PH_TRY(hipMemset(d_kept.p, 0, std::max<size_t>(16, (size_t)n_slots)), "result buffers");
    PH_TRY(hipMemset(d_flip.p, 0, std::max<size_t>(16, (size_t)n_slots)), "result buffers");
    PH_TRY(hipMemset(d_status.p, 0, std::max<size_t>(16, (size_t)P->n_regions)), "result buffers");
    PH_TRY(hipMalloc(&d_scratch.p, L.bytes * (size_t)n_blocks), "scratch block");
    const double t1 = now_ms();

    PhaseArgs A;
    A.col_ptr = (const long long*)d_col_ptr.p; A.cell = (const int*)d_cell.p; A.ad = (const int*)d_ad.p; A.dp = (const int*)d_dp.p;
    A.cell_enabled = (const unsigned char*)d_en.p; A.n_cells = P->n_cells;
    A.reg_ptr = (const long long*)d_reg_ptr.p; A.slot_col = (const int*)d_scol.p; A.slot_snp = (const int*)d_ssnp.p; A.slot_pos = (const long long*)d_spos.p;
    A.ref_hap = (signed char*)d_ref.p; A.alt_hap = (signed char*)d_alt.p;
    A.kept = (unsigned char*)d_kept.p; A.flip = (unsigned char*)d_flip.p; A.status = (unsigned char*)d_status.p;
    A.scratch = (char*)d_scratch.p; A.max_n = max_n; A.max_e = max_e; A.m_cap = m_cap; A.w_cap = w_cap; A.lds_snps = lds_snps;
    for (int l = 0; l < n_levels; l++) {               // one launch per level, in stream order: level l reads the state levels < l left
        const int cnt = plan.level_beg[l + 1] - plan.level_beg[l];
        if (cnt <= 0) continue;
        A.regs = (const int*)d_regs.p + plan.level_beg[l]; A.n_regs = cnt;
        hipLaunchKernelGGL(k_local_phase, dim3(std::min(cnt, n_blocks)), dim3(BT), 0, 0, A);
        PH_TRY(hipGetLastError(), "kernel launch");
    }
    PH_TRY(hipDeviceSynchronize(), "kernel");
    const double t2 = now_ms();
    if (n_slots) { PH_TRY(hipMemcpy(h_kept, d_kept.p, (size_t)n_slots, hipMemcpyDeviceToHost), "results to the host"); PH_TRY(hipMemcpy(h_flip, d_flip.p, (size_t)n_slots, hipMemcpyDeviceToHost), "results to the host"); }
    if (P->n_regions) PH_TRY(hipMemcpy(h_status, d_status.p, (size_t)P->n_regions, hipMemcpyDeviceToHost), "results to the host");
    if (P->n_snps) { PH_TRY(hipMemcpy(h_ref, d_ref.p, (size_t)P->n_snps, hipMemcpyDeviceToHost), "results to the host"); PH_TRY(hipMemcpy(h_alt, d_alt.p, (size_t)P->n_snps, hipMemcpyDeviceToHost), "results to the host"); }
    for (DevBuf* b : { &d_col_ptr, &d_cell, &d_ad, &d_dp, &d_en, &d_ref, &d_alt, &d_reg_ptr, &d_scol, &d_ssnp, &d_spos, &d_regs, &d_kept, &d_flip, &d_status, &d_scratch })
        if (b->p) { (void)hipFree(b->p); b->p = nullptr; }
    const double t3 = now_ms();
#undef PH_TRY
    R->n_slots = n_slots; R->kept = h_kept; R->flip = h_flip;
    R->n_regions = P->n_regions; R->n_snps = P->n_snps; R->status = h_status; R->ref_hap = h_ref; R->alt_hap = h_alt;
    R->n_levels = n_levels; R->n_blocks = n_blocks;
    R->ms_prepare = ms_prepare; R->ms_h2d = t1 - t0; R->ms_kernel = t2 - t1; R->ms_d2h = t3 - t2;
    hg.keep = true;
    *out = R;
    return XCK_OK;
}

void local_phase_free(xck_phase_result* r) {
    if (!r) return;
    free((void*)r->kept); free((void*)r->flip); free((void*)r->status); free((void*)r->ref_hap); free((void*)r->alt_hap);
    free(r);
}

}  // namespace xck
