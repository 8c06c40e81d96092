"""An extended-precision restatement of region-wise local phasing, with the margin of every float-decided step.

What it restates: reg_local_phasing (baf/fc/phasing.py) -> snp_local_phasing -> em_two_haplotypes -> gaussian_smooth
(baf/localphase.py), which csrc/local_phase.hip restates in fp64 on the device.  Neither module is imported.  All sums, logs and
exponentials run in numpy.longdouble (x87 extended, 64-bit mantissa, eps 1.1e-19), as plain array expressions in numpy's own order.

Steps decided by integers or by ONE float64 operation are computed exactly as the host and the device compute them:
  * which SNPs and cells have depth, the re-orientation of AD by ref_hap and by every round's flips, the majority rule: integers;
  * a cell's BAF is one float64 division of two integer sums, compared with the float64 literals 0.45 and 0.55 (9/20 == 0.45);
  * Z at the start of an EM is one float64 division of two integer sums;
  * a SNP without depth in the cells that remain makes the round a NaN round: nothing flips, the flips XORed so far stand (the
    host repeats the unchanged round until round 5 lets it stop, the device stops at once);
  * theta is clipped where the FLOAT64 theta is <= 0 or >= 1.  That happens through saturation (a posterior that rounds to 1.0
    makes 1 - z exactly 0), which extended precision does not reach at the same place, so the clip mask - the mask alone - is
    taken from a float64 evaluation of the same expression on the posteriors rounded to float64.  A clip that still differs moves
    one log by less than 1e-6 per read on a cell whose reads all agree with a saturated posterior, and by the same amount in
    ll_new and ll_old; it is not among the margins.

Steps decided by accumulated float arithmetic have a MARGIN, and a region is DECISIVE when every margin exceeds four times a
first-order bound on what float64 rounding and summation order can move (u = 2^-53; M cells, N SNPs, R reads of the region):

  stop rule  `it >= 10 and ll_new - ll_old < 1e-3`: margin |(ll_new - ll_old) - 1e-3| at every iteration where it is evaluated.
    ll = sum_k lse_k, lse_k = log(exp m_k0 + exp m_k1), m_kh = sum_c a_kc log th_ch + b_kc log(1 - th_ch).  Every term of m is
    <= 0, so the sum of the terms' magnitudes is |m| itself, and the standard bound for a sum of n terms in any order,
    |err| <= (n - 1) u sum |x_i|, gives |dm_kh| <= (M + 2) u |m_kh| with the product and the log rounded as well.  lse weighs
    dm_k0 and dm_k1 by the posterior, and z |m_k0| <= |lse_k| + 1 whichever component wins (x e^-x <= 1/e), so
    |dlse_k| <= (M + 4) u (|lse_k| + 1); the outer sum over N SNPs adds (N - 1) u |ll|.  The thetas that enter are themselves
    sums of at most N terms divided once: relative error (N + 2) u, which moves log th by as much and so m by (N + 2) u times
    the reads.  Together
        |d ll| <= u [ (M + N + 6) (|ll| + N) + (N + 3) R ]
    and the difference of two of them has twice that:   ll_bound = 4 * 2 * u * [(M + N + 6) (|ll| + N) + (N + 3) R].
    (A theta within 1e-3 of 0 or 1 amplifies its own error in the log of the other allele; reads of that other allele pull theta
    away unless their SNP's posterior is saturated, and then the term feeds the losing component, which lse ignores.)

  flip  `Z1 >= Z0`: margin |1 - 2 z| over all SNPs at the end of every non-NaN round.  z_i = sum_j w_ij zr_j with normalised
    weights, zr_k = 1 / (1 + exp(m_k1 - m_k0)).  The logistic function has slope <= 1/4, so
    |dzr_k| <= [(M + 2) (|m_k0| + |m_k1|) + 2 (N + 3) D_k] u / 4 + 3 u  (D_k reads of SNP k), and a convex combination of N such
    values with weights of relative error (N + 2) u adds (2 N + 4) u.  |1 - 2 z| moves by twice that:
        z_bound = 4 * 2 * u * [ max_k ((M + 2) (|m_k0| + |m_k1|) + 2 (N + 3) D_k) / 4 + 2 N + 7 ].
    This bounds one evaluation.  An error made in an earlier iteration reaches the last one through the EM map; near a fixed
    point that map contracts, and the factor of four is what is left for it.

The bounds are computed per region and per evaluation from that region's own M, N, R, |ll| and |m|.  At the sizes of these tests
(M <= 400, N <= 257, R <= 1.6e5, |ll| <= 1.3e4) the largest are 4.2e-9 for the stop rule and 4.5e-10 for the flip.  They were derived
before any comparison was run and are held from both sides: tests/test_local_phase_oracle_host.py requires the float64 host path to
equal the oracle on every decisive region (bounds too small would fail that) and at most 15 % of the generated sweep to be
non-decisive (bounds too large would fail that).
"""
import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
LOW_BAF, UP_BAF, EPS_THETA, TOL = 0.45, 0.55, 1e-6, 1e-3
EM_MIN_ITER, EM_MAX_ITER, RND_MIN_ITER, RND_MAX_ITER = 10, 1000, 5, 50
KERNEL_B = 20000
FACTOR = 4.0
INF = float("inf")


def ll_bound(M, N, R, ll_abs):
    return FACTOR * 2 * U64 * ((M + N + 6) * (ll_abs + N) + (N + 3) * R)


def z_bound(M, N, m_abs, D):
    """m_abs, D: per SNP |m_k0| + |m_k1| and reads."""
    return FACTOR * 2 * U64 * (float(np.max((M + 2) * m_abs + 2 * (N + 3) * D)) / 4 + 2 * N + 7)


class Margins:
    """The smallest margin / bound ratio of either kind, with the margin and the bound it was taken at."""

    def __init__(self):
        self.z, self.z_bound, self.ll, self.ll_bound, self.ll_abs = INF, 0.0, INF, 0.0, 0.0
        self.rounds = self.em_iters = self.nan_round = 0

    def see_ll(self, margin, bound, ll_abs):
        if self.ll == INF or margin * self.ll_bound < self.ll * bound:
            self.ll, self.ll_bound, self.ll_abs = margin, bound, ll_abs

    def see_z(self, margin, bound):
        if self.z == INF or margin * self.z_bound < self.z * bound:
            self.z, self.z_bound = margin, bound

    @property
    def decisive(self):
        return self.z > self.z_bound and self.ll > self.ll_bound


def _em(AD, DP, pos, mg):
    """AD, DP: SNP x cell int64, every SNP and every cell with depth.  -> z (longdouble) after the last smoothing."""
    N, M = AD.shape
    BD = DP - AD
    A, B = AD.astype(LD), BD.astype(LD)
    Af, Bf = AD.astype(np.float64), BD.astype(np.float64)
    depth, R, D = DP.sum(axis=0), int(DP.sum()), DP.sum(axis=1).astype(np.float64)
    dx = (pos[None, :] - pos[:, None]).astype(LD)
    W = np.exp(-(dx * dx) / (LD(KERNEL_B) * LD(KERNEL_B)))
    W = W / W.sum(axis=1, keepdims=True)

    def m_step(z):
        zf = z.astype(np.float64)
        zb = 1.0 - zf
        zc = 1.0 - zb
        logs = []
        for th, thf in (((z @ A + (1 - z) @ B) / depth, (zf @ Af + zb @ Bf) / depth), (((1 - z) @ A + z @ B) / depth, (zb @ Af + zc @ Bf) / depth)):
            th = np.where(thf <= 0, LD(EPS_THETA), np.where(thf >= 1, LD(1) - LD(EPS_THETA), th))
            logs.append((np.log(th), np.log(1 - th)))
        return logs

    def loglik(logs):
        m0, m1 = A @ logs[0][0] + B @ logs[0][1], A @ logs[1][0] + B @ logs[1][1]
        mx = np.maximum(m0, m1)
        e0, e1 = np.exp(m0 - mx), np.exp(m1 - mx)
        return m0, m1, e0 / (e0 + e1), np.sum(np.log(e0 + e1) + mx)

    z = (AD.sum(axis=1) / DP.sum(axis=1)).astype(LD)                     # one float64 division of two integer sums
    m0, m1, zr, ll_new = loglik(m_step(z))
    for it in range(EM_MAX_ITER):
        ll_old = ll_new
        z = W @ zr
        m0, m1, zr, ll_new = loglik(m_step(z))
        mg.em_iters += 1
        if it >= EM_MIN_ITER:
            gain = ll_new - ll_old
            ll_abs = float(max(abs(ll_new), abs(ll_old)))
            mg.see_ll(float(abs(gain - LD(TOL))), ll_bound(M, N, R, ll_abs), ll_abs)
            if gain < TOL:
                break
    # the z that decides came from the m of the iteration before the last; the last m has the same magnitudes to first order
    mg.see_z(float(np.min(np.abs(1 - 2 * z))), z_bound(M, N, (np.abs(m0) + np.abs(m1)).astype(np.float64), D))
    return z


def phase_region(AD, DP, ref_idx, pos):
    """One region.  AD, DP: cell x SNP integer counts of the enabled cells (AD on the REF allele); ref_idx: haplotype index of
    every SNP's REF allele now; pos: positions.  -> (kept: bool per SNP, flip: int per KEPT SNP or None, Margins)."""
    AD, DP = np.asarray(AD, dtype=np.int64), np.asarray(DP, dtype=np.int64)
    mg = Margins()
    kept = DP.sum(axis=0) > 0
    cells = DP.sum(axis=1) > 0
    AD, DP = AD[np.ix_(cells, kept)], DP[np.ix_(cells, kept)]
    pos = np.asarray(pos, dtype=np.int64)[kept]
    if AD.shape[0] == 0:
        return kept, None, mg
    swap = np.asarray(ref_idx)[kept] == 1
    AD = np.where(swap[None, :], DP - AD, AD)
    total = np.zeros(AD.shape[1], dtype=bool)
    for rnd in range(RND_MAX_ITER):
        baf = AD.sum(axis=1) / DP.sum(axis=1)                            # float64, as on both sides
        keep = (baf < LOW_BAF) | (baf > UP_BAF)
        AD, DP = AD[keep], DP[keep]
        if AD.shape[0] == 0:
            return kept, None, mg
        if (DP.sum(axis=0) == 0).any():
            mg.nan_round = 1
            break
        mg.rounds += 1
        z = _em(AD.T.copy(), DP.T.copy(), pos, mg)
        flip = (1 - z) >= z
        total ^= flip
        if rnd >= RND_MIN_ITER and (flip.all() or not flip.any()):
            break
        AD = np.where(flip[None, :], DP - AD, AD)
    n_flip = int(total.sum())
    if n_flip / len(total) > 0.5:                                        # float64 division of two integers, as on both sides
        total = ~total
    return kept, total.astype(int), mg


def phase_slots(n_cells, col_ptr, cell, ad, dp, ref_hap, alt_hap, reg_ptr, slot_col, slot_snp, slot_pos, cell_enabled=None):
    """A whole xck_local_phase problem, region after region in order, the SNP state handed on.  -> the dict of capi.local_phase
    (kept, flip, status, ref_hap, alt_hap, n_levels) plus margins: one Margins per region, and decisive: bool per region."""
    col_ptr, cell, ad, dp = np.asarray(col_ptr, dtype=np.int64), np.asarray(cell, dtype=np.int64), np.asarray(ad, dtype=np.int64), np.asarray(dp, dtype=np.int64)
    reg_ptr, slot_col, slot_snp, slot_pos = np.asarray(reg_ptr, dtype=np.int64), np.asarray(slot_col, dtype=np.int64), np.asarray(slot_snp, dtype=np.int64), np.asarray(slot_pos, dtype=np.int64)
    ref_hap, alt_hap = np.array(ref_hap, dtype=np.int8), np.array(alt_hap, dtype=np.int8)
    on = np.ones(n_cells, dtype=bool) if cell_enabled is None else np.asarray(cell_enabled).astype(bool)
    n_regions, n_slots = len(reg_ptr) - 1, int(reg_ptr[-1])
    kept_all, flip_all = np.zeros(n_slots, dtype=np.uint8), np.zeros(n_slots, dtype=np.uint8)
    status, margins = np.zeros(n_regions, dtype=np.uint8), []
    level_of_snp, n_levels = {}, 0
    for r in range(n_regions):
        a, b = int(reg_ptr[r]), int(reg_ptr[r + 1])
        n = b - a
        AD, DP = np.zeros((n_cells, n), dtype=np.int64), np.zeros((n_cells, n), dtype=np.int64)
        for j in range(n):
            col = int(slot_col[a + j])
            if col >= 0:
                e = slice(int(col_ptr[col]), int(col_ptr[col + 1]))
                AD[cell[e], j], DP[cell[e], j] = ad[e], dp[e]
        snp = slot_snp[a:b]
        kept, flip, mg = phase_region(AD[on], DP[on], ref_hap[snp], slot_pos[a:b])
        margins.append(mg)
        kept_all[a:b] = kept
        if flip is not None:
            status[r] = 1
            flip_all[a:b][kept] = flip
            sel = snp[kept][flip == 1]
            ref_hap[sel], alt_hap[sel] = 1 - ref_hap[sel], 1 - alt_hap[sel]
        lv = max([level_of_snp.get(s, -1) for s in snp.tolist()], default=-1) + 1
        for s in snp.tolist():
            level_of_snp[s] = lv
        n_levels = max(n_levels, lv + 1)
    return dict(kept=kept_all, flip=flip_all, status=status, ref_hap=ref_hap, alt_hap=alt_hap, n_levels=n_levels,
                margins=margins, decisive=np.array([m.decisive for m in margins], dtype=bool))


def snps_decided(reg_ptr, slot_snp, decisive, n_snps):
    """bool per SNP: every region that holds the SNP is decisive (its final state is then the oracle's)."""
    ok = np.ones(n_snps, dtype=bool)
    for r in np.flatnonzero(~np.asarray(decisive)):
        ok[np.asarray(slot_snp)[int(reg_ptr[r]):int(reg_ptr[r + 1])]] = False
    return ok


def compare(args, exp, got, what="device"):
    """kept and status equal on every region; flip equal on every decisive region; the final state equal on every SNP all of whose
    regions are decisive; flip 0 wherever kept is 0.  -> indices of the non-decisive regions whose flips differ (reported)."""
    assert np.array_equal(got["kept"], exp["kept"]), "%s: kept differs at slots %s" % (what, np.flatnonzero(got["kept"] != exp["kept"])[:20])
    assert np.array_equal(got["status"], exp["status"]), "%s: status differs at regions %s" % (what, np.flatnonzero(got["status"] != exp["status"])[:20])
    assert not np.asarray(got["flip"])[np.asarray(got["kept"]) == 0].any(), "%s: a flip on a slot that is not kept" % what
    reg_ptr = args["reg_ptr"]
    bad, loose = [], []
    for r in range(len(reg_ptr) - 1):
        a, b = int(reg_ptr[r]), int(reg_ptr[r + 1])
        if not np.array_equal(got["flip"][a:b], exp["flip"][a:b]):
            (bad if exp["decisive"][r] else loose).append(r)
    assert not bad, "%s: flip differs from the oracle on decisive regions %s" % (what, bad)
    ok = snps_decided(reg_ptr, args["slot_snp"], exp["decisive"], len(exp["ref_hap"]))
    assert np.array_equal(np.asarray(got["ref_hap"])[ok], exp["ref_hap"][ok]) and np.array_equal(np.asarray(got["alt_hap"])[ok], exp["alt_hap"][ok]), "%s: final SNP state differs" % what
    return loose
