"""Generated problems for xck_local_phase at the sizes where csrc/local_phase.hip changes its path, and hand-made edges.

Everything is built from seeds at call time and cached; nothing is read from a file.  The sweep holds two regions for every
number of kept SNPs N and every number of cells with depth M in SIZES: pow2_group() halves the lanes per item at 1|2, 2|3, 4|5,
8|9, ... 128|129 items (at 129 SNPs the weight matrix turns to its transposed layout), block_scan2() goes from one item per thread
to two at 256|257, and with XCK_PHASE_WCAP=16 / XCK_PHASE_LDS_SNPS=16 the stored weights and the LDS state end at 16|17 SNPs.
"""
import numpy as np

SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257)
RATIOS = (0.1, 0.25, 0.4)
SWEEP_SEED = 20
N_CELLS = 300
_cache = {}


def draw_region(rs, n_cells, n_snps, lam, ratio):
    """One synthetic region as tools/make_local_phase_fixture.py draws it: -> (AD on the REF allele, DP, ref_hap at entry,
    positions).  A clone of 60 % of the cells has allelic ratio `ratio` on a random true phase; positions spread over 400 kb."""
    DP = rs.poisson(lam, size=(n_cells, n_snps))
    phase = rs.randint(0, 2, size=n_snps)
    clone = rs.permutation(n_cells) < int(round(0.6 * n_cells))
    p_hap0 = np.where(clone, ratio, 0.5)
    p_ref = np.where(phase[None, :] == 0, p_hap0[:, None], 1 - p_hap0[:, None])
    AD = rs.binomial(DP, p_ref)
    ref_hap = rs.randint(0, 2, size=n_snps)
    pos = np.sort(rs.choice(np.arange(1, 400001), size=n_snps, replace=False)) + 1000000
    return AD, DP, ref_hap, pos


def columns_of(AD, DP, stored=None):
    """Pileup columns [(cells, ad, dp)] of dense cell x SNP counts; stored: which entries the CSC holds (default: depth > 0)."""
    AD, DP = np.asarray(AD), np.asarray(DP)
    stored = DP > 0 if stored is None else np.asarray(stored, dtype=bool)
    return [(np.flatnonzero(stored[:, j]), AD[stored[:, j], j], DP[stored[:, j], j]) for j in range(DP.shape[1])]


def make_problem(columns, regions, n_cells, ref_hap, cell_enabled=None):
    """columns: [(cells, ad, dp)]; regions: [(slot_col, slot_snp, slot_pos)]; -> the arguments of capi.local_phase."""
    col_ptr = np.concatenate([[0], np.cumsum([len(c[0]) for c in columns])]).astype(np.int64)
    cat = lambda k, dt: np.concatenate([np.asarray(c[k]) for c in columns]).astype(dt) if columns else np.zeros(0, dtype=dt)
    rcat = lambda k, dt: np.concatenate([np.asarray(r[k], dtype=dt) for r in regions]).astype(dt) if regions else np.zeros(0, dtype=dt)
    ref_hap = np.asarray(ref_hap, dtype=np.int8)
    return dict(n_cells=n_cells, col_ptr=col_ptr, cell=cat(0, np.int32), ad=cat(1, np.int32), dp=cat(2, np.int32),
                ref_hap=ref_hap, alt_hap=(1 - ref_hap).astype(np.int8),
                reg_ptr=np.concatenate([[0], np.cumsum([len(r[0]) for r in regions])]).astype(np.int64),
                slot_col=rcat(0, np.int32), slot_snp=rcat(1, np.int32), slot_pos=rcat(2, np.int64),
                cell_enabled=None if cell_enabled is None else np.asarray(cell_enabled, dtype=np.uint8))


def from_dense(regions, n_cells, cell_enabled=None, order=None):
    """regions: [(AD, DP, ref_hap, pos)] (cell x SNP, n_cells rows), every region with SNPs and columns of its own, laid out in
    `order` (default: as given).  -> problem"""
    order = list(range(len(regions))) if order is None else list(order)
    columns, regs, ref_hap = [], [], []
    for i in order:
        AD, DP, rh, pos = regions[i]
        n = len(pos)
        cols = columns_of(AD, DP)
        regs.append((np.arange(len(columns), len(columns) + n), np.arange(len(ref_hap), len(ref_hap) + n), pos))
        columns += cols
        ref_hap += np.asarray(rh).tolist()
    return make_problem(columns, regs, n_cells, ref_hap, cell_enabled)


def _scatter(rs, AD, DP, n_cells):
    """The region's cells on random rows of a table of n_cells."""
    rows = np.sort(rs.choice(n_cells, size=AD.shape[0], replace=False))
    A, D = np.zeros((n_cells, AD.shape[1]), dtype=np.int64), np.zeros((n_cells, AD.shape[1]), dtype=np.int64)
    A[rows], D[rows] = AD, DP
    return A, D


def _cover(AD, DP, axis):
    """Give every row (axis 1) or column (axis 0) without depth one REF read in its first entry, so that the count is exact."""
    AD, DP = AD.copy(), DP.copy()
    if axis == 1:
        z = DP.sum(axis=1) == 0
        DP[z, 0], AD[z, 0] = 1, 1
    else:
        z = DP.sum(axis=0) == 0
        DP[0, z], AD[0, z] = 1, 1
    return AD, DP


def sweep_regions():
    """-> [(name, AD, DP, ref_hap, pos)] on N_CELLS rows: the SNP sweep, then the cell sweep."""
    if "regions" not in _cache:
        rs = np.random.RandomState(SWEEP_SEED)
        out = []
        for n in SIZES:                                                  # kept SNPs, lambda 3
            # over many SNPs of random phase a cell's BAF tends to 0.5 and the filter drops it: large N needs many cells for a few
            # to stay, otherwise every such region ends in a NaN round before its first EM
            for rep, n_cells in enumerate((40, 60) if n < 128 else (100, 200)):
                ratio = RATIOS[(SIZES.index(n) + rep) % 3]
                AD, DP, rh, pos = draw_region(rs, n_cells, n, 3.0, ratio)
                AD, DP = _cover(AD, DP, 0)
                AD, DP = _cover(AD, DP, 1)
                out.append(("snps%d_cells%d_r%g" % (n, n_cells, ratio),) + _scatter(rs, AD, DP, N_CELLS) + (rh, pos))
        for m in SIZES:                                                  # cells with depth, at small N
            for rep, n in enumerate((4, 7)):
                ratio = RATIOS[(SIZES.index(m) + rep + 1) % 3]
                AD, DP, rh, pos = draw_region(rs, m, n, 3.0, ratio)
                AD, DP = _cover(AD, DP, 1)
                out.append(("cells%d_snps%d_r%g" % (m, n, ratio),) + _scatter(rs, AD, DP, N_CELLS) + (rh, pos))
        _cache["regions"] = out
    return _cache["regions"]


def sweep_problem():
    """All sweep regions in one problem, in shuffled order.  -> (problem, names in problem order)"""
    if "sweep" not in _cache:
        regs = sweep_regions()
        order = np.random.RandomState(SWEEP_SEED + 1).permutation(len(regs))
        p = from_dense([r[1:] for r in regs], N_CELLS, order=order)
        _cache["sweep"] = (p, [regs[i][0] for i in order])
    return _cache["sweep"]


def overlap_problem():
    """Windows of the sizes in SIZES over one strip of SNPs, consecutive windows sharing one to three SNPs: as many levels as
    windows, the SNP state handed from each to the next.  Every window has pileup columns of its own."""
    if "overlap" not in _cache:
        rs = np.random.RandomState(SWEEP_SEED + 2)
        sizes = [int(s) for s in rs.permutation(SIZES)]
        total = sum(sizes)
        AD, DP, rh, pos = draw_region(rs, 150, total, 3.0, 0.25)
        AD, DP = _scatter(rs, AD, DP, N_CELLS)
        columns, regs, names, start = [], [], [], 0
        for i, n in enumerate(sizes):
            if i:
                start -= min(1 + i % 3, n, sizes[i - 1])
            snp = np.arange(start, start + n)
            regs.append((np.arange(len(columns), len(columns) + n), snp, pos[snp]))
            columns += columns_of(AD[:, snp], DP[:, snp])
            names.append("window%d_at%d" % (n, start))
            start += n
        _cache["overlap"] = (make_problem(columns, regs, N_CELLS, rh), names)
    return _cache["overlap"]


STOP_RULE_SEEDS = {129: "tol+min_iter", 246: "tol", 261: "tol", 135: "min_iter", 214: "min_iter"}


def stop_rule_problem():
    """Regions whose answer the EM's stop rule decides.  In the sweep almost every EM has converged when the rule is first looked
    at, so a wrong tolerance or a wrong minimum of iterations would change no flip there.  These five were picked with the oracle
    alone from shallow draws (lambda 0.3 or 1): with TOL = 1e-2 (tol) or EM_MIN_ITER = 5 (min_iter) the oracle flips other SNPs,
    and tests/test_local_phase_oracle_host.py keeps that true.  -> (problem, names)"""
    if "stop_rule" not in _cache:
        regs, names = [], []
        for seed, what in STOP_RULE_SEEDS.items():
            rs = np.random.RandomState(seed)
            n_cells, n = int(rs.choice([40, 80, 150])), int(rs.choice([7, 20, 40]))
            lam, ratio = float(rs.choice([0.3, 1.0])), float(rs.choice([0.1, 0.25, 0.4]))
            AD, DP, rh, pos = draw_region(rs, n_cells, n, lam, ratio)
            regs.append(_scatter(rs, AD, DP, N_CELLS) + (rh, pos))
            names.append("seed%d_cells%d_snps%d_l%g_r%g_%s" % (seed, n_cells, n, lam, ratio, what))
        _cache["stop_rule"] = (from_dense(regs, N_CELLS), names)
    return _cache["stop_rule"]


# ---- hand-made edges ------------------------------------------------------------------------------------------------------------

P3 = [1000100, 1030000, 1060000]


def _small(seed, n_cells, n_snps, lam=3.0, ratio=0.15):
    AD, DP, rh, pos = draw_region(np.random.RandomState(seed), n_cells, n_snps, lam, ratio)
    return AD, DP, rh, pos


def edge_problems():
    """-> {name: (problem, expected: dict of what the host path answers, checked by the CPU test)}"""
    if "edges" in _cache:
        return _cache["edges"]
    out = {}
    AD, DP, rh, pos = _small(31, 4, 3)
    AD, DP = _cover(AD, DP, 0)
    p = from_dense([(AD, DP, rh, pos)], 4, cell_enabled=[0, 0, 0, 0])
    out["all_cells_disabled"] = (p, dict(kept=[0, 0, 0], status=[0], flip=[0, 0, 0]))
    # slots without a column and a pileup without columns
    p = make_problem([], [([-1, -1, -1], [0, 1, 2], P3)], 4, [0, 1, 0])
    out["no_columns"] = (p, dict(kept=[0, 0, 0], status=[0], flip=[0, 0, 0]))
    # an empty region between two normal ones
    a, b = _small(32, 20, 5), _small(33, 20, 6)
    cols = columns_of(a[0], a[1]) + columns_of(b[0], b[1])
    p = make_problem(cols, [(np.arange(5), np.arange(5), a[3]), ([], [], []), (np.arange(5, 11), np.arange(5, 11), b[3])], 20, np.concatenate([a[2], b[2]]))
    out["empty_between"] = (p, dict(status=[1, 0, 1]))
    # one SNP
    AD, DP, rh, pos = _small(34, 12, 1)
    p = from_dense([(AD, DP, [1], pos)], 12)
    out["one_snp"] = (p, dict(kept=[1], status=[1], flip=[0]))
    # dp == 0 entries kept in the CSC: every second place without depth is stored (the cell-major lists must skip them), column 2
    # holds nothing else (kept 0, although the column is not empty), cell 11 holds nothing else; the same data with the zeros dropped
    rs = np.random.RandomState(35)
    AD, DP, rh, pos = draw_region(rs, 12, 10, 1.0, 0.15)
    DP[:, 2], AD[:, 2] = 0, 0
    DP[11, :], AD[11, :] = 0, 0
    AD, DP = _cover(AD, DP, 1)
    DP[11, 0], AD[11, 0] = 0, 0
    stored = (DP > 0) | (rs.randint(0, 2, size=DP.shape) == 1)
    stored[:, 2] = False
    stored[[1, 4, 11], 2] = True
    stored[11, :] = True
    reg = [(np.arange(10), np.arange(10), pos)]
    kept = [int(j != 2) for j in range(10)]
    assert (DP.sum(axis=0) > 0).tolist() == [bool(k) for k in kept]
    out["stored_zero_depth"] = (make_problem(columns_of(AD, DP, stored), reg, 12, rh), dict(kept=kept, status=[1]))
    out["dropped_zero_depth"] = (make_problem(columns_of(AD, DP), reg, 12, rh), dict(kept=kept, status=[1]))
    # one pileup column used by two regions over different SNP indices
    AD, DP, rh, pos = _small(36, 25, 5)
    p = make_problem(columns_of(AD, DP), [([0, 1, 2], [0, 1, 2], pos[:3]), ([2, 3, 4], [3, 4, 5], pos[2:])], 25, np.concatenate([rh[:3], rh[2:]]))
    out["shared_column"] = (p, dict(status=[1, 1]))
    # cell_enabled switches off the one cell that holds a SNP's only depth, inside a larger region
    AD, DP, rh, pos = _small(37, 31, 20)
    DP[:, 11], AD[:, 11] = 0, 0
    DP[30, 11], AD[30, 11] = 9, 2
    en = np.ones(31, dtype=np.uint8)
    en[30] = 0
    p = from_dense([(AD, DP, rh, pos)], 31, cell_enabled=en)
    out["disabled_only_depth"] = (p, dict(kept=[int(j != 11) for j in range(20)], status=[1]))
    _cache["edges"] = out
    return out


def slice_reuse_regions():
    """The regions of the slice-reuse test on 300 cells, each (name, columns, slot_col relative to its columns, pos, ref_hap):
    257 SNPs x 300 cells, a failed region, a NaN-round region, a region whose cells are all without depth (M == 0), an empty
    region, two SNPs x three cells."""
    if "reuse" in _cache:
        return _cache["reuse"]
    pad = lambda A: np.vstack([np.asarray(A), np.zeros((N_CELLS - len(A), np.asarray(A).shape[1]), dtype=np.int64)])
    out = []
    AD, DP, rh, pos = draw_region(np.random.RandomState(41), N_CELLS, 257, 1.0, 0.2)
    out.append(("wide_257x300", columns_of(AD, DP), list(range(257)), pos, rh))
    out.append(("failed", columns_of(pad([[5, 5], [3, 3]]), pad([[10, 10], [6, 6]])), [0, 1], [1000100, 1060000], [0, 0]))
    dp = [[6, 6, 0], [5, 7, 0], [8, 4, 0], [2, 0, 2]]
    ad = [[6, 0, 0], [5, 1, 0], [1, 4, 0], [1, 0, 1]]
    out.append(("nan_round", columns_of(pad(ad), pad(dp)), [0, 1, 2], P3, [0, 0, 0]))
    zero = np.zeros((N_CELLS, 3), dtype=np.int64)
    stored = np.zeros((N_CELLS, 3), dtype=bool)
    stored[[3, 200], 0] = True
    stored[299, 2] = True
    out.append(("no_cell_with_depth", columns_of(zero, zero, stored), [0, 1, 2], P3, [1, 0, 1]))
    out.append(("empty", [], [], [], []))
    out.append(("two_snps_three_cells", columns_of(pad([[7, 1], [8, 0], [1, 6]]), pad(np.full((3, 2), 8))), [0, 1], [1000100, 1060000], [0, 1]))
    _cache["reuse"] = out
    return out


def slice_reuse_problem(order):
    """The regions of slice_reuse_regions() in `order` in one problem.  -> problem"""
    regs = slice_reuse_regions()
    columns, slots, ref_hap = [], [], []
    for i in order:
        _, cols, sc, pos, rh = regs[i]
        slots.append((np.asarray(sc, dtype=np.int64) + len(columns), np.arange(len(ref_hap), len(ref_hap) + len(sc)), pos))
        columns += cols
        ref_hap += list(np.asarray(rh).tolist())
    return make_problem(columns, slots, N_CELLS, ref_hap)


def subproblem(p, regions, ref_hap=None, alt_hap=None):
    """The problem with only `regions` (indices, in order) and, if given, another SNP state at entry; the pileup stays whole."""
    a, b = p["reg_ptr"][:-1], p["reg_ptr"][1:]
    sl = np.concatenate([np.arange(a[r], b[r]) for r in regions]).astype(np.int64) if len(regions) else np.zeros(0, dtype=np.int64)
    q = dict(p, reg_ptr=np.concatenate([[0], np.cumsum([b[r] - a[r] for r in regions])]).astype(np.int64),
             slot_col=p["slot_col"][sl], slot_snp=p["slot_snp"][sl], slot_pos=p["slot_pos"][sl])
    if ref_hap is not None:
        q["ref_hap"], q["alt_hap"] = np.asarray(ref_hap, dtype=np.int8), np.asarray(alt_hap, dtype=np.int8)
    return q


def state_after_flips(p, flip):
    """(ref_hap, alt_hap) at entry with every flipped slot's SNP swapped once per flip."""
    n = np.bincount(p["slot_snp"][np.asarray(flip) != 0], minlength=len(p["ref_hap"])) % 2
    return (p["ref_hap"] ^ n).astype(np.int8), (p["alt_hap"] ^ n).astype(np.int8)


def solved(key, problem):
    """The oracle's answer for a problem, computed once per process."""
    import local_phase_oracle as O
    if ("solved", key) not in _cache:
        _cache[("solved", key)] = O.phase_slots(**problem)
    return _cache[("solved", key)]
