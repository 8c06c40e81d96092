#!/usr/bin/env python
"""make_local_phase_fixture.py - writes tests/golden/local_phase/fixture.npz (CPU only; takes a few minutes).

The fixture holds PROBLEMS for xck_local_phase (include/xck.h) with the answer of the host path (baf/fc/phasing.py through
phasing_dev.host_phase_slots): kept / flip per slot, status per region, the final haplotype indices, the number of levels, and
per region a STABLE flag - the host's answer is the same under three random permutations of the cells, which change nothing
but the order of the float sums.  tests/test_gpu_local_phase.py compares the device with it.

  synthetic   120 regions drawn with numpy seed 7: 40 / 150 / 400 cells, 2 / 3 / 7 / 20 / 64 / 65 / 130 SNPs, Poisson depth with
              lambda 0.3 / 1 / 3, a clone of 60 % of the cells with allelic ratio 0.1 / 0.25 / 0.4 on a random true phase, random
              ref_hap at entry, positions spread over 400 kb
  hand-made   small problems, one per edge of the algorithm (hand_made() below says what each one must show, and checks it on the host path)

Usage: python tools/make_local_phase_fixture.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from xcltk_amd.baf import localphase                                   # noqa: E402
from xcltk_amd.baf.fc import phasing                                   # noqa: E402
from xcltk_amd.baf.fc.phasing_dev import host_phase_slots              # noqa: E402

FIELDS = ("n_cells", "col_ptr", "cell", "ad", "dp", "cell_enabled", "ref_hap", "alt_hap", "reg_ptr", "slot_col", "slot_snp", "slot_pos")
MIN_STABLE = 0.95


def dense_problem(regions, n_cells, cell_enabled=None, n_snps=None, ref_hap=None):
    """regions: [(AD, DP: cell x SNP dense, snp indices, positions)]; every region gets pileup columns of its own (a column of
    None data = slot without a column).  ref_hap: per SNP of the phased list."""
    col_ptr, cell, ad, dp, reg_ptr, slot_col, slot_snp, slot_pos = [0], [], [], [], [0], [], [], []
    for AD, DP, snp, pos in regions:
        AD, DP = np.asarray(AD), np.asarray(DP)
        for j in range(len(snp)):
            if j < DP.shape[1]:
                c = np.flatnonzero(DP[:, j] > 0)
                cell += c.tolist(); ad += AD[c, j].tolist(); dp += DP[c, j].tolist()
                slot_col.append(len(col_ptr) - 1)
                col_ptr.append(len(cell))
            else:
                slot_col.append(-1)
            slot_snp.append(int(snp[j])); slot_pos.append(int(pos[j]))
        reg_ptr.append(len(slot_col))
    n_snps = n_snps if n_snps is not None else max(slot_snp) + 1
    ref_hap = np.zeros(n_snps, dtype=np.int8) if ref_hap is None else np.asarray(ref_hap, dtype=np.int8)
    return dict(n_cells=n_cells, col_ptr=np.array(col_ptr, dtype=np.int64), cell=np.array(cell, dtype=np.int32), ad=np.array(ad, dtype=np.int32),
                dp=np.array(dp, dtype=np.int32), cell_enabled=None if cell_enabled is None else np.asarray(cell_enabled, dtype=np.uint8),
                ref_hap=ref_hap, alt_hap=(1 - ref_hap).astype(np.int8), reg_ptr=np.array(reg_ptr, dtype=np.int64),
                slot_col=np.array(slot_col, dtype=np.int32), slot_snp=np.array(slot_snp, dtype=np.int32), slot_pos=np.array(slot_pos, dtype=np.int64))


def draw_region(rs, n_cells, n_snps, lam, ratio):
    """One synthetic region: -> (AD on the REF allele, DP, ref_hap at entry, positions)."""
    DP = rs.poisson(lam, size=(n_cells, n_snps))
    phase = rs.randint(0, 2, size=n_snps)                                # true haplotype of the REF allele
    clone = rs.permutation(n_cells) < int(round(0.6 * n_cells))
    p_hap0 = np.where(clone, ratio, 0.5)                                 # share of haplotype 0 in the cell's reads
    p_ref = np.where(phase[None, :] == 0, p_hap0[:, None], 1 - p_hap0[:, None])
    AD = rs.binomial(DP, p_ref)
    ref_hap = rs.randint(0, 2, size=n_snps)
    pos = np.sort(rs.choice(np.arange(1, 400001), size=n_snps, replace=False)) + 1000000
    return AD, DP, ref_hap, pos


def synthetic(seed=7, n_regions=120):
    rs = np.random.RandomState(seed)
    regions, ref_hap, names, s = [], [], [], 0
    for r in range(n_regions):
        n_cells, n_snps = int(rs.choice([40, 150, 400])), int(rs.choice([2, 3, 7, 20, 64, 65, 130]))
        lam, ratio = float(rs.choice([0.3, 1, 3])), float(rs.choice([0.1, 0.25, 0.4]))
        AD, DP, rh, pos = draw_region(rs, n_cells, n_snps, lam, ratio)
        A = np.zeros((400, n_snps), dtype=np.int64); D = np.zeros((400, n_snps), dtype=np.int64)
        A[:n_cells], D[:n_cells] = AD, DP
        regions.append((A, D, np.arange(s, s + n_snps), pos))
        ref_hap += rh.tolist()
        names.append("syn%03d_c%d_s%d_l%g_r%g" % (r, n_cells, n_snps, lam, ratio))
        s += n_snps
    return dense_problem(regions, 400, n_snps=s, ref_hap=ref_hap), names


def counted_host(p, **kw):
    """host_phase_slots plus the number of EM calls per region."""
    calls, per_region = [0], []
    em = localphase.em_two_haplotypes
    reg = phasing.reg_local_phasing

    def em_counted(*a, **k):
        calls[0] += 1
        return em(*a, **k)

    def reg_counted(*a, **k):
        calls[0] = 0
        out = reg(*a, **k)
        per_region.append(calls[0])
        return out
    localphase.em_two_haplotypes, phasing.reg_local_phasing = em_counted, reg_counted
    try:
        return host_phase_slots(**dict(p, **kw)), per_region
    finally:
        localphase.em_two_haplotypes, phasing.reg_local_phasing = em, reg


def hand_made():
    """-> {name: (problem, region names)}; every problem is checked to show what its name says."""
    out = {}
    P1, P2 = [1000100, 1060000], [1000100, 1030000, 1060000]
    # cells at exactly 9/20 and 11/20 (18/40, 33/60) leave: alone they leave nothing (failed); cells at 8/20 and 12/20 stay
    tie_dp = np.array([[10, 10], [10, 10], [20, 20], [30, 30]])
    tie_ad = np.array([[4, 5], [6, 5], [9, 9], [20, 13]])
    edge_dp = np.array([[10, 10], [10, 10], [10, 10]])
    edge_ad = np.array([[4, 4], [6, 6], [7, 5]])
    p = dense_problem([(tie_ad, tie_dp, [0, 1], P1), (edge_ad, edge_dp, [2, 3], P1)], 4)
    h, calls = counted_host(p)
    assert h["status"].tolist() == [0, 1] and calls[0] == 0, (h, calls)
    out["baf_ties"] = (p, ["ties_9_11_of_20", "edge_8_12_of_20"])
    # every cell filtered in round 0 / in a later round -> failed, nothing flipped
    # (later round: SNP 0 lies alone and flips; SNPs 1-3 lie within 100 bp, where the smoothing lets the two weak ones outvote the strong
    # one, so nothing flips there; after the flip both cells have BAF 42/82 and 21/42)
    later = dense_problem([(np.array([[0, 0, 3, 3], [0, 0, 2, 2]]), np.array([[36, 40, 3, 3], [18, 20, 2, 2]]), [0, 1, 2, 3], [1000100, 1100000, 1100050, 1100100])], 2)
    h, calls = counted_host(later)
    assert h["status"][0] == 0 and calls[0] == 1 and not h["flip"].any(), (h, calls)
    out["filtered_later_round"] = (later, ["all_cells_filtered_in_a_later_round"])
    p = dense_problem([(np.array([[5, 5], [3, 3]]), np.array([[10, 10], [6, 6]]), [0, 1], P1)], 2)
    h, calls = counted_host(p)
    assert h["status"][0] == 0 and calls[0] == 0 and h["kept"].tolist() == [1, 1]
    out["filtered_round0"] = (p, ["all_cells_filtered_in_round_0"])
    # NaN: SNP 2 has depth only in a cell with BAF 0.5 -> Z is NaN, 6 EM calls, flip all 0
    dp = np.array([[6, 6, 0], [5, 7, 0], [8, 4, 0], [2, 0, 2]]); ad = np.array([[6, 0, 0], [5, 1, 0], [1, 4, 0], [1, 0, 1]])
    p = dense_problem([(ad, dp, [0, 1, 2], P2)], 4)
    h, calls = counted_host(p)
    assert h["status"][0] == 1 and calls[0] == 6 and h["flip"].tolist() == [0, 0, 0] and h["kept"].tolist() == [1, 1, 1], (h, calls)
    out["nan_snp"] = (p, ["snp_loses_all_depth"])
    # majority rule: two of three SNPs flip in the EM, so the rule inverts the vector
    dp = np.full((4, 3), 10); ad = np.array([[1, 1, 9], [0, 2, 10], [2, 1, 8], [9, 9, 1]])
    p = dense_problem([(ad, dp, [0, 1, 2], P2)], 4)
    h, _ = counted_host(p)
    raw = localphase.snp_local_phasing(ad, dp, np.array(P2))
    assert raw.tolist() == [True, True, False] and h["flip"].tolist() == [0, 0, 1], (raw, h)
    out["majority_inverts"] = (p, ["majority_inverts"])
    # a SNP without depth in the enabled cells leaves the list; cell_enabled removes the cell that would decide the phase
    dp = np.array([[10, 10, 0], [10, 10, 0], [0, 0, 5], [60, 40, 0]]); ad = np.array([[9, 8, 0], [8, 9, 0], [0, 0, 4], [3, 40, 0]])
    p_on = dense_problem([(ad, dp, [0, 1, 2], P2)], 4)
    p = dense_problem([(ad, dp, [0, 1, 2], P2)], 4, cell_enabled=[1, 1, 0, 0])
    h_on, _ = counted_host(p_on)
    h, _ = counted_host(p)
    assert h["kept"].tolist() == [1, 1, 0] and h_on["kept"].tolist() == [1, 1, 1] and h["flip"].tolist() != h_on["flip"].tolist(), (h, h_on)
    out["cell_enabled"] = (p, ["uncovered_snp_and_disabled_decider"])
    # two SNPs, the minimum; ref_hap = 1 at entry on one of them
    dp = np.full((3, 2), 8); ad = np.array([[7, 1], [8, 0], [1, 6]])
    p = dense_problem([(ad, dp, [0, 1], P1)], 3, ref_hap=[0, 1])
    out["two_snps"] = (p, ["two_snps"])
    # 257 SNPs x 300 cells: more than one block's threads either way
    rs = np.random.RandomState(13)
    AD, DP, rh, pos = draw_region(rs, 300, 257, 1.0, 0.2)
    out["wide_257x300"] = (dense_problem([(AD, DP, np.arange(257), pos)], 300, ref_hap=rh), ["snps257_cells300"])
    # three overlapping regions in a chain (A: SNPs 0-3, B: 2-6, C: 5-9), a duplicate of C, and an independent region: levels 0 1 2 3 0
    rs = np.random.RandomState(17)
    AD, DP, rh, pos = draw_region(rs, 60, 14, 3.0, 0.15)
    sets = [np.arange(0, 4), np.arange(2, 7), np.arange(5, 10), np.arange(5, 10), np.arange(10, 14)]
    p = dense_problem([(AD[:, s], DP[:, s], s, pos[s]) for s in sets], 60, n_snps=14, ref_hap=rh)
    h, _ = counted_host(p)
    assert h["n_levels"] == 4
    out["chain_and_duplicate"] = (p, ["chain_a", "chain_b", "chain_c", "duplicate_of_c", "independent"])
    # a list longer than the pileup: the last two slots have no column
    AD, DP, rh, pos = draw_region(rs, 30, 6, 3.0, 0.2)
    p = dense_problem([(AD[:, :4], DP[:, :4], np.arange(6), pos)], 30, ref_hap=rh)
    h, _ = counted_host(p)
    assert p["slot_col"].tolist()[4:] == [-1, -1] and h["kept"].tolist()[4:] == [0, 0]
    out["short_pileup"] = (p, ["slots_without_column"])
    return out


def solve(p, names, n_perm=3, seed=23):
    h = host_phase_slots(**p)
    rs = np.random.RandomState(seed)
    n_rows = p["n_cells"] if p["cell_enabled"] is None else int(np.sum(p["cell_enabled"]))
    stable = np.ones(len(names), dtype=np.uint8)
    for _ in range(n_perm):
        g = host_phase_slots(cell_perm=rs.permutation(n_rows), **p)
        for r in range(len(names)):
            a, b = int(p["reg_ptr"][r]), int(p["reg_ptr"][r + 1])
            if g["status"][r] != h["status"][r] or not np.array_equal(g["kept"][a:b], h["kept"][a:b]) or not np.array_equal(g["flip"][a:b], h["flip"][a:b]):
                stable[r] = 0
    return h, stable


def main(out_fn):
    problems = dict(hand_made())
    problems["synthetic"] = synthetic()
    arrays, n_regions, n_stable = {"problems": np.array(sorted(problems), dtype="U64")}, 0, 0
    for name in sorted(problems):
        p, names = problems[name]
        h, stable = solve(p, names)
        n_regions += len(names); n_stable += int(stable.sum())
        print("%-24s regions=%d stable=%d failed=%d flipped=%d levels=%d" % (name, len(names), int(stable.sum()), int(np.sum(h["status"] == 0)), int(h["flip"].sum()), h["n_levels"]))
        for k in FIELDS:
            v = p[k]
            arrays[name + "/" + k] = np.zeros(0, dtype=np.uint8) if v is None else np.asarray(v)
        arrays[name + "/has_cell_enabled"] = np.array(p["cell_enabled"] is not None)
        arrays[name + "/names"] = np.array(names, dtype="U64")
        arrays[name + "/stable"] = stable
        for k in ("kept", "flip", "status", "ref_hap", "alt_hap"):
            arrays[name + "/exp_" + k] = h[k]
        arrays[name + "/exp_n_levels"] = np.array(h["n_levels"])
        # the smallest types that hold the values keep the file small
        arrays[name + "/cell"] = arrays[name + "/cell"].astype(np.uint16); arrays[name + "/ad"] = arrays[name + "/ad"].astype(np.uint8); arrays[name + "/dp"] = arrays[name + "/dp"].astype(np.uint8)
    assert n_stable >= MIN_STABLE * n_regions, "only %d of %d regions are stable" % (n_stable, n_regions)
    os.makedirs(os.path.dirname(out_fn), exist_ok=True)
    np.savez_compressed(out_fn, **arrays)
    print("%s: %d regions, %d stable, %d bytes" % (out_fn, n_regions, n_stable, os.path.getsize(out_fn)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "local_phase", "fixture.npz"))
