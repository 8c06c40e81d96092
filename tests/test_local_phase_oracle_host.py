"""The extended-precision oracle of local phasing (tests/local_phase_oracle.py) validated without a GPU: against the committed
fixture, against the float64 host path on the generated boundary sweep (tests/local_phase_cases.py), and on the hand-made edges.
tests/test_gpu_local_phase_edges.py then holds the device to the same oracle."""
import numpy as np
import pytest

import local_phase_cases as C
import local_phase_oracle as O
import local_phase_util as U
from xcltk_amd.baf.fc.phasing_dev import host_phase_slots

MAX_NON_DECISIVE = 0.15


def test_the_oracle_runs_in_extended_precision():
    assert np.finfo(np.longdouble).eps < 1e-18


@pytest.mark.parametrize("name", U.problem_names())
def test_oracle_reproduces_the_fixture(name):
    """kept / status everywhere, flip on every decisive region, the final state, the levels: the committed answers of the host path."""
    args, exp = U.load_problem(name)
    o = C.solved("fixture/" + name, args)
    loose = O.compare(args, o, exp, "fixture")
    print("%s: %d regions, non-decisive %s, of these the fixture differs on %s" % (name, len(exp["names"]), np.flatnonzero(~o["decisive"]).tolist(), loose))
    assert o["n_levels"] == exp["n_levels"]
    if name != "synthetic":
        assert o["decisive"].all(), "the fixture's hand-made regions are decisive"


def _sweeps():
    return [("sweep",) + C.sweep_problem(), ("overlap",) + C.overlap_problem()]


def test_sweep_holds_every_size_and_is_mostly_decisive():
    """A condition on the generator, met by the reference alone: at most 15 % of the sweep's regions are non-decisive."""
    sizes_n, sizes_m, n, n_dec = set(), set(), 0, 0
    for key, p, names in _sweeps():
        o = C.solved(key, p)
        n += len(names); n_dec += int(o["decisive"].sum())
        for r, name in enumerate(names):
            a, b = int(p["reg_ptr"][r]), int(p["reg_ptr"][r + 1])
            sizes_n.add(int(o["kept"][a:b].sum()))
            e = np.concatenate([np.arange(p["col_ptr"][c], p["col_ptr"][c + 1]) for c in p["slot_col"][a:b]])
            sizes_m.add(len(np.unique(p["cell"][e][p["dp"][e] > 0])))
            m = o["margins"][r]
            if not m.decisive:
                print("non-decisive %s: z %.3g (bound %.3g), stop rule %.3g (bound %.3g)" % (name, m.z, m.z_bound, m.ll, m.ll_bound))
    assert set(C.SIZES) <= sizes_n and set(C.SIZES) <= sizes_m, (sorted(sizes_n), sorted(sizes_m))
    print("%d of %d regions decisive" % (n_dec, n))
    assert n - n_dec <= MAX_NON_DECISIVE * n


def _host_without_nan_rounds(p, o):
    """host_phase_slots over the problem, except that a region the oracle ends in a NaN round is not run (the host iterates 6 x 1000
    times over NaN there, half a minute for 256 SNPs): such a region flips nothing, so the state passes it unchanged, and the
    runs of regions between them are separate calls.  -> (host answer with the oracle's entries for the skipped regions, skipped)"""
    skip = [r for r, m in enumerate(o["margins"]) if m.nan_round]
    got = dict(kept=o["kept"].copy(), flip=o["flip"].copy(), status=o["status"].copy())
    ref, alt = p["ref_hap"], p["alt_hap"]
    n_regions = len(p["reg_ptr"]) - 1
    for lo, hi in zip([-1] + skip, skip + [n_regions]):
        regs = list(range(lo + 1, hi))
        if not regs:
            continue
        h = host_phase_slots(**C.subproblem(p, regs, ref, alt))
        a, b = int(p["reg_ptr"][regs[0]]), int(p["reg_ptr"][hi])
        got["kept"][a:b], got["flip"][a:b], got["status"][regs[0]:hi] = h["kept"], h["flip"], h["status"]
        ref, alt = h["ref_hap"], h["alt_hap"]
    got["ref_hap"], got["alt_hap"] = ref, alt
    return got, skip


@pytest.mark.parametrize("which", [0, 1])
def test_host_path_equals_the_oracle_on_the_sweep(which):
    key, p, names = _sweeps()[which]
    o = C.solved(key, p)
    h, skipped = _host_without_nan_rounds(p, o)
    assert len(skipped) <= 2 and all(o["status"][r] == 1 and not o["flip"][int(p["reg_ptr"][r]):int(p["reg_ptr"][r + 1])].any() for r in skipped)
    loose = O.compare(p, o, h, "host path")
    print("%s: NaN-round regions not run on the host %s; non-decisive regions where the host differs %s" % (key, [names[r] for r in skipped], [names[r] for r in loose]))


def test_stop_rule_regions_depend_on_the_stop_rule(monkeypatch):
    """Decisive, the host path agrees - and the oracle with another tolerance or another minimum of iterations flips other SNPs,
    so a device with either constant wrong cannot pass on these regions."""
    p, names = C.stop_rule_problem()
    o = C.solved("stop_rule", p)
    assert o["decisive"].all() and o["status"].all() and not any(m.nan_round for m in o["margins"])
    assert O.compare(p, o, host_phase_slots(**p), "host path") == []
    changed = {}
    for what, name, value in (("tol", "TOL", 1e-2), ("min_iter", "EM_MIN_ITER", 5)):
        with monkeypatch.context() as mp:
            mp.setattr(O, name, value)
            other = O.phase_slots(**p)
        changed[what] = [not np.array_equal(other["flip"][a:b], o["flip"][a:b]) for a, b in zip(p["reg_ptr"][:-1], p["reg_ptr"][1:])]
    for r, name in enumerate(names):
        wants = C.STOP_RULE_SEEDS[int(name.split("_")[0][4:])].split("+")
        assert all(changed[w][r] for w in wants), (name, changed["tol"][r], changed["min_iter"][r])


@pytest.mark.parametrize("name", sorted(C.edge_problems()))
def test_edges_are_decisive_and_the_host_path_answers_as_listed(name):
    p, want = C.edge_problems()[name]
    o = C.solved("edge/" + name, p)
    assert o["decisive"].all()
    h = host_phase_slots(**p)
    assert O.compare(p, o, h, "host path") == []
    for k, v in want.items():
        assert h[k].tolist() == v and o[k].tolist() == v, (k, h[k], o[k])
    ref, alt = C.state_after_flips(p, o["flip"])
    assert np.array_equal(o["ref_hap"], ref) and np.array_equal(o["alt_hap"], alt)


def test_edges_show_what_they_are_named_for():
    E = C.edge_problems()
    o = C.solved("edge/empty_between", E["empty_between"][0])
    assert o["status"].tolist() == [1, 0, 1] and o["kept"].all()
    z, d = C.solved("edge/stored_zero_depth", E["stored_zero_depth"][0]), C.solved("edge/dropped_zero_depth", E["dropped_zero_depth"][0])
    pz, pd = E["stored_zero_depth"][0], E["dropped_zero_depth"][0]
    assert len(pz["dp"]) > len(pd["dp"]) and (pz["dp"] == 0).sum() == len(pz["dp"]) - len(pd["dp"]) and (pd["dp"] > 0).all()
    c2 = slice(int(pz["col_ptr"][2]), int(pz["col_ptr"][3]))
    assert len(pz["dp"][c2]) == 3 and not pz["dp"][c2].any()                # a column that is not empty, and has no depth
    assert not pz["dp"][pz["cell"] == 11].any() and (pz["cell"] == 11).sum() == 10   # a cell of nothing else
    covered = np.isin(pz["cell"], pd["cell"])
    assert ((pz["dp"] == 0) & covered).sum() >= 10                          # and zeros inside the lists of cells that have depth
    for k in ("kept", "flip", "status", "ref_hap", "alt_hap"):
        assert np.array_equal(z[k], d[k])
    p = E["shared_column"][0]
    assert p["slot_col"].tolist() == [0, 1, 2, 2, 3, 4] and p["slot_snp"].tolist() == [0, 1, 2, 3, 4, 5]
    p = E["disabled_only_depth"][0]
    with_cell = O.phase_slots(**dict(p, cell_enabled=None))
    assert with_cell["kept"].all()


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5), (5, 4, 3, 2, 1, 0)])
def test_slice_reuse_regions_are_decisive_and_what_they_are_named_for(order):
    p = C.slice_reuse_problem(order)
    o = C.solved("reuse/%s" % (order,), p)
    assert o["decisive"].all()
    by_name = {C.slice_reuse_regions()[i][0]: r for r, i in enumerate(order)}
    mg, st = o["margins"], o["status"]
    assert st[by_name["wide_257x300"]] == 1 and mg[by_name["wide_257x300"]].rounds >= 1
    assert st[by_name["failed"]] == 0 and st[by_name["no_cell_with_depth"]] == 0 and st[by_name["empty"]] == 0
    assert st[by_name["nan_round"]] == 1 and mg[by_name["nan_round"]].nan_round
    assert st[by_name["two_snps_three_cells"]] == 1
    r = by_name["no_cell_with_depth"]
    assert not o["kept"][int(p["reg_ptr"][r]):int(p["reg_ptr"][r + 1])].any()
    if order[0] == 0:
        assert O.compare(p, o, host_phase_slots(**p), "host path") == []
