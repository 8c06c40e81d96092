"""xck_local_phase (csrc/local_phase.hip) against the extended-precision oracle (tests/local_phase_oracle.py) where the kernel
changes its path and where its branches begin: the generated boundary sweep and the hand-made edges of tests/local_phase_cases.py.
kept / status are compared on every region, flip on every DECISIVE region (every float-decided step of the oracle has a margin
beyond what float64 summation order can move), the final SNP state wherever all of a SNP's regions are decisive.
tests/test_local_phase_oracle_host.py ties the oracle to the host path and to the committed fixture without a GPU."""
import numpy as np
import pytest

import local_phase_cases as C
import local_phase_oracle as O
from xcltk_amd import capi

pytestmark = pytest.mark.gpu

KEYS = ("kept", "flip", "status", "ref_hap", "alt_hap")
SWEEPS = {"sweep": C.sweep_problem, "overlap": C.overlap_problem, "stop_rule": C.stop_rule_problem}
_runs = {}


def default_run(which):
    """The sweep problem on the device with no knob set, once per process."""
    if which not in _runs:
        _runs[which] = capi.local_phase(**SWEEPS[which]()[0])
    return _runs[which]


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in KEYS) and a["n_levels"] == b["n_levels"]


def check(p, o, got):
    """The device's answer against the oracle's, and what holds for any answer: flip only where kept, a failed region flips
    nothing, and the final state is the state at entry with exactly the flipped slots swapped - no other SNP is touched."""
    loose = O.compare(p, o, got)
    assert got["n_levels"] == o["n_levels"]
    for r in np.flatnonzero(got["status"] == 0):
        assert not got["flip"][int(p["reg_ptr"][r]):int(p["reg_ptr"][r + 1])].any()
    ref, alt = C.state_after_flips(p, got["flip"])
    assert np.array_equal(got["ref_hap"], ref) and np.array_equal(got["alt_hap"], alt)
    return loose


@pytest.mark.parametrize("which", sorted(SWEEPS))
def test_boundary_sweep_equals_the_oracle(which):
    p, names = SWEEPS[which]()
    o = C.solved(which, p)
    got = default_run(which)
    loose = check(p, o, got)
    print("%s: non-decisive regions %s; of these the device differs on %s" % (which, [names[r] for r in np.flatnonzero(~o["decisive"])], [names[r] for r in loose]))
    if which == "overlap":
        assert got["n_levels"] == len(names)


@pytest.mark.parametrize("which", sorted(SWEEPS))
@pytest.mark.parametrize("knobs", [dict(XCK_PHASE_WCAP="16"), dict(XCK_PHASE_LDS_SNPS="16"), dict(XCK_PHASE_WCAP="16", XCK_PHASE_LDS_SNPS="16"),
                                   dict(XCK_PHASE_BLOCKS="1")], ids=lambda k: "+".join("%s=%s" % (a[10:], b) for a, b in k.items()))
def test_knob_boundaries_change_no_byte(which, knobs, monkeypatch):
    """The sweep holds 16 and 17 SNPs: with the limits at 16 the stored weights / the state in LDS end exactly there.  One workgroup
    walks every region of a level through one scratch slice."""
    base = default_run(which)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    got = capi.local_phase(**SWEEPS[which]()[0])
    if "XCK_PHASE_BLOCKS" in knobs:
        assert got["n_blocks"] == 1
    assert same_bytes(base, got)


@pytest.mark.parametrize("which", sorted(SWEEPS))
def test_second_call_returns_identical_bytes(which):
    assert same_bytes(default_run(which), capi.local_phase(**SWEEPS[which]()[0]))


@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5), (5, 4, 3, 2, 1, 0)], ids=["large_first", "small_first"])
def test_one_slice_serves_unlike_regions_in_turn(order, monkeypatch):
    """257 SNPs x 300 cells, a failed region, a NaN-round region, one without any cell with depth, an empty one, two SNPs x three
    cells - and the reverse - through ONE scratch slice: every region answers as it does alone, and as the oracle says."""
    regs = C.slice_reuse_regions()
    alone = [capi.local_phase(**C.slice_reuse_problem([i])) for i in range(len(regs))]
    monkeypatch.setenv("XCK_PHASE_BLOCKS", "1")
    p = C.slice_reuse_problem(order)
    got = capi.local_phase(**p)
    assert got["n_blocks"] == 1 and got["n_levels"] == 1
    check(p, C.solved("reuse/%s" % (order,), p), got)
    snp = 0
    for r, i in enumerate(order):
        a, b = int(p["reg_ptr"][r]), int(p["reg_ptr"][r + 1])
        one = alone[i]
        assert got["status"][r] == one["status"][0], regs[i][0]
        assert np.array_equal(got["kept"][a:b], one["kept"]) and np.array_equal(got["flip"][a:b], one["flip"]), regs[i][0]
        assert np.array_equal(got["ref_hap"][snp:snp + b - a], one["ref_hap"]) and np.array_equal(got["alt_hap"][snp:snp + b - a], one["alt_hap"]), regs[i][0]
        snp += b - a


@pytest.mark.parametrize("name", sorted(C.edge_problems()))
def test_hand_made_edges_equal_the_oracle(name):
    """all_cells_disabled, no_columns: kept all 0, failed (the kernel's M == 0 branch, by three roads); empty_between: 1 0 1 and the
    neighbours as the oracle has them; one_snp: kept, not flipped, phased; stored / dropped_zero_depth: dp == 0 entries in the
    CSC, a column and a cell of nothing else; shared_column: one pileup column in two regions; disabled_only_depth: the mask
    switches off the one cell that covers SNP 11."""
    p, want = C.edge_problems()[name]
    o = C.solved("edge/" + name, p)
    assert o["decisive"].all()
    got = capi.local_phase(**p)
    assert check(p, o, got) == []
    for k, v in want.items():
        assert got[k].tolist() == v, (k, got[k])


def test_stored_zero_depth_entries_change_nothing():
    """The same dense counts with the dp == 0 entries stored and dropped: identical results."""
    E = C.edge_problems()
    a, b = capi.local_phase(**E["stored_zero_depth"][0]), capi.local_phase(**E["dropped_zero_depth"][0])
    assert same_bytes(a, b)


def test_empty_region_leaves_its_neighbours_alone():
    """The neighbours of the empty region answer as they do in a problem without it."""
    p = C.edge_problems()["empty_between"][0]
    got, without = capi.local_phase(**p), capi.local_phase(**C.subproblem(p, [0, 2]))
    assert got["status"].tolist() == [1, 0, 1] and without["status"].tolist() == [1, 1]
    assert all(got[k].tobytes() == without[k].tobytes() for k in ("kept", "flip", "ref_hap", "alt_hap"))
