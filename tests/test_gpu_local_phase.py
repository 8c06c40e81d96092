"""xck_local_phase (csrc/local_phase.hip): region-wise local phasing on the device against the host path (baf/fc/phasing.py,
baf/localphase.py), whose answers tests/golden/local_phase/fixture.npz holds (tools/make_local_phase_fixture.py).  The outputs are
discrete, so they are compared exactly: kept / status on every region, flip on every region whose host answer does not depend on
the order of the float sums (the fixture's stable flag); the others are reported by name."""
import numpy as np
import pytest

import local_phase_util as U
from xcltk_amd import capi

pytestmark = pytest.mark.gpu

_runs = {}


def device_run(name):
    if name not in _runs:
        args, _ = U.load_problem(name)
        _runs[name] = capi.local_phase(**args)
    return _runs[name]


def _same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("kept", "flip", "status", "ref_hap", "alt_hap")) and a["n_levels"] == b["n_levels"]


def test_synthetic_regions_equal_the_host_path():
    args, exp = U.load_problem("synthetic")
    assert len(exp["names"]) == 120 and exp["stable"].mean() >= U.MIN_STABLE
    got = device_run("synthetic")
    unstable = [n for n, s in zip(exp["names"], exp["stable"]) if not s]
    differ = U.compare(args, exp, got)
    print("unstable regions (host answer depends on the summation order): %s; of these the device differs on: %s" % (unstable, differ))
    assert got["n_levels"] == 1
    ok = exp["stable"] | ~np.isin(exp["names"], differ)
    # where every flip is the host's, so is the final state
    if ok.all():
        assert np.array_equal(got["ref_hap"], exp["ref_hap"]) and np.array_equal(got["alt_hap"], exp["alt_hap"])


def test_second_run_returns_identical_bytes():
    args, _ = U.load_problem("synthetic")
    assert _same_bytes(device_run("synthetic"), capi.local_phase(**args))


@pytest.mark.parametrize("knob,value", [("XCK_PHASE_WCAP", "16"), ("XCK_PHASE_LDS_SNPS", "16")])
def test_recomputed_weights_and_state_in_hbm_change_nothing(knob, value, monkeypatch):
    """Small limits send the regions of 20 SNPs and more down the other path: weights recomputed in every smoothing pass / z and
    orientation in the scratch slice instead of LDS.  Same bytes as the default run."""
    args, _ = U.load_problem("synthetic")
    monkeypatch.setenv(knob, value)
    assert _same_bytes(device_run("synthetic"), capi.local_phase(**args))
    args, _ = U.load_problem("wide_257x300")
    assert _same_bytes(device_run("wide_257x300"), capi.local_phase(**args))


HAND_MADE = [n for n in U.problem_names() if n != "synthetic"]


@pytest.mark.parametrize("name", HAND_MADE)
def test_hand_made_regions_equal_the_host_path(name):
    """baf_ties: cells at exactly 9/20, 11/20 leave (alone: failed), 8/20 and 12/20 stay; filtered_round0 / filtered_later_round:
    failed, nothing flipped; nan_snp: flip all 0; majority_inverts; cell_enabled: an uncovered SNP leaves (kept 0) and the disabled
    cell no longer decides; two_snps; wide_257x300: more SNPs and cells than threads; chain_and_duplicate: levels 0 1 2 3 0 and
    the state handed from region to region; short_pileup: slots without a column."""
    args, exp = U.load_problem(name)
    assert exp["stable"].all(), "hand-made regions are made to be stable"
    got = device_run(name)
    assert U.compare(args, exp, got) == []
    assert np.array_equal(got["ref_hap"], exp["ref_hap"]) and np.array_equal(got["alt_hap"], exp["alt_hap"])
    assert got["n_levels"] == exp["n_levels"]
    assert not got["flip"][got["kept"] == 0].any()
    for r in np.flatnonzero(exp["status"] == 0):                         # a failed region flips nothing
        assert not got["flip"][int(args["reg_ptr"][r]):int(args["reg_ptr"][r + 1])].any()


def test_what_the_hand_made_regions_show():
    """The properties the cases are named for, on the device's own answer."""
    g = device_run("baf_ties")
    assert g["status"].tolist() == [capi.XCK_PHASE_FAILED, capi.XCK_PHASE_PHASED]
    assert device_run("filtered_round0")["status"].tolist() == [0] and device_run("filtered_later_round")["status"].tolist() == [0]
    g = device_run("nan_snp")
    assert g["status"].tolist() == [1] and g["kept"].tolist() == [1, 1, 1] and g["flip"].tolist() == [0, 0, 0]
    assert device_run("majority_inverts")["flip"].tolist() == [0, 0, 1]
    assert device_run("cell_enabled")["kept"].tolist() == [1, 1, 0]
    assert device_run("chain_and_duplicate")["n_levels"] == 4
    args, _ = U.load_problem("short_pileup")
    assert device_run("short_pileup")["kept"][args["slot_col"] < 0].tolist() == [0, 0]


def test_cell_enabled_decides():
    """The same problem with every cell enabled flips SNP 0: the mask removes the cell that decided."""
    args, _ = U.load_problem("cell_enabled")
    on = capi.local_phase(**dict(args, cell_enabled=None))
    assert on["kept"].tolist() == [1, 1, 1] and on["flip"].tolist() != device_run("cell_enabled")["flip"].tolist()


def test_few_workgroups_walk_many_regions(monkeypatch):
    """Seven workgroups for 120 regions: the grid-stride loop reuses every scratch slice seventeen times.  Same bytes."""
    args, _ = U.load_problem("synthetic")
    monkeypatch.setenv("XCK_PHASE_BLOCKS", "7")
    got = capi.local_phase(**args)
    assert got["n_blocks"] == 7 and _same_bytes(device_run("synthetic"), got)
