"""Helpers of the local-phasing tests: the fixture of tests/golden/local_phase (tools/make_local_phase_fixture.py wrote it, with the
host path's answers) and the call that runs one of its problems on the device."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "local_phase", "fixture.npz")
FIELDS = ("col_ptr", "cell", "ad", "dp", "ref_hap", "alt_hap", "reg_ptr", "slot_col", "slot_snp", "slot_pos")
MIN_STABLE = 0.95                                                        # share of stable regions the fixture must have
_cache = {}


def problem_names():
    with np.load(FIXTURE) as z:
        return [str(n) for n in z["problems"]]


def load_problem(name):
    """-> (arguments of capi.local_phase / phasing_dev.host_phase_slots, expected: dict with names, stable, kept, flip, status, ...)"""
    if name not in _cache:
        with np.load(FIXTURE) as z:
            args = {k: z[name + "/" + k] for k in FIELDS}
            args["n_cells"] = int(z[name + "/n_cells"])
            args["cell_enabled"] = z[name + "/cell_enabled"] if bool(z[name + "/has_cell_enabled"]) else None
            exp = {k: z[name + "/exp_" + k] for k in ("kept", "flip", "status", "ref_hap", "alt_hap")}
            exp["n_levels"] = int(z[name + "/exp_n_levels"])
            exp["names"] = [str(n) for n in z[name + "/names"]]
            exp["stable"] = z[name + "/stable"].astype(bool)
        _cache[name] = (args, exp)
    return _cache[name]


def compare(args, exp, got):
    """kept, status and the dropped pairs are integer logic: equal on every region; flip: equal on every stable region.
    -> names of the unstable regions whose flips differ (reported, not asserted)."""
    assert np.array_equal(got["kept"], exp["kept"]), "kept differs"
    assert np.array_equal(got["status"], exp["status"]), "status differs: %s" % [n for n, a, b in zip(exp["names"], got["status"], exp["status"]) if a != b]
    reg_ptr = args["reg_ptr"]
    bad, unstable_diff = [], []
    for r, name in enumerate(exp["names"]):
        a, b = int(reg_ptr[r]), int(reg_ptr[r + 1])
        if not np.array_equal(got["flip"][a:b], exp["flip"][a:b]):
            (bad if exp["stable"][r] else unstable_diff).append(name)
    assert not bad, "flip differs from the host path on stable regions: %s" % bad
    return unstable_diff
