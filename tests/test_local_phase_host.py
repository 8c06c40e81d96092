"""The host side of the device local phasing (no GPU): the slot and level builder of baf/fc/phasing_dev.py against local_phasing()
of baf/fc/phasing.py, the argument checks of xck_local_phase that run before the device is touched, the switch, and the fixture."""
import logging
import os

import numpy as np
import pytest

import local_phase_util as U
import util
from xcltk_amd import capi
from xcltk_amd import fc_common as fcc
from xcltk_amd.baf.fc import phasing_dev as PD
from xcltk_amd.baf.fc.phasing import local_phasing
from xcltk_amd.engine import XckError
from xcltk_amd.utils.csp_io import CellSnpData, load_data

DS = os.path.join(util.GOLDEN, "datasets", "phasing")


def _tables(extra_regions=()):
    regions = fcc.load_region_from_txt(os.path.join(DS, "regions.tsv"), verbose=False) + list(extra_regions)
    snps = fcc.load_snp_from_tsv(os.path.join(DS, "snps.tsv"), verbose=False)
    return regions, snps


def _ref_cells():
    with open(os.path.join(DS, "ref_cells.tsv")) as fp:
        return [x.strip().split("\t")[0] for x in fp if x.strip()]


def _assert_tuples_equal(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert a[4] == b[4]


def _host_through_slots(regions, snps, csp, ref_cells):
    """build_slots -> the host's reg_local_phasing region by region (host_phase_slots) -> the tuple."""
    slots = PD.build_slots(regions, snps, csp, ref_cells)
    col_ptr, cell, ad, dp, enabled = slots["csc"]
    h = PD.host_phase_slots(csp.DP.shape[0], col_ptr, cell, ad, dp, [s[4] for s in snps], [s[5] for s in snps], slots["reg_ptr"],
                            slots["slot_col"], slots["slot_snp"], slots["slot_pos"], cell_enabled=enabled)
    return slots, PD.tuple_from_result(regions, slots, h["kept"], h["flip"], h["status"], h["ref_hap"], h["alt_hap"])


@pytest.mark.parametrize("cellsnp,with_ref_cells", [("cellsnp", False), ("cellsnp", True), ("cellsnp_short", False), ("cellsnp_surplus", False)])
def test_slots_reproduce_local_phasing_on_the_golden_dataset(cellsnp, with_ref_cells, caplog):
    regions, snps = _tables()
    csp = load_data(os.path.join(DS, cellsnp))
    ref_cells = _ref_cells() if with_ref_cells else None
    with caplog.at_level(logging.INFO):
        exp = local_phasing(regions, snps, csp, ref_cells)
        exp_log = [r.getMessage() for r in caplog.records]
        caplog.clear()
        slots, got = _host_through_slots(regions, snps, csp, ref_cells)
        got_log = [r.getMessage() for r in caplog.records]
    _assert_tuples_equal(got, exp)
    assert got_log == exp_log and len(exp_log) >= 2
    assert exp[4]["n_rlp"] == len(slots["region"]) > 0
    # long_a and long_b_overlaps_a share SNPs: two levels
    lv = PD.region_levels(slots["reg_ptr"], slots["slot_snp"])
    names = [regions[g][3] for g in slots["region"]]
    assert lv[names.index("long_a")] == 0 and lv[names.index("long_b_overlaps_a")] == 1 and lv.max() == 1
    if cellsnp == "cellsnp_short":
        assert slots["short"].any() and (slots["slot_col"][slots["short"]] == -1).all()


def test_chain_and_duplicate_regions_get_levels_and_hand_their_state_on():
    regions, snps = _tables([("1", 380001, 800000, "chain_c"), ("1", 380001, 800000, "chain_c_again"), ("1", 10001, 250000, "long_a_again")])
    csp = load_data(os.path.join(DS, "cellsnp"))
    exp = local_phasing(regions, snps, csp, None)
    slots, got = _host_through_slots(regions, snps, csp, None)
    _assert_tuples_equal(got, exp)
    names = [regions[g][3] for g in slots["region"]]
    lv = dict(zip(names, PD.region_levels(slots["reg_ptr"], slots["slot_snp"]).tolist()))
    assert lv["long_a"] == 0 and lv["long_b_overlaps_a"] == 1 and lv["chain_c"] == 2 and lv["chain_c_again"] == 3
    assert lv["long_a_again"] == lv["long_b_overlaps_a"] + 1
    # the fixture's chain: A B C, C again, and a region on its own
    args, fx = U.load_problem("chain_and_duplicate")
    assert PD.region_levels(args["reg_ptr"], args["slot_snp"]).tolist() == [0, 1, 2, 3, 0] and fx["n_levels"] == 4


def test_covered_surplus_columns_raise_as_on_the_host():
    """More covered pileup columns than SNPs in the list: numpy stops the host path, and the builder says the same."""
    snps = [("1", 1000 + 30000 * k, "A", "C", 0, 1) for k in range(3)]
    regions = [("1", 1, 100000, "g")]
    pos = [1000, 31000, 45000, 61000]                                    # 45000 is in the pileup, not in the list
    DP = np.array([[3, 2, 1, 4], [1, 5, 2, 2]])
    csp = CellSnpData(["1"] * 4, pos, ["A"] * 4, ["C"] * 4, ["c0", "c1"], DP // 2, DP, DP * 0)
    with pytest.raises(ValueError) as e_host:
        local_phasing(regions, snps, csp, None)
    with pytest.raises(ValueError) as e_dev:
        PD.build_slots(regions, snps, csp, None)
    assert str(e_dev.value) == str(e_host.value) and "covered beyond the list's length" in str(e_host.value)


def _tiny():
    return dict(n_cells=2, col_ptr=[0, 2, 4], cell=[0, 1, 0, 1], ad=[1, 0, 2, 1], dp=[2, 2, 2, 2], ref_hap=[0, 1], alt_hap=[1, 0],
                reg_ptr=[0, 2], slot_col=[0, 1], slot_snp=[0, 1], slot_pos=[100, 60000])


@pytest.mark.parametrize("change,text", [
    (dict(struct_size=8), "struct_size"),
    (dict(cell=[0, 2, 0, 1]), "cell index outside"),
    (dict(cell=[1, 0, 0, 1]), "strictly ascending"),
    (dict(cell=[0, 0, 0, 1]), "strictly ascending"),
    (dict(col_ptr=[0, 3, 2]), "col_ptr runs backwards"),
    (dict(col_ptr=[1, 2, 4]), "start at 0"),
    (dict(ad=[3, 0, 2, 1]), "ad outside"),
    (dict(ad=[-1, 0, 2, 1]), "ad outside"),
    (dict(ref_hap=[0, 2]), "haplotype index"),
    (dict(slot_col=[0, 2]), "slot column outside"),
    (dict(slot_col=[0, -2]), "slot column outside"),
    (dict(slot_snp=[0, 2]), "slot SNP outside"),
    (dict(slot_snp=[1, 1]), "twice in one region"),
    (dict(reg_ptr=[0, 2, 1]), "reg_ptr runs backwards"),
    (dict(n_cells=0), "table sizes"),
])
def test_bad_arguments_are_refused_before_the_device_is_touched(change, text):
    with pytest.raises(XckError) as e:
        capi.local_phase(**dict(_tiny(), **change))
    assert e.value.code == capi.XCK_E_ARG and text in str(e.value)


def test_binding_checks_array_lengths():
    with pytest.raises(ValueError):
        capi.local_phase(**dict(_tiny(), dp=[2, 2, 2]))
    with pytest.raises(ValueError):
        capi.local_phase(**dict(_tiny(), cell_enabled=[1]))
    with pytest.raises(ValueError):
        capi.local_phase(**dict(_tiny(), col_ptr=[0, 2, 5]))


def test_null_arguments():
    lib = capi.load()
    assert lib.xck_local_phase(None, None) == capi.XCK_E_ARG
    lib.xck_free_phase_result(None)


def test_the_switch(monkeypatch, caplog):
    from xcltk_amd.baf.fc.main import _device_phasing_or_host
    monkeypatch.delenv("XCK_DEVICE_PHASING", raising=False)
    assert _device_phasing_or_host(local_phasing) is local_phasing
    monkeypatch.setenv("XCK_DEVICE_PHASING", "0")
    assert _device_phasing_or_host(local_phasing) is local_phasing
    monkeypatch.setenv("XCK_DEVICE_PHASING", "1")
    with caplog.at_level(logging.INFO):
        fn = _device_phasing_or_host(local_phasing)
    if capi.load().xck_device_count() == 0:                              # no usable device: the host path, and the log says why
        assert fn is local_phasing and any("no usable HIP device" in r.getMessage() for r in caplog.records)
    else:
        assert fn is not local_phasing


def test_fixture_condition():
    """At least 95 % of the regions give the same host answer whatever the order of the cells."""
    n = n_stable = 0
    for name in U.problem_names():
        args, exp = U.load_problem(name)
        assert len(exp["names"]) == len(args["reg_ptr"]) - 1 == len(exp["status"]) == len(exp["stable"])
        assert len(exp["kept"]) == len(exp["flip"]) == int(args["reg_ptr"][-1])
        n += len(exp["names"]); n_stable += int(exp["stable"].sum())
    args, exp = U.load_problem("synthetic")
    assert len(exp["names"]) == 120 and exp["stable"].mean() >= U.MIN_STABLE and n_stable >= U.MIN_STABLE * n
    sizes = {(int(x.split("_")[1][1:]), int(x.split("_")[2][1:])) for x in exp["names"]}
    assert {c for c, _ in sizes} == {40, 150, 400} and {s for _, s in sizes} == {2, 3, 7, 20, 64, 65, 130}
