"""Key layouts on the host: the layout a handle reports for every shape of the grid of tests/test_gpu_layouts.py, and the oracle on
the targeted cases of tests/layout_cases.py against their by-construction answers - at table sizes where the oracle (which keeps
(cell, umi) structs and 64-bit coordinates and has no packed key) has not been run before.  No GPU."""
import numpy as np
import pytest

import layout_cases as LC
import oracle as O
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine

KW = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True, min_include=0.9, min_count=1, min_maf=0, no_dup_hap=True)


def test_layout_rule_on_known_points():
    """The points checked by hand when the grid was chosen (umi_bits as a decode-only handle reports them)."""
    assert LC.expected_layout(262143, 1 << 20) == (64, 26, 20, 18)
    assert LC.expected_layout(262144, 1 << 20) == (128, 64, 20, 19)
    assert LC.expected_layout(262143, (1 << 20) + 1) == (128, 64, 21, 18)
    assert LC.expected_layout(3, 16384)[1] == 48 and LC.expected_layout(3, 16385)[1] == 47
    assert LC.expected_layout(278528, 1 << 17)[1] == 28
    assert LC.expected_layout(63, 1 << 30) == (64, 28, 30, 6)
    assert LC.expected_layout(3, 2) == (64, 61, 1, 2)
    assert [sum(LC.expected_layout(r, c)[2:]) for r, c in ((255, 256), (65535, 65536), (65536, 65536))] == [16, 32, 33]
    assert LC.longest_direct(26) == 12 and LC.longest_direct(28) == 13 and LC.longest_direct(64) == 31
    assert LC.intern_id_limit(26) == (1 << 25) - 1


@pytest.mark.parametrize("baf", [False, True], ids=["basefc", "baf"])
@pytest.mark.parametrize("shape", LC.GRID, ids=lambda s: "%dx%d" % s)
def test_decode_only_handle_reports_the_expected_layout(shape, baf):
    n, n_cells = shape
    names, regions, snps = LC.make_table(n, with_snps=baf)
    key_bits, umi_bits, cbits, rbits = LC.expected_layout(n, n_cells, n if baf else 0)
    eng = Engine(capi.XCK_MODE_BAF if baf else capi.XCK_MODE_BASEFC, names, regions, n_cells, snps=snps, decode_only=True)
    try:
        assert eng.umi_bits == umi_bits
        assert (128 if eng.umi_bits == 64 else 64) == key_bits
    finally:
        eng.close()


def test_snps_alone_widen_the_row_field():
    """BAF sizes the row field for max(n_regions, n_snps): 4 regions with 262 143 / 262 144 SNPs sit on the two sides of the switch."""
    names, regions, _ = LC.make_table(4)
    for n_snps, want in ((262143, 26), (262144, 64)):
        _, _, snps = LC.make_table(n_snps, with_snps=True)
        eng = Engine(capi.XCK_MODE_BAF, names, regions, 1 << 20, snps=snps, decode_only=True)
        try:
            assert eng.umi_bits == want == LC.expected_layout(4, 1 << 20, n_snps)[1]
        finally:
            eng.close()


def test_umi_codes_fill_the_field():
    for ub in (26, 27, 28, 47, 61, 64):
        c = LC.umi_codes(ub, LC.ALL_UMIS)
        L = LC.longest_direct(ub)
        assert 2 * L + 1 <= ub - 1 < 2 * (L + 1) + 1                     # L is the longest direct length, L + 1 is interned
        assert c["direct_t"].bit_length() == 2 * L + 1 and c["direct_a"].bit_length() == 2 * L + 1
        assert c["intern_top"] == (1 << ub) - 2 and c["intern0"].bit_length() == ub   # the top bit of the field; all ones stays free
        assert len(set(c.values())) == len(c)


@pytest.mark.parametrize("shape", LC.GRID, ids=lambda s: "%dx%d" % s)
def test_oracle_equals_the_answer_by_construction(shape):
    """basefc: the oracle's matrix of the targeted case is the distinct-UMI count per (row, cell).  BAF: the case's full answer is short
    (one SNP per region, one base per molecule: layout_cases.answers()), so AD, DP and OTH are compared element-wise, and the sums the
    construction implies are checked on top: total DP = molecules showing REF or ALT, DP + OTH = all molecules, AD <= DP."""
    n, n_cells = shape
    case = LC.targeted_case(n, n_cells, n_snps=n)
    assert case.layout == LC.expected_layout(n, n_cells, n)
    b = util.batch_from_dict(case.d)
    n_mol = len({t for t in case.triples if t[2] != capi.XCK_UMI_NONE})
    assert n_mol == len(case.triples) * 5 // 6 and len(case.d["pos"]) > len(case.triples)      # duplicates are there to collapse
    cfg, keep = O.make_config(capi.XCK_MODE_BASEFC, case.names, case.regions, [], n_cells, **KW)
    exp = O.run_oracle(cfg, [b[0]])
    util.assert_coo_equal(exp, case.expected, ["count"])
    assert int(exp["count"][2].sum()) == n_mol and int(exp["count"][0].max()) == n - 1 and int(exp["count"][1].max()) == n_cells - 1
    cfg, keep = O.make_config(capi.XCK_MODE_BAF, case.names, case.regions, case.snps, n_cells, **KW)
    exp = O.run_oracle(cfg, [b[0]])
    util.assert_coo_equal(exp, case.expected, ["ad", "dp", "oth"])
    n_refalt = len({t for i, t in enumerate(case.triples) if t[2] != capi.XCK_UMI_NONE and i % 3 != 2})
    assert int(exp["dp"][2].sum()) == n_refalt and int(exp["dp"][2].sum()) + int(exp["oth"][2].sum()) == n_mol
    ad = dict(zip(zip(exp["ad"][0].tolist(), exp["ad"][1].tolist()), exp["ad"][2].tolist()))
    dp = dict(zip(zip(exp["dp"][0].tolist(), exp["dp"][1].tolist()), exp["dp"][2].tolist()))
    assert all(k in dp and 0 < v <= dp[k] for k, v in ad.items()) and 0 < sum(ad.values()) < sum(dp.values())
