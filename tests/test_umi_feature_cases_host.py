"""The cases and the model of the unique-feature tests (tests/umi_feature_cases.py) on the CPU: the model's pattern, collapsed by cell, is
the plain oracle matrix on every case, so what tests/test_gpu_umi_feature.py shows against the model it shows against the oracle's
join; the crafted cases have the answers they were built for; the generated ones exercise both branches of the rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import umi_feature_cases as UF
from xcltk_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (64, 128)


@pytest.mark.parametrize("key_bits", WIDTHS)
@pytest.mark.parametrize("name", UF.ALL)
def test_collapsed_pattern_is_the_plain_oracle(name, key_bits):
    c, m = UF.case(name, key_bits), UF.case_model(name, key_bits)
    plain = UF.plain_oracle(c)
    for got, exp in zip(m.collapsed, plain):
        assert np.array_equal(got, exp)
    assert m.counters["keys"] == int(plain[2].sum())
    assert m.counters["keys"] - m.counters["keys_dropped"] == int(m.count[2].sum())
    assert m.counters["multi_feature"] <= m.counters["molecules"] <= m.counters["keys"]


@pytest.mark.parametrize("key_bits", WIDTHS)
@pytest.mark.parametrize("name", sorted(UF.CRAFTED))
def test_crafted_cases_have_their_literal_answers(name, key_bits):
    c, m = UF.case(name, key_bits), UF.case_model(name, key_bits)
    count, counters = c.literal
    assert UF.coo_dict(m.count) == count and m.counters == counters
    if name == "none_dropped":
        assert UF.coo_dict(m.count) == UF.coo_dict(UF.plain_oracle(c)) and len(count) > 0
    if name == "all_dropped":
        assert len(m.count[0]) == 0 and len(UF.plain_oracle(c)[0]) > 0
    if name == "no_hits":
        assert len(UF.plain_oracle(c)[0]) == 0


def test_tile_cases_sit_on_the_boundary():
    """tile_pair: D[T - 1] and D[T] are the two keys of the one two-row molecule; tile_run: the repeated key covers index T of the sorted
    stream.  (D is sorted by cell | UMI | rank; both cases use one cell, and the 2-bit codes grow with the number they spell.)"""
    T = UF.tile_size()
    assert T == 2048
    c = UF.case("tile_pair", 64)
    keys = sorted({(int(u), s) for d in c.batches for u, s in zip(d["umi"].tolist(), (d["pos"] // UF.STRIDE).tolist())})
    assert keys[T - 1][0] == keys[T][0] == UF.direct(T - 1) and keys[T - 2][0] != keys[T - 1][0] and keys[T + 1][0] != keys[T][0]
    c = UF.case("tile_run", 64)
    stream = sorted(int(u) for d in c.batches for u in d["umi"].tolist())
    assert stream[T - 18] == stream[T] == stream[T + 21] == UF.direct(T - 18) and stream.count(UF.direct(T - 18)) == 40


@pytest.mark.parametrize("key_bits", WIDTHS)
@pytest.mark.parametrize("name", sorted(UF.GENERATED))
def test_generated_cases_take_both_branches(name, key_bits):
    c, m = UF.case(name, key_bits), UF.case_model(name, key_bits)
    n_reads = sum(len(d["pos"]) for d in c.batches)
    print(name, key_bits, "reads", n_reads, m.counters, "multi %.3f" % m.frac_multi)
    assert 5000 <= n_reads <= 8004 and m.n_molecules > 500
    assert 0.10 <= m.frac_multi <= 0.90
    rank_is_not_row = [r[3] for r in c.regions[:60]] == ["gene"] * 60 and c.regions[0][1] > c.regions[58][1]
    assert rank_is_not_row and len(c.batches) == 4 and {d["contig"] for d in c.batches} == {0, 1}


def test_header_and_bindings_agree():
    h = open(os.path.join(ROOT, "include", "xck.h")).read()
    assert int(re.search(r"#define XCK_F_UNIQUE_FEATURE\s+(\d+)", h).group(1)) == capi.XCK_F_UNIQUE_FEATURE == 1024
    body = re.search(r"typedef struct xck_umi_feature_stats \{(.*?)\} xck_umi_feature_stats;", h, re.S).group(1)
    fields = re.findall(r"int64_t\s+(\w+);", body)
    assert tuple(fields) == capi.UMI_FEATURE_FIELDS == ("molecules", "multi_feature", "keys", "keys_dropped")
    assert C.sizeof(capi.UmiFeatureStats) == 8 + 8 * len(fields)
    assert "int  xck_get_umi_feature_stats(xck_engine* e, xck_umi_feature_stats* out);" in h and "XCK_UMI_FEATURE=unique|all" in h
    assert ("xck_get_umi_feature_stats", C.c_int, [C.c_void_p, C.POINTER(capi.UmiFeatureStats)]) in capi.SYMBOLS


def test_summary_text():
    from xcltk_amd import fc_common as fcc
    st = dict(molecules=7, multi_feature=2, keys=9, keys_dropped=4)
    assert fcc.umi_feature_summary_text(st) == "molecules\t7\nmulti_feature\t2\nkeys\t9\nkeys_dropped\t4\n"
    assert fcc.umi_feature_summary_text(st, 2, 1) == "#ranks=2 cut_contigs=1\n" + fcc.umi_feature_summary_text(st)
