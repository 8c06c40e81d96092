"""The cases and the model of the UMI collapsing tests (tests/umi_dedup_cases.py) on the CPU: the model's pattern without collapsing is
the plain oracle matrix on every case, so what tests/test_gpu_umi_dedup.py shows against the model it shows against the oracle's join;
the crafted cases have the answers they were built for; the generated ones merge in some groups and not in others; the header, the
bindings and the summary text agree."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import umi_dedup_cases as UD
from xcltk_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (64, 128)
BIG = ("class_limits", "complete6", "parity7", "parity8")            # (their pairwise check would take minutes)


@pytest.mark.parametrize("key_bits", WIDTHS)
@pytest.mark.parametrize("name", UD.ALL)
def test_exact_pattern_is_the_plain_oracle(name, key_bits):
    c, m = UD.case(name, key_bits), UD.case_model(name, key_bits)
    plain = UD.plain_oracle(c)
    for got, exp in zip(m.exact, plain):
        assert np.array_equal(got, exp)
    assert m.counters["keys"] == int(plain[2].sum()) and m.counters["groups"] == len(plain[0])
    assert m.counters["molecules"] == int(m.count[2].sum())
    # every cell count is at most the exact count, and the two matrices have the same non-zeros
    assert np.array_equal(m.count[0], plain[0]) and np.array_equal(m.count[1], plain[1]) and (m.count[2] <= plain[2]).all() and (m.count[2] >= 1).all()
    assert m.counters["groups_changed"] == int((m.count[2] < plain[2]).sum())


@pytest.mark.parametrize("key_bits", WIDTHS)
@pytest.mark.parametrize("name", ["distance2", "group_boundary", "no_hits", "one_key", "all_dropped_upstream"])
def test_without_adjacent_pairs_the_model_is_the_plain_oracle(name, key_bits):
    c, m = UD.case(name, key_bits), UD.case_model(name, key_bits)
    plain = UD.plain_oracle(c)
    assert all(np.array_equal(a, b) for a, b in zip(m.count, plain)) and m.counters["groups_changed"] == 0


@pytest.mark.parametrize("key_bits", WIDTHS)
@pytest.mark.parametrize("name", sorted(UD.CRAFTED))
def test_crafted_cases_have_their_literal_answers(name, key_bits):
    c, m = UD.case(name, key_bits), UD.case_model(name, key_bits)
    count, counters = c.literal
    assert UD.coo_dict(m.count) == count and m.counters == counters
    if name in UD.WITH_UF:
        mu = UD.case_model(name, key_bits, True)
        count, counters = c.literal_uf
        assert UD.coo_dict(mu.count) == count and mu.counters == counters
    if name not in BIG:                                               # the neighbour search of the model against the pairwise test as the rule states it
        mp = UD.model(c, pairwise=True)
        assert UD.coo_dict(mp.count) == count if name not in UD.WITH_UF else UD.coo_dict(mp.count) == c.literal[0]


def test_the_rule_on_pairs():
    ub = 40
    d, i = UD.direct, UD.interned
    assert UD.adjacent(d(0b0110), d(0b0111), ub) and UD.adjacent(d(0b0110), d(0b1010), ub) and not UD.adjacent(d(0b0110), d(0b1011), ub)
    assert not UD.adjacent(d(5, 4), d(5, 4), ub)
    assert not UD.adjacent(d(5, 7), d((1 << 14) | 5, 8), ub)             # one field, other length
    assert not UD.adjacent(i(8, ub), i(12, ub), ub) and not UD.adjacent(i(d(5), ub), d(5), ub)
    assert sorted(UD.neighbours(d(0, 2))) == sorted(d(v, 2) for v in (1, 2, 3, 4, 8, 12))
    for L in (3, 5):
        code = UD.parity_code(L)
        assert len(code) == 4 ** (L - 1) and not any(UD.adjacent(d(a, L), d(b, L), ub) for a in code[:40] for b in code[:40])
    path = UD.staircase()
    assert len(path) == 25 and len(set(path)) == 25
    assert all(UD.adjacent(d(path[a]), d(path[b]), ub) == (abs(a - b) == 1) for a in range(25) for b in range(25))


def test_cases_reach_every_path_and_edge():
    S, M, T = UD.small_limit(), UD.medium_limit(), UD.tile_size()
    assert (S, T) == (64, 2048) and 4097 <= M < 16384                    # parity7 takes the LDS union-find, parity8 the one in the workspace
    sizes = sorted(len(v) for v in UD.case_model("class_limits", 64).groups.values())
    assert sizes == [1, 2, S - 1, S, S + 1, M - 1, M, M + 1]
    for name, at, n in (("tile_edge_pair", T - 1, 2), ("tile_edge_path", T - 9, 25)):
        m = UD.case_model(name, 64)
        keys = sorted((r, c, u) for (r, c), v in m.groups.items() for u in v)
        big = [k for k, v in m.groups.items() if len(v) == n]
        assert len(big) == 1 and [i for i, k in enumerate(keys) if k[:2] == big[0]] == list(range(at, at + n))
    c = UD.case("repeated", 64)
    assert sum(len(d["pos"]) for d in c.batches) == 5 * 52


@pytest.mark.parametrize("key_bits", WIDTHS)
@pytest.mark.parametrize("name", sorted(UD.GENERATED))
def test_generated_cases_merge_and_keep(name, key_bits):
    """Conditions on the inputs, for the model alone: of the groups with two or more keys at least a tenth change and a tenth do not."""
    c, m = UD.case(name, key_bits), UD.case_model(name, key_bits)
    print(name, key_bits, m.counters, "multi-key groups", m.n_multi, "changed %.3f" % m.frac_changed)
    assert m.n_multi >= 100 and 0.10 <= m.frac_changed <= 0.90
    assert m.counters["opaque_keys"] > 0 and m.counters["max_group"] <= UD.small_limit() * 40
    mu = UD.case_model(name, key_bits, True)
    assert 0 < mu.counters["keys"] < m.counters["keys"]                  # overlapping genes: the unique-feature rule has something to drop


def test_header_and_bindings_agree():
    h = open(os.path.join(ROOT, "include", "xck.h")).read()
    assert int(re.search(r"#define XCK_F_UMI_COLLAPSE\s+(\d+)", h).group(1)) == capi.XCK_F_UMI_COLLAPSE == 2048
    flags = [int(x) for x in re.findall(r"#define XCK_F_\w+\s+(\d+)\s", h)]
    assert len(set(flags)) == len(flags) and max(flags) == 2048          # the next free bit
    body = re.search(r"typedef struct xck_umi_dedup_stats \{(.*?)\} xck_umi_dedup_stats;", h, re.S).group(1)
    fields = re.findall(r"int64_t\s+(\w+);", body)
    assert tuple(fields) == capi.UMI_DEDUP_FIELDS == UD.FIELDS
    assert C.sizeof(capi.UmiDedupStats) == 8 + 8 * len(fields)
    assert "int  xck_get_umi_dedup_stats(xck_engine* e, xck_umi_dedup_stats* out);" in h and "XCK_UMI_DEDUP=1mm_all|exact" in h
    assert ("xck_get_umi_dedup_stats", C.c_int, [C.c_void_p, C.POINTER(capi.UmiDedupStats)]) in capi.SYMBOLS
    assert int(re.search(r"#define XCK_ABI_VERSION\s+(\d+)", h).group(1)) == 3


def test_knob_parser_and_argument_table():
    """XCK_UMI_DEDUP is read at xck_create: 1mm_all and exact (and an empty value) pass, anything else is XCK_E_ARG with the text quoted;
    the flag on a decode-only or BAF-only handle is XCK_E_ARG.  Decode-only handles touch no GPU."""
    from xcltk_amd.engine import Engine, XckError
    names, regions = ["1"], [("1", 1, 1000, "g")]
    def create(**kw):
        return Engine(kw.pop("mode", capi.XCK_MODE_BASEFC), names, regions, 2, decode_only=True, **dict(UD.KW, **kw))
    old = os.environ.get("XCK_UMI_DEDUP")
    try:
        for text, ok in (("1mm_all", True), ("exact", True), ("", True), ("1MM_All", False), ("directional", False), ("1", False), (" 1mm_all", False)):
            os.environ["XCK_UMI_DEDUP"] = text
            if ok:
                with create() as eng:
                    assert eng.umi_dedup_stats() is None              # (a decode-only handle ignores the knob)
            else:
                with pytest.raises(XckError) as ei:
                    create()
                assert ei.value.code == capi.XCK_E_ARG and "XCK_UMI_DEDUP" in str(ei.value) and text in str(ei.value)
        del os.environ["XCK_UMI_DEDUP"]
        with pytest.raises(XckError) as ei:
            create(umi_dedup="1mm_all")
        assert ei.value.code == capi.XCK_E_ARG and "XCK_F_UMI_COLLAPSE" in str(ei.value)
        with pytest.raises(XckError) as ei:
            create(mode=capi.XCK_MODE_BAF, flags=capi.XCK_F_UMI_COLLAPSE, snps=[("1", 50, "A", "C", 0, 1)])
        assert ei.value.code == capi.XCK_E_ARG
        with pytest.raises(ValueError):
            create(umi_dedup="directional")
        with create(umi_dedup="exact") as eng:
            assert eng.umi_dedup_stats() is None
    finally:
        os.environ.pop("XCK_UMI_DEDUP", None)
        if old is not None:
            os.environ["XCK_UMI_DEDUP"] = old


def test_summary_text():
    from xcltk_amd import fc_common as fcc
    st = dict(keys=9, molecules=7, groups=4, groups_changed=2, opaque_keys=1, max_group=5)
    assert fcc.umi_dedup_summary_text(st) == "keys\t9\nmolecules\t7\ngroups\t4\ngroups_changed\t2\nopaque_keys\t1\nmax_group\t5\n"
    assert fcc.umi_dedup_summary_text(st, 2, 0) == "#ranks=2 cut_contigs=0\n" + fcc.umi_dedup_summary_text(st)
