"""The model the consensus tests compare the engine with (tests/umi_consensus_model.py), held against the pinned oracle on the CPU:
under rule "first" it is the oracle on every input tests/test_gpu_umi_consensus.py uses, so what the GPU test shows under rule
"consensus" differs from the reference by the rule alone.  Also the ABI additions as the header and capi.py state them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle as O
import umi_consensus_model as UM
import util
from xcltk_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATS = ("ad", "dp", "oth")


def _oracle(c, flags=0):
    f = dict(UM.FILT); f.update(c.filt)
    cfg, keep = O.make_config(capi.XCK_MODE_BAF, c.names, c.regions, c.snps, c.n_cells, flags=flags, **f)
    return O.run_oracle(cfg, [util.batch_from_dict(d)[0] for d in c.batches])


def _same(m, exp):
    for k in MATS:
        for j, what in enumerate(("row", "col", "val")):
            assert np.array_equal(getattr(m, k)[j] if not isinstance(m, dict) else m[k][j], exp[k][j]), "%s.%s differs" % (k, what)


@pytest.mark.parametrize("name", UM.CASES)
def test_first_rule_is_the_oracle_on_the_crafted_cases(name):
    c = UM.case(name)
    m = UM.model(c.names, c.regions, c.snps, c.batches, c.filt, "first")
    _same(m, _oracle(c))


@pytest.mark.parametrize("seed", UM.FUZZ_SEEDS)
def test_first_rule_is_the_oracle_on_the_fuzz_cases_and_they_are_deep(seed):
    """(a) on the fuzz inputs, and (c) what their generator has to deliver: enough molecules, a third of them with several reads,
    some changed by the vote and at least one tie.  A seed that misses fails here: the GPU test would compare little."""
    c = UM.fuzz_case(seed)
    mols, _ = UM.molecules(c.names, c.snps, c.batches, c.filt)
    _same(UM.fold(c.names, c.regions, c.snps, c.filt, mols, "first"), _oracle(c, c.flags))
    n = UM.fold(c.names, c.regions, c.snps, c.filt, mols, "consensus").counters
    print(seed, n)
    assert n["molecules"] >= 200 and 3 * n["multi_read"] >= n["molecules"] and n["changed"] >= 5 and n["tied"] >= 1, n


def test_rules_agree_where_every_molecule_has_one_read():
    c = UM.case("single")
    mols, _ = UM.molecules(c.names, c.snps, c.batches, c.filt)
    assert mols and all(len(v) == 1 for v in mols.values())
    a, b = (UM.fold(c.names, c.regions, c.snps, c.filt, mols, rule) for rule in ("first", "consensus"))
    _same(a, {k: getattr(b, k) for k in MATS})
    assert np.array_equal(a.tally, b.tally) and a.tally.sum() > 0
    assert b.counters == dict(molecules=int(a.tally.sum()), multi_read=0, discordant=0, tied=0, changed=0)


def test_the_rule_on_its_run_shapes():
    """the vote, shape by shape, and that the first case is the one the default gets wrong"""
    r = lambda s: [(i, UM.NIB[ch] if ch not in "nd" else -1) for i, ch in enumerate(s)]
    show = lambda s, rule: UM.NT16[UM.call(r(s), rule)[0]] if UM.call(r(s), rule)[0] >= 0 else None
    assert show("ACC", "first") == "A" and show("ACC", "consensus") == "C" and UM.call(r("ACC"), "consensus")[1] == [1, 1, 1, 0, 1]
    assert show("AC", "consensus") == "A" and UM.call(r("AC"), "consensus")[1] == [1, 1, 1, 1, 0]
    assert show("TAACC", "consensus") == "A" and UM.call(r("TAACC"), "consensus")[1] == [1, 1, 1, 1, 1]
    assert show("NNA", "consensus") == "A" and show("N", "consensus") == "N" and show("M", "consensus") == "M" and show("MNC", "consensus") == "C"
    assert show("nC", "first") is None and show("nC", "consensus") == "C" and UM.call(r("nC"), "consensus")[1] == [1, 0, 0, 0, 0]
    assert show("nn", "consensus") is None and UM.call(r("nn"), "consensus")[1] == [0, 0, 0, 0, 0]
    c = UM.case("shapes")
    a, b = (UM.model(c.names, c.regions, c.snps, c.batches, c.filt, rule) for rule in ("first", "consensus"))
    assert a.tally[0].tolist() == [1, 0, 0, 0, 0] and b.tally[0].tolist() == [0, 1, 0, 0, 0]
    assert a.tally[7].sum() == 0 and b.tally[7].tolist() == [0, 1, 0, 0, 0] and b.tally[8].sum() == 0
    assert b.counters["changed"] >= 3 and b.counters["tied"] >= 3


def test_run_lengths_straddle_the_walk():
    W = UM.run_walk()
    assert W == 64
    mols, _ = UM.molecules(UM.NAMES, UM.SNPS, UM.case("walk").batches, {})
    assert sorted(len(v) for v in mols.values()) == sorted([W, W + 1, W + 2] * 3)
    mols, _ = UM.molecules(UM.NAMES, UM.SNPS, UM.case("long").batches, {})
    assert sorted(len(v) for v in mols.values()) == [3, 255, 256, 257, 1025]
    assert len(UM.SNPS) == 33 and UM.N_CELLS == 3


def test_header_flag_struct_and_symbol():
    with open(os.path.join(ROOT, "include", "xck.h")) as fp:
        h = fp.read()
    assert int(re.search(r"#define XCK_F_UMI_CONSENSUS\s+(\d+)", h).group(1)) == capi.XCK_F_UMI_CONSENSUS == 256
    body = re.search(r"typedef struct xck_molecule_stats \{(.*?)\} xck_molecule_stats;", h, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|int32_t|int64_t)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in capi.MoleculeStats._fields_]
    assert C.sizeof(capi.MoleculeStats) == 48 and capi.MOLECULE_FIELDS == UM.COUNTERS
    assert "int  xck_get_molecule_stats(xck_engine* e, xck_molecule_stats* out);" in h and "XCK_UMI_CONSENSUS=1" in h
    assert ("xck_get_molecule_stats", C.c_int, [C.c_void_p, C.POINTER(capi.MoleculeStats)]) in capi.SYMBOLS


def test_molecule_summary_text():
    from xcltk_amd import fc_common as fcc
    st = dict(zip(capi.MOLECULE_FIELDS, (7, 5, 3, 2, 1)))
    assert fcc.molecule_summary_text(st) == "molecules\t7\nmulti_read\t5\ndiscordant\t3\ntied\t2\nchanged\t1\n"
    assert fcc.molecule_summary_text(st, 2, 1).startswith("#ranks=2 cut_contigs=1\nmolecules\t7\n")
