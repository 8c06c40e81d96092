"""Host-side checks of the per-cell table (no GPU): the ctypes mirror of xck_cell_summary against the header text, the flag rules
xck_create decides without a device, the text of cell_summary.tsv, the writer, and the fixtures themselves."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cell_summary_util as U
import read_fate_util as R
from xcltk_amd import capi
from xcltk_amd import fc_common as fcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASEFC, BAF = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF


def _header():
    with open(os.path.join(ROOT, "include", "xck.h")) as fp:
        return fp.read()


def test_struct_mirrors_the_header():
    h = _header()
    body = re.search(r"typedef struct xck_cell_summary \{(.*?)\} xck_cell_summary;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, name = decl.rsplit(None, 1)
            fields.append((name, " ".join(ctype.split())))
    ctypes_of = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "const int64_t*": C.POINTER(C.c_int64)}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(capi.CellSummary._fields_)
    assert C.sizeof(capi.CellSummary) == 16 + 8 + 8 + 8
    assert capi.CELL_FATE_COLS == U.COLS == capi.READ_FATE_FIELDS[2:] and len(U.COLS) == 12
    assert capi.CELL_MATRIX_COLS == {BASEFC: ("umis", "features"), BAF: ("ad", "dp", "oth", "features")}
    assert int(re.search(r"#define XCK_F_CELL_SUMMARY\s+(\d+)", h).group(1)) == capi.XCK_F_CELL_SUMMARY == 64
    assert int(re.search(r"#define XCK_ABI_VERSION (\d+)", h).group(1)) == 3          # additive: the ABI version stays
    env = h.split("#ifndef XCK_H")[0]
    assert "XCK_CELL_SUMMARY=1" in env and "XCK_CELL_SUMMARY_SLOTS" in env           # the environment list names both knobs


def test_library_exports_the_entry_point(lib):
    assert lib.xck_abi_version() == 3
    assert ("xck_get_cell_summary", C.c_int, [C.c_void_p, C.c_int, C.POINTER(capi.CellSummary)]) in capi.SYMBOLS
    assert lib.xck_get_cell_summary.argtypes == [C.c_void_p, C.c_int, C.POINTER(capi.CellSummary)]


def test_flag_is_refused_on_decode_only_handles(lib, monkeypatch):
    from xcltk_amd.engine import Engine, XckError
    monkeypatch.delenv("XCK_CELL_SUMMARY", raising=False)
    with pytest.raises(XckError) as ei:
        Engine(BASEFC, ["1"], [("1", 1, 100, "g")], 1, flags=capi.XCK_F_CELL_SUMMARY, decode_only=True)
    assert ei.value.code == capi.XCK_E_ARG
    for env in (None, "1"):                                    # decode-only handles ignore the environment knob
        if env:
            monkeypatch.setenv("XCK_CELL_SUMMARY", env)
        with Engine(BASEFC, ["1"], [("1", 1, 100, "g")], 1, decode_only=True) as eng:
            cs = capi.CellSummary()
            cs.struct_size = C.sizeof(capi.CellSummary)
            assert lib.xck_get_cell_summary(eng.h, BASEFC, C.byref(cs)) == capi.XCK_E_STATE
            assert eng.cell_summary() is None and eng.read_fate() is None
            cs.struct_size = 8
            assert lib.xck_get_cell_summary(eng.h, BASEFC, C.byref(cs)) == capi.XCK_E_ARG
    assert lib.xck_get_cell_summary(None, BASEFC, None) == capi.XCK_E_ARG


def _hand_made():
    fate = np.arange(3 * 12, dtype=np.int64).reshape(3, 12)    # two cells and the `*` row
    matrix = np.array([[100, 7], [200, 9]], dtype=np.int64)
    return ["cellB", "cellA"], fate, matrix


def test_cell_summary_text():
    names, fate, matrix = _hand_made()
    one = fcc.cell_summary_text(names, fate, matrix, U.COLS, capi.CELL_MATRIX_COLS[BASEFC])
    lines = one.splitlines()
    assert one.endswith("\n") and len(lines) == 4
    assert lines[0] == "cell\treads\t" + "\t".join(U.COLS) + "\tumis\tfeatures"
    # the given order (the matrix columns), never sorted; reads = the ten class columns
    assert lines[1] == "cellB\t%d\t" % sum(range(10)) + "\t".join(str(v) for v in range(12)) + "\t100\t7"
    assert lines[2] == "cellA\t%d\t" % sum(range(12, 22)) + "\t".join(str(v) for v in range(12, 24)) + "\t200\t9"
    assert lines[3] == "*\t%d\t" % sum(range(24, 34)) + "\t".join(str(v) for v in range(24, 36)) + "\t0\t0"
    many = fcc.cell_summary_text(names, fate, matrix, U.COLS, capi.CELL_MATRIX_COLS[BASEFC], n_ranks=4, cut_contigs=2)
    assert many == "#ranks=4 cut_contigs=2\n" + one
    assert fcc.cell_summary_text(names, fate, matrix, U.COLS, capi.CELL_MATRIX_COLS[BASEFC], n_ranks=1) == one
    # before a finish there is no matrix: zeros
    none = fcc.cell_summary_text(names, fate, None, U.COLS, capi.CELL_MATRIX_COLS[BAF]).splitlines()
    assert none[0].endswith("\tad\tdp\toth\tfeatures") and none[1].endswith("\t11\t0\t0\t0\t0")


def test_writer_on_off_and_method_absent(tmp_path):
    names, fate, matrix = _hand_made()
    fn = str(tmp_path / "sub" / "cell_summary.tsv")

    class Off(object):
        def cell_summary(self, mode=None):
            return None

    class Absent(object):
        pass

    for eng in (Off(), Absent()):
        assert fcc.write_cell_summary(eng, None, fn, names) is None
        assert not os.path.exists(fn)

    class On(object):
        def cell_summary(self, mode=None):
            assert mode == BASEFC
            return dict(fate=fate, matrix=matrix, fate_cols=U.COLS, matrix_cols=capi.CELL_MATRIX_COLS[BASEFC])
    got = fcc.write_cell_summary(On(), None, fn, names, BASEFC, "[test]")
    assert np.array_equal(got["fate"], fate) and np.array_equal(got["matrix"], matrix)
    with open(fn) as fp:
        assert fp.read() == fcc.cell_summary_text(names, fate, matrix, U.COLS, capi.CELL_MATRIX_COLS[BASEFC])


def test_fixtures_pair_up_and_sum_to_the_global_counters():
    assert U.list_fixtures() == R.list_fixtures() and len(U.list_fixtures()) >= 11
    sizes = {"c1": 1000, "dense": 40, "multibam": 50, "special": 4, "well": 6}
    for name in U.list_fixtures():
        fx = R.load_fixture(name)
        cx, tab = U.load_cell_fixture(name)
        assert len(cx["cells"]) == sizes[cx["dataset"]] and tab.shape == (sizes[cx["dataset"]] + 1, 12)
        assert cx["cells"] == sorted(cx["cells"])                # the engine's column order
        assert [int(v) for v in tab.sum(axis=0)] == [fx["fate"][k] for k in U.COLS], name
        assert not tab[:-1, U.NO_CELL].any() and not tab[-1, U.NO_UMI:].any()
        assert os.path.getsize(os.path.join(U.CDIR, name + ".json")) < 100 * 1024


def test_restatement_on_a_hand_made_batch():
    """the plain-Python classification the GPU tests compare with, on reads whose classes can be told by eye"""
    M, N, S = 0, 3, 4
    regions = [("1", 101, 200, "a"), ("1", 151, 300, "b"), ("1", 151, 300, "b_again")]
    snps = [("1", 120, "A", "C", 0, 1), ("1", 145, "A", "C", 0, 1), ("2", 5, "A", "C", 0, 1)]
    filt = dict(min_mapq=20, min_len=30, excl_flag=772, incl_flag=0, no_orphan=True, min_include=0.9)
    reads = [  # pos, flag, mapq, cell, umi, cigar
        (100, 0, 19, 0, 1, [(M, 50)]),                # low_mapq
        (100, 4, 60, 0, 1, [(M, 50)]),                # excl_flag
        (100, 1, 60, 0, 1, [(M, 50)]),                # orphan
        (100, 0, 60, -1, 1, [(M, 50)]),               # no_cell -> the `*` row
        (100, 0, 60, 1, U.UMI_NONE, [(M, 50)]),       # no_umi
        (100, 0, 60, 1, 1, [(S, 30), (M, 20)]),       # short_aligned
        (100, 0, 60, 1, 1, [(M, 50)]),                # inside a alone, covers both SNPs
        (160, 0, 60, 1, 1, [(M, 40)]),                # inside a, b and b_again
        (90, 0, 60, 0, 1, [(M, 50)]),                 # 40 of 50 bases in a: include_fail; covers SNP 120 only
        (400, 0, 60, 0, 1, [(M, 20), (N, 100), (M, 20)]),   # no region, no SNP
    ]
    cig_off, words = [0], []
    for r in reads:
        words += [(l << 4) | op for op, l in r[5]]
        cig_off.append(len(words))
    b = dict(contig=0, pos=np.array([r[0] for r in reads]), flag=np.array([r[1] for r in reads]), mapq=np.array([r[2] for r in reads]),
             cell=np.array([r[3] for r in reads]), umi=np.array([r[4] for r in reads], dtype=np.uint64), cig_off=np.array(cig_off),
             cigar=np.array(words))
    tab, nj = U.restate(["1", "2"], regions, snps, 2, [b, dict(b, contig=1)], filt, True)
    assert nj == len(reads)                                    # contig "2" has no region
    want = np.zeros((3, 12), dtype=np.int64)
    want[0, [U.LOW_MAPQ, U.EXCL_FLAG, U.ORPHAN, U.INCLUDE_FAIL, U.NO_TARGET]] = 1
    want[1, [U.NO_UMI, U.SHORT]] = 1
    want[1, U.ASSIGNED], want[1, U.MULTI], want[1, U.PAIRS] = 2, 1, 4
    want[2, U.NO_CELL] = 1
    assert np.array_equal(tab, want), tab
    tab, nj = U.restate(["1", "2"], regions, snps, 2, [b], filt, False)
    assert nj == 0
    want[0, U.INCLUDE_FAIL], want[0, U.NO_TARGET] = 0, 1
    want[0, U.ASSIGNED], want[0, U.PAIRS] = 1, 1
    want[1, U.ASSIGNED], want[1, U.MULTI], want[1, U.PAIRS] = 1, 1, 2
    want[1, U.NO_TARGET] = 1
    assert np.array_equal(tab, want), tab
