"""xck_group_counts without a GPU: the symbol and its answer on a decode-only handle, the group-file parser of XCK_CELL_GROUPS
(fc_common.parse_cell_groups), and the numpy expected-value function of the GPU tests on an example small enough to check by hand."""
import ctypes as C
import logging

import numpy as np
import pytest

import group_util as G
from xcltk_amd import capi
from xcltk_amd import fc_common as fcc
from xcltk_amd.engine import Engine, XckError


def test_library_exports_the_call(lib):
    assert hasattr(lib, "xck_group_counts")
    assert ("xck_group_counts", C.c_int, [C.c_void_p, C.POINTER(capi.GroupConfig), C.POINTER(capi.Result)]) in capi.SYMBOLS
    assert lib.xck_abi_version() == 3                                    # additive
    assert C.sizeof(capi.GroupConfig) == 24 and capi.XCK_GROUP_MAX == 4096


def test_decode_only_handle_answers_state():
    snps = [("1", 100, "A", "C", 0, 1)]
    with Engine(capi.XCK_MODE_BAF, ["1"], [("1", 1, 500, "g")], 4, snps=snps, decode_only=True) as eng:
        for source in ("result", "snp"):
            with pytest.raises(XckError) as ei:
                eng.group_counts([0, 1, -1, 0], source=source)
            assert ei.value.code == capi.XCK_E_STATE
            assert b"decode-only" in eng.lib.xck_last_error(eng.h)
        res = capi.Result()
        assert eng.lib.xck_group_counts(eng.h, None, C.byref(res)) == capi.XCK_E_ARG
        cfg = capi.GroupConfig()
        assert eng.lib.xck_group_counts(eng.h, C.byref(cfg), C.byref(res)) == capi.XCK_E_ARG   # struct_size 0
        with pytest.raises(ValueError):
            eng.group_counts([0, 1])                                     # one entry per cell


CELLS = ["AAAC", "AAAG", "AACA", "AACC", "AACG"]                         # a run's cells, in column order


def test_parser_numbers_groups_by_first_appearance():
    lines = ["AACC\ttumour\n", "AAAC\tnormal\n", "AACG\ttumour\n", "AAAG\tstroma\n"]
    names, cg, ignored = fcc.parse_cell_groups(lines, CELLS)
    assert names == ["tumour", "normal", "stroma"]
    assert cg.dtype == np.int32 and cg.tolist() == [1, 2, -1, 0, 0]      # AACA is not named: left out
    assert ignored == 0


def test_parser_ignores_unknown_names_and_counts_them(tmp_path, monkeypatch, caplog):
    lines = ["TTTT\tother\n", "AAAC\ta\n", "GGGG\ta\n", "\n", "AACA\tb\r\n", "AAAC\ta\n"]   # a blank line, CRLF, a repeated line
    names, cg, ignored = fcc.parse_cell_groups(lines, CELLS)
    assert names == ["other", "a", "b"]                                  # numbered by the file, whoever is in the run
    assert cg.tolist() == [1, -1, 2, -1, -1] and ignored == 2
    fn = tmp_path / "groups.tsv"
    fn.write_text("".join(lines))
    monkeypatch.setenv("XCK_CELL_GROUPS", str(fn))
    with caplog.at_level(logging.INFO):
        got = fcc.load_cell_groups(CELLS)
    assert got[0] == names and got[1].tolist() == cg.tolist()
    assert any("2 names ignored" in r.getMessage() for r in caplog.records)
    monkeypatch.delenv("XCK_CELL_GROUPS")
    assert fcc.load_cell_groups(CELLS) is None                           # the knob unset: nothing
    monkeypatch.setenv("XCK_CELL_GROUPS", str(tmp_path / "missing.tsv"))
    with pytest.raises(ValueError):
        fcc.load_cell_groups(CELLS)


def test_parser_rejects_a_name_in_two_groups_and_too_many_groups():
    with pytest.raises(ValueError, match="two groups"):
        fcc.parse_cell_groups(["AAAC\ta\n", "AAAG\tb\n", "AAAC\tb\n"], CELLS)
    with pytest.raises(ValueError, match="two groups"):
        fcc.parse_cell_groups(["ZZZZ\ta\n", "ZZZZ\tb\n"], CELLS)            # also for a name outside the run
    with pytest.raises(ValueError):
        fcc.parse_cell_groups(["AAAC\n"], CELLS)
    many = ["c%d\tg%d\n" % (i, i) for i in range(capi.XCK_GROUP_MAX + 1)]
    with pytest.raises(ValueError, match="more than 4096"):
        fcc.parse_cell_groups(many, CELLS)
    names, cg, ignored = fcc.parse_cell_groups(many[:-1], ["c5", "c4095"])
    assert len(names) == 4096 and cg.tolist() == [5, 4095] and ignored == 4094


def test_parser_on_the_empty_file():
    names, cg, ignored = fcc.parse_cell_groups([], CELLS)
    assert names == [] and cg.tolist() == [-1] * 5 and ignored == 0


def test_aggregate_on_a_hand_written_example():
    """3 rows x 4 cells, cells 0 and 2 in group 1, cell 1 in group 0, cell 3 left out:
           cells  0  1  2  3          groups  0  1
       row 0      5  .  2  9    ->    row 0   .  7
       row 1      .  .  .  4    ->    row 1   .  .     (its only cell is left out)
       row 2      1  3  .  .    ->    row 2   3  1     (group 0 before group 1, though cell 0 comes first)"""
    coo = (np.array([0, 0, 0, 1, 2, 2], np.int32), np.array([0, 2, 3, 3, 0, 1], np.int32), np.array([5, 2, 9, 4, 1, 3], np.int32))
    row, col, val = G.aggregate(coo, [1, 0, 1, -1])
    assert row.tolist() == [0, 2, 2] and col.tolist() == [1, 0, 1] and val.tolist() == [7, 3, 1]
    assert all(a.dtype == np.int32 for a in (row, col, val))
    ident = G.aggregate(coo, [0, 1, 2, 3])
    assert all(np.array_equal(a, b) for a, b in zip(ident, coo))
    assert all(len(a) == 0 for a in G.aggregate(coo, [-1, -1, -1, -1]))
    z = np.zeros(0, np.int32)
    assert all(len(a) == 0 for a in G.aggregate((z, z, z), [0, 0, 0, 0]))
