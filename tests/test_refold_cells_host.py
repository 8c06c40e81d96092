"""Host side of the cell mask of xck_refold / Engine.refold(cell_enabled=...) / afc_variants' cell lists: what needs no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import util
from xcltk_amd import capi
from xcltk_amd.baf.fc import variants as V
from xcltk_amd.engine import Engine, XckError

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def _header_numbers(tmp_path, exprs):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xck.h"\nint main(void) {\n'
                   + "".join('printf("%%zu ", (size_t)(%s));\n' % e for e in exprs) + "return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


def test_cell_enabled_is_the_last_field_of_the_struct_in_header_and_ctypes(tmp_path):
    size, off, v1, abi = _header_numbers(tmp_path, ["sizeof(xck_refold_config)", "offsetof(xck_refold_config, cell_enabled)",
                                                   "XCK_REFOLD_CONFIG_SIZE_V1", "XCK_ABI_VERSION"])
    assert capi.RefoldConfig._fields_[-1][0] == "cell_enabled"
    assert size == C.sizeof(capi.RefoldConfig) and off == capi.RefoldConfig.cell_enabled.offset
    assert off + C.sizeof(C.c_void_p) == size                         # nothing behind it
    assert v1 == off == capi.RefoldConfig.excl_snp.offset + C.sizeof(C.c_void_p)   # the struct of the header without the field ends here
    assert abi == 3


def test_the_shorter_struct_is_still_accepted():
    """A caller built against the header without cell_enabled passes the shorter struct_size: the call gets as far as it did then - on a
    decode-only handle to XCK_E_STATE, not to the XCK_E_ARG of a struct_size mismatch.  The field behind the stated size is not read."""
    eng = Engine(capi.XCK_MODE_BAF, ["1"], [("1", 1, 100, "g")], 3, snps=[("1", 5, "A", "C", 0, 1)], decode_only=True)
    try:
        cfg, res = capi.RefoldConfig(), capi.Result()
        cfg.struct_size = capi.RefoldConfig.cell_enabled.offset
        cfg.cell_enabled = C.cast(C.c_void_p(1), C.POINTER(C.c_uint8))   # (not a pointer anyone may read)
        assert eng.lib.xck_refold(eng.h, C.byref(cfg), C.byref(res)) == capi.XCK_E_STATE
        assert b"decode-only" in eng.lib.xck_last_error(eng.h)
        cfg.cell_enabled = None
        cfg.struct_size = C.sizeof(capi.RefoldConfig)
        assert eng.lib.xck_refold(eng.h, C.byref(cfg), C.byref(res)) == capi.XCK_E_STATE
    finally:
        eng.close()


def test_engine_refold_rejects_a_mask_of_the_wrong_length_before_the_library_is_called(monkeypatch):
    eng = Engine(capi.XCK_MODE_BAF, ["1"], [("1", 1, 100, "g")], 3, snps=[("1", 5, "A", "C", 0, 1)], decode_only=True)
    try:
        calls = []
        real = eng.lib.xck_refold
        monkeypatch.setattr(eng.lib, "xck_refold", lambda *a: (calls.append(1), real(*a))[1])
        for bad in ([True, False], [True] * 4, np.ones((3, 1), bool), []):
            with pytest.raises(ValueError, match="one entry per cell"):
                eng.refold([("1", 1, 100, "g")], cell_enabled=bad)
        assert not calls                                                # the library has not been asked
        with pytest.raises(XckError) as ei:                             # the right length gets through to it (and to its state check)
            eng.refold([("1", 1, 100, "g")], cell_enabled=[True, False, True])
        assert calls == [1] and ei.value.code == capi.XCK_E_STATE
    finally:
        eng.close()


def test_renumber_columns_on_a_monotone_and_a_non_monotone_subset():
    # common cells 0 .. 5; three rows, sorted by (row, col)
    row = np.array([0, 0, 0, 1, 1, 2], np.int32); col = np.array([1, 3, 5, 0, 3, 5], np.int32); val = np.array([7, 8, 9, 1, 2, 3], np.int32)
    # monotone: the subset (1, 3, 5) in the common order -> columns 0, 1, 2; the entry of cell 0 is dropped; the order stays
    r, c, v = V.renumber_columns((row, col, val), [1, 3, 5], 6)
    assert r.tolist() == [0, 0, 0, 1, 2] and c.tolist() == [0, 1, 2, 1, 2] and v.tolist() == [7, 8, 9, 2, 3]
    # not monotone: the subset lists 5, 0, 3 -> cell 5 is column 0, cell 0 column 1, cell 3 column 2; rows are sorted again
    r, c, v = V.renumber_columns((row, col, val), [5, 0, 3], 6)
    assert r.tolist() == [0, 0, 1, 1, 2] and c.tolist() == [0, 2, 1, 2, 0] and v.tolist() == [9, 8, 1, 2, 3]
    assert all(a.dtype == np.int32 for a in (r, c, v))
    r, c, v = V.renumber_columns((row[:0], col[:0], val[:0]), [2], 6)
    assert len(r) == len(c) == len(v) == 0


def test_subset_columns():
    assert V.subset_columns(["a", "b", "c", "d"], ["d", "b"]).tolist() == [3, 1]
    with pytest.raises(ValueError, match="not in the common"):
        V.subset_columns(["a", "b"], ["a", "x"])
    with pytest.raises(ValueError, match="twice"):
        V.subset_columns(["a", "b"], ["a", "a"])


def _dense_variant(tmp_path):
    case, ddir, odir, exp = util.load_case("dense_baf_default", tmp_path)
    kw = dict(case["kwargs"])
    common = {k: kw.pop(k) for k in ("sam_fn", "barcode_fn", "phased_snp_fn")}
    return common, kw, ddir


def test_afc_variants_accepts_the_cell_list_keys():
    assert "barcode_fn" in V.VARIANT_KEYS and "sample_id_fn" in V.VARIANT_KEYS
    conf = V._variant_conf(dict(sam_fn="x.bam", barcode_fn="all.tsv"), dict(out_dir="o", region_fn="r", barcode_fn="some.tsv"))
    assert conf.barcode_fn == "all.tsv"                                 # the Config carries the common cells: the engine is made with them
    with pytest.raises(ValueError, match="cannot set"):
        V._variant_conf(dict(sam_fn="x.bam"), dict(out_dir="o", region_fn="r", cell_tag="CB"))


def test_afc_variants_refuses_a_cell_outside_the_common_list_before_counting(tmp_path):
    """ValueError, and no engine was asked for - this machine need not have a GPU."""
    common, var, ddir = _dense_variant(tmp_path)
    cells = open(os.path.join(ddir, "barcodes.tsv")).read().split()
    foreign = tmp_path / "foreign.tsv"
    foreign.write_text("\n".join(cells[:5] + ["NOT-A-CELL-1"]) + "\n")
    with pytest.raises(ValueError, match="NOT-A-CELL-1.*not in the common"):
        V.afc_variants(common, [dict(var), dict(var, out_dir=var["out_dir"] + "_b", barcode_fn=str(foreign))])
    with pytest.raises(ValueError, match="does not exist"):
        V.afc_variants(common, [dict(var, barcode_fn=str(tmp_path / "nowhere.tsv"))])
    with pytest.raises(ValueError, match="together"):
        V.afc_variants(common, [dict(var, barcode_fn=str(foreign), sample_id_fn=str(foreign))])
    assert not os.path.exists(os.path.join(var["out_dir"], "xcltk.DP.mtx"))
