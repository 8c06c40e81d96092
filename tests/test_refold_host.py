"""Host side of xck_refold / afc_variants: what needs no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import util
from xcltk_amd import capi
from xcltk_amd.baf.fc import variants as V
from xcltk_amd.engine import Engine

UNIVERSE = [("1", 100, "A", "C", 0, 1), ("1", 200, "C", "G", 1, 0), ("2", 100, "G", "T", 0, 1), ("2", 300, "T", "A", 0, 1)]


def test_ctypes_refold_config_matches_the_header(tmp_path):
    """capi.RefoldConfig is read by xck_refold through a plain pointer: its size and field offsets must be the C header's."""
    src = tmp_path / "sz.c"
    fields = [n for n, _ in capi.RefoldConfig._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xck.h"\nint main(void) { printf("%zu", sizeof(xck_refold_config));\n'
                   + "".join('printf(" %%zu", offsetof(xck_refold_config, %s));\n' % n for n in fields) + "return 0; }\n")
    exe = tmp_path / "sz"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I", inc, "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(capi.RefoldConfig)
    assert got[1:] == [getattr(capi.RefoldConfig, n).offset for n in fields]


def test_refold_on_a_decode_only_handle_is_a_state_error():
    eng = Engine(capi.XCK_MODE_BAF, ["1"], [("1", 1, 100, "g")], 1, snps=[("1", 5, "A", "C", 0, 1)], decode_only=True)
    try:
        cfg, res = capi.RefoldConfig(), capi.Result()
        cfg.struct_size = C.sizeof(capi.RefoldConfig)
        assert eng.lib.xck_refold(eng.h, C.byref(cfg), C.byref(res)) == capi.XCK_E_STATE
        assert b"decode-only" in eng.lib.xck_last_error(eng.h)
        assert eng.lib.xck_refold(eng.h, None, C.byref(res)) == capi.XCK_E_ARG
    finally:
        eng.close()


def test_variant_snps_map_to_universe_indices_and_mask():
    own = [("2", 300, "A", "T", 1, 0), ("1", 100, "A", "C", 0, 1)]            # a subset, in its own order, with its own alleles
    idx, enabled = V.map_to_universe(UNIVERSE, own)
    assert idx.tolist() == [3, 0] and enabled.tolist() == [True, False, False, True]
    idx, enabled = V.map_to_universe(UNIVERSE, UNIVERSE)
    assert idx.tolist() == [0, 1, 2, 3] and enabled.all()
    idx, enabled = V.map_to_universe(UNIVERSE, [])
    assert len(idx) == 0 and not enabled.any()


def test_variant_snps_outside_the_universe_are_refused():
    with pytest.raises(ValueError, match="not in the SNP universe"):
        V.map_to_universe(UNIVERSE, [("1", 101, "A", "C", 0, 1)])
    with pytest.raises(ValueError, match="not in the SNP universe"):
        V.map_to_universe(UNIVERSE, [("3", 100, "A", "C", 0, 1)])
    with pytest.raises(ValueError, match="twice"):
        V.map_to_universe(UNIVERSE + [("1", 200, "A", "T", 0, 1)], UNIVERSE[:1])
    with pytest.raises(ValueError, match="twice"):
        V.map_to_universe(UNIVERSE, [UNIVERSE[0], UNIVERSE[0]])


def _dense_variants(tmp_path, snp_fn=None):
    case, ddir, odir, exp = util.load_case("dense_baf_default", tmp_path)
    kw = dict(case["kwargs"])
    common = {k: kw.pop(k) for k in ("sam_fn", "barcode_fn", "phased_snp_fn")}
    if snp_fn:
        kw["phased_snp_fn"] = snp_fn
    return common, [kw], ddir


def test_afc_variants_refuses_bad_snp_files_before_counting(tmp_path):
    """A missing and a duplicated position: ValueError, and no engine was asked for - this machine need not have a GPU."""
    common, variants, ddir = _dense_variants(tmp_path)
    lines = open(os.path.join(ddir, "snps.tsv")).read().split("\n")
    f = lines[1].split("\t")
    missing = tmp_path / "missing.tsv"
    missing.write_text("\n".join(lines[:3] + ["\t".join([f[0], "999999999"] + f[2:])]) + "\n")
    with pytest.raises(ValueError, match="not in the SNP universe"):
        V.afc_variants(*_dense_variants(tmp_path, str(missing))[:2])
    dup = tmp_path / "dup.tsv"
    dup.write_text("\n".join(lines[:3] + [lines[1]]) + "\n")
    common2 = dict(common, phased_snp_fn=str(dup))
    with pytest.raises(ValueError, match="twice"):
        V.afc_variants(common2, [dict(variants[0])])
    assert not os.path.exists(os.path.join(variants[0]["out_dir"], "xcltk.DP.mtx"))


def test_afc_variants_refuses_a_multi_gpu_environment(tmp_path, monkeypatch):
    common, variants, ddir = _dense_variants(tmp_path)
    monkeypatch.setenv("XCK_DIST_FORCE", "1")
    with pytest.raises(ValueError, match="one GPU"):
        V.afc_variants(common, variants)
    monkeypatch.delenv("XCK_DIST_FORCE")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        V.afc_variants(common, variants)
    assert not os.path.exists(variants[0]["out_dir"])                        # nothing was prepared, let alone counted
