"""The front-ends at small XCK_CHUNK_BYTES on the GPU: the golden BAMs then fall into many chunks, most of them stitched serially
(a record straddles the chunk boundary: dense at 4096, special at 1024) or all of them taken from the walk tasks as they are (c1 at
70000, multibam at 20000; the counts are pinned by tests/test_host_logic.py), and every chunk goes through the push thread.  The
files written must still be the reference's, byte for byte."""
import os

import pytest

import util

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,chunk_bytes", [("dense_basefc_default", 4096), ("dense_baf_default", 4096), ("special_baf", 1024),
                                               ("c1_basefc_default", 70000), ("multibam_basefc", 20000)])
def test_frontend_matches_reference_outputs_with_small_chunks(name, chunk_bytes, tmp_path, monkeypatch):
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_main, fc_wrapper
    monkeypatch.setenv("XCK_CHUNK_BYTES", str(chunk_bytes))            # (read by xck_bam_open)
    case, ddir, odir, exp = util.load_case(name, tmp_path)
    if "argv" in case:
        ret = fc_main(["xcltk", "basefc"] + case["argv"])
    elif case["kind"] == "basefc":
        ret = fc_wrapper(**case["kwargs"])
    else:
        ret = afc_wrapper(**case["kwargs"])
    assert ret == 0
    util.assert_dirs_equal(odir, exp)


def test_fused_decode_matches_both_references_with_small_chunks(tmp_path, monkeypatch):
    from xcltk_amd.fused import fused_wrapper
    monkeypatch.setenv("XCK_CHUNK_BYTES", "4096")
    case, ddir, odir, exp_fc = util.load_case("dense_basefc_default", tmp_path)
    bcase, _, _, exp_baf = util.load_case("dense_baf_allreg_dup", tmp_path)
    kw = case["kwargs"]
    extra = {k: bcase["kwargs"][k] for k in ("no_dup_hap", "min_count", "min_maf") if k in bcase["kwargs"]}
    out = str(tmp_path / "fused")
    assert fused_wrapper(kw["sam_fn"], kw["barcode_fn"], kw["region_fn"], bcase["kwargs"]["phased_snp_fn"], out, ncores=2, **extra) == 0
    util.assert_dirs_equal(os.path.join(out, "basefc"), exp_fc)
    util.assert_dirs_equal(os.path.join(out, "baf"), exp_baf)
