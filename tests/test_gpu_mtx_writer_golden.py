"""The two ways xck_write_mtx has into its file (csrc/mtx_writer.cpp: the pipeline, the default; mapped, XCK_WRITE_MAP=1) behind the
product's front-ends: one golden 10x data set through fc_wrapper and afc_wrapper each way, at a chunk size that cuts its matrices into
dozens of chunks.  Both output trees must be, byte for byte, what the unmodified reference wrote (tests/golden/cases/*/expected) - and
so each other's.  Reference boundary: the reference's recorded outputs."""
import pytest

import util

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["c1_basefc_default", "c1_baf_allreg"])
def test_frontends_write_the_reference_bytes_through_either_writer(name, tmp_path, monkeypatch):
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_wrapper
    monkeypatch.setenv("XCK_WRITE_CHUNK_ENTRIES", "64")
    monkeypatch.setenv("XCK_WRITE_THREADS", "4")
    trees = []
    for knob in (None, "1"):
        if knob is None:
            monkeypatch.delenv("XCK_WRITE_MAP", raising=False)
        else:
            monkeypatch.setenv("XCK_WRITE_MAP", knob)
        sub = tmp_path / ("map_" + (knob or "default"))
        sub.mkdir()
        case, ddir, odir, exp = util.load_case(name, sub)
        assert (fc_wrapper if case["kind"] == "basefc" else afc_wrapper)(**case["kwargs"]) == 0
        util.assert_dirs_equal(odir, exp)
        trees.append(odir)
    util.assert_dirs_equal(trees[0], trees[1])
