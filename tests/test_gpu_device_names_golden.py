"""The UMI-less golden cases through the device-names mode (XCK_GPU_NAMES=1, csrc/intern_dev.hip): the five cases whose key is the read
name - class "inflate-only" of tests/device_decode_cases.py under the default environment - run through their front-ends over the
golden BAMs re-cut into small record-aligned blocks (tests/reblock.py), with every chunk of 64 blocks and more inflated, walked and
parsed on the device and every read name keyed by the handle's device table, and must write, byte for byte, what the unmodified
reference wrote for the original files.  xck_decode_stats, summed over the run's engines: no chunk fell back, and the device parsed
exactly the chunks predicted from the files' blocks and records as oracle/pybam.py reads them (tests/test_device_names_cases_host.py
checks on the CPU that every case has such a chunk).  Reference boundary: the reference's recorded outputs (tests/golden/cases/*/expected)."""
import pytest

import device_decode_cases as D
import util

pytestmark = pytest.mark.gpu
CASES = ("c1_basefc_noumi", "c1_baf_noumi", "well_basefc", "well_basefc_orphan", "well_baf")


@pytest.fixture
def device_names(monkeypatch):
    """-> list that receives the decode stats of every engine of the run when it is closed"""
    from xcltk_amd import engine
    seen = []

    def close(self, _orig=engine.Engine.close):
        if getattr(self, "h", None):
            seen.append(self.decode_stats())
        return _orig(self)
    monkeypatch.setattr(engine.Engine, "close", close)
    monkeypatch.setenv("XCK_GPU_NAMES", "1")
    monkeypatch.setenv("XCK_GPU_INFLATE", "100")
    monkeypatch.setenv("XCK_GPU_INFLATE_MIN_MB", "0")
    for k in ("XCK_GPU_PARSE", "XCK_GPU_INFLATE_RING", "XCK_GPU_NAMES_SLOTS0", "XCK_GPU_NAMES_ARENA0", "XCK_TEST_NAMES_HASH_BITS", "WORLD_SIZE", "XCK_DIST_FORCE"):
        monkeypatch.delenv(k, raising=False)
    return seen


def _frontend(case):
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_main, fc_wrapper
    if "argv" in case:
        return fc_main(["xcltk", "basefc"] + case["argv"])
    return fc_wrapper(**case["kwargs"]) if case["kind"] == "basefc" else afc_wrapper(**case["kwargs"])


@pytest.mark.parametrize("name", CASES)
def test_noumi_golden_case_with_device_names(name, tmp_path, monkeypatch, device_names):
    case, ddir, odir, exp, chunk_bytes, _ = D.recut_case(name, tmp_path)
    monkeypatch.setenv("XCK_CHUNK_BYTES", str(chunk_bytes))
    p = util.oracle_params(case)
    assert D.predict_case(case, chunk_bytes)["cls"] == "inflate-only"      # (what the knob changes)
    # the chunks the device takes, and those of them with a block of more than DP_MAX_RUNS contig runs (which fall back): predict_run
    # counts both when no record carries the tag it is asked about
    pred = D.predict_run(p["bam_fns"], p["region_fn"], p["snp_fn"] if case["kind"] != "basefc" else None, p["barcode_fn"], p["cell_tag"], "ZZ", chunk_bytes)
    assert _frontend(case) == 0
    util.assert_dirs_equal(odir, exp)
    keys = ("gpu_inflate_chunks", "gpu_parse_chunks", "gpu_parse_fallbacks", "gpu_names_interned", "gpu_names_distinct", "gpu_names_host_chunks")
    st = {k: sum(int(s[k]) for s in device_names) for k in keys}
    print("device names: %s: engines %d, predicted %s, stats %s" % (name, len(device_names), pred, st))
    assert st["gpu_parse_fallbacks"] == 0
    assert st["gpu_parse_chunks"] == pred["device_chunks"] - pred["fallbacks"] and st["gpu_parse_chunks"] > 0
    assert st["gpu_names_interned"] > 0 and st["gpu_names_distinct"] > 0
