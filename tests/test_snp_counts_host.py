"""xck_snp_counts and the one-pass `xcltk baf` without a GPU: the symbol and its answer on a decode-only handle, the fall-back
decision of baf/onepass.py case by case, and pipeline_wrapper taking exactly the two-pass functions when a reason is present."""
import ctypes as C
import os

import pytest

import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine

DS = os.path.join(util.GOLDEN, "datasets", "phasing")


def test_library_exports_the_call(lib):
    assert hasattr(lib, "xck_snp_counts")
    assert ("xck_snp_counts", C.c_int, [C.c_void_p, C.POINTER(capi.Result)]) in capi.SYMBOLS
    assert lib.xck_abi_version() == 3                                    # additive


def test_decode_only_handle_answers_state():
    snps = [("1", 100, "A", "C", 0, 1)]
    with Engine(capi.XCK_MODE_BAF, ["1"], [("1", 1, 500, "g")], 4, snps=snps, decode_only=True) as eng:
        res = capi.Result()
        assert eng.lib.xck_snp_counts(eng.h, C.byref(res)) == capi.XCK_E_STATE
        assert b"decode-only" in eng.lib.xck_last_error(eng.h)
        assert eng.lib.xck_snp_counts(eng.h, None) == capi.XCK_E_ARG
        from xcltk_amd.engine import XckError
        with pytest.raises(XckError) as ei:
            eng.snp_counts()
        assert ei.value.code == capi.XCK_E_STATE


CAND = [("1", 100, "A", "C", 0, 1), ("1", 200, "G", "T", 0, 1), ("2", 100, "C", "A", 0, 1)]
PHASED = [("1", 200, "G", "T", 1, 0), ("2", 100, "C", "A", 0, 1)]
STEP = dict(sam_fn_list=["a.bam"], samples=["c1", "c2"], barcodes=["c1", "c2"], cell_tag="CB", umi_tag="UB", min_mapq=20, min_len=30,
            incl_flag=0, excl_flag=772, no_orphan=True)


def _reason(**kw):
    from xcltk_amd.baf.onepass import fallback_reason
    a = dict(dist_requested=False, snp_vcf_fn="cand.vcf.gz", phased_snp_fn="phased.tsv", cand=CAND, phased=PHASED, step1=dict(STEP), step3=dict(STEP), env={})
    a.update(kw)
    return fallback_reason(**a)


def test_fall_back_decision():
    assert _reason() is None                                             # the plain case
    assert _reason(env={"XCK_READ_FATE": "0", "XCK_CELL_SUMMARY": ""}) is None
    assert "multi-GPU" in _reason(dist_requested=True)
    assert "snp_vcf_fn is None" in _reason(snp_vcf_fn=None)
    assert "phased" in _reason(phased_snp_fn=None)
    assert "1:100 appears twice" in _reason(cand=CAND + [("1", 100, "A", "G", 0, 1)])
    assert "phased SNP 2:300 is not among" in _reason(phased=PHASED + [("2", 300, "A", "G", 0, 1)])
    for k, v, what in (("excl_flag", 1796, "read filters"), ("min_mapq", 0, "read filters"), ("umi_tag", None, "tags"), ("no_orphan", False, "read filters"),
                       ("samples", ["c1"], "cell lists"), ("barcodes", None, "cell lists"), ("sam_fn_list", ["b.bam"], "BAM lists")):
        r = _reason(step3=dict(STEP, **{k: v}))
        assert r is not None and what in r, (k, r)
    for knob in ("XCK_READ_FATE", "XCK_CELL_SUMMARY", "XCK_FEATURE_SUMMARY"):
        assert knob in _reason(env={knob: "1"})
    assert _reason(cand=None, phased=None, step1=None, step3=None) is None   # the early call: nothing loaded yet


def _two_pass_calls(monkeypatch, tmp_path, **kw):
    """pipeline_wrapper on the `phasing` dataset with pileup and baf_fc replaced by recorders: -> (return code, calls)"""
    from xcltk_amd.baf import genotype as G
    from xcltk_amd.baf import pipeline as P
    calls = []

    def fake_pileup(**k):
        calls.append(("pileup", k["out_dir"], k["min_count"], k["min_maf"]))
        return "vcf", 5, 3

    def fake_fc(**k):
        calls.append(("baf_fc", k["out_dir"], k["cellsnp_dir"], k["output_all_reg"]))
        return 0
    monkeypatch.setattr(G, "pileup", fake_pileup)
    monkeypatch.setattr(P, "baf_fc", fake_fc)
    args = dict(sam_fn=os.path.join(DS, "possorted.bam"), barcode_fn=os.path.join(DS, "barcodes.tsv"),
                snp_vcf_fn=os.path.join(DS, "cellsnp", "cellSNP.base.vcf.gz"), region_fn=os.path.join(DS, "regions.tsv"),
                out_dir=str(tmp_path / "pipe"), phased_snp_fn=os.path.join(DS, "snps.tsv"), min_count=7, min_maf=0.2, ncores=1)
    args.update(kw)
    return P.pipeline_wrapper("smp", **args), calls


@pytest.mark.parametrize("case", ["switch_off", "multi_gpu", "summary_knob", "phased_outside", "no_vcf"])
def test_pipeline_takes_the_two_pass_functions_when_it_falls_back(case, monkeypatch, tmp_path, caplog):
    import logging
    caplog.set_level(logging.INFO)
    out = str(tmp_path / "pipe")
    want = [("pileup", os.path.join(out, "1_pileup"), 7, 0.2), ("baf_fc", os.path.join(out, "3_baf_fc"), os.path.join(out, "1_pileup"), True)]
    kw = {}
    monkeypatch.delenv("WORLD_SIZE", raising=False); monkeypatch.delenv("XCK_DIST_FORCE", raising=False)
    for k in ("XCK_READ_FATE", "XCK_CELL_SUMMARY", "XCK_FEATURE_SUMMARY"):
        monkeypatch.delenv(k, raising=False)
    if case == "switch_off":
        monkeypatch.delenv("XCK_BAF_ONE_PASS", raising=False)
    else:
        monkeypatch.setenv("XCK_BAF_ONE_PASS", "1")
    if case == "multi_gpu":
        monkeypatch.setenv("WORLD_SIZE", "2")
    if case == "summary_knob":
        monkeypatch.setenv("XCK_CELL_SUMMARY", "1")
    if case == "phased_outside":                                         # a phased SNP that is no candidate
        lines = open(os.path.join(DS, "snps.tsv")).read().splitlines()
        f = lines[1].split("\t")
        f[1] = str(987654321)
        kw["phased_snp_fn"] = str(tmp_path / "phased.tsv")
        open(kw["phased_snp_fn"], "w").write("\n".join(lines + ["\t".join(f)]) + "\n")
    if case == "no_vcf":
        kw["snp_vcf_fn"] = None
        want = want[1:]
        want[0] = ("baf_fc", os.path.join(out, "3_baf_fc"), None, True)
    ret, calls = _two_pass_calls(monkeypatch, tmp_path, **kw)
    assert ret == 0 and calls == want
    said = [r.getMessage() for r in caplog.records if "one-pass baf: falling back" in r.getMessage()]
    assert len(said) == (0 if case == "switch_off" else 1)               # one line naming the reason
    if case == "phased_outside":
        assert "987654321" in said[0]
    assert not os.path.exists(os.path.join(out, "1_pileup")) and not os.path.exists(os.path.join(out, "3_baf_fc", "xcltk.AD.mtx"))
