"""The device-decoded ingest (k_inflate -> k_walk -> k_scan -> k_parse -> engine_push_parsed -> joins -> folds: the path of every large
BAM with a UMI tag) against sources outside the product: every golden case, the fused front-end and an index-range ingest run over
the golden BAMs re-cut into small record-aligned BGZF blocks (tests/reblock.py), so that their chunks hold the 64 blocks and more that
send them to the device, and must write, byte for byte, what the unmodified reference wrote for the original files - an independent
reader does not care how a file is blocked (tests/test_device_decode_cases_host.py checks that, and every other condition these tests
rest on, on the CPU).  xck_decode_stats, summed over the engines of a run, says that the device path ran, and how each chunk went:
predicted per chunk from the records as oracle/pybam.py reads them (tests/device_decode_cases.py), not from the product.
Reference boundary: the reference's recorded outputs (tests/golden/cases/*/expected), and pysam's record iteration and get_tag as
restated by oracle/pybam.py with the counting of oracle/xck_oracle.c.

The classes: clean - a UMI tag, barcodes of at most 18 bytes, every UMI on a wanted contig codable in 2 bits per base: device parse
on every device chunk, no fallback; odd - some chunk holds a UMI the device leaves to the host (c1, dense and multibam hold a UMI with
N in every few hundred records, special a numeric one): that chunk falls back, whichever way a chunk went the bytes are the
reference's; inflate-only - no UMI tag: device inflate feeds the host walk."""
import os

import numpy as np
import pytest

import device_decode_cases as D
import oracle as O
import pybam
import reblock
import util
from xcltk_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture
def device_decode(monkeypatch):
    """Every chunk of 64 blocks and more goes to the device, whatever the file's size; -> list that receives the decode stats of
    every engine of the run when it is closed."""
    from xcltk_amd import engine
    seen = []

    def close(self, _orig=engine.Engine.close):
        if getattr(self, "h", None):
            seen.append(self.decode_stats())
        return _orig(self)
    monkeypatch.setattr(engine.Engine, "close", close)
    monkeypatch.setenv("XCK_GPU_INFLATE", "100")
    monkeypatch.setenv("XCK_GPU_INFLATE_MIN_MB", "0")
    for k in ("XCK_GPU_PARSE", "XCK_GPU_INFLATE_RING", "WORLD_SIZE", "XCK_DIST_FORCE"):
        monkeypatch.delenv(k, raising=False)
    return seen


def _frontend(case):
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_main, fc_wrapper
    if "argv" in case:
        return fc_main(["xcltk", "basefc"] + case["argv"])
    return fc_wrapper(**case["kwargs"]) if case["kind"] == "basefc" else afc_wrapper(**case["kwargs"])


def _report(what, pred, seen):
    st = D.sum_stats(seen)
    print("device decode: %s: class %s, engines %d, inflate chunks %d (predicted %d), parse chunks %d (%d), fallbacks %d (%d)" % (
        what, pred["cls"], len(seen), st["gpu_inflate_chunks"], pred["device_chunks"], st["gpu_parse_chunks"], pred["parse_chunks"],
        st["gpu_parse_fallbacks"], pred["fallbacks"]))
    return st


@pytest.mark.parametrize("name", util.list_cases())
def test_golden_case_through_the_device_decoder(name, tmp_path, monkeypatch, device_decode):
    case, ddir, odir, exp, chunk_bytes, _ = D.recut_case(name, tmp_path)
    monkeypatch.setenv("XCK_CHUNK_BYTES", str(chunk_bytes))
    pred = D.predict_case(case, chunk_bytes)
    assert _frontend(case) == 0
    util.assert_dirs_equal(odir, exp)
    D.assert_stats(pred, _report(name, pred, device_decode), len(device_decode))


@pytest.mark.parametrize("pair", [("c1_basefc_default", "c1_baf_allreg"), ("dense_basefc_default", "dense_baf_allreg_dup"),
                                  ("multibam_basefc", None), ("special_basefc", "special_baf")])
def test_fused_frontend_through_the_device_decoder(pair, tmp_path, monkeypatch, device_decode):
    """XCK_MODE_BOTH: one device-decoded pass feeds both pipelines (the pairs of test_fused_single_decode_matches_both_references)"""
    from xcltk_amd.fused import fused_wrapper
    fc_name, baf_name = pair
    case, ddir, odir, exp_fc, chunk_bytes, _ = D.recut_case(fc_name, tmp_path)
    monkeypatch.setenv("XCK_CHUNK_BYTES", str(chunk_bytes))
    kw, extra = case["kwargs"], {}
    if baf_name:
        bcase, _, _, exp_baf, _, _ = D.recut_case(baf_name, tmp_path)
        extra = {k: bcase["kwargs"][k] for k in ("no_dup_hap", "min_count", "min_maf") if k in bcase["kwargs"]}
        snp = bcase["kwargs"]["phased_snp_fn"]
    else:
        snp = os.path.join(ddir, "snps.tsv")
    pred = D.predict_case(case, chunk_bytes, fused_snp_fn=snp)
    out = str(tmp_path / "fused")
    assert fused_wrapper(kw["sam_fn"], kw["barcode_fn"], kw["region_fn"], snp, out, ncores=2, **extra) == 0
    util.assert_dirs_equal(os.path.join(out, "basefc"), exp_fc)
    if baf_name:
        util.assert_dirs_equal(os.path.join(out, "baf"), exp_baf)
    D.assert_stats(pred, _report("fused " + fc_name, pred, device_decode), len(device_decode))


@pytest.mark.parametrize("schedule", D.SHAPES)
@pytest.mark.parametrize("name", D.SHAPE_CASES)
def test_block_shapes(name, schedule, tmp_path, monkeypatch, device_decode):
    """The header's tail in one block with the first records (the chunk's first_skip is non-zero); the header's block alone; one record
    per block with an empty block after every third; blocks of more than 128 records (three k_parse rounds) among blocks of one.
    phasing holds codable UMIs only: every device chunk is parsed on the device, none falls back.  c1 and dense hold a UMI with N in
    every few hundred records, so the chunks with one fall back by design: the counts are then the predicted ones, chunk by chunk."""
    case, ddir, odir, exp, chunk_bytes, _ = D.recut_case(name, tmp_path, schedule)
    monkeypatch.setenv("XCK_CHUNK_BYTES", str(chunk_bytes))
    pred = D.predict_case(case, chunk_bytes)
    assert pred["exact"]
    assert _frontend(case) == 0
    util.assert_dirs_equal(odir, exp)
    st = _report("%s / %s" % (name, schedule), pred, device_decode)
    D.assert_stats(pred, st, len(device_decode))
    if pred["fallbacks"] == 0:
        assert st["gpu_parse_chunks"] > 0 and st["gpu_parse_fallbacks"] == 0


@pytest.mark.parametrize("which", ["c1", "crafted"])
def test_index_ranges_on_a_recut_file(which, tmp_path, monkeypatch, device_decode, oracle_lib):
    """A file re-cut through BamWriter, with the .bai that belongs to the re-cut file: a XCK_MODE_BOTH engine reads the index ranges
    of the contigs a mask keeps; the matrices are the oracle's on pybam's records with the other contigs mapped to -1.  c1 has one
    contig, which the mask keeps; the crafted file (tests/device_decode_cases.py) has three the tables know, of which the mask keeps
    the first and the last, and one they do not know."""
    from xcltk_amd.engine import Engine
    bam = str(tmp_path / "recut.bam")
    if which == "c1":
        ds = os.path.join(util.GOLDEN, "datasets", "c1")
        src, region_fn, snp_fn, barcode_fn, payload, chunk_bytes = (os.path.join(ds, "possorted.bam"), os.path.join(ds, "regions.tsv"), os.path.join(ds, "snps.tsv"),
                                                                    os.path.join(ds, "barcodes.tsv"), 3000, D.INDEXED_CHUNK_BYTES)
    else:
        c = D.craft(str(tmp_path / "crafted"), 23, False)
        src, region_fn, snp_fn, barcode_fn, payload, chunk_bytes = c["bam"], c["region_fn"], c["snp_fn"], c["barcode_fn"], 3000, D.INDEXED_CHUNK_BYTES
    reblock.reblock_bam_indexed(src, bam, payload)
    monkeypatch.setenv("XCK_CHUNK_BYTES", str(chunk_bytes))
    regions, snps = O.load_regions(region_fn), O.load_snps(snp_fn)
    with open(barcode_fn) as fp:
        barcodes = sorted(x.strip() for x in fp)
    names = O.contig_table(regions, snps)
    refs, recs = pybam.read_bam(bam)
    t2c = O.resolve_contigs([n for n, _ in refs], names)
    keep = np.ones(len(names), dtype=bool)
    keep[1:-1] = False
    eng = Engine(capi.XCK_MODE_BOTH, names, regions, len(barcodes), snps=snps, barcodes=barcodes, cell_tag="CB", umi_tag="UB", n_threads=4)
    try:
        n = eng.ingest_bam(bam, contig_mask=keep, use_index=True)
        got = eng.finish()
        umi_bits = eng.umi_bits
    finally:
        eng.close()
    masked = [c if c >= 0 and keep[c] else -1 for c in t2c]
    assert (which == "c1") == (masked == t2c)
    assert n > 0
    cell_index = {b: i for i, b in enumerate(barcodes)}
    exp = {}
    for mode in (capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF):
        cfg, keepalive = O.make_config(mode, names, regions, snps if mode == capi.XCK_MODE_BAF else [], len(barcodes))
        batches = O.encode_bam(recs, masked, 0, cell_index, "CB", "UB", umi_bits, {}, with_seq=True)
        exp.update({k: v for k, v in O.run_oracle(cfg, [b for b, _ in batches]).items()
                    if k in (("count",) if mode == capi.XCK_MODE_BASEFC else ("ad", "dp", "oth"))})
    util.assert_coo_equal(got, exp, ("count", "ad", "dp", "oth"))
    assert len(exp["count"][0]) > 1000 and len(exp["dp"][0]) > 100
    st = D.sum_stats(device_decode)
    print("device decode: index ranges on re-cut %s:" % which, st)
    assert st["gpu_inflate_chunks"] > 0 and st["gpu_parse_chunks"] > 0
