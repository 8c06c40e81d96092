"""The opt-in tag filter (xck_config.filter_tag / XCK_TAG_FILTER, include/xck.h) through the engine: the matrices of a filtered run over a
file are, bit for bit, those of an unfiltered run over the file without the failing records - whether the host parses the chunks
(XCK_GPU_INFLATE=0: csrc/bam_records.cpp parse_record) or the device does (csrc/parse_dev.hip k_parse, which also counts what it filters).
The verdicts and the pre-filtered files are Python's (tests/tag_filter_cases.py: oracle/pybam.py's records, copied bytes), the expected
matrices the unchanged oracle's over the pre-filtered file.  Reference boundary: pysam's get_tag (first occurrence, the value for a
numeric type) as restated by oracle/pybam.py, and `samtools view -d xf:25` for what the exact predicate keeps."""
import os

import numpy as np
import pytest

import device_decode_cases as D
import oracle as O
import tag_filter_cases as T
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine

pytestmark = pytest.mark.gpu

MATS = {capi.XCK_MODE_BASEFC: ("count",), capi.XCK_MODE_BAF: ("ad", "dp", "oth"), capi.XCK_MODE_BOTH: ("count", "ad", "dp", "oth")}
KNOBS = ("XCK_TAG_FILTER", "XCK_GPU_NAMES", "XCK_GPU_PARSE", "XCK_READ_FATE", "XCK_CELL_SUMMARY", "XCK_FEATURE_SUMMARY", "XCK_CELL_GROUPS")


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    """the crafted file, its tables and - made on first use, then shared and left alone - the pre-filtered file and the oracle's
    matrices for it per predicate"""
    d = tmp_path_factory.mktemp("tag_filter")
    c = T.craft(str(d))
    c["tables"] = T.tables(c)
    c["dir"], c["pre"], c["exp"] = str(d), {}, {}
    return c


def prefiltered(c, pred):
    if pred not in c["pre"]:
        value, mask = T.PREDICATES[pred]
        fn = os.path.join(c["dir"], "pre_%s.bam" % pred)
        n_keep, n_all = T.prefilter(c["bam"], fn, value, mask)
        _, ok, wanted = T.verdicts(c["bam"], c["tables"][0], value, mask)
        assert n_all == c["n_records"] and n_keep == int(ok.sum())
        c["pre"][pred] = dict(bam=fn, n_records=n_keep, n_filtered=int((~ok & wanted).sum()))
    return c["pre"][pred]


def expected(c, pred, oracle_lib):
    if pred not in c["exp"]:
        bam = prefiltered(c, pred)["bam"]
        fc = O.run_files(capi.XCK_MODE_BASEFC, [bam], c["region_fn"], barcode_fn=c["barcode_fn"])
        baf = O.run_files(capi.XCK_MODE_BAF, [bam], c["region_fn"], barcode_fn=c["barcode_fn"], snp_fn=c["snp_fn"])
        c["exp"][pred] = dict(count=fc["count"], ad=baf["ad"], dp=baf["dp"], oth=baf["oth"])
    return c["exp"][pred]


def set_parse(monkeypatch, parse):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if parse == "host":
        monkeypatch.setenv("XCK_GPU_INFLATE", "0")
    else:
        monkeypatch.setenv("XCK_GPU_INFLATE", "100")
        monkeypatch.setenv("XCK_GPU_INFLATE_MIN_MB", "0")
    monkeypatch.setenv("XCK_CHUNK_BYTES", str(T.CHUNK_BYTES))


def run(c, bam, mode, umi_tag="UB", summaries=False, **kw):
    """one engine over one file -> dict(mats, n, st, fate: {pipeline: read_fate}, cells: {pipeline: cell_summary})"""
    names, regions, snps, barcodes = c["tables"]
    eng = Engine(mode, names, regions, len(barcodes), snps=snps if mode & capi.XCK_MODE_BAF else (), barcodes=barcodes, cell_tag="CB", umi_tag=umi_tag,
                 n_threads=4, **kw)
    try:
        out = dict(n=eng.ingest_bam(bam), mats=eng.finish(), st=eng.decode_stats(), fate={}, cells={})
        if summaries:
            for m in (capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF):
                if mode & m:
                    out["fate"][m], out["cells"][m] = eng.read_fate(m), eng.cell_summary(m)
    finally:
        eng.close()
    return out


CASES = [(p, capi.XCK_MODE_BOTH) for p in sorted(T.PREDICATES)] + [("exact", capi.XCK_MODE_BASEFC), ("exact", capi.XCK_MODE_BAF)]


@pytest.mark.parametrize("parse", ["host", "device"])
@pytest.mark.parametrize("pred,mode", CASES)
def test_filtered_run_equals_the_run_over_the_prefiltered_file(crafted, pred, mode, parse, monkeypatch, oracle_lib):
    value, mask = T.PREDICATES[pred]
    pre, exp = prefiltered(crafted, pred), expected(crafted, pred, oracle_lib)
    set_parse(monkeypatch, parse)
    filt = run(crafted, crafted["bam"], mode, tag_filter=(T.TAG, value, mask))
    plain = run(crafted, pre["bam"], mode)
    full = run(crafted, crafted["bam"], mode)                                # (unfiltered, the whole file: the decode counters to compare with)
    print("tag filter %s, mode %d, %s parse: %d records, %d filtered (predicted %d); parse chunks %d / fallbacks %d, unfiltered %d / %d; nnz %s" % (
        pred, mode, parse, filt["n"], filt["st"]["tag_filtered"], pre["n_filtered"], filt["st"]["gpu_parse_chunks"], filt["st"]["gpu_parse_fallbacks"],
        full["st"]["gpu_parse_chunks"], full["st"]["gpu_parse_fallbacks"], [len(filt["mats"][m][0]) for m in MATS[mode]]))
    assert filt["n"] == full["n"] == crafted["n_records"] and plain["n"] == pre["n_records"]
    util.assert_coo_equal(filt["mats"], plain["mats"], MATS[mode])
    util.assert_coo_equal(filt["mats"], exp, MATS[mode])
    if pred == "none":
        assert all(len(filt["mats"][m][0]) == 0 for m in MATS[mode])
    else:
        assert all(0 < len(filt["mats"][m][0]) < len(full["mats"][m][0]) for m in MATS[mode] if m != "oth")
    # the filter causes no fallback and does not switch the device parse off
    for k in ("gpu_inflate_chunks", "gpu_parse_chunks", "gpu_parse_fallbacks"):
        assert filt["st"][k] == full["st"][k], k
    if parse == "device":
        pred_run = D.predict_run([crafted["bam"]], crafted["region_fn"], crafted["snp_fn"], crafted["barcode_fn"], "CB", "UB", T.CHUNK_BYTES)
        assert filt["st"]["gpu_parse_chunks"] > 0
        assert pred_run["exact"] and pred_run["fallbacks"] >= 1              # (the chunks with an N in a UMI: counted once, by their host parse)
        D.assert_stats(pred_run, D.sum_stats([filt["st"]]))
    else:
        assert filt["st"]["gpu_parse_chunks"] == 0 and filt["st"]["gpu_inflate_chunks"] == 0
    assert filt["st"]["tag_filtered"] == pre["n_filtered"]
    assert full["st"]["tag_filtered"] == 0 and plain["st"]["tag_filtered"] == 0


@pytest.mark.parametrize("parse", ["host", "device"])
def test_read_fate_counts_the_filtered_reads_as_no_cell(crafted, parse, monkeypatch):
    value, mask = T.PREDICATES["exact"]
    pre = prefiltered(crafted, "exact")
    set_parse(monkeypatch, parse)
    flags = capi.XCK_F_READ_FATE | capi.XCK_F_CELL_SUMMARY
    A = run(crafted, crafted["bam"], capi.XCK_MODE_BOTH, summaries=True, flags=flags, tag_filter=(T.TAG, value, mask))
    U = run(crafted, crafted["bam"], capi.XCK_MODE_BOTH, summaries=True, flags=flags)
    P = run(crafted, pre["bam"], capi.XCK_MODE_BOTH, summaries=True, flags=flags)
    # the filtered reads that pass the four tests ahead of the cell test (check_read: mapq, the two flag masks, orphans - the engine's
    # defaults 20, excl 772, incl 0, no_orphan), on the records as pybam reads them
    recs, ok, wanted = T.verdicts(crafted["bam"], crafted["tables"][0], value, mask)
    early = lambda r: r.mapq < 20 or (r.flag & 772) or ((r.flag & 1) and not (r.flag & 2))
    moved = sum(1 for r, o, w in zip(recs, ok, wanted) if w and not o and not early(r))
    assert 0 < moved < pre["n_filtered"]                                    # (some filtered reads also have a low MAPQ or an excluded flag)
    n_cells = len(crafted["tables"][3])
    for m in (capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF):
        a, u, p = A["fate"][m], U["fate"][m], P["fate"][m]
        print("read fate, pipeline %d, %s parse: filtered %s | unfiltered %s | pre-filtered %s" % (m, parse, a, u, p))
        for k in ("not_joined", "low_mapq", "excl_flag", "incl_flag", "orphan"):
            assert a[k] == u[k], k
        for k in ("no_umi", "short_aligned", "no_target", "include_fail", "assigned", "multi", "pairs"):
            assert a[k] == p[k], k
        assert a["no_cell"] == p["no_cell"] + moved
        assert a["n_reads"] == u["n_reads"] == sum(a[k] for k in capi.READ_FATE_CLASSES)
        assert a["low_mapq"] > 0 and a["excl_flag"] > 0 and p["no_cell"] > 0
        # the per-cell table: 12 columns, their sums the global fields; the filtered reads sit in the last row
        ca, cp = A["cells"][m], P["cells"][m]
        assert ca["fate"].shape == (n_cells + 1, 12) and ca["fate_cols"] == capi.CELL_FATE_COLS
        assert ca["fate"].sum(axis=0).tolist() == [a[k] for k in capi.CELL_FATE_COLS]
        k_nc = capi.CELL_FATE_COLS.index("no_cell")
        assert int(ca["fate"][n_cells, k_nc]) == a["no_cell"] and not ca["fate"][:n_cells, k_nc].any()
        assert np.array_equal(ca["fate"][:n_cells, k_nc + 1:], cp["fate"][:n_cells, k_nc + 1:])
        assert np.array_equal(ca["matrix"], cp["matrix"])


def test_pushed_batches_may_carry_the_sentinel(monkeypatch):
    """xck_push_batch: XCK_CELL_FILTERED in the cell column means what -1 means"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    from xcltk_amd.synth import soa
    regions, snps, names = soa.make_tables(150, 3000, [1500000], seed=4, max_len=100000)
    bs = soa.gen_reads(regions, names, 12000, 50, seed=5)
    rng = np.random.default_rng(6)
    got = {}
    for sentinel in (-1, capi.XCK_CELL_FILTERED):
        batches = []
        for b in bs:
            b = dict(b)
            cell = np.array(b["cell"], dtype=np.int32)
            cell[rng.random(len(cell)) < 0.3] = sentinel
            b["cell"] = cell
            batches.append(util.batch_from_dict(b))
        rng = np.random.default_rng(6)                                       # (the same reads lose their cell in the second round)
        for mode in (capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF):
            eng = Engine(mode, names, regions, 50, snps=snps if mode == capi.XCK_MODE_BAF else (), flags=capi.XCK_F_READ_FATE)
            try:
                for bt, _ in batches:
                    eng.push(bt)
                got[(sentinel, mode)] = (eng.finish(), eng.read_fate())
            finally:
                eng.close()
    for mode in (capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF):
        (m1, f1), (m2, f2) = got[(-1, mode)], got[(capi.XCK_CELL_FILTERED, mode)]
        util.assert_coo_equal(m2, m1, MATS[mode])
        assert f1 == f2 and f1["no_cell"] > 0 and len(m1[MATS[mode][-1 if mode == 1 else 1]][0]) > 0


def test_umi_less_handle_in_device_names_mode(crafted, monkeypatch):
    """the `--umi None` shape with barcodes kept: the key is the read name, interned on the device (XCK_GPU_NAMES=1) - also for the reads
    the filter rejects, whose keys are never used"""
    value, mask = T.PREDICATES["exact"]
    pre = prefiltered(crafted, "exact")
    set_parse(monkeypatch, "device")
    monkeypatch.setenv("XCK_GPU_NAMES", "1")
    filt = run(crafted, crafted["bam"], capi.XCK_MODE_BOTH, umi_tag=None, tag_filter=(T.TAG, value, mask))
    plain = run(crafted, pre["bam"], capi.XCK_MODE_BOTH, umi_tag=None)
    full = run(crafted, crafted["bam"], capi.XCK_MODE_BOTH, umi_tag=None)
    print("tag filter, device names: %s" % filt["st"])
    util.assert_coo_equal(filt["mats"], plain["mats"], MATS[capi.XCK_MODE_BOTH])
    assert 0 < len(filt["mats"]["count"][0]) < len(full["mats"]["count"][0])
    assert filt["st"]["gpu_parse_chunks"] > 0 and filt["st"]["gpu_names_interned"] > 0
    for k in ("gpu_parse_chunks", "gpu_parse_fallbacks", "gpu_names_interned", "gpu_names_distinct", "gpu_names_host_chunks"):
        assert filt["st"][k] == full["st"][k], k                             # (the names of filtered reads are interned all the same)
    assert filt["st"]["tag_filtered"] == pre["n_filtered"]


@pytest.mark.parametrize("name", ["c1_basefc_default", "c1_baf_allreg"])
def test_frontends_follow_the_knob(name, tmp_path, monkeypatch, caplog):
    """fc_wrapper / afc_wrapper with XCK_TAG_FILTER over a golden BAM that was given xf tags write what they write, without the knob, from
    the pre-filtered BAM; without the knob the tagged file gives the golden case's reference output (a tag nobody asks for changes nothing)"""
    import logging
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_wrapper
    for k in KNOBS + ("XCK_GPU_INFLATE", "XCK_CHUNK_BYTES"):
        monkeypatch.delenv(k, raising=False)
    wrapper = fc_wrapper if name == "c1_basefc_default" else afc_wrapper
    src = os.path.join(util.GOLDEN, "datasets", D.dataset_of(name))
    tagged, pre = str(tmp_path / "tagged"), str(tmp_path / "pre")
    T.copy_dataset(src, tagged, lambda s, d: T.tag_records(s, d))
    n = {}
    T.copy_dataset(tagged, pre, lambda s, d: n.update(kept=T.prefilter(s, d, 25, T.ALL, block_records=200)))
    assert 0 < n["kept"][0] < n["kept"][1]
    # what the log line must say: the failing records on the contigs of the front-end's tables (the others reach no batch)
    regions, snps = util.load_tables(tagged)
    names = O.contig_table(regions, snps if name == "c1_baf_allreg" else ())
    _, ok, wanted = T.verdicts(os.path.join(tagged, "possorted.bam"), names, 25, T.ALL)
    n_filtered = int((~ok & wanted).sum())
    assert n_filtered > 0
    outs = {}
    for what, ddir, knob in (("knob", tagged, "xf:25"), ("pre", pre, None), ("off", tagged, None)):
        os.makedirs(str(tmp_path / what), exist_ok=True)
        case, _, odir, exp = util.load_case(name, tmp_path / what, ddir)
        if knob:
            monkeypatch.setenv("XCK_TAG_FILTER", knob)
        else:
            monkeypatch.delenv("XCK_TAG_FILTER", raising=False)
        with caplog.at_level(logging.INFO):
            caplog.clear()
            assert wrapper(**case["kwargs"]) == 0
            lines = [r.getMessage() for r in caplog.records if "tag filter" in r.getMessage()]
        assert len(lines) == (1 if knob else 0), lines
        if knob:
            assert "xf" in lines[0] and "%d record(s) filtered out" % n_filtered in lines[0]
        outs[what] = odir
    util.assert_dirs_equal(outs["knob"], outs["pre"])
    util.assert_dirs_equal(outs["off"], exp)
    changed = "matrix.mtx" if name == "c1_basefc_default" else "xcltk.DP.mtx"
    assert open(os.path.join(outs["knob"], changed), "rb").read() != open(os.path.join(exp, changed), "rb").read()   # (the filter did something)
