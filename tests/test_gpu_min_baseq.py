"""The opt-in minimum base quality of the pileup (xck_config.min_baseq / XCK_MIN_BASEQ, include/xck.h) through the
engine, against the model of tests/baseq_cases.py, which tests/test_baseq_cases_host.py holds against the pinned oracle on the CPU both
without a floor and - the masked bases rewritten as deletions - under it.  Every case runs through push_batch(qual=) and through
xck_ingest_bam of a written BAM with the host parse and with the device inflate + parse forced on, under both molecule rules: matrices,
per-SNP tallies and verdicts (xck_get_feature_summary) and the pair counters (xck_get_baseq_stats) equal the model's, and the hits and the
decoder's counters are those of the run without a floor.  Every case masks a pair that changes a matrix, so none of this passes where the
floor is not applied."""
import ctypes as C
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import baseq_cases as B
import umi_consensus_model as UM
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAF = capi.XCK_MODE_BAF
MATS = ("ad", "dp", "oth")
KNOBS = ("XCK_MIN_BASEQ", "XCK_UMI_CONSENSUS", "XCK_GPU_INFLATE", "XCK_GPU_INFLATE_MIN_MB", "XCK_GPU_PARSE", "XCK_GPU_NAMES", "XCK_CHUNK_BYTES", "XCK_HIT_CAP0",
         "XCK_HIT_SLACK", "XCK_TAG_FILTER", "XCK_READ_FATE", "XCK_CELL_SUMMARY", "XCK_FEATURE_SUMMARY", "XCK_CELL_GROUPS")
RULES = (("first", False), ("consensus", True))


def set_env(monkeypatch, c, path):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    if path == "host":
        monkeypatch.setenv("XCK_GPU_PARSE", "0")
    elif path == "device":
        monkeypatch.setenv("XCK_GPU_INFLATE", "100")
        monkeypatch.setenv("XCK_GPU_INFLATE_MIN_MB", "0")


def make(c, q, consensus=False, mode=BAF, decoder=False, **kw):
    f = dict(B.FILT); f.update(c.filt); f.update(kw)
    dec = dict(barcodes=B.BARCODES, cell_tag="CB", umi_tag="UB", n_threads=2) if decoder else {}
    return Engine(mode, c.names, c.regions, c.n_cells, snps=c.snps, flags=c.flags | capi.XCK_F_FEATURE_SUMMARY, umi_consensus=consensus, min_baseq=q, **dict(f, **dec))


def feed(eng, c, q):
    for d, qual in zip(c.batches, c.quals):
        b, keep = util.batch_from_dict(d)
        if q:
            eng.push_batch(b, qual=qual)
        else:
            eng.push(b)
    return eng.finish()


def same(got, m, what=""):
    for k in MATS:
        for j, col in enumerate(("row", "col", "val")):
            e = getattr(m, k)[j] if not isinstance(m, dict) else m[k][j]
            assert np.array_equal(np.asarray(got[k][j]), e), "%s %s.%s differs from the model" % (what, k, col)


def check(eng, got, m, q, what):
    same(got, m, what)
    snp = eng.feature_summary(BAF)["snp"]
    assert np.array_equal(snp[:, 1:6], m.tally), "%s: the per-SNP tallies differ from the model" % what
    assert np.array_equal(snp[:, 6], m.kept), "%s: snp_kept differs from the model" % what
    assert eng.baseq_stats() == dict(m.stats, min_baseq=q), what


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    """the cases as BAM files, written on first use, then shared and left alone"""
    d, made = tmp_path_factory.mktemp("baseq"), {}

    def get(name):
        if name not in made:
            made[name] = str(d / (name + ".bam"))
            B.write_bam(B.case(name), made[name])
        return made[name]
    return get


@pytest.mark.parametrize("path", ["push", "host", "device"])
@pytest.mark.parametrize("name", B.CASES)
def test_case_matches_the_model(name, path, bams, monkeypatch):
    c = B.case(name)
    set_env(monkeypatch, c, path)
    runs = {}
    for q, rule, consensus in [(0, "first", False)] + [(c.q, r, k) for r, k in RULES]:
        with make(c, q, consensus, decoder=path != "push") as eng:
            if path == "push":
                got = feed(eng, c, q)
            else:
                assert eng.ingest_bam(bams(name)) == sum(len(g) for g in c.reads)
                got = eng.finish()
            m = B.model(c, q, rule)
            st, ds = eng.stats(), eng.decode_stats()
            print(name, path, "Q", q, rule, eng.baseq_stats(), "n_hits", st["n_hits"], "launches", st["n_join_launches"], "parse chunks / fallbacks",
                  ds["gpu_parse_chunks"], ds["gpu_parse_fallbacks"], "nnz", [len(got[k][0]) for k in MATS])
            if q:
                check(eng, got, m, q, "%s %s %s" % (name, path, rule))
            else:
                same(got, m, "%s %s Q = 0" % (name, path))
                assert eng.baseq_stats() is None
            runs[(q, rule)] = (got, st, ds)
    st0, ds0 = runs[(0, "first")][1:]
    assert st0["n_hits"] == B.model(c, 0).pairs
    for (q, rule), (got, st, ds) in runs.items():
        assert st["n_hits"] == st0["n_hits"], "the floor changed the hits (%s)" % rule
        for k in ("gpu_inflate_chunks", "gpu_parse_chunks", "gpu_parse_fallbacks"):
            assert ds[k] == ds0[k], "%s differs from the run without a floor (%s)" % (k, rule)
    if path == "device":
        assert ds0["gpu_parse_chunks"] >= 1                              # the device parsed the chunk, qualities included
    elif path == "host":
        assert ds0["gpu_parse_chunks"] == 0
    if c.env and path == "push":
        assert st0["n_join_launches"] >= 2                              # the launch was replayed: the pair counters above counted its tiles once
    # the floor changed a matrix: without it the comparison above would pass on the parent
    assert not all(np.array_equal(runs[(0, "first")][0][k][j], runs[(c.q, "first")][0][k][j]) for k in MATS for j in range(3))


def test_derived_calls_follow_the_floor():
    c = B.case("paths")
    m = B.model(c, c.q)
    regions2 = [("1", 2901, 3001, "both"), ("1", 3001, 3001, "snp"), ("1", 1, 100, "none")]   # (the handle's row field holds three regions)
    with make(c, c.q) as eng:
        check(eng, feed(eng, c, c.q), m, c.q, "finish")
        sc = UM.snp_counts(c.snps, m.allele)
        same(eng.snp_counts(), sc, "snp_counts")
        group = [0, 1, 0]
        same(eng.group_counts(group, source="result"), {k: UM.group_sum(getattr(m, k), group) for k in MATS}, "group_counts")
        same(eng.group_counts(group, source="snp"), {k: UM.group_sum(sc[k], group) for k in MATS}, "group_counts snp")
        m2 = UM.fold(c.names, regions2, c.snps, c.filt, m.mols, "first")
        same(eng.refold(regions2), m2, "refold")
        assert len(m2.dp[0]) > 0 and np.array_equal(eng.feature_summary(BAF)["snp"][:, 1:6], m2.tally)
        assert eng.baseq_stats() == dict(m.stats, min_baseq=c.q)      # the counters are the join's: a refold does not touch them
        eng.reset()
        assert eng.baseq_stats() == dict(min_baseq=c.q, pairs_with_base=0, pairs_masked=0)
        same(feed(eng, c, c.q), m2, "after reset")                      # (the handle's regions follow its last refold)
        assert eng.baseq_stats() == dict(m.stats, min_baseq=c.q)


def test_fused_handle_masks_in_its_baf_half_only():
    c = B.case("paths")
    m = B.model(c, c.q)
    res = []
    for q in (0, c.q):
        with make(c, q, mode=capi.XCK_MODE_BOTH, min_include=0) as eng:
            res.append(feed(eng, c, q))
            assert (eng.baseq_stats() == dict(m.stats, min_baseq=q)) if q else (eng.baseq_stats() is None)
    same(res[1], m, "fused")
    assert len(res[0]["count"][0]) > 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res[0]["count"], res[1]["count"]))
    assert not all(np.array_equal(a, b) for a, b in zip(res[0]["dp"], res[1]["dp"]))


def test_knob_equals_the_field(monkeypatch):
    c = B.case("q13")
    set_env(monkeypatch, c, "push")
    monkeypatch.setenv("XCK_MIN_BASEQ", "13")
    with make(c, 0) as eng:                                              # the knob supplies the field
        assert eng.min_baseq == 13
        check(eng, feed(eng, c, 13), B.model(c, 13), 13, "knob")
    with make(c, 1) as eng:                                              # ... only where the field is 0
        check(eng, feed(eng, c, 1), B.model(c, 1), 1, "field over knob")
    f = dict(B.FILT)
    with Engine(capi.XCK_MODE_BASEFC, c.names, c.regions, c.n_cells, **f) as eng:   # a basefc-only handle ignores it
        assert eng.baseq_stats() is None
        eng.push(util.batch_from_dict(c.batches[0])[0])


def test_refused_calls_and_interface(bams):
    c = B.case("q13")
    b, keep = util.batch_from_dict(c.batches[0])
    qp = c.quals[0].ctypes.data_as(C.POINTER(C.c_uint8))
    with make(c, 13, decoder=True) as eng:
        lib, h = eng.lib, eng.h
        # the three calls that carry no qualities
        assert lib.xck_push_batch(h, C.byref(b)) == capi.XCK_E_STATE and b"min_baseq" in lib.xck_last_error(h)
        assert lib.xck_push_batch_device(h, C.byref(b)) == capi.XCK_E_STATE and b"min_baseq" in lib.xck_last_error(h)
        rb, refs = eng._open(bams("q13"), 1)
        try:
            o, keep2 = eng._opts(refs, 0)
            out = capi.Batch()
            assert lib.xck_bam_next_batch(h, rb, C.byref(o), C.byref(out)) == capi.XCK_E_STATE and b"min_baseq" in lib.xck_last_error(h)
        finally:
            lib.xck_bam_close(rb)
        assert eng.stats()["n_reads"] == 0                               # nothing was queued by any of them
        # xck_push_batch_q: a null qual is refused, a good one counted; the stats struct is checked
        assert lib.xck_push_batch_q(h, C.byref(b), None) == capi.XCK_E_ARG
        assert lib.xck_push_batch_q(h, C.byref(b), qp) == 0
        out = capi.BaseqStats(); out.struct_size = C.sizeof(capi.BaseqStats)
        assert lib.xck_get_baseq_stats(h, C.byref(out)) == 0 and out.min_baseq == 13 and out.pairs_with_base == B.model(c, 13).stats["pairs_with_base"]
        out.struct_size = 16
        assert lib.xck_get_baseq_stats(h, C.byref(out)) == capi.XCK_E_ARG and lib.xck_get_baseq_stats(h, None) == capi.XCK_E_ARG
    with make(c, 0) as eng:                                              # no floor: qual is ignored (NULL too), the getter says so
        lib, h = eng.lib, eng.h
        assert lib.xck_push_batch_q(h, C.byref(b), qp) == 0 and lib.xck_push_batch_q(h, C.byref(b), None) == 0
        out = capi.BaseqStats(); out.struct_size = C.sizeof(capi.BaseqStats)
        assert lib.xck_get_baseq_stats(h, C.byref(out)) == capi.XCK_E_STATE and b"min_baseq" in lib.xck_last_error(h)
    for kw in (dict(mode=capi.XCK_MODE_BASEFC), dict(decode_only=True)):
        with pytest.raises(XckError) as ei:
            Engine(kw.pop("mode", BAF), c.names, c.regions, c.n_cells, snps=c.snps, min_baseq=13, **dict(B.FILT, **kw))
        assert ei.value.code == capi.XCK_E_ARG


# ----------------------------------------------------------------------------- host and device parser: the quality region
EXE = os.path.join(ROOT, "xcltk_amd", "csrc", "xck_gpu_parse_check")


def test_parsers_agree_on_the_quality_region(tmp_path):
    """xck_gpu_parse_check with PARSE_QUAL=1 on re-cut files (tests/reblock.py): the written "lengths" case (lengths 1, 2, odd and even,
    `*`) and a golden BAM with redrawn qualities - every byte of the region, pads included, equal in both parsers"""
    import reblock
    assert os.path.isfile(EXE), "built by __graft_entry__.build() / make -C xcltk_amd/csrc"
    bc = str(tmp_path / "barcodes.tsv")
    with open(bc, "w") as fp:
        fp.write("".join(b + "\n" for b in B.BARCODES))
    src = []
    # (file, records, blocks per chunk, quality bytes of the region: two per sequence byte of the kept records - None: not predicted)
    qbytes = lambda c: sum(len(r["seq"]) + (len(r["seq"]) & 1) for g in c.reads for r in g)
    a = str(tmp_path / "lengths.bam"); B.write_bam(B.case("lengths"), a, min_blocks=0); src.append((a, 33, 8, qbytes(B.case("lengths"))))
    s = str(tmp_path / "stored.bam"); B.write_bam(B.case("stored"), s, min_blocks=0); src.append((s, 6, 2, qbytes(B.case("stored"))))
    g = str(tmp_path / "golden_q.bam"); n = B.rewrite_quals(os.path.join(util.GOLDEN, "datasets", "dense", "possorted.bam"), g); src.append((g, n, 64, None))
    for k, (fn, n_rec, per, n_q) in enumerate(src):
        cut = str(tmp_path / ("cut%d.bam" % k))
        reblock.reblock_bam(fn, cut, [200, 700, 3000], np.random.default_rng(5 + k), share_header=k == 1)
        r = subprocess.run([EXE, cut, bc], env=dict(os.environ, PARSE_QUAL="1", PARSE_CHUNK_BLOCKS=str(per)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           universal_newlines=True, timeout=120)
        line = [l for l in r.stdout.splitlines() if "records compared" in l]
        assert line, r.stdout[-2000:]
        print(line[0])
        v = [int(x) for x in re.findall(r"-?\d+", line[0])]            # chunks, records, differences, flagged, flags, without cause, quality bytes
        assert r.returncode == 0 and v[2] == 0 and v[5] == 0, r.stdout[-2000:]
        if n_q is not None:                                             # the written cases: every record and every byte of the region compared, no chunk flagged
            assert v[1] == n_rec and v[3] == 0 and v[6] == n_q, line[0]
        else:                                                           # the golden file: the chunks with a UMI to intern are flagged and left out
            assert 0 < v[1] <= n_rec and v[6] > 0, line[0]
    # the plain call prints what it always printed
    r = subprocess.run([EXE, cut, bc], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0 and "quality bytes" not in r.stdout


# ----------------------------------------------------------------------------- through a front-end
GOLDEN_CASE = "dense_baf_default"


def _model_files(case, out_dir, q):
    """what oracle.run_files does for a BAF case, with the model under the floor in the oracle's place: the BAMs read by oracle/pybam.py
    and encoded by oracle.encode_bam, their qualities by baseq_cases.record_quals -> the reference-format files in out_dir, the model"""
    import oracle as O
    import pybam
    p = util.oracle_params(case)
    assert p.pop("mode") == BAF and "phase" not in p
    regions, snps = O.load_regions(p["region_fn"]), O.load_snps(p["snp_fn"])
    with open(p["barcode_fn"]) as fp:
        samples = sorted(x.strip() for x in fp)
    excl = p["excl_flag"] if p["excl_flag"] is not None and p["excl_flag"] >= 0 else (772 if p["umi_tag"] else 1796)
    names = O.contig_table(regions, snps)
    umi_bits = O.default_umi_bits(BAF, len(regions), len(snps), len(samples))
    cell_index, intern, batches, quals = {s: i for i, s in enumerate(samples)}, {}, [], []
    for bi, fn in enumerate(p["bam_fns"]):
        refs, recs = pybam.read_bam(fn)
        rq = B.record_quals(fn)
        assert len(rq) == len(recs)
        t2c = O.resolve_contigs([n for n, _ in refs], names)
        for b, keep in O.encode_bam(recs, t2c, bi, cell_index, p["cell_tag"], p["umi_tag"], umi_bits, intern):
            d = UM.batch_dict(b, keep)
            r0 = int(d["ordinal_base"]) & ((1 << 40) - 1)
            batches.append(d); quals.append(B.qual_column(rq[r0:r0 + len(d["pos"])], d["seq_off"]))
    filt = dict(min_mapq=p["min_mapq"], min_len=p["min_len"], incl_flag=p["incl_flag"], excl_flag=excl, no_orphan=p["no_orphan"],
                min_count=p["min_count"], min_maf=p["min_maf"], no_dup_hap=p["no_dup_hap"])
    c = SimpleNamespace(names=names, regions=regions, snps=snps, batches=batches, quals=quals, filt=filt)
    mols, pairs, stats, where = B.molecules(c, q)
    m = UM.fold(names, regions, snps, filt, mols, "first")
    O.write_outputs(BAF, out_dir, regions, snps, samples, {k: getattr(m, k) for k in MATS}, p["output_all_reg"])
    return stats


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if not f.startswith(".")}


def _child(args, knob, **env_more):
    env = dict(os.environ, **env_more)
    for k in KNOBS:
        env.pop(k, None)
    if knob:
        env["XCK_MIN_BASEQ"] = str(knob)
    return subprocess.run([sys.executable] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)


def test_afc_wrapper_with_the_knob(tmp_path):
    """afc_wrapper in a child process with XCK_MIN_BASEQ=13 on a golden BAF input whose qualities were redrawn: its files are the
    model's and its log line holds the model's pair counts; with the knob unset the same input gives the committed golden bytes"""
    import tag_filter_cases as T
    worker = os.path.join(ROOT, "tests", "baseq_worker.py")
    with open(os.path.join(util.GOLDEN, "cases", GOLDEN_CASE, "case.json")) as fp:
        import json
        dataset = json.load(fp)["dataset"]
    ddir = str(tmp_path / "data")
    T.copy_dataset(os.path.join(util.GOLDEN, "datasets", dataset), ddir, lambda s, d: B.rewrite_quals(s, d, block_records=100))
    on = tmp_path / "on"; on.mkdir()
    r = _child([worker, "afc", GOLDEN_CASE, str(on), ddir], 13)
    assert "AFC_DONE" in r.stdout, r.stdout[-2000:]
    got = _files(os.path.join(str(on), "out_" + GOLDEN_CASE))
    (tmp_path / "m").mkdir()
    case, _, _, exp_dir = util.load_case(GOLDEN_CASE, str(tmp_path / "m"), ddir)
    stats = _model_files(case, str(tmp_path / "model"), 13)
    print(GOLDEN_CASE, stats)
    assert stats["pairs_masked"] > 0
    line = "min base quality 13: %d (read, SNP) pair(s) with a base, %d masked" % (stats["pairs_with_base"], stats["pairs_masked"])
    assert r.stdout.count("min base quality 13:") == 1 and line in r.stdout, [l for l in r.stdout.splitlines() if "quality" in l]
    want = _files(str(tmp_path / "model"))
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], "%s differs from the model's" % f
    assert any(got[f] != open(os.path.join(exp_dir, f), "rb").read() for f in want), "the floor changed no file"
    # without the knob: the golden bytes, from the same rewritten input
    off = tmp_path / "off"; off.mkdir()
    r = _child([worker, "afc", GOLDEN_CASE, str(off), ddir], None)
    assert "AFC_DONE" in r.stdout and "min base quality" not in r.stdout, r.stdout[-2000:]
    util.assert_dirs_equal(os.path.join(str(off), "out_" + GOLDEN_CASE), exp_dir)
