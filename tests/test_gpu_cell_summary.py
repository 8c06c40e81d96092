"""Per-cell table (XCK_F_CELL_SUMMARY / XCK_CELL_SUMMARY=1, xck_get_cell_summary) on the GPU, through the C-ABI and the front-ends.

Expected values: tests/golden/cell_summary/*.json, produced by the reference's own check_read / sam_fetch / include code
(tools/make_read_fate_goldens.py); for generated inputs the plain-Python restatement of tests/cell_summary_util.py; for the matrix
half numpy.bincount over the arrays Engine.finish() returns and the .mtx files the reference wrote.  Every comparison is exact.
Invariants held on every input (_finish_and_check):
  (C1) the column sums of `fate` are the handle's xck_get_read_fate counters, low_mapq ... pairs;
  (C2) the pairs of the handle's pipelines sum to xck_stats.n_hits;
  (C3) a listed cell has no no_cell reads, and the row of the reads without a cell holds nothing beyond no_cell;
  (C4) has_matrix is 0 before the finish and 1 after it, and the matrix half equals the marginals of the finished matrices."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cell_summary_util as U
import read_fate_util as R
import util
from fuzz_cases import make_case
from xcltk_amd import capi
from xcltk_amd.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELL, FATE = capi.XCK_F_CELL_SUMMARY, capi.XCK_F_READ_FATE
BASEFC, BAF, BOTH = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF, capi.XCK_MODE_BOTH
FUZZ_SEEDS = list(range(1000, 1020)) + [1052, 1077, 1101, 1133]           # the seeds of tests/test_gpu_fuzz.py


def _pipelines(eng):
    return [BASEFC, BAF] if eng.mode == BOTH else [eng.mode]


def _finish_and_check(eng):
    """(C1) - (C4) -> {mode: (fate, matrix)}"""
    n = eng.n_cells
    for m in _pipelines(eng):
        before = eng.cell_summary(m)
        assert before["matrix"] is None and before["fate"].shape == (n + 1, 12)
    res = eng.finish()
    st = eng.stats()
    out = {}
    for m in _pipelines(eng):
        cs = eng.cell_summary(m)
        rf = eng.read_fate(m)
        fate, matrix = cs["fate"], cs["matrix"]
        assert fate.dtype == np.int64 and fate.shape == (n + 1, 12) and cs["fate_cols"] == U.COLS
        assert [int(v) for v in fate.sum(axis=0)] == [rf[k] for k in U.COLS], (m, fate.sum(axis=0), rf)
        assert not fate[:n, U.NO_CELL].any() and not fate[n, U.NO_UMI:].any() and (fate >= 0).all()
        want = U.expected_matrix(m == BASEFC, res, n)
        assert matrix is not None and matrix.dtype == np.int64 and matrix.shape == want.shape and cs["matrix_cols"] == capi.CELL_MATRIX_COLS[m]
        assert np.array_equal(matrix, want), (m, np.flatnonzero((matrix != want).any(axis=1))[:10])
        again = eng.cell_summary(m)                                      # (the cached matrix half)
        assert np.array_equal(again["fate"], fate) and np.array_equal(again["matrix"], matrix)
        out[m] = (fate, matrix)
    assert sum(int(f[:, U.PAIRS].sum()) for f, _ in out.values()) == st["n_hits"], st["n_hits"]
    return out


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[m][0], b[m][0]) and np.array_equal(a[m][1], b[m][1]) for m in a)


# ----------------------------------------------------------------------------- 1. the reference's numbers
@pytest.mark.parametrize("name", U.list_fixtures())
def test_fixture_tables_equal_the_reference(name):
    """alone and inside a XCK_MODE_BOTH handle, 64- and 128-bit keys"""
    fx = R.load_fixture(name)
    cx, want = U.load_cell_fixture(name)
    own = BASEFC if fx["mode"] == "basefc" else BAF
    for mode in (None, BOTH):
        for key128 in (False, True):
            with R.fixture_engine(fx, CELL | (capi.XCK_F_FORCE_KEY128 if key128 else 0), mode) as eng:
                if key128:
                    assert eng.stats()["key_bits"] == 128
                R.ingest_all(eng, fx)
                fate = _finish_and_check(eng)[own][0]
            bad = np.flatnonzero((fate != want).any(axis=1))
            assert bad.size == 0, (mode, key128, [(cx["cells"][i] if i < len(cx["cells"]) else "*", fate[i], want[i]) for i in bad[:5]])


def test_fixtures_are_there():
    assert len(U.list_fixtures()) >= 11 and U.list_fixtures() == R.list_fixtures()


# ----------------------------------------------------------------------------- 2. + 4. fuzz against the restatement
def _fuzz_engine(mode, case, flags):
    names, regions, snps, n_cells, batches, fc, baf, case_flags = case
    kw = dict(fc) if mode == BASEFC else dict(baf) if mode == BAF else dict(fc, **baf)
    return Engine(mode, names, regions, n_cells, snps=snps if mode & BAF else (), flags=flags, **kw)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_cases_equal_the_restatement(seed):
    """the 24 seeds of the fuzz suite (n_cells 1, 3, 40, 700, 70 000): both modes and BOTH against the per-read restatement"""
    case = make_case(seed)
    names, regions, snps, n_cells, batches, fc, baf, _ = case
    dicts = [U.batch_dict(keep, b.contig) for b, keep in batches]
    want = {BASEFC: U.restate(names, regions, (), n_cells, dicts, fc, True), BAF: U.restate(names, regions, snps, n_cells, dicts, baf, False)}
    for mode in (BASEFC, BAF, BOTH):
        with _fuzz_engine(mode, case, CELL) as eng:
            for b, _ in batches:
                eng.push(b)
            got = _finish_and_check(eng)
            for m in _pipelines(eng):
                assert eng.read_fate(m)["not_joined"] == want[m][1]
                bad = np.flatnonzero((got[m][0] != want[m][0]).any(axis=1))
                assert bad.size == 0, (mode, m, [(i, got[m][0][i], want[m][0][i]) for i in bad[:5]])


# ----------------------------------------------------------------------------- 5. the shapes at which the accumulation can go wrong
NAMES = ["1"]
REGIONS = [("1", 1001, 3000, "a"), ("1", 2001, 2600, "b"), ("1", 2001, 2600, "b2"), ("1", 5001, 5040, "c")]
SNPS = [("1", p, "A", "C", 0, 1) for p in range(1100, 6000, 23)]
FILT = dict(min_mapq=20, min_len=30, excl_flag=772, incl_flag=0, no_orphan=True, min_include=0.9)


def _shape_batch(cells, seed):
    """one batch: every class occurs, the cells are as given"""
    n = len(cells)
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, 7000, n)).astype(np.int32)
    flag = rng.choice([0, 16, 4, 1], n, p=[.6, .3, .05, .05]).astype(np.uint16)
    mapq = rng.choice([60, 19], n, p=[.9, .1]).astype(np.uint8)
    umi = rng.integers(1, 1 << 20, n).astype(np.uint64) | np.uint64(1 << 24)
    umi[rng.random(n) < 0.03] = np.uint64(capi.XCK_UMI_NONE)
    ln = rng.choice([50, 20], n, p=[.95, .05])
    cigar = ((ln << 4) | 0).astype(np.uint32)
    d = dict(contig=0, ordinal_base=0, pos=pos, flag=flag, mapq=mapq, cell=np.asarray(cells, dtype=np.int32), umi=umi,
             cig_off=np.arange(n + 1, dtype=np.uint32), cigar=cigar, seq_off=np.arange(n + 1, dtype=np.uint32) * 25,
             seq=np.full(n * 25, 0x11, dtype=np.uint8))
    return d


def _run_shape(n_cells, d):
    b, keep = util.batch_from_dict(d)
    with Engine(BOTH, NAMES, REGIONS, n_cells, snps=SNPS, flags=CELL, **FILT) as eng:
        eng.push(b)
        got = _finish_and_check(eng)
        assert eng.stats()["n_join_launches"] == 2               # one batch, one launch per pipeline
    return got


def _shape_cases():
    rng = np.random.default_rng(5)
    return {
        "a_one_cell_3_tiles_and_1": (1, np.zeros(3 * 1024 + 1, dtype=np.int32)),
        "b_1024_distinct": (1024, rng.permutation(1024)),
        "b_1025_distinct": (1025, rng.permutation(1025)),
        "d_no_cell_at_all": (7, np.full(2000, -1, dtype=np.int32)),
        "e_70000_cells_first_and_last_row": (70000, np.where(rng.random(2500) < 0.5, 0, 69999)),
        "few_cells_and_none": (3, rng.integers(-1, 3, 3000)),
    }


@pytest.mark.parametrize("shape", sorted(_shape_cases()))
def test_accumulation_shapes(shape, monkeypatch):
    """(a) - (e) of the accumulation: everything on one row over several tiles and a one-read tail; as many rows as reads (the LDS
    table at its worst case, then a second tile of one read); no listed cell at all; only the first and the last row of a large
    table.  Each again with XCK_CELL_SUMMARY_SLOTS so low that the rows of a tile do not fit: identical results."""
    n_cells, cells = _shape_cases()[shape]
    d = _shape_batch(cells, seed=len(cells))
    want = {BASEFC: U.restate(NAMES, REGIONS, (), n_cells, [d], FILT, True)[0], BAF: U.restate(NAMES, REGIONS, SNPS, n_cells, [d], FILT, False)[0]}
    assert all((w[:, :U.N_CLASSES].sum() == len(cells)) for w in want.values())
    if (np.asarray(cells) >= 0).all():
        assert all(want[BASEFC][:, c].sum() > 0 for c in (U.LOW_MAPQ, U.EXCL_FLAG, U.ORPHAN, U.SHORT, U.NO_TARGET, U.INCLUDE_FAIL, U.ASSIGNED, U.MULTI))
    monkeypatch.delenv("XCK_CELL_SUMMARY_SLOTS", raising=False)
    first = _run_shape(n_cells, d)
    for m in (BASEFC, BAF):
        bad = np.flatnonzero((first[m][0] != want[m]).any(axis=1))
        assert bad.size == 0, (m, [(i, first[m][0][i], want[m][i]) for i in bad[:5]])
    for slots in ("16", "1"):
        monkeypatch.setenv("XCK_CELL_SUMMARY_SLOTS", slots)       # read by the library at xck_create
        assert _same(_run_shape(n_cells, d), first), slots


# ----------------------------------------------------------------------------- 6. overflow replay
def test_overflow_replay_counts_once(monkeypatch):
    """XCK_HIT_CAP0 / XCK_HIT_SLACK so small that join launches overflow and are replayed: the table must not see a batch twice"""
    from test_gpu_parity import _dense_pileup_case
    regions, snps, names, batches = _dense_pileup_case(seed=21, n_reads=40000, n_cells=50, n_umis=5000, snp_step=3, span=60000, max_batch=40000, gap_max=900)
    fx = R.load_fixture("dense_basefc")

    def run_baf():
        with Engine(BAF, names, regions, 50, snps=snps, min_len=10, flags=CELL) as eng:
            for b, _ in batches:
                eng.push(b)
            return _finish_and_check(eng), eng.stats()["n_join_launches"], len(batches)

    def run_fc():
        with R.fixture_engine(fx, CELL) as eng:
            n = 0
            for d in eng.decode_bam(fx["bam_fns"][0], n_threads=2):
                eng.push(util.batch_from_dict(d)[0])
                n += 1
            return _finish_and_check(eng), eng.stats()["n_join_launches"], n

    for run in (run_baf, run_fc):
        monkeypatch.delenv("XCK_HIT_CAP0", raising=False)
        monkeypatch.delenv("XCK_HIT_SLACK", raising=False)
        want, launches, pushes = run()
        assert launches == pushes
        monkeypatch.setenv("XCK_HIT_CAP0", "64")
        monkeypatch.setenv("XCK_HIT_SLACK", "0")
        got, launches, pushes = run()
        assert launches > pushes, (launches, pushes)             # at least one launch was replayed
        assert _same(got, want)


# ----------------------------------------------------------------------------- 7. the push paths
@pytest.mark.parametrize("name", ["c1_basefc", "c1_baf", "special_baf_regions_un", "multibam_basefc"])
def test_push_paths_agree(name, monkeypatch):
    fx = R.load_fixture(name)
    with R.fixture_engine(fx, CELL) as eng:
        R.ingest_all(eng, fx)
        want = _finish_and_check(eng)
        eng.reset()                                              # zeroes the table, forgets the matrix half
        zero = eng.cell_summary()
        assert not zero["fate"].any() and zero["matrix"] is None
        for i, fn in enumerate(fx["bam_fns"]):                   # a sliced ingest (pause_records) equals one call
            with eng.open_stream(fn, sample=i, n_threads=2) as s:
                done = False
                while not done:
                    _, done = s.advance(1500)
        assert _same(_finish_and_check(eng), want)
    for stage in ("1", "0"):                                     # xck_push_batch, packed one-copy form and direct form
        monkeypatch.setenv("XCK_PUSH_STAGE", stage)
        with R.fixture_engine(fx, CELL) as eng:
            for i, fn in enumerate(fx["bam_fns"]):
                for d in eng.decode_bam(fn, sample=i, n_threads=2):
                    eng.push(util.batch_from_dict(d)[0])
            assert _same(_finish_and_check(eng), want), stage


def test_device_resident_batches_agree_with_host_batches():
    """xck_push_batch_device (the fused launch queue: several launches of up to 24 batches) against xck_push_batch of host copies"""
    import torch
    from xcltk_amd.synth import soa, soa_torch
    regions, snps, names = soa.make_tables(800, 20000, soa.HG38_LENGTHS[:4], seed=41, max_len=200000)
    arrays, contig_batches = soa_torch.gen_reads_device(regions, names, 300000, 200, seed=42, device=torch.device("cuda", 0))
    pieces = []
    for c, s, e in contig_batches:
        step = max(1, (e - s) // 9)
        pieces += [(c, a, min(e, a + step)) for a in range(s, e, step)]
    assert len(pieces) > 24
    hb = [util.batch_from_dict(soa_torch.host_batch_dict(arrays, c, s, e, True)) for c, s, e in pieces]
    for mode in (BASEFC, BAF, BOTH):
        with Engine(mode, names, regions, 200, snps=snps if mode & BAF else (), flags=CELL) as eng:
            for c, s, e in pieces:
                eng.push(soa_torch.device_batch(capi, arrays, c, s, e, bool(mode & BAF)), device_resident=True)
            dev = _finish_and_check(eng)
            assert eng.stats()["n_join_launches"] >= 2
            eng.reset()
            for b, _ in hb:
                eng.push(b)
            host = _finish_and_check(eng)
        assert _same(dev, host)
        assert all(f[:, U.ASSIGNED].sum() > 0 for f, _ in dev.values())


# ----------------------------------------------------------------------------- 8. off by default
def test_off_by_default_and_results_unchanged(monkeypatch):
    monkeypatch.delenv("XCK_CELL_SUMMARY", raising=False)
    monkeypatch.delenv("XCK_READ_FATE", raising=False)
    fx = R.load_fixture("c1_basefc")
    res = {}
    for flags in (0, FATE, CELL):
        for mode in (BASEFC, BAF):
            with R.fixture_engine(fx, flags, mode) as eng:
                R.ingest_all(eng, fx)
                res[flags, mode] = eng.finish()
                cs = capi.CellSummary()
                cs.struct_size = C.sizeof(capi.CellSummary)
                rf = capi.ReadFate()
                rf.struct_size = C.sizeof(capi.ReadFate)
                if flags != CELL:
                    assert eng.cell_summary() is None
                    assert eng.lib.xck_get_cell_summary(eng.h, mode, C.byref(cs)) == capi.XCK_E_STATE
                    # the read assignment summary keeps its own rule: there with its flag, XCK_E_STATE with neither
                    assert eng.lib.xck_get_read_fate(eng.h, mode, C.byref(rf)) == (0 if flags == FATE else capi.XCK_E_STATE)
                else:
                    assert eng.lib.xck_get_cell_summary(eng.h, mode, C.byref(cs)) == 0
                    assert (cs.mode, cs.n_cells, cs.n_fate_cols, cs.has_matrix, cs.n_matrix_cols) == (mode, 1000, 12, 1, 2 if mode == BASEFC else 4)
                    assert eng.lib.xck_get_cell_summary(eng.h, BASEFC + BAF - mode, C.byref(cs)) == capi.XCK_E_ARG   # a pipeline the handle does not have
                    assert eng.lib.xck_get_cell_summary(eng.h, BOTH, C.byref(cs)) == capi.XCK_E_ARG
                    cs.struct_size = 8
                    assert eng.lib.xck_get_cell_summary(eng.h, mode, C.byref(cs)) == capi.XCK_E_ARG
                    # the new flag alone implies the read assignment summary
                    assert eng.lib.xck_get_read_fate(eng.h, mode, C.byref(rf)) == 0 and rf.n_reads == 10000
                    assert eng.read_fate()["n_reads"] == 10000
    for mode in (BASEFC, BAF):
        for flags in (FATE, CELL):
            assert sorted(res[0, mode]) == sorted(res[flags, mode])
            for k in res[0, mode]:
                for a, b in zip(res[0, mode][k], res[flags, mode][k]):
                    assert np.array_equal(a, b), (mode, flags, k)


def test_environment_knob_sets_the_flag(monkeypatch):
    fx = R.load_fixture("special_basefc")
    cx, want = U.load_cell_fixture("special_basefc")
    monkeypatch.delenv("XCK_READ_FATE", raising=False)
    monkeypatch.setenv("XCK_CELL_SUMMARY", "1")
    with R.fixture_engine(fx, 0) as eng:
        R.ingest_all(eng, fx)
        assert np.array_equal(eng.cell_summary()["fate"], want)
        assert eng.read_fate()["assigned"] == fx["fate"]["assigned"]
    monkeypatch.setenv("XCK_CELL_SUMMARY", "0")
    with R.fixture_engine(fx, 0) as eng:
        assert eng.cell_summary() is None and eng.read_fate() is None


# ----------------------------------------------------------------------------- 9. front-ends
def _lines(path):
    with open(path) as fp:
        return fp.read().splitlines()


HEAD = "cell\treads\t" + "\t".join(U.COLS)


def _golden_matrix(kind, exp, n_cells):
    """the matrix half from the .mtx files the reference wrote"""
    if kind == "basefc":
        return np.stack(U.mtx_marginals(os.path.join(exp, "matrix.mtx"), n_cells), axis=1)
    ad, _ = U.mtx_marginals(os.path.join(exp, "xcltk.AD.mtx"), n_cells)
    dp, ndp = U.mtx_marginals(os.path.join(exp, "xcltk.DP.mtx"), n_cells)
    oth, _ = U.mtx_marginals(os.path.join(exp, "xcltk.OTH.mtx"), n_cells)
    return np.stack([ad, dp, oth, ndp], axis=1)


def _expected_file(kind, fixture, exp, names_fn):
    cx, tab = U.load_cell_fixture(fixture)
    names = [x.strip() for x in _lines(names_fn)]
    assert sorted(names) == cx["cells"]
    head = HEAD + "\t" + "\t".join(capi.CELL_MATRIX_COLS[BASEFC if kind == "basefc" else BAF])
    return [head] + U.expected_lines(cx, tab, _golden_matrix(kind, exp, len(names)), names)


@pytest.mark.parametrize("case_name,fixture", [("c1_basefc_default", "c1_basefc"), ("c1_baf_allreg", "c1_baf"),
                                               ("multibam_basefc", "multibam_basefc"), ("well_basefc", "well_basefc")])
def test_frontends_write_the_table_only_when_asked(case_name, fixture, tmp_path, monkeypatch):
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_wrapper
    assert R.load_fixture(fixture)["outside_table"] == 0
    case, ddir, odir, exp = util.load_case(case_name, tmp_path)
    run = fc_wrapper if case["kind"] == "basefc" else afc_wrapper
    pre = "" if case["kind"] == "basefc" else "xcltk."
    fn, fn_reads = os.path.join(odir, pre + "cell_summary.tsv"), os.path.join(odir, pre + "read_summary.tsv")
    monkeypatch.delenv("XCK_CELL_SUMMARY", raising=False)
    monkeypatch.delenv("XCK_READ_FATE", raising=False)
    assert run(**case["kwargs"]) == 0
    util.assert_dirs_equal(odir, exp)                         # (no such file)
    monkeypatch.setenv("XCK_READ_FATE", "1")                  # the read summary alone does not bring the table
    assert run(**case["kwargs"]) == 0
    assert os.path.exists(fn_reads) and not os.path.exists(fn)
    os.remove(fn_reads)
    monkeypatch.delenv("XCK_READ_FATE")
    monkeypatch.setenv("XCK_CELL_SUMMARY", "1")
    assert run(**case["kwargs"]) == 0
    names_fn = os.path.join(exp, "barcodes.tsv" if case["kind"] == "basefc" else "xcltk.samples.tsv")
    assert _lines(fn) == _expected_file(case["kind"], fixture, exp, names_fn)
    os.remove(fn)
    os.remove(fn_reads)                                       # (the flag implies the read summary)
    util.assert_dirs_equal(odir, exp)                         # the golden directory byte for byte, plus the two summaries


def test_fused_frontend_writes_one_table_per_pipeline(tmp_path, monkeypatch):
    from xcltk_amd.fused import fused_wrapper
    case, ddir, odir, exp_fc = util.load_case("c1_basefc_default", tmp_path)
    _, _, _, exp_baf = util.load_case("c1_baf_allreg", tmp_path)
    kw = case["kwargs"]
    off, on = str(tmp_path / "off"), str(tmp_path / "on")
    monkeypatch.delenv("XCK_CELL_SUMMARY", raising=False)
    monkeypatch.delenv("XCK_READ_FATE", raising=False)
    assert fused_wrapper(kw["sam_fn"], kw["barcode_fn"], kw["region_fn"], os.path.join(ddir, "snps.tsv"), off, ncores=2) == 0
    monkeypatch.setenv("XCK_CELL_SUMMARY", "1")
    assert fused_wrapper(kw["sam_fn"], kw["barcode_fn"], kw["region_fn"], os.path.join(ddir, "snps.tsv"), on, ncores=2) == 0
    got_fc = _lines(os.path.join(on, "basefc", "cell_summary.tsv"))
    assert got_fc == _expected_file("basefc", "c1_basefc", exp_fc, os.path.join(exp_fc, "barcodes.tsv"))
    # the pileup half: the fixture's table; its matrices (the fused front-end's own filters) from the files it wrote next to it
    got_baf = _lines(os.path.join(on, "baf", "xcltk.cell_summary.tsv"))
    assert got_baf == _expected_file("baf", "c1_baf", os.path.join(on, "baf"), os.path.join(on, "baf", "xcltk.samples.tsv"))
    for sub in ("basefc", "baf"):
        extra = sorted(set(os.listdir(os.path.join(on, sub))) - set(os.listdir(os.path.join(off, sub))))
        assert extra == sorted(p + s for p in ("" if sub == "basefc" else "xcltk.",) for s in ("cell_summary.tsv", "read_summary.tsv"))
        for f in os.listdir(os.path.join(off, sub)):
            assert open(os.path.join(on, sub, f), "rb").read() == open(os.path.join(off, sub, f), "rb").read(), f


def test_pileup_writes_the_table_only_when_asked(tmp_path, monkeypatch):
    """baf.genotype.pileup(): per-cell SNP coverage next to the pileup directory, which itself does not change"""
    from test_genotype import assert_cellsnp_dirs_equal
    from xcltk_amd.baf.genotype import pileup
    from xcltk_amd.utils import csp_io
    DS = os.path.join(util.GOLDEN, "datasets", "phasing")

    def run(out):
        return pileup(sam_fn=os.path.join(DS, "possorted.bam"), barcode_fn=os.path.join(DS, "barcodes.tsv"),
                      snp_vcf_fn=os.path.join(DS, "cellsnp", "cellSNP.base.vcf.gz"), out_dir=out, mode="droplet", ncores=2, min_count=20, min_maf=0.1)
    off, on = str(tmp_path / "off"), str(tmp_path / "on")
    monkeypatch.delenv("XCK_CELL_SUMMARY", raising=False)
    monkeypatch.delenv("XCK_READ_FATE", raising=False)
    want = run(off)[1:]
    assert not os.path.exists(os.path.join(off, "cell_summary.tsv"))
    monkeypatch.setenv("XCK_CELL_SUMMARY", "1")
    assert run(on)[1:] == want
    assert_cellsnp_dirs_equal(on, off)
    assert_cellsnp_dirs_equal(os.path.join(on, "raw"), os.path.join(off, "raw"))
    lines = _lines(os.path.join(on, "cell_summary.tsv"))
    raw = csp_io.load_data(os.path.join(on, "raw"))
    assert lines[0] == HEAD + "\tad\tdp\toth\tfeatures"
    assert [x.split("\t")[0] for x in lines[1:]] == list(raw.cells) + ["*"]
    tab = np.array([[int(v) for v in x.split("\t")[1:]] for x in lines[1:]], dtype=np.int64)
    # the matrix columns are the per-cell sums of the pileup directory: SNP coverage per cell
    for j, m in enumerate((raw.AD, raw.DP, raw.OTH)):
        assert np.array_equal(tab[:-1, 13 + j], np.asarray(m.sum(axis=1)).reshape(-1).astype(np.int64)), j
    assert np.array_equal(tab[:-1, 16], np.asarray((raw.DP != 0).sum(axis=1)).reshape(-1)) and not tab[-1, 13:].any()
    # the class columns sum to the read summary written next to it
    reads = dict(x.split("\t") for x in _lines(os.path.join(on, "read_summary.tsv")))
    assert [int(v) for v in tab[:, 1:13].sum(axis=0)] == [int(reads[k]) for k in U.COLS]
    assert np.array_equal(tab[:, 0], tab[:, 1:11].sum(axis=1)) and tab[:, 0].sum() == int(reads["n_reads"]) - int(reads["not_joined"])


# ----------------------------------------------------------------------------- 10. two ranks
@pytest.mark.parametrize("case_name", ["special_basefc", "special_baf"])
def test_two_ranks_sum_to_the_single_rank_table(case_name, tmp_path, monkeypatch):
    """two ranks over gloo on the one GPU; the dataset's contigs are not cut, so every record is decoded by exactly one rank and
    the summed table equals the single-rank one"""
    from test_gpu_multirank import _free_port
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_wrapper
    env = dict(os.environ, XCK_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", XCK_DEVICE="0", XCK_CELL_SUMMARY="1")
    two = tmp_path / "two"
    two.mkdir()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", _free_port(), os.path.join(ROOT, "tests", "cell_summary_dist_worker.py"), case_name, str(two)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert "CELL_SUMMARY_DIST_OK %s WORLD 2" % case_name in r.stdout, r.stdout[-3000:]   # (nothing more on the GPU after a failure)
    one = tmp_path / "one"
    one.mkdir()
    monkeypatch.setenv("XCK_CELL_SUMMARY", "1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    case, ddir, odir, exp = util.load_case(case_name, one)
    assert (fc_wrapper if case["kind"] == "basefc" else afc_wrapper)(**case["kwargs"]) == 0
    base = ("" if case["kind"] == "basefc" else "xcltk.") + "cell_summary.tsv"
    single = _lines(os.path.join(odir, base))
    summed = _lines(os.path.join(str(two), "out_" + case_name, base))
    assert summed[0] == "#ranks=2 cut_contigs=0"
    assert summed[1:] == single
    names_fn = os.path.join(exp, "barcodes.tsv" if case["kind"] == "basefc" else "xcltk.samples.tsv")
    assert single == _expected_file(case["kind"], case_name, exp, names_fn)
