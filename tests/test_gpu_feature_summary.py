"""Per-feature / per-SNP tables (XCK_F_FEATURE_SUMMARY / XCK_FEATURE_SUMMARY=1, xck_get_feature_summary) on the GPU, through the C-ABI and
the front-ends.

Expected values: tests/golden/feature_summary/*.json, produced by the reference's own check_read / sam_fetch / include code and
plp_snp (tools/make_feature_summary_goldens.py); for generated inputs the plain-Python restatement of tests/feature_summary_util.py;
for the matrix half numpy.bincount over the arrays Engine.finish() returns.  Every comparison is exact.
Invariants held on every input (_finish_and_check):
  (F1) the `pairs` column (BAF: `reads`) of the handle's pipelines sums to xck_stats.n_hits, and with XCK_F_READ_FATE also set it
       equals that pipeline's xck_read_fate.pairs;
  (F2) shared <= pairs per row, and shared sums to at least 2 * xck_read_fate.multi;
  (F3) has_matrix is 0 before the finish and 1 after it, and the matrix half equals the row marginals of the finished matrices
       (snps / snps_kept: the SNP -> region relation worked out in Python);
  (F4) every SNP's kept is the per-SNP filter recomputed in Python floats from its five tallies;
  (F5) a second call returns the same arrays, and xck_reset zeroes them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cell_summary_util as CU
import feature_summary_util as F
import read_fate_util as R
import util
from fuzz_cases import make_case
from xcltk_amd import capi
from xcltk_amd import fc_common as fcc
from xcltk_amd.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT, FATE, CELL, K128 = capi.XCK_F_FEATURE_SUMMARY, capi.XCK_F_READ_FATE, capi.XCK_F_CELL_SUMMARY, capi.XCK_F_FORCE_KEY128
BASEFC, BAF, BOTH = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF, capi.XCK_MODE_BOTH
FUZZ_SEEDS = list(range(1000, 1020)) + [1052, 1077, 1101, 1133]           # the seeds of tests/test_gpu_fuzz.py


def _pipelines(eng):
    return [BASEFC, BAF] if eng.mode == BOTH else [eng.mode]


def _finish_and_check(eng, regions, snps=(), min_count=1, min_maf=0, excl_pairs=None):
    """(F1) - (F5) -> {mode: (read half: `reads` [n_regions, 3] or `snp` [n_snps, 8], matrix)}; the handle is reset at the end"""
    n, snps = len(regions), list(snps)
    before = {}
    for m in _pipelines(eng):
        fs = before[m] = eng.feature_summary(m)
        assert fs["matrix"] is None and not fs["has_matrix"]
        if m == BASEFC:
            assert fs["snp"] is None and fs["reads"].shape == (n, 3) and fs["reads"].dtype == np.int64
        else:
            assert fs["reads"] is None and fs["snp"].shape == (len(snps), 8) and not fs["snp"][:, F.S_A:F.S_KEPT + 1].any()
    res = eng.finish()
    st = eng.stats()
    out, hits = {}, 0
    for m in _pipelines(eng):
        fs = eng.feature_summary(m)
        rf = eng.read_fate(m)                                            # (None on a handle without XCK_F_READ_FATE)
        assert fs["has_matrix"] and fs["matrix_cols"] == capi.FEATURE_MATRIX_COLS[m]
        if m == BASEFC:
            half = fs["reads"]
            assert np.array_equal(half, before[m]["reads"])              # the read half is complete before the finish
            pairs = int(half[:, F.PAIRS].sum())
            assert (half >= 0).all() and (half[:, F.SHARED] <= half[:, F.PAIRS]).all()
            if rf is not None:
                assert int(half[:, F.SHARED].sum()) >= 2 * rf["multi"]
            want = F.expected_matrix(True, res, regions)
        else:
            half = fs["snp"]
            assert np.array_equal(half[:, [F.S_READS, F.S_REGIONS]], before[m]["snp"][:, [F.S_READS, F.S_REGIONS]])
            pairs = int(half[:, F.S_READS].sum())
            assert (half >= 0).all() and set(half[:, F.S_KEPT].tolist()) <= {0, 1}
            for s, row in zip(snps, half.tolist()):
                if s[1] >= 1:
                    assert row[F.S_KEPT] == F.verdict(row[F.S_A:F.S_N + 1], s[2], s[3], min_count, min_maf), (s, row)
            assert np.array_equal(half[:, F.S_REGIONS], F.snp_region_counts(regions, snps, None, excl_pairs)[1])
            want = F.expected_matrix(False, res, regions, snps, half[:, F.S_KEPT], excl_pairs)
        if rf is not None:
            assert pairs == rf["pairs"], (m, pairs, rf)
        hits += pairs
        assert fs["matrix"].dtype == np.int64 and fs["matrix"].shape == want.shape
        assert np.array_equal(fs["matrix"], want), (m, np.flatnonzero((fs["matrix"] != want).any(axis=1))[:10])
        again = eng.feature_summary(m)                                   # (the cached half)
        assert np.array_equal(again["matrix"], fs["matrix"]) and np.array_equal(again["reads" if m == BASEFC else "snp"], half)
        out[m] = (half, fs["matrix"])
    assert hits == st["n_hits"], (hits, st["n_hits"])
    eng.reset()
    for m in _pipelines(eng):
        z = eng.feature_summary(m)
        assert z["matrix"] is None and not z["has_matrix"]
        assert not (z["reads"] if m == BASEFC else z["snp"][:, :F.S_REGIONS]).any()
    return out


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[m][0], b[m][0]) and np.array_equal(a[m][1], b[m][1]) for m in a)


# ----------------------------------------------------------------------------- 1. the reference's numbers
def _fixture_engine(fx, flags, mode=None):
    """R.fixture_engine with the fixture's per-SNP filters -> (engine, regions, snps)"""
    p = fx["params"]
    if mode is None:
        mode = BASEFC if fx["mode"] == "basefc" else BAF
    regions = fcc.load_region_from_txt(fx["region_fn"])
    snps = fcc.load_snp_from_tsv(os.path.join(fx["ddir"], "snps.tsv")) if mode & BAF else ()
    names = fcc.contig_table(regions, snps)
    barcodes = None
    if p["cell_tag"]:
        with open(os.path.join(fx["ddir"], fx["ds"]["barcodes"])) as fp:
            barcodes = sorted(x.strip() for x in fp)
    n_cells = len(barcodes) if barcodes is not None else len(fx["bam_fns"])
    eng = Engine(mode, names, regions, n_cells, snps=snps, barcodes=barcodes, cell_tag=p["cell_tag"], umi_tag=p["umi_tag"],
                 min_mapq=p["min_mapq"], min_len=p["min_len"], incl_flag=p["incl_flag"], excl_flag=p["excl_flag"],
                 no_orphan=p["no_orphan"], min_include=p["min_include"], min_count=p["min_count"], min_maf=p["min_maf"], flags=flags)
    return eng, regions, list(snps)


def _check_fixture(got, gx, want, what):
    if gx["mode"] == "basefc":
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (what, [(i, got[i], want[i]) for i in bad[:5]])
    else:
        g = np.concatenate([got[:, :F.S_KEPT], (got[:, F.S_KEPT] == 0)[:, None]], axis=1)
        w = np.concatenate([want[:, :6], (want[:, 6] != 0)[:, None]], axis=1)      # reads, the tallies, dropped or not
        bad = np.flatnonzero((g != w).any(axis=1))
        assert bad.size == 0, (what, [(i, got[i], want[i]) for i in bad[:5]])


@pytest.mark.parametrize("name", F.list_fixtures())
def test_fixture_tables_equal_the_reference(name, monkeypatch):
    """alone and inside a XCK_MODE_BOTH handle, 64- and 128-bit keys, with and without the read summary next to it; BAF also with the
    radix sorts and the sorted haplotype classification, each on a handle of its own (knobs are read at xck_create)"""
    fx, gx = F.load_fixture(name)
    own = BASEFC if gx["mode"] == "basefc" else BAF
    p = gx["params"]
    runs = [(mode, flags, None) for mode in (None, BOTH) for flags in (FEAT, FEAT | K128 | FATE)]
    if own == BAF:
        runs += [(None, FEAT, ("XCK_PILEUP_SORT", "radix")), (None, FEAT, ("XCK_PILEUP_HAP", "sorted"))]
    for mode, flags, knob in runs:
        for k in ("XCK_PILEUP_SORT", "XCK_PILEUP_HAP", "XCK_FEATURE_SUMMARY", "XCK_CELL_SUMMARY_SLOTS"):
            monkeypatch.delenv(k, raising=False)
        if knob:
            monkeypatch.setenv(*knob)
        eng, regions, snps = _fixture_engine(fx, flags, mode)
        with eng:
            if flags & K128:
                assert eng.stats()["key_bits"] == 128
            R.ingest_all(eng, fx)
            got = _finish_and_check(eng, regions, snps, p["min_count"], p["min_maf"])[own][0]
        _check_fixture(got, gx, F.fixture_table(gx, regions, snps), (mode, flags, knob))


def test_fixtures_are_there():
    assert len(F.list_fixtures()) >= 13 and set(R.list_fixtures()) <= set(F.list_fixtures())


# ----------------------------------------------------------------------------- 2. fuzz against the restatement
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_cases_equal_the_restatement(seed):
    """the 24 seeds of the fuzz suite: both modes and BOTH against the per-pair restatement"""
    names, regions, snps, n_cells, batches, fc, baf, _ = make_case(seed)
    dicts = [CU.batch_dict(keep, b.contig) for b, keep in batches]
    want = {BASEFC: F.restate(names, regions, (), dicts, fc, True), BAF: F.restate(names, regions, snps, dicts, baf, False)}
    for mode in (BASEFC, BAF, BOTH):
        kw = dict(fc) if mode == BASEFC else dict(baf) if mode == BAF else dict(fc, **baf)
        with Engine(mode, names, regions, n_cells, snps=snps if mode & BAF else (), flags=FEAT | FATE, **kw) as eng:
            for b, _ in batches:
                eng.push(b)
            multi = {m: eng.read_fate(m)["multi"] for m in _pipelines(eng)}
            got = _finish_and_check(eng, regions, snps if mode & BAF else (), baf.get("min_count", 1), baf.get("min_maf", 0))
        for m in got:
            assert multi[m] == want[m][1]
            g = got[m][0] if m == BASEFC else got[m][0][:, F.S_READS]
            bad = np.flatnonzero(g != want[m][0]) if m == BAF else np.flatnonzero((g != want[m][0]).any(axis=1))
            assert bad.size == 0, (mode, m, [(i, g[i], want[m][0][i]) for i in bad[:5]])


# ----------------------------------------------------------------------------- 3. the shapes at which the accumulation can go wrong
FILT = dict(min_mapq=20, min_len=30, excl_flag=772, incl_flag=0, no_orphan=True)
NIB = {"A": 1, "C": 2, "G": 4, "T": 8}


def _reads(pos, cells=None, bases="A", cigar=((0, 36),), contig=0, ordinal_base=0):
    """one batch of reads with one CIGAR, distinct UMIs, every base of read i the letter bases[i % len(bases)]"""
    n = len(pos)
    words = [(l << 4) | op for op, l in cigar]
    qlen = sum(l for op, l in cigar if op in (0, 1, 4, 7, 8))
    nb = (qlen + 1) // 2
    seq = np.concatenate([np.full(nb, NIB[bases[i % len(bases)]] * 17, dtype=np.uint8) for i in range(n)]) if n else np.zeros(0, dtype=np.uint8)
    return dict(contig=contig, ordinal_base=ordinal_base, pos=np.asarray(pos, dtype=np.int32), flag=np.zeros(n, dtype=np.uint16),
                mapq=np.full(n, 60, dtype=np.uint8), cell=np.zeros(n, dtype=np.int32) if cells is None else np.asarray(cells, dtype=np.int32),
                umi=(np.arange(n, dtype=np.uint64) + np.uint64(ordinal_base)) | np.uint64(1 << 24),
                cig_off=np.arange(n + 1, dtype=np.uint32) * len(words), cigar=np.tile(np.array(words, dtype=np.uint32), n),
                seq_off=np.arange(n + 1, dtype=np.uint32) * nb, seq=seq)


def _run_shape(mode, names, regions, snps, n_cells, ds, monkeypatch, min_include=0.9, min_count=1, min_maf=0):
    """the same batches with the LDS table at its built-in size, cut to 16 rows and to 1 row: identical tables -> the first"""
    first = None
    for slots in (None, "16", "1"):
        if slots is None:
            monkeypatch.delenv("XCK_CELL_SUMMARY_SLOTS", raising=False)
        else:
            monkeypatch.setenv("XCK_CELL_SUMMARY_SLOTS", slots)       # read by the library at xck_create
        kw = dict(FILT, min_include=min_include) if mode == BASEFC else dict(FILT, min_count=min_count, min_maf=min_maf)
        with Engine(mode, names, regions, n_cells, snps=snps, flags=FEAT | FATE, **kw) as eng:
            for d in ds:
                eng.push(util.batch_from_dict(d)[0])
            got = _finish_and_check(eng, regions, snps, min_count, min_maf)[mode]
        if first is None:
            first = got
            filt = dict(FILT, min_include=min_include)
            want = F.restate(names, regions, snps, ds, filt, mode == BASEFC)[0]
            g = got[0] if mode == BASEFC else got[0][:, F.S_READS]
            assert np.array_equal(g, want), np.flatnonzero(g != want)[:10]
        else:
            assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1]), slots
    return first


@pytest.mark.parametrize("n_cells", [1, 3])
def test_shape_one_region_two_tiles_and_one_read(n_cells, monkeypatch):
    regions = [("1", 1001, 3000, "a")]
    d = _reads(np.sort(np.random.default_rng(3).integers(1000, 2960, 2049)), cells=np.arange(2049) % n_cells)
    reads, matrix = _run_shape(BASEFC, ["1"], regions, (), n_cells, [d], monkeypatch)
    assert reads.tolist() == [[0, 2049, 0]] and matrix.tolist() == [[2049, n_cells]]


@pytest.mark.parametrize("n", [1024, 1025])
def test_shape_one_read_in_each_of_many_regions(n, monkeypatch):
    """more rows than the LDS table holds: every row must read `pairs 1`"""
    regions = [("1", 1001 + 100 * i, 1040 + 100 * i, "r%d" % i) for i in range(n)]
    d = _reads([1002 + 100 * i for i in range(n)])
    reads, matrix = _run_shape(BASEFC, ["1"], regions, (), 1, [d], monkeypatch)
    assert (reads == [0, 1, 0]).all() and (matrix == [1, 1]).all()


def test_shape_a_lane_walks_more_than_64_candidates(monkeypatch):
    regions = [("1", 2001, 2100, "dup%d" % i) for i in range(70)] + [("1", 1001, 3000, "outer")]
    d = _reads(np.sort(2000 + (np.arange(130) % 60)))
    reads, _ = _run_shape(BASEFC, ["1"], regions, (), 1, [d], monkeypatch)
    assert (reads == [0, 130, 130]).all()


@pytest.mark.parametrize("min_include", [0.9, 30])
def test_shape_include_fail_is_charged_to_the_region_that_fails(min_include, monkeypatch):
    """b inside a; the reads straddle b's start with 20 of their 36 bases inside b"""
    regions = [("1", 1001, 3000, "a"), ("1", 2001, 2500, "b")]
    d = _reads([1984] * 50)
    reads, _ = _run_shape(BASEFC, ["1"], regions, (), 1, [d], monkeypatch, min_include=min_include)
    assert reads.tolist() == [[0, 50, 0], [50, 0, 0]]


def test_shape_first_and_last_row_of_70000_regions(monkeypatch):
    regions = [(c, 1001 + 100 * i, 1040 + 100 * i, "%s_%d" % (c, i)) for c in ("1", "2") for i in range(35000)]
    ds = [_reads([1002] * 5, contig=0), _reads([1002 + 100 * 34999] * 7, contig=1, ordinal_base=100)]
    reads, matrix = _run_shape(BASEFC, ["1", "2"], regions, (), 1, ds, monkeypatch)
    assert reads[0].tolist() == [0, 5, 0] and reads[-1].tolist() == [0, 7, 0] and int(reads.sum()) == 12
    assert matrix[0].tolist() == [5, 1] and matrix[-1].tolist() == [7, 1] and int(matrix.sum()) == 14


def test_shape_nothing_to_count(monkeypatch):
    """a batch on a contig without regions, and no batch at all"""
    regions = [("1", 1001, 3000, "a")]
    for ds in ([_reads([1500] * 10, contig=1)], []):
        reads, matrix = _run_shape(BASEFC, ["1", "2"], regions, (), 1, ds, monkeypatch)
        assert not reads.any() and not matrix.any()


REG_BAF = [("1", 1, 100000, "all")]


def test_shape_one_snp_under_2049_reads(monkeypatch):
    snps = [("1", 1501, "A", "C", 0, 1)]
    d = _reads(np.sort(np.random.default_rng(4).integers(1470, 1500, 2049)), cells=np.arange(2049) % 3, bases="AAC")
    snp, matrix = _run_shape(BAF, ["1"], REG_BAF, snps, 3, [d], monkeypatch)
    assert snp.tolist() == [[2049, 1366, 683, 0, 0, 0, 1, 1]] and matrix.tolist() == [[1, 1, 683, 2049, 0, 3]]


def test_shape_1025_snps_one_read_over_each(monkeypatch):
    snps = [("1", 1011 + 40 * i, "A", "C", 0, 1) for i in range(1025)]
    d = _reads([1000 + 40 * i for i in range(1025)])
    snp, _ = _run_shape(BAF, ["1"], REG_BAF, snps, 1, [d], monkeypatch)
    assert (snp == [1, 1, 0, 0, 0, 0, 1, 1]).all()


def test_shape_100_consecutive_snps_under_130_reads(monkeypatch):
    snps = [("1", 2001 + i, "A", "C", 0, 1) for i in range(100)]
    d = _reads([1990] * 130, cigar=((0, 120),))
    snp, _ = _run_shape(BAF, ["1"], REG_BAF, snps, 1, [d], monkeypatch)
    assert (snp == [130, 130, 0, 0, 0, 0, 1, 1]).all()


def test_shape_two_list_entries_at_one_position_and_a_snp_in_a_gap(monkeypatch):
    snps = [("1", 1511, "A", "C", 0, 1), ("1", 1541, "A", "G", 0, 1), ("1", 1511, "A", "C", 0, 1)]
    d = _reads([1500] * 9, cigar=((0, 20), (3, 50), (0, 16)))            # 1541 lies in the N gap [1520, 1570)
    snp, _ = _run_shape(BAF, ["1"], REG_BAF, snps, 1, [d], monkeypatch)
    assert snp[0].tolist() == snp[2].tolist() == [9, 9, 0, 0, 0, 0, 1, 1]
    assert snp[1].tolist() == [9, 0, 0, 0, 0, 0, 0, 1]                   # in `reads`, not in the tallies (and so below min_count 1)


def test_shape_snp_on_a_contig_with_reads_and_no_region(monkeypatch):
    snps = [("1", 1511, "A", "C", 0, 1), ("2", 1511, "A", "C", 0, 1)]
    ds = [_reads([1500] * 4, contig=0), _reads([1500] * 6, contig=1, ordinal_base=100, bases="C")]
    snp, matrix = _run_shape(BAF, ["1", "2"], REG_BAF, snps, 1, ds, monkeypatch)
    assert snp.tolist() == [[4, 4, 0, 0, 0, 0, 1, 1], [6, 0, 6, 0, 0, 0, 1, 0]] and matrix.tolist() == [[1, 1, 0, 4, 0, 1]]


def test_shape_filter_thresholds(monkeypatch):
    """totals of min_count - 1 and min_count, and a minor count exactly at total * min_maf (10 molecules, 1 minor, 0.1)"""
    snps = [("1", 1511, "A", "C", 0, 1), ("1", 2511, "A", "C", 0, 1), ("1", 3511, "A", "C", 0, 1)]
    ds = [_reads([1500] * 4, bases="AAAC"), _reads([2500] * 5, bases="AAAAC", ordinal_base=100), _reads([3500] * 10, bases="AAAAAAAAAC", ordinal_base=200)]
    snp, matrix = _run_shape(BAF, ["1"], REG_BAF, snps, 1, ds, monkeypatch, min_count=5, min_maf=0.1)
    assert snp[:, F.S_A:F.S_N + 1].tolist() == [[3, 1, 0, 0, 0], [4, 1, 0, 0, 0], [9, 1, 0, 0, 0]]
    want = [F.verdict(t, "A", "C", 5, 0.1) for t in snp[:, F.S_A:F.S_N + 1].tolist()]
    assert snp[:, F.S_KEPT].tolist() == want and want[:2] == [0, 1]
    assert matrix[0, :2].tolist() == [3, sum(want)]


def test_shape_min_count_0_without_a_read(monkeypatch):
    snps = [("1", 1511, "A", "C", 0, 1), ("1", 2511, "N", "C", 0, 1)]
    snp, matrix = _run_shape(BAF, ["1"], REG_BAF, snps, 1, [], monkeypatch, min_count=0, min_maf=0.1)
    assert snp.tolist() == [[0, 0, 0, 0, 0, 0, 1, 1]] * 2 and matrix.tolist() == [[2, 2, 0, 0, 0, 0]]


# ----------------------------------------------------------------------------- 4. counted once
def test_overflow_replay_counts_once(monkeypatch):
    """XCK_HIT_CAP0 / XCK_HIT_SLACK so small that join launches overflow and are replayed: the tables must not see a batch twice"""
    from test_gpu_parity import _dense_pileup_case
    regions, snps, names, batches = _dense_pileup_case(seed=21, n_reads=40000, n_cells=50, n_umis=5000, snp_step=3, span=60000, max_batch=40000, gap_max=900)
    fx, _ = F.load_fixture("dense_basefc")

    def run_baf():
        with Engine(BAF, names, regions, 50, snps=snps, min_len=10, flags=FEAT) as eng:
            for b, _ in batches:
                eng.push(b)
            eng.flush()
            launches = eng.stats()["n_join_launches"]
            return _finish_and_check(eng, regions, snps), launches, len(batches)

    def run_fc():
        eng, fc_regions, _ = _fixture_engine(fx, FEAT)
        with eng:
            n = 0
            for d in eng.decode_bam(fx["bam_fns"][0], n_threads=2):
                eng.push(util.batch_from_dict(d)[0])
                n += 1
            eng.flush()
            launches = eng.stats()["n_join_launches"]
            return _finish_and_check(eng, fc_regions), launches, n

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


@pytest.mark.parametrize("name", ["c1_basefc", "c1_baf"])
def test_push_paths_agree(name):
    """xck_ingest_bam, xck_push_batch and xck_push_batch_device of one golden dataset"""
    import torch
    fx, gx = F.load_fixture(name)
    eng, regions, snps = _fixture_engine(fx, FEAT)
    with eng:
        R.ingest_all(eng, fx)
        want = _finish_and_check(eng, regions, snps)
        _check_fixture(want[eng.mode][0], gx, F.fixture_table(gx, regions, snps), name)
        ds = [d for fn in fx["bam_fns"] for d in eng.decode_bam(fn, n_threads=2)]
        for d in ds:
            eng.push(util.batch_from_dict(d)[0])
        assert _same(_finish_and_check(eng, regions, snps), want)
        keep = []
        for d in ds:                                             # the same arrays, resident in HBM
            b = capi.Batch()
            b.contig, b.n_reads, b.ordinal_base = d["contig"], len(d["pos"]), d["ordinal_base"]
            for k, ct in (("pos", C.c_int32), ("flag", C.c_uint16), ("mapq", C.c_uint8), ("cell", C.c_int32), ("umi", C.c_uint64),
                          ("cig_off", C.c_uint32), ("cigar", C.c_uint32), ("seq_off", C.c_uint32), ("seq", C.c_uint8)):
                if d.get(k) is None:
                    continue
                a = np.ascontiguousarray(d[k])
                t = torch.from_numpy(a.view(np.uint8) if a.size else np.zeros(8, dtype=np.uint8)).to("cuda:0")
                keep.append(t)
                setattr(b, k, C.cast(t.data_ptr(), C.POINTER(ct)))
            eng.push(b, device_resident=True)
        torch.cuda.synchronize()
        assert _same(_finish_and_check(eng, regions, snps), want)


# ----------------------------------------------------------------------------- off by default, the flag rules
def test_off_by_default_and_results_unchanged(monkeypatch):
    for k in ("XCK_FEATURE_SUMMARY", "XCK_CELL_SUMMARY", "XCK_READ_FATE"):
        monkeypatch.delenv(k, raising=False)
    fx, _ = F.load_fixture("c1_basefc")
    res = {}
    for flags in (0, FEAT, FEAT | CELL):
        for mode in (BASEFC, BAF):
            eng, regions, snps = _fixture_engine(fx, flags, mode)
            with eng:
                R.ingest_all(eng, fx)
                res[flags, mode] = eng.finish()
                fs = capi.FeatureSummary()
                fs.struct_size = C.sizeof(capi.FeatureSummary)
                if not flags:
                    assert eng.feature_summary() is None
                    assert eng.lib.xck_get_feature_summary(eng.h, mode, C.byref(fs)) == capi.XCK_E_STATE
                else:
                    assert eng.lib.xck_get_feature_summary(eng.h, mode, C.byref(fs)) == 0
                    assert (fs.mode, fs.n_regions, fs.has_matrix, fs.n_matrix_cols) == (mode, len(regions), 1, 2 if mode == BASEFC else 6)
                    assert (fs.n_read_cols, fs.n_snps, fs.n_snp_cols) == ((3, 0, 0) if mode == BASEFC else (0, len(snps), 8))
                    assert eng.lib.xck_get_feature_summary(eng.h, BASEFC + BAF - mode, C.byref(fs)) == capi.XCK_E_ARG
                    assert eng.lib.xck_get_feature_summary(eng.h, BOTH, C.byref(fs)) == capi.XCK_E_ARG
                    fs.struct_size = 8
                    assert eng.lib.xck_get_feature_summary(eng.h, mode, C.byref(fs)) == capi.XCK_E_ARG
                    # the flag does not imply the read summary; the per-cell flag still does
                    assert (eng.read_fate() is None) == (flags == FEAT)
    for mode in (BASEFC, BAF):
        for flags in (FEAT, FEAT | CELL):
            assert sorted(res[0, mode]) == sorted(res[flags, mode])
            for k in res[0, mode]:
                for a, b in zip(res[0, mode][k], res[flags, mode][k]):
                    assert np.array_equal(a, b), (mode, flags, k)


def test_environment_knob_sets_the_flag(monkeypatch):
    fx, gx = F.load_fixture("special_basefc")
    monkeypatch.setenv("XCK_FEATURE_SUMMARY", "1")
    eng, regions, snps = _fixture_engine(fx, 0)
    with eng:
        R.ingest_all(eng, fx)
        assert np.array_equal(eng.feature_summary()["reads"], F.fixture_table(gx, regions, snps)) and eng.read_fate() is None
    monkeypatch.setenv("XCK_FEATURE_SUMMARY", "0")
    eng, _, _ = _fixture_engine(fx, 0)
    with eng:
        assert eng.feature_summary() is None


# ----------------------------------------------------------------------------- 5. one-SNP regions
def _lines(path):
    with open(path) as fp:
        return fp.read().splitlines()


def _table(path, n_text):
    """(header fields, text columns, int64 table) of a summary file"""
    lines = _lines(path)
    rows = [x.split("\t") for x in lines[1:]]
    return lines[0].split("\t"), [r[:n_text] for r in rows], np.array([[int(v) for v in r[n_text:]] for r in rows], dtype=np.int64)


def test_pileup_one_snp_regions(tmp_path, monkeypatch):
    """baf.genotype.pileup(): every candidate SNP is a region of its own, so the two files describe the same molecules - for every kept
    SNP (duplicated positions apart) AD == its ALT tally, DP == REF + ALT, OTH == total - REF - ALT; the directory does not change"""
    from test_genotype import assert_cellsnp_dirs_equal
    from xcltk_amd.baf.genotype import pileup
    DS = os.path.join(util.GOLDEN, "datasets", "phasing")

    def run(out):
        return pileup(sam_fn=os.path.join(DS, "possorted.bam"), barcode_fn=os.path.join(DS, "barcodes.tsv"),
                      snp_vcf_fn=os.path.join(DS, "cellsnp", "cellSNP.base.vcf.gz"), out_dir=out, mode="droplet", ncores=2, min_count=20, min_maf=0.1)
    off, on = str(tmp_path / "off"), str(tmp_path / "on")
    monkeypatch.delenv("XCK_FEATURE_SUMMARY", raising=False)
    want = run(off)[1:]
    assert not os.path.exists(os.path.join(off, "feature_summary.tsv")) and not os.path.exists(os.path.join(off, "snp_summary.tsv"))
    monkeypatch.setenv("XCK_FEATURE_SUMMARY", "1")
    assert run(on)[1:] == want
    assert_cellsnp_dirs_equal(on, off)
    assert_cellsnp_dirs_equal(os.path.join(on, "raw"), os.path.join(off, "raw"))
    fh, ftext, ftab = _table(os.path.join(on, "feature_summary.tsv"), 4)
    sh, stext, stab = _table(os.path.join(on, "snp_summary.tsv"), 6)
    assert fh[4:] == list(F.MATRIX_COLS["baf"]) and sh[6:] == ["reads", "A", "C", "G", "T", "N", "total", "ref_umis", "alt_umis", "kept", "regions"]
    assert len(ftab) == len(stab) > 50 and [(t[0], t[1]) for t in ftext] == [(t[0], t[1]) for t in stext]
    seen = {}
    for t in stext:
        seen[t[0], t[1]] = seen.get((t[0], t[1]), 0) + 1
    n = 0
    for t, f, s in zip(stext, ftab.tolist(), stab.tolist()):
        total, ref, alt, kept = s[6], s[7], s[8], s[9]
        if seen[t[0], t[1]] > 1 or not kept:
            continue
        n += 1
        assert f[:2] == [1, 1] and f[2:5] == [alt, ref + alt, total - ref - alt], (t, f, s)
    assert n > 50


# ----------------------------------------------------------------------------- 6. front-ends
@pytest.mark.parametrize("case_name,fixture", [("c1_basefc_default", "c1_basefc"), ("c1_baf_allreg", "c1_baf"), ("multibam_basefc", "multibam_basefc")])
def test_frontends_write_the_files_only_when_asked(case_name, fixture, tmp_path, monkeypatch):
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_wrapper
    case, ddir, odir, exp = util.load_case(case_name, tmp_path)
    basefc = case["kind"] == "basefc"
    run = fc_wrapper if basefc else afc_wrapper
    pre = "" if basefc else "xcltk."
    fn, fn_snp = os.path.join(odir, pre + "feature_summary.tsv"), os.path.join(odir, pre + "snp_summary.tsv")
    for k in ("XCK_FEATURE_SUMMARY", "XCK_CELL_SUMMARY", "XCK_READ_FATE"):
        monkeypatch.delenv(k, raising=False)
    assert run(**case["kwargs"]) == 0
    util.assert_dirs_equal(odir, exp)                         # (no such files)
    monkeypatch.setenv("XCK_FEATURE_SUMMARY", "1")
    assert run(**case["kwargs"]) == 0
    fx, gx = F.load_fixture(fixture)
    regions = fcc.load_region_from_txt(fx["region_fn"])
    head, text, tab = _table(fn, 4)
    assert [tuple(t) for t in text] == [(r[0], str(r[1]), str(r[2]), r[3]) for r in regions]      # every input region, in input order
    if basefc:
        want = F.fixture_table(gx, regions)
        assert head[4:] == ["fetched"] + list(F.READ_COLS) + list(F.MATRIX_COLS["basefc"])
        assert np.array_equal(tab[:, 1:4], want) and np.array_equal(tab[:, 0], want[:, F.PAIRS] + want[:, F.INCLUDE_FAIL])
        assert not os.path.exists(fn_snp)
    else:
        snps = list(fcc.load_snp_from_tsv(os.path.join(fx["ddir"], "snps.tsv")))
        shead, stext, stab = _table(fn_snp, 6)
        assert [tuple(t[:4]) for t in stext] == [(s[0], str(s[1]), s[2], s[3]) for s in snps]
        want = F.fixture_table(gx, regions, snps)
        assert np.array_equal(stab[:, 0:6], want[:, 0:6]) and np.array_equal(stab[:, 9] == 0, want[:, 6] != 0)
        assert np.array_equal(stab[:, 6], want[:, 1:6].sum(axis=1))
        assert head[4:] == list(F.MATRIX_COLS["baf"])
        assert np.array_equal(tab[:, :2], F.snp_region_counts(regions, snps, stab[:, 9])[0])
        os.remove(fn_snp)
    # the matrix columns against the .mtx files the reference wrote: rows are numbered over the regions that have one
    mtx = os.path.join(exp, "matrix.mtx" if basefc else "xcltk.DP.mtx")
    with open(mtx) as fp:
        ent = [x.split() for x in fp if not x.startswith("%")][1:]
    with open(os.path.join(exp, "features.tsv" if basefc else "xcltk.region.tsv")) as fp:
        out_names = [x.rstrip("\n").split("\t")[3] for x in fp]
    row_of = {r[3]: i for i, r in enumerate(regions)}
    sums, cnt = np.zeros(len(regions), dtype=np.int64), np.zeros(len(regions), dtype=np.int64)
    for r, _, v in ent:
        sums[row_of[out_names[int(r) - 1]]] += int(v)
        cnt[row_of[out_names[int(r) - 1]]] += 1
    assert np.array_equal(tab[:, -2 if basefc else -3], sums) and np.array_equal(tab[:, -1], cnt)
    os.remove(fn)
    util.assert_dirs_equal(odir, exp)                         # the golden directory byte for byte, plus the summaries


def test_command_line_writes_the_file(tmp_path):
    """`python -m xcltk_amd basefc` with its own flag parsing in front of the writer, in a process of its own: the golden directory byte
    for byte plus feature_summary.tsv, whose counters equal the restatement under the flags of the command line"""
    case, ddir, odir, exp = util.load_case("dense_basefc_cli_flags", tmp_path)
    a = case["argv"]
    assert [a[a.index(k) + 1] for k in ("--exclFLAG", "--inclFLAG", "--minMAPQ", "--minINCLUDE")] == ["1024", "16", "2", "45"]
    env = dict(os.environ, XCK_FEATURE_SUMMARY="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("XCK_CELL_SUMMARY", "XCK_READ_FATE", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "xcltk_amd", "basefc"] + a, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:]
    fn = os.path.join(odir, "feature_summary.tsv")
    head, text, tab = _table(fn, 4)
    fx, _ = F.load_fixture("dense_basefc")
    regions = fcc.load_region_from_txt(fx["region_fn"])
    assert head[4:] == ["fetched"] + list(F.READ_COLS) + list(F.MATRIX_COLS["basefc"])
    assert [tuple(t) for t in text] == [(r_[0], str(r_[1]), str(r_[2]), r_[3]) for r_ in regions]
    with open(os.path.join(fx["ddir"], fx["ds"]["barcodes"])) as fp:
        barcodes = sorted(x.strip() for x in fp)
    names = fcc.contig_table(regions, ())
    filt = dict(min_mapq=2, min_len=30, excl_flag=1024, incl_flag=16, no_orphan=True, min_include=45)
    want, _ = F.restate(names, regions, (), F.bam_batches(fx, names, barcodes), filt, True)
    assert np.array_equal(tab[:, 1:4], want) and np.array_equal(tab[:, 0], want[:, F.PAIRS] + want[:, F.INCLUDE_FAIL]) and want[:, F.PAIRS].sum() > 1000
    os.remove(fn)
    util.assert_dirs_equal(odir, exp)


def test_reset_clears_the_tallies_of_the_last_finish(monkeypatch):
    """a finish with hits, xck_reset, then a finish that sees no batch: the fold returns before it clears its tallies, so the SNPs must
    read zero tallies (and the verdict of an empty SNP) because the reset cleared them"""
    monkeypatch.delenv("XCK_CELL_SUMMARY_SLOTS", raising=False)
    snps = [("1", 1511, "A", "C", 0, 1), ("1", 2511, "A", "C", 0, 1)]
    for min_count, kept in ((1, 0), (0, 1)):
        with Engine(BAF, ["1"], REG_BAF, 1, snps=snps, flags=FEAT, **dict(FILT, min_count=min_count, min_maf=0)) as eng:
            eng.push(util.batch_from_dict(_reads([1500] * 6, bases="AAC"))[0])
            first = _finish_and_check(eng, REG_BAF, snps, min_count, 0)[BAF]      # (ends with the reset)
            assert first[0].tolist() == [[6, 4, 2, 0, 0, 0, 1, 1], [0, 0, 0, 0, 0, 0, kept, 1]]
            again = _finish_and_check(eng, REG_BAF, snps, min_count, 0)[BAF]
            assert again[0].tolist() == [[0, 0, 0, 0, 0, 0, kept, 1]] * 2 and again[1].tolist() == [[2, 2 * kept, 0, 0, 0, 0]]


def test_fused_frontend_writes_the_files_per_pipeline(tmp_path, monkeypatch):
    from xcltk_amd.fused import fused_wrapper
    case, ddir, odir, exp_fc = util.load_case("c1_basefc_default", tmp_path)
    kw = case["kwargs"]
    off, on = str(tmp_path / "off"), str(tmp_path / "on")
    for k in ("XCK_FEATURE_SUMMARY", "XCK_CELL_SUMMARY", "XCK_READ_FATE"):
        monkeypatch.delenv(k, raising=False)
    assert fused_wrapper(kw["sam_fn"], kw["barcode_fn"], kw["region_fn"], os.path.join(ddir, "snps.tsv"), off, ncores=2) == 0
    monkeypatch.setenv("XCK_FEATURE_SUMMARY", "1")
    assert fused_wrapper(kw["sam_fn"], kw["barcode_fn"], kw["region_fn"], os.path.join(ddir, "snps.tsv"), on, ncores=2) == 0
    fx, gx = F.load_fixture("c1_basefc")
    regions = fcc.load_region_from_txt(fx["region_fn"])
    _, _, tab = _table(os.path.join(on, "basefc", "feature_summary.tsv"), 4)
    assert np.array_equal(tab[:, 1:4], F.fixture_table(gx, regions))
    fx, gx = F.load_fixture("c1_baf")
    snps = list(fcc.load_snp_from_tsv(os.path.join(fx["ddir"], "snps.tsv")))
    _, _, stab = _table(os.path.join(on, "baf", "xcltk.snp_summary.tsv"), 6)
    assert np.array_equal(stab[:, 0:6], F.fixture_table(gx, regions, snps)[:, 0:6])
    for sub, new in (("basefc", ["feature_summary.tsv"]), ("baf", ["xcltk.feature_summary.tsv", "xcltk.snp_summary.tsv"])):
        assert sorted(set(os.listdir(os.path.join(on, sub))) - set(os.listdir(os.path.join(off, sub)))) == new
        for f in os.listdir(os.path.join(off, sub)):
            assert open(os.path.join(on, sub, f), "rb").read() == open(os.path.join(off, sub, f), "rb").read(), f


@pytest.mark.parametrize("case_name", ["special_basefc", "special_baf"])
def test_two_ranks_sum_to_the_single_rank_files(case_name, tmp_path, monkeypatch):
    """two ranks over gloo on the one GPU (plain child processes): the files equal the one-rank files apart from the `#ranks` line"""
    from test_gpu_multirank import _free_port
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_wrapper
    env = dict(os.environ, XCK_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", XCK_DEVICE="0", XCK_FEATURE_SUMMARY="1")
    two = tmp_path / "two"
    two.mkdir()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", _free_port(), os.path.join(ROOT, "tests", "feature_summary_dist_worker.py"), case_name, str(two)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert "FEATURE_SUMMARY_DIST_OK %s WORLD 2" % case_name in r.stdout, r.stdout[-3000:]   # (nothing more on the GPU after a failure)
    one = tmp_path / "one"
    one.mkdir()
    monkeypatch.setenv("XCK_FEATURE_SUMMARY", "1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    case, ddir, odir, exp = util.load_case(case_name, one)
    basefc = case["kind"] == "basefc"
    assert (fc_wrapper if basefc else afc_wrapper)(**case["kwargs"]) == 0
    for base in ["feature_summary.tsv"] if basefc else ["xcltk.feature_summary.tsv", "xcltk.snp_summary.tsv"]:
        single = _lines(os.path.join(odir, base))
        summed = _lines(os.path.join(str(two), "out_" + case_name, base))
        assert summed[0] == "#ranks=2 cut_contigs=0" and summed[1:] == single, base
        assert len(single) > 5
