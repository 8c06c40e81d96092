"""Read assignment summary (XCK_F_READ_FATE / XCK_READ_FATE=1, xck_get_read_fate) on the GPU, through the C-ABI and the front-ends.

Expected values: tests/golden/read_fate/*.json, produced by the reference's own check_read / sam_fetch / include code
(tools/make_read_fate_goldens.py).  Two invariants hold on every input:
  (I1) the classes of a pipeline sum to n_reads = xck_stats.n_reads;
  (I2) pairs == xck_stats.n_hits, the join's own count of accepted pairs: k_read_fate states the accept rule a second time, and
       this pins the two statements to each other."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import read_fate_util as R
import util
from fuzz_cases import make_case
from xcltk_amd import capi
from xcltk_amd.engine import Engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FATE = capi.XCK_F_READ_FATE
BASEFC, BAF, BOTH = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF, capi.XCK_MODE_BOTH
FUZZ_SEEDS = list(range(1000, 1020)) + [1052, 1077, 1101, 1133]           # the seeds of tests/test_gpu_fuzz.py


def _pipelines(eng):
    return [BASEFC, BAF] if eng.mode == BOTH else [eng.mode]


def _finish_and_check(eng):
    """finish, then (I1) per pipeline and (I2) over the handle -> {mode: counters}"""
    eng.finish()
    st = eng.stats()
    out = {m: eng.read_fate(m) for m in _pipelines(eng)}
    for m, rf in out.items():
        print("mode", m, rf, "n_hits", st["n_hits"])
        R.check_invariants(rf, st["n_reads"])
    assert sum(rf["pairs"] for rf in out.values()) == st["n_hits"], (out, st["n_hits"])
    return out


# ----------------------------------------------------------------------------- 1. the reference's numbers
@pytest.mark.parametrize("name", R.list_fixtures())
def test_fixture_classes_equal_the_reference(name):
    fx = R.load_fixture(name)
    with R.fixture_engine(fx, FATE) as eng:
        records = R.ingest_all(eng, fx)
        rf = _finish_and_check(eng)[eng.mode]
    for k in R.CLASSES[1:] + ("multi", "pairs"):
        assert rf[k] == fx["fate"][k], (k, rf, fx["fate"])
    # records on references outside the contig table may be dropped by the decoder or forwarded as skipped batches
    assert rf["not_joined"] + (records - rf["n_reads"]) == fx["fate"]["not_joined"] + fx["outside_table"], (rf, records, fx)


def test_fixtures_cover_every_class():
    assert len(R.list_fixtures()) >= 11
    fxs = [R.load_fixture(n) for n in R.list_fixtures()]
    for k in R.CLASSES + ("multi", "pairs"):
        assert any(fx["fate"][k] > 0 for fx in fxs), k


# ----------------------------------------------------------------------------- 2. invariants
@pytest.mark.parametrize("key128", [False, True])
@pytest.mark.parametrize("name", R.list_fixtures())
def test_invariants_on_fixtures_both_pipelines(name, key128):
    """every fixture dataset through a XCK_MODE_BOTH handle: two pipelines with their own tables and counters.  The pipeline of the
    fixture's mode sees the regions / SNPs it sees alone, so apart from not_joined (the fused contig table is the union) it must
    still give the fixture's numbers"""
    fx = R.load_fixture(name)
    with R.fixture_engine(fx, FATE | (capi.XCK_F_FORCE_KEY128 if key128 else 0), BOTH) as eng:
        if key128:
            assert eng.stats()["key_bits"] == 128
        R.ingest_all(eng, fx)
        out = _finish_and_check(eng)
    own = out[BASEFC if fx["mode"] == "basefc" else BAF]
    for k in R.CLASSES[1:] + ("multi", "pairs"):
        assert own[k] == fx["fate"][k], (k, own, fx["fate"])


def _fuzz_engine(mode, case, flags):
    names, regions, snps, n_cells, batches, fc, baf, case_flags = case
    kw = dict(fc) if mode == BASEFC else dict(baf) if mode == BAF else dict(fc, **baf)
    return Engine(mode, names, regions, n_cells, snps=snps if mode & BAF else (), flags=flags, **kw)


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_invariants_on_fuzz_cases(seed):
    """the 24 seeds of the fuzz suite (unmapped-flagged / CIGAR-less reads, duplicate regions and SNPs, negative positions, unsorted
    region ends, every filter): both modes and BOTH, 64- and 128-bit keys"""
    case = make_case(seed)
    batches = case[4]
    n_in = sum(b.n_reads for b, _ in batches)
    for key128 in (False, True):
        flags = FATE | (capi.XCK_F_FORCE_KEY128 if key128 else 0)
        got = {}
        for mode in (BASEFC, BAF, BOTH):
            with _fuzz_engine(mode, case, flags) as eng:
                for b, _ in batches:
                    eng.push(b)
                got[mode] = _finish_and_check(eng)
                assert eng.stats()["n_reads"] == n_in
        # a pipeline counts the same alone and inside a fused handle, with either key width
        assert got[BOTH][BASEFC] == got[BASEFC][BASEFC] and got[BOTH][BAF] == got[BAF][BAF]
        if key128:
            assert got == first
        first = got


def test_overflow_replay_classifies_once(monkeypatch):
    """XCK_HIT_CAP0 / XCK_HIT_SLACK so small that join launches overflow their hit buffers (more than the first guess of 1.25 keys
    per read) and are replayed: the replay must not classify the batches a second time.  Pileup: a SNP every 3 bp; basefc: the
    `dense` dataset (2.7 accepted regions per read), pushed batch by batch so that launches can be counted."""
    from test_gpu_parity import _dense_pileup_case
    regions, snps, names, batches = _dense_pileup_case(seed=21, n_reads=40000, n_cells=50, n_umis=5000, snp_step=3, span=60000, max_batch=40000, gap_max=900)
    fx = R.load_fixture("dense_basefc")

    def run_baf():
        with Engine(BAF, names, regions, 50, snps=snps, min_len=10, flags=FATE) as eng:
            for b, _ in batches:
                eng.push(b)
            return _finish_and_check(eng)[BAF], eng.stats()["n_join_launches"], len(batches)

    def run_fc():
        with R.fixture_engine(fx, FATE) as eng:
            n = 0
            for d in eng.decode_bam(fx["bam_fns"][0], n_threads=2):
                eng.push(util.batch_from_dict(d)[0])
                n += 1
            return _finish_and_check(eng)[BASEFC], eng.stats()["n_join_launches"], n

    for run in (run_baf, run_fc):
        monkeypatch.delenv("XCK_HIT_CAP0", raising=False)
        monkeypatch.delenv("XCK_HIT_SLACK", raising=False)
        want, launches, pushes = run()
        assert launches == pushes and want["pairs"] > 0
        monkeypatch.setenv("XCK_HIT_CAP0", "64")                  # read by the library at xck_create
        monkeypatch.setenv("XCK_HIT_SLACK", "0")
        got, launches, pushes = run()
        assert launches > pushes, (launches, pushes)             # at least one launch was replayed
        assert got == want


# ----------------------------------------------------------------------------- 3. the push paths
@pytest.mark.parametrize("name", ["c1_basefc", "c1_baf", "special_baf_regions_un", "multibam_basefc"])
def test_push_paths_agree(name, monkeypatch):
    fx = R.load_fixture(name)
    with R.fixture_engine(fx, FATE) as eng:
        R.ingest_all(eng, fx)
        want = _finish_and_check(eng)[eng.mode]
        # reset() zeroes
        eng.reset()
        zero = eng.read_fate()
        assert all(v == 0 for v in zero.values()), zero
        # a sliced ingest (pause_records) equals one call
        for i, fn in enumerate(fx["bam_fns"]):
            with eng.open_stream(fn, sample=i, n_threads=2) as s:
                done, n_calls = False, 0
                while not done:
                    _, done = s.advance(1500)
                    n_calls += 1
        assert _finish_and_check(eng)[eng.mode] == want
    # host batches through xck_push_batch, packed one-copy form and direct form
    for stage in ("1", "0"):
        monkeypatch.setenv("XCK_PUSH_STAGE", stage)
        with R.fixture_engine(fx, FATE) as eng:
            for i, fn in enumerate(fx["bam_fns"]):
                for d in eng.decode_bam(fn, sample=i, n_threads=2):
                    b, keep = util.batch_from_dict(d)
                    eng.push(b)
            assert _finish_and_check(eng)[eng.mode] == want, stage


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
        with Engine(mode, names, regions, 200, snps=snps if mode & BAF else (), flags=FATE) as eng:
            for c, s, e in pieces:
                eng.push(soa_torch.device_batch(capi, arrays, c, s, e, bool(mode & BAF)), device_resident=True)
            dev = _finish_and_check(eng)
            assert eng.stats()["n_join_launches"] >= 2
            eng.reset()
            for b, _ in hb:
                eng.push(b)
            host = _finish_and_check(eng)
        assert dev == host
        assert all(rf["assigned"] > 0 for rf in dev.values())


# ----------------------------------------------------------------------------- 4. off by default
def test_off_by_default_and_results_unchanged(monkeypatch):
    monkeypatch.delenv("XCK_READ_FATE", raising=False)
    fx = R.load_fixture("c1_basefc")
    res = {}
    for flags in (0, FATE):
        for mode in (BASEFC, BAF):
            with R.fixture_engine(fx, flags, mode) as eng:
                R.ingest_all(eng, fx)
                res[flags, mode] = eng.finish()
                if not flags:
                    assert eng.read_fate() is None
                    rf = capi.ReadFate()
                    rf.struct_size = C.sizeof(capi.ReadFate)
                    assert eng.lib.xck_get_read_fate(eng.h, mode, C.byref(rf)) == capi.XCK_E_STATE
                else:
                    assert eng.read_fate()["n_reads"] == 10000
                    rf = capi.ReadFate()
                    rf.struct_size = C.sizeof(capi.ReadFate)
                    assert eng.lib.xck_get_read_fate(eng.h, BASEFC + BAF - mode, C.byref(rf)) == capi.XCK_E_ARG   # a pipeline the handle does not have
                    assert eng.lib.xck_get_read_fate(eng.h, BOTH, C.byref(rf)) == capi.XCK_E_ARG
    for mode in (BASEFC, BAF):
        assert sorted(res[0, mode]) == sorted(res[FATE, mode])
        for k in res[0, mode]:
            for a, b in zip(res[0, mode][k], res[FATE, mode][k]):
                assert np.array_equal(a, b), (mode, k)


def test_environment_knob_sets_the_flag(monkeypatch):
    fx = R.load_fixture("special_basefc")
    monkeypatch.setenv("XCK_READ_FATE", "1")
    with R.fixture_engine(fx, 0) as eng:
        R.ingest_all(eng, fx)
        assert eng.read_fate()["assigned"] == fx["fate"]["assigned"]
    monkeypatch.setenv("XCK_READ_FATE", "0")
    with R.fixture_engine(fx, 0) as eng:
        assert eng.read_fate() is None


def _summary_lines(path):
    with open(path) as fp:
        return fp.read().splitlines()


def _expected_lines(fx):
    want = dict(fx["fate"], n_reads=fx["records"] - fx["outside_table"])
    return ["%s\t%d" % (k, want[k]) for k in R.FIELDS]


@pytest.mark.parametrize("case_name,fixture", [("c1_basefc_default", "c1_basefc"), ("c1_baf_allreg", "c1_baf"),
                                               ("multibam_basefc", "multibam_basefc"), ("well_basefc", "well_basefc")])
def test_frontends_write_the_summary_only_when_asked(case_name, fixture, tmp_path, monkeypatch):
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_wrapper
    fx = R.load_fixture(fixture)
    assert fx["outside_table"] == 0
    case, ddir, odir, exp = util.load_case(case_name, tmp_path)
    run = fc_wrapper if case["kind"] == "basefc" else afc_wrapper
    fn = os.path.join(odir, ("" if case["kind"] == "basefc" else "xcltk.") + "read_summary.tsv")
    monkeypatch.delenv("XCK_READ_FATE", raising=False)
    assert run(**case["kwargs"]) == 0
    util.assert_dirs_equal(odir, exp)                         # (no such file)
    assert not os.path.exists(fn)
    monkeypatch.setenv("XCK_READ_FATE", "1")
    assert run(**case["kwargs"]) == 0
    assert _summary_lines(fn) == _expected_lines(fx)
    os.remove(fn)
    util.assert_dirs_equal(odir, exp)                         # the golden directory byte for byte, plus the summary


def test_fused_frontend_writes_one_summary_per_pipeline(tmp_path, monkeypatch):
    from xcltk_amd.fused import fused_wrapper
    monkeypatch.setenv("XCK_READ_FATE", "1")
    case, ddir, odir, exp_fc = util.load_case("c1_basefc_default", tmp_path)
    kw = case["kwargs"]
    out = str(tmp_path / "fused")
    assert fused_wrapper(kw["sam_fn"], kw["barcode_fn"], kw["region_fn"], os.path.join(ddir, "snps.tsv"), out, ncores=2) == 0
    assert _summary_lines(os.path.join(out, "basefc", "read_summary.tsv")) == _expected_lines(R.load_fixture("c1_basefc"))
    assert _summary_lines(os.path.join(out, "baf", "xcltk.read_summary.tsv")) == _expected_lines(R.load_fixture("c1_baf"))


# ----------------------------------------------------------------------------- 5. two ranks
@pytest.mark.parametrize("case_name,fixture", [("special_basefc", "special_basefc"), ("special_baf", "special_baf")])
def test_two_ranks_sum_to_the_single_rank_summary(case_name, fixture, tmp_path, monkeypatch):
    """two ranks over gloo on the one GPU; the dataset's contigs are not cut (its BAM is one BGZF block: no byte profile to cut by),
    so every record is decoded by exactly one rank and the summed counters equal the single-rank ones"""
    from test_gpu_multirank import _free_port
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.rdr.fc.main import fc_wrapper
    env = dict(os.environ, XCK_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", XCK_DEVICE="0", XCK_READ_FATE="1")
    two = tmp_path / "two"
    two.mkdir()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", _free_port(), os.path.join(ROOT, "tests", "read_fate_dist_worker.py"), case_name, str(two)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert "READ_FATE_DIST_OK %s WORLD 2" % case_name in r.stdout, r.stdout[-3000:]
    one = tmp_path / "one"
    one.mkdir()
    monkeypatch.setenv("XCK_READ_FATE", "1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    case, ddir, odir, exp = util.load_case(case_name, one)
    assert (fc_wrapper if case["kind"] == "basefc" else afc_wrapper)(**case["kwargs"]) == 0
    base = ("" if case["kind"] == "basefc" else "xcltk.") + "read_summary.tsv"
    single = _summary_lines(os.path.join(odir, base))
    summed = _summary_lines(os.path.join(str(two), "out_" + case_name, base))
    assert summed[0] == "#ranks=2 cut_contigs=0"
    assert summed[1:] == single
    fx = R.load_fixture(fixture)
    assert single == _expected_lines(fx)
