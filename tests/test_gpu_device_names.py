"""Read names interned on the device (csrc/intern_dev.hip, XCK_GPU_NAMES=1): a UMI-less handle keys every read by its name, and with the
knob the names get their ids from one table in HBM per handle - fed by k_intern_recs behind the device's parse and by the names the
host-parsed chunks send along - so the GPU-inflated chunks of such a handle are walked and parsed on the device.  The same name must
get the same key whichever side parsed its chunk: the files put the two records of a pair many chunks apart, or a few records apart
across chunk boundaries (tests/device_names_cases.py; tests/test_device_names_cases_host.py checks the files on the CPU).
Expected matrices: oracle/pybam.py's records through the oracle, and the host path with the knob unset.  Reference boundary: pysam's
record iteration and query_name as restated by oracle/pybam.py, with the counting of oracle/xck_oracle.c."""
import os
import subprocess
import sys

import numpy as np
import pytest

import device_names_cases as N
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("XCK_GPU_NAMES", "XCK_GPU_NAMES_SLOTS0", "XCK_GPU_NAMES_ARENA0", "XCK_TEST_NAMES_HASH_BITS", "XCK_GPU_INFLATE", "XCK_GPU_INFLATE_MIN_MB",
         "XCK_GPU_INFLATE_RING", "XCK_CHUNK_BYTES", "XCK_GPU_PARSE", "XCK_HIT_CAP0", "XCK_READ_FATE", "XCK_CELL_SUMMARY")


@pytest.fixture
def env():
    saved = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(XCK_GPU_INFLATE="100", XCK_GPU_INFLATE_MIN_MB="0", XCK_CHUNK_BYTES=str(N.CHUNK_BYTES), XCK_GPU_INFLATE_RING="6")
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("names"))
    out = dict(shared=os.path.join(tmp, "shared.bam"), packed=os.path.join(tmp, "packed.bam"), mates=os.path.join(tmp, "mates.bam"), shapes=os.path.join(tmp, "shapes.bam"))
    out["shared_recs"] = N.write_shared(out["shared"])
    N.write_shared(out["packed"], align=False)
    N.write_mates(out["mates"])
    N.write_shapes(out["shapes"])
    return out


def _engine(mode=capi.XCK_MODE_BASEFC, barcodes=True, n_cells=None, flags=0):
    regions, snps = (N.REGIONS, ()) if mode == capi.XCK_MODE_BASEFC else (N.BAF_REGIONS, N.BAF_SNPS)
    if barcodes:
        return Engine(mode, N.NAMES, regions, len(N.BARCODES), snps=snps, barcodes=N.BARCODES, cell_tag="CB", umi_tag=None, n_threads=8, flags=flags)
    return Engine(mode, N.NAMES, regions, n_cells, snps=snps, n_threads=8, flags=flags)


def _run(bam, mode=capi.XCK_MODE_BASEFC, fate=False):
    """-> (records, matrices, decode stats, umi_bits[, read fate]) of one pass"""
    eng = _engine(mode)
    try:
        n = eng.ingest_bam(bam)
        got = {k: tuple(np.array(a) for a in v) for k, v in eng.finish().items()}
        out = (n, got, eng.decode_stats(), eng.umi_bits)
        return out + (eng.read_fate(),) if fate else out
    finally:
        eng.close()


def _mats(mode):
    return ("count",) if mode == capi.XCK_MODE_BASEFC else ("ad", "dp", "oth")


def _off_on(env, bam, mode=capi.XCK_MODE_BASEFC, **on_env):
    """the knob unset, then set: the same records and matrices; -> (matrices, stats with the knob, umi_bits)"""
    env.pop("XCK_GPU_NAMES", None)
    n0, off, ds0, ub = _run(bam, mode)
    assert ds0["gpu_parse_chunks"] == 0 and ds0["gpu_names_interned"] == 0 and ds0["gpu_inflate_chunks"] > 0
    env["XCK_GPU_NAMES"] = "1"
    env.update(on_env)
    n1, on, ds1, _ = _run(bam, mode)
    print("device names:", os.path.basename(bam), on_env, ds1)
    assert n0 == n1
    util.assert_coo_equal(on, off, _mats(mode))
    return on, ds1, ub


_EXPECTED = {}


def _expected(bam, mode, ub):
    """pybam's records through the oracle: computed once per file and mode, shared and left unchanged"""
    key = (bam, mode, ub)
    if key not in _EXPECTED:
        regions, snps = (N.REGIONS, []) if mode == capi.XCK_MODE_BASEFC else (N.BAF_REGIONS, N.BAF_SNPS)
        _EXPECTED[key] = N.expected(bam, mode, regions, snps, ub)
    return _EXPECTED[key]


# 1 ------------------------------------------------------------------------------------------------------------------------------------
def test_names_shared_across_the_two_parsers(env, files, oracle_lib):
    bam = files["shared"]
    on, ds, ub = _off_on(env, bam)
    util.assert_coo_equal(on, _expected(bam, capi.XCK_MODE_BASEFC, ub), ("count",))
    # the whole-contig row of a cell counts its distinct names: half its records
    per_cell = np.bincount([c for _, c in files["shared_recs"]], minlength=len(N.BARCODES))
    row, col, val = on["count"]
    whole = {int(c): int(v) for r, c, v in zip(row, col, val) if r == 0}
    assert whole == {c: int(per_cell[c]) // 2 for c in range(len(N.BARCODES))}
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0 and ds["gpu_names_host_chunks"] >= 1
    assert ds["gpu_names_distinct"] == N.HALF and ds["gpu_names_interned"] == N.N


def test_names_shared_with_a_pool_share(env, files, oracle_lib):
    """a fixed share of the chunks stays with the pool: host-parsed chunks in mid-file feed the table too"""
    bam = files["shared"]
    on, ds, ub = _off_on(env, bam, XCK_GPU_INFLATE="60")
    util.assert_coo_equal(on, _expected(bam, capi.XCK_MODE_BASEFC, ub), ("count",))
    assert ds["gpu_parse_chunks"] > 1 and ds["gpu_names_host_chunks"] > 1 and ds["gpu_parse_fallbacks"] == 0
    assert ds["gpu_names_distinct"] == N.HALF


def test_mates_across_chunk_boundaries_baf(env, files, oracle_lib):
    bam = files["mates"]
    on, ds, ub = _off_on(env, bam, capi.XCK_MODE_BAF)
    util.assert_coo_equal(on, _expected(bam, capi.XCK_MODE_BAF, ub), ("ad", "dp", "oth"))
    assert len(on["dp"][0]) > 0 and int(on["dp"][2].sum()) > 1000
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0 and ds["gpu_names_host_chunks"] >= 1 and ds["gpu_names_distinct"] == N.HALF


# 2 ------------------------------------------------------------------------------------------------------------------------------------
def test_host_parsed_chunks_only(env, files, oracle_lib):
    """packed blocks: every device chunk falls back and the reader gives up - all names reach the table from the host's parse"""
    bam = files["packed"]
    on, ds, ub = _off_on(env, bam)
    util.assert_coo_equal(on, _expected(files["shared"], capi.XCK_MODE_BASEFC, ub), ("count",))     # (the same records)
    assert ds["gpu_parse_chunks"] == 0 and 4 <= ds["gpu_parse_fallbacks"] <= 12 and ds["gpu_names_host_chunks"] > 0
    assert ds["gpu_names_distinct"] == N.HALF


# 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hash_bits", [None, "4"])
def test_growth_and_collisions(hash_bits, env, files, oracle_lib):
    bam = files["shared"]
    extra = dict(XCK_GPU_NAMES_SLOTS0="64", XCK_GPU_NAMES_ARENA0="4096")
    if hash_bits:
        extra["XCK_TEST_NAMES_HASH_BITS"] = hash_bits
    on, ds, ub = _off_on(env, bam, **extra)
    util.assert_coo_equal(on, _expected(bam, capi.XCK_MODE_BASEFC, ub), ("count",))
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0 and ds["gpu_names_distinct"] == N.HALF


# 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_name_shapes(env, files, oracle_lib):
    bam = files["shapes"]
    on, ds, ub = _off_on(env, bam)
    exp = _expected(bam, capi.XCK_MODE_BASEFC, ub)
    util.assert_coo_equal(on, exp, ("count",))
    # the oracle's own answer for the two cells of the shaped records: one molecule per non-empty shape
    row, col, val = exp["count"]
    whole = {int(c): int(v) for r, c, v in zip(row, col, val) if r == 0}
    assert whole[0] == whole[1] == len([s for s in N.SHAPES if s])
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0 and ds["gpu_names_host_chunks"] >= 1
    n_direct = len([s for s in N.SHAPES if s and set(s) <= set("ACGT")])
    assert ds["gpu_names_distinct"] == N.N_SHAPES_FILE - 3 * len(N.SHAPES) - 1 + len([s for s in N.SHAPES if s]) - n_direct


# 5 ------------------------------------------------------------------------------------------------------------------------------------
def _well(bam, passes=1):
    eng = _engine(barcodes=False, n_cells=3)
    try:
        out = None
        for _ in range(passes):
            eng.reset()
            n = eng.ingest_bams([bam, bam, bam])
            got = {k: tuple(np.array(a) for a in v) for k, v in eng.finish().items()}
            ds = eng.decode_stats()
            assert out is None or all(np.array_equal(a, b) for a, b in zip(got["count"], out["count"]))
            out = got
        return n, out, ds
    finally:
        eng.close()


def test_well_mode_three_samples_and_two_passes(env, files):
    bam = files["shared"]
    n0, off, ds0 = _well(bam)
    assert ds0["gpu_parse_chunks"] == 0 and ds0["gpu_names_interned"] == 0
    env["XCK_GPU_NAMES"] = "1"
    n1, on, ds1 = _well(bam)
    assert n0 == n1 == 3 * N.N
    util.assert_coo_equal(on, off, ("count",))
    row, col, val = on["count"]
    cols = [sorted(zip(row[col == c].tolist(), val[col == c].tolist())) for c in range(3)]
    assert cols[0] == cols[1] == cols[2] and len(cols[0]) == len(N.REGIONS)
    assert ds1["gpu_parse_chunks"] > 0 and ds1["gpu_parse_fallbacks"] == 0 and ds1["gpu_names_host_chunks"] >= 3
    assert ds1["gpu_names_distinct"] == 3 * N.HALF                         # (the table is cleared per BAM: ids are summed over the clears)
    _, twice, ds2 = _well(bam, passes=2)
    util.assert_coo_equal(twice, off, ("count",))
    assert ds2["gpu_names_distinct"] == 3 * N.HALF and ds2["gpu_parse_chunks"] == ds1["gpu_parse_chunks"]      # (xck_reset starts the counters over)


# 6 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["well_baf", "c1_basefc_noumi"])
def test_capacity_is_retried_with_128bit_keys(name, tmp_path):
    """XCK_TEST_INTERN_LIMIT=40 (read once per process: a child): the device table's id space overflows, the ingest fails with
    XCK_E_CAPACITY and the front-end counts again with 128-bit keys and writes the reference's bytes."""
    env = dict(os.environ, XCK_TEST_INTERN_LIMIT="40", XCK_GPU_NAMES="1", XCK_DEBUG_TIMING="1", XCK_DEVICE="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "XCK_DIST_FORCE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dist_worker.py"), name, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    assert "MULTIRANK_OK " + name in r.stdout, r.stdout[-3000:]
    assert "counting again with 128-bit keys" in r.stdout, r.stdout[-3000:]
    assert "read names on the device" in r.stdout, r.stdout[-3000:]       # (the ids came from the device table)


# 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_replayed_launches_read_the_final_umi_column(env, files):
    bam = files["shared"]
    whole, _, _ = _off_on(env, bam)
    env["XCK_HIT_CAP0"] = "64"                                       # every launch overflows its first guess and is replayed
    _, got, ds, _ = _run(bam)
    util.assert_coo_equal(got, whole, ("count",))
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0


def test_summary_passes_read_the_final_umi_column(env, files):
    bam = files["shapes"]                                            # (holds reads without a key: the empty names)
    env.update(XCK_READ_FATE="1", XCK_CELL_SUMMARY="1")
    _, off, _, _, fate0 = _run(bam, fate=True)
    env["XCK_GPU_NAMES"] = "1"
    _, on, ds, _, fate1 = _run(bam, fate=True)
    util.assert_coo_equal(on, off, ("count",))
    assert fate0["no_umi"] == fate1["no_umi"] == 3 and fate0["assigned"] == fate1["assigned"] > 0
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0


# 8 ------------------------------------------------------------------------------------------------------------------------------------
def test_the_two_kinds_of_decode_call_do_not_mix(env, files):
    bam = files["shapes"]
    for knob in (None, "1"):
        if knob:
            env["XCK_GPU_NAMES"] = knob
        eng = _engine()
        try:
            assert eng.ingest_bam(bam) == N.N_SHAPES_FILE
            if knob:
                with pytest.raises(XckError) as ei:
                    next(iter(eng.decode_bam(bam)))
                assert ei.value.code == capi.XCK_E_STATE and "XCK_GPU_NAMES" in str(ei.value)
                eng.reset()                                          # a clear of the table: either kind may start over
            assert sum(b["n_reads"] for b in eng.decode_bam(bam)) == N.N_SHAPES_FILE
        finally:
            eng.close()


# 9 ------------------------------------------------------------------------------------------------------------------------------------
def test_knob_unset_changes_nothing(env, files):
    _, _, ds, _ = _run(files["shared"])
    assert ds["gpu_inflate_chunks"] > 0 and ds["gpu_parse_chunks"] == 0 and ds["gpu_parse_fallbacks"] == 0
    assert ds["gpu_names_interned"] == 0 and ds["gpu_names_distinct"] == 0 and ds["gpu_names_host_chunks"] == 0
