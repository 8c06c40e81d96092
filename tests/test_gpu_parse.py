"""Record walk and parse on the device for GPU-inflated chunks (csrc/parse_dev.hip, csrc/bam.cpp; XCK_GPU_PARSE): the matrices of a
run whose device chunks never visit the host equal those of XCK_GPU_PARSE=0 bit for bit - whole files, sliced ingests, index ranges
with position windows, replayed launches, device CRC checks, a second pass -, xck_decode_stats says that the device path ran, and a
chunk the device cannot finish (records that straddle blocks, UMIs to intern, a damaged stream) takes the host path, is counted, and
after four in a row the reader stops asking.  Reference boundary: pysam's record iteration and get_tag (xcltk/utils/sam.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from xcltk_amd import capi
from xcltk_amd.engine import Engine
from xcltk_amd.synth import bamwriter, soa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("XCK_GPU_INFLATE", "XCK_GPU_INFLATE_MIN_MB", "XCK_GPU_INFLATE_RING", "XCK_CHUNK_BYTES", "XCK_GPU_PARSE", "XCK_HIT_CAP0")


@pytest.fixture
def knob_env():
    saved = {k: os.environ.get(k) for k in KNOBS}
    os.environ["XCK_GPU_INFLATE"] = "100"
    os.environ["XCK_GPU_INFLATE_MIN_MB"] = "0"
    os.environ["XCK_CHUNK_BYTES"] = str(6 << 20)                  # ~90 blocks per chunk (the device takes chunks of 64 blocks and more)
    os.environ.pop("XCK_GPU_PARSE", None)
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


_TABLES = {}


def _tables(tmp):
    if not _TABLES:
        regions, snps, names = soa.make_tables(4000, 40000, soa.HG38_LENGTHS, seed=2)
        rng = np.random.default_rng(7)
        bcs = sorted({"".join("ACGT"[i] for i in rng.integers(0, 4, 16)) + "-1" for _ in range(500)})
        _TABLES.update(regions=regions, snps=snps, names=names, bcs=bcs)
    t = _TABLES
    open(os.path.join(tmp, "contigs.tsv"), "w").write("".join("chr%s\t%d\n" % (n, l) for n, l in zip(t["names"], soa.HG38_LENGTHS)))
    open(os.path.join(tmp, "regions.tsv"), "w").write("".join("chr%s\t%d\t%d\t%s\n" % r for r in t["regions"]))
    open(os.path.join(tmp, "barcodes.tsv"), "w").write("".join(b + "\n" for b in t["bcs"]))
    return t


def _synth(tmp, n_reads, level, shape=None):
    t = _tables(tmp)
    bam = os.path.join(tmp, "s%d%s.bam" % (level, shape or ""))
    env = dict(os.environ)
    if shape:
        env["XCK_SYNTH_SHAPE"] = shape
    subprocess.check_call([os.path.join(ROOT, "xcltk_amd", "csrc", "xck_synth_bam"), bam, os.path.join(tmp, "contigs.tsv"), os.path.join(tmp, "regions.tsv"),
                           os.path.join(tmp, "barcodes.tsv"), str(n_reads), "11", "8", str(level)], stderr=subprocess.DEVNULL, env=env)
    return bam, t


def _engine(t, flags=0, bcs=None):
    bcs = bcs or t["bcs"]
    return Engine(capi.XCK_MODE_BOTH, t["names"], t["regions"], len(bcs), snps=t["snps"], barcodes=bcs, cell_tag="CB", umi_tag="UB", min_include=0.9,
                  min_count=1, min_maf=0, no_dup_hap=True, min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True, n_threads=8, flags=flags)


def _run(t, bam, flags=0, passes=1, bcs=None, ingest=None):
    """-> (records, matrices, decode stats) of the last pass; every pass must give the same matrices"""
    eng = _engine(t, flags, bcs)
    try:
        out = None
        for _ in range(passes):
            eng.reset()
            n = ingest(eng) if ingest else eng.ingest_bam(bam)
            got = {k: tuple(np.array(a) for a in v) for k, v in eng.finish().items()}
            ds = eng.decode_stats()
            assert out is None or all(np.array_equal(a, b) for k in got for a, b in zip(got[k], out[k]))
            out = got
        return n, out, ds
    finally:
        eng.close()


def _same(x, y):
    assert x.keys() == y.keys()
    for k in x:
        for a, b in zip(x[k], y[k]):
            assert np.array_equal(a, b), k


def _both(env, t, bam, **kw):
    """knob off, then the default: identical records and matrices; -> (matrices, stats off, stats on)"""
    env["XCK_GPU_PARSE"] = "0"
    n0, off, ds0 = _run(t, bam, **kw)
    env.pop("XCK_GPU_PARSE")
    n1, on, ds1 = _run(t, bam, **kw)
    assert n0 == n1
    _same(off, on)
    assert ds0["gpu_parse_chunks"] == 0 and ds0["gpu_parse_fallbacks"] == 0 and ds0["gpu_inflate_chunks"] > 0
    return on, ds0, ds1


@pytest.mark.parametrize("level,shape", [(0, None), (6, None), (6, "cellranger")])
def test_device_parse_changes_nothing(level, shape, knob_env, tmp_path):
    bam, t = _synth(str(tmp_path), 600000, level, shape)
    on, ds0, ds1 = _both(knob_env, t, bam)
    assert len(on["count"][0]) > 5000 and len(on["dp"][0]) > 50
    assert ds1["gpu_parse_chunks"] > 0 and ds1["gpu_parse_fallbacks"] == 0 and ds1["gpu_parse_chunks"] <= ds1["gpu_inflate_chunks"]


@pytest.fixture(scope="module")
def bam600(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("parse600"))
    return _synth(tmp, 600000, 6)


def test_sliced_ingest(bam600, knob_env):
    bam, t = bam600

    def sliced(eng):
        st = eng.open_stream(bam)
        n = 0
        while not st.done:
            n, _ = st.advance(70000)
        st.close()
        return n
    whole, _, _ = _both(knob_env, t, bam)
    n, got, ds = _run(t, bam, ingest=sliced)
    _same(whole, got)
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0


def test_contig_mask_index_and_windows(bam600, knob_env):
    bam, t = bam600
    mask = np.zeros(len(t["names"]), dtype=bool)
    mask[[0, 2, 5]] = True
    windows = {0: (20000000, 120000000), 2: (0, 90000000), 5: (50000000, 0)}
    _, _, ds = _both(knob_env, t, bam, ingest=lambda eng: eng.ingest_bam(bam, contig_mask=mask, use_index=True, windows=windows))
    print("index ranges + windows:", ds)
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0


def test_replayed_launches_read_the_parsed_slot(bam600, knob_env):
    bam, t = bam600
    whole, _, _ = _both(knob_env, t, bam)
    knob_env["XCK_HIT_CAP0"] = "64"                                 # every launch overflows its first guess and is replayed
    _, got, ds = _run(t, bam)
    _same(whole, got)
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0


def test_device_crc_and_two_passes(bam600, knob_env):
    bam, t = bam600
    _, _, ds = _both(knob_env, t, bam, flags=capi.XCK_F_DEVICE_CRC, passes=2)
    assert ds["gpu_parse_chunks"] > 0 and ds["gpu_parse_fallbacks"] == 0 and ds["crc_blocks_device"] > 0 and ds["crc_mismatch_device"] == 0


# ---- fallbacks: small files from the Python writer, small BGZF blocks so that a chunk still holds >= 64 of them ----
def _write(tmp, name, t, n=24000, align=True, umi=lambda i, rng: "".join("ACGT"[k] for k in rng.integers(0, 4, 10)), umi_type="Z", bcs=None):
    rng = np.random.default_rng(3)
    bcs = bcs or t["bcs"]
    refs = [("chr%s" % nm, l) for nm, l in zip(t["names"], soa.HG38_LENGTHS)]
    path = os.path.join(tmp, name)
    w = bamwriter.BamWriter(path, refs, align_records=align, block_payload=3000)
    per = n // 3
    for tid in range(3):
        pos = np.sort(rng.integers(1000, soa.HG38_LENGTHS[tid] - 1000, per))
        for i in range(per):
            seq = "".join("ACGT"[k] for k in rng.integers(0, 4, 60))
            u = umi(i, rng)
            tags = [("CB", bcs[int(rng.integers(0, len(bcs)))])] + ([("UB", u, umi_type)] if umi_type != "Z" else [("UB", u)])
            w.write(tid, int(pos[i]), "r%07d" % (tid * per + i), 0, 60, "60M", seq, tags)
    w.close()
    return path


@pytest.fixture
def small_chunks(knob_env):
    knob_env["XCK_CHUNK_BYTES"] = "200000"                          # ~70 blocks of 3000 bytes: ~18 chunks per file
    knob_env["XCK_GPU_INFLATE_RING"] = "6"                          # (few chunks in flight: those scheduled before the reader gives up fall back too)
    return knob_env


def test_packed_blocks_fall_back_and_the_reader_gives_up(small_chunks, tmp_path):
    t = _tables(str(tmp_path))
    bam = _write(str(tmp_path), "packed.bam", t, align=False)
    _, _, ds = _both(small_chunks, t, bam)
    assert ds["gpu_parse_chunks"] == 0 and 4 <= ds["gpu_parse_fallbacks"] <= 12 and ds["gpu_parse_fallbacks"] < ds["gpu_inflate_chunks"]


def test_umis_with_n_fall_back_and_the_reader_gives_up(small_chunks, tmp_path):
    t = _tables(str(tmp_path))
    bam = _write(str(tmp_path), "n.bam", t, umi=lambda i, rng: "ACGTNACGTA" if i % 50 == 0 else "".join("ACGT"[k] for k in rng.integers(0, 4, 10)))
    _, _, ds = _both(small_chunks, t, bam)
    assert ds["gpu_parse_chunks"] == 0 and 4 <= ds["gpu_parse_fallbacks"] <= 12 and ds["gpu_parse_fallbacks"] < ds["gpu_inflate_chunks"]


def test_numeric_umi_falls_back(small_chunks, tmp_path):
    t = _tables(str(tmp_path))
    bam = _write(str(tmp_path), "num.bam", t, umi=lambda i, rng: int(rng.integers(1, 1000)), umi_type="i")
    _, _, ds = _both(small_chunks, t, bam)
    assert ds["gpu_parse_chunks"] == 0 and 4 <= ds["gpu_parse_fallbacks"] <= 12 and ds["gpu_parse_fallbacks"] < ds["gpu_inflate_chunks"]


def test_long_barcodes_keep_the_host_path(small_chunks, tmp_path):
    t = _tables(str(tmp_path))
    bcs = [b[:16] + "ACGT"[i % 4] * 2 + "-1" for i, b in enumerate(t["bcs"])]       # 20 bytes: the table's slots hold 18
    bam = _write(str(tmp_path), "bc20.bam", t, bcs=bcs)
    _, _, ds = _both(small_chunks, t, bam, bcs=bcs)
    assert ds["gpu_parse_chunks"] == 0 and ds["gpu_parse_fallbacks"] == 0 and ds["gpu_inflate_chunks"] > 8


def _error_of(t, bam):
    eng = _engine(t)
    try:
        with pytest.raises(Exception) as ei:
            eng.ingest_bam(bam)
        return getattr(ei.value, "code", None), str(ei.value), eng.decode_stats()
    finally:
        eng.close()


def _rewrite_blocks(src, dst, edit):
    """copy a BAM block by block; edit(k, payload) -> new payload of block k"""
    import zlib
    raw = open(src, "rb").read()
    out, at, k = [], 0, 0
    while at < len(raw):
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        payload = zlib.decompress(raw[at + 18:at + bsize - 8], -15)
        out.append(bamwriter.bgzf_block(edit(k, payload)))
        at += bsize; k += 1
    open(dst, "wb").write(b"".join(out))
    return k


def test_short_block_size_in_mid_file_is_reported_as_on_the_host(small_chunks, tmp_path):
    t = _tables(str(tmp_path))
    good = _write(str(tmp_path), "good.bam", t)
    bad = os.path.join(str(tmp_path), "short.bam")

    def edit(k, payload):
        return struct.pack("<i", 20) + payload[4:] if k == 300 else payload    # the first record of block 300 claims 20 bytes
    assert _rewrite_blocks(good, bad, edit) > 400
    small_chunks["XCK_GPU_PARSE"] = "0"
    code0, text0, _ = _error_of(t, bad)
    small_chunks.pop("XCK_GPU_PARSE")
    code1, text1, ds = _error_of(t, bad)
    assert code0 is not None and (code0, text0) == (code1, text1)
    assert ds["gpu_parse_fallbacks"] >= 1


def test_damaged_stream_is_reported_as_on_the_host(knob_env, bam600, tmp_path):
    bam, t = bam600
    raw = bytearray(open(bam, "rb").read())
    at = len(raw) * 2 // 3
    raw[at:at + 64] = bytes(64)
    bad = os.path.join(str(tmp_path), "damaged.bam")
    open(bad, "wb").write(raw)
    knob_env["XCK_GPU_PARSE"] = "0"
    code0, text0, _ = _error_of(t, bad)
    knob_env.pop("XCK_GPU_PARSE")
    code1, text1, ds = _error_of(t, bad)
    assert code0 is not None and (code0, text0) == (code1, text1)
    assert ds["gpu_parse_fallbacks"] >= 1 and ds["gpu_parse_chunks"] > 0
