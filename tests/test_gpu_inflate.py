"""The GPU share of the BGZF inflate (csrc/inflate_dev.hip, csrc/bam.cpp; XCK_GPU_INFLATE): the matrices of a run whose chunks are
partly inflated on the device equal those of the host-only run bit for bit - for blocks written by zlib and by this repo's fast
compressor -, the statistics say that the device took part, parked slots serve the next reader, and asking for CRC checks keeps the
inflate on the host.  Reference boundary: the inflate inside pysam / htslib's fetch (xcltk/rdr/fc/core.py:73-76)."""
import os
import subprocess

import numpy as np
import pytest

import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine
from xcltk_amd.synth import soa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("XCK_GPU_INFLATE", "XCK_GPU_INFLATE_DEPTH", "XCK_GPU_INFLATE_MIN_MB", "XCK_CHUNK_BYTES")


@pytest.fixture
def knob_env():
    saved = {k: os.environ.get(k) for k in KNOBS}
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _make_bam(tmp, n_reads, level):
    regions, snps, names = soa.make_tables(4000, 40000, soa.HG38_LENGTHS, seed=2)
    rng = np.random.default_rng(7)
    bcs = sorted({"".join("ACGT"[i] for i in rng.integers(0, 4, 16)) + "-1" for _ in range(500)})
    open(os.path.join(tmp, "contigs.tsv"), "w").write("".join("chr%s\t%d\n" % (n, l) for n, l in zip(names, soa.HG38_LENGTHS)))
    open(os.path.join(tmp, "regions.tsv"), "w").write("".join("chr%s\t%d\t%d\t%s\n" % r for r in regions))
    open(os.path.join(tmp, "barcodes.tsv"), "w").write("".join(b + "\n" for b in bcs))
    bam = os.path.join(tmp, "l%d.bam" % level)
    subprocess.check_call([os.path.join(ROOT, "xcltk_amd", "csrc", "xck_synth_bam"), bam, os.path.join(tmp, "contigs.tsv"), os.path.join(tmp, "regions.tsv"),
                           os.path.join(tmp, "barcodes.tsv"), str(n_reads), "11", "8", str(level)], stderr=subprocess.DEVNULL)
    return bam, regions, snps, names, bcs


def _count(bam, regions, snps, names, bcs, flags=0, passes=1):
    eng = Engine(capi.XCK_MODE_BOTH, names, regions, len(bcs), snps=snps, barcodes=bcs, cell_tag="CB", umi_tag="UB", min_include=0.9,
                 min_count=1, min_maf=0, no_dup_hap=True, min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True, n_threads=8, flags=flags)
    try:
        out = None
        for _ in range(passes):                                   # (a second pass opens a second reader: parked slots)
            eng.reset()
            n = eng.ingest_bam(bam)
            got = eng.finish()
            got = {k: tuple(np.array(a) for a in v) for k, v in got.items()}
            st = eng.stats()
            assert out is None or all(np.array_equal(a, b) for k in got for a, b in zip(got[k], out[k]))
            out = got
    finally:
        eng.close()
    return n, out, st


@pytest.mark.parametrize("level", [6, 0])
def test_device_share_of_the_inflate_changes_nothing(level, knob_env, tmp_path):
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 1500000, level)
    knob_env["XCK_CHUNK_BYTES"] = str(6 << 20)                    # ~90 blocks per chunk: dozens of chunks, each large enough for the device
    knob_env["XCK_GPU_INFLATE_MIN_MB"] = "0"                      # (auto mode leaves files below 96 MB to the host)
    knob_env["XCK_GPU_INFLATE"] = "0"
    n0, host, st0 = _count(bam, regions, snps, names, bcs)
    assert n0 == 1500000 and st0["gpu_inflate_chunks"] == 0 and len(host["count"][0]) > 10000 and len(host["dp"][0]) > 100
    for share, depth in (("50", "4"), ("auto", "3"), ("100", "4")):
        knob_env["XCK_GPU_INFLATE"], knob_env["XCK_GPU_INFLATE_DEPTH"] = share, depth
        n1, dev, st1 = _count(bam, regions, snps, names, bcs, passes=2)
        assert n1 == n0 and st1["gpu_inflate_chunks"] >= 5, (share, st1["gpu_inflate_chunks"])
        for k in host:
            for a, b in zip(host[k], dev[k]):
                assert np.array_equal(a, b), (share, k)
    # CRC verification wanted: the inflate stays on the host (the device does not compute the checksum)
    knob_env["XCK_GPU_INFLATE"] = "50"
    n2, crc, st2 = _count(bam, regions, snps, names, bcs, flags=capi.XCK_F_VERIFY_CRC)
    assert n2 == n0 and st2["gpu_inflate_chunks"] == 0
    for k in host:
        for a, b in zip(host[k], crc[k]):
            assert np.array_equal(a, b)


def _engine(regions, snps, names, bcs):
    return Engine(capi.XCK_MODE_BOTH, names, regions, len(bcs), snps=snps, barcodes=bcs, cell_tag="CB", umi_tag="UB", min_include=0.9,
                  min_count=1, min_maf=0, no_dup_hap=True, min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True, n_threads=8)


@pytest.mark.parametrize("share", ["0", "100"])
def test_sliced_ingest_equals_one_call(share, knob_env, tmp_path):
    """xck_ingest_opts.pause_records: the parse and the push of a chunk run behind the decoder's coordinator (csrc/bam.cpp: ChunkJob,
    Pusher); a call that returns at a chunk boundary has drained them, so slices of any size give the matrices of one call."""
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 600000, 6)
    knob_env["XCK_CHUNK_BYTES"] = str(3 << 20)
    knob_env["XCK_GPU_INFLATE_MIN_MB"] = "0"
    knob_env["XCK_GPU_INFLATE"] = share
    n0, whole, _ = _count(bam, regions, snps, names, bcs)
    eng = _engine(regions, snps, names, bcs)
    try:
        st = eng.open_stream(bam)
        seen = []
        while not st.done:
            n, done = st.advance(70000)
            assert n > (seen[-1] if seen else 0) or done
            seen.append(n)
        st.close()
        assert seen[-1] == n0 and len(seen) >= 5
        got = eng.finish()
        for k in whole:
            for a, b in zip(whole[k], got[k]):
                assert np.array_equal(np.array(b), a), k
    finally:
        eng.close()


def test_damaged_file_ends_the_ingest_with_an_error_and_the_handle_lives_on(knob_env, tmp_path):
    """A BGZF block whose DEFLATE stream is damaged in the middle of the file: the device leaves it to the host (non-zero status), the
    host decoder reports it, xck_ingest_bam returns XCK_E_IO after draining what was in flight - and after xck_reset the same handle
    counts the intact file correctly."""
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 600000, 6)
    knob_env["XCK_CHUNK_BYTES"] = str(3 << 20)
    knob_env["XCK_GPU_INFLATE_MIN_MB"] = "0"
    knob_env["XCK_GPU_INFLATE"] = "100"
    n0, whole, _ = _count(bam, regions, snps, names, bcs)
    raw = bytearray(open(bam, "rb").read())
    at = len(raw) * 2 // 3
    raw[at:at + 64] = bytes(64)                                   # zeros in the middle of some block's compressed stream
    bad = os.path.join(str(tmp_path), "damaged.bam")
    open(bad, "wb").write(raw)
    eng = _engine(regions, snps, names, bcs)
    try:
        with pytest.raises(Exception) as ei:
            eng.ingest_bam(bad)
        assert getattr(ei.value, "code", capi.XCK_E_IO) in (capi.XCK_E_IO, capi.XCK_E_ARG), ei.value
        eng.reset()
        assert eng.ingest_bam(bam) == n0
        got = eng.finish()
        for k in whole:
            for a, b in zip(whole[k], got[k]):
                assert np.array_equal(np.array(b), a), k
    finally:
        eng.close()


def _bgzf_block(payload, level=6, strategy=None, flushes=()):
    """One BGZF block around a raw DEFLATE stream made by zlib with the given level / strategy; `flushes` = offsets at which the
    stream is flushed (Z_FULL_FLUSH: an empty stored block in the middle of the stream, then a new block)."""
    import struct
    import zlib
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY if strategy is None else strategy)
    out, at = b"", 0
    for f in list(flushes) + [len(payload)]:
        out += co.compress(payload[at:f])
        if f < len(payload):
            out += co.flush(zlib.Z_FULL_FLUSH)
        at = f
    out += co.flush()
    assert len(out) + 26 <= 65536, len(out)
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(out) + 25) + out
            + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def test_device_decoder_on_crafted_streams(tmp_path):
    """csrc/inflate_dev.hip against zlib on streams the synthetic BAMs do not hold: stored blocks (incompressible bytes, level 0),
    fixed-Huffman blocks, Huffman-only and run-length streams, several DEFLATE blocks per BGZF block with empty stored blocks between
    them, distance-1 and short-period overlapping matches of the maximum length, code lengths up to 15 bits, empty and tiny blocks.
    Every block must equal zlib's output or be left to the host (status != 0);
    none may be wrong, and no more than a handful may be left."""
    import zlib
    exe = os.path.join(ROOT, "xcltk_amd", "csrc", "xck_gpu_inflate_check")
    assert os.path.isfile(exe), "built by __graft_entry__.build() / make -C xcltk_amd/csrc"
    rng = np.random.default_rng(5)
    blocks = []
    def add(payload, **kw):
        blocks.append(_bgzf_block(bytes(payload), **kw))
    add(b"")                                                          # the BGZF end-of-file block: a fixed-Huffman block holding only end-of-block
    add(b"A"); add(b"AC"); add(b"ACG" * 5)
    rnd = rng.integers(0, 256, 60000, dtype=np.uint8).tobytes()
    add(rnd); add(rnd, level=0); add(rnd[:40000], flushes=(1, 2, 1000, 20000))   # stored blocks, also in the middle of a stream
    add(bytes(65000))                                                 # zeros: distance 1, length 258, over and over
    for period in (1, 2, 3, 5, 7, 13, 64, 255, 256, 257, 258, 259, 1000, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768):
        unit = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
        add((unit * (65000 // period + 1))[:65000])
        add((unit * (65000 // period + 1))[:65000], strategy=zlib.Z_RLE)
    alphabet = np.frombuffer(b"ACGTN\n\t!#IF:,0123456789abcdefXYZxyz-_=+*", dtype=np.uint8)
    w = np.array([2.0 ** -min(i, 20) for i in range(len(alphabet))])
    text = bytes(rng.choice(alphabet, 64000, p=w / w.sum()))
    for kw in (dict(), dict(level=1), dict(level=9), dict(strategy=zlib.Z_FIXED), dict(strategy=zlib.Z_HUFFMAN_ONLY), dict(strategy=zlib.Z_FILTERED),
               dict(flushes=(10, 11, 5000, 5001, 30000))):
        add(text, **kw)
    # code lengths up to 15 bits: symbol frequencies that fall like Fibonacci numbers (Huffman-only: the literal code alone decides)
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    skew = np.concatenate([np.full(f, i, dtype=np.uint8) for i, f in enumerate(fib)])
    skew = np.concatenate([skew, np.arange(24, 256, dtype=np.uint8)])[:64000]
    rng.shuffle(skew)
    add(skew.tobytes(), strategy=zlib.Z_HUFFMAN_ONLY); add(skew.tobytes(), level=9)
    # many blocks of BAM-like records at every level
    rec = b"".join(b"%04d\0read%06d\0" % (i % 7919, i) + bytes(rng.integers(0, 4, 40, dtype=np.uint8)) + b"IIIIFFFF" * 6 + b"CBZACGTACGTACGTACGT-1\0UBZACGTACGTAC\0" for i in range(500))
    for lvl in range(0, 10):
        add(rec[: 60000], level=lvl)
    fn = os.path.join(str(tmp_path), "crafted.bgzf")
    open(fn, "wb").write(b"".join(blocks))
    for variant in ("0", "10"):                                       # (10: the same kernel with its phase clocks compiled in)
        r = subprocess.run([exe, fn], env=dict(os.environ, INFLATE_VARIANT=variant, INFLATE_STATUSES="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
        line = [l for l in r.stdout.splitlines() if l.startswith("verified against zlib")]
        assert r.returncode == 0 and line, r.stdout[-2000:]
        wrong, left = int(line[0].split(":")[1].split()[0]), int(line[0].split("wrong,")[1].split()[0])
        st = [int(x) for l in r.stdout.splitlines() if l.startswith("statuses:") for x in l.split()[1:]]
        which = {k: s for k, s in enumerate(st) if s != 0}                # (block index in the order of the add() calls above -> status)
        assert len(st) == len(blocks) and "%d blocks" % len(blocks) in r.stdout and wrong == 0 and left == 0 and not which, (variant, line[0], which)
