"""BGZF CRC32 checks on the device (XCK_F_DEVICE_CRC, XCK_VERIFY_CRC=device): the inflate kernel (csrc/inflate_dev.hip, check_crc)
checks the blocks it inflates, the host those it leaves, the matrices of intact files are those of an unchecked run, and a damaged
block - a bad footer, or a changed payload byte that still inflates to isize bytes - fails the ingest with XCK_E_IO, found by the GPU.
Reference boundary: htslib checks the CRC of every BGZF block it reads (xcltk/rdr/fc/core.py:73-76, utils/sam.py:105-118)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError
from xcltk_amd.synth import soa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("XCK_GPU_INFLATE", "XCK_GPU_INFLATE_DEPTH", "XCK_GPU_INFLATE_MIN_MB", "XCK_CHUNK_BYTES", "XCK_VERIFY_CRC")


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


def _bgzf_blocks(raw):
    """[(offset, total length, isize)] of every BGZF block of a file."""
    out, o = [], 0
    while o + 18 <= len(raw):
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        x, bsize = o + 12, None
        while x + 4 <= o + 12 + xlen:
            sl = struct.unpack_from("<H", raw, x + 2)[0]
            if raw[x:x + 2] == b"BC" and sl == 2:
                bsize = struct.unpack_from("<H", raw, x + 4)[0]
            x += 4 + sl
        total = bsize + 1
        out.append((o, total, struct.unpack_from("<I", raw, o + total - 4)[0]))
        o += total
    return out


def _record_blocks(raw):
    """Indices of the non-empty blocks from the one that holds the first alignment record to the end of the file."""
    blocks = _bgzf_blocks(raw)
    data = b""
    for o, total, isize in blocks:                                    # inflate until the header is complete
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        data += zlib.decompress(raw[o + 12 + xlen:o + total - 8], -15)
        if len(data) < 12:
            continue
        p = 8 + struct.unpack_from("<I", data, 4)[0]
        if len(data) < p + 4:
            continue
        n_ref, p, ok = struct.unpack_from("<I", data, p)[0], p + 4, True
        for _ in range(n_ref):
            if len(data) < p + 4 or len(data) < p + 8 + struct.unpack_from("<I", data, p)[0]:
                ok = False
                break
            p += 8 + struct.unpack_from("<I", data, p)[0]
        if ok:
            break
    ustart, idx = 0, []
    for i, (o, total, isize) in enumerate(blocks):
        if ustart + isize > p and isize > 0:                          # (p: uncompressed offset of the first record)
            idx.append(i)
        ustart += isize
    return idx


def _engine(regions, snps, names, bcs, flags=0):
    return Engine(capi.XCK_MODE_BOTH, names, regions, len(bcs), snps=snps, barcodes=bcs, cell_tag="CB", umi_tag="UB", min_include=0.9,
                  min_count=1, min_maf=0, no_dup_hap=True, min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True, n_threads=8, flags=flags)


def _count(bam, regions, snps, names, bcs, flags=0):
    eng = _engine(regions, snps, names, bcs, flags)
    try:
        n = eng.ingest_bam(bam)
        got = eng.finish()
        got = {k: tuple(np.array(a) for a in v) for k, v in got.items()}
        return n, got, eng.stats(), eng.decode_stats()
    finally:
        eng.close()


def _assert_same(a, b, what=""):
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert np.array_equal(np.asarray(x), np.asarray(y)), (what, k)


def _device_knobs(env, share="100", depth="4"):
    env["XCK_CHUNK_BYTES"] = str(6 << 20)                             # ~90 blocks per chunk: dozens of chunks, each large enough for the device
    env["XCK_GPU_INFLATE_MIN_MB"] = "0"                               # (auto mode leaves files below 96 MB to the host)
    env["XCK_GPU_INFLATE"], env["XCK_GPU_INFLATE_DEPTH"] = share, depth
    env.pop("XCK_VERIFY_CRC", None)


@pytest.mark.parametrize("level", [6, 0])
def test_device_crc_on_clean_files_changes_nothing(level, knob_env, tmp_path):
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 1500000, level)
    n_rec = len(_record_blocks(open(bam, "rb").read()))
    _device_knobs(knob_env)
    knob_env["XCK_GPU_INFLATE"] = "0"
    n0, host, _, ds0 = _count(bam, regions, snps, names, bcs)
    assert n0 == 1500000 and ds0["gpu_inflate_chunks"] == 0 and ds0["crc_blocks_host"] == 0
    for share, depth in (("100", "4"), ("auto", "3")):
        _device_knobs(knob_env, share, depth)
        n1, dev, st, ds = _count(bam, regions, snps, names, bcs, flags=capi.XCK_F_DEVICE_CRC)
        assert n1 == n0
        _assert_same(host, dev, share)
        assert st["gpu_inflate_chunks"] == ds["gpu_inflate_chunks"] >= 5, (share, ds)
        assert ds["crc_blocks_device"] >= 0.95 * ds["gpu_inflate_blocks"], (share, ds)     # the device checks its blocks, it does not hand them back
        assert ds["crc_blocks_device"] + ds["crc_blocks_host"] == n_rec, (share, ds, n_rec)
        assert ds["crc_mismatch_device"] == 0 and ds["crc_device_host_disagree"] == 0 and ds["gpu_path_given_up"] == 0, (share, ds)


def test_knob_device_equals_the_flag(knob_env, tmp_path):
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 1000000, 6)
    _device_knobs(knob_env)
    knob_env["XCK_GPU_INFLATE"] = "0"
    n0, host, _, _ = _count(bam, regions, snps, names, bcs)
    _device_knobs(knob_env)
    knob_env["XCK_VERIFY_CRC"] = "device"
    n1, dev, _, ds = _count(bam, regions, snps, names, bcs, flags=0)
    assert n1 == n0
    _assert_same(host, dev)
    assert ds["gpu_inflate_chunks"] > 0 and ds["crc_blocks_device"] > 0 and ds["crc_mismatch_device"] == 0, ds
    assert ds["crc_blocks_device"] + ds["crc_blocks_host"] == len(_record_blocks(open(bam, "rb").read()))


def _ingest_fails_on_crc(eng, fn):
    with pytest.raises(XckError) as ei:
        eng.ingest_bam(fn)
    assert ei.value.code == capi.XCK_E_IO and "CRC" in str(ei.value), ei.value
    return str(ei.value)


def test_damaged_footer_is_found_by_the_device(knob_env, tmp_path):
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 1000000, 6)
    _device_knobs(knob_env)
    n0, whole, _, _ = _count(bam, regions, snps, names, bcs)
    raw = open(bam, "rb").read()
    rec = _record_blocks(raw)
    o, total, _ = _bgzf_blocks(raw)[rec[len(rec) * 2 // 3]]
    bad = bytearray(raw)
    bad[o + total - 8] ^= 1                                           # bit 0 of the footer's CRC
    fn = os.path.join(str(tmp_path), "bad_footer.bam")
    open(fn, "wb").write(bytes(bad))
    eng = _engine(regions, snps, names, bcs, capi.XCK_F_DEVICE_CRC)
    try:
        msg = _ingest_fails_on_crc(eng, fn)
        assert "bad_footer.bam" in msg and str(o) in msg, msg
        ds = eng.decode_stats()
        assert ds["crc_mismatch_device"] >= 1 and ds["crc_device_host_disagree"] == 0, ds
        eng.reset()                                                   # the handle lives on: the intact file counts exactly
        assert eng.ingest_bam(bam) == n0
        got = eng.finish()
        _assert_same(whole, got)
        assert eng.decode_stats()["crc_mismatch_device"] == 0
    finally:
        eng.close()
    # no flag: the footer is not read, the damaged file counts like the intact one (the default is unchanged)
    n1, got, _, ds = _count(fn, regions, snps, names, bcs)
    assert n1 == n0 and ds["gpu_inflate_chunks"] > 0 and ds["crc_blocks_device"] == 0
    _assert_same(whole, got)
    # XCK_F_VERIFY_CRC alone: checked on the host, the device takes no part
    eng = _engine(regions, snps, names, bcs, capi.XCK_F_VERIFY_CRC)
    try:
        _ingest_fails_on_crc(eng, fn)
        assert eng.stats()["gpu_inflate_chunks"] == 0 and eng.decode_stats()["gpu_inflate_chunks"] == 0
    finally:
        eng.close()


def _bgzf(payload_deflated, crc, isize):
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(payload_deflated) + 25) + payload_deflated
            + struct.pack("<II", crc & 0xffffffff, isize))


def _deflate(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out = co.compress(payload) + co.flush()
    assert len(out) + 26 <= 65536, len(out)
    return out


@pytest.mark.parametrize("level", [0, 6])
def test_changed_payload_that_still_inflates_is_found_by_the_device(level, knob_env, tmp_path):
    """One byte of a mid-file block's data changed and the block re-deflated (stored at level 0, dynamic Huffman at 6) behind the
    ORIGINAL footer: it inflates cleanly to isize bytes, only the CRC tells."""
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 1000000, 6)
    _device_knobs(knob_env)
    raw = open(bam, "rb").read()
    blocks = _bgzf_blocks(raw)
    rec = _record_blocks(raw)
    i = rec[len(rec) * 2 // 3]
    o, total, isize = blocks[i]
    xlen = struct.unpack_from("<H", raw, o + 10)[0]
    p = zlib.decompress(raw[o + 12 + xlen:o + total - 8], -15)
    assert len(p) == isize and isize > 1000
    q = bytearray(p)
    q[isize // 2] ^= 0x5a
    crc, _ = struct.unpack_from("<II", raw, o + total - 8)
    assert crc == zlib.crc32(p) & 0xffffffff
    blk = _bgzf(_deflate(bytes(q), level), crc, isize)
    assert zlib.decompress(blk[18:-8], -15) == bytes(q)               # (a clean stream of isize bytes)
    fn = os.path.join(str(tmp_path), "changed_l%d.bam" % level)
    open(fn, "wb").write(raw[:o] + blk + raw[o + total:])
    eng = _engine(regions, snps, names, bcs, capi.XCK_F_DEVICE_CRC)
    try:
        _ingest_fails_on_crc(eng, fn)
        ds = eng.decode_stats()
        assert ds["crc_mismatch_device"] >= 1 and ds["crc_device_host_disagree"] == 0, ds
    finally:
        eng.close()


def test_kernel_checks_crc_on_crafted_blocks(tmp_path):
    """xck_gpu_inflate_check with INFLATE_CRC=1 on blocks of every size class and kind, written back to back (so the blocks' output
    offsets take every alignment mod 16): every correct footer passes, every wrong one is flagged (INFLATE_ST_CRC), none is wrong."""
    exe = os.path.join(ROOT, "xcltk_amd", "csrc", "xck_gpu_inflate_check")
    assert os.path.isfile(exe), "built by __graft_entry__.build() / make -C xcltk_amd/csrc"
    rng = np.random.default_rng(11)
    alphabet = np.frombuffer(b"ACGTN\n\t!#IF:,0123456789abcdefXYZxyz-_=+*", dtype=np.uint8)
    w = np.array([2.0 ** -min(i, 20) for i in range(len(alphabet))])
    text = bytes(rng.choice(alphabet, 65536, p=w / w.sum()))
    rnd = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    kinds = (("stored", 0, zlib.Z_DEFAULT_STRATEGY), ("fixed", 6, zlib.Z_FIXED), ("dynamic", 6, zlib.Z_DEFAULT_STRATEGY),
             ("rle", 6, zlib.Z_RLE), ("huffman", 6, zlib.Z_HUFFMAN_ONLY))
    blocks, wrong = [], set()
    wrong_kinds = ("bit0", "bit31", "ones", "other")
    k = 0
    for size in (0, 1, 15, 16, 17, 1023, 1024, 1025, 65536):
        for name, level, strategy in kinds:
            if name == "stored" and size == 65536:
                continue                                              # (64 KiB of stored bytes do not fit a BGZF block)
            payload = (rnd if name == "stored" else text)[:size]
            crc = zlib.crc32(payload) & 0xffffffff
            blocks.append(_bgzf(_deflate(payload, level, strategy), crc, size))
            if size == 0:
                continue                                              # (empty blocks are not checked, as on the host)
            bad = wrong_kinds[k % 4]
            k += 1
            if bad == "bit0":
                crc ^= 1
            elif bad == "bit31":
                crc ^= 1 << 31
            elif bad == "ones":
                crc = 0xffffffff if crc != 0xffffffff else 0
            else:
                other = bytearray(payload)
                other[size // 2] ^= 1
                crc = zlib.crc32(bytes(other)) & 0xffffffff
            wrong.add(len(blocks))
            blocks.append(_bgzf(_deflate(payload, level, strategy), crc, size))
            blocks.append(_bgzf(_deflate(payload, level, strategy), zlib.crc32(payload) & 0xffffffff, size))   # (and the right one again)
    fn = os.path.join(str(tmp_path), "crafted_crc.bgzf")
    open(fn, "wb").write(b"".join(blocks))
    for variant in ("0", "10"):
        r = subprocess.run([exe, fn], env=dict(os.environ, INFLATE_VARIANT=variant, INFLATE_CRC="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           universal_newlines=True, timeout=120)
        line = [l for l in r.stdout.splitlines() if l.startswith("verified against zlib")]
        assert r.returncode == 0 and line, r.stdout[-2000:]
        wrong_bytes = int(line[0].split(":")[1].split()[0])
        cl = [l for l in r.stdout.splitlines() if l.startswith("crc on the device:")]
        assert cl, r.stdout[-2000:]
        verified, mismatched, left, disagree = (int(cl[0].split(":")[1].split(",")[j].split()[0]) for j in range(4))
        flagged = {int(x) for x in cl[0].split("first mismatched blocks:")[1].strip(" )").split()}
        assert "%d blocks" % len(blocks) in r.stdout and wrong_bytes == 0, (variant, line[0])
        assert flagged == wrong and mismatched == len(wrong), (variant, sorted(flagged ^ wrong))
        assert disagree == 0 and left <= 4, (variant, cl[0])
        assert verified + mismatched + left == len(blocks) - sum(1 for b in blocks if struct.unpack_from("<I", b, len(b) - 4)[0] == 0)
