"""BGZF CRC32 checks of the record decoder on the host (no device needed): XCK_F_DEVICE_CRC and the XCK_VERIFY_CRC knob check every
block the decoder inflates - on a decode-only handle all of them on the host -, the batches of an intact file are those of an unchecked
run, and a damaged footer fails the decode with XCK_E_IO instead of being counted.  xck_decode_stats says how many blocks were checked
where.  Reference boundary: htslib checks the CRC of every BGZF block it reads (xcltk/rdr/fc/core.py:73-76, utils/sam.py:105-118)."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError
from xcltk_amd.synth import soa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("XCK_VERIFY_CRC", "XCK_CHUNK_BYTES")


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


def bgzf_blocks(raw):
    """[(offset, total length, isize)] of every BGZF block of a file."""
    out, o = [], 0
    while o + 18 <= len(raw):
        assert raw[o:o + 4] == b"\x1f\x8b\x08\x04", o
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


def record_blocks(raw):
    """Indices of the non-empty blocks from the one that holds the first alignment record to the end of the file."""
    blocks = bgzf_blocks(raw)
    data, ends = b"", []
    for o, total, isize in blocks:                                    # inflate until the header is complete
        xlen = struct.unpack_from("<H", raw, o + 10)[0]
        data += zlib.decompress(raw[o + 12 + xlen:o + total - 8], -15)
        ends.append(len(data))
        if len(data) >= 12:
            l_text = struct.unpack_from("<I", data, 4)[0]
            p = 8 + l_text
            if len(data) >= p + 4:
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


def flip_footer_crc(raw, at_fraction, bit=0):
    """A copy of the file with one bit of the footer CRC of the record block at about `at_fraction` of the file flipped."""
    blocks = bgzf_blocks(raw)
    rec = record_blocks(raw)
    i = rec[int(len(rec) * at_fraction)]
    o, total, _ = blocks[i]
    bad = bytearray(raw)
    bad[o + total - 8 + bit // 8] ^= 1 << (bit % 8)
    return bytes(bad), o


def _engine(regions, snps, names, bcs, flags=0):
    return Engine(capi.XCK_MODE_BAF, names, regions, len(bcs), snps=snps, barcodes=bcs, cell_tag="CB", umi_tag="UB", decode_only=True,
                  n_threads=4, flags=flags)


def _decode(bam, regions, snps, names, bcs, flags=0):
    eng = _engine(regions, snps, names, bcs, flags)
    try:
        got = list(eng.decode_bam(bam))
        return got, eng.decode_stats()
    finally:
        eng.close()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert np.array_equal(np.asarray(x[k]), np.asarray(y[k])), k


def test_ctypes_decode_stats_mirror_matches_the_header(tmp_path):
    """capi.DecodeStats is filled by xck_get_decode_stats through a plain pointer: its size and field offsets must be the C header's."""
    src = tmp_path / "sz.c"
    fields = [n for n, _ in capi.DecodeStats._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xck.h"\nint main(void) { printf("%zu", sizeof(xck_decode_stats));\n'
                   + "".join('printf(" %%zu", offsetof(xck_decode_stats, %s));\n' % n for n in fields) + "return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == C.sizeof(capi.DecodeStats)
    assert got[1:] == [getattr(capi.DecodeStats, n).offset for n in fields]


def test_decode_stats_refuses_a_short_struct():
    eng = Engine(capi.XCK_MODE_BASEFC, ["1"], [("1", 1, 100, "g")], 1, decode_only=True)
    try:
        st = capi.DecodeStats()
        st.struct_size = 8
        assert eng.lib.xck_get_decode_stats(eng.h, C.byref(st)) == capi.XCK_E_ARG
        assert all(v == 0 for v in eng.decode_stats().values())
    finally:
        eng.close()


@pytest.mark.parametrize("level", [6, 0])
def test_checked_decode_equals_the_unchecked_one(level, knob_env, tmp_path):
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 120000, level)
    knob_env["XCK_CHUNK_BYTES"] = str(1 << 20)                       # several chunks
    knob_env.pop("XCK_VERIFY_CRC", None)
    plain, st0 = _decode(bam, regions, snps, names, bcs)
    assert sum(b["n_reads"] for b in plain) == 120000
    assert st0["crc_blocks_host"] == 0 and st0["crc_blocks_device"] == 0
    n_rec = len(record_blocks(open(bam, "rb").read()))
    assert n_rec > 20
    for flags, knob in ((capi.XCK_F_DEVICE_CRC, None), (capi.XCK_F_VERIFY_CRC, None), (0, "host"), (0, "device")):
        if knob:
            knob_env["XCK_VERIFY_CRC"] = knob
        else:
            knob_env.pop("XCK_VERIFY_CRC", None)
        got, st = _decode(bam, regions, snps, names, bcs, flags)
        _same(plain, got)
        # a decode-only handle has no device: the host checks every record block
        assert st["crc_blocks_host"] == n_rec, (flags, knob, st)
        for k in ("gpu_inflate_chunks", "gpu_inflate_blocks", "gpu_blocks_left_to_host", "crc_blocks_device", "crc_mismatch_device",
                  "crc_device_host_disagree", "gpu_path_given_up"):
            assert st[k] == 0, (flags, knob, k, st)


def test_counters_add_up_over_readers(knob_env, tmp_path):
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 40000, 6)
    knob_env.pop("XCK_VERIFY_CRC", None)
    n_rec = len(record_blocks(open(bam, "rb").read()))
    eng = _engine(regions, snps, names, bcs, capi.XCK_F_DEVICE_CRC)
    try:
        list(eng.decode_bam(bam))
        assert eng.decode_stats()["crc_blocks_host"] == n_rec
        list(eng.decode_bam(bam))
        assert eng.decode_stats()["crc_blocks_host"] == 2 * n_rec
    finally:
        eng.close()


@pytest.mark.parametrize("bit", [0, 31])
def test_damaged_footer_fails_a_checked_decode_only(bit, knob_env, tmp_path):
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 120000, 6)
    knob_env["XCK_CHUNK_BYTES"] = str(1 << 20)
    knob_env.pop("XCK_VERIFY_CRC", None)
    raw = open(bam, "rb").read()
    intact, _ = _decode(bam, regions, snps, names, bcs)
    bad, coff = flip_footer_crc(raw, 0.5, bit)
    fn = os.path.join(str(tmp_path), "bad_footer.bam")
    open(fn, "wb").write(bad)
    for flags, knob in ((capi.XCK_F_DEVICE_CRC, None), (0, "host"), (0, "device"), (capi.XCK_F_VERIFY_CRC, None)):
        if knob:
            knob_env["XCK_VERIFY_CRC"] = knob
        else:
            knob_env.pop("XCK_VERIFY_CRC", None)
        with pytest.raises(XckError) as ei:
            _decode(fn, regions, snps, names, bcs, flags)
        msg = str(ei.value)
        assert ei.value.code == capi.XCK_E_IO and "CRC" in msg, (flags, knob, msg)
        assert "bad_footer.bam" in msg and str(coff) in msg, msg     # the file and the block's compressed offset
    # no flag, no knob: the default is unchanged - the footer is not read, the damaged file decodes like the intact one
    knob_env.pop("XCK_VERIFY_CRC", None)
    got, st = _decode(fn, regions, snps, names, bcs)
    _same(intact, got)
    assert st["crc_blocks_host"] == 0
