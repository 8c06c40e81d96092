"""csrc/inflate_dev.hip on DEFLATE streams that zlib's compressor never writes (tests/deflate_corpus.py: runs of code lengths across
the HLIT/HDIST border as libdeflate writes them, non-longest / far / overlapping matches, 48-bit symbols across the input window's
borders, match batches whose lengths sum to exactly 64 and 65, codes at the 15-bit limit, hundreds of DEFLATE blocks per BGZF block,
stored blocks at every bit phase and alignment) and on streams that are wrong in one place.  The reference is zlib's inflate, block by
block, inside xck_gpu_inflate_check; INFLATE_STATUSES=1 makes it print every block's status.  A valid block must come back with
status 0 and zlib's bytes - none may be left to the host: a complete code never exceeds the kernel's table budget (DESIGN.md
section 6) -, an invalid one with a status that is not 0.  Then the same kind of streams through the whole ingest."""
import os
import random
import subprocess

import numpy as np
import pytest

import deflate_corpus
import deflate_craft
from test_gpu_inflate import KNOBS, _count, _make_bam

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def corpus_file(tmp_path_factory):
    data, recs = deflate_corpus.corpus()
    fn = str(tmp_path_factory.mktemp("streams") / "corpus.bgzf")
    with open(fn, "wb") as f:
        f.write(data)
    return fn, recs


@pytest.mark.parametrize("crc", [False, True])
@pytest.mark.parametrize("variant", ["0", "10"])                      # (10: the same kernel with its phase clocks compiled in)
def test_device_decoder_on_the_corpus(corpus_file, variant, crc):
    fn, recs = corpus_file
    exe = os.path.join(ROOT, "xcltk_amd", "csrc", "xck_gpu_inflate_check")
    assert os.path.isfile(exe), "built by __graft_entry__.build() / make -C xcltk_amd/csrc"
    env = dict(os.environ, INFLATE_VARIANT=variant, INFLATE_STATUSES="1")
    if crc:
        env["INFLATE_CRC"] = "1"
    r = subprocess.run([exe, fn], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    lines = {l.split(":")[0]: l for l in r.stdout.splitlines()}
    assert "verified against zlib" in lines and "statuses" in lines, r.stdout[-2000:]
    st = [int(x) for x in lines["statuses"].split()[1:]]
    assert len(st) == len(recs) and "%d blocks" % len(recs) in r.stdout, (len(st), len(recs))
    print(lines["verified against zlib"])
    refused = {x["name"]: s for x, s in zip(recs, st) if s != 0}
    print("refused:", refused)
    assert "verified against zlib: 0 blocks wrong" in r.stdout and r.returncode == 0, (lines["verified against zlib"], r.stdout[-1500:])
    invalid = {x["name"] for x in recs if not x["valid"]}
    passed = invalid - set(refused)
    assert not passed, "invalid blocks the device lets pass: %s" % sorted(passed)
    left = set(refused) - invalid
    assert left <= deflate_corpus.MAY_BE_LEFT, "valid blocks left to the host: %s" % {n: refused[n] for n in left - deflate_corpus.MAY_BE_LEFT}
    assert set(refused) == invalid | (left & deflate_corpus.MAY_BE_LEFT)
    if crc:
        print(lines["crc on the device"])
        # every valid block CRC-checked and found good (the invalid ones carry the CRC of what they claim to hold: never reached)
        n_valid = len(recs) - len(invalid)
        assert "crc on the device: %d verified, 0 mismatched, %d left, 0 disagree with zlib" % (n_valid - len(left), len(refused)) in r.stdout, lines["crc on the device"]


@pytest.fixture
def knob_env():
    saved = {k: os.environ.get(k) for k in KNOBS}
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def test_ingest_of_a_redeflated_bam(knob_env, tmp_path):
    """A zlib-written BAM and the same BAM with every BGZF block re-deflated by the random-parse writer (1 .. 6 DEFLATE blocks of
    mixed type per BGZF block, the payload boundaries kept): the device share and the host decoder give the same matrices."""
    bam, regions, snps, names, bcs = _make_bam(str(tmp_path), 20000, 6)
    data = open(bam, "rb").read()
    n_blocks = len(deflate_craft.bgzf_blocks(data))
    assert 70 <= n_blocks <= 130, n_blocks                             # (a chunk goes to the device from 64 blocks on)
    re_bam = os.path.join(str(tmp_path), "redeflated.bam")
    with open(re_bam, "wb") as f:
        f.write(deflate_craft.redeflate_bgzf(data, random.Random(3)))
    knob_env["XCK_CHUNK_BYTES"] = str(8 << 20)                        # (48 MB by default) the whole file is one chunk
    knob_env["XCK_GPU_INFLATE_MIN_MB"] = "0"
    knob_env["XCK_GPU_INFLATE"] = "100"
    n0, orig, st0 = _count(bam, regions, snps, names, bcs)
    n1, dev, st1 = _count(re_bam, regions, snps, names, bcs)
    knob_env["XCK_GPU_INFLATE"] = "0"
    n2, host, st2 = _count(re_bam, regions, snps, names, bcs)
    assert n0 == n1 == n2 == 20000 and len(orig["count"][0]) > 1000
    assert st0["gpu_inflate_chunks"] >= 1 and st1["gpu_inflate_chunks"] >= 1 and st2["gpu_inflate_chunks"] == 0, (st0["gpu_inflate_chunks"], st1["gpu_inflate_chunks"])
    for k in orig:
        for a, b, c in zip(orig[k], dev[k], host[k]):
            assert np.array_equal(a, b) and np.array_equal(a, c), k
