"""csrc/inflate_fast.h - the host decoder that takes over whatever the device declines - on the corpus of tests/deflate_corpus.py:
DEFLATE streams that zlib's compressor never writes (runs of code lengths across the HLIT/HDIST border, non-longest and far matches,
48-bit symbols, codes at the 15-bit limit, hundreds of DEFLATE blocks per BGZF block, stored blocks at every bit phase ...) and
streams that are wrong in one place.  xck_inflate_test holds every block against zlib; with INFLATE_STATUSES=1 it also prints the
decoder's verdict per block.  Needs no GPU; the corpus itself is proven against zlib while it is made."""
import os
import subprocess

import pytest

import deflate_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def corpus_file(tmp_path_factory):
    data, recs = deflate_corpus.corpus()
    fn = str(tmp_path_factory.mktemp("streams") / "corpus.bgzf")
    with open(fn, "wb") as f:
        f.write(data)
    return fn, recs


def test_the_corpus_is_what_it_says(corpus_file):
    """Sizes, alignments and the placing of the invalid blocks, from the file offsets."""
    import deflate_craft as dc
    fn, recs = corpus_file
    data = open(fn, "rb").read()
    blocks = dc.bgzf_blocks(data)
    assert len(blocks) == len(recs) and 200 <= len(recs) <= 600
    n_ld = sum(1 for r in recs if r["group"] == "libdeflate")
    print("libdeflate-written blocks (optional): %s" % (n_ld if n_ld else "absent, libdeflate.so.0 does not load here"))
    for (off, raw, isize), r in zip(blocks, recs):
        assert off == r["offset"] and isize == len(r["payload"]) and (off + 18) % 4 == r["A"], r["name"]
        ok, out = dc.zlib_verdict(raw, isize)
        assert ok == r["valid"] and (not ok or out == r["payload"]), r["name"]
    assert 1e6 < sum(len(r["payload"]) for r in recs) < 5e6
    invalid = [k for k, r in enumerate(recs) if not r["valid"]]
    assert 15 <= len(invalid) <= 30 and 0 < min(invalid) and max(invalid) < len(recs) - 1
    # the alignment-sensitive groups exist at every A = address & 3 of the stream
    stems = {}
    for r in recs:
        if r["group"] in deflate_corpus.ALIGNED_GROUPS:
            # (the A measured from the file offset is cut out of the name: a name that keeps its "_A<n>" says the block is not where it asked to be)
            stem = r["name"].replace("_A%d" % r["A"], "_A*")
            assert stem != r["name"], r["name"]
            stems.setdefault(stem, set()).add(r["A"])
    assert len(stems) >= 10 and all(v == {0, 1, 2, 3} for v in stems.values()), stems
    assert {r["A"] for r in recs if r["group"] == "parse"} == {0, 1, 2, 3}


def test_host_decoder_on_the_corpus(corpus_file):
    """Every valid block: rc 0 and zlib's bytes (`mismatches 0`); every invalid block: rc != 0."""
    fn, recs = corpus_file
    exe = os.path.join(ROOT, "xcltk_amd", "csrc", "xck_inflate_test")
    assert os.path.isfile(exe), "built by __graft_entry__.build() / make -C xcltk_amd/csrc"
    r = subprocess.run([exe, fn], env=dict(os.environ, INFLATE_STATUSES="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    line = [l for l in r.stdout.splitlines() if l.startswith("statuses:")]
    assert line, r.stdout[-2000:]
    rc = [int(x) for x in line[0].split()[1:]]
    assert len(rc) == len(recs), (len(rc), len(recs))
    declined = {x["name"]: c for x, c in zip(recs, rc) if c != 0}
    invalid = {x["name"] for x in recs if not x["valid"]}
    assert set(declined) - invalid == set(), "valid blocks the host decoder declines: %s" % {n: declined[n] for n in set(declined) - invalid}
    assert invalid - set(declined) == set(), "invalid blocks the host decoder lets pass: %s" % sorted(invalid - set(declined))
    assert r.returncode == 0 and " mismatches 0 " in r.stdout, r.stdout[-2000:]
