"""csrc/inflate_dev.hip on the streams of tests/test_inflate_tables_cases_host.py: dynamic headers at the edges of the code-length
code, of the runs and of the alphabet sizes; codes whose ranks cross the chunks of 64 symbols a lane owns one of each; the largest
sub-tables a code can ask for, prefixes with one sub-table and codes of two lengths under it; distance codes with no, one and too
many codes; several DEFLATE blocks that build their tables in the same LDS one after the other.  (That file shows on the CPU that
every stream is what it is named for, and that every payload uses every code its header defines.)  The reference is zlib's inflate,
block by block, inside xck_gpu_inflate_check: a valid block comes back with status 0 and zlib's bytes, an invalid one with another
status - and its valid neighbours intact; with INFLATE_CRC=1 the kernel's own read-back of every valid block agrees with the footer."""
import os
import subprocess

import pytest

import test_inflate_tables_cases_host as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def corpus_file(tmp_path_factory):
    data, recs = cases.corpus()
    fn = str(tmp_path_factory.mktemp("tables") / "tables.bgzf")
    with open(fn, "wb") as f:
        f.write(data)
    return fn, recs


@pytest.mark.parametrize("crc", [False, True])
@pytest.mark.parametrize("variant", ["0", "10"])                      # (10: the same kernel with its phase clocks compiled in)
def test_device_decoder_on_the_tables_corpus(corpus_file, variant, crc):
    fn, recs = corpus_file
    exe = os.path.join(ROOT, "xcltk_amd", "csrc", "xck_gpu_inflate_check")
    assert os.path.isfile(exe), "built by __graft_entry__.build() / make -C xcltk_amd/csrc"
    env = dict(os.environ, INFLATE_VARIANT=variant, INFLATE_STATUSES="1")
    env.pop("INFLATE_CRC", None)
    if crc:
        env["INFLATE_CRC"] = "1"
    r = subprocess.run(["timeout", "-k", "10", "120", exe, fn], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    lines = {l.split(":")[0]: l for l in r.stdout.splitlines()}
    assert "verified against zlib" in lines and "statuses" in lines, (r.returncode, r.stdout[-2000:])
    st = [int(x) for x in lines["statuses"].split()[1:]]
    assert len(st) == len(recs) and "%d blocks" % len(recs) in r.stdout, (len(st), len(recs))
    print(lines["verified against zlib"])
    refused = {x["name"]: s for x, s in zip(recs, st) if s != 0}
    print("refused:", refused)
    assert "verified against zlib: 0 blocks wrong" in r.stdout and r.returncode == 0, (lines["verified against zlib"], r.stdout[-1500:])
    invalid = {x["name"] for x in recs if not x["valid"]}
    assert not invalid - set(refused), "invalid blocks the device lets pass: %s" % sorted(invalid - set(refused))
    assert not set(refused) - invalid, "valid blocks left to the host: %s" % {n: refused[n] for n in set(refused) - invalid}
    if crc:
        print(lines["crc on the device"])
        # every valid block CRC-checked and found good (the invalid ones are refused before their CRC is looked at)
        assert "crc on the device: %d verified, 0 mismatched, %d left, 0 disagree with zlib" % (len(recs) - len(invalid), len(invalid)) in r.stdout, lines["crc on the device"]
