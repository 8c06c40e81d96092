"""Every column of every record: xck_gpu_parse_check (tools/gpu_parse_check.hip) runs inflate + walk + scan + parse on the device chunk
by chunk and compares the nine SoA columns with what the host's parse_record (csrc/bam_records.cpp) writes for the same bytes - on synthetic
files of the headline shape (levels 0 and 6), of the Cell Ranger shape and without tags, and on a crafted file with the records the
synthetic ones do not hold (empty and one-record blocks, a record that fills its block, no CIGAR, no / odd-length sequence, CB of
type A and H, B arrays ahead of CB, a duplicated tag, a Z value without its NUL, barcodes outside the list, a contig change inside a
block, unmapped records at the end, more contig runs in a block than a summary holds).  Reference boundary: pysam's get_tag
(xcltk/utils/sam.py) as restated by parse_record."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from xcltk_amd.synth import bamwriter, soa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "xcltk_amd", "csrc", "xck_gpu_parse_check")


def _check(bam, barcodes, **env):
    assert os.path.isfile(EXE), "built by __graft_entry__.build() / make -C xcltk_amd/csrc"
    r = subprocess.run([EXE, bam, barcodes], env=dict(os.environ, **{k: str(v) for k, v in env.items()}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True, timeout=120)
    line = [l for l in r.stdout.splitlines() if "records compared" in l]
    assert line, r.stdout[-2000:]
    v = [int(x) for x in re.findall(r"-?\d+", line[0])]            # chunks, records, differences, flagged, flags, flagged without cause
    out = dict(chunks=v[0], records=v[1], differences=v[2], flagged=v[3], without_cause=v[5], rc=r.returncode, text=r.stdout[-2000:])
    print(line[0])
    return out


def _inputs(tmp):
    regions, snps, names = soa.make_tables(2000, 1000, soa.HG38_LENGTHS, seed=2)
    rng = np.random.default_rng(7)
    bcs = sorted({"".join("ACGT"[i] for i in rng.integers(0, 4, 16)) + "-1" for _ in range(500)})
    open(os.path.join(tmp, "contigs.tsv"), "w").write("".join("chr%s\t%d\n" % (n, l) for n, l in zip(names, soa.HG38_LENGTHS)))
    open(os.path.join(tmp, "regions.tsv"), "w").write("".join("chr%s\t%d\t%d\t%s\n" % r for r in regions))
    open(os.path.join(tmp, "barcodes.tsv"), "w").write("".join(b + "\n" for b in bcs))
    return names, bcs


@pytest.mark.parametrize("level,shape,notags", [(0, None, False), (6, None, False), (6, "cellranger", False), (6, None, True)])
def test_columns_of_synthetic_files(level, shape, notags, tmp_path):
    tmp = str(tmp_path)
    _inputs(tmp)
    bam = os.path.join(tmp, "s.bam")
    env = dict(os.environ)
    if shape:
        env["XCK_SYNTH_SHAPE"] = shape
    if notags:
        env["XCK_SYNTH_NOTAGS"] = "1"
    subprocess.check_call([os.path.join(ROOT, "xcltk_amd", "csrc", "xck_synth_bam"), bam, os.path.join(tmp, "contigs.tsv"), os.path.join(tmp, "regions.tsv"),
                           os.path.join(tmp, "barcodes.tsv"), "200000", "11", "8", str(level)], stderr=subprocess.DEVNULL, env=env)
    for extra in (dict(), dict(PARSE_SEQ=0, PARSE_DROP=3, PARSE_TEND=100000000)):
        got = _check(bam, os.path.join(tmp, "barcodes.tsv"), **extra)
        assert got["rc"] == 0 and got["differences"] == 0 and got["flagged"] == 0 and got["records"] > 50000 and got["chunks"] > 3, got


def test_columns_of_a_crafted_file(tmp_path):
    tmp = str(tmp_path)
    names, bcs = _inputs(tmp)
    rng = np.random.default_rng(11)
    refs = [("chr%s" % nm, l) for nm, l in zip(names, soa.HG38_LENGTHS)]
    path = os.path.join(tmp, "crafted.bam")
    w = bamwriter.BamWriter(path, refs)                              # (the header, in blocks of its own)

    def seq(n):
        return "".join("ACGT"[k] for k in rng.integers(0, 4, n))

    def rec(tid, pos, cigar="60M", s=None, tags=None, name="r"):
        s = seq(60) if s is None else s
        tags = [("CB", bcs[int(rng.integers(0, len(bcs)))]), ("UB", seq(10))] if tags is None else tags
        return bamwriter.pack_record(tid, pos, name + "%05d" % int(rng.integers(0, 99999)), 0, 60, cigar, s, tags)[0]

    def no_nul(blob):                                                # the last tag's Z value loses its NUL
        body = blob[4:-1]
        return struct.pack("<i", len(body)) + body

    ordinary = lambda tid, n, p0=1000: [rec(tid, p0 + 10 * i) for i in range(n)]
    blocks = [ordinary(0, 40), [], [rec(0, 5000)], ordinary(0, 30, 6000)]                  # blocks with 0 and with 1 record
    fill = rec(0, 7000, s=seq(400), tags=[("CB", bcs[3]), ("UB", seq(10)), ("XX", "x" * 200)])
    blocks.append([fill])                                                                  # (its payload is the record exactly: see below)
    blocks.append([rec(0, 8000, cigar=""), rec(0, 8010, s=""), rec(0, 8020, cigar="61M", s=seq(61)), rec(0, 8030, cigar="", s=""),
                   rec(0, 8040, tags=[("CB", "A", "A"), ("UB", seq(10))]), rec(0, 8050, tags=[("CB", "1AE3", "H"), ("UB", seq(10))]),
                   rec(0, 8060, tags=[("XB", ("s", [1, -2, 3]), "B"), ("YB", ("C", list(range(50))), "B"), ("ZB", ("f", [1.5]), "B"), ("CB", bcs[5]), ("UB", seq(10))]),
                   rec(0, 8070, tags=[("CB", bcs[6]), ("CB", bcs[7]), ("UB", seq(10)), ("UB", seq(10))]),           # duplicated tags: the first wins
                   no_nul(rec(0, 8080, tags=[("UB", seq(10)), ("CB", bcs[8])])), no_nul(rec(0, 8090, tags=[("CB", bcs[9]), ("UB", seq(9))])),
                   rec(0, 8100, tags=[("CB", "TTTTTTTTTTTTTTTT-9"), ("UB", seq(10))]), rec(0, 8110, tags=[("CB", "ACGTACGTACGTACGTACGTACGT-1"), ("UB", seq(10))]),
                   rec(0, 8120, tags=[("UB", seq(10))]), rec(0, 8130, tags=[("CB", bcs[1])]), rec(0, 8140, tags=[]), rec(0, 8150, tags=[("UB", "")]),
                   rec(0, 8160, tags=[("NH", 1, "i"), ("AS", 3, "C"), ("xs", -7, "s"), ("fl", 0.5, "f"), ("CB", bcs[2]), ("UB", seq(12))])])
    blocks.append(ordinary(0, 10, 9000) + ordinary(1, 10) + ordinary(2, 10))               # contig changes inside a block
    blocks += [ordinary(3, 50) for _ in range(10)]
    blocks.append(ordinary(4, 20) + [rec(-1, -1) for _ in range(20)])                      # unmapped records at the end ...
    blocks.append([rec(-1, -1) for _ in range(30)])
    while len(blocks) % 8:
        blocks.append([rec(-1, -1)])
    blocks.append([rec(t, 1000 + i) for i, t in enumerate([0, 1, 0, 1, 0, 1, 0, 1])])      # ... and, in a chunk of its own, more runs than a summary holds
    assert len(b"".join(blocks[4])) == len(fill) and blocks[4] == [fill]
    for blk in blocks:
        payload = b"".join(blk)
        assert len(payload) <= 0xff00
        w.fp.write(bamwriter.bgzf_block(payload))
    w.close()
    for extra in (dict(), dict(PARSE_SEQ=0), dict(PARSE_DROP=2), dict(PARSE_TEND=8100)):
        got = _check(path, os.path.join(tmp, "barcodes.tsv"), PARSE_CHUNK_BLOCKS=8, **extra)
        assert got["rc"] == 0 and got["differences"] == 0 and got["without_cause"] == 0 and got["records"] > 100, got      # (639 kept records with every reference wanted)
        assert got["flagged"] == 1, got                              # the chunk of the last block alone
