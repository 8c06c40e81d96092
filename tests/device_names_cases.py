"""What the device-names tests share (tests/test_device_names_cases_host.py on the CPU, tests/test_gpu_device_names.py on the GPU): the
small BAMs whose read names are the keys - pairs of records that share a name, cell and region and lie many chunks apart, mates a
few records apart over one SNP, names of every shape the key rule tells apart - with their tables, and the expected matrices from
oracle/pybam.py plus the oracle.  Nothing here calls the product decoder.

The files come from synth/bamwriter.py in BGZF blocks of 3,000 bytes; a reader with XCK_CHUNK_BYTES = CHUNK_BYTES cuts them into
chunks of about 70 blocks (the device takes chunks of 64 blocks and more, csrc/bam.cpp schedule_chunk) and a short tail chunk."""
import os

import numpy as np

import oracle as O
import pybam
import reblock
from xcltk_amd import capi
from xcltk_amd.synth import bamwriter

CHUNK_BYTES = 200000
BLOCK_PAYLOAD = 3000
MIN_BLOCKS = 64                  # csrc/bam.cpp schedule_chunk
N = 24000
HALF = N // 2
REFS = [("chr1", 2000000)]
NAMES = ["1"]
BARCODES = ["ACGTACGTACGTAC%s-1" % (a + b) for a in "AC" for b in "ACGT"]       # 8 barcodes of 18 bytes
REGIONS = [("1", 1, 2000000, "whole"), ("1", 100001, 300000, "a"), ("1", 500001, 900000, "b"), ("1", 1200001, 1500000, "c")]
SNP_POS = 50030                  # 1-based
BAF_REGIONS = [("1", 40001, 60000, "g")]
BAF_SNPS = [("1", SNP_POS, "A", "G", 0, 1)]


def _seq(rng, n=60):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def write_shared(path, align=True):
    """Record i and record i + 12,000 share name, cell and position (so every region): the file is two passes over the same sorted
    positions.  -> the list of (name, cell) per record"""
    rng = np.random.default_rng(5)
    pos = np.sort(rng.integers(1000, 1900000, HALF))
    cell = rng.integers(0, len(BARCODES), HALF)
    w = bamwriter.BamWriter(path, REFS, align_records=align, block_payload=BLOCK_PAYLOAD)
    out = []
    for i in range(N):
        k = i % HALF
        w.write(0, int(pos[k]), "r%07d" % k, 0, 60, "60M", _seq(rng), [("CB", BARCODES[int(cell[k])])])
        out.append(("r%07d" % k, int(cell[k])))
    w.close()
    return out


def write_mates(path):
    """All records over one SNP; the mates of a pair (same name, cell and base at the SNP) lie 1, 2, 3 and 2 records apart:
    x x y z y w z w per eight records.  -> the pair index of every record"""
    rng = np.random.default_rng(6)
    order = (0, 0, 1, 2, 1, 3, 2, 3)
    w = bamwriter.BamWriter(path, REFS, align_records=True, block_payload=BLOCK_PAYLOAD)
    pair_of, start = [], np.sort(rng.integers(SNP_POS - 1 - 55, SNP_POS - 1 - 4, N))      # 0-based starts: the SNP lies inside every read
    base, cell = {}, {}
    for i in range(N):
        p = (i // 8) * 4 + order[i % 8]
        if p not in base:
            base[p], cell[p] = "AGC"[int(rng.integers(0, 3))], int(rng.integers(0, len(BARCODES)))
        s = list(_seq(rng))
        s[SNP_POS - 1 - int(start[i])] = base[p]
        w.write(0, int(start[i]), "m%07d" % p, 0, 60, "60M", "".join(s), [("CB", BARCODES[cell[p]])])
        pair_of.append(p)
    w.close()
    return pair_of


SHAPES = ["", "x", "abcdefgh", "abcdefghi", "n" * 254, "n" * 253 + "m", "ACGT", "ACGTACGTAC", "TTTT", "TTTTT", "ACGTN", "qqqq", "qqqqq", "A", "N"]
N_SHAPES_FILE = 6000


def write_shapes(path):
    """Every name of SHAPES twice in cell 0 - once near the file's start, once in its last records (the tail chunk) - and once in cell 1,
    in mid-file; "ACGT" a third time in cell 0 right behind its first copy (a mate of itself).  All other records have names of their
    own and cells 2 .. 7.  One region holds them all.  -> {record index: (name, cell)} of the shaped records"""
    rng = np.random.default_rng(8)
    pos = np.sort(rng.integers(1000, 1900000, N_SHAPES_FILE))
    at = {}
    for k, s in enumerate(SHAPES):
        at[100 + 3 * k] = (s, 0)
        at[N_SHAPES_FILE // 2 + 5 * k] = (s, 1)
        at[N_SHAPES_FILE - 60 + 2 * k] = (s, 0)
    at[100 + 3 * SHAPES.index("ACGT") + 1] = ("ACGT", 0)
    w = bamwriter.BamWriter(path, REFS, align_records=True, block_payload=BLOCK_PAYLOAD)
    for i in range(N_SHAPES_FILE):
        name, cell = at.get(i, ("f%06d" % i, 2 + i % 6))
        w.write(0, int(pos[i]), name, 0, 60, "60M", _seq(rng), [("CB", BARCODES[cell])])
    w.close()
    return at


def expected(bam, mode, regions, snps, umi_bits, cell_tag="CB", sample=0, n_cells=None):
    """the matrices of pybam's records through the oracle, the read name as the key"""
    refs, recs = pybam.read_bam(bam)
    t2c = O.resolve_contigs([n for n, _ in refs], NAMES)
    cfg, keep = O.make_config(mode, NAMES, regions, snps if mode == capi.XCK_MODE_BAF else [], n_cells or len(BARCODES))
    cell_index = {b: i for i, b in enumerate(BARCODES)}
    batches = O.encode_bam(recs, t2c, sample, cell_index, cell_tag, None, umi_bits, {}, with_seq=True)
    return O.run_oracle(cfg, [b for b, _ in batches])


def chunk_of_record(bam, chunk_bytes=CHUNK_BYTES):
    """-> (chunk index of every record, blocks per chunk) for a record-aligned file, from its blocks alone"""
    blocks = reblock.block_records(bam)[2]
    chunks = reblock.plan_chunks(bam, chunk_bytes)
    out, at = [], 0
    for ci, n in enumerate(chunks):
        for b in blocks[at:at + n]:
            out += [ci] * len(b)
        at += n
    return out, chunks
