"""What the tag-filter tests share (tests/test_tag_filter_host.py on the CPU, tests/test_gpu_tag_filter.py on the GPU): a crafted 10x-shaped
BAM whose records carry the filter tag `xf` in every shape the rule of include/xck.h (xck_config.filter_tag) speaks of, the rule itself
restated on the records as oracle/pybam.py reads them, and the oracle of the feature: "pre-filter the file" - the passing records, in
their order, written to a second BAM that the unchanged oracle and an unfiltered engine then count.

Nothing here calls the product decoder.  The block shape (8 records per block, XCK_CHUNK_BYTES = 130000, so a chunk holds 64 blocks and
more) is the one tests/device_decode_cases.py uses for its crafted file."""
import os
import struct

import numpy as np

import oracle as O
import pybam
import reblock
from xcltk_amd.synth import bamwriter

TAG = "xf"
ALL = 0xFFFFFFFF
# name -> (value, mask): exact (Cell Ranger's "confidently mapped, counted"), one bit (the read counted for its UMI), every integer-typed
# non-negative tag, and a value no record carries
PREDICATES = {"exact": (25, ALL), "bit": (8, 8), "any_int": (0, 0), "none": (12345, ALL)}

REFS = [("chr1", 2000000), ("chr2", 2000000), ("chrU", 2000000)]            # the tables know 1 and 2
SLOTS = {0: 80, 1: 50}
SLOT = 20000
PER_SLOT = 28
N_CELLS = 40
N_UNKNOWN = 20                                                              # records on chrU: they reach no batch
N_UNMAPPED = 40
BLOCK_RECORDS = 8
CHUNK_BYTES = 130000                                                        # about 85 blocks of 8 records
SMALL_CHUNK_BYTES = 20000                                                   # the host tests: a dozen blocks per chunk, many chunks
UNLISTED = "TTTTGGGGCCCCAAAA-1"
# kept records (counted over the records on chr1 / chr2) whose UMI holds an N: the device leaves their chunks to the host.  With about
# 680 records per chunk they sit in the second and the fourth chunk; the first and the third stay on the device.
N_UMI_AT = (800, 1000, 1200, 2600)

# the filter tag of a record: a list of (tag, value, type), the first of which decides
KINDS_COMMON = [[(TAG, 25, t)] for t in "cCsSiI"]                          # every integer storage type
KINDS_RARE = [
    [(TAG, 17, "C")], [(TAG, 8, "C")], [(TAG, 0, "C")], [(TAG, 0, "i")], [(TAG, 24, "s")],
    [(TAG, 281, "S")], [(TAG, 300, "s")], [(TAG, 40000, "S")], [(TAG, 70025, "i")],          # values that need the wider types (281 = 256 + 25)
    [(TAG, -3, "c")], [(TAG, -300, "s")], [(TAG, -70000, "i")], [(TAG, -1, "i")],            # negative: fail, whatever their low bits
    [(TAG, 0x80000019, "I")], [(TAG, 4000000000, "I")], [(TAG, ALL, "I")],                   # above 2^31
    [],                                                                                     # absent
    [(TAG, "25", "Z")], [(TAG, "1", "A")], [(TAG, "19", "H")], [(TAG, 25.0, "f")], [(TAG, ("C", [25, 25]), "B")], [(TAG, ("i", [25]), "B")],
    [(TAG, 25, "C"), (TAG, 0, "C")], [(TAG, 0, "C"), (TAG, 25, "C")],                        # twice, different verdicts
    [(TAG, "25", "Z"), (TAG, 25, "C")], [(TAG, 25, "i"), (TAG, -1, "i")],
]

_B = "ACGT"


def _bases(rng, n):
    return "".join(_B[k] for k in rng.integers(0, 4, n))


def passes(rec, value, mask, tag=TAG):
    """the rule of xck_config.filter_tag on a pybam record (whose tags hold the first occurrence of every tag, with its type)"""
    if not rec.has_tag(tag):
        return False
    typ, v = rec.tags[tag]
    return typ in "cCsSiI" and 0 <= v <= ALL and (v & mask) == value


def craft(outdir):
    """Write <outdir>/{regions.tsv, snps.tsv, barcodes.tsv, crafted.bam}.  -> dict(bam, region_fn, snp_fn, barcode_fn, n_records)"""
    os.makedirs(outdir, exist_ok=True)
    rng = np.random.default_rng(715)
    cells = sorted({_bases(rng, 16) + "-1" for _ in range(N_CELLS + 8)})[:N_CELLS]
    regions, snps, per_tid, n_kept = [], [], {}, 0
    for tid in (0, 1):
        out = []
        for j in range(SLOTS[tid]):
            S = SLOT * j
            regions.append((REFS[tid][0][3:], S + 1, S + 600, "g%d_%03d" % (tid, j)))
            for k, d in enumerate((100, 300, 500)):
                snps.append((REFS[tid][0][3:], S + d, _B[k], _B[(k + 1) % 4], k & 1, 1 - (k & 1)))
            for p in np.sort(rng.integers(S, S + 520, PER_SLOT)).tolist():
                kind = KINDS_COMMON[int(rng.integers(0, len(KINDS_COMMON)))] if rng.random() < 0.5 else KINDS_RARE[int(rng.integers(0, len(KINDS_RARE)))]
                cb = ("CB", UNLISTED if rng.random() < 0.04 else cells[int(rng.integers(0, len(cells)))])
                ub = ("UB", "ACGTNACGTA" if n_kept in N_UMI_AT else _bases(rng, 10))
                where = int(rng.integers(0, 3))                             # the (first) filter tag: before CB, between CB and UB, last
                front = [("XB", ("s", [1, -2, 300]), "B"), ("XZ", "some text", "Z")] if rng.random() < 0.2 else []
                first, rest = kind[:1], kind[1:]
                tags = front + (first if where == 0 else []) + [cb] + (first if where == 1 else []) + [ub, ("NH", 1, "C")] + (first if where == 2 else []) + rest
                mapq = 5 if rng.random() < 0.04 else 60
                flag = 256 if rng.random() < 0.02 else 0
                out.append(bamwriter.pack_record(tid, int(p), "r%d_%d_%d" % (tid, j, len(out)), flag, mapq, [(0, 60)], _bases(rng, 60), tags)[0])
                n_kept += 1
        per_tid[tid] = out
    unknown = [bamwriter.pack_record(2, 1000 + 50 * k, "u%d" % k, 0, 60, [(0, 60)], _bases(rng, 60),
                                     [("CB", cells[k % len(cells)]), ("UB", _bases(rng, 10))] + ([(TAG, 25, "C")] if k & 1 else []))[0] for k in range(N_UNKNOWN)]
    unmapped = [bamwriter.pack_record(-1, -1, "x%d" % k, 4, 0, [], _bases(rng, 60), [("CB", cells[k % len(cells)]), ("UB", _bases(rng, 10))])[0]
                for k in range(N_UNMAPPED)]
    recs = per_tid[0] + per_tid[1] + unknown + unmapped
    out = dict(bam=os.path.join(outdir, "crafted.bam"), region_fn=os.path.join(outdir, "regions.tsv"), snp_fn=os.path.join(outdir, "snps.tsv"),
               barcode_fn=os.path.join(outdir, "barcodes.tsv"), n_records=len(recs))
    write_bam(out["bam"], header_bytes(REFS), recs)
    with open(out["region_fn"], "w") as fp:
        fp.write("".join("chr%s\t%d\t%d\t%s\n" % r for r in regions))
    with open(out["snp_fn"], "w") as fp:
        fp.write("chrom\tpos\tref\talt\tref_hap\talt_hap\n" + "".join("chr%s\t%d\t%s\t%s\t%d\t%d\n" % s for s in snps))
    with open(out["barcode_fn"], "w") as fp:
        fp.write("".join(b + "\n" for b in cells))
    return out


def header_bytes(refs):
    ht = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    hdr = b"BAM\x01" + struct.pack("<i", len(ht)) + ht.encode() + struct.pack("<i", len(refs))
    for n, l in refs:
        hdr += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    return hdr


def write_bam(path, header, recs, block_records=BLOCK_RECORDS):
    """header in a block of its own, then `block_records` whole records per BGZF block"""
    with open(path, "wb") as fp:
        fp.write(bamwriter.bgzf_block(header) + b"".join(bamwriter.bgzf_block(b"".join(recs[k:k + block_records])) for k in range(0, len(recs), block_records))
                 + bamwriter.BGZF_EOF)


def tables(c):
    """-> (contig names, regions, snps, sorted barcodes) of a crafted file, as the oracle's loaders read them"""
    regions, snps = O.load_regions(c["region_fn"]), O.load_snps(c["snp_fn"])
    with open(c["barcode_fn"]) as fp:
        barcodes = sorted(x.strip() for x in fp)
    return O.contig_table(regions, snps), regions, snps, barcodes


def verdicts(bam, names, value, mask, tag=TAG):
    """-> (pybam records of the file, pass per record, `in a batch` per record: on a contig of the table `names`)"""
    refs, recs = pybam.read_bam(bam)
    t2c = O.resolve_contigs([n for n, _ in refs], names)
    wanted = np.array([0 <= r.tid < len(t2c) and t2c[r.tid] >= 0 for r in recs], dtype=bool)
    return recs, np.array([passes(r, value, mask, tag) for r in recs], dtype=bool), wanted


def prefilter(src, dst, value, mask, tag=TAG, block_records=BLOCK_RECORDS):
    """The oracle of the feature: the records of `src` that pass, in their order, under the same header -> `dst`.  The verdicts are
    pybam's (gzip + the BAM specification); the bytes of a record are copied as they are (tests/reblock.py split_bam).
    -> (records kept, records of src)"""
    _, recs = pybam.read_bam(src)
    header, blobs = reblock.split_bam(src)
    assert len(blobs) == len(recs)
    keep = [b for b, r in zip(blobs, recs) if passes(r, value, mask, tag)]
    write_bam(dst, header, keep, block_records)
    return len(keep), len(blobs)


def tag_records(src, dst, seed=3):
    """A golden BAM (which holds no `xf`) with the tag appended to every record: xf:C:25 on three of four, and on the others 17, 0, a
    negative i, a Z string or nothing.  Same header and blocks of the source's size class (64 KB payloads).  -> number of records"""
    rng = np.random.default_rng(seed)
    header, blobs = reblock.split_bam(src)
    other = [bamwriter.pack_tag(TAG, 17, "C"), bamwriter.pack_tag(TAG, 0, "C"), bamwriter.pack_tag(TAG, -25, "i"), bamwriter.pack_tag(TAG, "25", "Z"), b""]
    out = []
    for b in blobs:
        t = bamwriter.pack_tag(TAG, 25, "C") if rng.random() < 0.75 else other[int(rng.integers(0, len(other)))]
        out.append(struct.pack("<i", len(b) - 4 + len(t)) + b[4:] + t)
    write_bam(dst, header, out, 200)
    return len(out)


def copy_dataset(src_dir, dst_dir, per_bam):
    """a golden dataset under dst_dir with every BAM made by per_bam(src bam, dst bam); the .bai files are left out"""
    return reblock.recut_dataset(src_dir, dst_dir, per_bam)
