"""What the device-decode tests share (tests/test_device_decode_cases_host.py on the CPU, tests/test_gpu_device_decode_golden.py and
tests/test_gpu_device_decode_crafted.py on the GPU): the block schedules the golden BAMs are re-cut by (tests/reblock.py), the class a
case's run is expected to fall into, predicted from the records as oracle/pybam.py reads them, and the crafted BAMs with their tables.

Nothing here calls the product decoder: the numbers (64 blocks per device chunk, 64 records per k_parse round, DP_MAX_RUNS contig runs
per block, the 18-byte barcode slots, n_max = (umi_bits - 2) // 2 bases in a 2-bit UMI code) are conditions taken from csrc/bam.cpp,
csrc/parse_dev.h and encode_key_direct, and the CPU test checks that the files meet them with pybam and the oracle alone."""
import json
import os
import struct

import numpy as np

import oracle as O
import pybam
import reblock
import util
from xcltk_amd import capi
from xcltk_amd.synth import bamwriter

MIN_BLOCKS = 64                 # csrc/bam.cpp schedule_chunk: a chunk goes to the device with at least this many BGZF blocks
HEADROOM = 80                   # what the intended chunks of the re-cut files hold at least
MAX_RUNS = 4                    # csrc/parse_dev.h DP_MAX_RUNS: contig runs of one block the walk's summary holds
BC_SLOT = 18                    # DecodeCfg::BcSlot::key: the device parse is on only if every barcode fits
WHOLE = 1 << 30                 # XCK_CHUNK_BYTES that keeps a small file in one chunk

MIXED = (400, 1500, 3000, 3000, 20000)
# name -> (payload targets, share_header, empty_every)
SCHEDULES = {
    "mixed_shared": (MIXED, True, 0),                                      # header's tail + first records in one block: first_skip > 0
    "mixed_alone": (MIXED, False, 0),                                      # the header's block ends first
    "single": ((1,), True, 3),                                             # one record per block, an empty block after every third
    "many": ((250,) * 7 + (40000,), False, 0),                             # most blocks hold one record, every eighth 170 and more: three k_parse rounds
    "ten": ((400, 900, 1800), False, 0),                                   # at most about 10 records per block (the per-cell BAMs)
    "single_empty": ((1,), True, 1),                                       # one record per block, every other block empty (41 records -> 64 blocks and more)
}
# dataset -> (schedule, XCK_CHUNK_BYTES) of the golden cases
DATASET_PLAN = {"c1": ("mixed_shared", 600000), "dense": ("mixed_alone", 600000), "multibam": ("mixed_shared", WHOLE),
                "phasing": ("mixed_alone", WHOLE), "well": ("ten", WHOLE), "special": ("single_empty", WHOLE)}
# the block shapes: the cases, the schedules and their XCK_CHUNK_BYTES.  c1 and dense hold a UMI with N in every 400 records or so
# (10x-style data), phasing holds none: with one record per block the chunks are short enough for most of them to be free of such a UMI
SHAPE_CASES = ("c1_basefc_default", "dense_baf_allreg_dup", "phasing_baf_allreg")
SHAPES = ("mixed_shared", "mixed_alone", "single", "many")


def shape_chunk_bytes(dataset, schedule):
    return 50000 if schedule == "single" else WHOLE if dataset == "phasing" else 700000 if schedule == "many" else 600000


def recut(schedule, seed=11):
    """-> the function reblock.recut_dataset calls per BAM"""
    sizes, share, empty = SCHEDULES[schedule]
    rng = np.random.default_rng(seed)
    return lambda src, dst: reblock.reblock_bam(src, dst, sizes, rng, share, empty)


def dataset_of(name):
    with open(os.path.join(util.GOLDEN, "cases", name, "case.json")) as fp:
        return json.load(fp)["dataset"]


def recut_case(name, tmp, schedule=None, sub="ds"):
    """Golden case `name` on a copy of its dataset under tmp whose BAMs are re-cut.  -> (case, dataset dir, out dir, expected dir,
    XCK_CHUNK_BYTES, {bam: (records, blocks, most records in a block)})"""
    dataset = dataset_of(name)
    plan = DATASET_PLAN[dataset] if schedule is None else (schedule, shape_chunk_bytes(dataset, schedule))
    ddir = os.path.join(str(tmp), sub + "_" + dataset + "_" + plan[0])
    if os.path.isdir(ddir):                                                 # (a second case of the same test on the same files)
        with open(os.path.join(ddir, "recut.json")) as fp:
            info = json.load(fp)
    else:
        info = reblock.recut_dataset(os.path.join(util.GOLDEN, "datasets", dataset), ddir, recut(plan[0]))
        with open(os.path.join(ddir, "recut.json"), "w") as fp:
            json.dump(info, fp)
    case, ddir, odir, exp = util.load_case(name, tmp, ddir)
    return case, ddir, odir, exp, plan[1], info


# ----------------------------------------------------------------------------- the class of a run
def contig_runs(recs, t2c):
    """number of runs of equal engine contig (-1: not wanted) in a block's [(tid, pos)]: what k_walk counts against DP_MAX_RUNS"""
    n, cur = 0, None
    for tid, _ in recs:
        c = t2c[tid] if 0 <= tid < len(t2c) else -1
        if c != cur:
            n, cur = n + 1, c
    return n


def _uncodable(r, umi_tag, n_max):
    """does the device leave this record's UMI to the host?  (numeric type, a byte outside ACGT, more than n_max bases; an absent tag
    and an empty value give XCK_UMI_NONE without the intern table)"""
    if not r.has_tag(umi_tag):
        return False
    typ, val = r.tags[umi_tag]
    return typ not in "ZAH" or len(val) > n_max or any(c not in "ACGT" for c in val)


def predict_run(bam_fns, region_fn, snp_fn, barcode_fn, cell_tag, umi_tag, chunk_bytes, n_max=None):
    """What a run over these files with XCK_GPU_INFLATE=100 and XCK_CHUNK_BYTES=chunk_bytes is expected to report, from pybam's records
    and the files' blocks alone.  -> dict(cls, device_chunks, parse_chunks, fallbacks, exact):
    cls "inflate-only" - no UMI tag (the key is the read name, interned on the host), or a barcode that does not fit a slot: no device parse;
        "odd"          - some record on a wanted contig in a device chunk has a UMI the device cannot code, or some block holds more than
                         MAX_RUNS contig runs: that chunk falls back to the host path;
        "clean"        - otherwise.
    device_chunks: chunks of MIN_BLOCKS blocks and more; fallbacks / parse_chunks: those of them with / without such a record or block;
    exact: no four fallbacks follow in a row, after which the reader would stop asking and the two counts depend on what was in flight."""
    none = lambda t: not t or t.upper() == "NONE"
    barcodes = []
    if barcode_fn and not none(cell_tag):
        with open(barcode_fn) as fp:
            barcodes = [x.strip() for x in fp]
    parse = not none(umi_tag) and all(len(b.encode()) <= BC_SLOT for b in barcodes)
    regions = O.load_regions(region_fn)
    snps = O.load_snps(snp_fn) if snp_fn else []
    names = O.contig_table(regions, snps)
    ub = O.default_umi_bits(capi.XCK_MODE_BAF if snps else capi.XCK_MODE_BASEFC, len(regions), len(snps), max(len(barcodes), len(bam_fns)))
    if n_max is None:                                                       # (the 64-bit key layout, unless the caller knows the handle's)
        n_max = (ub - 2) // 2
    out = dict(cls="clean" if parse else "inflate-only", device_chunks=0, parse_chunks=0, fallbacks=0, exact=True)
    for fn in bam_fns:
        refs, recs = pybam.read_bam(fn)
        t2c = O.resolve_contigs([n for n, _ in refs], names)
        blocks = reblock.block_records(fn)[2]
        at, i, row = 0, 0, 0                                                # (the reader's count of fallbacks in a row starts anew with every file)
        for n in reblock.plan_chunks(fn, chunk_bytes):
            n_rec = sum(len(b) for b in blocks[at:at + n])
            if n >= MIN_BLOCKS:
                out["device_chunks"] += 1
                bad = parse and (any(0 <= r.tid < len(t2c) and t2c[r.tid] >= 0 and _uncodable(r, umi_tag, n_max) for r in recs[i:i + n_rec]) or
                                 any(contig_runs(b, t2c) > MAX_RUNS for b in blocks[at:at + n]))
                if parse:
                    out["fallbacks" if bad else "parse_chunks"] += 1
                row = row + 1 if bad else 0
                if bad:
                    out["cls"] = "odd"
                if row >= 4:
                    out["exact"] = False
            at, i = at + n, i + n_rec
    return out


def predict_case(case, chunk_bytes, fused_snp_fn=None):
    p = util.oracle_params(case)
    snp_fn = fused_snp_fn or (p["snp_fn"] if p["mode"] == capi.XCK_MODE_BAF else None)
    return predict_run(p["bam_fns"], p["region_fn"], snp_fn, p["barcode_fn"], p["cell_tag"], p["umi_tag"], chunk_bytes)


def sum_stats(seen):
    keys = ("gpu_inflate_chunks", "gpu_inflate_blocks", "gpu_parse_chunks", "gpu_parse_fallbacks")
    return {k: sum(int(s[k]) for s in seen) for k in keys}


def assert_stats(pred, st, n_engines=1):
    """the decode stats of a run against what predict_run said: the class's assertion, and the counts themselves where they are exact"""
    cls = pred["cls"]
    assert st["gpu_inflate_chunks"] > 0, st
    if cls == "clean":
        assert st["gpu_parse_chunks"] > 0 and st["gpu_parse_fallbacks"] == 0, st
    elif cls == "odd":
        assert st["gpu_parse_chunks"] + st["gpu_parse_fallbacks"] > 0, st
    else:
        assert cls == "inflate-only" and st["gpu_parse_chunks"] == 0 and st["gpu_parse_fallbacks"] == 0, st
    if pred["exact"] and n_engines == 1:
        assert (st["gpu_inflate_chunks"], st["gpu_parse_chunks"], st["gpu_parse_fallbacks"]) == (pred["device_chunks"], pred["parse_chunks"], pred["fallbacks"]), (st, pred)


# ----------------------------------------------------------------------------- crafted records
# Genome: four references, chr1 chr2 chrU chr3; the tables know 1, 2 and 3.  Every 20 kb slot of a known reference has a filler region
# [S + 1, S + 600] with three SNPs and, for a slot that hosts an edge record, an edge region [S + 10001, S + 14000] with one SNP on the
# record's 11th base.  An edge record has a barcode of its own, so its fate is one entry of the matrices: (its region, its cell).
REFS = [("chr1", 2000000), ("chr2", 2000000), ("chrU", 2000000), ("chr3", 2000000)]
SLOTS = {0: 60, 1: 40, 3: 20}                                              # tid -> slots
SLOT = 20000
N_FILLER_CELLS = 40
FILLERS_PER_SLOT = 34
N_UNKNOWN = 25                                                             # records on chrU: all of them sit in the "alternating" block
ALT_EACH = 25                                                              # ... between the last 25 of chr2 and the first 25 of chr3
N_UNMAPPED = 100
BLOCK_RECORDS = 8                                                          # records per block elsewhere (about 1.5 kB)
INDEXED_CHUNK_BYTES = 300000                                               # ... of the BamWriter re-cut of c1 (blocks of 3,000 bytes)
CHUNK_BYTES = 130000                                                       # XCK_CHUNK_BYTES of the crafted runs: about 85 such blocks

_B = "ACGT"


def _bases(rng, n):
    return "".join(_B[k] for k in rng.integers(0, 4, n))


def _long_cigar():
    """200 operations over 1,000 query bases: 5S, 33 x (10M 1I 10M 2D 9M 50N), 5M.  -> (cigar, query offset and reference offset of
    the first base of the 31st unit's last M run)"""
    ops, q, r, at = [(4, 5)], 5, 0, None
    for u in range(33):
        for op, l in ((0, 10), (1, 1), (0, 10), (2, 2), (0, 9), (3, 50)):
            if u == 30 and (op, l) == (0, 9):
                at = (q, r)
            if op in (0, 1):
                q += l
            if op in (0, 2, 3):
                r += l
            ops.append((op, l))
    ops.append((0, 5))
    assert q + 5 == 1000 and len(ops) == 200
    return ops, at


def craft(outdir, n_max, odd):
    """Write <outdir>/{regions.tsv, snps.tsv, barcodes.tsv, crafted.bam} (n_max: the longest UMI the handle codes in 2 bits; odd: with
    the records the device cannot code).  -> dict(bam, region_fn, snp_fn, barcode_fn, edges, odd_keys): edges = [dict(name, row,
    barcode, hit, val)] - the entry (row, cell of barcode) must be non-zero (hit; val: its count where the test names one) or absent
    (barcode None: the whole row is empty); odd_keys = the (tid, pos) of the records that send a chunk down the host path."""
    os.makedirs(outdir, exist_ok=True)
    rng = np.random.default_rng(2024)
    cells = sorted({_bases(rng, 16) + "-1" for _ in range(N_FILLER_CELLS + 8)})[:N_FILLER_CELLS]
    regions, snps, recs, edges, odd_keys, extra_bc = [], [], [], [], [], []
    long_ops, (long_q, long_r) = _long_cigar()

    # ---- the edge records: (name, spec) in the order they take their slots
    def E(name, **kw):
        return dict(name=name, **kw)
    clean = [
        E("cb_type_A", cb=("Q", "A")),
        E("cb_type_H", cb=("1AE301", "H")),
        E("arrays_and_numbers_first", front=[("XB", ("c", [1, -2, 3]), "B"), ("XS", ("S", [1, 2, 65535, 4, 5]), "B"), ("XF", ("f", [1.5, -2.5]), "B"),
                                             ("Xc", -3, "c"), ("XC", 200, "C"), ("Xs", -300, "s"), ("XT", 60000, "S"), ("Xi", -70000, "i"),
                                             ("XI", 4000000000, "I"), ("Xf", 0.25, "f")]),
        E("tags_twice", twice=True, val=1),
        E("cb_absent", cb=None, hit=False),
        E("cb_unlisted", cb=("TTTTGGGGCCCCAAAA-1", "Z"), listed=False, hit=False),
        E("cb_long_unlisted", cb=("ACGTACGTACGTACGTACGTAC-1", "Z"), listed=False, hit=False),
        E("ub_absent", ub=None, hit=False),
        E("ub_empty", ub=("", "Z"), hit=False),
        E("ub_type_A", ub=("G", "A")),
        E("umi_len_1", ub=("C", "Z")),
        E("umi_len_nmax_minus_1", ub=("ACGT" * 16, "Z"), ulen=n_max - 1),
        E("umi_len_nmax", ub=("TGCA" * 16, "Z"), ulen=n_max),
        E("no_cigar", cigar=[], hit=False),                                 # no aligned base: below min_len, the reference skips it
        E("l_seq_0", seq="", baf_hit=False),                                # counted by basefc (CIGAR only); no base for the pileup
        E("l_seq_odd", cigar=[(0, 61)], seq_len=61, snp_at=60),            # the SNP reads the last, half-filled sequence byte
        E("long_cigar", cigar=long_ops, seq_len=1000, snp_at=long_q, snp_ref=long_r),
        E("empty_name", qname=""),
        E("name_254", qname="n" * 254),
    ]
    odd_recs = [
        E("umi_len_nmax_plus_1", ub=("GATC" * 16, "Z"), ulen=n_max + 1),
        E("umi_with_N", ub=("ACGTNACGTA", "Z")),
        E("umi_lowercase", ub=("acgtacgtac", "Z")),
        E("ub_numeric_0", ub=(0, "i"), hit=False),
        E("ub_numeric_c", ub=(-7, "c")),
        E("ub_numeric_S", ub=(513, "S")),
        E("ub_numeric_i", ub=(123456, "i")),
        E("ub_numeric_f", ub=(1.5, "f")),
    ]
    # slots of the edge records: the clean ones spread over the three references; the odd ones in two narrow ranges of chr1 that
    # land in two chunks with clean chunks before, between and after them (the CPU test checks where they land)
    clean_slots = [(0, 1 + 3 * k) for k in range(12)] + [(1, 2 + 4 * k) for k in range(5)] + [(3, 2 + 5 * k) for k in range(3)]
    odd_slots = [(0, 5), (0, 6), (0, 8), (0, 9), (0, 45), (0, 47), (0, 48), (0, 50)]
    placed = dict(zip([e["name"] for e in clean], clean_slots))
    if odd:
        placed.update(zip([e["name"] for e in odd_recs], odd_slots))
    by_slot = {v: k for k, v in placed.items()}
    assert len(by_slot) == len(placed)
    specs = {e["name"]: e for e in clean + odd_recs}

    def edge_record(tid, S, e, row):
        bc = "E%02d%s-1" % (len(extra_bc), _bases(rng, 12))
        cb = e.get("cb", (bc, "Z"))
        if cb is not None and e.get("listed", True):
            extra_bc.append(cb[0])
        ub = e.get("ub", ("ACGTTGCAAC", "Z"))
        if ub is not None and "ulen" in e:
            ub = (ub[0][:e["ulen"]], "Z")
            assert len(ub[0]) == e["ulen"]
        pos = S + 10100
        cigar = e.get("cigar", [(0, 60)])
        seq = e["seq"] if "seq" in e else _bases(rng, e.get("seq_len", 60))
        snp_at, snp_ref = e.get("snp_at", 10), e.get("snp_ref", e.get("snp_at", 10))
        if seq:
            seq = seq[:snp_at] + "C" + seq[snp_at + 1:]                     # the read shows the ALT base at its SNP
        tags = list(e.get("front", []))
        if e.get("twice"):
            other = "E%02d%s-1" % (len(extra_bc), _bases(rng, 12))
            extra_bc.append(other)
            tags += [("CB", cb[0], "Z"), ("UB", "ACGTTGCAAC", "Z"), ("CB", other, "Z"), ("UB", "TTTTTTTTTT", "Z")]
            edges.append(dict(name="tags_twice_second_barcode", row=row, barcode=other, hit=False, baf_hit=False, val=None))
        else:
            tags += ([("CB",) + cb] if cb is not None else []) + ([("UB",) + ub] if ub is not None else [])
        tags.append(("NH", 1, "C"))
        blobs = [bamwriter.pack_record(tid, pos, e.get("qname", "edge_" + e["name"]), 0, 60, cigar, seq, tags)[0]]
        if e.get("twice"):                                                  # a second read of the pair with the FIRST of the two UMIs: one molecule
            s2 = _bases(rng, 60)
            blobs.append(bamwriter.pack_record(tid, pos + 5, "edge_partner", 0, 60, [(0, 60)], s2[:5] + "C" + s2[6:], [("CB", cb[0]), ("UB", "ACGTTGCAAC")])[0])
        regions.append((REFS[tid][0][3:], S + 10001, S + 14000, "edge_" + e["name"]))
        snps.append((REFS[tid][0][3:], pos + snp_ref + 1, "A", "C", 0, 1))
        hit = e.get("hit", True)
        edges.append(dict(name=e["name"], row=row, barcode=cb[0] if cb is not None and e.get("listed", True) else None, hit=hit,
                          baf_hit=e.get("baf_hit", hit), val=e.get("val")))
        if any(e is x for x in odd_recs):
            odd_keys.append((tid, pos))
        return blobs

    per_tid = {}
    for tid in (0, 1, 3):
        out = []
        for j in range(SLOTS[tid]):
            S = SLOT * j
            row = len(regions)
            regions.append((REFS[tid][0][3:], S + 1, S + 600, "g%d_%03d" % (tid, j)))
            for k, d in enumerate((100, 300, 500)):
                snps.append((REFS[tid][0][3:], S + d, _B[k], _B[(k + 1) % 4], k & 1, 1 - (k & 1)))
            for p in np.sort(rng.integers(S, S + 520, FILLERS_PER_SLOT)).tolist():
                tags = [("CB", cells[int(rng.integers(0, len(cells)))]), ("UB", _bases(rng, 10)), ("NH", 1, "C")]
                out.append(bamwriter.pack_record(tid, int(p), "r%d_%d_%d" % (tid, j, len(out)), 0, 60, [(0, 60)], _bases(rng, 60), tags)[0])
            if (tid, j) in by_slot:
                out += edge_record(tid, S, specs[by_slot[(tid, j)]], len(regions))
        per_tid[tid] = out
    unknown = [bamwriter.pack_record(2, 1000 + 50 * k, "u%d" % k, 0, 60, [(0, 60)], _bases(rng, 60),
                                     [("CB", cells[k % len(cells)]), ("UB", _bases(rng, 10))])[0] for k in range(N_UNKNOWN)]
    unmapped = [bamwriter.pack_record(-1, -1, "x%d" % k, 4, 0, [], _bases(rng, 60), [("CB", cells[k % len(cells)]), ("UB", _bases(rng, 10))])[0]
                for k in range(N_UNMAPPED)]

    # ---- blocks: BLOCK_RECORDS records each; one block holds the end of chr2, all of chrU and the start of chr3
    blocks = []

    def cut(rs):
        for k in range(0, len(rs), BLOCK_RECORDS):
            blocks.append(rs[k:k + BLOCK_RECORDS])
    cut(per_tid[0] + per_tid[1][:-ALT_EACH])                                # (8 does not divide chr1's count: a block holds both references)
    blocks.append(per_tid[1][-ALT_EACH:] + unknown + per_tid[3][:ALT_EACH])
    cut(per_tid[3][ALT_EACH:] + unmapped)
    ht = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
    hdr = b"BAM\x01" + struct.pack("<i", len(ht)) + ht.encode() + struct.pack("<i", len(REFS))
    for n, l in REFS:
        hdr += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l)
    bam = os.path.join(outdir, "crafted.bam")
    with open(bam, "wb") as fp:
        fp.write(bamwriter.bgzf_block(hdr) + b"".join(bamwriter.bgzf_block(b"".join(b)) for b in blocks) + bamwriter.BGZF_EOF)
    out = dict(bam=bam, region_fn=os.path.join(outdir, "regions.tsv"), snp_fn=os.path.join(outdir, "snps.tsv"),
               barcode_fn=os.path.join(outdir, "barcodes.tsv"), edges=edges, odd_keys=odd_keys, n_records=sum(len(b) for b in blocks))
    with open(out["region_fn"], "w") as fp:
        fp.write("".join("chr%s\t%d\t%d\t%s\n" % r for r in regions))
    with open(out["snp_fn"], "w") as fp:
        fp.write("chrom\tpos\tref\talt\tref_hap\talt_hap\n" + "".join("chr%s\t%d\t%s\t%s\t%d\t%d\n" % s for s in snps))
    with open(out["barcode_fn"], "w") as fp:
        fp.write("".join(b + "\n" for b in cells + extra_bc))
    return out


def crafted_tables(c):
    """-> (contig names, regions, snps, sorted barcodes) of a crafted file, as the oracle's loaders read them"""
    regions, snps = O.load_regions(c["region_fn"]), O.load_snps(c["snp_fn"])
    with open(c["barcode_fn"]) as fp:
        barcodes = sorted(x.strip() for x in fp)
    return O.contig_table(regions, snps), regions, snps, barcodes


def crafted_expected(c):
    """the oracle's matrices for a crafted file: basefc and the pileup, each by O.run_files -> {"count", "ad", "dp", "oth"}"""
    fc = O.run_files(capi.XCK_MODE_BASEFC, [c["bam"]], c["region_fn"], barcode_fn=c["barcode_fn"])
    baf = O.run_files(capi.XCK_MODE_BAF, [c["bam"]], c["region_fn"], barcode_fn=c["barcode_fn"], snp_fn=c["snp_fn"])
    return dict(count=fc["count"], ad=baf["ad"], dp=baf["dp"], oth=baf["oth"])


def check_crafted_conditions(c, exp):
    """the conditions of the crafted files, on the oracle's output alone"""
    _, _, _, barcodes = crafted_tables(c)
    cell = {b: i for i, b in enumerate(barcodes)}
    assert len(exp["count"][0]) > 1000

    def at(m, row, col):
        r, cc, v = exp[m]
        k = np.flatnonzero((r == row) & (cc == col))
        return int(v[k[0]]) if len(k) else 0
    for e in c["edges"]:
        if e["barcode"] is None:                                            # no listed cell: the record's own region stays empty
            assert not (exp["count"][0] == e["row"]).any() and not (exp["dp"][0] == e["row"]).any(), e["name"]
            continue
        n, d = at("count", e["row"], cell[e["barcode"]]), at("dp", e["row"], cell[e["barcode"]])
        assert (n > 0) == e["hit"], (e["name"], n)
        assert (d > 0) == e["baf_hit"], (e["name"], d)
        if e["baf_hit"]:
            assert at("ad", e["row"], cell[e["barcode"]]) == d, e["name"]   # the record shows ALT at its SNP
        if e["val"] is not None:
            assert n == e["val"] and d == e["val"], (e["name"], n, d)
