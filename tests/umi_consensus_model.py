"""A plain-Python model of the pileup fold under both molecule rules (XCK_F_UMI_CONSENSUS, include/xck.h), and the
inputs the consensus tests share; no GPU, no HIP, never calls the library.  Batches, tables and filters are in the form
tests/join_tile_cases.py uses (batch dicts of numpy columns, (chrom, start1, end1, name) regions, (chrom, pos1, ref, alt, ref_hap,
alt_hap) SNPs, a dict of filters over JT.FILT); its read summary and SNP walk are used as they are.

  molecules()  per (SNP, cell, UMI) the reads that cover the SNP in fetch order, each with the nibble it shows there or -1 (gap, no
               sequence) - the read side, the same under both rules
  fold()       rule "first": the first read decides, a first read without a base silences the molecule (baf/fc/mcount.py:109-127);
               rule "consensus": plurality vote over the reads with a base, ties to the bucket seen earliest, N abstains unless alone,
               reads without a base abstain.  Then the tallies per SNP, the per-SNP filter, the fan-out to the regions and the haplotype
               algebra per (region, cell) as oracle/xck_oracle.c states them -> AD / DP / OTH, tallies, the five counters.
Used by tests/test_umi_consensus_model_host.py (the model against the pinned oracle) and tests/test_gpu_umi_consensus.py."""
import bisect
import functools
import os
from types import SimpleNamespace

import numpy as np

import join_tile_cases as JT
from join_tile_cases import M, D, N, _read_snps, _read_summary

NT16 = "=ACMGRSVTWYHKDBN"
NIB = {c: i for i, c in enumerate(NT16)}
COUNTERS = ("molecules", "multi_read", "discordant", "tied", "changed")
N_CELLS = 3
FILT = dict(JT.FILT)


def run_walk():
    """RUN_WALK of finish.hip: followers a run head walks itself; a longer run takes one block (k_first_long / k_consensus_long)."""
    with open(os.path.join(JT.CSRC, "finish.hip")) as fp:
        return JT._int(fp.read(), r"constexpr\s+long\s+long\s+RUN_WALK\s*=\s*(\d+)\s*;")


def bucket(nib):
    """A, C, G, T -> 0 .. 3, anything else (N, IUPAC, '=') -> 4: nib_bucket() / the reference's tcount order"""
    return {1: 0, 2: 1, 4: 2, 8: 3}.get(nib, 4)


# ----------------------------------------------------------------------------- the read side
def _nibble_at(d, i, r, p0):
    """allele_at(): the nibble read i of batch d shows at 0-based position p0, or -1 (gap, or beyond the stored sequence)"""
    rp, q = r.pos, 0
    for op, l in r.cig:
        if op in (M, JT.EQ, JT.X):
            if rp <= p0 < rp + l:
                qi = q + p0 - rp
                if (qi >> 1) >= r.sl:
                    return -1
                by = int(d["seq"][int(d["seq_off"][i]) + (qi >> 1)])
                return (by & 15) if (qi & 1) else (by >> 4)
            rp += l; q += l
        elif op in (JT.I, JT.S):
            q += l
        elif op in (D, N):
            rp += l
    return -1


def molecules(names, snps, batches, filt):
    """-> {(snp index, cell, umi): [(ordinal, nibble or -1), ...] in fetch order}, over the SNP entries in input order (a position listed
    twice is two SNPs); accepted (read, SNP) pairs"""
    f = dict(FILT); f.update(filt)
    by_contig = {}
    for k, s in enumerate(snps):
        if s[1] >= 1:
            by_contig.setdefault(names.index(s[0]), []).append((s[1] - 1, k))
    mols, pairs = {}, 0
    for d in batches:
        c = int(d["contig"])
        if c not in by_contig:
            continue
        ent = sorted(by_contig[c])
        p0 = sorted(set(p for p, _ in ent))
        ks = {p: [k for q, k in ent if q == p] for p in p0} if len(p0) != len(ent) else {p: [k] for p, k in ent}
        for i, r in enumerate(_read_summary(d, f)):
            if not r.ok:
                continue
            base, nobase, gaps = _read_snps(r, p0)
            hit = [(j, True) for j in base] + [(j, False) for j in nobase] + [(j, False) for a, b in gaps for j in range(a, b)]
            for j, has in hit:
                nib = _nibble_at(d, i, r, p0[j])
                assert (nib >= 0) == has, "the model's base lookup and join_tile_cases._read_snps disagree"
                for k in ks[p0[j]]:
                    mols.setdefault((k, r.cell, r.umi), []).append((int(d["ordinal_base"]) + i, nib))
                    pairs += 1
    for v in mols.values():
        v.sort()
    return mols, pairs


# ----------------------------------------------------------------------------- the two rules
def call(reads, rule):
    """reads [(ordinal, nibble or -1)] in fetch order -> (nibble or -1, flags of the five counters)"""
    shown = [(o, n) for o, n in reads if n >= 0]
    flags = [0] * 5
    if shown:
        c, first = [0] * 5, [None] * 5
        for o, n in shown:
            b = bucket(n)
            c[b] += 1
            if first[b] is None:
                first[b] = (o, n)
        voters = [b for b in range(4) if c[b]]
        if voters:
            top = max(c[b] for b in voters)
            tied = [b for b in voters if c[b] == top]
            win = min(tied, key=lambda b: first[b][0])
        else:
            tied, win = [], 4
        flags = [1, int(len(shown) >= 2), int(sum(1 for x in c if x) >= 2), int(len(tied) >= 2), int(win != bucket(shown[0][1]))]
        if rule == "consensus":
            return first[win][1], flags
    if rule == "consensus":
        return -1, flags
    assert rule == "first"
    return reads[0][1], flags


def fold(names, regions, snps, filt, mols, rule, cell_enabled=None, excl_pairs=None):
    """-> SimpleNamespace(ad, dp, oth: (row, col, val) int32 sorted by (row, col); tally: int64 [n_snps, 5] in input order; counters: dict;
    allele: {molecule: nibble} of the molecules that show one).  cell_enabled (bool per cell): the others' molecules are left out of
    the tallies and the matrices (xck_refold's mask), never of the counters, which belong to the finish."""
    f = dict(FILT); f.update(filt)
    allele, cnt = {}, [0] * 5
    for key, reads in mols.items():
        nib, flags = call(reads, rule)
        cnt = [a + b for a, b in zip(cnt, flags)]
        if nib >= 0:
            allele[key] = nib
    on = (lambda cell: True) if cell_enabled is None else (lambda cell: bool(cell_enabled[cell]))
    tally = np.zeros((len(snps), 5), dtype=np.int64)
    per_snp = {}
    for (k, cell, umi), nib in allele.items():
        if on(cell):
            tally[k, bucket(nib)] += 1
            per_snp.setdefault(k, []).append((cell, umi, nib))
    kept = []
    for k, s in enumerate(snps):
        t = tally[k]
        tot = int(t.sum())
        minor = min(int(t[bucket(NIB.get(s[2], 15))]), int(t[bucket(NIB.get(s[3], 15))]))
        kept.append(s[1] >= 1 and not (tot < f["min_count"]) and not (minor < tot * f["min_maf"]))
    excl = set(zip(excl_pairs[0], excl_pairs[1])) if excl_pairs is not None else set()
    out = {m: ([], [], []) for m in ("ad", "dp", "oth")}
    by_chrom = {}
    for k in per_snp:
        by_chrom.setdefault(snps[k][0], []).append((snps[k][1], k))
    for v in by_chrom.values():
        v.sort()
    for g, rg in enumerate(regions):
        bits = {}
        v = by_chrom.get(rg[0], [])
        for _, k in v[bisect.bisect_left(v, (rg[1], -1)):bisect.bisect_left(v, (rg[2] + 1, -1))]:
            s = snps[k]
            if not kept[k] or (g, k) in excl:
                continue
            for cell, umi, nib in per_snp.get(k, ()):
                ch, idx = NT16[nib], -1
                if ch == s[2]:
                    idx = s[4]
                if ch == s[3]:
                    idx = s[5]
                bits[(cell, umi)] = bits.get((cell, umi), 0) | (1 if idx == 0 else 2 if idx == 1 else 4)
        cells = {}
        for (cell, umi), b in bits.items():
            x = cells.setdefault(cell, [0, 0, 0, 0])
            x[0] += 1 if b & 1 else 0; x[1] += 1 if b & 2 else 0
            if b & 3:
                x[2] += 1
            elif b & 4:
                x[3] += 1
        for cell in sorted(cells):
            ref, alt, dp, oth = cells[cell]
            if ref + alt != dp:
                if f["no_dup_hap"]:
                    share = ref + alt - dp; ref -= share; alt -= share
                dp = ref + alt
            if dp + oth <= 0:
                continue
            for m, v in (("ad", alt), ("dp", dp), ("oth", oth)):
                if v > 0:
                    out[m][0].append(g); out[m][1].append(cell); out[m][2].append(v)
    res = {m: tuple(np.array(a, dtype=np.int32) for a in out[m]) for m in out}
    return SimpleNamespace(tally=tally, counters=dict(zip(COUNTERS, cnt)), allele=allele, **res)


def model(names, regions, snps, batches, filt, rule, cell_enabled=None, excl_pairs=None):
    mols, _ = molecules(names, snps, batches, filt)
    return fold(names, regions, snps, filt, mols, rule, cell_enabled, excl_pairs)


def snp_counts(snps, allele):
    """xck_snp_counts restated: per (SNP, cell) AD = molecules that show ALT, DP = REF or ALT (ALT wins when REF == ALT), OTH = the others"""
    acc = {}
    for (k, cell, umi), nib in allele.items():
        x = acc.setdefault((k, cell), [0, 0, 0])
        ch = NT16[nib]
        if ch == snps[k][3]:
            x[0] += 1; x[1] += 1
        elif ch == snps[k][2]:
            x[1] += 1
        else:
            x[2] += 1
    out = {}
    for j, m in enumerate(("ad", "dp", "oth")):
        ent = sorted((k, cell, v[j]) for (k, cell), v in acc.items() if v[j] > 0)
        out[m] = tuple(np.array([e[q] for e in ent], dtype=np.int32) for q in range(3))
    return out


def group_sum(coo, cell_group):
    """xck_group_counts restated: the columns of one (row, col, val) summed per group, -1 left out, sorted by (row, group)"""
    acc = {}
    for r, c, v in zip(*(a.tolist() for a in coo)):
        if cell_group[c] >= 0:
            acc[(r, cell_group[c])] = acc.get((r, cell_group[c]), 0) + v
    ent = sorted((r, g, v) for (r, g), v in acc.items() if v)
    return tuple(np.array([e[q] for e in ent], dtype=np.int32) for q in range(3))


def batch_dict(b, keep):
    """the numpy columns of a (capi.Batch, keepalive) pair as capi.make_batch / oracle.encode_bam build it -> batch dict"""
    cols = dict(zip(("pos", "flag", "mapq", "cell", "umi", "cig_off", "cigar", "seq_off", "seq"), keep))
    return dict(contig=int(b.contig), ordinal_base=int(b.ordinal_base), **cols)


# ----------------------------------------------------------------------------- crafted inputs
# 33 SNPs ten bases apart (a block of 32 SNPs is crossed), REF A on haplotype 0, ALT C on haplotype 1; one one-base region per SNP, one
# region over the first twenty and one over them all; 3 cells.  A read over SNP k is five aligned bases with the SNP under the middle one;
# a gap read is 2M 6N|D 2M with the SNP inside the gap.  Reads of one SNP start at one position, gap reads two bases earlier, and the
# batch is sorted by position (stable): the order a run lists its reads in is their fetch order.
N_SNPS, SNP0, STEP = 33, 1000, 10
NAMES = ["1"]
SNPS = [("1", SNP0 + STEP * k + 1, "A", "C", 0, 1) for k in range(N_SNPS)]
REGIONS = [("1", s[1], s[1], "s%d" % k) for k, s in enumerate(SNPS)] + [("1", SNP0, SNP0 + STEP * 20, "first20"), ("1", 1, SNP0 + STEP * N_SNPS, "all")]
REGIONS2 = [("1", SNP0 + STEP * 3 * g + 1, SNP0 + STEP * (3 * g + 2) + 1, "t%d" % g) for g in range(11)] + [("1", SNP0 + STEP * 30, SNP0 + STEP * 40, "tail")]


def _read(k, base, cell, umi):
    """base: a letter of NT16 shown at SNP k, "n" / "d": the SNP inside an N / D gap"""
    p0 = SNP0 + STEP * k
    if base in ("n", "d"):
        return dict(pos=p0 - 4, cig=[(M, 2), (N if base == "n" else D, 6), (M, 2)], seq="TTTT", cell=cell, umi=umi)
    return dict(pos=p0 - 2, cig=[(M, 5)], seq="TT" + base + "TT", cell=cell, umi=umi)


def build(reads, contig=0):
    """read dicts -> one batch dict (sorted by position, stable), min_len of the case's filter is 1"""
    reads = sorted(reads, key=lambda r: r["pos"])
    cw, cig_off, sq, seq_off = [], [0], [], [0]
    for r in reads:
        cw += [(l << 4) | op for op, l in r["cig"]]; cig_off.append(len(cw))
        nib = [NIB[c] for c in r["seq"]] + ([0] if len(r["seq"]) & 1 else [])
        sq += [(nib[j] << 4) | nib[j + 1] for j in range(0, len(nib), 2)]; seq_off.append(len(sq))
    n = len(reads)
    return dict(contig=contig, ordinal_base=0, pos=np.array([r["pos"] for r in reads], np.int32), flag=np.zeros(n, np.uint16),
                mapq=np.full(n, 60, np.uint8), cell=np.array([r["cell"] for r in reads], np.int32),
                umi=np.array([JT.UMI0 | r["umi"] for r in reads], np.uint64), cig_off=np.array(cig_off, np.uint32),
                cigar=np.array(cw + [0], np.uint32), seq_off=np.array(seq_off, np.uint32), seq=np.array(sq + [0], np.uint8))


def _runs(specs):
    """specs [(SNP, cell, string of read letters in fetch order)]: every run a molecule of its own"""
    out = []
    for u, (k, cell, letters) in enumerate(specs):
        out += [_read(k, ch, cell, u) for ch in letters]
    return out


def _mixed(length, place):
    """a run of `length` reads, (length - 1) // 2 of them A and the others C - C wins, by one read when the length is odd - with the
    A reads first, last, or ending at follower RUN_WALK (the last one a head lane reads)"""
    n_a = (length - 1) // 2
    end = {"first": n_a, "last": length, "boundary": min(length, run_walk() + 1)}[place]
    return "".join("A" if end - n_a <= j < end else "C" for j in range(length))


SHAPES = [
    (0, 0, "ACC"),       # the default answers A, the vote C: changed
    (1, 1, "AC"),        # a tie: the earlier read wins
    (2, 2, "TAACC"),     # a tie between A and C, the earliest read in neither: A, changed
    (3, 0, "NNA"),       # N abstains: A, changed
    (4, 1, "N"),         # N alone
    (5, 2, "M"),         # an IUPAC nibble alone: kept as it is, tallied under N
    (6, 0, "MNC"),       # ... and beside a voter
    (7, 1, "nC"),        # a gap read first: counted under consensus, silenced under the default
    (8, 2, "nn"),        # gap reads only
    (9, 0, "dC"),        # a D gap
    (10, 1, "ndCnA"),    # both gaps among the voters: a tie, C earlier
    (31, 2, "A"), (31, 2, "CA"), (31, 0, "CCA"),      # lengths 1, 2, 3 on both sides of the block boundary
    (32, 0, "C"), (32, 1, "AC"), (32, 2, "ACC"),
    (20, 0, "A"), (20, 0, "C"), (20, 1, "A"), (21, 0, "C"),   # neighbours that agree: one read per molecule
]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> SimpleNamespace(names, regions, snps, n_cells, batches, filt)"""
    W = run_walk()
    if name == "shapes":
        reads = _runs(SHAPES)
    elif name == "acc":
        reads = _runs([(0, 0, "ACC")])
    elif name == "single":                                       # every molecule one read (gap reads have molecules of their own)
        reads = _runs([(k % N_SNPS, k % 3, "ACGTNMnd"[k % 8]) for k in range(120)])
    elif name == "walk":                                         # run lengths around the head lane's walk
        reads = _runs([(3 * j + i, i, _mixed(W + d, place)) for j, d in enumerate((0, 1, 2)) for i, place in enumerate(("first", "last", "boundary"))])
    elif name == "long":                                         # one block per run: its stride of 256 at -1, 0, +1 and four times round
        reads = _runs([(j, j % 3, _mixed(n, "first")) for j, n in enumerate((255, 256, 257, 1025))] + [(12, 0, "ACC")])
    elif name == "deep":                                         # more reads in one (SNP, cell) than a work item of the partition sort holds
        reads = _runs([(5, 1, _mixed(2100, "last")), (6, 1, "ACC")])
    else:
        raise KeyError(name)
    return SimpleNamespace(name=name, names=NAMES, regions=REGIONS, snps=SNPS, n_cells=N_CELLS, batches=[build(reads)], filt={})


CASES = ("shapes", "acc", "single", "walk", "long", "deep")


# ----------------------------------------------------------------------------- fuzz inputs
# (chosen on the CPU: the seeds of 0 .. 239 whose case is quick and, with one UMI code, meets the conditions of tests/test_umi_consensus_model_host.py;
#  four of them leave non-empty matrices under their filters, one uses 128-bit keys)
FUZZ_SEEDS = (8, 26, 91, 148, 150, 195)
FUZZ_POOL = 1


@functools.lru_cache(maxsize=None)
def fuzz_case(seed):
    """tests/fuzz_cases.make_case(seed) with its UMIs re-keyed to FUZZ_POOL codes, so that molecules are deep
    -> SimpleNamespace(names, regions, snps, n_cells, batches (dicts), filt, flags)"""
    import fuzz_cases
    names, regions, snps, n_cells, batches, fc, baf, flags = fuzz_cases.make_case(seed, many_cells=False, long=False)
    out = []
    for b, keep in batches:
        d = batch_dict(b, [a.copy() for a in keep])
        u = d["umi"]
        some = u != np.uint64(0xFFFFFFFFFFFFFFFF)
        u[some] = np.uint64(1 << 8) | (u[some] % np.uint64(FUZZ_POOL))
        out.append(d)
    return SimpleNamespace(name="fuzz%d" % seed, names=names, regions=regions, snps=snps, n_cells=n_cells, batches=out, filt=baf, flags=flags)
