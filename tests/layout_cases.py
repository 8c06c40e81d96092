"""Case builders with a known answer for the key-layout tests (tests/test_layouts_host.py, tests/test_gpu_layouts.py); no GPU.

Every count travels as a packed key row | cell | umi whose field widths follow from the table sizes alone (key_layout() in
xcltk_amd/csrc/xck_internal.h, restated in expected_layout() below).  targeted_case() builds a table of a requested size
arithmetically and a handful of reads whose (row, cell, UMI code) sit at the edges of those fields - first and last row and cell,
the values around the top bit of each field, the widest 2-bit and interned UMI codes of the layout - so that a wrong mask or shift
anywhere between the join and the matrices moves a count to another entry.  The answer is known by construction."""
import itertools
from types import SimpleNamespace

import numpy as np

from xcltk_amd import capi

XCK_UMI_NONE = capi.XCK_UMI_NONE
READ_LEN = 91
SNP_OFF = 50                      # 1-based offset of a region's SNP inside the region
REF, ALT, THIRD = "A", "C", "G"   # every SNP of a targeted table; THIRD is what an "other" read shows
NIB = {"A": 1, "C": 2, "G": 4, "T": 8}

# the grid of tests/test_gpu_layouts.py section 3: (n_regions | n_snps, n_cells)
GRID = [(3, 2), (3, 2048), (3, 2049), (3, 16384), (3, 16385), (3, 65536), (3, 65537), (63, 1 << 30), (255, 256), (65535, 65536),
        (65536, 65536), (262143, 1 << 20), (262144, 1 << 20), (262143, (1 << 20) + 1)]


def bits_for_count(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def expected_layout(n_regions, n_cells, n_snps=0):
    """-> (key_bits, umi_bits, cbits, rbits) by the documented rule: cbits = bits_for_count(n_cells), rbits = bits_for_count(max(n_regions,
    n_snps) + 1) (the SNPs count for the BAF pipeline only; the cases here have n_snps in (0, n_regions)), the UMI field gets the rest
    of 64 bits, and fewer than 26 bits for it mean 128-bit keys with a 64-bit UMI field."""
    cbits = bits_for_count(max(n_cells, 2))
    rbits = bits_for_count(max(n_regions, n_snps, 2) + 1)
    ub = 64 - rbits - cbits
    return (128, 64, cbits, rbits) if ub < 26 else (64, ub, cbits, rbits)


def intern_id_limit(umi_bits):
    """Number of interned ids a UMI field of this width holds (bam_records.cpp intern_id_limit): the top bit marks an interned code and the all-ones
    code is kept free, for XCK_UMI_NONE at 64 bits and for the folds' empty word below."""
    return (1 << 63) - 1 if umi_bits >= 64 else (1 << (umi_bits - 1)) - 1


def longest_direct(umi_bits):
    """Longest UMI the decoder codes with 2 bits per base: 2 L + 1 <= umi_bits - 1 (bam_records.cpp encode_key_direct)."""
    return (umi_bits - 2) // 2


def umi_codes(umi_bits, kinds):
    """name -> code, exactly as the decoder would produce them for this UMI width."""
    L = longest_direct(umi_bits)
    top = 1 << (umi_bits - 1)
    every = dict(direct_a=1 << (2 * L),                       # AAA...A of the longest direct length: only the length bit
                 direct_t=(1 << (2 * L + 1)) - 1,             # TTT...T: all ones below and including the length bit
                 mer12_t=(1 << 25) - 1,                       # TTTTTTTTTTTT: the 12-mer of droplet data (fits every 64-bit layout)
                 mer4=(1 << 8) | 0x1B,                        # ACGT
                 intern0=top, intern_top=top | (intern_id_limit(umi_bits) - 1),
                 none=XCK_UMI_NONE)
    return {k: every[k] for k in kinds}


ALL_UMIS = ("direct_a", "direct_t", "mer4", "intern0", "intern_top", "none")


def make_table(n_regions, stride=1000, width=1000, with_snps=False, base=0):
    """Region i = [base + 1 + stride * i, base + stride * i + width] on contig "1", optionally one SNP per region at offset SNP_OFF (REF / ALT,
    haplotypes alternating).  Built column-wise: 10^6 rows take well under a second."""
    i = np.arange(n_regions, dtype=np.int64)
    assert base + stride * (n_regions - 1) + width <= 2 ** 31 - 1 and width >= READ_LEN + 4 and SNP_OFF + 4 <= width
    start = (base + 1 + stride * i).tolist(); end = (base + stride * i + width).tolist()
    regions = list(zip(itertools.repeat("1"), start, end, itertools.repeat("r")))
    snps = []
    if with_snps:
        rh = (i & 1).tolist()
        snps = list(zip(itertools.repeat("1"), (base + stride * i + SNP_OFF).tolist(), itertools.repeat(REF), itertools.repeat(ALT),
                        rh, (1 - (i & 1)).tolist()))
    return ["1"], regions, snps


def edge_values(n, bits):
    """{0, 1, 2^(bits-1) - 1, 2^(bits-1), n - 2, n - 1} within [0, n): the top bit of the field both clear and set."""
    half = 1 << (bits - 1)
    return sorted({v for v in (0, 1, half - 1, half, n - 2, n - 1) if 0 <= v < n})


def reads_from_triples(triples, stride=1000, base=0, ordinal_base=0):
    """One 91M read per copy of a (row, cell, umi code) triple, wholly inside region `row` and over its SNP.  Triple t appears 1 + t % 4
    times (copy j starts j bases into the region) and shows REF, ALT or THIRD at the SNP by t % 3, the same base in every copy.
    -> batch dict (reads sorted by position), show (base per triple)."""
    t = np.arange(len(triples))
    copies = 1 + t % 4
    rep = np.repeat(t, copies)
    j = np.arange(len(rep)) - np.repeat(np.cumsum(copies) - copies, copies)
    row = np.array([x[0] for x in triples], np.int64)[rep]
    pos = base + stride * row + j                                  # 0-based; the SNP is at 0-based base + stride * row + SNP_OFF - 1
    assert int(j.max()) < SNP_OFF <= READ_LEN
    show = [(REF, ALT, THIRD)[x % 3] for x in t.tolist()]
    nib = np.full((len(rep), READ_LEN + 1), NIB[REF], np.uint8); nib[:, READ_LEN] = 0
    nib[np.arange(len(rep)), SNP_OFF - 1 - j] = np.array([NIB[b] for b in show], np.uint8)[rep]
    seq = ((nib[:, 0::2] << 4) | nib[:, 1::2]).astype(np.uint8)
    order = np.argsort(pos, kind="stable")
    n, nb = len(rep), seq.shape[1]
    d = dict(contig=0, ordinal_base=ordinal_base, pos=pos[order].astype(np.int32), flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8),
             cell=np.array([x[1] for x in triples], np.int32)[rep][order], umi=np.array([x[2] for x in triples], np.uint64)[rep][order],
             cig_off=np.arange(n + 1, dtype=np.uint32), cigar=np.full(n, (READ_LEN << 4) | 0, np.uint32),
             seq_off=(np.arange(n + 1) * nb).astype(np.uint32), seq=seq[order].reshape(-1))
    return d, show


def _coo(counts):
    """{(row, cell): count} -> (row, col, val) int32 arrays sorted by (row, col), zero counts left out."""
    items = sorted((k, v) for k, v in counts.items() if v > 0)
    return tuple(np.array([f(x) for x in items], np.int32) for f in (lambda x: x[0][0], lambda x: x[0][1], lambda x: x[1]))


def answers(triples, show, snps):
    """The matrices by construction.  basefc: distinct UMI codes per (row, cell), XCK_UMI_NONE counting nothing.  BAF (one SNP per region,
    every copy of a triple showing the same base, so one class per molecule and no molecule on both haplotypes): DP = molecules showing
    REF or ALT, AD = those of them whose base is on haplotype 1, OTH = molecules showing THIRD."""
    seen = set()
    count, ad, dp, oth = {}, {}, {}, {}
    for (row, cell, umi), b in zip(triples, show):
        if umi == XCK_UMI_NONE or (row, cell, umi) in seen:
            continue
        seen.add((row, cell, umi))
        k = (row, cell)
        count[k] = count.get(k, 0) + 1
        if snps:
            if b == THIRD:
                oth[k] = oth.get(k, 0) + 1
            else:
                dp[k] = dp.get(k, 0) + 1
                if snps[row][4 if b == REF else 5] == 1:
                    ad[k] = ad.get(k, 0) + 1
    return {"count": _coo(count), "ad": _coo(ad), "dp": _coo(dp), "oth": _coo(oth)}


def targeted_case(n_regions, n_cells, n_snps=0, umi_kinds=ALL_UMIS, stride=1000, width=1000, base=0, ordinal_base=0):
    """Table of n_regions regions (n_snps = 0, or n_regions for one SNP per region) and the reads of the cross product
    rows x cells x UMI codes at the edges of the layout's fields.  -> namespace: names, regions, snps, n_cells, d (batch dict), triples,
    layout (key_bits, umi_bits, cbits, rbits - computed here, never read from a handle), codes, expected (matrices by construction)."""
    assert n_snps in (0, n_regions)
    layout = expected_layout(n_regions, n_cells, n_snps)
    key_bits, umi_bits, cbits, rbits = layout
    names, regions, snps = make_table(n_regions, stride, width, n_snps > 0, base)
    codes = umi_codes(umi_bits, umi_kinds)
    triples = list(itertools.product(edge_values(n_regions, rbits), edge_values(n_cells, cbits), codes.values()))
    d, show = reads_from_triples(triples, stride, base, ordinal_base)
    return SimpleNamespace(names=names, regions=regions, snps=snps, n_cells=n_cells, d=d, triples=triples, layout=layout, codes=codes,
                           expected=answers(triples, show, snps))


# ----------------------------------------------------------------------------- larger tables, reads with CIGARs
def snp_table(n_snps, step=100, per_region=64):
    """n_snps SNPs, SNP k at 1-based position step * k + 50 with alleles cycling through the bases, and one region per `per_region`
    SNPs (the last region holds the remainder).  -> names, regions, snps"""
    k = np.arange(n_snps, dtype=np.int64)
    snps = list(zip(itertools.repeat("1"), (step * k + 50).tolist(), ["ACGT"[i & 3] for i in range(n_snps)],
                    ["ACGT"[(i + 1 + (i >> 2) % 3) & 3] for i in range(n_snps)], (k & 1).tolist(), (1 - (k & 1)).tolist()))
    g = np.arange((n_snps + per_region - 1) // per_region, dtype=np.int64)
    regions = list(zip(itertools.repeat("1"), (step * per_region * g + 1).tolist(), (step * per_region * (g + 1)).tolist(), itertools.repeat("r")))
    return ["1"], regions, snps


def plain_reads(pos, cell, umi, seed, ordinal_base=0):
    """91M reads with random bases at the given 0-based positions (sorted here).  -> batch dict"""
    rng = np.random.default_rng(seed)
    order = np.argsort(pos, kind="stable")
    n, nb = len(pos), (READ_LEN + 1) // 2
    nib = (1 << rng.integers(0, 4, (n, 2 * nb))).astype(np.uint8)
    return dict(contig=0, ordinal_base=ordinal_base, pos=np.asarray(pos)[order].astype(np.int32), flag=np.zeros(n, np.uint16),
                mapq=np.full(n, 60, np.uint8), cell=np.asarray(cell, np.int32)[order], umi=np.asarray(umi, np.uint64)[order],
                cig_off=np.arange(n + 1, dtype=np.uint32), cigar=np.full(n, (READ_LEN << 4) | 0, np.uint32),
                seq_off=(np.arange(n + 1) * nb).astype(np.uint32), seq=((nib[:, 0::2] << 4) | nib[:, 1::2]).reshape(-1))


M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8
TOP = 2 ** 31 - 1                 # the last 1-based position of a BAM contig; a read's end (0-based, exclusive) may equal it


def cigar_kinds(rng, L=91, gap_max=3000):
    """One CIGAR of every kind tests/fuzz_cases.py make_case() draws: M, N gaps, D, S + I, = / X, H + two N gaps + S."""
    a = int(rng.integers(1, L))
    return [[(M, L)], [(M, a), (N, int(rng.integers(1, gap_max))), (M, L - a)], [(M, a), (D, int(rng.integers(1, 400))), (M, L - a)],
            [(S, 3), (M, a), (I, 2), (M, L - a)], [(EQ, a), (X, 1), (M, max(1, L - a - 1))],
            [(H, 5), (M, a), (N, int(rng.integers(1, gap_max))), (M, 5), (N, int(rng.integers(1, gap_max))), (M, L), (S, 2)]]


def ref_len(cig):
    return sum(l for op, l in cig if op in (M, D, N, EQ, X))


def batch_from_records(recs, ordinal_base=0):
    """recs: (pos0, cigar [(op, len)], cell, umi) -> batch dict, sorted by position, with random bases."""
    recs = sorted(recs, key=lambda r: r[0])
    rng = np.random.default_rng(len(recs))
    cw, sq, cig_off, seq_off = [], [], [0], [0]
    for pos, cig, cell, umi in recs:
        cw += [(l << 4) | op for op, l in cig]; cig_off.append(len(cw))
        qlen = sum(l for op, l in cig if op in (M, I, S, EQ, X))
        nib = (1 << rng.integers(0, 4, qlen + (qlen & 1))).astype(np.uint8)
        sq.append((nib[0::2] << 4) | nib[1::2]); seq_off.append(seq_off[-1] + len(sq[-1]))
    n = len(recs)
    return dict(contig=0, ordinal_base=ordinal_base, pos=np.array([r[0] for r in recs], np.int32), flag=np.zeros(n, np.uint16),
                mapq=np.full(n, 60, np.uint8), cell=np.array([r[2] for r in recs], np.int32), umi=np.array([r[3] for r in recs], np.uint64),
                cig_off=np.array(cig_off, np.uint32), cigar=np.array(cw, np.uint32), seq_off=np.array(seq_off, np.uint32), seq=np.concatenate(sq))


def edge_coordinate_case(seed=7, n_reads=1500, n_cells=40, span=200000):
    """One contig with the same features at both ends of BAM's coordinate range: regions and SNPs in [1, span] and, mirrored, in
    [2^31 - span, 2^31 - 1] - a region starting at 1, one ending at 2^31 - 1, SNPs at positions 1 and 2^31 - 1 - and reads of every
    CIGAR kind over them.  Every read ends at or below 2^31 - 1 (asserted); some end exactly there, one 1M read starts at 2^31 - 2,
    some start at 0.  -> names, regions, snps, n_cells, batch dict"""
    rng = np.random.default_rng(seed)
    lo_regions = [(1, 500), (1, span)] + [(s, s + int(rng.choice([50, 500, 5000, 60000]))) for s in rng.integers(2, span - 61000, 30).tolist()]
    regions = [("1", s, e, "lo") for s, e in lo_regions] + [("1", TOP + 1 - e, TOP + 1 - s, "hi") for s, e in lo_regions]
    lo_snps = [1] + list(range(int(rng.integers(2, 40)), span, 37))
    snps = []
    for p in lo_snps + [TOP + 1 - p for p in reversed(lo_snps)]:
        r = int(rng.integers(0, 4)); h = int(rng.integers(0, 2))
        snps.append(("1", p, "ACGT"[r], "ACGT"[(r + int(rng.integers(1, 4))) % 4], h, 1 - h))
    assert regions[-1][2] <= TOP and max(r[2] for r in regions) == TOP and snps[-1][1] == TOP and regions[0][1] == 1
    recs = []
    for i in range(n_reads):
        cig = cigar_kinds(rng)[i % 6]
        rl = ref_len(cig)
        u = (1 << 24) | int(rng.integers(0, 3000))
        c = int(rng.integers(0, n_cells))
        p = int(rng.integers(0, span - 10))
        at_edge = i % 10 == 0                                            # every kind in turn ends exactly at 2^31 - 1 / starts at 0
        recs.append((0 if at_edge else p, cig, c, u))
        recs.append((TOP - rl if at_edge else min(TOP - span + p, TOP - rl), cig, c, u + 5000))
    recs.append((TOP - 1, [(M, 1)], 0, (1 << 24) | 9000))               # starts at 2^31 - 2, ends at 2^31 - 1: covers the last position only
    recs.append((0, [(M, 1)], 0, (1 << 24) | 9001))
    assert all(0 <= p and p + ref_len(cig) <= TOP for p, cig, _, _ in recs) and sum(p + ref_len(cig) == TOP for p, cig, _, _ in recs) > 100
    return ["1"], regions, snps, n_cells, batch_from_records(recs)
