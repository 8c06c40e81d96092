"""Hand-built read sets of the cell-mask tests of xck_refold (tests only): batches with the SNP depths, allele splits and gap records
the masked kernels branch on, the same batches with cell = -1 written in for the disabled cells, and the tallies counted on the host."""
import numpy as np

import util
from xcltk_amd import capi

FILT = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True)
NIB = {"A": 1, "C": 2, "G": 4, "T": 8}
M, N_OP = 0, 3                                                       # CIGAR op codes


def mask_batches(raw, enabled):
    """raw: [(Batch, holder)] as util.batch_from_dict returns them.  -> the same list with cell = -1 for every read of a cell that
    `enabled` (bool per cell) switches off: what a handle sees that never knew those cells.  The originals are not touched."""
    enabled = np.asarray(enabled, dtype=bool)
    out = []
    for b, keep in raw:
        cell = keep[3].copy()
        known = (cell >= 0) & (cell < len(enabled))
        off = known.copy()
        off[known] = ~enabled[cell[known]]
        cell[off] = -1
        nb = capi.Batch.from_buffer_copy(b)
        nb.cell = capi.np_ptr(cell, capi.C.c_int32)
        out.append((nb, (keep, cell)))
    return out


def _batch(reads, rng, read_len=31):
    """reads: [(pos0, cell, umi, [(len, op), ..], {read offset: nibble})] -> one position-sorted batch of read_len-base reads (stable:
    reads at one position keep their order, which is the fetch order)."""
    reads = [reads[i] for i in np.argsort(np.array([r[0] for r in reads]), kind="stable")]
    n, nb = len(reads), (read_len + 1) // 2
    seq = (1 << rng.integers(0, 4, (n, 2 * nb))).astype(np.uint8)
    for i, r in enumerate(reads):
        for off, nib in r[4].items():
            seq[i, off] = nib
    cig_off = np.zeros(n + 1, np.uint32)
    np.cumsum([len(r[3]) for r in reads], out=cig_off[1:])
    cigar = np.array([(ln << 4) | op for r in reads for ln, op in r[3]], dtype=np.uint32)
    d = dict(contig=0, ordinal_base=0, pos=np.array([r[0] for r in reads], np.int32), flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8),
             cell=np.array([r[1] for r in reads], np.int32), umi=np.array([(1 << 24) | r[2] for r in reads], np.uint64),
             cig_off=cig_off, cigar=cigar, seq_off=(np.arange(n + 1) * nb).astype(np.uint32),
             seq=((seq[:, 0::2] << 4) | seq[:, 1::2]).astype(np.uint8).ravel())
    return util.batch_from_dict(d)


def spread_case(n_cells, n_reads=900, seed=8):
    """A SNP every 60 bases, 30 regions, 91M reads of random cells and 64 UMIs (so molecules have several reads).
    -> names, regions, snps, [(Batch, holder)]"""
    rng = np.random.default_rng(seed + n_cells)
    snps = [("1", p, "ACGT"[k % 4], "ACGT"[(k + 1) % 4], k & 1, 1 - (k & 1)) for k, p in enumerate(range(10, 20000, 60))]
    regions = [("1", 100 + 650 * g, 700 + 650 * g, "g%d" % g) for g in range(30)]
    reads = [(int(rng.integers(0, 19900)), int(rng.integers(0, n_cells)), int(rng.integers(0, 64)), [(91, M)], {}) for _ in range(n_reads)]
    return ["1"], regions, snps, [_batch(reads, rng, 91)]


# ---- the deep case: 41 cells, every second one enabled ----
DEEP_CELLS, DEEP_SPAN, DEEP_MIN_COUNT, DEEP_MIN_MAF, GAP_MOLECULES = 41, 20000, 6, 0.1, 20
SNP_OFF = 10                                                         # where a read of the case shows its SNP
DEEP_SNPS = [("d2048", 1000), ("d2049", 2000), ("d4097", 3000), ("count_flip", 4000), ("maf_flip", 5000), ("gap", 6000)]


def deep_case(seed=1):
    """One contig.  SNP g lies in region g alone (regions of 11 bases), REF A on haplotype 0, ALT C on haplotype 1.
      d2048 / d2049 / d4097  that many molecules (molecule m: cell m % 41, UMI m // 41, one read each): TALLY_LONG, one more, and
                             one more than TALLY_PIECE - the short masked walk at its limit, one piece, two pieces
      count_flip             10 molecules, 4 of them in enabled cells: kept over all cells under min_count 6, dropped under the mask
      maf_flip               40 REF molecules in disabled cells, 4 REF + 2 ALT in enabled ones: minor share 2 / 46 < 0.1 over all
                             cells, 2 / 6 under the mask
      gap                    20 molecules in cells 0 .. 19 with UMI 7; two reads with an N gap over the SNP, earlier in fetch order,
                             carry (cell 0, UMI 7) and (cell 1, UMI 7): each claims its molecule, which then counts nowhere
      fillers                a SNP every 300 bases behind them under random reads with repeated (cell, UMI)
    -> names, regions, snps, [(Batch, holder)], mask, {SNP name: index}, {SNP name: [(cell, nibble) of every counted molecule]}"""
    rng = np.random.default_rng(seed)
    mask = np.arange(DEEP_CELLS) % 2 == 0
    pos_of = dict(DEEP_SNPS)
    fill = list(range(7000, 19000, 300))
    snps = [("1", p, "A", "C", 0, 1) for _, p in DEEP_SNPS] + [("1", p, "ACGT"[k % 4], "ACGT"[(k + 2) % 4], k & 1, 1 - (k & 1)) for k, p in enumerate(fill)]
    regions = [("1", s[1] - 5, s[1] + 5, "r%d" % g) for g, s in enumerate(snps)]
    idx = {name: g for g, (name, _) in enumerate(DEEP_SNPS)}
    reads, mols = [], {}

    def molecule(name, cell, umi, base):
        reads.append((pos_of[name] - 1 - SNP_OFF, cell, umi, [(31, M)], {SNP_OFF: NIB[base]}))
        mols.setdefault(name, []).append((cell, NIB[base]))

    for name, depth in (("d2048", 2048), ("d2049", 2049), ("d4097", 4097)):
        for m, base in enumerate(rng.choice(list("ACGT"), depth, p=[0.6, 0.3, 0.05, 0.05])):
            molecule(name, m % DEEP_CELLS, m // DEEP_CELLS, str(base))
    for m in range(10):                                              # enabled cells 0, 2, 4, 6; disabled 1, 3, 5, 7, 9, 11
        molecule("count_flip", [0, 2, 4, 6, 1, 3, 5, 7, 9, 11][m], 3, "AC"[m % 2])
    for m in range(40):
        molecule("maf_flip", 1 + 2 * (m % 20), m // 20, "A")
    for m in range(6):
        molecule("maf_flip", 2 * m, 5, "AAAACC"[m])
    for m in range(GAP_MOLECULES):
        molecule("gap", m, 7, "AC"[(m // 2) % 2])
    for cell in (0, 1):                                              # 5M 20N 26M from 15 bases left of the SNP: it lies in the gap
        reads.append((pos_of["gap"] - 1 - 15, cell, 7, [(5, M), (20, N_OP), (26, M)], {}))
    mols["gap"] = [(c, nb) for c, nb in mols["gap"] if c not in (0, 1)]
    for _ in range(1500):
        reads.append((int(rng.integers(6900, 18950)), int(rng.integers(0, DEEP_CELLS)), int(rng.integers(0, 48)), [(31, M)], {}))
    return ["1"], regions, snps, [_batch(reads, rng)], mask, idx, mols


def expected_tally(deep, name, mask):
    """[A, C, G, T, N] of the molecules of one named SNP of deep_case(), over the enabled cells (mask None: all)"""
    out = np.zeros(5, dtype=np.int64)
    for cell, nib in deep[6][name]:
        if mask is None or mask[cell]:
            out[{1: 0, 2: 1, 4: 2, 8: 3}.get(nib, 4)] += 1
    return out
