"""Helpers of the per-cell table tests (tests/test_cell_summary_host.py, tests/test_gpu_cell_summary.py, the two-rank worker): the
fixtures under tests/golden/cell_summary/ (written by tools/make_read_fate_goldens.py from the reference's own check_read /
sam_fetch / include code, next to the read_fate ones) and a plain-Python restatement of the classification, read by read and
grouped by cell, written from the comments of xck_read_fate / xck_config in include/xck.h - it never calls the library."""
import bisect
import json
import os

import numpy as np

import read_fate_util as R

CDIR = os.path.join(R.GOLDEN, "cell_summary")
# the columns of xck_cell_summary.fate: the classes a kernel can give a read, then the two sums over the assigned reads
COLS = R.CLASSES[1:] + ("multi", "pairs")
N_CLASSES = len(COLS) - 2
(LOW_MAPQ, EXCL_FLAG, INCL_FLAG, ORPHAN, NO_CELL, NO_UMI, SHORT, NO_TARGET, INCLUDE_FAIL, ASSIGNED, MULTI, PAIRS) = range(12)
UMI_NONE = 0xFFFFFFFFFFFFFFFF
OP_REF = (0, 2, 3, 7, 8)          # M D N = X consume the reference
OP_ALIGNED = (0, 7, 8)            # M = X are aligned bases


def list_fixtures():
    return sorted(f[:-5] for f in os.listdir(CDIR) if f.endswith(".json")) if os.path.isdir(CDIR) else []


def load_cell_fixture(name):
    """-> (the fixture dict, its table as int64 [(n_cells + 1), 12] in the engine's row order: the listed cells, then `*`)"""
    with open(os.path.join(CDIR, name + ".json")) as fp:
        cx = json.load(fp)
    assert tuple(cx["columns"]) == COLS
    row_of = {c: i for i, c in enumerate(cx["cells"])}
    row_of["*"] = len(cx["cells"])
    tab = np.zeros((len(cx["cells"]) + 1, len(COLS)), dtype=np.int64)
    for k, v in cx["rows"].items():
        tab[row_of[k]] = v
    return cx, tab


def expected_lines(cx, tab, matrix, names=None):
    """lines of cell_summary.tsv below the header (and without a `#ranks` line) for a fixture's table and the column marginals
    `matrix` [n_cells, k]; names: the matrix columns in the order of the run (the fixture lists them sorted)"""
    names = list(cx["cells"]) if names is None else list(names)
    row_of = {c: i for i, c in enumerate(cx["cells"])}
    out = []
    for i, name in enumerate(names + ["*"]):
        f = tab[row_of[name]] if i < len(names) else tab[-1]
        m = matrix[i] if i < len(names) else np.zeros(matrix.shape[1], dtype=np.int64)
        vals = [int(f[:N_CLASSES].sum())] + [int(x) for x in f] + [int(x) for x in m]
        out.append(name + "\t" + "\t".join(str(v) for v in vals))
    return out


def mtx_marginals(path, n_cells):
    """(column sums, entries per column) of a MatrixMarket file the reference wrote"""
    s = np.zeros(n_cells, dtype=np.int64)
    c = np.zeros(n_cells, dtype=np.int64)
    with open(path) as fp:
        lines = [x for x in fp if not x.startswith("%")]
    assert int(lines[0].split()[1]) == n_cells
    for x in lines[1:]:
        _, col, val = x.split()
        s[int(col) - 1] += int(val)
        c[int(col) - 1] += 1
    return s, c


def coo_marginals(coo, n_cells):
    row, col, val = coo
    return (np.bincount(col, weights=None if len(val) == 0 else val.astype(np.float64), minlength=n_cells).astype(np.int64),
            np.bincount(col, minlength=n_cells).astype(np.int64))


def expected_matrix(mode_is_basefc, res, n_cells):
    """the matrix half from the arrays Engine.finish() returned: basefc (umis, features), BAF (ad, dp, oth, features of DP)"""
    if mode_is_basefc:
        s, c = coo_marginals(res["count"], n_cells)
        return np.stack([s, c], axis=1)
    ad, _ = coo_marginals(res["ad"], n_cells)
    dp, ndp = coo_marginals(res["dp"], n_cells)
    oth, _ = coo_marginals(res["oth"], n_cells)
    return np.stack([ad, dp, oth, ndp], axis=1)


# ----------------------------------------------------------------------------- the restatement
class Tables(object):
    """what a pipeline's kernels judge a read against: per contig the regions fetch() accepts (1-based inclusive start / end ->
    0-based half-open [start - 1, end); start < 1 or start - 1 > end fetches nothing) and the sorted 0-based SNP positions"""

    def __init__(self, names, regions, snps):
        cidx = {n: i for i, n in enumerate(names)}
        self.regs = [[] for _ in names]
        for r in regions:
            if r[1] < 1 or r[1] - 1 > r[2]:
                continue
            self.regs[cidx[r[0]]].append((r[1] - 1, r[2]))
        self.snps = [[] for _ in names]
        for s in snps:
            if s[1] >= 1:
                self.snps[cidx[s[0]]].append(s[1] - 1)
        for v in self.snps:
            v.sort()


def classify(t, basefc, contig, pos, flag, mapq, cell, umi, cig, f):
    """-> (class, pairs) of one read: the first class that applies in the order of the fields of xck_read_fate"""
    if mapq < f["min_mapq"]:
        return LOW_MAPQ, 0
    if f["excl_flag"] and (flag & f["excl_flag"]):
        return EXCL_FLAG, 0
    if f["incl_flag"] and not (flag & f["incl_flag"]):
        return INCL_FLAG, 0
    if f["no_orphan"] and (flag & 1) and not (flag & 2):
        return ORPHAN, 0
    if cell < 0:
        return NO_CELL, 0
    if umi == UMI_NONE:
        return NO_UMI, 0
    ops = [(w & 15, w >> 4) for w in cig]
    n_al = sum(l for op, l in ops if op in OP_ALIGNED)
    if n_al < f["min_len"]:
        return SHORT, 0
    rlen = sum(l for op, l in ops if op in OP_REF)
    mapped_span = not ((flag & 4) or not ops or rlen == 0)      # otherwise the read spans one base, as htslib's bam_endpos() has it
    end = pos + (rlen if mapped_span else 1)
    if not basefc:
        v = t.snps[contig]
        n = bisect.bisect_left(v, end) - bisect.bisect_left(v, pos)      # SNPs with pos <= p0 < end, duplicates count each
        return (ASSIGNED, n) if n else (NO_TARGET, 0)
    mi = f["min_include"]
    n_ov = n_acc = 0
    for s0, e0 in t.regs[contig]:
        if not (pos < e0 and end > s0):
            continue
        n_ov += 1
        if mapped_span and pos >= s0 and end <= e0:
            m = n_al
        else:                                                    # aligned bases inside [s0, e0)
            m, p = 0, pos
            for op, l in ops:
                if op in OP_ALIGNED:
                    m += max(0, min(p + l, e0) - max(p, s0))
                if op in OP_REF:
                    p += l
        if 0 < mi < 1:
            if n_al <= 0 or m / float(n_al) < mi:
                continue
        elif m < mi:
            continue
        n_acc += 1
    if n_acc:
        return ASSIGNED, n_acc
    return (INCLUDE_FAIL if n_ov else NO_TARGET), 0


def restate(names, regions, snps, n_cells, batches, filt, basefc):
    """batches: dicts of numpy arrays (contig, pos, flag, mapq, cell, umi, cig_off, cigar).  -> (table int64 [(n_cells + 1), 12],
    reads of the batches no kernel sees: contig < 0, or a contig without a region / without a SNP)"""
    t = Tables(names, regions, snps)
    tab = np.zeros((n_cells + 1, len(COLS)), dtype=np.int64)
    not_joined = 0
    for b in batches:
        c = int(b["contig"])
        n = len(b["pos"])
        if c < 0 or not (t.regs[c] if basefc else t.snps[c]):
            not_joined += n
            continue
        pos, flag, mapq, cell, umi = (b[k].tolist() for k in ("pos", "flag", "mapq", "cell", "umi"))
        off, cigar = b["cig_off"].tolist(), b["cigar"].tolist()
        for i in range(n):
            cls, pairs = classify(t, basefc, c, pos[i], flag[i], mapq[i], cell[i], umi[i], cigar[off[i]:off[i + 1]], filt)
            row = cell[i] if cell[i] >= 0 else n_cells
            tab[row, cls] += 1
            if pairs:
                tab[row, PAIRS] += pairs
                tab[row, MULTI] += 1 if pairs >= 2 else 0
    return tab, not_joined


def batch_dict(keep, contig):
    """the arrays capi.make_batch() kept alive (util.batch_from_dict returns them next to the struct) as a dict for restate()"""
    return dict(contig=contig, pos=keep[0], flag=keep[1], mapq=keep[2], cell=keep[3], umi=keep[4], cig_off=keep[5], cigar=keep[6])
