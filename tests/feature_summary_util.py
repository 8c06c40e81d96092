"""Helpers of the per-feature / per-SNP table tests (tests/test_feature_summary_host.py, tests/test_gpu_feature_summary.py, the two-rank
worker): the fixtures under tests/golden/feature_summary/ (written by tools/make_feature_summary_goldens.py from the reference's own
check_read / sam_fetch / include code and plp_snp) and a plain-Python restatement, pair by pair, written from the comments of
xck_feature_summary / xck_read_fate / xck_config in include/xck.h - it never calls the library."""
import bisect
import json
import os

import numpy as np

import cell_summary_util as CU
import read_fate_util as R

FDIR = os.path.join(R.GOLDEN, "feature_summary")
READ_COLS = ("include_fail", "pairs", "shared")
INCLUDE_FAIL, PAIRS, SHARED = range(3)
SNP_COLS = ("reads", "a", "c", "g", "t", "n", "kept", "regions")
S_READS, S_A, S_N, S_KEPT, S_REGIONS = 0, 1, 5, 6, 7
MATRIX_COLS = {"basefc": ("umis", "cells"), "baf": ("snps", "snps_kept", "ad", "dp", "oth", "cells")}
BASE_IDX = {"A": 0, "C": 1, "G": 2, "T": 3}


def list_fixtures():
    return sorted(f[:-5] for f in os.listdir(FDIR) if f.endswith(".json")) if os.path.isdir(FDIR) else []


def load_fixture(name):
    """-> (the read-fate style fixture dict that R.fixture_engine takes, the feature fixture dict)"""
    with open(os.path.join(FDIR, name + ".json")) as fp:
        gx = json.load(fp)
    fx = R.load_fixture(gx["fate"])
    fx = dict(fx, params=dict(fx["params"], **{k: gx["params"][k] for k in ("min_count", "min_maf")}))
    return fx, gx


def snp_keys(snps):
    """the fixture's row keys of a SNP list: `chrom:pos:ref:alt#k`, k counting the entries with the same text"""
    seen, out = {}, []
    for s in snps:
        text = "%s:%d:%s:%s" % (s[0], s[1], s[2], s[3])
        out.append("%s#%d" % (text, seen.get(text, 0)))
        seen[text] = seen.get(text, 0) + 1
    return out


def fixture_table(gx, regions=None, snps=None):
    """the fixture's rows as int64 [n, columns] in the order of the given input list (basefc: regions, BAF: snps)"""
    if gx["mode"] == "basefc":
        assert gx["keys"] == ["%s:%d-%d" % (r[0], r[1], r[2]) for r in regions]
        keys = [str(i) for i in range(len(regions))]
    else:
        keys = snp_keys(snps)
        assert sorted(keys) == sorted(gx["keys"])
    tab = np.zeros((len(keys), len(gx["columns"])), dtype=np.int64)
    if gx["mode"] != "basefc":
        tab[:, 6] = 3                                            # (a SNP without a row: no read, no tally, dropped for min_count)
    for i, k in enumerate(keys):
        if k in gx["rows"]:
            tab[i] = gx["rows"][k]
    return tab


# ----------------------------------------------------------------------------- the restatement
def read_span(pos, flag, mapq, cell, umi, cig, f):
    """None for a read that fails anything up to short_aligned (check_read, a listed cell, a non-empty key, min_len), else
    (pos, end, aligned bases, [(op, len)], whether the fetch span is the CIGAR's)"""
    if mapq < f["min_mapq"]:
        return None
    if f["excl_flag"] and (flag & f["excl_flag"]):
        return None
    if f["incl_flag"] and not (flag & f["incl_flag"]):
        return None
    if f["no_orphan"] and (flag & 1) and not (flag & 2):
        return None
    if cell < 0 or umi == CU.UMI_NONE:
        return None
    ops = [(w & 15, w >> 4) for w in cig]
    n_al = sum(l for op, l in ops if op in CU.OP_ALIGNED)
    if n_al < f["min_len"]:
        return None
    rlen = sum(l for op, l in ops if op in CU.OP_REF)
    mapped_span = not ((flag & 4) or not ops or rlen == 0)      # otherwise one base, as htslib's bam_endpos() has it
    return pos, pos + (rlen if mapped_span else 1), n_al, ops, mapped_span


def region_outcome(span, s0, e0, min_include):
    """None: the region [s0, e0) does not fetch the read; False: fetched, fails min_include; True: accepted"""
    pos, end, n_al, ops, mapped_span = span
    if not (pos < e0 and end > s0):
        return None
    m, p = 0, pos                                                # aligned bases inside [s0, e0)
    for op, l in ops:
        if op in CU.OP_ALIGNED:
            m += max(0, min(p + l, e0) - max(p, s0))
        if op in CU.OP_REF:
            p += l
    if 0 < min_include < 1:
        return n_al > 0 and not (m / float(n_al) < min_include)
    return not (m < min_include)


def restate(names, regions, snps, batches, filt, basefc):
    """batches: dicts of numpy arrays (contig, pos, flag, mapq, cell, umi, cig_off, cigar).
    basefc -> (int64 [n_regions, 3]: include_fail, pairs, shared in input order; reads with two or more accepting regions)
    BAF    -> (int64 [n_snps]: reads per SNP in input order; reads over two or more SNPs)"""
    cidx = {n: i for i, n in enumerate(names)}
    multi = 0
    if basefc:
        tab = np.zeros((len(regions), 3), dtype=np.int64)
        regs = [[] for _ in names]
        for g, r in enumerate(regions):
            if r[1] >= 1 and r[1] - 1 <= r[2]:                   # (what fetch() accepts)
                regs[cidx[r[0]]].append((r[1] - 1, r[2], g))
    else:
        tab = np.zeros(len(snps), dtype=np.int64)
        pos_of = [[] for _ in names]
        for k, s in enumerate(snps):
            if s[1] >= 1:
                pos_of[cidx[s[0]]].append((s[1] - 1, k))
        for v in pos_of:
            v.sort()
        p0_of = [[p for p, _ in v] for v in pos_of]
    for b in batches:
        c = int(b["contig"])
        if c < 0:
            continue
        pos, flag, mapq, cell, umi = (b[k].tolist() for k in ("pos", "flag", "mapq", "cell", "umi"))
        off, cigar = b["cig_off"].tolist(), b["cigar"].tolist()
        for i in range(len(pos)):
            span = read_span(pos[i], flag[i], mapq[i], cell[i], umi[i], cigar[off[i]:off[i + 1]], filt)
            if span is None:
                continue
            if basefc:
                acc = []
                for s0, e0, g in regs[c]:
                    o = region_outcome(span, s0, e0, filt["min_include"])
                    if o is False:
                        tab[g, INCLUDE_FAIL] += 1
                    elif o:
                        acc.append(g)
                for g in acc:
                    tab[g, PAIRS] += 1
                    tab[g, SHARED] += 1 if len(acc) >= 2 else 0
                multi += 1 if len(acc) >= 2 else 0
            else:
                lo, hi = bisect.bisect_left(p0_of[c], span[0]), bisect.bisect_left(p0_of[c], span[1])
                for _, k in pos_of[c][lo:hi]:
                    tab[k] += 1
                multi += 1 if hi - lo >= 2 else 0
    return tab, multi


def bam_batches(fx, names, barcodes):
    """the records of a fixture's BAMs, read by oracle/pybam.py, as one batch dict per (file, contig) for restate(): cell = index of
    the barcode in `barcodes` (sorted list) or of the file (barcodes None); umi = 1, or UMI_NONE for a missing / empty key"""
    import oracle as O
    import pybam
    p = fx["params"]
    cell_of = {b: i for i, b in enumerate(barcodes)} if barcodes is not None else None
    out = []
    for bi, fn in enumerate(fx["bam_fns"]):
        refs, recs = pybam.read_bam(fn)
        t2c = O.resolve_contigs([n for n, _ in refs], names)
        per = {}
        for r in recs:
            c = t2c[r.tid] if 0 <= r.tid < len(t2c) else -1
            if c < 0:
                continue
            if cell_of is not None:
                tag = r.get_tag(p["cell_tag"]) if r.has_tag(p["cell_tag"]) else None
                cell = cell_of.get(tag, -1) if isinstance(tag, str) else -1
            else:
                cell = bi
            if p["umi_tag"]:
                key = r.get_tag(p["umi_tag"]) if r.has_tag(p["umi_tag"]) else None
            else:
                key = r.query_name
            d = per.setdefault(c, dict(pos=[], flag=[], mapq=[], cell=[], umi=[], cig_off=[0], cigar=[]))
            d["pos"].append(r.pos); d["flag"].append(r.flag); d["mapq"].append(r.mapq); d["cell"].append(cell)
            d["umi"].append(1 if key else CU.UMI_NONE)
            d["cigar"] += [(l << 4) | op for op, l in (r.cigartuples or [])]
            d["cig_off"].append(len(d["cigar"]))
        for c, d in sorted(per.items()):
            out.append(dict(contig=c, pos=np.array(d["pos"], dtype=np.int64), flag=np.array(d["flag"], dtype=np.int64),
                            mapq=np.array(d["mapq"], dtype=np.int64), cell=np.array(d["cell"], dtype=np.int64),
                            umi=np.array(d["umi"], dtype=np.uint64), cig_off=np.array(d["cig_off"], dtype=np.int64),
                            cigar=np.array(d["cigar"], dtype=np.int64)))
    return out


# ----------------------------------------------------------------------------- the matrix half
def snp_region_counts(regions, snps, kept=None, excl_pairs=None):
    """per region: SNPs of the list joined to it (same contig, start <= pos <= end, minus the exclusion pairs) and, given the per-SNP
    `kept` column, those of them that were kept; per SNP: the regions it feeds.  int64 [n_regions, 2], int64 [n_snps]"""
    excl = set(zip(excl_pairs[0], excl_pairs[1])) if excl_pairs else set()
    out = np.zeros((len(regions), 2), dtype=np.int64)
    fan = np.zeros(len(snps), dtype=np.int64)
    by_chrom = {}
    for k, s in enumerate(snps):
        if s[1] >= 1:
            by_chrom.setdefault(s[0], []).append((s[1], k))
    for v in by_chrom.values():
        v.sort()
    for g, r in enumerate(regions):
        v = by_chrom.get(r[0], [])
        for _, k in v[bisect.bisect_left(v, (r[1], -1)):bisect.bisect_left(v, (r[2] + 1, -1))]:
            if (g, k) in excl:
                continue
            out[g, 0] += 1
            fan[k] += 1
            if kept is not None and kept[k]:
                out[g, 1] += 1
    return out, fan


def _row_marginals(coo, n):
    row, col, val = coo
    return (np.bincount(row, weights=None if len(val) == 0 else val.astype(np.float64), minlength=n).astype(np.int64),
            np.bincount(row, minlength=n).astype(np.int64))


def expected_matrix(mode_is_basefc, res, regions, snps=(), kept=None, excl_pairs=None):
    """the matrix half from the arrays Engine.finish() returned: basefc (umis, cells); BAF (snps, snps_kept, ad, dp, oth, cells of DP)"""
    n = len(regions)
    if mode_is_basefc:
        s, c = _row_marginals(res["count"], n)
        return np.stack([s, c], axis=1)
    rs, _ = snp_region_counts(regions, snps, kept, excl_pairs)
    ad, _ = _row_marginals(res["ad"], n)
    dp, ndp = _row_marginals(res["dp"], n)
    oth, _ = _row_marginals(res["oth"], n)
    return np.stack([rs[:, 0], rs[:, 1], ad, dp, oth, ndp], axis=1)


def verdict(tally, ref, alt, min_count, min_maf):
    """the per-SNP filter, in Python floats: kept unless the total is below min_count or the minor count below total * min_maf"""
    tot = int(sum(tally))
    minor = min(int(tally[BASE_IDX.get(ref, 4)]), int(tally[BASE_IDX.get(alt, 4)]))
    return 0 if (tot < min_count or minor < tot * min_maf) else 1
