"""Shared helpers of the xck_refold tests (tests only; may import oracle/): a set of tables and filters ("variant"), the oracle and a
fresh engine under it, and random variants for the cases of tests/fuzz_cases.py."""
import ctypes as C

import numpy as np

import oracle as O
from xcltk_amd import capi
from xcltk_amd.engine import Engine

MATS = ["ad", "dp", "oth"]


def variant(regions, snps, enabled=None, excl=None, min_count=1, min_maf=0, no_dup_hap=True):
    return dict(regions=list(regions), snps=list(snps), enabled=None if enabled is None else np.asarray(enabled, dtype=bool),
                excl=excl, min_count=min_count, min_maf=min_maf, no_dup_hap=no_dup_hap)


def subset(v):
    """The variant as a fresh handle sees it: the SNP list without the disabled SNPs, the exclusion pairs renumbered to it (pairs
    of a disabled SNP dropped).  -> (snps, excl or None)"""
    if v["enabled"] is None:
        return v["snps"], v["excl"]
    en = v["enabled"]
    new_idx = np.cumsum(en) - 1
    snps = [s for s, e in zip(v["snps"], en.tolist()) if e]
    excl = None
    if v["excl"] is not None:
        er, es = (np.asarray(x, dtype=np.int64) for x in v["excl"])
        ok = en[es]
        excl = (er[ok].astype(np.int32), new_idx[es[ok]].astype(np.int32))
    return snps, excl


def filters_of(v):
    return dict(min_count=v["min_count"], min_maf=v["min_maf"], no_dup_hap=v["no_dup_hap"])


def refold(eng, v, copy=True):
    return eng.refold(v["regions"], snps=v["snps"], snp_enabled=v["enabled"], excl_pairs=v["excl"], copy=copy, **filters_of(v))


def oracle_of(names, v, n_cells, batches, read_filters, flags=0, unknown_contig=None):
    """unknown_contig: name of a contig outside `names`: its regions get contig -1 (they keep empty rows)."""
    snps, excl = subset(v)
    regions = v["regions"]
    if unknown_contig is not None:
        regions = [(names[0],) + tuple(r[1:]) if r[0] == unknown_contig else r for r in regions]
    cfg, keep = O.make_config(capi.XCK_MODE_BAF, names, regions, snps, n_cells, flags=flags, **read_filters, **filters_of(v))
    if unknown_contig is not None:
        keep[0]["contig"][[i for i, r in enumerate(v["regions"]) if r[0] == unknown_contig]] = -1
    if excl is not None and len(excl[0]):
        er, es = (np.ascontiguousarray(x, dtype=np.int32) for x in excl)
        cfg.n_excl_pairs = len(er)
        cfg.excl_region = er.ctypes.data_as(C.POINTER(C.c_int32))
        cfg.excl_snp = es.ctypes.data_as(C.POINTER(C.c_int32))
        keep = keep + (er, es)
    return O.run_oracle(cfg, batches)


def fresh_engine(names, v, n_cells, read_filters, flags=0, mode=capi.XCK_MODE_BAF, **kw):
    snps, excl = subset(v)
    return Engine(mode, names, v["regions"], n_cells, snps=snps, flags=flags, excl_pairs=excl, **read_filters, **filters_of(v), **kw)


def fresh_result(names, v, n_cells, batches, read_filters, flags=0):
    eng = fresh_engine(names, v, n_cells, read_filters, flags)
    try:
        for b in batches:
            eng.push(b)
        return eng.finish()
    finally:
        eng.close()


def random_variant(rng, names, regions, snps, span):
    """Other tables for the same reads: random regions (overlapping and duplicated ones included, never more than the larger of the
    two tables the handle was sized for), haplotype bits flipped, REF / ALT swapped on some SNPs, a random third of the SNPs
    disabled, other filters, no_dup_hap drawn anew, exclusion pairs - real (region, SNP) overlaps, pairs that do not overlap, and
    duplicates."""
    n_max = max(len(regions), len(snps), 2)
    n_reg = int(rng.integers(1, min(80, n_max) + 1))
    reg = []
    for g in range(n_reg):
        c = names[int(rng.integers(0, len(names)))]
        s = int(rng.integers(1, span - 100)); ln = int(rng.choice([50, 500, 5000, 60000, span]))
        reg.append((c, s, min(span, s + int(rng.integers(1, ln + 1))), "b%d" % g))
    for _ in range(min(3, n_max - len(reg))):
        reg.append(reg[int(rng.integers(0, len(reg)))][:3] + ("dup",))
    new = []
    for s in snps:
        ref, alt, rh, ah = s[2], s[3], s[4], s[5]
        if rng.random() < 0.4:
            rh, ah = ah, rh
        if rng.random() < 0.3:
            ref, alt = alt, ref
        new.append((s[0], s[1], ref, alt, rh, ah))
    enabled = rng.random(len(snps)) >= 1 / 3
    er, es = [], []
    if len(snps):
        by = {}
        for i, s in enumerate(snps):
            by.setdefault(s[0], []).append((s[1], i))
        for g, r in enumerate(reg):
            inside = [i for p, i in by.get(r[0], []) if r[1] <= p <= r[2]]
            for i in inside:
                if rng.random() < 0.15:
                    er.append(g); es.append(i)
        for _ in range(10):                                            # pairs that need not overlap
            er.append(int(rng.integers(0, len(reg)))); es.append(int(rng.integers(0, len(snps))))
        er += er[:5]; es += es[:5]                                     # duplicates
    excl = (np.array(er, dtype=np.int32), np.array(es, dtype=np.int32)) if er else None
    return variant(reg, new, enabled, excl, min_count=int(rng.choice([1, 2, 5])), min_maf=float(rng.choice([0, 0.1, 0.3])),
                   no_dup_hap=bool(rng.random() < 0.5))


def brute_force_membership(names, v):
    """-> (regions per SNP, SNPs per region) of a variant by the definition: start <= pos <= end, end >= start, same known contig,
    SNP enabled and in the tables (known contig, pos >= 1), the pair not excluded; duplicates of a pair count once."""
    regions, snps = v["regions"], v["snps"]
    known = set(names)
    en = np.ones(len(snps), dtype=bool) if v["enabled"] is None else v["enabled"]
    ex = set(zip(*[x.tolist() for x in v["excl"]])) if v["excl"] is not None else set()
    per_snp = np.zeros(len(snps), dtype=np.int64); per_reg = np.zeros(len(regions), dtype=np.int64)
    pos = np.array([s[1] for s in snps], dtype=np.int64); chrom = np.array([s[0] for s in snps])
    ok = en & (pos >= 1) & np.array([c in known for c in chrom.tolist()], dtype=bool) if len(snps) else en
    for g, r in enumerate(regions):
        if r[0] not in known or r[2] < r[1] or not len(snps):
            continue
        hit = np.flatnonzero(ok & (chrom == r[0]) & (pos >= r[1]) & (pos <= r[2]))
        if ex:
            hit = np.array([i for i in hit.tolist() if (g, i) not in ex], dtype=np.int64)
        per_snp[hit] += 1; per_reg[g] += len(hit)
    return per_snp, per_reg
