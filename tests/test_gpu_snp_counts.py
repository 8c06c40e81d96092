"""xck_snp_counts / Engine.snp_counts: the SNP x cell AD / DP / OTH matrices of a finished pileup, counted from what xck_finish keeps
of the molecule stage (csrc/snp_counts.h), and the one-pass `xcltk baf` built on it (baf/onepass.py).  The expected matrices come from
the CPU oracle driven with one one-base region per SNP (REF on haplotype 0, ALT on 1, min_count 1, min_maf 0, no_dup_hap) - the
construction baf/genotype.py has always used.  Every test calls the new method or the new module, so none passes without them."""
import collections
import functools
import os
import re

import numpy as np
import pytest

import fuzz_cases
import refold_util as R
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError

pytestmark = pytest.mark.gpu
BAF = capi.XCK_MODE_BAF
READ_FILTER_KEYS = ("min_mapq", "min_len", "incl_flag", "excl_flag", "no_orphan")
FILT = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xcltk_amd", "csrc")


def _const(fn, name):
    """An integer constant of a kernel source file (`NAME = 123` inside a constexpr line)."""
    m = re.search(r"\b%s\s*=\s*(\d+)\b" % name, open(os.path.join(CSRC, fn)).read())
    assert m, name
    return int(m.group(1))


RUN_WALK = _const("finish.hip", "RUN_WALK")                          # followers a run head walks itself
SNC_TILE = _const("snp_counts.h", "SNC_BLOCK") * _const("snp_counts.h", "SNC_ITEMS")
SC_TILE = _const("fold_partition.h", "SC_T") * _const("fold_partition.h", "SC_I")
SC_PASS = SC_TILE * int(re.search(r"__launch_bounds__\((\d+)\) void k_scan_top", open(os.path.join(CSRC, "fold_partition.h")).read()).group(1))


def onebase(snps):
    """The variant with one one-base region per SNP, REF on haplotype 0 and ALT on 1: its region-level matrices are the SNP-level
    ones.  Two SNPs at one position would meet in each other's region: those pairs are excluded, so a row holds its own SNP alone."""
    regions = [(s[0], s[1], s[1], "s%d" % i) for i, s in enumerate(snps)]
    by = collections.defaultdict(list)
    for i, s in enumerate(snps):
        by[(s[0], s[1])].append(i)
    er, es = [], []
    for grp in by.values():
        for g in grp:
            for i in grp:
                if g != i:
                    er.append(g); es.append(i)
    excl = (np.array(er, dtype=np.int32), np.array(es, dtype=np.int32)) if er else None
    return R.variant(regions, [(s[0], s[1], s[2], s[3], 0, 1) for s in snps], excl=excl)


def _same(a, b):
    util.assert_coo_equal(a, b, R.MATS)


def _sorted_by_row_col(m, n_rows):
    for k in R.MATS:
        row, col, val = (x.astype(np.int64) for x in m[k])
        assert np.all(val > 0)
        if len(row):
            assert row.min() >= 0 and row.max() < n_rows
            key = row * (1 << 32) + col
            assert np.all(key[1:] > key[:-1]), k


# ---------------------------------------------------------------------------------------------- 1. fuzz, every fold path
def _dev_blocks(eng):
    import torch
    from xcltk_amd import shard
    out = {}
    for m, (ptr, nnz) in eng.result_device().items():
        out[m] = (ptr, nnz, torch.as_tensor(shard._DevArray(ptr, 3 * nnz), device="cuda:0").cpu().numpy() if nnz else np.zeros(0, np.int32))
    return out


def _roundtrip(seed, flags=0, mode=BAF, case=None):
    names, regions, snps, n_cells, raw, fc, baf, case_flags = case or fuzz_cases.make_case(seed, many_cells=False, long=False)
    batches = [b for b, _ in raw]
    flags |= case_flags
    rf = {k: baf[k] for k in READ_FILTER_KEYS}
    a = R.variant(regions, snps, min_count=baf["min_count"], min_maf=baf["min_maf"], no_dup_hap=baf["no_dup_hap"])
    one = onebase(snps)
    exp = R.oracle_of(names, one, n_cells, batches, rf, flags)
    eng = R.fresh_engine(names, a, n_cells, rf, flags, mode=mode, **(dict(min_include=fc["min_include"]) if mode != BAF else {}))
    try:
        for bt in batches:
            eng.push(bt)
        r_a = eng.finish()
        got = eng.snp_counts()
        _same(got, exp)
        _sorted_by_row_col(got, len(snps))
        r_one = R.refold(eng, one)                                   # the detour: one one-base region per SNP on the same handle
        _same(r_one, got)
        _same(eng.snp_counts(), got)                                 # ... after which the call answers the same
        view = R.refold(eng, a, copy=False)                          # back to the original tables: views of the pinned result blocks
        snap = {k: tuple(x.copy() for x in view[k]) for k in R.MATS}
        dev = _dev_blocks(eng)
        _same(snap, r_a)
        _same(eng.snp_counts(), got)
        _same(eng.snp_counts(copy=False), got)
        _same(view, snap)                                            # the region-level result did not move or change
        dev2 = _dev_blocks(eng)
        for m in R.MATS:
            assert dev2[m][:2] == dev[m][:2] and np.array_equal(dev2[m][2], dev[m][2]) and np.array_equal(dev[m][2], np.concatenate(snap[m]))
        # other alleles, a SNP mask, other regions and filters: the call follows the alleles and nothing else
        b = R.random_variant(np.random.default_rng(1000 + seed), names, regions, snps, max([r[2] for r in regions] + [s[1] for s in snps] + [400]))
        r_b = R.refold(eng, b)
        _same(eng.snp_counts(), R.oracle_of(names, onebase(b["snps"]), n_cells, batches, rf, flags))
        _same(eng.refold(b["regions"], snps=b["snps"], snp_enabled=b["enabled"], excl_pairs=b["excl"], **R.filters_of(b)), r_b)
        print("seed %d: %d SNPs, nnz(dp) %d, nnz(oth) %d" % (seed, len(snps), len(got["dp"][0]), len(got["oth"][0])))
        return eng.stats()
    finally:
        eng.close()


@pytest.mark.parametrize("seed", [11, 13, 24, 25, 29, 39, 43, 46, 52, 53])
def test_snp_counts_matches_oracle_and_the_one_base_refold(seed):
    _roundtrip(seed)


@pytest.mark.parametrize("seed", [25, 53])
@pytest.mark.parametrize("knob", ["radix", "key128", "fold_c", "hit_cap0", "both"])
def test_snp_counts_on_every_fold_path(seed, knob, monkeypatch):
    from test_gpu_refold import _dense_case
    env = {"radix": ("XCK_PILEUP_SORT", "radix"), "fold_c": ("XCK_FOLD_C", "64"), "hit_cap0": ("XCK_HIT_CAP0", "64")}
    if knob in env:
        monkeypatch.setenv(*env[knob])                               # (a handle reads its knobs at xck_create)
    if knob == "hit_cap0":
        monkeypatch.setenv("XCK_HIT_SLACK", "0")                     # the first launch overflows and is replayed
    st = _roundtrip(seed, flags=capi.XCK_F_FORCE_KEY128 if knob == "key128" else 0, mode=capi.XCK_MODE_BOTH if knob == "both" else BAF,
                    case=_dense_case(seed) if knob == "hit_cap0" else None)
    if knob == "hit_cap0":
        assert st["n_join_launches"] > 1
    if knob == "radix":
        assert st["pileup_sort_path"] in (0, 2)                      # mol_keys sits in d_keys
    if knob == "key128":
        assert st["key_bits"] == 128


# ---------------------------------------------------------------------------------------------- 2. run shapes, gaps, alleles
def _batch(reads, seed, n_frac=0.0):
    """reads: [(pos0, cell, umi, cigar ops [(op, len)])] in fetch order, on contig 0; random bases (a share n_frac of them N)."""
    rng = np.random.default_rng(seed)
    n = len(reads)
    cig_off = np.zeros(n + 1, np.uint32); seq_off = np.zeros(n + 1, np.uint32); cw, sq = [], []
    for t, (_, _, _, cig) in enumerate(reads):
        cw += [(ln << 4) | op for op, ln in cig]
        qlen = sum(ln for op, ln in cig if op in (0, 1, 4, 7, 8))
        nib = (1 << rng.integers(0, 4, qlen + (qlen & 1))).astype(np.uint8)
        nib[rng.random(len(nib)) < n_frac] = 15
        sq.append((nib[0::2] << 4) | nib[1::2])
        cig_off[t + 1] = len(cw); seq_off[t + 1] = seq_off[t] + len(sq[-1])
    d = dict(contig=0, ordinal_base=0, pos=np.array([r[0] for r in reads], np.int32), flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8),
             cell=np.array([r[1] for r in reads], np.int32), umi=np.array([(1 << 24) | r[2] for r in reads], np.uint64),
             cig_off=cig_off, cigar=np.array(cw, np.uint32), seq_off=seq_off, seq=np.concatenate(sq))
    return util.batch_from_dict(d)


def _count(names, regions, snps, n_cells, batch, flags=0):
    """-> (snp_counts of a fresh engine fed the batch, the oracle's one-base matrices)"""
    with Engine(BAF, names, regions, n_cells, snps=snps, flags=flags, **FILT) as eng:
        eng.push(batch[0])
        eng.finish()
        got = eng.snp_counts()
    return got, R.oracle_of(names, onebase(snps), n_cells, [batch[0]], FILT, flags)


M91 = [(0, 91)]


def test_run_shapes():
    """All reads are 91M at position 50 and cover the three SNPs, so every SNP's part of the sorted stream is one (SNP, cell) run
    per cell, a molecule per entry, in cell order.  Cells 0..5 have one read per molecule: runs of 1, RUN_WALK, RUN_WALK + 1 (the
    longest a head walks), RUN_WALK + 2 (the shortest that goes to k_snc_long), a filler that ends one entry before the tile does,
    and 5 000 - two long runs back to back, the second beginning on the last entry of tile 0.  Cell 6 has three reads per molecule
    (entries that are no molecule heads inside a run) and is a long run and the last of the stream."""
    sizes = [1, RUN_WALK, RUN_WALK + 1, RUN_WALK + 2]
    sizes += [SNC_TILE - 1 - sum(sizes), 5000]
    assert sizes[4] > RUN_WALK + 1 and sum(sizes[:5]) == SNC_TILE - 1
    reads, u = [], 0
    for cell, m in enumerate(sizes):
        for _ in range(m):
            reads.append((50, cell, u, M91)); u += 1
    for k in range(300 * 3):
        reads.append((50, 6, 100000 + k % 300, M91))
    order = np.random.default_rng(1).permutation(len(reads))            # fetch order is not stream order
    reads = [reads[i] for i in order.tolist()]
    snps = [("1", 100, "A", "C", 0, 1), ("1", 120, "G", "T", 1, 0), ("1", 135, "T", "A", 0, 1)]
    got, exp = _count(["1"], [("1", 1, 500, "g")], snps, 7, _batch(reads, 2))
    _same(got, exp)
    dp = {(r, c): v for r, c, v in zip(*[x.tolist() for x in got["dp"]])}
    oth = {(r, c): v for r, c, v in zip(*[x.tolist() for x in got["oth"]])}
    for s in range(3):                                                   # random bases: a molecule is REF or ALT, or another base
        for cell, m in enumerate(sizes + [300]):
            assert dp.get((s, cell), 0) + oth.get((s, cell), 0) == m


def test_molecules_claimed_by_gap_records_count_nowhere():
    """A read with an N or D gap over the SNPs comes earlier in fetch order than the read that shows a base for the same (cell,
    UMI): the molecule belongs to the gap read and counts in no matrix.  Cell 2 has only such molecules: it appears nowhere, while
    cells 1 and 3 keep their places around it.  Cells 0, 1, 3 and 4 mix claimed molecules, molecules whose base read comes first,
    and molecules without a gap read.  64-bit keys, split path (the default)."""
    rng = np.random.default_rng(7)
    gapN, gapD = [(0, 20), (3, 60), (0, 30)], [(0, 20), (2, 60), (0, 30)]   # 50..69, gap over 70..129, then 30 bases
    reads = []
    for cell in range(5):
        for umi in range(40):
            kind = 0 if cell == 2 else int(rng.integers(0, 3))              # 0 gap read first, 1 base read first, 2 no gap read
            gap = (50, cell, umi, gapN if rng.random() < 0.5 else gapD)
            base = (60, cell, umi, M91)
            reads += [gap, base] if kind == 0 else [base, gap] if kind == 1 else [base, base]
    snps = [("1", 100, "A", "C", 0, 1), ("1", 110, "C", "G", 0, 1), ("1", 120, "G", "T", 0, 1), ("1", 65, "A", "T", 0, 1)]
    got, exp = _count(["1"], [("1", 1, 500, "g")], snps, 5, _batch(reads, 8))
    _same(got, exp)
    for k in R.MATS:
        row, col = got[k][0], got[k][1]
        assert not np.any((col == 2) & (row < 3))                          # only claimed molecules at the SNPs inside the gap
        assert np.any((col == 1) & (row < 3)) and np.any((col == 3) & (row < 3))
    assert np.any((got["dp"][1] == 2) & (got["dp"][0] == 3)) or np.any((got["oth"][1] == 2) & (got["oth"][0] == 3))   # position 65: in front of the gap


def test_alleles_and_what_a_refold_changes():
    """REF == ALT (ALT wins), REF or ALT N, read bases N, bases that are neither; a refold that swaps REF / ALT on some SNPs is
    followed, a SNP mask and other regions are not."""
    rng = np.random.default_rng(3)
    reads = [(int(p), int(c), int(u), M91) for p, c, u in zip(np.sort(rng.integers(0, 400, 3000)), rng.integers(0, 6, 3000), rng.integers(0, 500, 3000))]
    alle = [("A", "A"), ("N", "C"), ("G", "N"), ("N", "N"), ("A", "C"), ("C", "A"), ("T", "G"), ("G", "G")]
    snps = [("1", 95 + 7 * k, alle[k % 8][0], alle[k % 8][1], k & 1, 1 - (k & 1)) for k in range(48)]
    regions = [("1", 1, 300, "a"), ("1", 200, 500, "b")]
    batch = _batch(reads, 4, n_frac=0.1)
    with Engine(BAF, ["1"], regions, 6, snps=snps, **FILT) as eng:
        eng.push(batch[0])
        first = eng.finish()
        got = eng.snp_counts()
        _same(got, R.oracle_of(["1"], onebase(snps), 6, [batch[0]], FILT))
        ad = {(r, c): v for r, c, v in zip(*[x.tolist() for x in got["ad"]])}
        dp = {(r, c): v for r, c, v in zip(*[x.tolist() for x in got["dp"]])}
        for (r, c), v in dp.items():
            if alle[r % 8][0] == alle[r % 8][1]:
                assert ad.get((r, c), 0) == v                               # REF == ALT: every REF / ALT molecule is ALT
        assert len(got["oth"][0]) > 0
        swapped = [(s[0], s[1], s[3], s[2], s[4], s[5]) if k % 3 == 0 else s for k, s in enumerate(snps)]
        eng.refold(regions, snps=swapped)
        got2 = eng.snp_counts()
        _same(got2, R.oracle_of(["1"], onebase(swapped), 6, [batch[0]], FILT))
        assert not np.array_equal(got2["ad"][2], got["ad"][2]) or len(got2["ad"][2]) != len(got["ad"][2])
        mask = np.arange(len(snps)) % 2 == 0
        eng.refold([("1", 50, 60, "elsewhere")], snps=swapped, snp_enabled=mask, min_count=5, min_maf=0.2, no_dup_hap=False)
        _same(eng.snp_counts(), got2)
        _same(eng.refold(regions, snps=snps), first)
        _same(eng.snp_counts(), got)


# ---------------------------------------------------------------------------------------------- 3. order
@pytest.mark.parametrize("n_snps", [SC_TILE + 1, SC_PASS])
def test_rows_are_the_callers_indices(n_snps, monkeypatch):
    """A shuffled SNP list over three contigs with distinct positions, among them SNPs on a contig the handle does not know, at
    positions < 1, and (most of them) where no read is.  The per-row counts are scanned in the caller's order over n_snps + 1
    values by k_scan_reduce / k_scan_top / k_scan_apply: SC_TILE + 1 SNPs need a second tile, and SC_PASS = 1024 * SC_TILE SNPs give
    one value more than one pass of k_scan_top holds.  Expected: the oracle on the SNPs that can be covered, rows mapped back."""
    import xcltk_amd.engine as E
    from xcltk_amd.snptable import SnpTable
    orig = E.snp_array
    monkeypatch.setattr(E, "snp_array", lambda snps, cidx: orig(snps, collections.defaultdict(lambda: -1, cidx)))   # a contig outside the table: -1
    rng = np.random.default_rng(5)
    names, lengths = ["1", "2", "3"], [6000, 6000, 6000]
    chrom = rng.integers(0, 4, n_snps).astype(np.int32)                   # 3 = "zz"
    per = np.zeros(n_snps, np.int64)
    for c in range(4):
        idx = np.flatnonzero(chrom == c)
        per[idx] = rng.permutation(len(idx)) * 3 - 20 + c                 # distinct per contig, in random order; the first ones < 1
    k = np.arange(n_snps)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    table = SnpTable(names + ["zz"], chrom, per, acgt[k % 4], acgt[(k + 1 + k // 4) % 4], np.zeros(n_snps, np.int8), np.ones(n_snps, np.int8))
    from test_gpu_refold import _reads
    batches, keep = _reads(names, lengths, 900, 4, seed=9)
    with Engine(BAF, names, [("1", 1, 100, "seed")], 4, snps=table, **FILT) as eng:
        for b in batches:
            eng.push(b)
        eng.finish()
        got = eng.snp_counts()
    sub = np.flatnonzero((chrom < 3) & (per >= 1) & (per <= 6200))        # what a read can cover, in the caller's order
    small = [(names[chrom[i]], int(per[i]), chr(table.ref[i]), chr(table.alt[i]), 0, 1) for i in sub.tolist()]
    exp = R.oracle_of(names, onebase(small), 4, batches, FILT)
    exp = {m: (sub[exp[m][0]].astype(np.int32), exp[m][1], exp[m][2]) for m in R.MATS}
    _same(got, exp)
    _sorted_by_row_col(got, n_snps)
    assert len(got["dp"][0]) > 1000 and len(np.unique(got["dp"][0])) > 500
    assert np.any(np.diff(got["dp"][0].astype(np.int64)) > 1)              # rows in between stay empty


# ---------------------------------------------------------------------------------------------- 4. state and errors
def _code(fn):
    with pytest.raises(XckError) as ei:
        fn()
    return ei.value.code


def test_state_and_errors():
    """XCK_E_STATE before a finish and after a reset, XCK_E_ARG for a null out and on a basefc handle, a handle without hits, and the
    handle usable after each.  Two answers are NOT exercised here, because neither can be brought about without breaking a fold or
    the allocator on purpose: XCK_E_STATE after a failed fold (fold_failed / !mol_valid, checked first in engine_snp_counts), and
    that running out of memory inside the call leaves the handle unmarked (the call writes only to buffers of its own and never
    sets fold_failed).  Both are covered by reading csrc/snp_counts.h only; so is XCK_E_CAPACITY for a stream of 2^32 hits."""
    from test_gpu_refold import _reads, _snps_every
    names = ["1", "2"]
    snps = _snps_every("1", 60, 30000) + _snps_every("2", 90, 30000)
    regions = [("1", 100 + 700 * g, 600 + 700 * g, "g%d" % g) for g in range(40)]
    batches, keep = _reads(names, [30000, 30000], 800, 6, seed=6)
    exp = R.oracle_of(names, onebase(snps), 6, batches, FILT)
    import ctypes as C
    with Engine(BAF, names, regions, 6, snps=snps, **FILT) as eng:
        assert _code(eng.snp_counts) == capi.XCK_E_STATE                  # before a finish
        for b in batches:
            eng.push(b)
        assert _code(eng.snp_counts) == capi.XCK_E_STATE
        first = eng.finish()
        assert eng.lib.xck_snp_counts(eng.h, None) == capi.XCK_E_ARG      # null out
        _same(eng.snp_counts(), exp)
        _same(eng.finish(), first)
        eng.reset()
        assert _code(eng.snp_counts) == capi.XCK_E_STATE                  # after a reset
        empty = eng.finish()                                              # a handle with no hits
        assert all(len(empty[m][0]) == 0 for m in R.MATS)
        none = eng.snp_counts()
        assert all(len(none[m][j]) == 0 for m in R.MATS for j in range(3))
        eng.reset()
        for b in batches:                                                 # ... and it is usable after each of these
            eng.push(b)
        _same(eng.finish(), first)
        _same(eng.snp_counts(), exp)
    with Engine(capi.XCK_MODE_BASEFC, names, regions, 6, **FILT) as eng:
        for b in batches:
            eng.push(b)
        cnt = eng.finish()
        assert _code(eng.snp_counts) == capi.XCK_E_ARG                    # a basefc handle
        res = capi.Result()
        assert eng.lib.xck_snp_counts(eng.h, C.byref(res)) == capi.XCK_E_ARG
        util.assert_coo_equal(eng.finish(), cnt, ["count"])


# ---------------------------------------------------------------------------------------------- 5. either side of the copy-out threshold
COPY_STREAM_BYTES = 8 << 20               # a result of this many bytes or more crosses on the copy stream, a smaller one is stored by the CUs
THR_SNPS, THR_CELLS, THR_READS = 700, 500, 70
THR_REGIONS = [("1", 1, 7000, "g")]


@functools.lru_cache(maxsize=None)
def threshold_case(n_snps, cells_with_reads=THR_CELLS):
    """A pileup whose SNP x cell matrices are dense: SNPs nine bases apart (REF A, ALT C), and for every cell 0 .. cells_with_reads - 1
    THR_READS 91M reads laid end to end over them (the last base of a read is the first of the next), a UMI each, every base C.  Every
    cell shows ALT at every SNP, so AD and DP hold n_snps * cells_with_reads entries each and OTH none: with THR_CELLS cells,
    THR_SNPS SNPs give 3 * 4 * 2 * 350 000 = 8 400 000 bytes >= 8 MiB = 8 388 608 and four SNPs fewer 8 352 000.
    -> (snps, batch, the oracle's one-base matrices over THR_CELLS columns); made once per size and shared (test_gpu_group_counts.py
    reads it too): nobody writes to it."""
    assert n_snps <= THR_SNPS
    snps = [("1", 101 + 9 * k, "A", "C", 0, 1) for k in range(n_snps)]
    j, cell = (x.ravel() for x in np.meshgrid(np.arange(THR_READS), np.arange(cells_with_reads), indexing="ij"))
    n = len(j)
    d = dict(contig=0, ordinal_base=0, pos=(100 + 90 * j).astype(np.int32), flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8),
             cell=cell.astype(np.int32), umi=((1 << 24) | np.arange(n)).astype(np.uint64), cig_off=np.arange(n + 1, dtype=np.uint32),
             cigar=np.full(n, (91 << 4) | 0, np.uint32), seq_off=(46 * np.arange(n + 1)).astype(np.uint32), seq=np.full(46 * n, 0x22, np.uint8))
    batch = util.batch_from_dict(d)
    exp = R.oracle_of(["1"], onebase(snps), THR_CELLS, [batch[0]], FILT)
    assert len(exp["ad"][0]) == len(exp["dp"][0]) == n_snps * cells_with_reads and len(exp["oth"][0]) == 0
    return snps, batch, {k: exp[k] for k in R.MATS}


def coo_bytes(m):
    """What a derived-matrix call hands to the host: three int32 arrays per matrix."""
    return 3 * 4 * sum(len(m[k][0]) for k in R.MATS)


def _snp_counts_of(eng, batch):
    eng.push(batch[0])
    eng.finish()
    return eng.snp_counts()


@pytest.mark.parametrize("n_snps,large", [(THR_SNPS, True), (THR_SNPS - 4, False)], ids=["copy_stream", "mapped_store"])
def test_result_on_either_side_of_the_copy_out_threshold(n_snps, large):
    snps, batch, exp = threshold_case(n_snps)
    with Engine(BAF, ["1"], THR_REGIONS, THR_CELLS, snps=snps, **FILT) as eng:
        got = _snp_counts_of(eng, batch)
    print("%d SNPs: %d bytes" % (n_snps, coo_bytes(got)))
    if large:
        assert coo_bytes(got) >= COPY_STREAM_BYTES
    else:
        assert coo_bytes(got) < COPY_STREAM_BYTES
    _same(got, exp)
    _sorted_by_row_col(got, n_snps)


def test_a_smaller_result_after_a_larger_one_on_one_handle():
    """small, large, small: the call's buffers only grow, so the third call finds a scratch block, a device block and a pinned block
    sized for the second - and the large result takes the copy stream where its neighbours take the store kernel."""
    snps, big, exp_big = threshold_case(THR_SNPS)
    _, small, exp_small = threshold_case(THR_SNPS, 7)
    with Engine(BAF, ["1"], THR_REGIONS, THR_CELLS, snps=snps, **FILT) as eng:
        for batch, exp, large in ((small, exp_small, False), (big, exp_big, True), (small, exp_small, False)):
            got = _snp_counts_of(eng, batch)
            assert (coo_bytes(got) >= COPY_STREAM_BYTES) == large
            _same(got, exp)
            eng.reset()


# ---------------------------------------------------------------------------------------------- 6. one pass for `xcltk baf`
DS = os.path.join(util.GOLDEN, "datasets", "phasing")


@pytest.mark.parametrize("name,case", __import__("test_genotype")._genotype_cases())
def test_one_pass_pipeline_equals_the_two_pass_pipeline(name, case, tmp_path, monkeypatch):
    """pipeline_wrapper with XCK_BAF_ONE_PASS=1 against the default on the `phasing` dataset, the phased list built as in
    test_gpu_genotype.test_pipeline_steps_1_and_3_with_engine_pileup (the SNPs the pileup VCF of the case lists): the same 1_pileup (raw and filtered; also equal to the
    fixtures the reference's filter made) and the same 3_baf_fc, from one ingest where the default needs two."""
    from test_genotype import GT, assert_cellsnp_dirs_equal
    from xcltk_amd.baf.pipeline import pipeline_wrapper
    from xcltk_amd.utils import csp_io
    covered = set(csp_io.load_data(os.path.join(GT, name)).pos.tolist())  # the phased list derives from the filtered pileup VCF: the SNPs it keeps
    lines = open(os.path.join(DS, "snps.tsv")).read().splitlines()
    snp_fn = str(tmp_path / "phased.tsv")
    open(snp_fn, "w").write("\n".join([lines[0]] + [l for l in lines[1:] if int(l.split("\t")[1]) in covered]) + "\n")
    ingests = []
    for fn in ("ingest_bam", "ingest_bams"):
        def counted(self, *a, _orig=getattr(Engine, fn), _fn=fn, **k):
            ingests.append(_fn)
            return _orig(self, *a, **k)
        monkeypatch.setattr(Engine, fn, counted)
    for k in ("XCK_READ_FATE", "XCK_CELL_SUMMARY", "XCK_FEATURE_SUMMARY", "WORLD_SIZE", "XCK_DIST_FORCE"):
        monkeypatch.delenv(k, raising=False)
    outs, n_ingests = {}, {}
    for how in ("two", "one"):
        if how == "one":
            monkeypatch.setenv("XCK_BAF_ONE_PASS", "1")
        else:
            monkeypatch.delenv("XCK_BAF_ONE_PASS", raising=False)
        del ingests[:]
        outs[how] = str(tmp_path / how)
        ret = pipeline_wrapper("smp", sam_fn=os.path.join(DS, "possorted.bam"), barcode_fn=os.path.join(DS, "barcodes.tsv"),
                               snp_vcf_fn=os.path.join(DS, "cellsnp", "cellSNP.base.vcf.gz"), region_fn=os.path.join(DS, "regions.tsv"),
                               out_dir=outs[how], phased_snp_fn=snp_fn, ref_cell_fn=os.path.join(DS, "ref_cells.tsv"),
                               min_count=case["min_count"], min_maf=case["min_maf"], ncores=2)
        assert ret == 0
        n_ingests[how] = len(ingests)
    assert n_ingests == {"two": 2, "one": 1}
    p1, p2 = os.path.join(outs["one"], "1_pileup"), os.path.join(outs["two"], "1_pileup")
    assert_cellsnp_dirs_equal(os.path.join(p1, "raw"), os.path.join(p2, "raw"))
    assert_cellsnp_dirs_equal(p1, p2)
    assert_cellsnp_dirs_equal(os.path.join(p1, "raw"), os.path.join(GT, "raw"))
    assert_cellsnp_dirs_equal(p1, os.path.join(GT, name))
    util.assert_dirs_equal(os.path.join(outs["one"], "3_baf_fc"), os.path.join(outs["two"], "3_baf_fc"))
    assert os.path.getsize(os.path.join(outs["one"], "3_baf_fc", "xcltk.DP.mtx")) > 200
