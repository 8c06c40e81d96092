"""xck_refold / Engine.refold / afc_variants: the pileup recounted under new regions, phasing and filters without the reads.
Every test calls one of the three, so none passes without the feature."""
import os

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


# ---------------------------------------------------------------------------------------------- 1. reference-pinned, front-end
COMMON_KEYS = ("sam_fn", "barcode_fn", "phased_snp_fn")
DATASETS = {
    "dense": ["dense_baf_default", "dense_baf_filters", "dense_baf_allreg_dup"],
    "phasing": ["phasing_baf_off", "phasing_baf_allreg", "phasing_baf_refcells", "phasing_baf_short_pileup", "phasing_baf_surplus_pileup"],
}


@pytest.mark.parametrize("dataset", sorted(DATASETS))
def test_variants_front_end_matches_the_reference_outputs(dataset, tmp_path):
    """One afc_variants call per order; every directory byte for byte what the unmodified reference wrote.  All variants of a
    dataset have the same number of regions, so the first of the list makes the engine and comes from finish(): two orders with
    different heads, and every case has also come from refold()."""
    from xcltk_amd.baf.fc.variants import afc_variants
    names = DATASETS[dataset]
    for rot in (0, 1, len(names) - 1):
        order = names[rot:] + names[:rot]
        sub = tmp_path / ("rot%d" % rot)
        sub.mkdir()
        common, variants, expected = None, [], []
        for name in order:
            case, ddir, odir, exp = util.load_case(name, sub)
            kw = dict(case["kwargs"])
            c = {k: kw.pop(k) for k in COMMON_KEYS}
            assert common is None or c == common                     # they share reads, cells and the SNP universe
            common = c
            variants.append(kw); expected.append((odir, exp))
        assert afc_variants(common, variants) == 0
        for odir, exp in expected:
            util.assert_dirs_equal(odir, exp)


# ---------------------------------------------------------------------------------------------- 2. kernel level
def _span(regions, snps):
    return max([r[2] for r in regions] + [s[1] for s in snps] + [400])


def _dense_case(seed):
    """A SNP every 3 bp: ~30 hits with a base per read overrun the first capacity guess (1.25 keys per read) of the pileup streams."""
    from test_gpu_parity import _dense_pileup_case
    regions, snps, names, batches = _dense_pileup_case(seed=seed, n_reads=20000, n_cells=20, n_umis=500, snp_step=3, span=60000, max_batch=20000, gap_max=900)
    opts = dict(min_mapq=20, min_len=10, incl_flag=0, excl_flag=772, no_orphan=True, min_count=1, min_maf=0, no_dup_hap=True)
    return names, regions, snps, 20, batches, dict(opts, min_include=0.9), opts, 0


def _roundtrip(seed, flags=0, mode=BAF, case=None):
    """finish under A == oracle(A); refold to B == oracle(B) == fresh handle(B); refold back to A == the first finish."""
    names, regions, snps, n_cells, raw, fc, baf, case_flags = case or fuzz_cases.make_case(seed, many_cells=False, long=False)
    batches = [b for b, _ in raw]                                    # (raw keeps the arrays alive)
    flags |= case_flags
    rf = {k: baf[k] for k in READ_FILTER_KEYS}
    a = R.variant(regions, snps, min_count=baf["min_count"], min_maf=baf["min_maf"], no_dup_hap=baf["no_dup_hap"])
    b = R.random_variant(np.random.default_rng(1000 + seed), names, regions, snps, _span(regions, snps))
    eng = R.fresh_engine(names, a, n_cells, rf, flags, mode=mode, **(dict(min_include=fc["min_include"]) if mode != BAF else {}))
    try:
        for bt in batches:
            eng.push(bt)
        r_a = eng.finish()
        util.assert_coo_equal(r_a, R.oracle_of(names, a, n_cells, batches, rf, flags), R.MATS)
        r_b = R.refold(eng, b)
        util.assert_coo_equal(r_b, R.oracle_of(names, b, n_cells, batches, rf, flags), R.MATS)
        util.assert_coo_equal(r_b, R.fresh_result(names, b, n_cells, batches, rf, flags), R.MATS)
        r_a2 = R.refold(eng, a)
        util.assert_coo_equal(r_a2, r_a, R.MATS)
        if mode != BAF:                                              # the count matrix is the finish's, untouched
            util.assert_coo_equal(r_b, r_a, ["count"]); util.assert_coo_equal(r_a2, r_a, ["count"])
        if case is not None:                                         # (a dense case: both results hold entries, and not the same ones)
            assert len(r_a["dp"][0]) > 0 and len(r_b["dp"][0]) > 0 and not np.array_equal(r_a["dp"][2], r_b["dp"][2])
        print("seed %d: nnz(dp) A %d, B %d" % (seed, len(r_a["dp"][0]), len(r_b["dp"][0])))
        return eng.stats()
    finally:
        eng.close()


@pytest.mark.parametrize("seed", [11, 12, 13, 14, 15, 16, 17, 18, 19, 20])
def test_refold_matches_oracle_and_fresh_handle(seed):
    _roundtrip(seed)


@pytest.mark.parametrize("seed", [21, 22])
@pytest.mark.parametrize("knob", ["radix", "key128", "hap_sorted", "hap_values", "fold_c", "hit_cap0", "both"])
def test_refold_on_every_fold_path(seed, knob, monkeypatch):
    env = {"radix": ("XCK_PILEUP_SORT", "radix"), "hap_sorted": ("XCK_PILEUP_HAP", "sorted"), "hap_values": ("XCK_PILEUP_HAP", "values"),
           "fold_c": ("XCK_FOLD_C", "64"), "hit_cap0": ("XCK_HIT_CAP0", "64")}
    if knob in env:
        monkeypatch.setenv(*env[knob])                               # (a handle reads its knobs at xck_create)
    if knob == "hit_cap0":
        monkeypatch.setenv("XCK_HIT_SLACK", "0")                     # the first launch overflows and is replayed
    st = _roundtrip(seed, flags=capi.XCK_F_FORCE_KEY128 if knob == "key128" else 0, mode=capi.XCK_MODE_BOTH if knob == "both" else BAF,
                    case=_dense_case(seed) if knob == "hit_cap0" else None)
    if knob == "hit_cap0":
        assert st["n_join_launches"] > 1                             # the launch was replayed: the hits went through an overflow
    if knob == "radix":
        assert st["pileup_sort_path"] in (0, 2)
    if knob == "key128":
        assert st["key_bits"] == 128


# ---------------------------------------------------------------------------------------------- 3. table builder shapes
FILT = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True)


def _reads(names, lengths, n_reads, n_cells, seed):
    """A few hundred 91M reads spread over the contigs, as one batch per contig."""
    rng = np.random.default_rng(seed)
    out, ordinal = [], 0
    for ci, ln in enumerate(lengths):
        n = n_reads // len(lengths)
        pos = np.sort(rng.integers(0, max(ln - 100, 1), n)).astype(np.int32)
        nb = 46
        seq = (1 << rng.integers(0, 4, (n * nb, 2))).astype(np.uint8)
        d = dict(contig=ci, ordinal_base=ordinal, pos=pos, flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8),
                 cell=rng.integers(0, n_cells, n).astype(np.int32), umi=((1 << 24) | rng.integers(0, 4096, n)).astype(np.uint64),
                 cig_off=np.arange(n + 1, dtype=np.uint32), cigar=np.full(n, (91 << 4) | 0, np.uint32),
                 seq_off=(np.arange(n + 1) * nb).astype(np.uint32), seq=(seq[:, 0] << 4) | seq[:, 1])
        out.append(util.batch_from_dict(d)); ordinal += n
    return [b for b, _ in out], out


def _snps_every(name, step, hi, lo=10):
    return [(name, p, "ACGT"[k % 4], "ACGT"[(k + 1) % 4], k & 1, 1 - (k & 1)) for k, p in enumerate(range(lo, hi, step))]


def _shape_case(shape):
    """-> names the handle knows, regions / SNPs it is created with, the variant to refold to, contig lengths, unknown contig name"""
    if shape == "fanout":                                            # (a) SNPs in 0, 1, 64, 65 and 300 regions
        snps = _snps_every("1", 100, 50000)
        reg = [("1", 1000, 1999, "one")]
        reg += [("1", 5000 - g, 6000 + g, "n64_%d" % g) for g in range(64)]                   # nested: 64 around 5000..6000
        reg += [("1", 10000 - g, 11000 + g, "n65_%d" % g) for g in range(65)]
        reg += [("1", 20000, 20500, "same")] * 300                                             # one region listed 300 times
        return ["1"], [("1", 1, 100, "seed")], snps, R.variant(reg, snps), [50000], None
    if shape == "edges":                                             # (b) SNPs exactly at start and at end; odd regions
        snps = _snps_every("1", 50, 20000)                                                     # positions 10, 60, 110, ...
        reg = [("1", 110, 160, "both_ends"), ("1", 161, 209, "none_inside"), ("1", 210, 210, "one_base"), ("1", 900, 100, "inverted"),
               ("1", 0, 60, "starts_at_0"), ("1", -5, 10, "starts_below_0"), ("zz", 1, 20000, "unknown_contig"), ("1", 19000, 40000, "past_the_end")]
        return ["1"], [("1", 1, 100, "seed")] * 8, snps, R.variant(reg, snps), [20000], "zz"
    if shape == "spanning":                                          # (c) 3 000 short regions behind one that spans the contig
        snps = _snps_every("1", 40, 120000)
        reg = [("1", 1, 120000, "whole")] + [("1", 30 + 40 * g, 30 + 40 * g + 25, "s%d" % g) for g in range(3000)]
        return ["1"], [("1", 1, 100, "seed")] * 3001, snps, R.variant(reg, snps), [120000], None
    if shape == "contigs":                                           # (d) a contig with SNPs and no regions, one with regions and no SNPs
        snps = _snps_every("1", 70, 30000) + _snps_every("2", 70, 30000)
        reg = [("1", 100 + 500 * g, 400 + 500 * g, "a%d" % g) for g in range(40)] + [("3", 100 + 500 * g, 400 + 500 * g, "c%d" % g) for g in range(40)]
        return ["1", "2", "3"], [("2", 1, 30000, "seed"), ("3", 5, 50, "seed3")] * 40, snps, R.variant(reg, snps), [30000, 30000, 30000], None
    raise KeyError(shape)


@pytest.mark.parametrize("shape", ["fanout", "edges", "spanning", "contigs"])
def test_table_builder_shapes(shape):
    names, regions0, snps, v, lengths, unknown = _shape_case(shape)
    batches, keep = _reads(names, lengths, 600, 5, seed=3)
    eng = Engine(BAF, names, regions0, 5, snps=snps, flags=capi.XCK_F_FEATURE_SUMMARY, **FILT)
    try:
        for b in batches:
            eng.push(b)
        eng.finish()
        got = R.refold(eng, v)
        exp = R.oracle_of(names, v, 5, batches, FILT, unknown_contig=unknown)
        util.assert_coo_equal(got, exp, R.MATS)
        assert len(got["dp"][0]) > 0
        fs = eng.feature_summary()
        per_snp, per_reg = R.brute_force_membership(names, v)
        assert np.array_equal(fs["snp"][:, capi.SNP_COLS.index("regions")], per_snp)
        assert np.array_equal(fs["matrix"][:, 0], per_reg)
        if shape == "fanout":
            assert {0, 1, 64, 65, 300} <= set(per_snp.tolist())
        if shape == "edges":
            assert per_reg.tolist() == [2, 0, 1, 0, 2, 1, 0, 20]
    finally:
        eng.close()


def test_no_regions_gives_three_empty_matrices():
    """(e)"""
    snps = _snps_every("1", 100, 20000)
    batches, keep = _reads(["1"], [20000], 300, 3, seed=4)
    with Engine(BAF, ["1"], [("1", 1, 20000, "all")], 3, snps=snps, **FILT) as eng:
        for b in batches:
            eng.push(b)
        first = eng.finish()
        assert len(first["dp"][0]) > 0
        got = eng.refold([])
        assert all(len(got[m][j]) == 0 for m in R.MATS for j in range(3))
        util.assert_coo_equal(eng.refold([("1", 1, 20000, "all")]), first, R.MATS)


def test_one_more_snp_than_one_pass_of_the_scan():
    """(f) The builder's device-wide scan (k_scan_reduce / k_scan_top / k_scan_apply of fold_partition.h) scans csr_off's n_snps + 1
    counts in tiles of SC_TILE = 256 * 16 = 4096 elements, and k_scan_top walks the tiles' sums 1024 at a time: one pass of it covers
    1024 * 4096 = 4 194 304 counts.  4 194 304 SNPs give one count more.  The SNPs are 2 apart, so most lie far behind the reads;
    the regions per SNP and SNPs per region are compared with their closed forms, the matrices with a fresh handle."""
    n = 1024 * 4096
    pos = np.arange(n, dtype=np.int64) * 2 + 10
    from xcltk_amd.snptable import SnpTable
    k = np.arange(n)
    snps = SnpTable(["1"], np.zeros(n, np.int32), pos, np.frombuffer(b"ACGT", np.uint8)[k % 4], np.frombuffer(b"ACGT", np.uint8)[(k + 1) % 4], k & 1, 1 - (k & 1))
    last = int(pos[-1])
    reg_a = [("1", 1, 5000, "head")]
    reg_b = [("1", 1, 5000, "head"), ("1", 3000, last, "tail"), ("1", last, last, "last_snp"), ("1", 4096 * 2 + 10, 4096 * 2 + 10, "tile_edge")]
    batches, keep = _reads(["1"], [6000], 400, 3, seed=5)
    with Engine(BAF, ["1"], reg_a, 3, snps=snps, flags=capi.XCK_F_FEATURE_SUMMARY, **FILT) as eng:
        for b in batches:
            eng.push(b)
        eng.finish()
        got = eng.refold(reg_b)
        fs = eng.feature_summary()
    per_snp = (pos <= 5000).astype(np.int64) + (pos >= 3000) + (pos == last) + (pos == 4096 * 2 + 10)
    assert np.array_equal(fs["snp"][:, capi.SNP_COLS.index("regions")], per_snp)
    assert fs["matrix"][:, 0].tolist() == [int((pos <= 5000).sum()), int((pos >= 3000).sum()), 1, 1]
    with Engine(BAF, ["1"], reg_b, 3, snps=snps, **FILT) as eng:
        for b in batches:
            eng.push(b)
        util.assert_coo_equal(got, eng.finish(), R.MATS)
    assert len(got["dp"][0]) > 0 and set(got["dp"][0].tolist()) <= {0, 1}


# ---------------------------------------------------------------------------------------------- 4. state and errors
@pytest.fixture(scope="module")
def small():
    names = ["1", "2"]
    snps = _snps_every("1", 60, 30000) + _snps_every("2", 90, 30000)
    regions = [("1", 100 + 700 * g, 600 + 700 * g, "g%d" % g) for g in range(40)] + [("2", 1, 30000, "all2")]
    batches, keep = _reads(names, [30000, 30000], 800, 6, seed=6)
    return names, regions, snps, batches, keep


def _code(fn):
    with pytest.raises(XckError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_refold_state_errors(small):
    names, regions, snps, batches, keep = small
    with Engine(BAF, names, regions, 6, snps=snps, **FILT) as eng:
        assert _code(lambda: eng.refold(regions))[0] == capi.XCK_E_STATE          # before a finish
        for b in batches:
            eng.push(b)
        assert _code(lambda: eng.refold(regions))[0] == capi.XCK_E_STATE
        first = eng.finish()
        util.assert_coo_equal(eng.refold(regions), first, R.MATS)
        eng.reset()
        assert _code(lambda: eng.refold(regions))[0] == capi.XCK_E_STATE          # after a reset
    with Engine(capi.XCK_MODE_BASEFC, names, regions, 6, **FILT) as eng:
        for b in batches:
            eng.push(b)
        eng.finish()
        res, cfg = capi.Result(), capi.RefoldConfig()
        import ctypes as C
        cfg.struct_size = C.sizeof(capi.RefoldConfig)
        assert eng.lib.xck_refold(eng.h, C.byref(cfg), C.byref(res)) == capi.XCK_E_ARG    # a basefc handle


def test_refold_argument_errors_leave_the_handle_usable(small):
    names, regions, snps, batches, keep = small
    with Engine(BAF, names, regions, 6, snps=snps, **FILT) as eng:
        for b in batches:
            eng.push(b)
        first = eng.finish()
        moved = list(snps); moved[7] = (moved[7][0], moved[7][1] + 1) + tuple(moved[7][2:])
        assert _code(lambda: eng.refold(regions, snps=moved))[0] == capi.XCK_E_ARG
        assert _code(lambda: eng.refold(regions, snps=snps[:-1]))[0] == capi.XCK_E_ARG
        # the row field was sized from max(41 regions, 834 SNPs) + 1 -> 10 bits: 1023 regions fit, 1024 do not
        assert len(snps) == 834
        code, msg = _code(lambda: eng.refold([("1", 1, 50, "x")] * 1024))
        assert code == capi.XCK_E_ARG and "1023" in msg and "row field" in msg
        assert _code(lambda: eng.refold(regions, excl_pairs=([len(regions)], [0])))[0] == capi.XCK_E_ARG
        assert _code(lambda: eng.refold(regions, excl_pairs=([0], [len(snps)])))[0] == capi.XCK_E_ARG
        util.assert_coo_equal(eng.refold(regions), first, R.MATS)                 # as it was
        v = R.variant([("1", 1, 30000, "all1")] + [("1", 1, 50, "x")] * 1022, snps)                       # 1023 regions fit
        util.assert_coo_equal(R.refold(eng, v), R.oracle_of(names, v, 6, batches, FILT), R.MATS)


def test_summaries_and_device_result_follow_the_refold(small):
    import torch
    from xcltk_amd import shard
    names, regions, snps, batches, keep = small
    flags = capi.XCK_F_FEATURE_SUMMARY | capi.XCK_F_CELL_SUMMARY
    b = R.random_variant(np.random.default_rng(77), names, regions, snps, 30000)
    with Engine(BAF, names, regions, 6, snps=snps, flags=flags, **FILT) as eng:
        for bt in batches:
            eng.push(bt)
        eng.finish()
        fs_a, cs_a = eng.feature_summary(), eng.cell_summary()
        got = R.refold(eng, b)
        fs, cs = eng.feature_summary(), eng.cell_summary()
        dev = eng.result_device()
        for m in R.MATS:                                                          # xck_get_result_device: the refolded blocks
            ptr, nnz = dev[m]
            assert nnz == len(got[m][0])
            if nnz:
                blk = torch.as_tensor(shard._DevArray(ptr, 3 * nnz), device="cuda:0").cpu().numpy()
                assert np.array_equal(blk, np.concatenate(got[m]))
    with R.fresh_engine(names, b, 6, FILT, flags) as eng:
        for bt in batches:
            eng.push(bt)
        exp = eng.finish()
        fs_f, cs_f = eng.feature_summary(), eng.cell_summary()
    util.assert_coo_equal(got, exp, R.MATS)
    assert np.array_equal(fs["matrix"], fs_f["matrix"]) and not np.array_equal(fs["matrix"].shape, fs_a["matrix"].shape)
    assert np.array_equal(cs["matrix"], cs_f["matrix"])
    assert np.array_equal(cs["fate"], cs_a["fate"])                               # the read side does not change
    en = b["enabled"]
    kept, nreg = capi.SNP_COLS.index("kept"), capi.SNP_COLS.index("regions")
    assert np.array_equal(fs["snp"][en][:, [kept, nreg]], fs_f["snp"][:, [kept, nreg]])
    assert np.array_equal(fs["snp"][en][:, :6], fs_f["snp"][:, :6])               # reads and tallies
    assert not fs["snp"][~en][:, nreg].any()                                      # a disabled SNP feeds no region
    assert np.array_equal(fs["snp"][:, :6], fs_a["snp"][:, :6])
