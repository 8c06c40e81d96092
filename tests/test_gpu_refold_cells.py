"""xck_refold with a cell mask / Engine.refold(cell_enabled=...) / afc_variants with a cell list per variant: the pileup recounted
for a subset of the cells without the reads.  Every case compares three ways - the masked refold, the C oracle and a fresh handle,
the last two fed the same batches with cell = -1 written in for the disabled cells - so none passes without the feature."""
import os

import numpy as np
import pytest

import fuzz_cases
import refold_cells_cases as K
import refold_util as R
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine

pytestmark = pytest.mark.gpu
BAF = capi.XCK_MODE_BAF
READ_FILTER_KEYS = ("min_mapq", "min_len", "incl_flag", "excl_flag", "no_orphan")
KEPT, TALLY = capi.SNP_COLS.index("kept"), slice(1, 6)


def _three_way(eng, names, v, n_cells, raw, rf, mask, flags=0):
    """masked refold == oracle == fresh handle; -> the refold's result"""
    got = eng.refold(v["regions"], snps=v["snps"], snp_enabled=v["enabled"], excl_pairs=v["excl"], cell_enabled=mask, **R.filters_of(v))
    held = K.mask_batches(raw, mask) if mask is not None else raw      # (the holders keep the edited cell arrays alive)
    edited = [b for b, _ in held]
    util.assert_coo_equal(got, R.oracle_of(names, v, n_cells, edited, rf, flags), R.MATS)
    util.assert_coo_equal(got, R.fresh_result(names, v, n_cells, edited, rf, flags), R.MATS)
    del held
    if mask is not None:                                              # a disabled cell simply has no entries
        assert all(np.asarray(mask, dtype=bool)[got[m][1]].all() for m in R.MATS)
    return got


def _pushed(names, v, n_cells, raw, rf, flags=0):
    eng = R.fresh_engine(names, v, n_cells, rf, flags)
    for b, _ in raw:
        eng.push(b)
    return eng


# ---------------------------------------------------------------------------------------------- 1. the word edges of the bit table
@pytest.mark.parametrize("n_cells", [1, 31, 32, 33, 64, 65])
def test_masks_at_the_word_edges_of_the_bit_table(n_cells):
    names, regions, snps, raw = K.spread_case(n_cells)
    v = R.variant(regions, snps)
    first = np.zeros(n_cells, bool); first[0] = True
    last = np.zeros(n_cells, bool); last[-1] = True
    even = np.arange(n_cells) % 2 == 0
    masks = {m.tobytes(): m for m in (first, last, even, ~even)}      # (one cell: these are two masks, all-ones and all-zeros)
    eng = _pushed(names, v, n_cells, raw, K.FILT)
    try:
        eng.finish()
        n_nonempty = 0
        for m in masks.values():
            got = _three_way(eng, names, v, n_cells, raw, K.FILT, m)
            n_nonempty += len(got["dp"][0]) > 0
        assert n_nonempty >= (1 if n_cells == 1 else 3)
    finally:
        eng.close()


def test_a_bit_table_larger_than_its_lds_copy():
    """Up to CM_LDS_WORDS = 4096 words (131072 cells) the tally kernels copy the table to LDS; one word more and they read it where it
    lies.  Masks: a random half, and only the cells of the words past the LDS size."""
    n_cells = 4096 * 32 + 33
    names, regions, snps, raw = K.spread_case(n_cells, n_reads=1200)
    cell = raw[0][1][3]
    cell[:40] = n_cells - 1; cell[40:80] = 4096 * 32; cell[80:120] = 4096 * 32 - 1      # (both sides of the last full word, and the last cell)
    v = R.variant(regions, snps)
    eng = _pushed(names, v, n_cells, raw, K.FILT)
    try:
        eng.finish()
        half = np.random.default_rng(2).random(n_cells) < 0.5
        half[n_cells - 1], half[4096 * 32 - 1] = True, False
        assert len(_three_way(eng, names, v, n_cells, raw, K.FILT, half)["dp"][0]) > 0
        tail = np.arange(n_cells) >= 4096 * 32
        got = _three_way(eng, names, v, n_cells, raw, K.FILT, tail)
        assert {4096 * 32, n_cells - 1} <= set(got["dp"][1].tolist()) and got["dp"][1].min() >= 4096 * 32
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 2. deep SNPs, verdict flips, gap records
@pytest.fixture(scope="module")
def deep():
    return K.deep_case()


def _deep_run(deep, flags=0):
    """finish, then the masked refold of the deep case three ways; -> (SNP table over all cells, under the mask, both results)"""
    names, regions, snps, raw, mask, idx, _ = deep
    v = R.variant(regions, snps, min_count=K.DEEP_MIN_COUNT, min_maf=K.DEEP_MIN_MAF)
    eng = _pushed(names, v, K.DEEP_CELLS, raw, K.FILT, flags | capi.XCK_F_FEATURE_SUMMARY)
    try:
        full = eng.finish()
        util.assert_coo_equal(full, R.oracle_of(names, v, K.DEEP_CELLS, [b for b, _ in raw], K.FILT, flags), R.MATS)
        fs_all = eng.feature_summary()["snp"].copy()
        got = _three_way(eng, names, v, K.DEEP_CELLS, raw, K.FILT, mask, flags)
        fs_m = eng.feature_summary()["snp"].copy()
        st = eng.stats()
    finally:
        eng.close()
    return fs_all, fs_m, full, got, st


def test_deep_snps_verdict_flips_and_gap_claims(deep):
    names, regions, snps, raw, mask, idx, _ = deep
    fs_all, fs_m, full, got, _ = _deep_run(deep)
    # the case is what it says: SNPs of exactly TALLY_LONG, TALLY_LONG + 1 and TALLY_PIECE + 1 molecules over all cells
    for name, depth in (("d2048", 2048), ("d2049", 2049), ("d4097", 4097)):
        assert fs_all[idx[name], TALLY].sum() == depth
        assert 0 < fs_m[idx[name], TALLY].sum() < depth
    # the tallies under the mask are those of the enabled cells' molecules (K.expected_tally: counted on the host from the reads)
    for name, s in idx.items():
        assert fs_m[s, TALLY].tolist() == K.expected_tally(deep, name, mask).tolist(), name
        assert fs_all[s, TALLY].tolist() == K.expected_tally(deep, name, None).tolist(), name
    # min_count: kept over all cells, dropped under the mask; min_maf: the minor allele lives in the enabled cells
    assert fs_all[idx["count_flip"], KEPT] == 1 and fs_m[idx["count_flip"], KEPT] == 0
    assert fs_all[idx["maf_flip"], KEPT] == 0 and fs_m[idx["maf_flip"], KEPT] == 1
    rows_all, rows_m = set(full["dp"][0].tolist()), set(got["dp"][0].tolist())
    assert idx["count_flip"] in rows_all and idx["count_flip"] not in rows_m      # (region g = the one around SNP g)
    assert idx["maf_flip"] not in rows_all and idx["maf_flip"] in rows_m
    # gap records: one claims a molecule of an enabled cell, one of a disabled cell - both are gone over all cells, one under the mask
    assert fs_all[idx["gap"], TALLY].sum() == K.GAP_MOLECULES - 2
    assert fs_m[idx["gap"], TALLY].sum() == K.GAP_MOLECULES // 2 - 1


@pytest.mark.parametrize("knob", ["radix", "hap_sorted", "hap_values", "key128", "fold_c"])
def test_masked_refold_on_every_fold_path(deep, knob, monkeypatch):
    env = {"radix": ("XCK_PILEUP_SORT", "radix"), "hap_sorted": ("XCK_PILEUP_HAP", "sorted"), "hap_values": ("XCK_PILEUP_HAP", "values"),
           "fold_c": ("XCK_FOLD_C", "64")}
    if knob in env:
        monkeypatch.setenv(*env[knob])                               # (a handle reads its knobs at xck_create)
    fs_all, fs_m, full, got, st = _deep_run(deep, capi.XCK_F_FORCE_KEY128 if knob == "key128" else 0)
    names, regions, snps, raw, mask, idx, _ = deep
    assert fs_m[idx["d4097"], TALLY].tolist() == K.expected_tally(deep, "d4097", mask).tolist()
    if knob == "radix":
        assert st["pileup_sort_path"] in (0, 2)                      # the sorted stream lives in d_keys
    if knob == "key128":
        assert st["key_bits"] == 128


@pytest.mark.parametrize("seed", [31, 32, 33])
@pytest.mark.parametrize("key128", [False, True])
def test_masked_refold_of_fuzz_cases_with_other_tables(seed, key128):
    """A random mask together with snp_enabled, new regions, other alleles, exclusion pairs and filters."""
    names, regions, snps, n_cells, raw, fc, baf, case_flags = fuzz_cases.make_case(seed, many_cells=False, long=False)
    flags = case_flags | (capi.XCK_F_FORCE_KEY128 if key128 else 0)
    rf = {k: baf[k] for k in READ_FILTER_KEYS}
    rng = np.random.default_rng(500 + seed)
    a = R.variant(regions, snps, min_count=baf["min_count"], min_maf=baf["min_maf"], no_dup_hap=baf["no_dup_hap"])
    b = R.random_variant(rng, names, regions, snps, max([r[2] for r in regions] + [s[1] for s in snps] + [400]))
    eng = _pushed(names, a, n_cells, raw, rf, flags)
    try:
        eng.finish()
        _three_way(eng, names, a, n_cells, raw, rf, rng.random(n_cells) < 0.5, flags)
        _three_way(eng, names, b, n_cells, raw, rf, rng.random(n_cells) < 0.7, flags)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 3. sequences on one handle
def test_sequences_of_masked_and_unmasked_calls_on_one_handle(deep):
    names, regions, snps, raw, mask, idx, _ = deep
    n = K.DEEP_CELLS
    v = R.variant(regions, snps, min_count=K.DEEP_MIN_COUNT, min_maf=K.DEEP_MIN_MAF)
    rng = np.random.default_rng(9)
    other = rng.random(n) < 0.3
    b = R.random_variant(rng, names, regions, snps, K.DEEP_SPAN)
    eng = _pushed(names, v, n, raw, K.FILT, capi.XCK_F_FEATURE_SUMMARY)
    try:
        first = eng.finish()
        sc_all = eng.snp_counts()
        fs_all = eng.feature_summary()["snp"].copy()
        masked = _three_way(eng, names, v, n, raw, K.FILT, mask)
        assert not np.array_equal(masked["dp"][2], first["dp"][2])
        # snp_counts() keeps answering for every cell
        util.assert_coo_equal(eng.snp_counts(), sc_all, R.MATS)
        # group_counts() sums the masked matrices: every cell its own group gives them back
        util.assert_coo_equal(eng.group_counts(np.arange(n, dtype=np.int32), n_groups=n), masked, R.MATS)
        one = eng.group_counts(np.zeros(n, dtype=np.int32), n_groups=1)
        for m in R.MATS:
            assert int(one[m][2].sum()) == int(masked[m][2].sum())
        # the mask belongs to the call: without one every cell counts again, tallies and verdicts included
        util.assert_coo_equal(R.refold(eng, v), first, R.MATS)
        assert np.array_equal(eng.feature_summary()["snp"], fs_all)
        _three_way(eng, names, v, n, raw, K.FILT, other)                                  # another mask
        _three_way(eng, names, b, n, raw, K.FILT, mask)                                   # with snp_enabled, new regions, other filters
        # all-ones == NULL == the plain refold
        util.assert_coo_equal(eng.refold(regions, snps=snps, cell_enabled=np.ones(n, bool), **R.filters_of(v)), first, R.MATS)
        assert np.array_equal(eng.feature_summary()["snp"], fs_all)
        # all-zeros: XCK_OK and three empty matrices; the tallies are zero, and the handle goes on
        empty = eng.refold(regions, snps=snps, cell_enabled=np.zeros(n, bool), **R.filters_of(v))
        assert all(len(empty[m][j]) == 0 for m in R.MATS for j in range(3))
        assert not eng.feature_summary()["snp"][:, TALLY].any()
        util.assert_coo_equal(eng.refold(regions, snps=snps, cell_enabled=mask, **R.filters_of(v)), masked, R.MATS)
        with pytest.raises(ValueError):
            eng.refold(regions, cell_enabled=np.ones(n + 1, bool))
        util.assert_coo_equal(R.refold(eng, v), first, R.MATS)
    finally:
        eng.close()


def test_masked_refold_of_a_handle_without_hits():
    names, regions, snps, raw = K.spread_case(5)
    with Engine(BAF, names, regions, 5, snps=snps, **K.FILT) as eng:
        eng.finish()
        got = eng.refold(regions, cell_enabled=[True, False, True, False, True])
        assert all(len(got[m][j]) == 0 for m in R.MATS for j in range(3))


# ---------------------------------------------------------------------------------------------- 4. front-end
CASES = {"dense": "dense_baf_default", "phasing": "phasing_baf_off"}


@pytest.mark.parametrize("dataset", sorted(CASES))
def test_afc_variants_with_cell_lists_of_their_own(dataset, tmp_path, monkeypatch):
    """One pass over the BAM for three directories: the full list (== the reference's recorded files) and two subsets, each byte for
    byte what afc_wrapper writes when the subset is its barcode file."""
    from xcltk_amd import fc_common as fcc
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.baf.fc.variants import afc_variants
    case, ddir, odir, exp = util.load_case(CASES[dataset], tmp_path)
    kw = dict(case["kwargs"])
    with open(kw["barcode_fn"]) as fp:
        cells = [x.strip() for x in fp if x.strip()]
    rng = np.random.default_rng(3)
    subsets = {"odd": cells[1::2], "few": [cells[i] for i in rng.permutation(len(cells))[:len(cells) // 4]]}   # (the second in file order != sorted order)
    files = {}
    for name, sub in subsets.items():
        files[name] = str(tmp_path / ("barcodes_%s.tsv" % name))
        with open(files[name], "w") as fp:
            fp.write("".join(c + "\n" for c in sub))
    common = {k: kw[k] for k in ("sam_fn", "barcode_fn", "phased_snp_fn")}
    rest = {k: v for k, v in kw.items() if k not in common and k != "out_dir"}
    variants = [dict(rest, out_dir=str(tmp_path / ("var_" + name)), barcode_fn=files[name], min_count=mc) for name, mc in (("odd", 3), ("few", 2))]
    variants.insert(1, dict(rest, out_dir=odir))
    passes = []
    real = fcc.stream_bams
    monkeypatch.setattr(fcc, "stream_bams", lambda *a, **k: (passes.append(1), real(*a, **k))[1])
    assert afc_variants(common, variants) == 0
    assert len(passes) == 1                                            # one ingest for all three
    monkeypatch.setattr(fcc, "stream_bams", real)
    util.assert_dirs_equal(odir, exp)
    for var in (variants[0], variants[2]):
        fresh = var["out_dir"] + "_fresh"
        args = dict(kw, barcode_fn=var["barcode_fn"], out_dir=fresh, min_count=var["min_count"])
        assert afc_wrapper(**args) == 0
        util.assert_dirs_equal(var["out_dir"], fresh)
        with open(os.path.join(fresh, "xcltk.samples.tsv")) as fp:
            assert [x.strip() for x in fp] == sorted(x for x in open(var["barcode_fn"]).read().split())
        assert os.path.getsize(os.path.join(fresh, "xcltk.DP.mtx")) > 100
