"""Key layouts and table sizes through the join and both folds on the GPU.

Every count travels as a packed key row | cell | umi whose field widths follow from the table sizes alone (key_layout(),
xcltk_amd/csrc/xck_internal.h), and many code paths are chosen from those widths: the span bitmap and the cell groups of the partition
fold, the digits of the radix-sort fold, the packed haplotype class of the pileup, 64- against 128-bit keys.  The cases of
tests/layout_cases.py put keys at the edges of every field at each of those widths; the oracle (oracle/xck_oracle.c: (cell, umi)
structs, 64-bit coordinates, no packed key) is the reference, compared exactly, and for the targeted basefc cases the answer is also
known by construction.  Knobs are read at xck_create: they are set before an Engine is made and restored by `fold_env`."""
import functools
import os

import numpy as np
import pytest

import layout_cases as LC
import oracle as O
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine
from xcltk_amd.synth import soa

pytestmark = pytest.mark.gpu

KNOBS = ("XCK_FOLD", "XCK_FOLD_C", "XCK_FOLD_LGG", "XCK_FULL_SORT", "XCK_PILEUP_SORT", "XCK_PILEUP_HAP")
KW = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True, min_include=0.9, min_count=1, min_maf=0, no_dup_hap=True)
FC, BAF = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF
MATS = {FC: ["count"], BAF: ["ad", "dp", "oth"]}


@pytest.fixture
def fold_env():
    saved = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    yield os.environ
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _knobs(env, **kv):
    """Exactly these knobs (FOLD="sort" -> XCK_FOLD=sort), every other one of KNOBS unset."""
    for k in KNOBS:
        env.pop(k, None)
    for k, v in kv.items():
        env["XCK_" + k] = str(v)


def _engine(mode, names, regions, snps, n_cells, batches, repeat=False, second=None, **filt):
    """The engine alone -> (matrices, stats); repeat: then reset, push and finish again on the same handle -> (first, second, stats).
    second: the batches of that second round when they are not the first's; a pileup handle then also recounts the second finish
    with its own tables (refold) -> (first, second, refolded or None, (stats of the first round, of the second))."""
    kw = dict(KW); kw.update(filt)
    eng = Engine(mode, names, regions, n_cells, snps=snps if mode == BAF else (), **kw)
    try:
        outs, sts = [], []
        for rnd in range(2 if repeat else 1):
            if rnd:
                eng.reset()
            for b, _keep in (second if rnd and second is not None else batches):
                eng.push(b)
            outs.append({k: tuple(np.array(a) for a in v) for k, v in eng.finish().items()})
            sts.append(eng.stats())
        if second is not None:
            outs.append({k: tuple(np.array(a) for a in v) for k, v in eng.refold(regions).items()} if mode == BAF else None)
    finally:
        eng.close()
    return tuple(outs) + ((tuple(sts),) if second is not None else (sts[-1],))


def _oracle(mode, names, regions, snps, n_cells, batches, **filt):
    kw = dict(KW); kw.update(filt)
    cfg, keep = O.make_config(mode, names, regions, snps if mode == BAF else [], n_cells, **kw)
    return O.run_oracle(cfg, [b for b, _ in batches])


# ----------------------------------------------------------------------------- 3. the layout grid
@pytest.mark.parametrize("shape", LC.GRID, ids=lambda s: "%dx%d" % s)
def test_grid_basefc(shape, fold_env):
    """Targeted keys at every shape of the grid: (3, 2) the floor (cbits 1, rbits 2); (3, 2048 | 2049) span bitmap 2^11 -> 2^12;
    (3, 16384 | 16385) 2^14 -> 2^15; (3, 65536 | 65537) 2^16, then lg_min 0 -> 1; (63, 2^30) cbits 30, ubits 28, lg_min 14;
    (255, 256), (65535, 65536), (65536, 65536) rbits + cbits = 16, 32, 33 (whole digits of the sort fold, and one bit more);
    (262143, 2^20) ubits 26, the narrowest 64-bit key; (262144, 2^20) and (262143, 2^20 + 1) 128-bit keys without the force flag.
    The matrix equals the oracle and the by-construction answer, and the handle reports the layout computed from the rule; 64-bit
    layouts run again under the radix-sort fold (partial and full sort) and with pages of 8 keys."""
    n, n_cells = shape
    case = LC.targeted_case(n, n_cells)
    key_bits, umi_bits, cbits, rbits = case.layout
    batches = [util.batch_from_dict(case.d)]
    got, exp, st = util.engine_vs_oracle(FC, case.names, case.regions, [], n_cells, batches)
    util.assert_coo_equal(got, exp, ["count"])
    util.assert_coo_equal(got, case.expected, ["count"])
    assert (st["key_bits"], st["umi_bits"]) == (key_bits, umi_bits)
    if key_bits == 128:
        assert st["fold_path"] == 2 and st["fold_fallbacks"] == 0            # the partition fold takes 64-bit keys only
        return
    assert st["fold_path"] == 1 and st["fold_fallbacks"] == 0
    for knobs, paths in ((dict(FOLD="sort"), (2,)), (dict(FOLD_C=8), (1, 2)), (dict(FOLD="sort", FULL_SORT=1), (2,))):
        _knobs(fold_env, **knobs)
        alt, st = _engine(FC, case.names, case.regions, [], n_cells, batches)
        util.assert_coo_equal(alt, case.expected, ["count"])
        assert st["fold_path"] in paths and (st["key_bits"], st["umi_bits"]) == (key_bits, umi_bits), knobs


@pytest.mark.parametrize("shape", LC.GRID, ids=lambda s: "%dx%d" % s)
def test_grid_baf(shape, fold_env):
    """The same shapes with one SNP per region (n_snps = n_regions: the SNP rows of the pileup and the region rows of its second stage
    use the same row width), each read showing REF, ALT or a third base: AD, DP, OTH equal the oracle and the by-construction answer
    under the default sorts, with the haplotype class in a value word (XCK_PILEUP_HAP=values), on completely sorted items (=sorted)
    under the library radix sort, and with pages of 8 keys in both partition sorts.  (The interned codes of the case fill the UMI field, so the default run carries the class in
    a value word as well: test_packed_haplotype_class_on_both_sides_of_its_bound covers the packed class.)"""
    n, n_cells = shape
    case = LC.targeted_case(n, n_cells, n_snps=n)
    key_bits, umi_bits, cbits, rbits = case.layout
    batches = [util.batch_from_dict(case.d)]
    got, exp, st = util.engine_vs_oracle(BAF, case.names, case.regions, case.snps, n_cells, batches)
    util.assert_coo_equal(got, exp, MATS[BAF])
    util.assert_coo_equal(got, case.expected, MATS[BAF])
    assert (st["key_bits"], st["umi_bits"]) == (key_bits, umi_bits) and len(exp["dp"][0]) > 0 and len(exp["oth"][0]) > 0
    assert (st["pileup_sort_path"], st["pileup_sort2_path"]) == ((1, 1) if key_bits == 64 else (2, 2))
    for knobs, paths in ((dict(PILEUP_HAP="values"), (1, 1)), (dict(PILEUP_HAP="sorted"), (1, 3)), (dict(PILEUP_SORT="radix"), (2, 2)),
                         (dict(FOLD_C=8), (1, 1) if cbits == 1 else (2, 1))):
        # (pages of 8 keys: an item of the partition sorts holds 16 hits.  A SNP's ~60 hits get 2^4 cell groups, so from 5 cell bits on cells
        #  0 and 1 share a group of ~25 hits and the first sort hands over to the radix sort; with 2 cells each is a group of its own (<= 14 hits).
        #  The region-level hits are one per molecule: 5 per (region, cell), within an item.)
        _knobs(fold_env, **knobs)
        alt, st = _engine(BAF, case.names, case.regions, case.snps, n_cells, batches)
        print(shape, knobs, "pileup_sort_path %d pileup_sort2_path %d" % (st["pileup_sort_path"], st["pileup_sort2_path"]))
        util.assert_coo_equal(alt, case.expected, MATS[BAF])
        assert (st["pileup_sort_path"], st["pileup_sort2_path"]) == (paths if key_bits == 64 else (2, 2)), knobs


# (n_regions = n_snps, n_cells) -> ubits 26, 27, 28
NARROW = [(262143, 1 << 20), (131071, 1 << 20), (63, 1 << 30)]


@pytest.mark.parametrize("shape", NARROW, ids=lambda s: "%dx%d" % s)
def test_packed_haplotype_class_on_both_sides_of_its_bound(shape, fold_env):
    """sort_region_hits() keeps the haplotype class of a region-level hit in two free bits of the UMI field when used2 + 2 <= ubits
    (used2 = bits of the OR of the UMI codes seen) and in a value word otherwise.  With 2-bit coded UMIs only and the all-T 12-mer
    (25 bits) the widest code, used2 + 2 = 27:
      ubits 26 (262143 x 2^20): one above ubits -> value word;
      ubits 27 (131071 x 2^20): equal to ubits  -> packed, the class sits in the top two bits of the field;
      ubits 28 (63 x 2^30):     one below ubits -> packed, one free bit above the class.
    The longest direct code of the layout itself (12-mer at 26 and 27 bits, 13-mer = 27 bits at 28) is run as well: at ubits 28 it
    gives used2 + 2 = 29, the value word again.  pileup_sort2_path == 1 says that k_hap_items summed the runs in either form."""
    n, n_cells = shape
    ub = LC.expected_layout(n, n_cells, n)[1]
    assert ub == 26 + NARROW.index(shape)
    for kinds, used2 in ((("mer12_t", "mer4", "none"), 25), (("direct_t", "direct_a", "mer4"), 2 * LC.longest_direct(ub) + 1)):
        case = LC.targeted_case(n, n_cells, n_snps=n, umi_kinds=kinds)
        assert max(c for c in case.codes.values() if c != capi.XCK_UMI_NONE).bit_length() == used2
        packed = used2 + 2 <= ub
        assert packed == {(26, 25): False, (27, 25): True, (28, 25): True, (28, 27): False}[(ub, used2)]
        batches = [util.batch_from_dict(case.d)]
        got, exp, st = util.engine_vs_oracle(BAF, case.names, case.regions, case.snps, n_cells, batches)
        util.assert_coo_equal(got, exp, MATS[BAF])
        util.assert_coo_equal(got, case.expected, MATS[BAF])
        assert (st["key_bits"], st["umi_bits"], st["pileup_sort2_path"]) == (64, ub, 1)


# ----------------------------------------------------------------------------- 4. every cell-bit regime with depth
CELLS = [2048, 4096, 8192, 16384, 32768, 65536, 131072, 1 << 20]


@functools.lru_cache(maxsize=None)
def _deep_tables(mode):
    """basefc: 4 genes on 400 kb; BAF: 120 regions and 4000 SNPs."""
    if mode == FC:
        return soa.make_tables(4, 0, [400000], seed=71, max_len=150000)
    return soa.make_tables(120, 4000, [1500000], seed=73, max_len=150000)


def _deep_reads(mode, n_cells, last_cells_deep=False):
    """200 k reads (BAF: 100 k) with cells drawn evenly from [0, n_cells) - for basefc tens of thousands of keys per row, so the bucket
    kernels see full pages at every cell count.  last_cells_deep: every second molecule moves to one of the last 64 cells, which makes
    the top of the cell field deep and the cells of the row's last group far from even."""
    regions, snps, names = _deep_tables(mode)
    bs = soa.gen_reads(regions, names, 200000 if mode == FC else 100000, n_cells, seed=72 + mode, with_seq=mode == BAF)
    if last_cells_deep:
        for b in bs:
            c = b["cell"].astype(np.int64)
            b["cell"] = np.where((c >= 0) & (c & 1 == 1), n_cells - 1 - (c >> 1) % 64, c).astype(np.int32)
    return names, regions, snps, [util.batch_from_dict(b) for b in bs]


@pytest.mark.parametrize("n_cells", CELLS)
def test_partition_fold_at_every_span_width(n_cells, fold_env):
    """cbits 11 ... 17 and 20: span bitmaps of 2^11 ... 2^16 (row, cell) pairs and, from 17 cell bits on, rows of at least 2 and 16
    cell groups (lg_min 1, 4), with ~40 k keys per row.  Default page size: the partition fold, no hand-over.  Pages of 64 keys: big
    cells and level 2, with the cell groups left to the fold and with at most 8 per row (XCK_FOLD_LGG=3; lg_min still holds)."""
    names, regions, snps, batches = _deep_reads(FC, n_cells)
    cbits = LC.bits_for_count(n_cells)
    assert cbits == {2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15, 65536: 16, 131072: 17, 1 << 20: 20}[n_cells]
    got, exp, st = util.engine_vs_oracle(FC, names, regions, [], n_cells, batches)
    util.assert_coo_equal(got, exp, ["count"])
    assert st["fold_path"] == 1 and st["fold_fallbacks"] == 0 and st["key_bits"] == 64 and st["umi_bits"] == 64 - 3 - cbits
    assert len(exp["count"][0]) > 4000 and int(exp["count"][1].max()) >= n_cells - n_cells // 16 and int(exp["count"][1].min()) < n_cells // 16
    for knobs in (dict(FOLD_C=64), dict(FOLD_C=64, FOLD_LGG=3)):
        _knobs(fold_env, **knobs)
        alt, st = _engine(FC, names, regions, [], n_cells, batches)
        util.assert_coo_equal(alt, exp, ["count"])
        assert st["fold_path"] in (1, 2), knobs


# n_cells -> (fold_path, fold_fallbacks) at the default page size, (fold_path, fold_fallbacks) at pages of 64 keys
LAST_CELLS_DEEP = {2048: ((1, 0), (1, 0)), 4096: ((1, 0), (1, 0)), 8192: ((1, 0), (1, 0)), 16384: ((1, 0), (1, 0)), 32768: ((1, 0), (1, 0)),
                   65536: ((2, 1), (1, 0)), 131072: ((2, 1), (2, 1)), 1 << 20: ((2, 1), (2, 1))}


@pytest.mark.parametrize("n_cells", CELLS)
def test_partition_fold_with_the_last_cells_deep(n_cells, fold_env):
    """The same reads with every second molecule in one of the last 64 cells: the top of the cell field holds ~150 keys per (row,
    cell), and the last cell group of a row (2^sg cells, sg = cbits - 6: a hot row gets 2^6 groups) is "big", ~11 k keys, with cells far
    from even.  Level 2 sizes its sub-cells for even cells; the sub-cell that holds the 64 deep cells comes out above a work item, and
    the group asks for single cells cut into 2^more UMI-hash parts, more = bits that bring the sub-cell's keys under a quarter page
    (k_pf_plan2).  The request is granted while sg + more <= 16 - a big cell has at most 2^16 sub-cells - and while all level-2 cells
    together fit their room (64 per page of big keys + 64 per big cell + 65536: ~68 k here at the default page); otherwise the fold
    hands over to the radix-sort fold: fold_path 2, fold_fallbacks 1.  Default page (1024 keys, quarter page 256), ~45 k big keys:
      up to 2^15 cells: sg <= 9, more <= 4: at most one refinement, 4 x 2^13 level-2 cells, the partition fold finishes (1, 0);
      2^16 cells: sg = 10, ~5.6 k keys in the deep sub-cell, more = 5: granted, but 4 rows x 2^15 = 131 072 level-2 cells exceed the room;
      2^17 cells: sg = 11, 64 cells per sub-cell, ~10 k keys, more = 6 -> 17 > 16: refused;
      2^20 cells: sg = 14, ~16.7 k keys, more = 7 -> 21: refused.
    Pages of 64 keys take the same side at every width but 2^16 cells: there nearly all ~89 k keys are in big cells and the room is
    64 x 1390 + 64 x 256 + 65536 = ~170 k level-2 cells, enough for the 131 072, so the partition fold finishes.  The inputs are seeded, so the path is the same in every run; LAST_CELLS_DEEP
    lists it per cell count (the matrix equals the oracle on either path)."""
    names, regions, snps, batches = _deep_reads(FC, n_cells, last_cells_deep=True)
    got, exp, st = util.engine_vs_oracle(FC, names, regions, [], n_cells, batches)
    print("last cells deep, n_cells %d, default page: fold_path %d fallbacks %d refinements %d" % (n_cells, st["fold_path"], st["fold_fallbacks"], st["fold_refinements"]))
    util.assert_coo_equal(got, exp, ["count"])
    assert int(exp["count"][1].max()) == n_cells - 1 and int(exp["count"][2][exp["count"][1] >= n_cells - 64].max()) > 100
    assert (st["fold_path"], st["fold_fallbacks"]) == LAST_CELLS_DEEP[n_cells][0]
    _knobs(fold_env, FOLD_C=64)
    alt, st = _engine(FC, names, regions, [], n_cells, batches)
    print("last cells deep, n_cells %d, pages of 64: fold_path %d fallbacks %d refinements %d" % (n_cells, st["fold_path"], st["fold_fallbacks"], st["fold_refinements"]))
    util.assert_coo_equal(alt, exp, ["count"])
    assert (st["fold_path"], st["fold_fallbacks"]) == LAST_CELLS_DEEP[n_cells][1]


@pytest.mark.parametrize("n_cells", CELLS)
def test_pileup_partition_sort_at_every_cell_width(n_cells, fold_env):
    """The pileup's two partition sorts at the same cell widths, at the default page size and with pages of 8 keys."""
    names, regions, snps, batches = _deep_reads(BAF, n_cells)
    got, exp, st = util.engine_vs_oracle(BAF, names, regions, snps, n_cells, batches)
    util.assert_coo_equal(got, exp, MATS[BAF])
    assert st["pileup_sort_path"] == 1 and st["pileup_sort2_path"] == 1 and len(exp["dp"][0]) > 1000
    _knobs(fold_env, FOLD_C=8)
    alt, st = _engine(BAF, names, regions, snps, n_cells, batches)
    util.assert_coo_equal(alt, exp, MATS[BAF])
    assert st["pileup_sort_path"] in (1, 2) and st["pileup_sort2_path"] in (1, 2)


# ----------------------------------------------------------------------------- 5. many rows
def _bins_case(n_rows, n_cells, n_reads, seed):
    """Bins of 1 kb on one contig, n_reads synthetic reads over them and the targeted keys of the layout as a second file."""
    case = LC.targeted_case(n_rows, n_cells, ordinal_base=1 << 40)
    bs = soa.gen_reads(case.regions, case.names, n_reads, n_cells, seed=seed, with_seq=False)
    return case, [util.batch_from_dict(b) for b in bs] + [util.batch_from_dict(case.d)]


def _assert_targeted_rows(got, case):
    """The entries of the targeted keys that no synthetic read shares (the interned codes are theirs alone) are in the matrix."""
    have = set(zip(got["count"][0].tolist(), got["count"][1].tolist()))
    assert all((r, c) in have for r, c in zip(case.expected["count"][0].tolist(), case.expected["count"][1].tolist()))


@pytest.mark.parametrize("n_rows,tiles,iterations", [(278528, 1089, 2), (1048577, 4097, 5)])
def test_partition_fold_scans_more_counters_than_one_pass_of_the_top_scan(n_rows, tiles, iterations, fold_env):
    """Level 1 of the partition fold scans (Z << 4) + 1 counters (Z = level-1 cells >= rows; 2^4 copies of every counter) in tiles of
    4096, and k_scan_top walks the tile sums 1024 at a time, carrying the running total from one iteration to the next.
    278 528 rows: >= 4 456 449 counters = 1089 tiles -> a second iteration with a partial tail of 65 tile sums.
    1 048 577 rows (rbits 21): >= 16 777 233 counters = 4097 tiles -> 5 iterations, the last with one tile sum.
    A lost carry moves every count of the later tiles to the wrong work item.  4096 cells, 200 k reads plus the targeted keys (first
    and last row, the rows around the top bit of the row field): the partition fold, no hand-over, equal to the oracle and to the
    radix-sort fold."""
    assert ((n_rows << 4) + 1 + 4095) // 4096 == tiles and (tiles + 1023) // 1024 == iterations
    case, batches = _bins_case(n_rows, 4096, 200000, seed=81)
    got, exp, st = util.engine_vs_oracle(FC, case.names, case.regions, [], 4096, batches)
    util.assert_coo_equal(got, exp, ["count"])
    _assert_targeted_rows(got, case)
    assert st["fold_path"] == 1 and st["fold_fallbacks"] == 0 and st["umi_bits"] == 64 - 12 - LC.bits_for_count(n_rows + 1)
    assert len(exp["count"][0]) > 20000 and int(exp["count"][0].max()) == n_rows - 1
    _knobs(fold_env, FOLD="sort")
    alt, st = _engine(FC, case.names, case.regions, [], 4096, batches)
    assert st["fold_path"] == 2
    util.assert_coo_equal(alt, exp, ["count"])


def test_million_rows_at_the_narrowest_key_and_beyond_it(fold_env):
    """1 048 577 rows take 21 row bits, which leaves 64-bit keys at most 17 cell bits.
    2^17 cells: ubits 26, the narrowest 64-bit key, with lg_min = 1, so every row has two cell groups and the level-1 cell bound is
    (rows << 1) + ... = 2.1 M, far below 2^24: the partition fold, no hand-over.
    2^20 cells: rbits + cbits = 41 > 38, so the keys are 128 bits wide and the radix-sort fold is the only one (fold_path 2 without a
    hand-over: fold_fallbacks counts partition folds that gave up, and none was started).  The level-1 cell bound of the partition
    fold, rows << lg_min <= 2^24, cannot be exceeded by 64-bit keys of a table of this size: lg_min = cbits - 16 > 0 needs
    rbits + cbits <= 38, and then rows << lg_min < 2^(rbits + cbits - 16) <= 2^22."""
    for n_cells, layout, path in ((1 << 17, (64, 26, 17, 21), 1), (1 << 20, (128, 64, 20, 21), 2)):
        case, batches = _bins_case(1048577, n_cells, 60000, seed=83)
        assert case.layout == layout
        got, exp, st = util.engine_vs_oracle(FC, case.names, case.regions, [], n_cells, batches)
        util.assert_coo_equal(got, exp, ["count"])
        _assert_targeted_rows(got, case)
        assert (st["key_bits"], st["umi_bits"]) == layout[:2] and st["fold_path"] == path and st["fold_fallbacks"] == 0
        assert int(exp["count"][0].max()) == 1048576 and int(exp["count"][1].max()) == n_cells - 1


def test_pileup_with_a_million_snps_and_the_last_row_hit(fold_env):
    """1 048 577 SNPs (rbits 21), one region per 64 of them, 4096 cells; reads over the first, the middle and the last 1000 SNPs, so the
    SNP window index, the row partition and k_tally_rows run at 2^20 rows with the last row in use.  Equal to the oracle under the
    partition sorts and under the library radix sort."""
    n_snps, step = 1048577, 100
    names, regions, snps = LC.snp_table(n_snps, step)
    rng = np.random.default_rng(91)
    first = np.array([0, n_snps // 2 - 500, n_snps - 1000], np.int64)
    pos = (first[rng.integers(0, 3, 30000)] * step + rng.integers(-60, 1000 * step, 30000)).clip(0, None)
    umi = ((1 << 24) | rng.integers(0, 1 << 24, 30000)).astype(np.uint64)
    batches = [util.batch_from_dict(LC.plain_reads(pos, rng.integers(0, 4096, 30000), umi, seed=92))]
    got, exp, st = util.engine_vs_oracle(BAF, names, regions, snps, 4096, batches)
    util.assert_coo_equal(got, exp, MATS[BAF])
    assert (st["key_bits"], st["umi_bits"]) == (64, 31) and st["pileup_sort_path"] == 1 and st["pileup_sort2_path"] == 1
    rows = set(exp["dp"][0].tolist())
    assert {0, len(regions) - 1} <= rows and len(rows) > 40 and len(exp["dp"][0]) > 10000
    _knobs(fold_env, PILEUP_SORT="radix")
    alt, st = _engine(BAF, names, regions, snps, 4096, batches)
    util.assert_coo_equal(alt, exp, MATS[BAF])
    assert st["pileup_sort_path"] == 2 and st["pileup_sort2_path"] == 2


# ----------------------------------------------------------------------------- 6. the sort fold's digits under a giant run
@pytest.mark.parametrize("rc_bits,n_regions,n_cells", [(8, 2, 40), (15, 300, 40), (16, 600, 40), (17, 1200, 40), (24, 3000, 4096)])
def test_sort_fold_digits_under_a_giant_run(rc_bits, n_regions, n_cells, fold_env):
    """The "giant" workload of test_basefc_long_runs_hash_fold_and_fallback (70 % of 150 k reads in one (region, cell)) under
    XCK_FOLD=sort at rbits + cbits = 8, 15, 16, 17, 24 - a multiple of the 8-bit digit, one below, one above - the region table padded
    in front with regions no read touches, so that the keys are in the last two rows.  begin_for() cuts whole digits from the top of
    the key: the sort then reaches 0 ... 7 bits into the UMI field, and every FOLD_GIANT retry one digit further.
      4-mer codes:   used = 9, the keys are squeezed, the sort is partial;
      12-mer codes:  used = 25, squeezed and partial, and the hot pair holds ~50 k distinct UMIs: a giant run that needs further digits;
      interned ids:  used = ubits, top_fc = 64 > 62: the classic path on fully sorted keys.
    A second finish() of the same handle after reset() and the same reads starts from the remembered extra digits and must give the
    same matrix."""
    rng = np.random.default_rng(3)
    n = 150000
    names = ["1"]
    # the padding comes first: the keys lie in the last two rows, n_regions - 2 and n_regions - 1, which differ in bit 0 and have the
    # high bits of the row field set (299 | 298, 599 | 598, 1199 | 1198, 2999 | 2998) - a wrong upper end of the sorted bit range shows
    regions = [("1", 300000 + 10 * i, 300005 + 10 * i, "pad") for i in range(n_regions - 2)] + [("1", 1, 200000, "hot"), ("1", 50000, 60000, "inner")]
    key_bits, ub, cbits, rbits = LC.expected_layout(n_regions, n_cells)
    assert rbits + cbits == rc_bits and key_bits == 64
    pos = np.sort(rng.integers(0, 190000, n)).astype(np.int32)
    cell = np.where(rng.random(n) < 0.7, n_cells - 1, rng.integers(0, n_cells, n)).astype(np.int32)
    draw = rng.integers(0, 60000, n)
    _knobs(fold_env, FOLD="sort")
    for kind, umi in (("mer4", (1 << 8) | (draw & 255)), ("mer12", (1 << 24) | draw), ("interned", (1 << (ub - 1)) | draw)):
        d = dict(contig=0, ordinal_base=0, pos=pos, flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8), cell=cell, umi=umi.astype(np.uint64),
                 cig_off=np.arange(n + 1, dtype=np.uint32), cigar=np.full(n, (91 << 4) | 0, np.uint32))
        batches = [util.batch_from_dict(d)]
        exp = _oracle(FC, names, regions, [], n_cells, batches)
        assert int(exp["count"][2].max()) > (30000 if kind != "mer4" else 255), kind
        first, second, st = _engine(FC, names, regions, [], n_cells, batches, repeat=True)
        util.assert_coo_equal(first, exp, ["count"])
        util.assert_coo_equal(second, exp, ["count"])
        assert st["fold_path"] == 2 and (st["key_bits"], st["umi_bits"]) == (64, ub), kind


# ----------------------------------------------------------------------------- 6b. a workspace freed and allocated anew between two finishes
@functools.lru_cache(maxsize=None)
def _regrow_case(mode):
    """-> names, regions, snps, n_cells, small batches, large batches, oracle of the large ones, lower bound on the large input's keys.
    basefc: 120 genes, 100 reads, then 650 k; the distinct (region, cell, UMI) the oracle counts bound the keys in HBM from below.
    pileup: 40 000 SNPs on the same genes (one per ~100 bases of gene, so that 250 k reads leave the hits the bound asks for), 100 reads,
    then 250 k; the bound: the molecules whose first read shows a base (DP + OTH with one one-base region per SNP, REF on haplotype 0
    and ALT on 1), each of which is at least one hit with a base."""
    n_cells = 2000
    regions, snps, names = soa.make_tables(120, 0 if mode == FC else 40000, [1500000], seed=73, max_len=150000)
    small, large = ([util.batch_from_dict(b) for b in soa.gen_reads(regions, names, n, n_cells, seed=s, with_seq=mode == BAF)] for n, s in ((100, 5), (650000 if mode == FC else 250000, 74)))
    exp = _oracle(mode, names, regions, snps, n_cells, large)
    if mode == FC:
        return names, regions, snps, n_cells, small, large, exp, int(exp["count"][2].sum())
    one = _oracle(mode, names, [(s[0], s[1], s[1], "s%d" % i) for i, s in enumerate(snps)], [(s[0], s[1], s[2], s[3], 0, 1) for s in snps], n_cells, large)
    return names, regions, snps, n_cells, small, large, exp, int(one["dp"][2].sum() + one["oth"][2].sum())


@pytest.mark.parametrize("knobs", [dict(), dict(FOLD="sort"), dict(PILEUP_SORT="radix")], ids=["default", "fold-sort", "pileup-radix"])
@pytest.mark.parametrize("mode", [FC, BAF], ids=["fc", "baf"])
def test_workspaces_grow_between_two_finishes_of_one_handle(mode, knobs, fold_env):
    """One handle: a first input that leaves at most 1000 keys, finish, reset, then one that leaves at least 400 k keys (basefc) /
    200 k hits with a base (pileup), finish.  A workspace keeps need + need / 4 + 1 MiB bytes; workspace 1 of the second finish holds at
    least 8 bytes per basefc key and 16 per pileup hit, 3.2 MB, against at most 2.3 MB kept from the first: every fold's arenas are
    freed and allocated anew between the two, under the default folds, the radix-sort fold and the library sort of the pileup.  The
    second result equals the oracle on the second input alone, and on the pileup handle a refold with the handle's own tables equals
    that finish (the region stage begins workspace 2 again on what the molecule stage left in workspace 1)."""
    names, regions, snps, n_cells, small, large, exp, keys_at_least = _regrow_case(mode)
    assert keys_at_least >= (400000 if mode == FC else 200000)
    _knobs(fold_env, **knobs)
    first, second, refolded, (st1, st2) = _engine(mode, names, regions, snps, n_cells, small, repeat=True, second=large)
    print("mode %d %s: n_hits_unique %d then %d (bound from the oracle %d)" % (mode, knobs, st1["n_hits_unique"], st2["n_hits_unique"], keys_at_least))
    assert 0 < st1["n_hits_unique"] <= 1000 and st2["n_hits_unique"] >= keys_at_least
    assert all(len(first[m][0]) > 0 for m in MATS[mode])
    util.assert_coo_equal(second, exp, MATS[mode])
    if mode == FC:
        assert st2["fold_path"] == 2 or knobs.get("FOLD") != "sort"
    else:
        assert (st2["pileup_sort_path"], st2["pileup_sort2_path"]) == (2, 2) or knobs.get("PILEUP_SORT") != "radix"
        util.assert_coo_equal(refolded, second, MATS[BAF])


# ----------------------------------------------------------------------------- 7. coordinates at the top of BAM's range
@pytest.mark.parametrize("mode,filt", [(FC, dict(min_include=0.9)), (FC, dict(min_include=30)), (BAF, dict())], ids=["fc-0.9", "fc-30", "baf"])
def test_coordinates_at_both_ends_of_the_range(mode, filt, fold_env):
    """Regions, SNPs and reads of every CIGAR kind in [2^31 - 200 000, 2^31 - 1] and, mirrored, in [1, 200 000] of one contig: the last
    region ends and the last SNP lies at 2^31 - 1, reads end exactly there, one starts at 2^31 - 2; a region starts at 1, reads at 0.
    Every read ends at or below 2^31 - 1, the format's range (layout_cases.edge_coordinate_case asserts it).
    Read from the code for these inputs, all in int32: load_read() forms endpos = pos + rlen <= 2^31 - 1; included_len() forms p + l
    only for ops inside the read, so p + l <= endpos, and compares with the region's s0 = start - 1 >= 0 and e0 = end <= 2^31 - 1;
    pileup_complex() forms rp + l <= endpos and min(rp + l, endpos); the SNP window index has (2^31 - 1 >> 10) + 1 = 2^21 windows
    and forms w << 10 <= 2^31 - 1024 for the last of them; a SNP's 0-based position is pos - 1 <= 2^31 - 2.  Nothing wraps; the
    first sum that would is endpos of a read beyond the format's range, which is not pushed here."""
    names, regions, snps, n_cells, d = LC.edge_coordinate_case()
    batches = [util.batch_from_dict(d)]
    got, exp, st = util.engine_vs_oracle(mode, names, regions, snps, n_cells, batches, min_len=1, **filt)
    util.assert_coo_equal(got, exp, MATS[mode])
    m = exp["count" if mode == FC else "dp"]
    n_lo = len(regions) // 2
    assert (m[0] < n_lo).sum() > 200 and (m[0] >= n_lo).sum() > 200 and int(m[0].max()) == len(regions) - 1
    assert st["key_bits"] == 64
