"""xck_group_counts / Engine.group_counts: the handle's matrices with their columns summed per cell group (csrc/group_counts.h), and
the group files the front-ends write with XCK_CELL_GROUPS.  Expected values are always group_util.aggregate() - plain numpy - of
per-cell matrices that do not come from the new code: the CPU oracle's for the random cases, the engine's own finish() / refold()
/ snp_counts() output (which other tests pin to the oracle) and the reference's golden files elsewhere.  Comparison is exact
equality of the three arrays.  Every test calls the new method or reads the new files, so none passes without them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fuzz_cases
import group_util as G
import oracle as O
import refold_util as R
import util
from test_gpu_snp_counts import onebase
from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError

pytestmark = pytest.mark.gpu
BASEFC, BAF, BOTH = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF, capi.XCK_MODE_BOTH
FILT = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True)
READ_FILTER_KEYS = tuple(FILT)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mats(mode):
    return (["count"] if mode & BASEFC else []) + (R.MATS if mode & BAF else [])


def _same(got, exp, names):
    assert sorted(got) == sorted(names)
    util.assert_coo_equal(got, exp, names)


def _random_groups(rng, n_cells, n_groups):
    """Groups drawn at random (not monotone in the cell index), about 20 % of the cells left out."""
    cg = rng.integers(0, n_groups, n_cells).astype(np.int32)
    cg[rng.random(n_cells) < 0.2] = -1
    return cg


def _reversed_groups(n_cells, n_groups):
    """Cell c in group (n_groups - 1 - c) % n_groups: inside a row the groups arrive in descending order."""
    return ((n_groups - 1 - np.arange(n_cells)) % n_groups).astype(np.int32)


def _code(fn):
    with pytest.raises(XckError) as ei:
        fn()
    return ei.value.code


# ---------------------------------------------------------------------------------------------- 1. random cases
@pytest.mark.parametrize("key128", [False, True], ids=["key64", "key128"])
@pytest.mark.parametrize("mode", [BASEFC, BAF, BOTH], ids=["basefc", "baf", "both"])
@pytest.mark.parametrize("seed", [11, 25, 53])
def test_random_cases_against_the_oracle(seed, mode, key128):
    names, regions, snps, n_cells, raw, fc, baf, case_flags = fuzz_cases.make_case(seed, many_cells=False, long=False)
    batches = [b for b, _ in raw]
    flags = (case_flags & ~capi.XCK_F_FORCE_KEY128) | (capi.XCK_F_FORCE_KEY128 if key128 else 0)   # the key width is this test's to choose
    rf = {k: baf[k] for k in READ_FILTER_KEYS}
    a = R.variant(regions, snps, min_count=baf["min_count"], min_maf=baf["min_maf"], no_dup_hap=baf["no_dup_hap"])
    b = R.random_variant(np.random.default_rng(1000 + seed), names, regions, snps, max([r[2] for r in regions] + [s[1] for s in snps] + [400]))
    exp = {}                                                             # per-cell matrices, all from the oracle
    if mode & BASEFC:
        cfg, keep = O.make_config(BASEFC, names, regions, [], n_cells, flags=flags, min_include=fc["min_include"], min_count=1, min_maf=0, no_dup_hap=True, **rf)
        exp["count"] = O.run_oracle(cfg, batches)["count"]
    exp_b = dict(exp)
    if mode & BAF:
        pick = lambda d: {k: d[k] for k in R.MATS}
        exp.update(pick(R.oracle_of(names, a, n_cells, batches, rf, flags)))
        exp_b.update(pick(R.oracle_of(names, b, n_cells, batches, rf, flags)))
        exp_snp = pick(R.oracle_of(names, onebase(snps), n_cells, batches, rf, flags))
    rng = np.random.default_rng(seed)
    ng = int(rng.integers(2, 8))
    maps = [(_random_groups(rng, n_cells, ng), ng), (_reversed_groups(n_cells, 5), 5)]
    eng = R.fresh_engine(names, a, n_cells, rf, flags, mode=mode, **(dict(min_include=fc["min_include"]) if mode & BASEFC else {})) if mode & BAF else \
        Engine(BASEFC, names, regions, n_cells, flags=flags, min_include=fc["min_include"], **rf)
    try:
        for bt in batches:
            eng.push(bt)
        util.assert_coo_equal(eng.finish(), exp, _mats(mode))            # (the handle holds what the oracle says)
        assert not key128 or eng.stats()["key_bits"] == 128
        for cg, n in maps:
            _same(eng.group_counts(cg, n), G.aggregate_all(exp, cg), _mats(mode))
        if mode & BAF:
            eng.snp_counts()
            for cg, n in maps:
                _same(eng.group_counts(cg, n, source="snp"), G.aggregate_all(exp_snp, cg), R.MATS)
            R.refold(eng, b)                                             # other regions: the output follows
            for cg, n in maps:
                _same(eng.group_counts(cg, n), G.aggregate_all(exp_b, cg), _mats(mode))
        print("seed %d mode %d: %d cells, nnz %s" % (seed, mode, n_cells, {k: len(v[0]) for k, v in exp.items()}))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 2. mapping corner cases
def _dense():
    names, regions, snps, d = util.unsorted_case(3000)
    return names, regions, snps, util.batch_from_dict(d)


@pytest.mark.parametrize("mode", [BASEFC, BAF], ids=["basefc", "baf"])
def test_mapping_corner_cases(mode):
    names, regions, snps, batch = _dense()
    mats = _mats(mode)
    with Engine(mode, names, regions, 40, snps=snps if mode == BAF else (), flags=capi.XCK_F_FEATURE_SUMMARY, **FILT) as eng:
        eng.push(batch[0])
        res = eng.finish()
        assert all(len(res[m][0]) > 100 for m in mats)
        # identity: the source matrices
        _same(eng.group_counts(np.arange(40), 40), res, mats)
        # one group holding every cell: a single column of row sums - those of the per-feature table
        one = eng.group_counts(np.zeros(40, np.int32))
        fs = eng.feature_summary()
        cols = capi.FEATURE_MATRIX_COLS[mode]
        for m, name in zip(mats, ["umis"] if mode == BASEFC else ["ad", "dp", "oth"]):
            row, col, val = one[m]
            assert not col.any() and np.all(np.diff(row.astype(np.int64)) > 0)
            dense = np.zeros(len(regions), np.int64); dense[row] = val
            assert np.array_equal(dense, fs["matrix"][:, cols.index(name)]), m
        _same(one, G.aggregate_all(res, np.zeros(40, np.int32)), mats)
        # all cells left out: XCK_OK and empty matrices
        none = eng.group_counts(np.full(40, -1, np.int32), 3)
        assert sorted(none) == sorted(mats) and all(len(none[m][j]) == 0 for m in mats for j in range(3))
        # groups without cells are absent
        cg = np.array([1, 4, 7], np.int32)[np.arange(40) % 3]; cg[::5] = -1
        got = eng.group_counts(cg, 10)
        _same(got, G.aggregate_all(res, cg), mats)
        assert all(set(got[m][1].tolist()) == {1, 4, 7} for m in mats)
        # n_groups defaults to max + 1
        _same(eng.group_counts(cg), got, mats)
        # bounds
        assert _code(lambda: eng.group_counts(np.zeros(40, np.int32), capi.XCK_GROUP_MAX + 1)) == capi.XCK_E_ARG
        assert _code(lambda: eng.group_counts(np.zeros(40, np.int32), 0)) == capi.XCK_E_ARG
        bad = np.zeros(40, np.int32); bad[17] = 6
        assert _code(lambda: eng.group_counts(bad, 6)) == capi.XCK_E_ARG           # an entry of n_groups
        bad[17] = -2
        assert _code(lambda: eng.group_counts(bad, 6)) == capi.XCK_E_ARG
        assert _code(lambda: eng.group_counts(cg, 10, source=7)) == capi.XCK_E_ARG
        if mode == BASEFC:
            assert _code(lambda: eng.group_counts(cg, 10, source="snp")) == capi.XCK_E_ARG   # source SNP on a basefc-only handle
        _same(eng.group_counts(cg, 10), got, mats)                       # the handle stays as it was
        _same(eng.finish(), res, mats)
    with Engine(mode, names, regions, 40, snps=snps if mode == BAF else (), **FILT) as eng:   # a handle without hits
        eng.finish()
        none = eng.group_counts(np.arange(40) % 4)
        assert sorted(none) == sorted(mats) and all(len(none[m][j]) == 0 for m in mats for j in range(3))
        if mode == BAF:
            eng.snp_counts()
            none = eng.group_counts(np.arange(40) % 4, source="snp")
            assert all(len(none[m][j]) == 0 for m in R.MATS for j in range(3))


# ---------------------------------------------------------------------------------------------- 3. row shapes
def _shape_engine(row_cells, n_cells):
    """A basefc handle whose count matrix has exactly the wanted (row, cell) entries: non-overlapping 100-base regions, one 50M read
    inside its region per entry with a UMI of its own, and a second UMI on every third entry, so the values are 1 and 2."""
    regions = [("1", 1000 * g + 1, 1000 * g + 100, "r%d" % g) for g in range(len(row_cells))]
    pos, cell = [], []
    k = 0
    for g, cells in enumerate(row_cells):
        for c in cells:
            rep = 2 if k % 3 == 0 else 1
            pos += [1000 * g + 20] * rep; cell += [c] * rep
            k += 1
    n = len(pos)
    d = dict(contig=0, ordinal_base=0, pos=np.array(pos, np.int32), flag=np.zeros(n, np.uint16), mapq=np.full(n, 60, np.uint8), cell=np.array(cell, np.int32),
             umi=((1 << 24) | np.arange(n)).astype(np.uint64), cig_off=np.arange(n + 1, dtype=np.uint32), cigar=np.full(n, (50 << 4) | 0, np.uint32))
    batch = util.batch_from_dict(d)
    eng = Engine(BASEFC, ["1"], regions, n_cells, min_include=0.9, **FILT)
    eng.push(batch[0])
    res = eng.finish()
    assert len(res["count"][0]) == k and set(res["count"][2].tolist()) == {1, 2}
    assert np.array_equal(np.bincount(res["count"][0], minlength=len(row_cells)), [len(c) for c in row_cells])
    return eng, res


def _pick(rng, n_cells, k):
    return np.sort(rng.choice(n_cells, k, replace=False)).tolist()


def _shape_rows(which):
    rng = np.random.default_rng(3)
    if which == "short_and_adjacent_long":                               # rows of 1, 7, 8, 9 entries; empty rows first, in the middle, last; two long rows side by side
        return [[], _pick(rng, 128, 1), _pick(rng, 128, 7), [], _pick(rng, 128, 8), _pick(rng, 128, 9), [], _pick(rng, 128, 70), _pick(rng, 128, 100), []], 128
    if which == "one_row_of_3000":                                       # longer than one pass of a 256-thread block
        return [list(range(3000))], 3000
    assert which == "5000_rows_then_long"                                # the row offsets cross a scan tile (4096 values)
    return [[int(c)] for c in rng.integers(0, 300, 5000)] + [list(range(300))], 300


@pytest.mark.parametrize("long_row", ["8", None], ids=["long_row_8", "long_row_default"])
@pytest.mark.parametrize("which", ["short_and_adjacent_long", "one_row_of_3000", "5000_rows_then_long"])
def test_row_shapes(which, long_row, monkeypatch):
    if long_row is None:
        monkeypatch.delenv("XCK_GROUP_LONG_ROW", raising=False)
    else:
        monkeypatch.setenv("XCK_GROUP_LONG_ROW", long_row)               # (a handle reads its knobs at xck_create)
    rows, n_cells = _shape_rows(which)
    eng, res = _shape_engine(rows, n_cells)
    try:
        rng = np.random.default_rng(8)
        maps = [(_random_groups(rng, n_cells, 5), 5), (_reversed_groups(n_cells, 7), 7), (np.arange(n_cells, dtype=np.int32), n_cells),
                (rng.permutation(n_cells).astype(np.int32) % 1000, 1000), (_random_groups(rng, n_cells, 4096), 4096)]
        for cg, n in maps:
            got = eng.group_counts(cg, n)
            _same(got, G.aggregate_all(res, cg), ["count"])
        assert int(got["count"][2].max()) >= 1
    finally:
        eng.close()


def test_4096_groups_with_5000_cells():
    rng = np.random.default_rng(4)
    eng, res = _shape_engine([list(range(5000)), _pick(rng, 5000, 40), [], _pick(rng, 5000, 900)], 5000)
    try:
        cg = (rng.permutation(5000) % 4096).astype(np.int32)             # every group has a cell, 904 groups have two
        got = eng.group_counts(cg, 4096)
        _same(got, G.aggregate_all(res, cg), ["count"])
        assert len(np.unique(got["count"][1][got["count"][0] == 0])) == 4096
        assert _code(lambda: eng.group_counts(cg, 4097)) == capi.XCK_E_ARG
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------- 4. state and lifetimes
def test_state_and_lifetimes():
    names, regions, snps, batch = _dense()
    rng = np.random.default_rng(2)
    cg1, cg2 = _random_groups(rng, 40, 4), _reversed_groups(40, 6)
    other = R.variant([("1", 500 * g + 1, 500 * g + 400, "h%d" % g) for g in range(300)], snps)
    with Engine(BAF, names, regions, 40, snps=snps, **FILT) as eng:
        assert _code(lambda: eng.group_counts(cg1, 4)) == capi.XCK_E_STATE             # before a finish
        eng.push(batch[0])
        assert _code(lambda: eng.group_counts(cg1, 4)) == capi.XCK_E_STATE
        view = eng.finish(copy=False)
        snap = {k: tuple(x.copy() for x in view[k]) for k in R.MATS}
        assert _code(lambda: eng.group_counts(cg1, 4, source="snp")) == capi.XCK_E_STATE   # no snp_counts yet
        sview = eng.snp_counts(copy=False)
        ssnap = {k: tuple(x.copy() for x in sview[k]) for k in R.MATS}
        g1 = eng.group_counts(cg1, 4, copy=False)
        g1snap = {k: tuple(x.copy() for x in g1[k]) for k in R.MATS}
        _same(g1snap, G.aggregate_all(snap, cg1), R.MATS)
        _same(view, snap, R.MATS); _same(sview, ssnap, R.MATS)            # the views handed out earlier hold the same bytes
        r2 = R.refold(eng, other)                                          # a later refold / snp_counts leaves the group blocks alone
        eng.snp_counts()
        _same(g1, g1snap, R.MATS)
        g2 = eng.group_counts(cg2, 6)                                      # two calls in a row, two mappings, two answers
        g3 = eng.group_counts(cg1, 4)
        _same(g2, G.aggregate_all(r2, cg2), R.MATS)
        _same(g3, G.aggregate_all(r2, cg1), R.MATS)
        _same(eng.group_counts(cg2, 6, source="snp"), G.aggregate_all(ssnap, cg2), R.MATS)
        eng.reset()
        assert _code(lambda: eng.group_counts(cg1, 4)) == capi.XCK_E_STATE             # after a reset
        assert _code(lambda: eng.group_counts(cg1, 4, source="snp")) == capi.XCK_E_STATE
        eng.push(batch[0])
        again = eng.finish()                                               # (under the tables of the refold, which the handle keeps)
        _same(again, r2, R.MATS)
        assert _code(lambda: eng.group_counts(cg1, 4, source="snp")) == capi.XCK_E_STATE   # ... none since the reset
        _same(eng.group_counts(cg1, 4), g3, R.MATS)


def test_snp_source_on_either_side_of_the_copy_out_threshold():
    """The dense SNP x cell case of test_gpu_snp_counts.threshold_case as the source.  Under the identity mapping the output is as
    large as the source and crosses on the copy stream; under a mapping into three groups on the same handle it is stored by the CUs
    into buffers that the large call grew.  A view of the snp_counts blocks taken before holds the same bytes afterwards."""
    from test_gpu_snp_counts import COPY_STREAM_BYTES, THR_CELLS, THR_REGIONS, THR_SNPS, coo_bytes, threshold_case
    snps, batch, exp = threshold_case(THR_SNPS)
    with Engine(BAF, ["1"], THR_REGIONS, THR_CELLS, snps=snps, **FILT) as eng:
        eng.push(batch[0])
        eng.finish()
        sview = eng.snp_counts(copy=False)
        ssnap = {k: tuple(x.copy() for x in sview[k]) for k in R.MATS}
        _same(ssnap, exp, R.MATS)
        ident = np.arange(THR_CELLS, dtype=np.int32)
        big = eng.group_counts(ident, THR_CELLS, source="snp")
        assert coo_bytes(big) >= COPY_STREAM_BYTES
        _same(big, G.aggregate_all(exp, ident), R.MATS)
        _same(sview, ssnap, R.MATS)                                        # the source blocks did not move or change
        cg3 = (np.arange(THR_CELLS) % 3).astype(np.int32)
        small = eng.group_counts(cg3, 3, source="snp")
        assert 0 < coo_bytes(small) < COPY_STREAM_BYTES
        _same(small, G.aggregate_all(exp, cg3), R.MATS)
        _same(sview, ssnap, R.MATS)


def test_debug_timing_prints_one_line():
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import numpy as np, util\nfrom xcltk_amd import capi\nfrom xcltk_amd.engine import Engine\n"
            "names, regions, snps, d = util.unsorted_case(2000)\n"
            "eng = Engine(capi.XCK_MODE_BOTH, names, regions, 40, snps=snps)\n"
            "eng.push(util.batch_from_dict(d)[0]); eng.finish(); eng.group_counts(np.arange(40) %% 3); eng.close()\n"
            % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", code], env=dict(os.environ, XCK_DEBUG_TIMING="1"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("[xck] group_counts:")]
    assert len(lines) == 1 and "source result, 3 groups" in lines[0], r.stdout[-2000:]


# ---------------------------------------------------------------------------------------------- 5. front-ends
def _group_file(tmp_path, barcode_fn):
    """Three groups over the case's barcodes in an order of their own, every seventh barcode not named, and a name outside the run."""
    bcs = [x.strip() for x in open(barcode_fn)]
    gnames = ["tumour", "normal", "stroma"]
    grouped = {}
    for i, bc in enumerate(reversed(bcs)):
        if i % 7 == 3:
            continue
        grouped[bc] = gnames[(i * 5 + i // 3) % 3]
    order = []
    for bc, g in grouped.items():
        if g not in order:
            order.append(g)
    lines = ["%s\t%s\n" % kv for kv in grouped.items()] + ["NOT-A-CELL\t%s\n" % order[0]]
    fn = str(tmp_path / "cell_groups.tsv")
    open(fn, "w").write("".join(lines))
    cells = sorted(bcs)                                                   # column j = j-th sorted barcode
    cg = np.array([order.index(grouped[c]) if c in grouped else -1 for c in cells], np.int32)
    assert len(order) == 3 and (cg == -1).any()
    return fn, order, cg


def _expected_mtx(exp_dir, fn):
    return G.read_mtx(os.path.join(exp_dir, fn))


def _check_group_files(out_dir, exp_dir, prefix, pairs, order, cg, names_fn, same_bytes=True):
    """pairs: [(cell file, group file)] of out_dir; the cell files are the reference's bytes (same_bytes=False: its entries, for the
    cellSNP fixtures, whose text another writer made), the group files parse to aggregate() of the reference's matrices with the
    cell files' row count and one column per group."""
    assert open(os.path.join(out_dir, names_fn)).read() == "".join(g + "\n" for g in order)
    for cell_fn, group_fn in pairs:
        (n_rows, n_cols, _), coo = _expected_mtx(exp_dir, cell_fn)
        if same_bytes:
            assert open(os.path.join(out_dir, cell_fn), "rb").read() == open(os.path.join(exp_dir, cell_fn), "rb").read()
        else:
            dims, mine = G.read_mtx(os.path.join(out_dir, cell_fn))
            assert dims == (n_rows, n_cols, len(coo[0]))
            key = lambda m: sorted(zip(*[a.tolist() for a in m]))
            assert key(mine) == key(coo), cell_fn
        dims, got = G.read_mtx(os.path.join(out_dir, group_fn))
        exp = G.aggregate(coo, cg)
        assert dims == (n_rows, 3, len(exp[0])), group_fn
        assert all(np.array_equal(a, b) for a, b in zip(got, exp)), group_fn


BAF_PAIRS = [("xcltk.%s.mtx" % k, "xcltk.%s.groups.mtx" % k) for k in ("AD", "DP", "OTH")]


def test_front_ends_write_group_files(tmp_path, monkeypatch):
    from xcltk_amd.baf.fc.main import afc_wrapper
    from xcltk_amd.fused import fused_wrapper
    from xcltk_amd.rdr.fc.main import fc_wrapper
    for k in ("WORLD_SIZE", "XCK_DIST_FORCE", "RANK"):
        monkeypatch.delenv(k, raising=False)
    case, ddir, odir, exp_fc = util.load_case("dense_basefc_default", tmp_path)
    fn, order, cg = _group_file(tmp_path, case["kwargs"]["barcode_fn"])
    monkeypatch.setenv("XCK_CELL_GROUPS", fn)
    assert fc_wrapper(**case["kwargs"]) == 0
    _check_group_files(odir, exp_fc, "", [("matrix.mtx", "matrix.groups.mtx")], order, cg, "groups.tsv")
    for f in os.listdir(exp_fc):
        assert open(os.path.join(odir, f), "rb").read() == open(os.path.join(exp_fc, f), "rb").read()
    bcase, _, bdir, exp_baf = util.load_case("dense_baf_default", tmp_path)
    assert afc_wrapper(**bcase["kwargs"]) == 0
    _check_group_files(bdir, exp_baf, "xcltk.", BAF_PAIRS, order, cg, "xcltk.groups.tsv")
    for f in os.listdir(exp_baf):
        assert open(os.path.join(bdir, f), "rb").read() == open(os.path.join(exp_baf, f), "rb").read()
    # the fused path: one decode, both sets (dense_baf_allreg_dup is the BAF reference of a fused run: every region keeps its row)
    acase, _, _, exp_all = util.load_case("dense_baf_allreg_dup", tmp_path)
    extra = {k: acase["kwargs"][k] for k in ("no_dup_hap", "min_count", "min_maf") if k in acase["kwargs"]}
    out = str(tmp_path / "fused")
    kw = case["kwargs"]
    assert fused_wrapper(kw["sam_fn"], kw["barcode_fn"], kw["region_fn"], acase["kwargs"]["phased_snp_fn"], out, ncores=2, **extra) == 0
    _check_group_files(os.path.join(out, "basefc"), exp_fc, "", [("matrix.mtx", "matrix.groups.mtx")], order, cg, "groups.tsv")
    _check_group_files(os.path.join(out, "baf"), exp_all, "xcltk.", BAF_PAIRS, order, cg, "xcltk.groups.tsv")
    # a name in two groups: the front-end fails before it opens a BAM and writes no matrix
    open(fn, "a").write("%s\tsomething-else\n" % sorted(x.strip() for x in open(kw["barcode_fn"]))[0])
    bad = dict(kw, out_dir=str(tmp_path / "bad"))
    assert fc_wrapper(**bad) == -1 and not os.path.exists(os.path.join(bad["out_dir"], "matrix.mtx"))


def test_afc_variants_writes_group_files_in_both_directories(tmp_path, monkeypatch):
    from xcltk_amd.baf.fc.variants import afc_variants
    for k in ("WORLD_SIZE", "XCK_DIST_FORCE", "RANK"):
        monkeypatch.delenv(k, raising=False)
    c1, ddir, o1, e1 = util.load_case("dense_baf_default", tmp_path)
    c2, _, o2, e2 = util.load_case("dense_baf_allreg_dup", tmp_path)
    fn, order, cg = _group_file(tmp_path, c1["kwargs"]["barcode_fn"])
    monkeypatch.setenv("XCK_CELL_GROUPS", fn)
    common = {k: c1["kwargs"][k] for k in ("sam_fn", "barcode_fn", "phased_snp_fn")}
    variants = [{k: v for k, v in c["kwargs"].items() if k not in common} for c in (c1, c2)]
    assert afc_variants(common, variants) == 0
    _check_group_files(o1, e1, "xcltk.", BAF_PAIRS, order, cg, "xcltk.groups.tsv")
    _check_group_files(o2, e2, "xcltk.", BAF_PAIRS, order, cg, "xcltk.groups.tsv")


@pytest.mark.parametrize("one_pass", [True, False], ids=["one_pass", "two_pass"])
def test_pipeline_writes_step_1_group_files(one_pass, tmp_path, monkeypatch):
    """`xcltk baf` with XCK_BAF_ONE_PASS=1 (source SNP) and without (source RESULT of the pileup's one-base handle): the step-1 group
    files in the raw and in the filtered directory have the rows of the cell files next to them and are aggregate() of those files,
    which are the reference's fixtures; step 3 writes its own."""
    from test_genotype import GT, assert_cellsnp_dirs_equal
    from xcltk_amd.baf.pipeline import pipeline_wrapper
    from xcltk_amd.utils import csp_io
    DS = os.path.join(util.GOLDEN, "datasets", "phasing")
    name, case = __import__("test_genotype")._genotype_cases()[0]
    covered = set(csp_io.load_data(os.path.join(GT, name)).pos.tolist())
    lines = open(os.path.join(DS, "snps.tsv")).read().splitlines()
    snp_fn = str(tmp_path / "phased.tsv")
    open(snp_fn, "w").write("\n".join([lines[0]] + [l for l in lines[1:] if int(l.split("\t")[1]) in covered]) + "\n")
    for k in ("XCK_READ_FATE", "XCK_CELL_SUMMARY", "XCK_FEATURE_SUMMARY", "WORLD_SIZE", "XCK_DIST_FORCE", "RANK", "XCK_BAF_ONE_PASS"):
        monkeypatch.delenv(k, raising=False)
    if one_pass:
        monkeypatch.setenv("XCK_BAF_ONE_PASS", "1")
    fn, order, cg = _group_file(tmp_path, os.path.join(DS, "barcodes.tsv"))
    monkeypatch.setenv("XCK_CELL_GROUPS", fn)
    out = str(tmp_path / "out")
    assert pipeline_wrapper("smp", sam_fn=os.path.join(DS, "possorted.bam"), barcode_fn=os.path.join(DS, "barcodes.tsv"),
                            snp_vcf_fn=os.path.join(DS, "cellsnp", "cellSNP.base.vcf.gz"), region_fn=os.path.join(DS, "regions.tsv"),
                            out_dir=out, phased_snp_fn=snp_fn, ref_cell_fn=os.path.join(DS, "ref_cells.tsv"),
                            min_count=case["min_count"], min_maf=case["min_maf"], ncores=2) == 0
    p1 = os.path.join(out, "1_pileup")
    pairs = [("cellSNP.tag.%s.mtx" % k, "cellSNP.tag.%s.groups.mtx" % k) for k in ("AD", "DP", "OTH")]
    for got_dir, exp_dir in ((os.path.join(p1, "raw"), os.path.join(GT, "raw")), (p1, os.path.join(GT, name))):
        _check_group_files(got_dir, exp_dir, "cellSNP.", pairs, order, cg, "cellSNP.groups.tsv", same_bytes=False)
    fc = os.path.join(out, "3_baf_fc")
    assert open(os.path.join(fc, "xcltk.groups.tsv")).read() == "".join(g + "\n" for g in order)
    for cell_fn, group_fn in BAF_PAIRS:
        (n_rows, _, _), coo = G.read_mtx(os.path.join(fc, cell_fn))
        dims, got = G.read_mtx(os.path.join(fc, group_fn))
        exp = G.aggregate(coo, cg)
        assert dims == (n_rows, 3, len(exp[0])) and all(np.array_equal(a, b) for a, b in zip(got, exp))
