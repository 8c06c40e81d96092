"""min_include, min_maf / min_count and min_mapq / min_len on the device at the values where their decisions flip
(tests/threshold_cases.py): exact ties m / n == f, the pairs a reciprocal multiply, float32 or an exact-rational compare get wrong,
non-integer thresholds, each include pair in every shape that reaches frac_below / full_ok / included_len's shortcuts by another
path.  Every case runs with 64- and with 128-bit keys against the CPU oracle and against the plain-Python rule, compared exactly;
the opt-in summaries (read_fate.h repeats the decision) must flip at the same pairs; xck_refold re-judges one finished pileup under
every min_maf / min_count and under a cell mask.  tests/test_threshold_cases_host.py shows on the CPU that every wrong model of a rule
changes the expected matrices of some case, i.e. that a kernel which computes one of them cannot pass here."""
import numpy as np
import pytest

import cell_summary_util as CU
import feature_summary_util as F
import oracle as O
import refold_cells_cases as K
import refold_util as R
import threshold_cases as T
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine

pytestmark = pytest.mark.gpu
F128 = capi.XCK_F_FORCE_KEY128
SUMMARIES = capi.XCK_F_READ_FATE | capi.XCK_F_CELL_SUMMARY | capi.XCK_F_FEATURE_SUMMARY
BAF_MATS = ["ad", "dp", "oth"]
KEYS = pytest.mark.parametrize("flags", [0, F128], ids=["key64", "key128"])
SETTINGS = T.snp_settings()


# ----------------------------------------------------------------------------- min_include, min_mapq, min_len
@KEYS
@pytest.mark.parametrize("name", T.NAMES)
def test_include_and_read_filter_case(name, flags):
    c = T.case(name)
    batches = [util.batch_from_dict(d) for d in c.batches]
    got, exp, stats = util.engine_vs_oracle(c.mode, c.names, c.regions, c.snps, c.n_cells, batches, flags=flags, **c.filt)
    want, n_acc = T.expected_entries(c)
    print("%s flags=%d: %d reads, %d pairs under test, %d accepted, n_hits %d" % (name, flags, c.n_reads, len(c.pairs), n_acc, stats["n_hits"]))
    util.assert_coo_equal(got, exp, ["count"])
    bad = sorted(set(T.entries_of(got["count"]).items()) ^ set(want.items()))
    rows = {r for (r, _), _ in bad}
    assert not bad, [(p["shape"], p["m"], p["n"]) for p in c.pairs if p["row"] in rows][:10]
    assert stats["n_hits"] == n_acc
    assert stats["key_bits"] == (128 if flags else 64)


@pytest.mark.parametrize("name", T.NAMES)
def test_summaries_flip_with_the_join(name):
    """read fate, per-cell and per-region tables: include_fail / assigned / pairs are those of feature_summary_util.region_outcome
    over every fetched pair of the case"""
    c = T.case(name)
    reg, cell, tot = T.summary_expect(c)
    with Engine(c.mode, c.names, c.regions, c.n_cells, flags=SUMMARIES, **c.filt) as eng:
        for d in c.batches:
            eng.push(util.batch_from_dict(d)[0])
        rf, cs, fs = eng.read_fate(), eng.cell_summary(), eng.feature_summary()
        eng.finish()
        n_hits = eng.stats()["n_hits"]
    print("%s: read fate %r" % (name, {k: rf[k] for k in tot}))
    assert {k: rf[k] for k in tot} == tot
    assert np.array_equal(cs["fate"][:, [CU.INCLUDE_FAIL, CU.ASSIGNED, CU.PAIRS]], cell), np.flatnonzero((cs["fate"][:, [CU.INCLUDE_FAIL, CU.ASSIGNED, CU.PAIRS]] != cell).any(axis=1))[:10]
    assert np.array_equal(fs["reads"][:, [F.INCLUDE_FAIL, F.PAIRS]], reg), np.flatnonzero((fs["reads"][:, [F.INCLUDE_FAIL, F.PAIRS]] != reg).any(axis=1))[:10]
    assert n_hits == tot["pairs"] == T.expected_entries(c)[1]


# ----------------------------------------------------------------------------- min_maf, min_count
@pytest.fixture(scope="module")
def pool():
    p = T.snp_pool()
    return p, T.pool_batches(p)


def _check_baf(got, want, what):
    for m in BAF_MATS:
        bad = sorted(set(T.entries_of(got[m]).items()) ^ set(want[m].items()))
        assert not bad, (what, m, bad[:10])


def _check_kept(eng, p, kept, mask=None):
    snp = eng.feature_summary()["snp"]
    assert snp[:, F.S_A:F.S_N + 1].tolist() == [T.tally(p, s, mask) for s in range(len(p.snps))]
    bad = [s for s in range(len(p.snps)) if bool(snp[s, F.S_KEPT]) != kept[s]]
    assert not bad, [(s, T.tally(p, s, mask)) for s in bad]


@KEYS
@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_snp_setting(pool, setting, flags):
    p, raw = pool
    _, min_count, min_maf = setting
    v = R.variant(p.regions, p.snps, min_count=min_count, min_maf=min_maf)
    kept, want = T.snp_expected(p, min_count, min_maf)
    with R.fresh_engine(p.names, v, p.n_cells, T.SNP_FILT, flags | capi.XCK_F_FEATURE_SUMMARY) as eng:
        for b, _ in raw:
            eng.push(b)
        got = eng.finish()
        _check_kept(eng, p, kept)
    print("%s flags=%d: %d of %d SNPs kept" % (setting[0], flags, sum(kept), len(kept)))
    util.assert_coo_equal(got, R.oracle_of(p.names, v, p.n_cells, [b for b, _ in raw], T.SNP_FILT, flags), BAF_MATS)
    _check_baf(got, want, setting[0])


@KEYS
def test_refold_under_every_setting_and_the_mask(pool, flags):
    """one finished handle, no further push: each setting's refold equals the rule and a fresh engine made with it; the masked one
    equals a fresh engine that saw cell = -1 for the disabled cells"""
    p, raw = pool
    first = R.variant(p.regions, p.snps, min_count=SETTINGS[0][1], min_maf=SETTINGS[0][2])
    with R.fresh_engine(p.names, first, p.n_cells, T.SNP_FILT, flags | capi.XCK_F_FEATURE_SUMMARY) as eng:
        for b, _ in raw:
            eng.push(b)
        _check_baf(eng.finish(), T.snp_expected(p, SETTINGS[0][1], SETTINGS[0][2])[1], SETTINGS[0][0])
        for name, min_count, min_maf in SETTINGS[1:] + SETTINGS[:1]:
            v = R.variant(p.regions, p.snps, min_count=min_count, min_maf=min_maf)
            got = R.refold(eng, v)
            kept, want = T.snp_expected(p, min_count, min_maf)
            _check_baf(got, want, name)
            _check_kept(eng, p, kept)
            util.assert_coo_equal(got, R.fresh_result(p.names, v, p.n_cells, [b for b, _ in raw], T.SNP_FILT, flags), BAF_MATS)
        v = R.variant(p.regions, p.snps, min_count=1, min_maf=T.MASK_MAF)
        got = eng.refold(v["regions"], snps=v["snps"], cell_enabled=p.mask, **R.filters_of(v))
        kept, want = T.snp_expected(p, 1, T.MASK_MAF, mask=p.mask)
        _check_baf(got, want, "mask")
        _check_kept(eng, p, kept, p.mask)
        a, b = p.idx["tie_all"], p.idx["tie_enabled"]
        assert (kept[a], kept[b]) == (False, True) and T.snp_expected(p, 1, T.MASK_MAF)[0][a] and not T.snp_expected(p, 1, T.MASK_MAF)[0][b]
        held = K.mask_batches(raw, p.mask)                              # (the holders keep the edited cell arrays alive)
        util.assert_coo_equal(got, R.fresh_result(p.names, v, p.n_cells, [x for x, _ in held], T.SNP_FILT, flags), BAF_MATS)
        del held
        _check_baf(R.refold(eng, v), T.snp_expected(p, 1, T.MASK_MAF)[1], "after the mask")      # the mask was the call's


# ----------------------------------------------------------------------------- both pipelines in one handle
def test_mode_both(pool):
    """the 0.9 include case on contig 1 and the SNP pool on contig 2 through one XCK_MODE_BOTH handle under min_maf 0.1"""
    p, _ = pool
    c = T.case("include_frac_0.9")
    n0 = len(c.regions)
    names = ["1", "2"]
    regions = c.regions + [("2",) + r[1:] for r in p.regions]
    snps = [("2",) + s[1:] for s in p.snps]
    raw = [util.batch_from_dict(d) for d in c.batches] + T.pool_batches(p)
    raw[-1][0].contig = 1
    raw[-1][0].ordinal_base = 1 << 24
    kw = dict(c.filt, min_count=1, min_maf=0.1)
    with Engine(T.BOTH, names, regions, c.n_cells, snps=snps, **kw) as eng:
        for b, _ in raw:
            eng.push(b)
        got = eng.finish()
    exp = {}
    for mode in (T.FC, T.BAF):
        cfg, keep = O.make_config(mode, names, regions, snps if mode == T.BAF else [], c.n_cells, **kw)
        exp.update({k: v for k, v in O.run_oracle(cfg, [b for b, _ in raw]).items() if k in (["count"] if mode == T.FC else BAF_MATS)})
    util.assert_coo_equal(got, exp, ["count"] + BAF_MATS)
    assert T.entries_of(got["count"]) == T.expected_entries(c)[0]
    _, want = T.snp_expected(p, 1, 0.1)
    _check_baf(got, {m: {(s + n0, cell): v for (s, cell), v in want[m].items()} for m in BAF_MATS}, "both")
