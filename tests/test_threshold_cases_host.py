"""The threshold cases on the host (tests/threshold_cases.py): the CPU oracle's matrices equal what the plain-Python rules predict,
every named wrong model of a rule ("mutant") changes the expected matrix of at least one case, every read under test and every
molecule of a tie SNP changes the oracle's answer, and every include shape reaches the path it is named for.  No GPU."""
import numpy as np
import pytest

import join_tile_cases as JT
import oracle as O
import threshold_cases as T
import util

BAF_MATS = ["ad", "dp", "oth"]


def _oracle(c, batches):
    cfg, keep = O.make_config(c.mode, c.names, c.regions, [], c.n_cells, **c.filt)
    held = [util.batch_from_dict(d) for d in batches]
    return O.run_oracle(cfg, [b for b, _ in held])


def _snp_oracle(pool, held, min_count, min_maf):
    cfg, keep = O.make_config(T.BAF, pool.names, pool.regions, pool.snps, pool.n_cells, min_count=min_count, min_maf=min_maf, **T.SNP_FILT)
    return O.run_oracle(cfg, [b for b, _ in held])


# ----------------------------------------------------------------------------- 1. oracle agreement
@pytest.mark.parametrize("name", T.NAMES)
def test_oracle_equals_the_rule(name, oracle_lib):
    """count == the entries include_passes / read_passes predict from the designed (m, n) of every pair; the designed values are
    the ones the batch holds (recomputed from CIGAR and region), every pair of a read that passes the filter is fetched by its
    region, and no region fetches a read it was not built for.  At most 3073 reads."""
    c = T.case(name)
    assert c.n_reads <= T.MAX_READS
    want, n_acc = T.expected_entries(c)
    got = T.entries_of(_oracle(c, c.batches)["count"])
    assert got == want, sorted(set(got.items()) ^ set(want.items()))[:10]
    assert n_acc > 0 and (n_acc < len(c.pairs) or name.endswith("_0"))      # both verdicts occur (a threshold of 0 rejects nothing)
    for p, q in zip(c.pairs, T.paths(c)):
        assert (q.m, q.n) == (p["m"], p["n"]) and (q.fetched or not q.ok), (p["shape"], p["m"], p["n"], q)
    designed = {(p["rec"]["at"], p["row"]) for p in c.pairs}
    fetched = {(at, g) for at, g, _ in T.fetch_outcomes(c)}
    assert fetched <= designed
    # the witness rule: a cell per read (distinct within a tile), a UMI per read
    cells = [int(x) for d in c.batches for x in d["cell"]]
    umis = [int(x) for d in c.batches for x in d["umi"]]
    assert len(set(umis)) == len(umis) and all(len(set(cells[k:k + T.N_CELLS])) == len(cells[k:k + T.N_CELLS]) for k in range(0, len(cells), T.N_CELLS))


@pytest.mark.parametrize("setting", T.snp_settings(), ids=[s[0] for s in T.snp_settings()])
def test_snp_oracle_equals_the_rule(setting, oracle_lib):
    """AD / DP / OTH == what snp_passes keeps of the pool, entry by entry; both verdicts occur among the SNPs with molecules"""
    _, min_count, min_maf = setting
    pool = T.snp_pool()
    kept, want = T.snp_expected(pool, min_count, min_maf)
    got = _snp_oracle(pool, T.pool_batches(pool), min_count, min_maf)
    for m in BAF_MATS:
        assert T.entries_of(got[m]) == want[m], m
    with_reads = [k for s, k in enumerate(kept) if pool.mols[s]]
    assert any(with_reads) and (not all(with_reads) or (min_count <= 1 and min_maf == 0))


def test_snp_mask_variant(oracle_lib):
    """the two mask SNPs sit where they say: on the tie over all cells and off it under the mask, and the other way round; the
    oracle fed cell = -1 for the disabled cells equals the rule over the enabled molecules"""
    import refold_cells_cases as K
    pool = T.snp_pool()
    assert len(pool.reads) <= T.MAX_READS and len({(r[1], r[2]) for r in pool.reads}) == len(pool.reads)      # a (cell, UMI) per molecule
    a, b = pool.idx["tie_all"], pool.idx["tie_enabled"]
    ta, tb = T.tally(pool, a), T.tally(pool, b)
    ma, mb = T.tally(pool, a, pool.mask), T.tally(pool, b, pool.mask)
    assert (ta[1], sum(ta), ma[1], sum(ma)) == (2, 20, 1, 15) and (tb[1], sum(tb), mb[1], sum(mb)) == (2, 25, 2, 20)
    assert a in T.snp_ties(pool, T.MASK_MAF) and b not in T.snp_ties(pool, T.MASK_MAF)
    k_all, _ = T.snp_expected(pool, 1, T.MASK_MAF)
    k_on, want = T.snp_expected(pool, 1, T.MASK_MAF, mask=pool.mask)
    assert (k_all[a], k_on[a], k_all[b], k_on[b]) == (True, False, False, True)
    got = _snp_oracle(pool, K.mask_batches(T.pool_batches(pool), pool.mask), 1, T.MASK_MAF)
    for m in BAF_MATS:
        assert T.entries_of(got[m]) == want[m], m


# ----------------------------------------------------------------------------- 2. mutant kill
def _kill_table(mutants, cases, differs):
    table = {name: [c for c in cases if differs(fn, c)] for name, fn in mutants.items()}
    for name, killers in table.items():
        print("  %-34s killed by %d case(s): %s" % (name, len(killers), ", ".join(killers[:8]) + (" ..." if len(killers) > 8 else "")))
    return table


def test_every_mutant_is_killed():
    """Substituted for the rule, every named mutant changes the expected matrix of at least one case; the table is printed.  The
    multiply form m < f * n changes none (known equivalent for these thresholds and n <= 5000; the large n apart) and is exempt."""
    def inc_differs(fn, name):
        return T.expected_entries(T.case(name), include_fn=fn) != T.expected_entries(T.case(name))

    def read_differs(fn, name):
        return T.expected_entries(T.case(name), read_fn=fn) != T.expected_entries(T.case(name))

    pool = T.snp_pool()
    settings = {s[0]: s for s in T.snp_settings()}

    def snp_differs(fn, sname):
        _, c, f = settings[sname]
        return T.snp_expected(pool, c, f, snp_fn=fn) != T.snp_expected(pool, c, f)

    print("\ninclude rule (rdr/fc/core.py:160-165):")
    inc = _kill_table(T.INCLUDE_MUTANTS, T.INCLUDE_NAMES, inc_differs)
    eq = _kill_table(T.INCLUDE_EQUIVALENT, T.INCLUDE_NAMES, inc_differs)
    print("per-SNP filter (baf/fc/core.py:239-246):")
    snp = _kill_table(T.SNP_MUTANTS, list(settings), snp_differs)
    print("read filter (rdr/fc/core.py:47, :60):")
    rd = _kill_table(T.READ_MUTANTS, T.READ_NAMES, read_differs)
    alive = [k for tab in (inc, snp, rd) for k, v in tab.items() if not v]
    assert alive == [], "no case kills %r" % alive
    # the separators the cases were built around
    assert "include_frac_0.9" in inc["reciprocal"] and "include_frac_0.5" in inc["reciprocal"] and "include_frac_0.05" in inc["reciprocal"]
    assert {"include_frac_0.9", "include_frac_0.5+ulp"} <= set(inc["float32"])
    assert {"include_frac_0.9", "include_frac_0.1", "include_frac_0.2", "include_frac_0.05"} <= set(inc["exact_rational"])
    assert {"include_frac_" + l for l, _ in T.FRACS if l not in ("1e-9", "0.5-ulp", "0.5+ulp")} <= set(inc["le_for_lt"])
    assert {"include_len_" + l for l, _ in T.LENS if l != "29.5"} <= set(inc["le_for_lt"])      # (no integer m ties with 29.5)
    assert inc["trunc_for_ceil"] == ["include_len_29.5"] and "include_frac_0.5+ulp" in inc["bounds_without_divide(not below)"]
    assert {"maf_0.3", "maf_0.15"} <= set(snp["float32"]) and {"maf_0.05", "maf_0.1", "maf_0.2"} <= set(snp["exact_rational"])
    assert snp["trunc_for_ceil"] == ["count_2.5"] and rd["trunc_for_ceil"] == ["min_mapq_19.5"]
    assert set(eq["multiply"]) <= {"include_frac_0.9", "include_frac_0.5+ulp"}          # (only where the large n are)


def test_reciprocal_and_float32_pairs_are_in_the_cases():
    """the pairs the reciprocal and float32 forms get wrong, named in DESIGN.md, are pairs of the cases"""
    def has(name, m, n):
        return any((p["m"], p["n"]) == (m, n) for p in T.case(name).pairs)
    for name, m, n in (("0.9", 99, 110), ("0.9", 198, 220), ("0.5", 49, 98), ("0.5", 98, 196), ("0.5", 103, 206), ("0.1", 7, 70), ("0.1", 11, 110),
                       ("0.2", 7, 35), ("0.2", 11, 55), ("0.05", 7, 140)):
        assert has("include_frac_" + name, m, n), (name, m, n)
        f = dict(T.FRACS)[name]
        assert T.INCLUDE_MUTANTS["reciprocal"](m, n, f) != T.include_passes(m, n, f)
    pool = T.snp_pool()
    tallies = {(min(t[0], t[1]), sum(t)) for t in (T.tally(pool, s) for s in range(len(pool.snps)))}
    assert {(15, 50), (27, 90), (30, 100), (15, 100), (27, 180), (1, 10), (2, 20), (1, 20), (1, 5)} <= tallies


# ----------------------------------------------------------------------------- 3. witness
@pytest.mark.parametrize("name", T.NAMES)
def test_witness(name, oracle_lib):
    """Without any one read that the rule accepts the expected entries differ (a region row and a cell of its own), and the oracle
    follows: checked on the oracle for up to 24 accepted reads per case, spread over the case, every tie among them first."""
    c = T.case(name)
    full, _ = T.expected_entries(c)
    th = c.filt["min_include"]
    acc = [p for p in c.pairs if T.read_passes(p["mapq"], p["n"], c.filt["min_mapq"], c.filt["min_len"]) and T.include_passes(p["m"], p["n"], th)]
    for p in acc:
        assert T.expected_entries(c, skip=p["rec"]["at"])[0] != full
    ties = [p for p in acc if 0 < th < 1 and p["m"] < p["n"] and p["m"] / float(p["n"]) == th]
    for p in JT.spread(ties, 12) + JT.spread(acc, 12):
        at = p["rec"]["at"]
        got = T.entries_of(_oracle(c, JT.without_read(c.batches, at))["count"])
        assert got == T.expected_entries(c, skip=at)[0] != full, (name, p["shape"], p["m"], p["n"])


@pytest.mark.parametrize("label,maf", T.MAFS, ids=[l for l, _ in T.MAFS])
def test_witness_of_tie_snps(label, maf, oracle_lib):
    """every single molecule of a SNP on the tie changes the oracle's output (up to 20 molecules per SNP, ALT ones first)"""
    pool = T.snp_pool()
    ties = T.snp_ties(pool, maf)
    assert ties or label in ("1_3",)                                 # (RN(1/3) * 3 == 1.0 is a tie too, see below)
    _, full = T.snp_expected(pool, 1, maf)
    for s in ties:
        for cell, base, j in pool.mols[s][:20]:
            _, want = T.snp_expected(pool, 1, maf, skip=j)
            assert want != full
            got = _snp_oracle(pool, T.pool_batches(pool, skip=j), 1, maf)
            assert all(T.entries_of(got[m]) == want[m] for m in BAF_MATS), (s, j)


# ----------------------------------------------------------------------------- 4. paths
@pytest.mark.parametrize("name", T.INCLUDE_NAMES)
def test_every_shape_reaches_its_path(name):
    """From the branch conditions of included_len() and join_regions() (threshold_cases.paths): every pair of a shape takes the path
    the shape is named for; a fraction case meets all four outcomes of frac_below's bounds (the 1e-9 case has no m between them);
    the plain wave of shape e is decided by full_ok, the two variants are not and keep every other read's verdict."""
    c = T.case(name)
    ps = T.paths(c)
    seen = {}
    for p, q in zip(c.pairs, ps):
        assert q.ok and q.fetched and q.path in T.path_of(p["shape"]), (p["shape"], p["m"], p["n"], q)
        seen.setdefault(p["shape"], set()).add(q.path)
    th = c.filt["min_include"]
    if 0 < th < 1:
        assert {"a_end", "a_start", "bN_gap", "bN_edge", "bN_block", "bD_gap", "bD_edge", "bD_block", "c_gap", "c_plain", "d_plain", "d_gap", "f_exact",
                "z_no_aligned"} <= set(seen) and {"whole", "block", "walk"} <= set().union(*seen.values())
        assert {q.frac for q in ps} - {None} >= ({"skip", "rej", "acc"} if name.endswith("1e-9") else {"skip", "rej", "acc", "divide"})
        # a tie always goes to the divide: f * n is then within 2^-50 of m
        assert all(q.frac == "divide" for p, q in zip(c.pairs, ps) if p["m"] < p["n"] and p["m"] / float(p["n"]) == th and q.frac)
    else:
        assert seen["e_plain"] == {"wave"} and seen["e_out"] == {"block"} and seen["e_unmapped"] == {"walk"}
        by = {v: [(p["m"], p["n"]) for p in c.pairs if p["shape"] == s] for v, s in (("plain", "e_plain"), ("out", "e_out_in"), ("unmapped", "e_unmapped_in"))}
        assert len(by["plain"]) == 64 and by["out"] == by["plain"][:63] and by["unmapped"] == by["plain"][:63]
        T_ = int(np.ceil(th))
        assert {n for _, n in by["plain"]} == {max(T_ - 1, 0), max(T_, 1)}
