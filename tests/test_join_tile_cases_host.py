"""The join's per-tile limit cases on the host (tests/join_tile_cases.py): the capacities read from the source, the model's facts for
every case, the side of the limit it is on - and the witness: the CPU oracle's answer without any single read under test differs
from its answer with it, so a join that loses that read's pair cannot pass tests/test_gpu_join_tiles.py.  No GPU."""
import numpy as np
import pytest

import join_tile_cases as JT
import oracle as O
import util

MATS = {JT.FC: ["count"], JT.BAF: ["ad", "dp", "oth"]}


def _oracle(c, batches):
    kw = dict(JT.FILT); kw.update(c.filt)
    cfg, keep = O.make_config(c.mode, c.names, c.regions, c.snps if c.mode == JT.BAF else [], c.n_cells, **kw)
    held = [util.batch_from_dict(d) for d in batches]
    return O.run_oracle(cfg, [b for b, _ in held])


def _same(a, b, mats):
    return all(len(a[k][0]) == len(b[k][0]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])) for k in mats)


def test_limits_are_found_and_derived():
    """Every number of the limit table is found in the source, and the capacities JoinSmem derives from them
    are the documented ones."""
    L = JT.limits()
    assert (L.cx_cap, L.cg_cap, L.cg_cap_baf, L.st_cap, L.st_win) == (128, 1536, 1408, 256, 64)
    assert (L.join_block, L.tile_items, L.tile, L.wave, L.waves, L.park_slots) == (256, 4, 1024, 64, 4, 64)
    assert (L.bqueue_bytes, L.nqueue_bytes, L.bqcap, L.nqcap) == (3072, 3072, 192, 192)
    assert (L.hs_bytes, L.hs_slots, L.probes, L.qcap_fc128, L.qcap_baf128) == (16384, 2048, 24, 1024, 256)
    assert (L.gap_piece, L.ws_snp) == (32, 10)
    assert JT.N_CELLS > L.tile and all(JT.N_CELLS % q for q in range(2, 33))


def test_every_limit_has_its_three_sides():
    """The case list holds limit - 1, the limit and limit + 1 of every capacity (names are built from limits())."""
    for stem, vals in (("cx_%d", (127, 128, 129, 1024)), ("st_snp_k0+%d", (255, 256, 257)), ("win_%d", (63, 64, 65)), ("bhits_%d", (191, 192, 193)),
                       ("nrec_%d", (191, 192, 193)), ("sweep128_%d", (255, 256, 257)), ("batch_%d", (1, 255, 256, 257, 1023, 1024, 1025, 2049)),
                       ("fc_st_e0+%d", (255, 256, 257)), ("fc_keys_%d", (2047, 2048, 2049)), ("fc_sweep128_%d", (1023, 1024, 1025))):
        assert all(stem % v in JT.NAMES for v in vals), stem


@pytest.mark.parametrize("name", JT.NAMES)
def test_facts_and_side(name):
    """The model gives the case's facts, and the second paths the input takes are exactly the ones the case names (with 64-bit keys;
    with 128-bit keys where the case says so).  Structure: at most 3073 reads and 16 reads under test, cells and UMIs distinct within
    every tile except for shadows, every hit without a base of a read under test shadowed by a later read with a base there."""
    c = JT.case(name)
    L = JT.limits()
    tiles, pairs = JT.model(c.mode, c.names, c.regions, c.snps, c.batches, c.filt)
    assert len(tiles) <= 3 or len(c.batches) > 1
    assert sum(len(d["pos"]) for d in c.batches) <= JT.MAX_READS and 0 < len(c.under_test) <= JT.MAX_UNDER_TEST
    for t, kv in c.facts.items():
        for k, v in kv.items():
            assert tiles[t][k] == v, "%s: tile %d %s = %r, expected %r" % (name, t, k, tiles[t][k], v)
    assert JT.crossed(c.mode, tiles) == c.crosses, name
    if c.crosses128 is not None:
        t128, pairs128 = JT.model(c.mode, c.names, c.regions, c.snps, c.batches, c.filt, JT.F128)
        assert pairs128 == pairs and c.crosses128 <= JT.crossed(c.mode, t128) and "q128" not in JT.crossed(c.mode, t128) - c.crosses128
    if "cg" in c.crosses:
        beyond = {at for t in tiles for at in t["beyond_cap"]}
        assert set(c.under_test) & beyond and ("over" not in name or set(c.under_test) <= beyond)
    # pairs that only the include test rejects: not accepted by the model, although the read passed the filter, is accepted by another
    # region (so it is live) and has the aligned bases a shortcut asks for before it emits the whole wave
    if name.startswith("fc_contain"):
        assert len(c.not_accepted) >= 4
    if c.not_accepted:
        f = dict(JT.FILT); f.update(c.filt)
        rs = [JT._read_summary(d, f) for d in c.batches]
        accepted = {p for t in tiles for p in t["accepted"]}
        for at, row in c.not_accepted:
            r = rs[at[0]][at[1]]
            assert (at, row) not in accepted and any(a == at for a, _ in accepted)
            assert r.ok and (r.n_al > 0 if 0.0 < f["min_include"] < 1.0 else r.n_al >= f["min_include"])
    # cells and UMIs
    seen = {}
    for bi, d in enumerate(c.batches):
        for i in range(len(d["pos"])):
            seen.setdefault((int(d["cell"][i]), int(d["umi"][i])), []).append((bi, i))
    own = {at for v in seen.values() if len(v) == 1 for at in v}
    first = {v[0]: v[1:] for v in seen.values()}
    for bi, d in enumerate(c.batches):
        for r0 in range(0, len(d["pos"]), L.tile):
            cells = [int(d["cell"][i]) for i in range(r0, min(r0 + L.tile, len(d["pos"]))) if (bi, i) in own or (bi, i) in first]
            assert len(set(cells)) == len(cells)
    # shadows
    if c.mode == JT.BAF:
        f = dict(JT.FILT); f.update(c.filt)
        rs = [JT._read_summary(d, f) for d in c.batches]
        p0, _ = JT._snp_table(c.snps, c.names, 0, L.ws_snp)
        for at in c.under_test:
            base, nobase, gaps = JT._read_snps(rs[at[0]][at[1]], p0)
            dark = nobase + [k for a, b in gaps for k in range(a, b)]
            assert base or dark, "a read under test meets a SNP"
            lit = set()
            for sb, si in first.get(at, []):
                assert (sb, si) > at
                lit |= set(JT._read_snps(rs[sb][si], p0)[0])
            assert set(dark) <= lit, "%s: read %r has hits without a base and no shadow" % (name, at)


@pytest.mark.parametrize("name", JT.NAMES)
def test_witness(name, oracle_lib):
    """Zero blind reads: for every read under test, the oracle's matrices without it differ from the full ones.  The model's accepted
    pairs are checked against the oracle on the way: basefc counts one per pair (every read is a molecule of its own), the pileup one
    per hit with a base whose molecule holds no earlier hit at that SNP."""
    c = JT.case(name)
    mats = MATS[c.mode]
    full = _oracle(c, c.batches)
    tiles, pairs = JT.model(c.mode, c.names, c.regions, c.snps, c.batches, c.filt)
    if c.mode == JT.FC:
        assert int(full["count"][2].sum()) == pairs == sum(t["distinct_keys"] for t in tiles)
    else:
        f = dict(JT.FILT); f.update(c.filt)
        p0, _ = JT._snp_table(c.snps, c.names, 0, JT.limits().ws_snp)
        holder, n_base, n_all = {}, 0, 0
        for d in c.batches:
            for r in JT._read_summary(d, f):
                if r.ok:
                    base, nobase, gaps = JT._read_snps(r, p0)
                    n_base += len(base); n_all += len(base) + len(nobase) + sum(b - a for a, b in gaps)
                    for k in nobase + [k for a, b in gaps for k in range(a, b)]:
                        holder.setdefault((k, r.cell, r.umi), 0)
                    for k in base:
                        holder.setdefault((k, r.cell, r.umi), 1)
        assert n_all == pairs and n_base == sum(t["base_hits"] for t in tiles)
        assert int(full["dp"][2].sum()) + int(full["oth"][2].sum()) == sum(holder.values()) > 0
    blind = [at for at in c.under_test if _same(full, _oracle(c, JT.without_read(c.batches, at)), mats)]
    assert blind == [], "%s: the result does not change without reads %r" % (name, blind)
