"""Cases and the model for the 1-mismatch UMI collapsing of the basefc fold (XCK_F_UMI_COLLAPSE, include/xck.h);
no GPU.  Used by tests/test_umi_dedup_cases_host.py (the model against the pinned oracle, the literal answers of the crafted cases) and
tests/test_gpu_umi_dedup.py (the engine against the model).

The rule: within one (row, cell) two distinct UMI key codes are adjacent when both are direct 2-bit codes of the same length that
differ in exactly one base; the matrix value is the number of connected components.  Interned codes are adjacent to nothing.

model() reuses the trick of umi_feature_cases.model: every read's cell is relabelled to a dense id of its (contig, cell, UMI) and the
UNCHANGED oracle runs; the non-zero pattern of what it returns is the relation rows x (cell, UMI).  The components of every (row, cell)
come from a plain union-find over the substitution neighbours of its codes; with unique_feature=True the keys of the molecules on two
or more rows leave the pattern first (the order the engine documents).

A case is a namespace of names, regions, n_cells, key_bits, umi_bits, batches and, for the crafted ones, `literal`: (matrix {(row,
cell): count}, counters) known by construction - and `literal_uf`, the same under XCK_F_UNIQUE_FEATURE, where the case has one."""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np

import layout_cases as LC
import oracle as O
import umi_feature_cases as UF
from xcltk_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XCK_UMI_NONE = capi.XCK_UMI_NONE
FC, KW, STRIDE, READ_LEN = UF.FC, UF.KW, UF.STRIDE, UF.READ_LEN
direct, interned, batch_of, plain_oracle, coo_dict, grouped, umi_bits_for = UF.direct, UF.interned, UF.batch_of, UF.plain_oracle, UF.coo_dict, UF.grouped, UF.umi_bits_for
FIELDS = ("keys", "molecules", "groups", "groups_changed", "opaque_keys", "max_group")


def _const(name):
    src = open(os.path.join(ROOT, "xcltk_amd", "csrc", "umi_collapse.h")).read()
    return int(re.search(r"constexpr int %s\s*=\s*(\d+)\s*;" % name, src).group(1))


def small_limit():
    """Largest group of the tile path (k_uc_small), read from the source."""
    return _const("UC_SMALL")


def medium_limit():
    """Largest group whose union-find runs in LDS (k_uc_big), read from the source."""
    return _const("UC_MEDIUM")


def tile_size():
    src = open(os.path.join(ROOT, "xcltk_amd", "csrc", "umi_collapse.h")).read()
    m = re.search(r"UC_BLOCK\s*=\s*(\d+)\s*,\s*UC_ITEMS\s*=\s*(\d+)", src)
    return int(m.group(1)) * int(m.group(2))


# ----------------------------------------------------------------------------- the rule, twice
def is_opaque(u, umi_bits):
    return bool((u >> (umi_bits - 1)) & 1)


def adjacent(a, b, umi_bits):
    """The pairwise test as the issue states it."""
    if is_opaque(a, umi_bits) or is_opaque(b, umi_bits) or a == 0 or b == 0 or a.bit_length() != b.bit_length():
        return False
    x = a ^ b
    return bin((x | (x >> 1)) & 0x5555555555555555).count("1") == 1


def neighbours(u):
    """The 3L codes one substitution away from the direct code u of L bases."""
    L = (u.bit_length() - 1) // 2
    return [u ^ (d << (2 * f)) for f in range(L) for d in (1, 2, 3)]


def components(umis, umi_bits, pairwise=False):
    """Number of connected components of the adjacency graph over the distinct codes `umis`."""
    us = sorted(set(umis))
    idx = {u: i for i, u in enumerate(us)}
    parent = list(range(len(us)))
    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]; x = parent[x]
        return x
    for i, u in enumerate(us):
        if pairwise:
            near = [j for j in range(i) if adjacent(u, us[j], umi_bits)]
        else:
            near = [] if is_opaque(u, umi_bits) or u == 0 else [idx[v] for v in neighbours(u) if v in idx]
        for j in near:
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return sum(1 for i in range(len(us)) if find(i) == i)


# ----------------------------------------------------------------------------- the model
def model(case, unique_feature=False, pairwise=False):
    """-> namespace: count (COO sorted by (row, col)), counters, exact (the matrix without collapsing, from the same pattern),
    groups {(row, cell): [codes]}, frac_changed (of the groups with two or more keys)"""
    ids, cell_of, umi_of = {}, [], []
    relabelled = []
    for d in case.batches:
        mol = np.full(len(d["cell"]), -1, np.int32)
        for i, (c, u) in enumerate(zip(d["cell"].tolist(), d["umi"].tolist())):
            if c < 0 or u == XCK_UMI_NONE:
                continue
            k = (d["contig"], c, u)
            if k not in ids:
                ids[k] = len(ids); cell_of.append(c); umi_of.append(u)
            mol[i] = ids[k]
        relabelled.append(dict(d, cell=mol))
    cfg, keep = O.make_config(FC, case.names, case.regions, [], max(len(ids), 2), **KW)
    bs = [batch_of(d) for d in relabelled]
    row, col, val = O.run_oracle(cfg, [b for b, _ in bs])["count"]
    assert (val == 1).all()
    rows_of = np.bincount(col, minlength=max(len(ids), 1))
    groups = {}
    for r, m in zip(row.tolist(), col.tolist()):
        if unique_feature and rows_of[m] != 1:
            continue
        groups.setdefault((r, cell_of[m]), set()).add(umi_of[m])
    count = {k: components(v, case.umi_bits, pairwise) for k, v in groups.items()}
    exact = {k: len(v) for k, v in groups.items()}
    multi = [k for k in groups if exact[k] >= 2]
    changed = [k for k in multi if count[k] < exact[k]]
    counters = dict(keys=sum(exact.values()), molecules=sum(count.values()), groups=len(groups), groups_changed=len(changed),
                    opaque_keys=sum(is_opaque(u, case.umi_bits) for v in groups.values() for u in v), max_group=max(exact.values(), default=0))
    return SimpleNamespace(count=UF._coo(count), counters=counters, exact=UF._coo(exact), groups=groups,
                           frac_changed=len(changed) / len(multi) if multi else 0.0, n_multi=len(multi))


# ----------------------------------------------------------------------------- crafted cases
def build(name, kb, n_slots, n_cells, hits, literal, n_batches=1, extra_batches=(), literal_uf=None, regions=None, names=("1",)):
    """hits: (contig index, slot, cell, umi code) - one read each, wholly inside slot `slot` of the table of UF.slots (row = slot on a
    one-contig table), or - `regions` given - (contig index, position, cell, umi code)."""
    names = list(names)
    if regions is None:
        regions, row_of = UF.slots(names, n_slots)
        c = UF.crafted(name, kb, names, regions, row_of, n_cells, list(hits), n_batches=n_batches, extra_batches=extra_batches)
        batches = c.batches
    else:
        batches = []
        for b in range(n_batches):
            part = list(hits)[b::n_batches]
            for ci in sorted({h[0] for h in part}):
                sel = [h for h in part if h[0] == ci]
                batches.append(UF.reads(ci, [h[1] for h in sel], [h[2] for h in sel], [h[3] for h in sel], b, ordinal_base=len(batches) << 20))
    return SimpleNamespace(name=name, names=names, regions=regions, n_cells=n_cells, key_bits=kb, umi_bits=umi_bits_for(len(regions), n_cells, kb),
                           batches=batches, literal=literal, literal_uf=literal_uf)


def counters(keys, molecules, groups, groups_changed, opaque_keys, max_group):
    return dict(keys=keys, molecules=molecules, groups=groups, groups_changed=groups_changed, opaque_keys=opaque_keys, max_group=max_group)


def parity_code(L):
    """All UMIs of L bases whose base sum is 0 mod 4, as numbers, ascending: any two differ in at least two bases."""
    v = np.arange(4 ** L, dtype=np.int64)
    s = np.zeros_like(v)
    for f in range(L):
        s += (v >> (2 * f)) & 3
    return v[(s & 3) == 0].tolist()


def _pair_last_base(kb):
    """Two codes that differ in the last base: neighbours in sort order; unrelated codes around them."""
    A = 0b0110110001101100
    hits = [(0, 0, 0, direct(A)), (0, 0, 0, direct(A ^ 1)), (0, 0, 0, direct(A ^ 0b0101 << 4)), (0, 0, 0, direct(77))]
    return build("pair_last_base", kb, 2, 2, hits, ({(0, 0): 3}, counters(4, 3, 1, 1, 0, 4)))


def _pair_first_base(kb):
    """Two codes that differ in the first base, eleven unrelated codes between them in sort order."""
    A = 0b0010110001101100
    mid = [A + 16 * 5 * k + 5 for k in range(1, 12)]                      # (each differs from A and from A ^ top in two or more bases, and from each other)
    hits = [(0, 0, 0, direct(A)), (0, 0, 0, direct(A ^ (3 << 14)))] + [(0, 0, 0, direct(m)) for m in mid]
    return build("pair_first_base", kb, 2, 2, hits, None)                 # (literal filled in below, once the spacing of `mid` is asserted)


def _distance2(kb):
    A = 0b1110010011100100
    hits = [(0, 1, 1, direct(A)), (0, 1, 1, direct(A ^ 0b0101))]
    return build("distance2", kb, 2, 2, hits, ({(1, 1): 2}, counters(2, 2, 1, 0, 0, 2)))


def _chain_abc(kb):
    """A - B - C with A and C two bases apart: one component."""
    A = 0b1110010011100100
    hits = [(0, 1, 0, direct(A)), (0, 1, 0, direct(A ^ 1)), (0, 1, 0, direct(A ^ 1 ^ (2 << 6)))]
    return build("chain_abc", kb, 2, 1, hits, ({(1, 0): 1}, counters(3, 1, 1, 1, 0, 3)))


def staircase(L=8, start=0):
    """An induced path of 3L + 1 codes: base f goes 0 -> 1 for f = 0 .. L-1, then 1 -> 2, then 2 -> 3.  Code i and code j differ in
    |i - j| bases' worth of steps: adjacent exactly when |i - j| = 1."""
    v, out = start, [start]
    for sweep in range(3):
        for f in range(L):
            v += 1 << (2 * f)
            out.append(v)
    return out


def _staircase(kb):
    path = staircase()
    hits = [(0, 0, 1, direct(v)) for v in path]
    return build("staircase", kb, 1, 2, hits, ({(0, 1): 1}, counters(25, 1, 1, 1, 0, 25)), n_batches=2)


def _length_confusion(kb):
    """X of 7 bases and C.X of 8 bases: the codes differ in one 2-bit field (the leading one moves), and must not merge; Y of 7 bases
    one substitution from X does."""
    x = 0b01101100011011
    X, CX = direct(x, 7), direct((1 << 14) | x, 8)
    assert X ^ CX == 1 << 16
    hits = [(0, 0, 0, X), (0, 0, 0, CX), (0, 0, 0, direct(x ^ 2, 7))]
    return build("length_confusion", kb, 1, 1, hits, ({(0, 0): 2}, counters(3, 2, 1, 1, 0, 3)))


def _opaque_confusion(kb):
    """Two interned ids that differ in one 2-bit field; an interned id whose low bits equal a direct code of the group (the XOR is the top
    bit alone); a direct pair beside them that does merge."""
    ub = umi_bits_for(2, 2, kb)
    d5 = direct(0b0110110001101100)
    hits = [(0, 0, 0, interned(8, ub)), (0, 0, 0, interned(8 ^ 4, ub)), (0, 0, 0, interned(d5, ub)), (0, 0, 0, d5), (0, 0, 0, d5 ^ 2)]
    return build("opaque_confusion", kb, 2, 2, hits, ({(0, 0): 4}, counters(5, 4, 1, 1, 3, 5)))


def _split_cells_rows(kb):
    """The same adjacent pair split across two cells, and across two rows: nothing merges.  The pair whole in (2, 2): merges."""
    A = direct(0b1001110001101100)
    hits = [(0, 0, 0, A), (0, 0, 1, A ^ 1), (0, 1, 0, A), (0, 2, 0, A ^ 1), (0, 2, 2, A), (0, 2, 2, A ^ 1)]
    return build("split_cells_rows", kb, 3, 3, hits, ({(0, 0): 1, (0, 1): 1, (1, 0): 1, (2, 0): 1, (2, 2): 1}, counters(6, 5, 5, 1, 0, 2)))


def _group_boundary(kb):
    """The last key of one group is one substitution from the first key of the next (cell 0 -> cell 1, and row 0 -> row 1): no merge."""
    hits = [(0, 0, 0, direct(5)), (0, 0, 0, direct(100)), (0, 0, 1, direct(101)), (0, 0, 1, direct(300)), (0, 1, 0, direct(301)), (0, 1, 0, direct(900))]
    return build("group_boundary", kb, 2, 2, hits, ({(0, 0): 2, (0, 1): 2, (1, 0): 2}, counters(6, 6, 3, 0, 0, 2)))


def _sized_group(n, code, L):
    """n codes of one group with n - 1 components: n - 1 words of the parity code, of which the first has a partner that differs from it
    in the last base; the other L - 1 code words next to that partner are left out."""
    w0 = code[0]
    partner = w0 ^ 1
    shun = set(neighbours(direct(partner, L))) - {direct(w0, L)}
    words = [w for w in code if direct(w, L) not in shun][:n - 1]
    assert len(words) == n - 1 and words[0] == w0
    return [direct(w, L) for w in words] + [direct(partner, L)]


def _class_limits(kb):
    """Groups of 1, 2 and limit - 1, limit, limit + 1 keys for both class limits, one per cell; every group of two or more keys holds
    exactly one adjacent pair."""
    S, M = small_limit(), medium_limit()
    code = parity_code(8)
    sizes = [1, 2, S - 1, S, S + 1, M - 1, M, M + 1]
    hits, count = [], {}
    for cell, n in enumerate(sizes):
        umis = [direct(code[3])] if n == 1 else _sized_group(n, code, 8)
        hits += [(0, 0, cell, u) for u in umis]
        count[(0, cell)] = max(n - 1, 1)
    return build("class_limits", kb, 1, len(sizes), hits, (count, counters(sum(sizes), sum(count.values()), len(sizes), len(sizes) - 1, 0, M + 1)), n_batches=3)


def _straddle(name, kb, in_front, tail):
    """Filler groups of three non-adjacent keys (cells 0, 1, ...) put `in_front` keys ahead of the group `tail` in D, which therefore
    starts at index in_front of D.  tail: the codes of one group; filler groups behind it."""
    code = parity_code(8)
    hits, count, cell = [], {}, 0
    left = in_front
    while left > 0:
        k = min(3, left)
        hits += [(0, 0, cell, direct(w)) for w in code[10:10 + k]]
        count[(0, cell)] = k; cell += 1; left -= k
    hits += [(0, 0, cell, u) for u in tail]
    target = cell; cell += 1
    for _ in range(40):
        hits += [(0, 0, cell, direct(w)) for w in code[20:23]]
        count[(0, cell)] = 3; cell += 1
    return hits, count, target, cell


def _tile_edge_pair(kb):
    """A group of two adjacent keys at D[T - 1] and D[T]: each key's only partner lies in the other tile."""
    T = tile_size()
    A = direct(0b1001110001101100)
    hits, count, target, n_cells = _straddle("tile_edge_pair", kb, T - 1, [A, A ^ 3])
    count[(0, target)] = 1
    n_keys = T - 1 + 2 + 120
    return build("tile_edge_pair", kb, 1, n_cells, hits, (count, counters(n_keys, n_keys - 1, len(count), 1, 0, 3)), n_batches=2)


def _tile_edge_path(kb):
    """The staircase path of 25 keys with 9 keys in one tile and 16 in the next."""
    T = tile_size()
    hits, count, target, n_cells = _straddle("tile_edge_path", kb, T - 9, [direct(v) for v in staircase()])
    count[(0, target)] = 1
    n_keys = T - 9 + 25 + 120
    return build("tile_edge_path", kb, 1, n_cells, hits, (count, counters(n_keys, n_keys - 24, len(count), 1, 0, 25)), n_batches=2)


def _complete(L):
    def make(kb):
        hits = [(0, 0, 0, direct(v, L)) for v in range(4 ** L)] + [(0, 0, 1, direct(3, L)), (0, 0, 1, direct(3 ^ 0b0101, L))]
        return build("complete%d" % L, kb, 1, 2, hits, ({(0, 0): 1, (0, 1): 2}, counters(4 ** L + 2, 3, 2, 1, 0, 4 ** L)), n_batches=2)
    return make


def _parity(L):
    """The whole parity code of L bases in one group - nothing merges - and in a second group with one key off the code, which joins the L
    code words around it: size - L + 1 components."""
    def make(kb):
        code = parity_code(L)
        n = len(code)
        assert n == 4 ** (L - 1)
        off = code[n // 2] ^ 2
        hits = [(0, 0, 0, direct(w, L)) for w in code] + [(0, 0, 1, direct(w, L)) for w in code] + [(0, 0, 1, direct(off, L))]
        lit = {7: (4096, 4090), 8: (16384, 16377)}[L]
        assert lit == (n, n - L + 1)
        return build("parity%d" % L, kb, 1, 2, hits, ({(0, 0): lit[0], (0, 1): lit[1]}, counters(2 * n + 1, lit[0] + lit[1], 2, 1, 0, n + 1)), n_batches=4)
    return make


def _repeated(kb):
    """Every key arrives five times, in batches of their own (other tiles, so other shard slices)."""
    A = 0b1001110001101100
    hits = []
    for cell in range(4):
        for k in range(12):
            hits.append((0, k % 2, cell, direct(A + 85 * k)))             # (85 = 0b1010101: four bases change per step)
        hits.append((0, 0, cell, direct(A ^ (1 + cell % 3))))             # one partner of A in row 0
    c = build("repeated", kb, 2, 4, hits, None, extra_batches=[hits] * 4)
    count = {(r, cell): 6 for r in (0, 1) for cell in range(4)}
    c.literal = (count, counters(4 * 13, 4 * 12, 8, 4, 0, 7))
    return c


def _no_hits(kb):
    hits = [(0, 1, -1, direct(1)), (0, 1, 0, XCK_UMI_NONE), (0, 7, 0, direct(2))]
    return build("no_hits", kb, 3, 2, hits, ({}, counters(0, 0, 0, 0, 0, 0)), literal_uf=({}, counters(0, 0, 0, 0, 0, 0)))


def _one_key(kb):
    return build("one_key", kb, 3, 2, [(0, 1, 1, direct(77))], ({(1, 1): 1}, counters(1, 1, 1, 0, 0, 1)), literal_uf=({(1, 1): 1}, counters(1, 1, 1, 0, 0, 1)))


def _with_unique_feature(kb):
    """Rows 1 and 2 overlap.  UMI u is accepted by both, u' - one substitution from u - by row 1 only.  Unique-feature first: u leaves both
    rows, u' stays: row 1 counts 1, row 2 nothing.  (Collapsing first would leave one molecule in row 1 and u in row 2 - both on u, so
    both dropped.)  Without the unique-feature rule: one component in row 1, one key in row 2.  Row 0 holds an untouched pair."""
    regions = [("1", 1, 1000, "g0"), ("1", 1001, 2000, "g1"), ("1", 1501, 2500, "g2")]
    u = direct(0b1001110001101100)
    v = u ^ (0b0101 << 8)
    hits = [(0, 1600, 0, u), (0, 1100, 0, u ^ 1), (0, 100, 0, v), (0, 200, 0, v ^ 2)]
    return build("with_unique_feature", kb, 0, 2, hits, ({(0, 0): 1, (1, 0): 1, (2, 0): 1}, counters(5, 3, 3, 2, 0, 2)),
                 literal_uf=({(0, 0): 1, (1, 0): 1}, counters(3, 2, 2, 1, 0, 2)), regions=regions)


def _all_dropped_upstream(kb):
    """Every molecule lies on two rows: under XCK_F_UNIQUE_FEATURE nothing reaches the collapsing stage."""
    regions = [("1", 1001, 2000, "g1"), ("1", 1501, 2500, "g2")]
    u = direct(0b1001110001101100)
    hits = [(0, 1600, 0, u), (0, 1650, 1, u ^ 1)]
    return build("all_dropped_upstream", kb, 0, 2, hits, ({(0, 0): 1, (1, 0): 1, (0, 1): 1, (1, 1): 1}, counters(4, 4, 4, 0, 0, 1)),
                 literal_uf=({}, counters(0, 0, 0, 0, 0, 0)), regions=regions)


def _fix_pair_first_base(make):
    def f(kb):
        c = make(kb)
        us = sorted(int(u) for d in c.batches for u in d["umi"].tolist())
        A = direct(0b0010110001101100)
        assert us[0] == A and us[-1] == A ^ (3 << 14) and len(us) == 13
        c.literal = ({(0, 0): 12}, counters(13, 12, 1, 1, 0, 13))
        return c
    return f


CRAFTED = dict(pair_last_base=_pair_last_base, pair_first_base=_fix_pair_first_base(_pair_first_base), distance2=_distance2, chain_abc=_chain_abc,
               staircase=_staircase, length_confusion=_length_confusion, opaque_confusion=_opaque_confusion, split_cells_rows=_split_cells_rows,
               group_boundary=_group_boundary, class_limits=_class_limits, tile_edge_pair=_tile_edge_pair, tile_edge_path=_tile_edge_path,
               complete3=_complete(3), complete4=_complete(4), complete6=_complete(6), parity7=_parity(7), parity8=_parity(8), repeated=_repeated,
               no_hits=_no_hits, one_key=_one_key, with_unique_feature=_with_unique_feature, all_dropped_upstream=_all_dropped_upstream)
WITH_UF = ("with_unique_feature", "all_dropped_upstream", "no_hits", "one_key")


# ----------------------------------------------------------------------------- generated cases
GENERATED = {"gen_p3": (11, 5000, 3), "gen_p4": (12, 6000, 4), "gen_p5": (13, 7000, 5)}   # seed, reads, bases of the UMI (pool 4^L)
CONTIG_LEN = 100000


def generated(name, key_bits, with_snps=False):
    """Two contigs of 100 kb; 40 genes of 2 .. 8 kb (they overlap here and there), given in reverse order.  Reads: molecules of 1 .. 4 reads
    within 40 bases of an anchor, (cell, UMI) drawn from 12 cells x a pool of 4^L UMIs of L bases - small, so that the UMIs of a (gene,
    cell) are often one substitution apart.  One read in 25 has no cell, one in 25 no UMI, one in 25 an interned UMI.  Two batches per contig."""
    seed, n_reads, L = GENERATED[name]
    rng = np.random.default_rng(seed)
    names = ["1", "2"]; n_cells = 12
    genes = []
    for c in names:
        st = rng.integers(1, CONTIG_LEN - 9000, 20)
        genes += [(c, int(s), int(s + rng.integers(2000, 8001)), "gene") for s in st]
    genes.sort(key=lambda g: -g[1])
    regions = genes
    snps = []
    if with_snps:
        for ci, c in enumerate(names):
            for p in range(40, CONTIG_LEN, 211):
                r = (p // 211 + ci) & 3
                snps.append((c, p, "ACGT"[r], "ACGT"[(r + 1 + (p // 633) % 3) & 3], (p // 211) & 1, 1 - ((p // 211) & 1)))
    umi_bits = umi_bits_for(max(len(regions), len(snps)), n_cells, key_bits)   # (a handle with a pileup pipeline sizes the row field for the SNPs as well)
    per = {0: [], 1: []}
    n = 0
    while n < n_reads:
        k = int(rng.integers(1, 5)); c = int(rng.integers(0, 2))
        anchor = int(rng.integers(0, CONTIG_LEN - 200)); cell = int(rng.integers(0, n_cells)); u = direct(int(rng.integers(0, 4 ** L)), L)
        for _ in range(k):
            r = int(rng.integers(0, 25))
            per[c].append((anchor + int(rng.integers(0, 41)), -1 if r == 0 else cell, XCK_UMI_NONE if r == 1 else interned(int(rng.integers(0, 50)), umi_bits) if r == 2 else u))
        n += k
    batches = []
    for c in (0, 1):
        recs = per[c]
        for half in (recs[0::2], recs[1::2]):
            batches.append(UF.reads(c, [x[0] for x in half], [x[1] for x in half], [x[2] for x in half], seed + len(batches), ordinal_base=len(batches) << 24))
    return SimpleNamespace(name=name, names=names, regions=regions, n_cells=n_cells, key_bits=key_bits, umi_bits=umi_bits, batches=batches,
                           literal=None, literal_uf=None, snps=snps)


ALL = tuple(CRAFTED) + tuple(GENERATED)


@functools.lru_cache(maxsize=None)
def case(name, key_bits):
    return CRAFTED[name](key_bits) if name in CRAFTED else generated(name, key_bits)


@functools.lru_cache(maxsize=None)
def case_model(name, key_bits, unique_feature=False):
    """The model of a case, computed once and shared (nobody changes it)."""
    return model(case(name, key_bits), unique_feature)
