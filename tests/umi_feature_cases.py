"""Cases and the model for the unique-feature molecules of the basefc fold (XCK_F_UNIQUE_FEATURE, include/xck.h);
no GPU.  Used by tests/test_umi_feature_cases_host.py (the model against the pinned oracle, the literal answers of the crafted cases)
and tests/test_gpu_umi_feature.py (the engine against the model).

The rule: a molecule is (contig, cell, UMI code); a (row, cell, UMI) key counts only when its molecule has no other row on that contig.

model() needs no second implementation of the join: every read's cell is relabelled to a dense id of its (batch contig, cell, UMI) -
reads without a cell or without a UMI keep -1 - and the UNCHANGED oracle runs with n_cells = the number of molecules.  The non-zero
pattern of what it returns is exactly the relation rows x molecules, every value 1.  From it: the expected matrix (the entries of the
molecules with one row, summed per (row, original cell)), the four counters, and - the pattern collapsed by cell - the plain matrix,
which tests/test_umi_feature_cases_host.py holds against the oracle run on the reads as they are.

A case is built for a key width (64 or 128 bits: the UMI codes follow the width of the UMI field, layout_cases.expected_layout) and is a
namespace of names (contigs), regions, n_cells, key_bits, umi_bits, batches (batch dicts, in push order) and, for the crafted ones,
`literal`: (matrix {(row, cell): count}, counters) known by construction."""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np

import layout_cases as LC
import oracle as O
from xcltk_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XCK_UMI_NONE = capi.XCK_UMI_NONE
FC = capi.XCK_MODE_BASEFC
KW = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True, min_include=0.9, min_count=1, min_maf=0, no_dup_hap=True)
READ_LEN = LC.READ_LEN
STRIDE = 1000                      # crafted tables: slot i of a contig is [1 + STRIDE * i, STRIDE * (i + 1)]; a read at STRIDE * i + j lies in slot i alone


def tile_size():
    """Keys per block of the heads / distinct / verdict / emit kernels, read from the source."""
    src = open(os.path.join(ROOT, "xcltk_amd", "csrc", "umi_feature.h")).read()
    m = re.search(r"UF_BLOCK\s*=\s*(\d+)\s*,\s*UF_ITEMS\s*=\s*(\d+)", src)
    return int(m.group(1)) * int(m.group(2))


# ----------------------------------------------------------------------------- the model
def _coo(counts):
    items = sorted((k, v) for k, v in counts.items() if v > 0)
    return tuple(np.array([f(x) for x in items], np.int32) for f in (lambda x: x[0][0], lambda x: x[0][1], lambda x: x[1]))


def coo_dict(coo):
    return {(int(r), int(c)): int(v) for r, c, v in zip(*coo)}


def plain_oracle(case):
    cfg, keep = O.make_config(FC, case.names, case.regions, [], case.n_cells, **KW)
    bs = [batch_of(d) for d in case.batches]                             # (batch, the arrays it points into)
    return O.run_oracle(cfg, [b for b, _ in bs])["count"]


def batch_of(d):
    return capi.make_batch(d["contig"], d["ordinal_base"], d["pos"], d["flag"], d["mapq"], d["cell"], d["umi"], d["cig_off"], d["cigar"],
                           d.get("seq_off"), d.get("seq"))


def model(case):
    """-> namespace: count (COO sorted by (row, col)), counters, collapsed (the plain matrix from the same pattern), n_molecules, frac_multi"""
    ids, cell_of = {}, []
    relabelled = []
    for d in case.batches:
        mol = np.full(len(d["cell"]), -1, np.int32)
        for i, (c, u) in enumerate(zip(d["cell"].tolist(), d["umi"].tolist())):
            if c < 0 or u == XCK_UMI_NONE:
                continue
            k = (d["contig"], c, u)
            if k not in ids:
                ids[k] = len(ids); cell_of.append(c)
            mol[i] = ids[k]
        relabelled.append(dict(d, cell=mol))
    cfg, keep = O.make_config(FC, case.names, case.regions, [], max(len(ids), 2), **KW)
    bs = [batch_of(d) for d in relabelled]
    row, col, val = O.run_oracle(cfg, [b for b, _ in bs])["count"]
    assert (val == 1).all()                                              # one (contig, cell, UMI) per column: the pattern is the relation
    rows_of = np.bincount(col, minlength=max(len(ids), 1))
    count, collapsed = {}, {}
    for r, m in zip(row.tolist(), col.tolist()):
        k = (r, cell_of[m])
        collapsed[k] = collapsed.get(k, 0) + 1
        if rows_of[m] == 1:
            count[k] = count.get(k, 0) + 1
    molecules = int((rows_of >= 1).sum()); multi = int((rows_of >= 2).sum())
    counters = dict(molecules=molecules, multi_feature=multi, keys=int(len(row)), keys_dropped=int(rows_of[rows_of >= 2].sum()))
    return SimpleNamespace(count=_coo(count), counters=counters, collapsed=_coo(collapsed), n_molecules=molecules,
                           frac_multi=multi / molecules if molecules else 0.0)


def grouped(coo, cell_group, n_groups):
    """The matrix summed per cell group (cells of group -1 left out) -> COO sorted by (row, group)."""
    out = {}
    for r, c, v in zip(*(a.tolist() for a in coo)):
        g = int(cell_group[c])
        if 0 <= g < n_groups:
            out[(r, g)] = out.get((r, g), 0) + v
    return _coo(out)


# ----------------------------------------------------------------------------- reads
def umi_bits_for(n_regions, n_cells, key_bits):
    kb, ub, _, _ = LC.expected_layout(n_regions, n_cells)
    return 64 if key_bits == 128 else ub


def reads(contig, pos, cell, umi, seed=0, ordinal_base=0):
    """91M reads on contig index `contig` (sorted by position here) -> batch dict"""
    d = LC.plain_reads(np.asarray(pos, np.int64), cell, umi, seed, ordinal_base)
    d["contig"] = contig
    return d


def direct(v, L=8):
    """2-bit code of a UMI of L bases whose bases spell the number v"""
    assert 0 <= v < 4 ** L
    return (1 << (2 * L)) | v


def interned(i, umi_bits):
    """interned id i: the top bit of the UMI field set"""
    assert 0 <= i < LC.intern_id_limit(umi_bits)
    return (1 << (umi_bits - 1)) | i


# ----------------------------------------------------------------------------- crafted cases
def slots(names, per_contig, order=None, dup=(), inverted=()):
    """Region table of per_contig slots on every contig of `names`, given in `order` (a permutation of range(len(names) * per_contig) over
    the (contig, slot) pairs in contig-major order; None: that order).  dup: pairs that get a second entry with the same interval at the
    END of the table; inverted: pairs whose entry is given with end < start - 1 (it never enters the join's table).
    -> regions, row_of {(contig index, slot): [rows]}"""
    pairs = [(c, s) for c in range(len(names)) for s in range(per_contig)]
    if order is not None:
        pairs = [pairs[i] for i in order]
    pairs += list(dup)
    regions, row_of = [], {}
    for row, (c, s) in enumerate(pairs):
        lo, hi = 1 + STRIDE * s, STRIDE * (s + 1)
        if (c, s) in inverted:
            regions.append((names[c], hi, lo - 5, "inv%d" % row))
            continue
        regions.append((names[c], lo, hi, "g%d" % row))
        row_of.setdefault((c, s), []).append(row)
    return regions, row_of


def crafted(name, key_bits, names, regions, row_of, n_cells, hits, n_batches=1, extra_batches=()):
    """hits: (contig index, slot, cell, umi code) - one read each, wholly inside that slot.  The reads of a contig go into n_batches
    batches (round robin, each sorted by position); extra_batches: further lists of hits, one batch per (contig of a) list, pushed
    behind the others.  -> the case, with `literal` worked out from the hits alone: a hit puts its (cell, UMI) on every row of its
    slot, a molecule counts where it is on one row only."""
    batches = []
    def add(hs, seed):
        for c in sorted({h[0] for h in hs}):
            sel = [h for h in hs if h[0] == c]
            # (offset inside the slot: anywhere the 91-base read stays inside [STRIDE * s, STRIDE * (s + 1)))
            batches.append(reads(c, [STRIDE * s + (7 * i) % (STRIDE - READ_LEN) for i, (_, s, _, _) in enumerate(sel)], [h[2] for h in sel], [h[3] for h in sel],
                                 seed, ordinal_base=len(batches) << 20))
    for b in range(n_batches):
        part = hits[b::n_batches]
        if part:
            add(part, b)
    for k, hs in enumerate(extra_batches):
        add(list(hs), 100 + k)
    rows = {}
    for c, s, cell, umi in list(hits) + [h for hs in extra_batches for h in hs]:
        if cell < 0 or umi == XCK_UMI_NONE:
            continue
        rows.setdefault((c, cell, umi), set()).update(row_of.get((c, s), []))
    rows = {k: v for k, v in rows.items() if v}
    count = {}
    for (c, cell, umi), rs in rows.items():
        if len(rs) == 1:
            k = (next(iter(rs)), cell)
            count[k] = count.get(k, 0) + 1
    counters = dict(molecules=len(rows), multi_feature=sum(len(v) > 1 for v in rows.values()), keys=sum(len(v) for v in rows.values()),
                    keys_dropped=sum(len(v) for v in rows.values() if len(v) > 1))
    return SimpleNamespace(name=name, names=names, regions=regions, n_cells=n_cells, key_bits=key_bits,
                           umi_bits=umi_bits_for(len(regions), n_cells, key_bits), batches=batches, literal=(count, counters))


def _tile_pair(kb):
    """A two-row molecule whose keys are the last of one tile and the first of the next: one cell, T - 1 one-row molecules with smaller
    UMI codes in front (D is sorted by cell | UMI | rank), the pair at D[T - 1] and D[T], a few hundred one-row molecules behind."""
    T = tile_size(); names = ["1"]
    regions, ro = slots(names, 6)
    hits = [(0, u % 6, 0, direct(u)) for u in range(T - 1)] + [(0, 2, 0, direct(T - 1)), (0, 4, 0, direct(T - 1))] + [(0, u % 6, 0, direct(u)) for u in range(T, T + 300)]
    c = crafted("tile_pair", kb, names, regions, ro, 2, hits, n_batches=2)
    assert c.literal[1] == dict(molecules=T + 300, multi_feature=1, keys=T + 301, keys_dropped=2)
    return c


def _tile_run(kb):
    """One key repeated 40 times across the tile boundary of the sorted stream: T - 18 one-row molecules in front, then the same read in 40
    batches of its own (one tile each, so every copy reaches HBM, through every shard slice), then one-row molecules behind."""
    T = tile_size(); names = ["1"]
    regions, ro = slots(names, 4)
    front = [(0, u % 4, 0, direct(u)) for u in range(T - 18)]
    back = [(0, u % 4, 0, direct(u)) for u in range(T, T + 200)]
    c = crafted("tile_run", kb, names, regions, ro, 1, front + back, extra_batches=[[(0, 1, 0, direct(T - 18))]] * 40)
    assert c.literal[1] == dict(molecules=T - 18 + 200 + 1, multi_feature=0, keys=T - 18 + 200 + 1, keys_dropped=0)
    return c


def _first_last(kb):
    """The first and the last key of D belong to two-row molecules (smallest cell and UMI; largest cell and UMI), one-row molecules between."""
    names = ["1"]; regions, ro = slots(names, 5)
    hits = [(0, 0, 0, direct(0)), (0, 1, 0, direct(0))] + [(0, u % 5, 1 + u % 2, direct(u)) for u in range(1, 200)] + [(0, 3, 3, direct(65535)), (0, 4, 3, direct(65535))]
    c = crafted("first_last", kb, names, regions, ro, 4, hits)
    assert c.literal[1] == dict(molecules=201, multi_feature=2, keys=203, keys_dropped=4)
    return c


def _one_key(kb):
    names = ["1"]; regions, ro = slots(names, 3)
    c = crafted("one_key", kb, names, regions, ro, 2, [(0, 1, 1, direct(77))])
    assert c.literal == ({(1, 1): 1}, dict(molecules=1, multi_feature=0, keys=1, keys_dropped=0))
    return c


def _no_hits(kb):
    """Reads without a cell, without a UMI, and outside every region: nothing is accepted."""
    names = ["1"]; regions, ro = slots(names, 3)
    c = crafted("no_hits", kb, names, regions, ro, 2, [(0, 1, -1, direct(1)), (0, 1, 0, XCK_UMI_NONE), (0, 7, 0, direct(2)), (0, 9, 1, direct(3))])
    assert c.literal == ({}, dict(molecules=0, multi_feature=0, keys=0, keys_dropped=0))
    return c


def _all_dropped(kb):
    names = ["1"]; regions, ro = slots(names, 4)
    hits = [(0, s, u % 3, direct(u)) for u in range(150) for s in (u % 4, (u + 1) % 4)]
    c = crafted("all_dropped", kb, names, regions, ro, 3, hits, n_batches=2)
    assert c.literal == ({}, dict(molecules=150, multi_feature=150, keys=300, keys_dropped=300))
    return c


def _none_dropped(kb):
    names = ["1", "2"]; regions, ro = slots(names, 4)
    hits = [(u % 2, u % 4, u % 5, direct(u)) for u in range(300)]
    c = crafted("none_dropped", kb, names, regions, ro, 5, hits, n_batches=2)
    assert c.literal[1] == dict(molecules=300, multi_feature=0, keys=300, keys_dropped=0)
    return c


def _same_umi_two_cells(kb):
    """UMI 5 in cell 0 on row 0 and in cell 1 on row 2: two molecules, both kept.  UMI 6 in cell 0 on rows 0 and 2: dropped."""
    names = ["1"]; regions, ro = slots(names, 3)
    c = crafted("same_umi_two_cells", kb, names, regions, ro, 2, [(0, 0, 0, direct(5)), (0, 2, 1, direct(5)), (0, 0, 0, direct(6)), (0, 2, 0, direct(6))])
    assert c.literal == ({(0, 0): 1, (2, 1): 1}, dict(molecules=3, multi_feature=1, keys=4, keys_dropped=2))
    return c


def _two_contigs(kb):
    """The same (cell, UMI) on the last slot of contig 1 and the first slot of contig 2 - neighbouring ranks, two molecules, both kept;
    another on two slots of contig 2 and one of contig 1: the contig-1 key stays, the two of contig 2 drop."""
    names = ["1", "2"]; regions, ro = slots(names, 3)
    hits = [(0, 2, 0, direct(9)), (1, 0, 0, direct(9)), (0, 1, 1, direct(4)), (1, 0, 1, direct(4)), (1, 2, 1, direct(4))]
    c = crafted("two_contigs", kb, names, regions, ro, 2, hits)
    assert c.literal == ({(2, 0): 1, (3, 0): 1, (1, 1): 1}, dict(molecules=4, multi_feature=1, keys=5, keys_dropped=2))
    return c


def _dup_interval(kb):
    """Slot 1 is in the table twice (rows 1 and 3): whatever it accepts is on two rows and drops; the other slots keep theirs."""
    names = ["1"]; regions, ro = slots(names, 3, dup=[(0, 1)])
    hits = [(0, 1, 0, direct(1)), (0, 1, 1, direct(2)), (0, 0, 0, direct(3)), (0, 2, 1, direct(1))]
    c = crafted("dup_interval", kb, names, regions, ro, 2, hits)
    assert ro[(0, 1)] == [1, 3] and c.literal == ({(0, 0): 1, (2, 1): 1}, dict(molecules=4, multi_feature=2, keys=6, keys_dropped=4))
    return c


def _three_rows(kb):
    names = ["1"]; regions, ro = slots(names, 4)
    c = crafted("three_rows", kb, names, regions, ro, 2, [(0, 0, 1, direct(8)), (0, 1, 1, direct(8)), (0, 3, 1, direct(8)), (0, 2, 1, direct(10))])
    assert c.literal == ({(2, 1): 1}, dict(molecules=2, multi_feature=1, keys=4, keys_dropped=3))
    return c


def _shuffled_order(kb):
    """Two contigs, 8 slots each, the table given slot-descending with the contigs interleaved (rank != row for every row); molecules on
    one slot, on two slots of one contig, and on one slot of each contig."""
    names = ["1", "2"]; n = 8
    order = [c * n + s for s in range(n - 1, -1, -1) for c in (1, 0)]
    regions, ro = slots(names, n, order=order)
    hits = []
    for u in range(120):
        c, s, cell = u % 2, (3 * u) % n, u % 3
        hits.append((c, s, cell, direct(u)))
        if u % 3 == 1:
            hits.append((c, (s + 1 + u % 5) % n, cell, direct(u)))       # a second slot of the same contig (never the same slot: 1 + u % 5 < 8)
        if u % 3 == 2:
            hits.append((1 - c, s, cell, direct(u)))                     # the other contig: a molecule of its own
    c = crafted("shuffled_order", kb, names, regions, ro, 3, hits, n_batches=3)
    assert ro[(0, 0)] == [15] and ro[(1, 7)] == [0] and c.literal[1] == dict(molecules=160, multi_feature=40, keys=200, keys_dropped=80)
    return c


def _inverted_region(kb):
    """Slot 1 is given inverted (row 1 exists but never enters the join's table): its reads count nowhere, the ranks of the rows behind
    it are one less than their rows, and a molecule on slots 0 and 2 still drops."""
    names = ["1"]; regions, ro = slots(names, 4, inverted=[(0, 1)])
    hits = [(0, 1, 0, direct(1)), (0, 0, 0, direct(2)), (0, 2, 0, direct(2)), (0, 3, 1, direct(1)), (0, 1, 1, direct(1)), (0, 2, 1, direct(7))]
    c = crafted("inverted_region", kb, names, regions, ro, 2, hits)
    assert c.literal == ({(3, 1): 1, (2, 1): 1}, dict(molecules=3, multi_feature=1, keys=4, keys_dropped=2))
    return c


def _interned_mix(kb):
    """Interned codes (top bit of the UMI field set; the smallest and the largest id) beside 2-bit codes, the same low bits in both
    codings: no two of them are one molecule."""
    names = ["1"]; regions, ro = slots(names, 4); ub = umi_bits_for(4, 3, kb)
    top = LC.intern_id_limit(ub) - 1
    hits = [(0, 0, 0, interned(0, ub)), (0, 1, 0, interned(0, ub)),              # dropped
            (0, 0, 1, interned(top, ub)), (0, 2, 2, interned(top, ub)),          # two cells: kept
            (0, 3, 0, direct(5)), (0, 2, 0, interned(direct(5), ub)),            # two codings: kept
            (0, 1, 2, direct(6)), (0, 3, 2, direct(6)),                          # dropped
            (0, 1, 1, LC.umi_codes(ub, ("direct_t",))["direct_t"])]              # the widest 2-bit code
    c = crafted("interned_mix", kb, names, regions, ro, 3, hits)
    assert c.literal == ({(0, 1): 1, (2, 2): 1, (3, 0): 1, (2, 0): 1, (1, 1): 1}, dict(molecules=7, multi_feature=2, keys=9, keys_dropped=4))
    return c


def _repeated_batches(kb):
    """Every key arrives five times: the same hits in five batches per contig, pushed one after the other (different tiles, so different
    shard slices, and different launches when the queue is flushed between them)."""
    names = ["1", "2"]; regions, ro = slots(names, 5)
    hits = []
    for u in range(90):
        c, s, cell = u % 2, u % 5, u % 4
        hits.append((c, s, cell, direct(u)))
        if u % 2:
            hits.append((c, (s + 2) % 5, cell, direct(u)))
    c = crafted("repeated_batches", kb, names, regions, ro, 4, hits, extra_batches=[hits] * 4)
    assert c.literal[1] == dict(molecules=90, multi_feature=45, keys=135, keys_dropped=90)
    return c


CRAFTED = dict(tile_pair=_tile_pair, tile_run=_tile_run, first_last=_first_last, one_key=_one_key, no_hits=_no_hits, all_dropped=_all_dropped,
               none_dropped=_none_dropped, same_umi_two_cells=_same_umi_two_cells, two_contigs=_two_contigs, dup_interval=_dup_interval,
               three_rows=_three_rows, shuffled_order=_shuffled_order, inverted_region=_inverted_region, interned_mix=_interned_mix,
               repeated_batches=_repeated_batches)


# ----------------------------------------------------------------------------- generated cases
GENERATED = {"gen_s1": (1, 6000, 4 ** 3), "gen_s2": (2, 5000, 4 ** 5), "gen_s3": (3, 8000, 4 ** 8), "gen_s4": (4, 7000, 4 ** 4)}   # seed, reads, UMI pool
CONTIG_LEN = 100000


def generated(name, key_bits, with_snps=False):
    """Two contigs of 100 kb.  Table: 60 genes (30 per contig, 400 .. 2000 bases) given in reverse order with the contigs interleaved, then
    2 kb bins over both contigs, a second entry for one gene's interval and a gene nested in another.  Reads: molecules of 1 .. 5 reads
    within 40 bases of an anchor, (cell, UMI) drawn from 24 cells x the pool - a small pool makes the same (cell, UMI) turn up at far
    places of a contig and on both contigs.  One read in 25 has no cell, one in 25 no UMI.  Every contig's reads go into two batches."""
    seed, n_reads, pool = GENERATED[name]
    rng = np.random.default_rng(seed)
    names = ["1", "2"]; n_cells = 24
    genes = []
    for c in names:
        st = rng.integers(1, CONTIG_LEN - 2500, 30)
        genes += [(c, int(s), int(s + rng.integers(400, 2001)), "gene") for s in st]
    genes.sort(key=lambda g: -g[1])                                      # descending start: reverse coordinate order, the contigs mixed
    genes = genes[0::2] + genes[1::2]
    bins = [(c, s, s + 1999, "bin") for c in names for s in range(1, CONTIG_LEN, 2000)]
    g0, g1 = genes[7], genes[20]
    regions = genes + bins + [(g0[0], g0[1], g0[2], "dup"), (g1[0], g1[1] + 50, g1[2] - 50, "nested")]
    umi_bits = umi_bits_for(len(regions), n_cells, key_bits)
    per = {0: [], 1: []}
    n = 0
    while n < n_reads:
        k = int(rng.integers(1, 6)); c = int(rng.integers(0, 2))
        anchor = int(rng.integers(0, CONTIG_LEN - 200)); cell = int(rng.integers(0, n_cells)); u = direct(int(rng.integers(0, pool)))
        for _ in range(k):
            r = int(rng.integers(0, 25))
            per[c].append((anchor + int(rng.integers(0, 41)), -1 if r == 0 else cell, XCK_UMI_NONE if r == 1 else u))
        n += k
    batches = []
    for c in (0, 1):
        recs = per[c]
        for half in (recs[0::2], recs[1::2]):
            batches.append(reads(c, [x[0] for x in half], [x[1] for x in half], [x[2] for x in half], seed + len(batches), ordinal_base=len(batches) << 24))
    snps = []
    if with_snps:
        for ci, c in enumerate(names):
            for p in range(40, CONTIG_LEN, 211):
                r = (p // 211 + ci) & 3
                snps.append((c, p, "ACGT"[r], "ACGT"[(r + 1 + (p // 633) % 3) & 3], (p // 211) & 1, 1 - ((p // 211) & 1)))
    return SimpleNamespace(name=name, names=names, regions=regions, n_cells=n_cells, key_bits=key_bits, umi_bits=umi_bits, batches=batches,
                           literal=None, snps=snps)


ALL = tuple(CRAFTED) + tuple(GENERATED)


@functools.lru_cache(maxsize=None)
def case(name, key_bits):
    return CRAFTED[name](key_bits) if name in CRAFTED else generated(name, key_bits)


@functools.lru_cache(maxsize=None)
def case_model(name, key_bits):
    """The model of a case, computed once and shared (nobody changes it)."""
    return model(case(name, key_bits))
