"""The three numeric thresholds of the engine - min_include (fraction and length mode), min_maf / min_count and the read filter's
min_mapq / min_len - at the values where their decisions flip; no GPU, no HIP.  Used by tests/test_threshold_cases_host.py (rule
against the CPU oracle, mutant kill, witness, path check) and tests/test_gpu_thresholds.py (engine against oracle and rule).

The rules are stated once, in Python floats, with the reference's line numbers; next to them stand named wrong models of each rule
("mutants": `<=` for `<`, a reciprocal multiply, float32, an exact-rational compare, truncation for ceil, the total over REF + ALT
only, the minor count over every base, the integer bounds of frac_below without its divide).  The cases are built so that every
mutant changes the expected matrix of at least one of them - the host test fails for a mutant no case kills.

Include cases (basefc), one per threshold: for each aligned length n of a short list - every n <= 120 with an exact tie m / n == f,
the smallest pairs at which a reciprocal multiply differs, a few n with f * n far from an integer, and 4097 / 65537 / 16777217 as
single-M reads for the float32 form - reads with overlap m* - 1, m* and m* + 1 (m* = the smallest accepted m), each in every shape
that reaches the decision by another path of included_len() / join_regions() (shapes(), below).  Witness rule as in
join_tile_cases: every read has a cell (index modulo the prime N_CELLS) and a UMI of its own and every (read, region) pair under
test a region row of its own, so one flipped pair changes one matrix entry.  SNP cases (pileup): one one-base region per SNP, REF on
haplotype 0, ALT on haplotype 1, one read per molecule with its own (cell, UMI); one pool of SNPs built to tallies (minor, total) at
m* - 1 / m* of every min_maf and to totals c - 1 / c of every min_count, judged under each of those settings."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import feature_summary_util as F
import join_tile_cases as JT
import refold_cells_cases as K
from join_tile_cases import D, EQ, FUNMAP, I, M, N, N_CELLS, S, X, build_batches, rec
from xcltk_amd import capi

FC, BAF, BOTH = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF, capi.XCK_MODE_BOTH
MAX_READS = JT.MAX_READS
BASE = {"A": 0, "C": 1, "G": 2, "T": 3}
# the unmapped flag is taken out of the exclusion mask (shape d), min_len 0 lets a read without an aligned base reach the include test
FILT = dict(JT.FILT, min_len=0, excl_flag=768)


# ----------------------------------------------------------------------------- the rules
def include_passes(m, n, min_include):
    """rdr/fc/core.py:160-165: `0 < f < 1` -> the read stays unless m / float(n) < f (:32-37; n == 0 gives None there, the pair is
    dropped - what the oracle does); else it stays unless m < f.  m: aligned bases inside the region, n: aligned bases."""
    if 0 < min_include < 1:
        if n <= 0:
            return False
        return not (m / float(n) < min_include)
    return not (m < min_include)


def snp_passes(tally5, ref, alt, min_count, min_maf):
    """baf/fc/core.py:239-246: out when the total over A, C, G, T, N is below min_count, out when min(REF, ALT) < total * min_maf"""
    t = [int(x) for x in tally5]
    tot = sum(t)
    if tot < min_count:
        return False
    minor = min(t[BASE.get(ref, 4)], t[BASE.get(alt, 4)])
    if minor < tot * min_maf:
        return False
    return True


def read_passes(mapq, n_al, min_mapq, min_len):
    """check_read(), rdr/fc/core.py:47 and :60 (== baf/fc/core.py:19, :32): mapq < min_mapq and len(positions) < min_len drop the read"""
    if mapq < min_mapq:
        return False
    if n_al < min_len:
        return False
    return True


# ----------------------------------------------------------------------------- the mutants
def _frac_only(fn):
    """a wrong model of the fraction rule; length mode and n == 0 as the rule"""
    def g(m, n, f):
        if 0 < f < 1 and n > 0:
            return fn(m, n, f)
        return include_passes(m, n, f)
    return g


def frac_bounds(n, f):
    """frac_bounds() of engine.hip: m < m_rej fails, m >= m_acc passes, between them the divide decides"""
    p = f * float(n)
    return math.ceil(p * (1.0 - 2.0 ** -50)), math.floor(p * (1.0 + 2.0 ** -50)) + 1


def _bounds_const(below):
    """join_regions' `m != n_al && frac_below(..)` with frac_below's last line replaced by the constant `below`"""
    def fn(m, n, f):
        if m == n:
            return True
        m_rej, m_acc = frac_bounds(n, f)
        if m < m_rej:
            return False
        if m >= m_acc:
            return True
        return not below
    return fn


def _exact(m, n, f):
    num, den = f.as_integer_ratio()                                    # the threshold's exact value: m / n < num / den in integers
    return not (m * den < num * n)


INCLUDE_MUTANTS = {
    "le_for_lt": lambda m, n, f: (n > 0 and not (m / float(n) <= f)) if 0 < f < 1 else not (m <= f),
    "reciprocal": _frac_only(lambda m, n, f: not (m * (1.0 / n) < f)),
    "float32": _frac_only(lambda m, n, f: not (np.float32(m) / np.float32(n) < np.float32(f))),
    "exact_rational": _frac_only(_exact),
    "trunc_for_ceil": lambda m, n, f: include_passes(m, n, f) if 0 < f < 1 else not (m < int(f)),
    "bounds_without_divide(below)": _frac_only(_bounds_const(True)),
    "bounds_without_divide(not below)": _frac_only(_bounds_const(False)),
}
# the multiply form m < f * n agrees with the rule for every threshold of the list and n <= 5000: listed, not asked to be killed
INCLUDE_EQUIVALENT = {"multiply": _frac_only(lambda m, n, f: not (m < f * n))}


def _snp_model(tot_of=lambda t, r, a: sum(t), minor_of=lambda t, r, a: min(t[r], t[a]), count_out=lambda tot, c: tot < c,
               maf_out=lambda minor, tot, f: minor < tot * f):
    def fn(tally5, ref, alt, min_count, min_maf):
        t = [int(x) for x in tally5]
        r, a = BASE.get(ref, 4), BASE.get(alt, 4)
        tot = tot_of(t, r, a)
        if count_out(tot, min_count):
            return False
        return not maf_out(minor_of(t, r, a), tot, min_maf)
    return fn


SNP_MUTANTS = {
    "le_for_lt(count)": _snp_model(count_out=lambda tot, c: tot <= c),
    "le_for_lt(maf)": _snp_model(maf_out=lambda minor, tot, f: minor <= tot * f),
    "float32": _snp_model(maf_out=lambda minor, tot, f: np.float32(minor) < np.float32(tot) * np.float32(f)),
    "exact_rational": _snp_model(maf_out=lambda minor, tot, f: minor * float(f).as_integer_ratio()[1] < tot * float(f).as_integer_ratio()[0]),
    "trunc_for_ceil": _snp_model(count_out=lambda tot, c: tot < int(c)),
    "tot_ref_alt_only": _snp_model(tot_of=lambda t, r, a: t[r] + t[a]),
    "minor_over_all_bases": _snp_model(minor_of=lambda t, r, a: sum(t) - max(t)),
}
READ_MUTANTS = {
    "le_for_lt(mapq)": lambda mapq, n_al, q, l: not (mapq <= q) and not (n_al < l),
    "le_for_lt(len)": lambda mapq, n_al, q, l: not (mapq < q) and not (n_al <= l),
    "trunc_for_ceil": lambda mapq, n_al, q, l: not (mapq < int(q)) and not (n_al < l),
}


# ----------------------------------------------------------------------------- include cases
FRACS = [("0.9", 0.9), ("0.5", 0.5), ("0.1", 0.1), ("0.2", 0.2), ("0.3", 0.3), ("0.7", 0.7), ("1_3", 1 / 3), ("2_3", 2 / 3), ("0.05", 0.05),
         ("0.999", 0.999), ("1e-9", 1e-9), ("0.5-ulp", float(np.nextafter(0.5, 0))), ("0.5+ulp", float(np.nextafter(0.5, 1)))]
LENS = [("0", 0), ("1.0", 1.0), ("20", 20), ("29.5", 29.5), ("30", 30), ("91", 91)]
# the smallest n at which m * (1.0 / n) < f differs from the rule, and what else a threshold's list holds beyond its ties
RECIPROCAL_N = {"0.9": [110, 220], "0.5": [98, 196, 206], "0.1": [70, 110], "0.2": [35, 55], "0.05": [140]}
EVEN_N = list(range(2, 41, 2)) + [98, 196]                            # (k, 2k): every one of them flips in float32 under 0.5 + ulp
EXTRA_N = {"0.999": [999, 1000, 2000], "0.5-ulp": EVEN_N, "0.5+ulp": EVEN_N, "1e-9": [100]}
FAR_N = [1, 2, 7, 13, 37, 101]                                        # f * n far from an integer for most thresholds
LARGE_N = {"0.9": [4097, 65537, 16777217], "0.5+ulp": [4097, 65537, 16777217]}      # single-M reads without a stored sequence
GAP = 7


def tie_ns(f, n_max=120):
    """the n <= n_max that have an m with m / float(n) == f in double: the only pairs that separate `<` from `<=`"""
    return [n for n in range(2, n_max + 1) if any(m / float(n) == f for m in range(1, n))]


def m_star(n, th):
    """the smallest m in [0, n] the rule accepts, or None"""
    lo = 0
    if 0 < th < 1 and n > 4096:
        lo = max(int(th * n) - 3, 0)
        assert not include_passes(lo, n, th)
    for m in range(lo, n + 1):
        if include_passes(m, n, th):
            return m
    return None


def shapes(m, n, P):
    """The shapes of a read with n aligned bases at P of which m lie inside its region, by the path they take to the decision:
      a_end / a_start    plain nM cut by the region's end / start: included_len's second shortcut (one aligned block)
      f_exact            the same with m == n: the region ends exactly at endpos, the first shortcut
      bN_* / bD_*        an N / D gap, so that endpos - pos != n_al and the CIGAR walk runs; the region edge inside the gap (_gap), on
                         a block edge (_edge: end of the first block for N, start of the second for D), inside an aligned block
                         (_block), and the region wholly inside the gap (_zero: fetched, m == 0)
      c_gap / c_plain    the same with S, I, =, X mixed in (n_al counts aligned ops only): a start cut inside an N gap, and a read
                         without D / N (span == n_al although the query is longer)
      d_plain / _gap / _zero   unmapped-flagged: fetched by its first base only, m counted over the whole CIGAR
    -> [(shape, CIGAR, flag, s0, e0)] with the region 0-based half-open"""
    out = []
    if 1 <= m <= n:
        out.append(("f_exact" if m == n else "a_end", [(M, n)], 0, P - 3, P + m))
        out.append(("d_plain", [(M, n)], FUNMAP, P - 3, P + m))
    if 1 <= m < n:
        out.append(("a_start", [(M, n)], 0, P + n - m, P + n + 3))
        n1 = max(1, n // 2)
        out.append(("c_plain", [(S, 2), (EQ, n1), (I, 1), (X, n - n1)], 0, P - 3, P + m))
        out.append(("c_gap", [(S, 3), (EQ, n - m), (I, 2), (N, GAP), (X, m), (S, 1)], 0, P + n - m + 4, P + n + GAP + 3))
        out.append(("d_gap", [(M, m), (N, GAP), (M, n - m)], FUNMAP, P - 3, P + m + 3))
        for tag, op in (("bN", N), ("bD", D)):
            cig = [(M, m), (op, GAP), (M, n - m)]
            out.append((tag + "_gap", cig, 0, P - 3, P + m + 3))
            out.append((tag + "_edge", cig, 0, P - 3, P + m if op == N else P + m + GAP))
            if m >= 2:
                out.append((tag + "_block", [(M, m - 1), (op, GAP), (M, n - m + 1)], 0, P - 3, P + m - 1 + GAP + 1))
            elif n >= 3:
                out.append((tag + "_block", [(M, 2), (op, GAP), (M, n - 2)], 0, P - 3, P + 1))
    if m == 0 and n >= 1:
        for tag, op in (("bN", N), ("bD", D)):
            cig = [(M, n // 2), (op, GAP), (M, n - n // 2)] if n >= 2 else [(M, 1), (op, GAP)]
            out.append((tag + "_zero", cig, 0, P + max(n // 2, 1) + 2, P + max(n // 2, 1) + 5))
        out.append(("d_zero", [(N, 5), (M, n)], FUNMAP, P - 2, P + 3))
    return out


PATH_OF = {"a_end": {"block"}, "a_start": {"block"}, "c_plain": {"block"}, "f_exact": {"whole", "wave"}, "f_minus1": {"block"}, "large": {"block", "whole"},
           "z_no_aligned": {"walk"}, "filter": {"whole", "wave", "walk"}, "e_plain": {"wave"}, "e_out_in": {"whole"}, "e_out": {"block"}, "e_unmapped_in": {"whole"},
           "e_unmapped": {"walk"}}


def path_of(shape):
    """the paths a shape is named for (restated by paths() from the branch conditions)"""
    if shape in PATH_OF:
        return PATH_OF[shape]
    return {"walk"}                                                   # b*, c_gap, d_*


class _Builder(object):
    """reads and regions of one basefc case; every pair under test gets a locus and a region row of its own"""

    def __init__(self):
        self.cursor, self.regions, self.pairs, self.groups = 2000, [], [], [[]]

    def locus(self, span):
        P = self.cursor
        self.cursor += max(1000, (span // 100 + 7) * 100)
        return P

    def region(self, s0, e0):
        assert 0 <= s0 < e0
        self.regions.append(("1", s0 + 1, e0, "r%d" % len(self.regions)))
        return len(self.regions) - 1

    def pair(self, shape, cig, flag, s0, e0, m, n, pos, mapq=60, group=0, row=None):
        r = rec(pos, cig, flag=flag, seq=False, ut=True)
        r["mapq"] = mapq
        self.groups[group].append(r)
        self.pairs.append(dict(rec=r, row=self.region(s0, e0) if row is None else row, m=m, n=n, shape=shape, mapq=mapq))
        return r

    def shaped(self, m, n, only=None):
        span = n + GAP + 10
        for shape, cig, flag, s0, e0 in shapes(m, n, 0):
            if only is not None and shape not in only:
                continue
            P = self.locus(span)
            self.pair(shape, cig, flag, P + s0, P + e0, m, n, P)


def _finish(name, b, filt, kind):
    batches, _ = build_batches(b.groups)
    for p in b.pairs:                                                  # (build_batches gives every read mapq 60)
        bi, i = p["rec"]["at"]
        batches[bi]["mapq"][i] = p["mapq"]
    n_reads = sum(len(d["pos"]) for d in batches)
    assert n_reads <= MAX_READS, (name, n_reads)
    return SimpleNamespace(name=name, kind=kind, mode=FC, names=["1"], regions=b.regions, snps=[], n_cells=N_CELLS, batches=batches,
                           filt=dict(FILT, **filt), pairs=b.pairs, n_reads=n_reads)


def include_ns(label, th):
    if 0 < th < 1:
        return sorted(set(tie_ns(th) + RECIPROCAL_N.get(label, []) + EXTRA_N.get(label, []) + FAR_N))
    T = int(math.ceil(th))
    return sorted({n for n in (T - 1, T, T + 1, T + 7, 2 * T + 3) if n >= 1})


def include_case(label, th):
    """One threshold.  Per n: m* - 1, m*, m* + 1 in every shape, m == n at a region that ends exactly at endpos and one that ends at
    endpos - 1 (f_exact, f_minus1), a read without an aligned base; the large n as plain reads; in length mode the three waves of
    shape e, each a batch of its own (a batch starts a tile, its first 64 reads are a wave)."""
    frac = 0 < th < 1
    b = _Builder()
    for n in include_ns(label, th):
        ms = m_star(n, th) if frac else int(math.ceil(th))
        star = [m for m in ((ms - 1, ms, ms + 1) if ms is not None else ()) if 0 <= m <= n]
        for m in star:
            b.shaped(m, n)
        for m, shape in ((n, "f_exact"), (n - 1, "f_minus1")):
            if m not in star and m >= 1:
                P = b.locus(n)
                b.pair(shape, [(M, n)], 0, P - 3, P + m, m, n, P)
    for n in LARGE_N.get(label, []):
        ms = m_star(n, th)
        for m in (ms - 1, ms, ms + 1, n):
            P = b.locus(n)
            b.pair("large", [(M, n)], 0, P - 3, P + m, m, n, P)
            if m < n:
                P = b.locus(n)
                b.pair("large", [(M, n)], 0, P + n - m, P + n + 3, m, n, P)
    P = b.locus(10)
    b.pair("z_no_aligned", [(S, 4)], 0, P - 3, P + 3, 0, 0, P)         # fraction mode: dropped (n == 0); length mode: 0 < f decides
    if not frac:
        T = int(math.ceil(th))
        for variant in ("plain", "out", "unmapped"):
            R0 = b.locus(400)
            row = b.region(R0, R0 + 400)
            b.groups.append([])
            g = len(b.groups) - 1
            for i in range(64):
                n = max(T - 1, 0) if i % 3 == 0 else max(T, 1)         # ceil(threshold) - 1 and ceil(threshold); 0 and 1 under threshold 0
                cig = [(M, n)] if n else [(N, 3)]                      # (no aligned base, yet a reference span of its own: the wave stays all_span)
                pos = R0 + 10 + 2 * i
                if i == 63 and variant == "out":                       # 3 bases beyond the region's end; as much inside as still overlaps
                    m_in = T - 1 if T - 1 >= 1 else max(T, 1)
                    b.pair("e_out", [(M, m_in + 3)], 0, R0, R0 + 400, m_in, m_in + 3, R0 + 400 - m_in, group=g, row=row)
                elif i == 63 and variant == "unmapped":
                    b.pair("e_unmapped", [(M, max(T, 1))], FUNMAP, R0, R0 + 400, max(T, 1), max(T, 1), pos, group=g, row=row)
                else:
                    b.pair("e_plain" if variant == "plain" else "e_%s_in" % variant, cig, 0, R0, R0 + 400, n, n, pos, group=g, row=row)
    return _finish("include_%s_%s" % ("frac" if frac else "len", label), b, dict(min_include=th), "include")


# ----------------------------------------------------------------------------- read-filter cases
MAPQS = [("0", 0), ("19.5", 19.5), ("20", 20), ("255", 255)]
MIN_LENS = [("0", 0), ("1", 1), ("30", 30)]


def mapq_case(label, t):
    """mapq t - 1, t, t + 1 (t = the smallest integer that passes) on 40M reads, each wholly inside a region of its own"""
    b = _Builder()
    T = int(math.ceil(t))
    for q in sorted({q for q in (T - 1, T, T + 1, 0, 255) if 0 <= q <= 255}):
        for _ in range(2):
            P = b.locus(40)
            b.pair("filter", [(M, 40)], 0, P - 3, P + 43, 40, 40, P, mapq=q)
    return _finish("min_mapq_%s" % label, b, dict(min_mapq=t, min_include=0.9), "read")


def min_len_case(label, t):
    """n_al t - 1, t, t + 1 as plain reads and with S / I / D around the aligned blocks (they do not count); min_include 0, so that a
    read without an aligned base is accepted by its region and witnesses min_len 0 against 1"""
    b = _Builder()
    for n in sorted({n for n in (t - 1, t, t + 1) if n >= 0}):
        cigs = [[(M, n)], [(S, 2), (M, n - n // 2), (I, 3), (D, 2), (EQ, n // 2), (S, 1)]] if n >= 2 else [[(M, 1)], [(S, 3), (X, 1), (I, 2)]] if n == 1 \
            else [[(S, 4)], [(I, 2), (D, 3)]]
        for cig in cigs:
            P = b.locus(n + 10)
            b.pair("filter", cig, 0, P - 3, P + n + 10, n, n, P)
    return _finish("min_len_%s" % label, b, dict(min_len=t, min_include=0), "read")


def _builders():
    out = {}
    for label, th in FRACS:
        out["include_frac_" + label] = functools.partial(include_case, label, th)
    for label, th in LENS:
        out["include_len_" + label] = functools.partial(include_case, label, th)
    for label, t in MAPQS:
        out["min_mapq_" + label] = functools.partial(mapq_case, label, t)
    for label, t in MIN_LENS:
        out["min_len_" + label] = functools.partial(min_len_case, label, t)
    return out


NAMES = list(_builders())
INCLUDE_NAMES = [n for n in NAMES if n.startswith("include_")]
READ_NAMES = [n for n in NAMES if not n.startswith("include_")]


@functools.lru_cache(maxsize=None)
def case(name):
    return _builders()[name]()


def expected_entries(c, include_fn=include_passes, read_fn=read_passes, skip=None):
    """{(region row, cell): molecules} of a basefc case under a model of the two rules (every read is a molecule of its own), and the
    number of accepted pairs.  skip: a read (batch, index) left out."""
    f = c.filt
    out, n_acc = {}, 0
    for p in c.pairs:
        if p["rec"]["at"] == skip:
            continue
        if read_fn(p["mapq"], p["n"], f["min_mapq"], f["min_len"]) and include_fn(p["m"], p["n"], f["min_include"]):
            k = (p["row"], p["rec"]["cell"])
            out[k] = out.get(k, 0) + 1
            n_acc += 1
    return out, n_acc


def entries_of(coo):
    return {(int(r), int(cl)): int(v) for r, cl, v in zip(*coo)}


# ---- restatements used by the path check and the summaries
def read_summaries(c):
    return [JT._read_summary(d, c.filt) for d in c.batches]


def paths(c):
    """Per pair under test, from the branch conditions of included_len() and join_regions(): the designed m and n recomputed from the
    batch (JT._included, JT._read_summary), and the path - `wave` (all_span and the region contains the wave's filtered reads: decided
    by full_ok), `whole` (first shortcut), `block` (second shortcut), `walk` - and in fraction mode what frac_below does with it:
    `skip` (m == n_al: not called), `rej` / `acc` (outside the integer bounds), `divide`."""
    rs = read_summaries(c)
    waves = {}
    for bi, v in enumerate(rs):
        for w0 in range(0, len(v), JT.limits().wave):
            ok = [r for r in v[w0:w0 + JT.limits().wave] if r.ok]
            if ok:
                waves[bi, w0 // JT.limits().wave] = (min(r.pos for r in ok), max(r.endpos for r in ok), all(r.span for r in ok))
    th = c.filt["min_include"]
    out = []
    for p in c.pairs:
        bi, i = p["rec"]["at"]
        r = rs[bi][i]
        s0, e0 = c.regions[p["row"]][1] - 1, c.regions[p["row"]][2]
        fetched = r.pos < e0 and r.endpos > s0
        m = JT._included(r, s0, e0)
        path = frac = None
        if r.ok and fetched:
            wmin, wmax, all_span = waves[bi, i // JT.limits().wave]
            if all_span and wmin >= s0 and wmax <= e0:
                path = "wave"
            elif r.span and r.pos >= s0 and r.endpos <= e0:
                path = "whole"
            elif r.span and r.endpos - r.pos == r.n_al:
                path = "block"
            else:
                path = "walk"
            if 0 < th < 1 and r.n_al > 0 and path != "wave":
                m_rej, m_acc = frac_bounds(r.n_al, th)
                frac = "skip" if m == r.n_al else "rej" if m < m_rej else "acc" if m >= m_acc else "divide"
        out.append(SimpleNamespace(ok=r.ok, fetched=fetched, m=m, n=r.n_al, path=path, frac=frac))
    return out


def fetch_outcomes(c):
    """every (read, region) pair of the case that the region fetches, whether under test or not: [((batch, read), row, accepted)],
    through feature_summary_util.read_span / region_outcome"""
    s0 = np.array([r[1] - 1 for r in c.regions], np.int64)
    e0 = np.array([r[2] for r in c.regions], np.int64)
    out = []
    for bi, d in enumerate(c.batches):
        spans = [F.read_span(int(d["pos"][i]), int(d["flag"][i]), int(d["mapq"][i]), int(d["cell"][i]), int(d["umi"][i]),
                             [int(w) for w in d["cigar"][int(d["cig_off"][i]):int(d["cig_off"][i + 1])]], c.filt) for i in range(len(d["pos"]))]
        live = [i for i, s in enumerate(spans) if s is not None]
        pos = np.array([spans[i][0] for i in live], np.int64)
        end = np.array([spans[i][1] for i in live], np.int64)
        ri, gi = np.nonzero((pos[:, None] < e0[None, :]) & (end[:, None] > s0[None, :]))
        for k, g in zip(ri.tolist(), gi.tolist()):
            o = F.region_outcome(spans[live[k]], int(s0[g]), int(e0[g]), c.filt["min_include"])
            assert o is not None
            out.append(((bi, live[k]), g, bool(o)))
    return out


def summary_expect(c):
    """what the three opt-in summaries must say about the include test: per region [include_fail, pairs], per cell
    [include_fail, assigned, pairs], and the read totals (include_fail, assigned, multi, pairs)"""
    reg = np.zeros((len(c.regions), 2), np.int64)
    per_read = {}
    for at, g, acc in fetch_outcomes(c):
        reg[g, 1 if acc else 0] += 1
        a = per_read.setdefault(at, [0, 0])
        a[1 if acc else 0] += 1
    cell = np.zeros((c.n_cells + 1, 3), np.int64)
    tot = dict(include_fail=0, assigned=0, multi=0, pairs=0)
    for (bi, i), (n_fail, n_acc) in per_read.items():
        cl = int(c.batches[bi]["cell"][i])
        if n_acc:
            cell[cl, 1] += 1; cell[cl, 2] += n_acc
            tot["assigned"] += 1; tot["pairs"] += n_acc; tot["multi"] += n_acc >= 2
        else:
            cell[cl, 0] += 1
            tot["include_fail"] += 1
    return reg, cell, tot


# ----------------------------------------------------------------------------- SNP cases
MAFS = [("0.05", 0.05), ("0.1", 0.1), ("0.15", 0.15), ("0.2", 0.2), ("0.3", 0.3), ("1_3", 1 / 3), ("0.5", 0.5)]
COUNTS = [("0", 0), ("1", 1), ("2.5", 2.5), ("6", 6), ("20", 20)]
# totals per min_maf: the ties (1,20) / (1,10), (2,20) / (3,20) / (1,5) / (3,10) / (1,3) / (1,2), the pairs at which float32 differs
# - (15,50), (27,90), (30,100) for 0.3 and (15,100), (27,180) for 0.15 - and totals whose product is far from an integer
MAF_TOTS = {"0.05": [20, 40, 33], "0.1": [10, 20, 37], "0.15": [20, 100, 180, 47], "0.2": [5, 10, 23], "0.3": [10, 50, 90, 100, 33], "1_3": [3, 6, 30, 50],
            "0.5": [2, 4, 50, 31]}
SNP_FILT = dict(K.FILT)
MASK_MAF = 0.1


def maf_star(tot, maf, others=0):
    """the smallest minor count the rule keeps under min_count 1, or None (the minor allele holds at most half of REF + ALT)"""
    for minor in range(0, (tot - others) // 2 + 1):
        if snp_passes([tot - minor - others, minor, others, 0, 0], "A", "C", 1, maf):
            return minor
    return None


def snp_settings():
    """[(name, min_count, min_maf)]: every min_maf under min_count 1, every min_count under min_maf 0"""
    return [("maf_" + l, 1, f) for l, f in MAFS] + [("count_" + l, c, 0) for l, c in COUNTS]


@functools.lru_cache(maxsize=None)
def snp_pool():
    """The SNPs of every setting in one read set (a refold judges the same pileup under each).  SNP s at 1000 + 100 s (1-based) in the
    one-base region s, REF A / ALT C; its molecules are 31M reads that show their base at offset K.SNP_OFF: `alt` C, `ref` A, then G and
    N (nibble 15) molecules that count in the total only.  The last two SNPs are the mask variant: under MASK_MAF `tie_all` is (2, 20)
    over all cells and (1, 15) over the enabled (even) ones, `tie_enabled` (2, 25) over all cells and (2, 20) over the enabled ones.
    -> SimpleNamespace(names, regions, snps, n_cells, reads, mols [per SNP: (cell, base, read index)], mask, idx {name: SNP})"""
    want, seen = [], set()

    def add(minor, tot, others, name=None):
        ref = tot - minor - others
        key = (ref, minor, others)
        if minor < 0 or ref < minor or key in seen:
            return
        seen.add(key)
        want.append((name or "t%d_%d_%d" % (minor, tot, others), ref, minor, others - others // 2, others // 2))

    for label, maf in MAFS:
        for k, tot in enumerate(MAF_TOTS[label]):
            for others in (0, tot // 2) if k < 2 and tot <= 40 else (0,):
                ms = maf_star(tot, maf, others)
                for minor in ((tot - others) // 2,) if ms is None else (ms - 1, ms):
                    add(minor, tot, others)
    for label, c in COUNTS:
        for tot in (int(math.ceil(c)) - 1, int(math.ceil(c))):
            if tot >= 0:
                add(tot // 2, tot, 0)
                add(tot // 6, tot, tot // 2)
    reads, mols, snps, idx = [], [], [], {}

    def molecule(s, base, cell=None):
        j = len(reads)
        cell = j % N_CELLS if cell is None else cell
        reads.append((1000 + 100 * s - 1 - K.SNP_OFF, cell, j, [(31, K.M)], {K.SNP_OFF: 15 if base == "N" else K.NIB[base]}))
        mols[s].append((cell, base, j))

    for name, ref, alt, g, nn in want:
        s = len(snps)
        idx[name] = s
        snps.append(("1", 1000 + 100 * s, "A", "C", 0, 1)); mols.append([])
        for base, k in (("C", alt), ("A", ref), ("G", g), ("N", nn)):
            for _ in range(k):
                molecule(s, base)
    mask = np.arange(N_CELLS) % 2 == 0
    for name, on, off in (("tie_all", "C" + "A" * 14, "C" + "A" * 4), ("tie_enabled", "CC" + "A" * 18, "A" * 5)):
        s = len(snps)
        idx[name] = s
        snps.append(("1", 1000 + 100 * s, "A", "C", 0, 1)); mols.append([])
        for k, base in enumerate(on):
            molecule(s, base, 2 * k + 100 * (s % 5))
        for k, base in enumerate(off):
            molecule(s, base, 2 * k + 1 + 100 * (s % 5))
    assert len(reads) <= MAX_READS, len(reads)
    regions = [("1", sn[1], sn[1], "s%d" % s) for s, sn in enumerate(snps)]
    return SimpleNamespace(names=["1"], regions=regions, snps=snps, n_cells=N_CELLS, reads=reads, mols=mols, mask=mask, idx=idx)


def pool_batches(pool, skip=None):
    """[(Batch, holder)] of the pool's reads (refold_cells_cases._batch: sorted by position, bases as given); skip: a read index left out"""
    reads = [r for j, r in enumerate(pool.reads) if j != skip]
    return [K._batch(reads, np.random.default_rng(5))]


def tally(pool, s, mask=None, skip=None):
    t = [0, 0, 0, 0, 0]
    for cell, base, j in pool.mols[s]:
        if j != skip and (mask is None or mask[cell]):
            t[BASE.get(base, 4)] += 1
    return t


def snp_expected(pool, min_count, min_maf, snp_fn=snp_passes, mask=None, skip=None):
    """-> (kept verdict per SNP, {"ad" / "dp" / "oth": {(row, cell): molecules}}) under a model of the rule: a kept SNP gives its
    region one DP per REF / ALT molecule, one AD per ALT molecule, one OTH per molecule of another base"""
    kept, mats = [], dict(ad={}, dp={}, oth={})
    for s, sn in enumerate(pool.snps):
        ok = bool(snp_fn(tally(pool, s, mask, skip), sn[2], sn[3], min_count, min_maf))
        kept.append(ok)
        if not ok:
            continue
        for cell, base, j in pool.mols[s]:
            if j == skip or (mask is not None and not mask[cell]):
                continue
            for m in (["ad", "dp"] if base == sn[3] else ["dp"] if base == sn[2] else ["oth"]):
                mats[m][s, cell] = mats[m].get((s, cell), 0) + 1
    return kept, mats


def snp_ties(pool, min_maf):
    """the SNPs whose minor count equals total * min_maf in double (minor > 0)"""
    out = []
    for s, sn in enumerate(pool.snps):
        t = tally(pool, s)
        minor = min(t[0], t[1])
        if minor > 0 and float(minor) == sum(t) * min_maf:
            out.append(s)
    return out
