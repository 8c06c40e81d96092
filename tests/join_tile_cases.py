"""Inputs that sit at limit - 1, at the limit and at limit + 1 of every per-tile capacity of k_join (xcltk_amd/csrc/engine.hip), with a
model of the tile that says on which side a case lies; no GPU, no HIP.  Used by tests/test_join_tile_cases_host.py (the model, the
facts and the witness on the CPU oracle) and tests/test_gpu_join_tiles.py (engine against oracle).

The join stages per tile of 1024 reads a slice of the CIGAR words, of the regions / SNPs and of the SNP windows, sets spliced reads
aside, parks (read, SNP) pairs per wave and queues its output in LDS; each of these is "a cache, never a correctness assumption", i.e.
has a second, rarely taken path behind it.  limits() reads the capacities out of the source (a changed default moves the cases with
it), model() restates k_tile_meta, load_read and the counting side of pileup_sweep / pileup_complex / join_regions in plain Python,
and crossed() names the second paths an input takes.  Every case follows the witness rule: each read has a cell (index modulo the prime
N_CELLS, so distinct within a tile) and a UMI of its own, pileup cases have one one-base region per SNP (REF on haplotype 0, ALT on
haplotype 1, min_count 1, min_maf 0), basefc cases have (read, region) pairs with rows of their own - so a single lost pair changes a
matrix.  The exception are hits without a base (SNP inside an N / D gap, read without sequence or CIGAR): such a hit shows only
through a later read of the same (cell, UMI) WITH a base there, whose base then stays uncounted; every such SNP of a read under test
has that shadow read."""
import bisect
import functools
import os
import re
from types import SimpleNamespace

import numpy as np

from xcltk_amd import capi

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "xcltk_amd", "csrc")
M, I, D, N, S, H, EQ, X = 0, 1, 2, 3, 4, 5, 7, 8
FC, BAF = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF
F128 = capi.XCK_F_FORCE_KEY128
FUNMAP = 4
N_CELLS = 1031                    # prime, above the tile size: index % N_CELLS is distinct within any tile
UMI0 = 1 << 30                    # UMI code of read i of a case: UMI0 | i (a direct 2-bit code of 15 bases)
REF, ALT = "A", "C"
FILT = dict(min_mapq=20, min_len=1, incl_flag=0, excl_flag=772, no_orphan=True, min_include=0.9, min_count=1, min_maf=0, no_dup_hap=True)
MAX_READS = 3073
MAX_UNDER_TEST = 16


# ----------------------------------------------------------------------------- the capacities, from the source
def _int(text, pattern):
    m = re.search(pattern, text)
    assert m, "not found in the engine's source: %s" % pattern
    return int(m.group(1))


@functools.lru_cache(maxsize=None)
def limits():
    """The defaults of engine.hip (integers only) and what JoinSmem derives from them."""
    with open(os.path.join(CSRC, "engine.hip")) as fp:
        eng = fp.read()
    with open(os.path.join(CSRC, "engine_impl.h")) as fp:
        impl = fp.read()
    d = lambda name: _int(eng, r"#define\s+%s\s+(\d+)\b" % name)
    c = lambda text, name: _int(text, r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name)
    L = SimpleNamespace(ws_snp=d("XCK_WS_SNP"), tile_items=d("XCK_TILE_ITEMS"), nqueue_bytes=d("XCK_BAF_NQUEUE_BYTES"),
                        bqueue_bytes=d("XCK_BAF_BQUEUE_BYTES"), cx_cap=d("XCK_CX_CAP"), hs_bytes=d("XCK_HS_BYTES"), cg_cap=d("XCK_CG_CAP"),
                        cg_cap_baf=d("XCK_CG_CAP_BAF"), st_cap=d("XCK_ST_CAP"), st_win=c(eng, "ST_WIN"), join_block=c(impl, "JOIN_BLOCK"),
                        wave=_int(eng, r"wcnt\[JOIN_BLOCK\s*/\s*(\d+)\]"), probes=_int(eng, r"probe\s*<\s*(\d+)\s*;"),
                        gap_piece=_int(eng, r"ks\s*\+=\s*(\d+)\s*\)"), baf_queue_bytes=_int(eng, r"XCK_BAF_BQUEUE_BYTES\s*:\s*(\d+)\s*\)"),
                        park_slots=_int(eng, r"pr_n\s*\+\s*n_new\s*>\s*(\d+)\s*\)"))
    L.tile = L.join_block * L.tile_items                     # TILE
    L.hs_slots = L.hs_bytes // 8                              # HS_SLOTS: the 64-bit key set of basefc
    L.qcap_fc128 = L.hs_bytes // 16                           # QCAP, basefc with 128-bit keys (no value)
    L.qcap_baf128 = L.baf_queue_bytes // (16 + 8)             # QCAP, pileup with 128-bit keys (key + value)
    L.bqcap = L.bqueue_bytes // (8 + 8)                       # QCAP, pileup split mode: hits with a base
    L.nqcap = L.nqueue_bytes // 16                            # NQCAP, pileup split mode: records without a base
    L.waves = L.join_block // L.wave
    return L


# ----------------------------------------------------------------------------- records -> batch dicts
def rec(pos, cig, flag=0, seq=True, shadow_of=None, ut=False):
    """One read: 0-based position, CIGAR [(op, len)], flag; seq=False: no sequence stored; shadow_of: an earlier rec whose (cell, UMI)
    this read shares; ut: the read is under test."""
    return dict(pos=pos, cig=list(cig), flag=flag, seq=seq, shadow_of=shadow_of, ut=ut)


def fill(n, pos, cig=((M, 12),)):
    return [rec(pos, cig) for _ in range(n)]


def build_batches(groups, contig=0, sort=True):
    """groups: one list of recs per batch (ordinals run on from batch to batch).  Reads are sorted by position inside a batch (stable;
    sort=False keeps the given order).  Read i of the case gets cell i % N_CELLS and UMI UMI0 | i, a shadow the (cell, UMI) of its
    target, which must come earlier.  -> batch dicts, under_test [(batch, read)]"""
    out, under, base = [], [], 0
    for bi, recs in enumerate(groups):
        if sort:
            recs = sorted(recs, key=lambda r: r["pos"])
        cw, sq, cig_off, seq_off, cell, umi = [], [], [0], [0], [], []
        for i, r in enumerate(recs):
            r["at"] = (bi, i)
            if r["shadow_of"] is None:
                r["cell"], r["umi"] = (base + i) % N_CELLS, UMI0 | (base + i)
            else:
                t = r["shadow_of"]
                assert "cell" in t and t["at"] < (bi, i), "a shadow comes after its target"
                r["cell"], r["umi"] = t["cell"], t["umi"]
            cell.append(r["cell"]); umi.append(r["umi"])
            cw += [(l << 4) | op for op, l in r["cig"]]; cig_off.append(len(cw))
            qlen = sum(l for op, l in r["cig"] if op in (M, I, S, EQ, X)) if r["seq"] else 0
            nib = (1 << np.random.default_rng(base + i).integers(0, 4, qlen + (qlen & 1))).astype(np.uint8)
            sq.append((nib[0::2] << 4) | nib[1::2]); seq_off.append(seq_off[-1] + len(sq[-1]))
            if r["ut"]:
                under.append((bi, i))
        n = len(recs)
        out.append(dict(contig=contig, ordinal_base=base, pos=np.array([r["pos"] for r in recs], np.int32),
                        flag=np.array([r["flag"] for r in recs], np.uint16), mapq=np.full(n, 60, np.uint8), cell=np.array(cell, np.int32),
                        umi=np.array(umi, np.uint64), cig_off=np.array(cig_off, np.uint32), cigar=np.array(cw + [0], np.uint32),
                        seq_off=np.array(seq_off, np.uint32), seq=np.concatenate(sq + [np.zeros(1, np.uint8)])))
        base += n
    return out, under


def spread(items, k=MAX_UNDER_TEST):
    """At most k of the items, evenly spread, first and last among them."""
    items = list(items)
    if len(items) <= k:
        return items
    return [items[(len(items) - 1) * j // (k - 1)] for j in range(k)]


def mark(recs, k=MAX_UNDER_TEST):
    for r in spread(recs, k):
        r["ut"] = True


def snp_rows(p0s):
    """SNPs at these 0-based positions (sorted, distinct) and one one-base region per SNP."""
    p0s = sorted(set(p0s))
    snps = [("1", p + 1, REF, ALT, 0, 1) for p in p0s]
    return [("1", p + 1, p + 1, "s%d" % k) for k, p in enumerate(p0s)], snps


# ----------------------------------------------------------------------------- the model
def _read_summary(d, f):
    """load_read(): filter, reference length, aligned bases, span_is_cigar, endpos, simple - per read of a batch."""
    n = len(d["pos"])
    out = []
    for i in range(n):
        flag, pos = int(d["flag"][i]), int(d["pos"][i])
        c0, c1 = int(d["cig_off"][i]), int(d["cig_off"][i + 1])
        ok = int(d["mapq"][i]) >= f["min_mapq"]
        ok = ok and not (f["excl_flag"] and (flag & f["excl_flag"])) and not (f["incl_flag"] and not (flag & f["incl_flag"]))
        ok = ok and not (f["no_orphan"] and (flag & 1) and not (flag & 2))
        ok = ok and int(d["cell"][i]) >= 0 and int(d["umi"][i]) != capi.XCK_UMI_NONE
        cig = [(int(w) & 15, int(w) >> 4) for w in d["cigar"][c0:c1]]
        rlen = sum(l for op, l in cig if op in (M, D, N, EQ, X))
        n_al = sum(l for op, l in cig if op in (M, EQ, X))
        span = not ((flag & FUNMAP) or c1 == c0 or rlen == 0)
        if not span:
            rlen = 1
        ok = ok and n_al >= f["min_len"]
        out.append(SimpleNamespace(ok=ok, pos=pos, endpos=pos + rlen, n_al=n_al, span=span, cig=cig, c0=c0, c1=c1,
                                   simple=ok and span and rlen == n_al, sl=int(d["seq_off"][i + 1]) - int(d["seq_off"][i]),
                                   cell=int(d["cell"][i]), umi=int(d["umi"][i])))
    return out


def _snp_table(snps, names, contig, ws):
    """build_tables(): 0-based SNP positions of a contig, sorted, and the first SNP of every 2^ws-base window."""
    p0 = sorted(s[1] - 1 for s in snps if names.index(s[0]) == contig and s[1] >= 1)
    n_swin = ((p0[-1] + 1) >> ws) + 1 if p0 else 0
    return p0, [bisect.bisect_left(p0, w << ws) for w in range(n_swin)]


def _region_table(regions, names, contig):
    """build_tables(): the contig's valid regions by (start, end, row): 0-based start, exclusive end, row, running maximum of the ends;
    and the number of valid regions on the contigs before it (reg_lo)."""
    lo = sum(1 for r in regions if names.index(r[0]) < contig and not (r[1] < 1 or r[1] - 1 > r[2]))
    v = sorted((r[1], r[2], g) for g, r in enumerate(regions) if names.index(r[0]) == contig and not (r[1] < 1 or r[1] - 1 > r[2]))
    s0, e0, row = [x[0] - 1 for x in v], [x[1] for x in v], [x[2] for x in v]
    return lo, s0, e0, row, list(np.maximum.accumulate(e0)) if e0 else []


def _read_snps(r, p0):
    """The counting side of pileup_complex() (a simple read gives the same through pileup_sweep): -> SNP indices under aligned bases
    with a stored base, those without one, and the (first, end) SNP ranges inside gaps."""
    base, nobase, gaps = [], [], []
    k = bisect.bisect_left(p0, r.pos)
    rp, q = r.pos, 0
    for op, l in r.cig:
        if rp >= r.endpos:
            break
        if op in (M, D, N, EQ, X) and l:
            k2 = bisect.bisect_left(p0, min(rp + l, r.endpos), lo=k)
            if op in (M, EQ, X):
                for kk in range(k, k2):
                    qi = q + p0[kk] - rp
                    (base if (qi >> 1) < r.sl else nobase).append(kk)
            elif k2 > k:
                gaps.append((k, k2))
            k = k2; rp += l
        if op in (M, EQ, X, I, S):
            q += l
    if rp < r.endpos:
        k2 = bisect.bisect_left(p0, r.endpos, lo=k)
        if k2 > k:
            gaps.append((k, k2))
    return base, nobase, gaps


def _included(r, s0, e0):
    p, m = r.pos, 0
    for op, l in r.cig:
        if op in (M, EQ, X):
            m += max(min(p + l, e0) - max(p, s0), 0); p += l
        elif op in (D, N):
            p += l
    return m


def model(mode, names, regions, snps, batches, filt, flags=0):
    """-> one dict per tile, in launch order, and the accepted (read, region | SNP) pairs of the whole input (xck_stats.n_hits)."""
    L = limits()
    f = dict(FILT); f.update(filt)
    key128 = bool(flags & F128)
    cg_cap = L.cg_cap_baf if mode == BAF else L.cg_cap
    tiles, n_pairs = [], 0
    for bi, d in enumerate(batches):
        rs = _read_summary(d, f)
        n = len(rs)
        if mode == BAF:
            p0, swin = _snp_table(snps, names, d["contig"], L.ws_snp)
            n_swin = len(swin)
        else:
            reg_lo, rs0, re0, rrow, pmax = _region_table(regions, names, d["contig"])
        for r0 in range(0, n, L.tile):
            r1 = min(r0 + L.tile, n)
            words = int(d["cig_off"][r1]) - int(d["cig_off"][r0])
            c_lo = int(d["cig_off"][r0])
            t = dict(batch=bi, r0=r0, reads=r1 - r0, c_lo=c_lo, words=words, cg_all=words <= cg_cap,
                     beyond_cap=[(bi, i) for i in range(r0, r1) if rs[i].ok and rs[i].c1 - c_lo > cg_cap])
            sweep_pairs = [0] * L.tile_items
            if mode == BAF:
                w0 = max(rs[r0].pos, 0) >> L.ws_snp
                k0 = nk = nw = 0
                if w0 < n_swin:
                    k0 = swin[w0]; nk = min(len(p0) - k0, L.st_cap); nw = min(n_swin - w0, L.st_win)
                t.update(w0=w0, nw=nw, k0=k0, nk=nk, complex=sum(1 for i in range(r0, r1) if rs[i].ok and not rs[i].simple))
                touched, wins, gap_sizes = [], [], []
                n_base = n_rec = 0
                for i in range(r0, r1):
                    r = rs[i]
                    if not r.ok:
                        continue
                    base, nobase, gaps = _read_snps(r, p0)
                    n_base += len(base); n_rec += len(nobase) + sum(-(-(b - a) // L.gap_piece) for a, b in gaps)
                    pairs = len(base) + len(nobase) + sum(b - a for a, b in gaps)
                    n_pairs += pairs
                    if not r.simple:                                      # set aside, walked in the last sweep (in place beyond the list:
                        sweep_pairs[L.tile_items - 1] += pairs             # which reads those are depends on the order of the waves)
                    touched += base + nobase + [k for a, b in gaps for k in range(a, b)]
                    gap_sizes += [b - a for a, b in gaps]
                    if not r.simple and (max(r.pos, 0) >> L.ws_snp) < n_swin:
                        wins.append((max(r.pos, 0) >> L.ws_snp) - w0)
                # the SNP-major walk of the simple reads: per wave and SNP step, the pairs parked before it and its hits
                steps = []
                for w in range(L.waves):
                    pr_n = 0
                    for j in range(L.tile_items):
                        lanes = [i for i in range(r0 + j * L.join_block + w * L.wave, min(r0 + j * L.join_block + (w + 1) * L.wave, r1))]
                        sim = [rs[i] for i in lanes if rs[i].simple]
                        if not sim:
                            continue
                        p_w = rs[lanes[0]].pos
                        if any(r.pos < p_w for r in sim):
                            k = 0
                        else:
                            ww = max(p_w, 0) >> L.ws_snp
                            k = len(p0) if ww >= n_swin else swin[ww]
                            if ww < n_swin:
                                wins.append(ww - w0)
                        while k < len(p0):
                            reach = [r for r in sim if p0[k] < r.endpos]
                            if not reach:
                                break
                            hits = sum(1 for r in reach if p0[k] >= r.pos)
                            if hits:
                                steps.append((j, w, pr_n, hits))
                                if pr_n + hits > L.park_slots:                # drain: the parked pairs reach the queue in this sweep
                                    sweep_pairs[j] += pr_n; pr_n = 0
                                pr_n += hits
                            k += 1
                    sweep_pairs[L.tile_items - 1] += pr_n                      # what is still parked leaves in the last sweep
                t.update(base_hits=n_base, nobase_records=n_rec, gap_sizes=sorted(gap_sizes), park_steps=steps,
                         park_max=max([s[2] + s[3] for s in steps], default=0),
                         snp_rel_min=min(touched, default=k0) - k0, snp_rel_max=max(touched, default=k0) - k0,
                         win_rel_min=min(wins, default=0), win_rel_max=max(wins, default=0))
            else:
                p_first = rs[r0].pos
                e0 = bisect.bisect_right(pmax, p_first)                       # first region whose running-maximum end lies beyond it
                n_ent = min(len(rs0) - e0, L.st_cap)
                keys, rel, accepted = set(), [], set()
                frac = 0.0 < f["min_include"] < 1.0
                for i in range(r0, r1):
                    r = rs[i]
                    if not r.ok:
                        continue
                    for g in range(len(rs0)):
                        if rs0[g] >= r.endpos:
                            break
                        if not (r.pos < re0[g] and r.endpos > rs0[g]):
                            continue
                        rel.append(g - e0)
                        m = _included(r, rs0[g], re0[g])
                        if (r.n_al <= 0 or m / float(r.n_al) < f["min_include"]) if frac else m < f["min_include"]:
                            continue
                        keys.add((rrow[g], r.cell, r.umi)); n_pairs += 1; sweep_pairs[(i - r0) // L.join_block] += 1
                        accepted.add(((bi, i), rrow[g]))
                # per wave of 64 reads: smallest position and largest end of its filtered reads, and whether each of them spans its CIGAR
                spans = []
                for w0_ in range(r0, r1, L.wave):
                    okr = [rs[i] for i in range(w0_, min(w0_ + L.wave, r1)) if rs[i].ok]
                    spans.append((min(r.pos for r in okr), max(r.endpos for r in okr), all(r.span for r in okr)) if okr else None)
                t.update(e0=reg_lo + e0, n_ent=n_ent, reg_lo=reg_lo, n_regions=len(rs0), distinct_keys=len(keys), accepted=accepted, wave_span=spans,
                         reg_rel_min=min(rel, default=0), reg_rel_max=max(rel, default=0))
            t["sweep_pairs"] = sweep_pairs
            t["key128"] = key128
            tiles.append(t)
    return tiles, n_pairs


def crossed(mode, tiles):
    """The limits whose second path the input takes in some tile: cx (set-aside list full), cg (CIGAR run not staged whole and a read
    has words beyond it), st (a region / SNP outside the staged slice), win (a SNP window outside the staged ones), park (a drain in the
    middle of a walk), bq / nq (split mode: either queue full), q128 (128-bit keys: more records between two flushes - one per sweep - than the queue holds; a
    parked pileup pair counts in the sweep that drains it), hs (more distinct keys than
    the set has slots)."""
    L = limits()
    out = set()
    for t in tiles:
        if not t["cg_all"] and t["beyond_cap"]:
            out.add("cg")
        if mode == BAF:
            if t["complex"] > L.cx_cap:
                out.add("cx")
            if t["base_hits"] + t["nobase_records"] and (t["snp_rel_min"] < 0 or t["snp_rel_max"] >= t["nk"]):
                out.add("st")
            if t["win_rel_min"] < 0 or t["win_rel_max"] >= max(t["nw"], 1):
                out.add("win")
            if t["park_max"] > L.park_slots:
                out.add("park")
            if t["key128"]:
                if max(t["sweep_pairs"]) > L.qcap_baf128:
                    out.add("q128")
            else:
                if t["base_hits"] > L.bqcap:
                    out.add("bq")
                if t["nobase_records"] > L.nqcap:
                    out.add("nq")
        else:
            if t["reg_rel_min"] < 0 or t["reg_rel_max"] >= max(t["n_ent"], 1):
                out.add("st")
            if t["key128"]:
                if max(t["sweep_pairs"]) > L.qcap_fc128:
                    out.add("q128")
            elif t["distinct_keys"] > L.hs_slots:
                out.add("hs")
    return out


# ----------------------------------------------------------------------------- cases
def _case(name, mode, regions, snps, groups, facts, crosses, filt=None, names=("1",), contig=0, sort=True, crosses128=None, not_accepted=()):
    """not_accepted: (rec, region row) pairs the include test rejects although a shortcut taken wrongly would emit them."""
    batches, under = build_batches(groups, contig, sort)
    assert 0 < len(under) <= MAX_UNDER_TEST and sum(len(d["pos"]) for d in batches) <= MAX_READS, name
    return SimpleNamespace(name=name, mode=mode, names=list(names), regions=regions, snps=snps, n_cells=N_CELLS, batches=batches,
                           filt=dict(filt or {}), facts=facts, under_test=under, crosses=set(crosses), crosses128=crosses128,
                           not_accepted=[(r["at"], row) for r, row in not_accepted])


def _loci(n, base=5000, step=40):
    return [base + step * j for j in range(n)]


# ---- pileup 1: spliced reads of a tile around XCK_CX_CAP
CX = [(M, 6), (N, 10), (M, 6)]                          # one SNP, under the second block (pos + 18); none inside the gap


def case_cx(n_cx, second=0):
    L = limits()
    loci = _loci(100)
    cx = [rec(loci[i % 100], CX) for i in range(n_cx)]
    mark(cx, MAX_UNDER_TEST - second)
    groups = [fill(L.tile - n_cx, 100) + cx]
    p0s = [p + 18 for p in loci]
    facts = {0: dict(complex=n_cx, reads=L.tile, k0=0, nk=100 + second, base_hits=n_cx)}
    if second:                                             # cx_n is per tile: a second tile with one more spliced read
        last = rec(9600, CX, ut=True)
        groups[0] += fill(9, 9500) + [last]
        p0s += [9618]
        facts[1] = dict(complex=1, reads=10)
    regions, snps = snp_rows(p0s)
    return _case("cx", BAF, regions, snps, groups, facts, ({"cx"} if n_cx > L.cx_cap else set()) | ({"bq"} if n_cx > L.bqcap else set()) | ({"cg"} if L.tile + 2 * n_cx > L.cg_cap_baf else set()))


# ---- pileup 2 / basefc 11: CIGAR words of a tile's run around the staged capacity
SIMPLE_SI = ([(S, 2), (M, 4), (I, 1), (M, 4)], 6)       # (CIGAR, offset of its SNP: under the second block, behind S and I)
SPLICED = ([(M, 4), (N, 6), (M, 4)], 12)                # the SNP under the second block, none inside the gap
LONG = ([(M, 1), (I, 1)] * 10 + [(M, 4)], 12)           # 21 words: wherever it lies, some of them straddle the capacity


def _cig_tile(base, total_words, specials, n_reads):
    """n_reads reads whose CIGAR run is total_words long: fillers of one or two words at `base`, then the special reads (CIGAR, SNP
    offset), each at a locus of its own right of the fillers.  -> recs, special recs, SNP positions"""
    sp = [rec(base + 1000 + 40 * j, cig) for j, (cig, off) in enumerate(specials)]
    n_fill = n_reads - len(sp)
    two = total_words - sum(len(r["cig"]) for r in sp) - n_fill
    assert 0 <= two <= n_fill
    return fill(two, base, [(S, 1), (M, 11)]) + fill(n_fill - two, base) + sp, sp, [r["pos"] + off for r, (cig, off) in zip(sp, specials)]


def case_cig(delta, specials):
    """Two tiles (cg_lo != 0 in the second) whose runs are the pileup's capacity + delta words long; the special reads come last."""
    L = limits()
    recs, p0s, facts = [], [], {}
    for t in range(2):
        r, sp, p = _cig_tile(100 + 3000 * t, L.cg_cap_baf + delta, specials, L.tile)
        for x in sp:
            x["ut"] = True
        recs += r; p0s += p
        facts[t] = dict(words=L.cg_cap_baf + delta, cg_all=delta <= 0, reads=L.tile)
    facts[1]["c_lo"] = L.cg_cap_baf + delta
    regions, snps = snp_rows(p0s)
    return _case("cig", BAF, regions, snps, [recs], facts, {"cg"} if delta > 0 else set())


# ---- pileup 3: the furthest SNP of a read around the staged SNP slice
def case_st(t):
    """SNP k at 2000 + 10 k; the tile's first read lies left of them all (k0 = 0).  A simple read over SNP t alone, and a spliced read
    with SNP t - 3 under its first block, SNPs t - 2 and t - 1 inside its gap (shadowed) and SNP t under its second block."""
    p0 = [2000 + 10 * k for k in range(300)]
    simple = rec(p0[t] - 3, [(M, 8)], ut=True)
    cx = rec(p0[t - 3] - 2, [(M, 4), (N, 26), (M, 4)], ut=True)
    shadows = [rec(p0[g] - 1, [(M, 3)], shadow_of=cx) for g in (t - 2, t - 1)]
    regions, snps = snp_rows(p0)
    return _case("st", BAF, regions, snps, [fill(100, 100) + [cx] + shadows + [simple]], {0: dict(k0=0, nk=limits().st_cap, snp_rel_max=t)},
                 {"st"} if t >= limits().st_cap else set())


def case_snp_left():
    """Unsorted input: the tile's first read lies two windows right of a simple and a spliced read of the same tile (k_from < k0)."""
    p0 = [1000 + 10 * k for k in range(250)]
    first = rec(3050, [(M, 8)])
    simple = rec(1097, [(M, 8)], ut=True)
    cx = rec(1208, [(M, 4), (N, 6), (M, 4)], ut=True)       # SNPs 1210 and 1220 under its blocks
    regions, snps = snp_rows(p0)
    return _case("snp_left", BAF, regions, snps, [[first] + fill(70, 3600) + [simple, cx]], {0: dict(w0=2, k0=105, snp_rel_min=-95)}, {"st", "win"},
                 sort=False)


# ---- pileup 4: SNP windows around the staged ones
def _win_snps():
    return [1024 * w + 20 + 10 * i for w in (63, 64, 65) for i in range(4)] + [1024 * 70 + 5]


def case_win(w):
    """Wave 1 of the tile starts w windows right of the tile's first read: simple reads over the first SNP of that window and two spliced
    reads; the last read lies right of the last SNP window and meets nothing."""
    hit = [rec(1024 * w + 15, [(M, 12)]) for _ in range(62)]
    cx = [rec(1024 * w + 28, [(M, 4), (N, 4), (M, 4)]) for _ in range(2)]
    mark(hit, 8); mark(cx)
    regions, snps = snp_rows(_win_snps())
    return _case("win", BAF, regions, snps, [fill(64, 100) + hit + cx + [rec(1024 * 75, [(M, 12)])]],
                 {0: dict(w0=0, nw=limits().st_win, win_rel_max=w, reads=129)}, {"win"} if w >= limits().st_win else set())


def case_win_tile_right():
    """Unsorted input whose first read lies right of the last SNP window (nk = nw = 0): nothing is staged, every read of the tile goes
    to global memory for its window and its SNPs."""
    hit = [rec(1024 * 63 + 15, [(M, 12)]) for _ in range(62)]
    cx = [rec(1024 * 63 + 28, [(M, 4), (N, 4), (M, 4)]) for _ in range(2)]
    mark(hit, 8); mark(cx)
    regions, snps = snp_rows(_win_snps())
    return _case("win_tile_right", BAF, regions, snps, [[rec(1024 * 80, [(M, 12)])] + fill(63, 1024 * 80 + 1) + hit + cx], {0: dict(nk=0, nw=0, w0=80)},
                 {"st", "win"}, sort=False)


def case_pos_minus1():
    """The tile's first read at position -1 (kept: fetch() only asks pos < stop and endpos > start), simple and spliced."""
    regions, snps = snp_rows([0, 5, 300])
    return _case("pos_minus1", BAF, regions, snps, [[rec(-1, [(M, 8)], ut=True), rec(-1, [(M, 3), (N, 2), (M, 3)], ut=True)] + fill(20, 100)],
                 {0: dict(w0=0, k0=0, base_hits=4)}, set())


# ---- pileup 5: parked pairs of a wave around its 64 slots
def case_park(kind):
    a, b = 3000, 3002
    p0s = [a, b, 4000]
    if kind == "64_64":      # 64 reads over both SNPs: 64 parked, 64 more arrive
        hit = [rec(2998, [(M, 8)]) for _ in range(64)]; recs = hit; steps = [(0, 0, 0, 64), (0, 0, 64, 64)]
    elif kind == "63_1":     # 63 over A, one over B: the segment is exactly full
        hit = [rec(2994, [(M, 8)]) for _ in range(63)] + [rec(3001, [(M, 8)])]; recs = hit; steps = [(0, 0, 0, 63), (0, 0, 63, 1)]
    elif kind == "63_2":     # 62 over A, one over both, one over B
        hit = [rec(2994, [(M, 8)]) for _ in range(62)] + [rec(2998, [(M, 8)]), rec(3001, [(M, 8)])]; recs = hit; steps = [(0, 0, 0, 63), (0, 0, 63, 2)]
    else:                    # 40 pairs left parked by sweep 0 of wave 0, 30 more in its sweep 1
        h0 = [rec(2994, [(M, 8)]) for _ in range(40)]; h1 = [rec(3998, [(M, 8)]) for _ in range(30)]
        hit = h0 + h1; recs = h0 + fill(limits().join_block - 40, 3100) + h1; steps = [(0, 0, 0, 40), (1, 0, 40, 30)]
    mark(hit)
    regions, snps = snp_rows(p0s)
    over = steps[-1][2] + steps[-1][3] > limits().park_slots
    return _case("park", BAF, regions, snps, [recs], {0: dict(park_steps=steps)}, {"park"} if over else set())


# ---- pileup 6: the queues
def case_bhits(h):
    """h hits with a base in one tile (split mode: the queue of XCK_BAF_BQUEUE_BYTES)."""
    L = limits()
    loci = _loci(150, step=20)
    hit = [rec(loci[i % 150] - 3, [(M, 8)]) for i in range(h)]
    mark(hit)
    regions, snps = snp_rows(loci)
    return _case("bhits", BAF, regions, snps, [fill(L.tile - h, 100) + hit], {0: dict(base_hits=h, nobase_records=0, complex=0, nk=150)},
                 {"bq"} if h > L.bqcap else set())


def case_nrec(n):
    """n records without a base in one tile (split mode: the queue of XCK_BAF_NQUEUE_BYTES): 100 spliced reads with one SNP inside the
    gap and n - 100 simple reads without a sequence; their shadows are two batches of their own, so that no tile's hits with a base
    reach the other queue's capacity."""
    L = limits()
    loci = _loci(150, step=20)
    cx = [rec(loci[i % 150] - 5, [(M, 4), (N, 4), (M, 4)]) for i in range(100)]
    ns = [rec(loci[i % 150] - 3, [(M, 8)], seq=False) for i in range(100, n)]
    mark(cx, 8); mark(ns, 8)
    sh = [rec(r["pos"] + (4 if r["seq"] else 2), [(M, 3)], shadow_of=r) for r in cx + ns]
    plain = [rec(loci[i] - 3, [(M, 8)]) for i in range(5)]
    regions, snps = snp_rows(loci)
    return _case("nrec", BAF, regions, snps, [fill(L.tile - n - 5, 100) + cx + ns + plain, sh[:n // 2], sh[n // 2:]],
                 {0: dict(base_hits=5, nobase_records=n, complex=100), 1: dict(base_hits=n // 2), 2: dict(base_hits=n - n // 2)},
                 {"nq"} if n > L.nqcap else set())


def case_sweep128(h):
    """h records reach the queue between two flushes (128-bit keys: one flush after every sweep).  A hit of a simple read reaches the
    queue when its wave drains, not in the sweep that found it: here every wave of sweep 0 parks at most 64 pairs and keeps them until
    the last sweep, where one spliced read adds the 257th record; the other sweeps meet nothing."""
    L = limits()
    loci = _loci(150, step=20)
    hit = [rec(loci[i % 150] - 3, [(M, 8)]) for i in range(min(h, L.join_block))]
    hit += [rec(8500, CX) for _ in range(h - len(hit))]
    mark(hit)
    regions, snps = snp_rows(loci + [8518])
    return _case("sweep128", BAF, regions, snps, [hit + fill(L.tile - len(hit), 9000)],
                 {0: dict(base_hits=h, sweep_pairs=[0, 0, 0, h], park_max=min(h, L.join_block) // L.waves + (h < L.join_block))}, {"bq"},
                 crosses128={"q128"} if h > L.qcap_baf128 else set())


# ---- pileup 7: gaps, and reads that are not one aligned block for other reasons
def case_gaps(op):
    """One read per gap size: SNPs under both blocks, g SNPs (two bases apart) inside the N / D gap, each with its shadow; the shadows
    are batches of their own (fewer hits with a base per tile than the queue holds)."""
    reads, shadows, p0s, sizes = [], [[], []], [], (0, 1, 31, 32, 33, 64, 65)
    for c, g in enumerate(sizes):
        b = 10000 + 1000 * c
        r = rec(b, [(M, 4), (op, 2 * g + 2), (M, 4)], ut=True)
        reads.append(r)
        p0s += [b + 1, b + 7 + 2 * g] + [b + 5 + 2 * i for i in range(g)]
        shadows[g >= 64] += [rec(b + 4 + 2 * i, [(M, 3)], shadow_of=r) for i in range(g)]
    regions, snps = snp_rows(p0s)
    return _case("gaps", BAF, regions, snps, [reads] + shadows,
                 {0: dict(complex=7, base_hits=14, gap_sizes=[1, 31, 32, 33, 64, 65], nobase_records=sum(-(-g // limits().gap_piece) for g in sizes))}, set())


def case_odd_reads():
    """An unmapped-flagged read whose CIGAR starts with a gap (fetched by its first base only: the gap is cut short by endpos), a read
    without CIGAR on a SNP, an unmapped-flagged read with a plain CIGAR, a SNP on the last base of an odd and of an even query length,
    and a read without sequence.  The unmapped flag is taken out of the exclusion mask, min_len is 0 (a read without CIGAR has no
    aligned base)."""
    a = rec(20000, [(N, 5), (M, 8)], flag=FUNMAP, ut=True)            # SNP 20000 inside the gap; 20002 is beyond its one-base span
    b = rec(20100, [], ut=True)                                         # SNP 20100
    c = rec(20200, [(M, 8)], flag=FUNMAP, ut=True)                      # SNP 20200 with its first base; 20203 is beyond its span
    d1, d2 = rec(20300, [(M, 9)], ut=True), rec(20400, [(M, 8)], ut=True)   # SNPs 20308, 20407: the last base
    e = rec(20500, [(M, 8)], seq=False, ut=True)                        # SNP 20504
    sh = [rec(20000, [(M, 3)], shadow_of=a), rec(20100, [(M, 3)], shadow_of=b), rec(20503, [(M, 3)], shadow_of=e)]
    regions, snps = snp_rows([20000, 20002, 20100, 20200, 20203, 20308, 20407, 20504])
    return _case("odd_reads", BAF, regions, snps, [[a, sh[0], b, sh[1], c, d1, d2, e, sh[2]]],
                 {0: dict(complex=3, base_hits=3 + 2 + 1 + 1, nobase_records=3, gap_sizes=[1, 1])}, set(), filt=dict(excl_flag=768, min_len=0))


# ---- pileup 8: batch sizes around the wave, sweep and tile
def case_batch(n):
    regions, snps = snp_rows([3004, 3100])
    return _case("batch", BAF, regions, snps, [fill(n - 1, 100) + [rec(3000, [(M, 8)], ut=True)]],
                 {(n - 1) // limits().tile: dict(reads=(n - 1) % limits().tile + 1, base_hits=1)}, set())


# ---- basefc 9: regions around the staged slice and around the chunks of 64
def _grid(n, start=1000, step=20, width=10, contig="1"):
    return [(contig, start + step * k + 1, start + step * k + width, "g%d" % k) for k in range(n)]


def case_fc_st(ts, n_regions=300, two_contigs=False):
    """Region k = [1000 + 20 k, 1000 + 20 k + 10); the tile's first read lies left of them all (e0 = the contig's first region); one
    10M read exactly on each region of ts.  two_contigs: the same on a second contig behind 70 regions of the first (reg_lo != 0)."""
    L = limits()
    regions = (_grid(70) if two_contigs else []) + _grid(n_regions, contig="2" if two_contigs else "1")
    hit = [rec(1000 + 20 * t, [(M, 10)], ut=True) for t in ts]
    lo = 70 if two_contigs else 0
    return _case("fc_st", FC, regions, [], [fill(100, 100) + hit],
                 {0: dict(e0=lo, reg_lo=lo, n_ent=min(n_regions, L.st_cap), reg_rel_max=max(ts), n_regions=n_regions, distinct_keys=len(ts))},
                 {"st"} if max(ts) >= L.st_cap else set(), names=("1", "2") if two_contigs else ("1",), contig=1 if two_contigs else 0)


# ---- basefc 10: the key set and the 128-bit queue
def case_fc_keys(n_keys):
    """1023 reads over two adjacent regions each and a last one over 1, 2 or 3 (min_include 0: every overlapped region counts)."""
    L = limits()
    regions = _grid(200, step=10)
    hit = [rec(1000 + 10 * (i % 199), [(M, 20)]) for i in range(L.tile - 1)]
    last = rec(1000, [(M, 10 * (n_keys - 2 * (L.tile - 1)))])
    mark(hit, 15); last["ut"] = True
    return _case("fc_keys", FC, regions, [], [hit + [last]], {0: dict(distinct_keys=n_keys, e0=0, n_ent=200, reads=L.tile)},
                 {"hs"} if n_keys > L.hs_slots else set(), filt=dict(min_include=0))


def case_fc_sweep128(n_pairs):
    """n_pairs accepted pairs in sweep 0 of a tile (128-bit keys: the queue is flushed after every sweep); the other sweeps meet nothing."""
    L = limits()
    regions = _grid(200, step=10)
    hit = [rec(1000 + 10 * (i % 190), [(M, 40)]) for i in range(L.join_block - 1)]
    last = rec(1000, [(M, 10 * (n_pairs - 4 * (L.join_block - 1)))])
    mark(hit, 15); last["ut"] = True
    return _case("fc_sweep128", FC, regions, [], [hit + [last] + fill(L.tile - L.join_block, 5000)],
                 {0: dict(distinct_keys=n_pairs, sweep_pairs=[n_pairs, 0, 0, 0])}, set(), filt=dict(min_include=0),
                 crosses128={"q128"} if n_pairs > L.qcap_fc128 else set())


# ---- basefc 11: the containing-region shortcut at its edge
def case_fc_contain(min_include):
    """Wave 0 spans [2000, 2060) (wmin, wmax) and meets regions A = the span exactly, B / C = one base short at the left / right end,
    D = a base to spare at both ends, E = a base short at both, F and G cutting into it (rows 0 - 6).  Besides 40M reads the wave holds,
    flush at wmin and flush at wmax, a 1M, a 9M and a 30M read: the base that B, C and E lack makes the include test reject them (no
    overlap at all, 8 / 9 < 0.9, 29 < 30), while a shortcut that takes a region one base short for a containing one emits them.
    Wave 1 spans [4000, 4060) the same way (rows 7 - 13) and holds one unmapped-flagged 60M read at 4035: fetched by its first base
    only, inside A and D, but with 25 of its 60 aligned bases inside them - rejected by the walk (under 0.9 and 30), emitted by a
    shortcut that forgets all_span.  Under min_include 0 every overlapping pair is accepted by either path; there only the 1M reads
    (which do not overlap the short regions at all) tell the paths apart."""
    def reg(s0, e0):
        return ("1", s0 + 1, e0, "r")
    regions = []
    for b in (2000, 4000):
        regions += [reg(b, b + 60), reg(b + 1, b + 60), reg(b, b + 59), reg(b - 1, b + 61), reg(b + 1, b + 59), reg(b + 10, b + 50), reg(b + 30, b + 100)]
    A, B, C, D_, E = 0, 1, 2, 3, 4
    lo = {n: rec(2000, [(M, n)]) for n in (1, 9, 30)}                 # flush at wmin
    hi = {n: rec(2060 - n, [(M, n)]) for n in (1, 9, 30)}             # flush at wmax
    plain0 = [rec(2000 + i % 21, [(M, 40)]) for i in range(64 - 6)]
    um = rec(4035, [(M, 60)], flag=FUNMAP, ut=True)
    plain1 = [rec(4000 + i % 21, [(M, 40)]) for i in range(63)]
    frac, length = 0.0 < min_include < 1.0, min_include >= 1
    live = [n for n in (1, 9, 30) if not length or n >= min_include]  # (in length mode a shorter read is accepted nowhere: no witness)
    for n in live:
        lo[n]["ut"] = hi[n]["ut"] = True
    mark(plain0, 4); mark(plain1, 4)
    short = [1, 9] if frac else [30] if length else [1]
    rejected = [(lo[n], r) for n in short for r in (B, E)] + [(hi[n], r) for n in short for r in (C, E)]
    if min_include > 0:
        rejected += [(um, 7 + A), (um, 7 + D_)]
    w0 = sorted(list(lo.values()) + list(hi.values()) + plain0, key=lambda r: r["pos"])
    return _case("fc_contain", FC, regions, [], [w0 + plain1 + [um]],
                 {0: dict(e0=0, n_ent=14, reads=128, wave_span=[(2000, 2060, True), (4000, 4060, False)])}, set(),
                 filt=dict(min_include=min_include, excl_flag=768), not_accepted=rejected)


def case_fc_cig(delta):
    """A tile whose CIGAR run is the basefc capacity + delta words long; its last four reads are spliced across region boundaries
    (included_len's walk), with all their words beyond the capacity when delta = 12."""
    L = limits()
    regions = [("1", 6001, 6045, "h"), ("1", 5991, 6049, "j"), ("1", 6006, 6100, "k")]
    sp = [([(M, 10), (N, 30), (M, 10)], 0)] * 4
    recs, spr, _ = _cig_tile(100, L.cg_cap + delta, sp, L.tile)
    for r in spr:
        r["pos"] = 6000; r["ut"] = True
    return _case("fc_cig", FC, regions, [], [recs], {0: dict(words=L.cg_cap + delta, cg_all=delta <= 0, distinct_keys=4)}, {"cg"} if delta > 0 else set())


def _builders():
    L = limits()
    b = {}
    for n in (L.cx_cap - 1, L.cx_cap, L.cx_cap + 1, L.tile):
        b["cx_%d" % n] = functools.partial(case_cx, n)
    b["cx_%d_then_1" % (L.cx_cap + 1)] = functools.partial(case_cx, L.cx_cap + 1, 1)
    for tag, delta in (("cap-1", -1), ("cap", 0), ("cap+1", 1)):           # the last read's words straddle the capacity at cap + 1
        b["cig_%s" % tag] = functools.partial(case_cig, delta, [SIMPLE_SI, SPLICED, LONG])
    b["cig_over_simple"] = functools.partial(case_cig, 40, [SIMPLE_SI] * 8)
    b["cig_over_spliced"] = functools.partial(case_cig, 40, [SPLICED] * 8)
    b["cig_over_straddle"] = functools.partial(case_cig, 10, [LONG])
    for t in (L.st_cap - 1, L.st_cap, L.st_cap + 1):
        b["st_snp_k0+%d" % t] = functools.partial(case_st, t)
    b["st_snp_left_of_tile"] = case_snp_left
    for w in (L.st_win - 1, L.st_win, L.st_win + 1):
        b["win_%d" % w] = functools.partial(case_win, w)
    b["win_tile_right_of_last"] = case_win_tile_right
    b["win_pos_minus1"] = case_pos_minus1
    for kind in ("64_64", "63_1", "63_2", "carry_40_30"):
        b["park_%s" % kind] = functools.partial(case_park, kind)
    for h in (L.bqcap - 1, L.bqcap, L.bqcap + 1):
        b["bhits_%d" % h] = functools.partial(case_bhits, h)
    for n in (L.nqcap - 1, L.nqcap, L.nqcap + 1):
        b["nrec_%d" % n] = functools.partial(case_nrec, n)
    for h in (L.qcap_baf128 - 1, L.qcap_baf128, L.qcap_baf128 + 1):
        b["sweep128_%d" % h] = functools.partial(case_sweep128, h)
    b["gaps_N"] = functools.partial(case_gaps, N)
    b["gaps_D"] = functools.partial(case_gaps, D)
    b["odd_reads"] = case_odd_reads
    for n in (1, L.join_block - 1, L.join_block, L.join_block + 1, L.tile - 1, L.tile, L.tile + 1, 2 * L.tile + 1):
        b["batch_%d" % n] = functools.partial(case_batch, n)
    for t in (L.st_cap - 1, L.st_cap, L.st_cap + 1):
        b["fc_st_e0+%d" % t] = functools.partial(case_fc_st, [t])
    b["fc_chunk_63_64_65"] = functools.partial(case_fc_st, [L.wave - 1, L.wave, L.wave + 1])
    b["fc_last_chunk_staged"] = functools.partial(case_fc_st, [99], 100)
    b["fc_last_chunk_unstaged"] = functools.partial(case_fc_st, [299], 300)
    b["fc_second_contig"] = functools.partial(case_fc_st, [L.wave - 1, L.wave, L.wave + 1, L.st_cap - 1, L.st_cap, 299], 300, True)
    for n in (L.hs_slots - 1, L.hs_slots, L.hs_slots + 1):
        b["fc_keys_%d" % n] = functools.partial(case_fc_keys, n)
    for n in (L.qcap_fc128 - 1, L.qcap_fc128, L.qcap_fc128 + 1):
        b["fc_sweep128_%d" % n] = functools.partial(case_fc_sweep128, n)
    for tag, v in (("0.9", 0.9), ("30", 30), ("0", 0)):
        b["fc_contain_%s" % tag] = functools.partial(case_fc_contain, v)
    b["fc_cig_cap"] = functools.partial(case_fc_cig, 0)
    b["fc_cig_over_spliced"] = functools.partial(case_fc_cig, 12)
    return b


NAMES = list(_builders())


@functools.lru_cache(maxsize=None)
def case(name):
    c = _builders()[name]()
    c.name = name
    return c


def without_read(batches, at):
    """The batch dicts without read `at` = (batch, read); ordinal bases stay as they are."""
    out = []
    for bi, d in enumerate(batches):
        if bi != at[0]:
            out.append(d); continue
        keep = np.array([i for i in range(len(d["pos"])) if i != at[1]], np.int64)
        e = dict(contig=d["contig"], ordinal_base=d["ordinal_base"])
        for k in ("pos", "flag", "mapq", "cell", "umi"):
            e[k] = d[k][keep].copy()
        for off, dat in (("cig_off", "cigar"), ("seq_off", "seq")):
            parts = [d[dat][int(d[off][i]):int(d[off][i + 1])] for i in keep]
            e[off] = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint32)
            e[dat] = np.concatenate(parts + [np.zeros(1, d[dat].dtype)])
        out.append(e)
    return out
