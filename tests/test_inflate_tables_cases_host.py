"""The corpus of tests/test_gpu_inflate_tables.py, and the proof - on the CPU - that every one of its streams is what it is named for.

csrc/inflate_dev.hip sets a dynamic block up on all 64 lanes: the code-length code becomes a 128-entry look-up table, lane 0 only
marks where a run of equal lengths begins and the wave spreads the marks over lens[]; build_table counts the lengths and ranks every
symbol among the symbols of its length by ballots over chunks of 64 symbols (lane i owns the symbols i, i + 64, ...), takes the extra
bits of every first-level prefix as a maximum on the table entry itself, and hands the sub-tables out by a scan over the prefixes.
The header's scratch lies over the literal / length table.  The streams here are the smallest at which each of these can go wrong.
For every stream: zlib accepts or refuses it as intended (deflate_craft.check, when it is made), and canonical / kraft /
subtable_need / fill_lengths / rle_lengths show the property it is named for.  Every payload uses every code its header defines, so a
wrong table entry changes the bytes.  Otherwise the GPU test could pass without meeting the code."""
import functools
import random

import deflate_craft as dc
from deflate_craft import Bits

D_LIT_TB, D_DIST_TB = 9, 8                                             # csrc/inflate_dev.hip
D_LIT_MAX, D_DIST_MAX = (1 << D_LIT_TB) + 768, (1 << D_DIST_TB) + 256
NOISE = 300                                                            # bytes of a stored block in front: something to copy from


# ---- codes -----------------------------------------------------------------------------------------------------------------
def lengths(n, fixed):
    out = [0] * n
    for s, l in fixed.items():
        out[s] = l
    return out


def complete(fixed, fillers, avoid=()):
    """{symbol: length}: `fixed` as given, and the rest of the code space handed to the first of `fillers` - shortest codes first, all
    but the last three or fewer - so that the code is complete.  No filler gets a length in `avoid`."""
    rest = 32768 - sum(1 << (15 - l) for l in fixed.values())
    assert rest > 0
    items = [15 - k for k in range(15, -1, -1) if rest >> k & 1]
    while any(l in avoid or l == 0 for l in items) or len(items) < len(fillers) - 3:
        bad = [i for i, l in enumerate(items) if l in avoid or l == 0]
        i = bad[0] if bad else min(range(len(items)), key=lambda i: items[i])
        assert items[i] < 15
        items[i:i + 1] = [items[i] + 1] * 2
    assert len(items) <= len(fillers), (len(items), len(fillers))
    out = dict(fixed)
    out.update(zip(fillers, sorted(items)))
    assert len(out) == len(fixed) + len(items) and dc.kraft(list(out.values())) == 32768
    return out


def cover(ll, dl, pos, rng):
    """Tokens that use every code of ll / dl at least once, `pos` bytes of output standing before them."""
    toks = [s for s in range(256) if ll[s]]
    rng.shuffle(toks)
    pos += len(toks)
    ls = [s for s in range(257, min(len(ll), 286)) if ll[s]]
    ds = [s for s in range(min(len(dl), 30)) if dl[s]]
    assert bool(ls) == bool(ds), "a length code needs a distance code and the other way round"
    for k in range(max(len(ls), len(ds)) if ls else 0):
        a, b = ls[k % len(ls)] - 257, ds[k % len(ds)]
        length = dc.LEN_BASE[a] + rng.randrange(min(1 << dc.LEN_EXTRA[a], 31))     # (227 + 31 would go out as code 285)
        dist = dc.DIST_BASE[b] + rng.randrange(1 << dc.DIST_EXTRA[b])
        assert dist <= pos, (dist, pos)
        toks.append((length, dist))
        pos += length
    return toks


def uses_every_code(toks, ll, dl):
    lf, df = dc.frequencies(toks)
    return all(lf[s] for s in range(min(len(ll), 286)) if ll[s]) and all(df[s] for s in range(min(len(dl), 30)) if dl[s])


def expand(syms):
    """The code lengths a list of rle_lengths symbols writes, and where every symbol's lengths begin."""
    out, at = [], []
    for s, x, _ in syms:
        at.append(len(out))
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        else:
            out += [0] * ((3 if s == 17 else 11) + x)
    return out, at


def history(dl):
    """Bytes that must stand before a payload that uses every distance code of dl."""
    ds = [s for s in range(min(len(dl), 30)) if dl[s]]
    return max([NOISE] + [dc.DIST_BASE[s] + (1 << dc.DIST_EXTRA[s]) for s in ds])


# ---- the largest sub-table need ------------------------------------------------------------------------------------------------
def largest_need(root, n_sym, complete_only=True):
    """The largest second-level need (dc.subtable_need) of a code of at most n_sym symbols that is not over-subscribed, and the sorted
    lengths of one that has it.  A canonical code fills the code space from the left in ascending length, so the first-level prefixes
    that carry long codes are the last P of the 2^root, each of them full (but, in an incomplete code, the last) and the deepest
    code of prefix j, m_j, is its last and never shorter than m_(j-1).  Prefix j is sized 2^(m_j - root).  It holds no code shorter than
    a = max(root + 1, m_(j-1)): at the least 2^(a - root) - 1 codes of a bits and, under the last node of that depth, the comb
    a + 1, ..., m_j - 1, m_j, m_j - 2^(a - root) + (m_j - a) codes.  The 2^root - P prefixes before them take one short code per set
    bit of that number at the least.  So: a search over (P, m_P, symbols used) for the largest sum of sizes."""
    top = 1 << root
    best = {(0, root + 1): {0: (0, None)}}                               # (P, m) -> symbols used -> (need, where from)
    states = [(0, root + 1)]
    result = (0, None)
    seen = set(states)
    while states:
        nxt = []
        for P, m0 in states:
            for used, (need, _) in list(best[(P, m0)].items()):
                short = bin(top - P).count("1")
                if used + short <= n_sym and need > result[0]:
                    result = (need, (P, m0, used))
                if not complete_only and used + 1 + short <= n_sym + 1 and P + 1 < top:    # one code of 15 bits alone in one more prefix
                    if used + 1 + bin(top - P - 1).count("1") <= n_sym and need + (1 << (15 - root)) > result[0]:
                        result = (need + (1 << (15 - root)), (P, m0, used, "partial"))
                a = m0
                for m in range(a, 16):
                    cost = (1 << (a - root)) + (m - a)
                    u2 = used + cost
                    if u2 + 1 > n_sym:
                        break
                    d = best.setdefault((P + 1, m), {})
                    if u2 not in d or d[u2][0] < need + (1 << (m - root)):
                        d[u2] = (need + (1 << (m - root)), (P, m0, used))
                        if (P + 1, m) not in seen:
                            seen.add((P + 1, m))
                            nxt.append((P + 1, m))
        states = nxt
    need, at = result
    lens, partial = [], len(at) == 4
    if partial:
        lens.append(15)
    P, m, used = at[:3]
    top_p = P + (1 if partial else 0)
    while P:
        _, (P0, a, used0) = best[(P, m)][used]
        lens = [a] * ((1 << (a - root)) - 1) + ([a] if m == a else list(range(a + 1, m)) + [m, m]) + lens
        P, m, used = P0, a, used0
    short = [root - k for k in range(root, -1, -1) if (top - top_p) >> k & 1]
    return need, short + lens


# ---- the cases -----------------------------------------------------------------------------------------------------------------
class Cases:
    def __init__(self):
        self.entries = []

    def add(self, name, group, raw, payload, facts, valid=True):
        payload = bytes(payload)
        dc.check(raw, payload, valid)
        assert len(payload) > 0, name
        self.entries.append(dict(name=name, group=group, blk=dc.bgzf(raw, payload), payload=payload, valid=valid, facts=facts))


class Stream:
    def __init__(self, rng, noise=NOISE):
        self.w, self.out, self.rng = Bits(), bytearray(), rng
        if noise:
            self.stored(bytes(rng.randrange(256) for _ in range(noise)))

    def stored(self, data, final=0):
        dc.put_stored(self.w, data, final)
        self.out += data

    def fixed(self, toks, final=0):
        dc.put_fixed(self.w, toks, final)
        dc.detok(toks, self.out)

    def dynamic(self, ll, dl, final=1, syms=None, hlit=None, hdist=None, toks=None, **kw):
        """A dynamic block whose payload uses every code; syms: the header's length symbols when they are not rle_lengths' own."""
        toks = cover(ll, dl, len(self.out), self.rng) if toks is None else toks
        syms = dc.rle_lengths(list(ll) + list(dl)) if syms is None else syms
        cl = dc.put_dynamic_header(self.w, final, len(ll) if hlit is None else hlit, len(dl) if hdist is None else hdist, syms, **kw)
        dc.put_tokens(self.w, toks, ll, dl)
        dc.detok(toks, self.out)
        return toks, syms, cl


LITS = [65, 67, 71, 84, 78, 10, 9, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 44, 33]


def small_code(rng, n_lit=12, n_len=4, n_dist=4):
    """A complete literal / length code over a few literals, the end-of-block code and a few lengths; a complete distance code."""
    lf = [0] * 286
    for s in rng.sample(LITS, n_lit) + [256] + rng.sample(range(257, 270), n_len):
        lf[s] = 1 + rng.randrange(40)
    ll = dc.huffman_lengths(lf, 9)
    dl = dc.huffman_lengths([1 + rng.randrange(9) for _ in range(n_dist)], 8)
    return dc.trim(ll, 257), dl


def g_code_length_code(c, rng):
    ll, dl = small_code(rng)
    # HCLEN 19 although fewer would do; the code-length code at its 7-bit limit, every length coded on its own
    s = Stream(rng)
    toks, syms, cl = s.dynamic(ll, dl, hclen=19)
    c.add("cl_hclen19", "cl", s.w.getvalue(), s.out, dict(every_code=uses_every_code(toks, ll, dl), fewer_would_do=max(k for k in range(19) if cl[dc.CL_ORDER[k]]) < 18))
    l7, d7 = full_code(rng)
    s = Stream(rng, history(d7))
    toks, syms, cl = s.dynamic(l7, d7, syms=[(v, 0, 0) for v in l7 + d7], cl_skew=True)
    c.add("cl_seven_bit_code", "cl", s.w.getvalue(), s.out, dict(every_code=uses_every_code(toks, l7, d7), seven_bits=max(cl) == 7 and dc.kraft(cl) == 32768,
                                                                 it_is_used=any(cl[v] == 7 for v, _, _ in syms)))
    # HCLEN 4 reaches the symbols 16, 17, 18 and 0 only: a header made of nothing but runs, every length zero, no end-of-block code
    w = Bits()
    dc.put_dynamic_header(w, 1, 257, 1, [(18, 127, 7), (18, 120 - 11, 7)], hclen=4, cl_lens=[1 if x in (0, 18) else 0 for x in range(19)])
    w.put(0, 32)
    c.add("cl_hclen4_only_runs_all_zero", "cl", w.getvalue(), b"no end-of-block code", dict(runs_only=True, all_zero=expand([(18, 127, 7), (18, 109, 7)])[0] == [0] * 258), valid=False)
    # two symbols only (0 and 8, HCLEN 5): 1-bit codes; the same with 2-bit codes is incomplete, a third 1-bit code over-subscribes it
    l2 = [8] * 255 + [0, 8]
    singles = [(v, 0, 0) for v in l2 + [0]]
    s = Stream(rng, 0)
    toks, _, cl = s.dynamic(l2, [0], syms=singles)
    raw_ok, payload = s.w.getvalue(), bytes(s.out)
    c.add("cl_two_symbols", "cl", raw_ok, payload, dict(every_code=uses_every_code(toks, l2, [0]), two=sorted(x for x in cl if x) == [1, 1], hclen5=max(k for k in range(19) if cl[dc.CL_ORDER[k]]) == 4))
    for name, cl_lens in (("cl_incomplete", {0: 2, 8: 2}), ("cl_oversubscribed", {0: 1, 8: 1, 7: 1})):
        s = Stream(rng, 0)
        s.dynamic(l2, [0], syms=singles, toks=toks, cl_lens=lengths(19, cl_lens))
        k = sum(128 >> l for l in cl_lens.values())
        c.add(name, "cl", s.w.getvalue(), payload, dict(as_named=(k < 128) == (name == "cl_incomplete") and k != 128, zlib_reads_the_twin=True), valid=False)


def g_runs(c, rng):
    ll, dl = small_code(rng)
    ll = ll + [0] * (286 - len(ll))
    good = dc.rle_lengths(ll + dl)
    s = Stream(rng)
    toks, _, _ = s.dynamic(ll, dl)
    payload = bytes(s.out)
    c.add("run_valid_twin", "runs", s.w.getvalue(), payload, dict(every_code=uses_every_code(toks, ll, dl)))

    def variant(name, syms, facts, valid=False, l2=None, d2=None, **kw):
        s = Stream(rng)
        s.out = bytearray(payload[:NOISE])
        s.w = Bits()
        dc.put_stored(s.w, payload[:NOISE], 0)
        s.dynamic(ll if l2 is None else l2, dl if d2 is None else d2, syms=syms, toks=toks, **kw)
        c.add(name, "runs", s.w.getvalue(), payload, facts, valid=valid)
    variant("run16_is_the_first_symbol", [(16, 0, 2)] + good, dict(first=True, rest_is_the_twin=expand(good)[0] == ll + dl), hlit=286, hdist=len(dl))
    # 16 repeats the last literal / length length into the distance lengths
    fixed = {284: 5, 285: 5}
    l3 = lengths(286, complete(fixed, [256] + rng.sample(LITS, 10), avoid=(5,)))
    d3 = [5, 5, 5, 1, 2, 3, 5]
    syms = dc.rle_lengths(l3 + d3)
    out, at = expand(syms)
    s = Stream(rng)
    toks3, _, _ = s.dynamic(l3, d3)
    c.add("run16_crosses_the_hlit_border", "runs", s.w.getvalue(), s.out,
          dict(every_code=uses_every_code(toks3, l3, d3), crosses=any(x[0] == 16 and a < 286 < a + 3 + x[1] for x, a in zip(syms, at)), writes=out == l3 + d3, complete=dc.kraft(d3) == 32768))
    # 17 and 18 that end exactly at HLIT + HDIST, and one past it
    for sym, k in ((17, 5), (18, 12)):
        d4 = dl + [0] * k
        syms = dc.rle_lengths(ll + d4)
        last = syms[-1]
        s = Stream(rng)
        t4, _, _ = s.dynamic(ll, d4)
        c.add("run%d_ends_at_hlit_plus_hdist" % sym, "runs", s.w.getvalue(), s.out, dict(every_code=uses_every_code(t4, ll, d4), last_is_the_run=last[0] == sym and len(expand(syms)[0]) == 286 + len(d4)))
        over = syms[:-1] + [(last[0], last[1] + 1, last[2])]
        variant("run%d_ends_one_past" % sym, over, dict(one_past=len(expand(over)[0]) == 286 + len(d4) + 1), d2=d4)
    # an 18 of 138
    l5 = lengths(286, complete({}, [256, 257, 258] + [200 + k for k in range(12)]))
    s = Stream(rng)
    t5, syms, _ = s.dynamic(l5, dl)
    c.add("run18_of_138", "runs", s.w.getvalue(), s.out, dict(every_code=uses_every_code(t5, l5, dl), has_it=(18, 127, 7) in syms))
    # nearly nothing but runs (255 lengths of 8 from one 8 and repeats); no run at all: 316 single lengths
    l6 = [8] * 255 + [0, 8]
    s = Stream(rng, 0)
    t6, syms, _ = s.dynamic(l6, [0], syms=[(8, 0, 0)] + [(16, 3, 2)] * 41 + [(16, 2, 2), (16, 0, 2), (0, 0, 0), (8, 0, 0), (0, 0, 0)])
    c.add("runs_nearly_only", "runs", s.w.getvalue(), s.out, dict(every_code=uses_every_code(t6, l6, [0]), writes=expand(syms)[0] == l6 + [0], singles=sum(1 for x in syms if x[0] < 16) <= 4, runs=sum(1 for x in syms if x[0] >= 16) >= 40))
    l7, d7 = full_code(rng)
    s = Stream(rng, history(d7))
    t7, syms, _ = s.dynamic(l7, d7, syms=[(v, 0, 0) for v in l7 + d7])
    c.add("runs_none_316_single_lengths", "runs", s.w.getvalue(), s.out, dict(every_code=uses_every_code(t7, l7, d7), n=len(syms) == 316 and all(x[0] < 16 for x in syms)))


def full_code(rng):
    """Every one of the 286 + 30 symbols coded."""
    ll = dc.huffman_lengths([1 + rng.randrange(200) for _ in range(286)], 15)
    dl = dc.huffman_lengths([1 + rng.randrange(50) for _ in range(30)], 15)
    assert min(ll) > 0 and min(dl) > 0
    return ll, dl


def g_alphabet_sizes(c, rng):
    l1 = lengths(257, complete({}, [256] + rng.sample(LITS, 9)))
    s = Stream(rng, 0)
    t1, _, _ = s.dynamic(l1, [0])
    c.add("size_hlit257_hdist1", "sizes", s.w.getvalue(), s.out, dict(every_code=uses_every_code(t1, l1, [0]), no_distance_code=True))
    ll, dl = full_code(rng)
    s = Stream(rng, history(dl))
    toks, _, _ = s.dynamic(ll, dl)
    payload, hist = bytes(s.out), history(dl)
    c.add("size_hlit286_hdist30", "sizes", s.w.getvalue(), payload, dict(every_code=uses_every_code(toks, ll, dl), full=len(ll) == 286 and len(dl) == 30))

    def variant(name, l2, d2, facts):
        w = Bits()
        dc.put_stored(w, payload[:hist], 0)
        dc.put_dynamic_header(w, 1, len(l2), len(d2), dc.rle_lengths(l2 + d2))
        dc.put_tokens(w, toks, ll, dl)
        c.add(name, "sizes", w.getvalue(), payload, facts, valid=False)
    variant("size_hlit_field_30", ll + [0], dl, dict(field=len(ll) + 1 - 257 == 30))
    variant("size_hlit_field_31", ll + [0, 0], dl, dict(field=len(ll) + 2 - 257 == 31))
    variant("size_hdist_field_30", ll, dl + [0], dict(field=len(dl) + 1 - 1 == 30))
    variant("size_hdist_field_31", ll, dl + [0, 0], dict(field=len(dl) + 2 - 1 == 31))
    noeob = list(ll)
    noeob[256] = 0
    variant("size_no_end_of_block_code", noeob, dl, dict(none=noeob[256] == 0 and ll[256] > 0))


def g_ranks(c, rng):
    """Symbols of one length in every chunk of 64; a length whose two symbols are the first and the last; all 15 lengths at once."""
    dl = [1, 1]
    eights = list(range(0, 40)) + list(range(64, 104)) + list(range(128, 168)) + list(range(192, 232)) + list(range(256, 281))
    ll = lengths(286, complete({x: 8 for x in eights}, [50, 110, 180, 240, 250, 251, 252, 253], avoid=(8,)))
    s = Stream(rng)
    toks, _, _ = s.dynamic(ll, dl)
    per_chunk = [sum(1 for x in range(k, min(k + 64, 286)) if ll[x] == 8) for k in range(0, 320, 64)]
    c.add("rank_one_length_in_all_five_chunks", "ranks", s.w.getvalue(), s.out, dict(every_code=uses_every_code(toks, ll, dl), over_128=sum(per_chunk) > 128, every_chunk=min(per_chunk) > 0 and len(per_chunk) == 5))
    ll = lengths(286, complete({0: 3, 285: 3}, [256, 100, 65, 200, 270, 30], avoid=(3,)))
    s = Stream(rng)
    toks, _, _ = s.dynamic(ll, dl)
    c.add("rank_first_and_last_symbol_share_a_length", "ranks", s.w.getvalue(), s.out, dict(every_code=uses_every_code(toks, ll, dl), only_two=[x for x in range(286) if ll[x] == 3] == [0, 285]))
    order = [65, 285, 0, 256, 130, 63, 64, 257, 191, 192, 255, 127, 128, 10, 284, 200]
    ll = lengths(286, dict(zip(order, list(range(1, 15)) + [15, 15])))
    s = Stream(rng)
    toks, _, _ = s.dynamic(ll, dl)
    c.add("rank_all_15_lengths_at_once", "ranks", s.w.getvalue(), s.out, dict(every_code=uses_every_code(toks, ll, dl), all_15={x for x in ll if x} == set(range(1, 16)), complete=dc.kraft(ll) == 32768))


def spread(n, sorted_lens, rng, keep=()):
    """sorted_lens handed to symbols in a random order (the symbols of `keep` among them)."""
    syms = list(keep) + rng.sample([x for x in range(n) if x not in keep], len(sorted_lens) - len(keep))
    rng.shuffle(syms)
    return lengths(n, dict(zip(syms, sorted_lens)))


def g_sub_tables(c, rng):
    # the largest need a code of 286 / 30 symbols can have
    need_l, sorted_l = largest_need(D_LIT_TB, 286)
    need_d, sorted_d = largest_need(D_DIST_TB, 30)
    ll, dl = spread(286, sorted_l, rng, keep=(256,)), spread(30, sorted_d, rng)
    s = Stream(rng, history(dl))
    toks, _, _ = s.dynamic(ll, dl)
    c.add("sub_largest_need", "sub", s.w.getvalue(), s.out,
          dict(every_code=uses_every_code(toks, ll, dl), complete=dc.kraft(ll) == 32768 and dc.kraft(dl) == 32768, has_it=dc.subtable_need(ll, D_LIT_TB)[0] == need_l and dc.subtable_need(dl, D_DIST_TB)[0] == need_d,
               fits=need_l <= D_LIT_MAX - 512 and need_d <= D_DIST_MAX - 256,
               # ... nor does a literal / length code that is merely not over-subscribed, of the 288 lengths of a fixed block even, go over
               no_literal_code_is_over_budget=largest_need(D_LIT_TB, 288, False)[0] <= D_LIT_MAX - 512))
    # an incomplete distance code can: its last prefix holds one code of 15 bits alone.  zlib refuses the code for being incomplete
    need_i, sorted_i = largest_need(D_DIST_TB, 30, False)
    di = spread(30, sorted_i, rng)
    li = lengths(286, complete({}, [256] + rng.sample(LITS, 9)))
    s = Stream(rng, 0)
    s.dynamic(li, di, toks=cover(li, [0], 0, rng))
    c.add("sub_over_budget_incomplete_distance_code", "sub", s.w.getvalue(), s.out,
          dict(over_budget=dc.subtable_need(di, D_DIST_TB)[0] == need_i > D_DIST_MAX - 256, incomplete_not_oversubscribed=dc.kraft(di) < 32768 and len(di) == 30), valid=False)
    # exactly one prefix carries long codes, of two lengths: the sub-table is sized by the longer.  All long codes of one length under one prefix
    d2 = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10][::-1]
    for name, tail, bits in (("sub_one_prefix_two_lengths", [10, 11, 12, 12], 3), ("sub_one_prefix_one_length", [12] * 8, 3)):
        ll = spread(286, list(range(1, 10)) + tail, rng, keep=(256, 257))
        s = Stream(rng)
        toks, _, _ = s.dynamic(ll, d2)
        codes = dc.canonical(ll)
        under = {codes[x] & 511 for x in range(286) if ll[x] > 9}
        c.add(name, "sub", s.w.getvalue(), s.out, dict(every_code=uses_every_code(toks, ll, d2), one_prefix=len(under) == 1 and dc.subtable_need(ll, 9) == (1 << bits, 1),
                                                      lengths_as_named=len({l for l in ll if l > 9}) == (3 if "two" in name else 1), sized_by_the_longest=max(ll) - 9 == bits,
                                                      distance_too=dc.subtable_need(d2, 8) == (4, 1)))


def g_distance_codes(c, rng):
    l1 = lengths(286, complete({}, [256] + rng.sample(LITS, 9)))
    s = Stream(rng, 0)
    t1, _, _ = s.dynamic(l1, [0] * 30)
    c.add("dist_all_30_lengths_zero", "dist", s.w.getvalue(), s.out, dict(every_code=uses_every_code(t1, l1, [0] * 30), literals_only=all(type(t) is int for t in t1)))
    l2 = lengths(286, complete({}, [256, 257, 260, 285] + rng.sample(LITS, 9)))
    for name, d2, valid in (("dist_single_code", [0, 0, 0, 1], True), ("dist_oversubscribed", [1, 1, 0, 1], False)):
        s = Stream(rng)
        if valid:
            t2, _, _ = s.dynamic(l2, d2)
            keep = (list(t2), bytes(s.out))
            facts = dict(every_code=uses_every_code(t2, l2, d2), incomplete=dc.kraft(d2) == 16384)
        else:
            s.out = bytearray(keep[1][:NOISE])
            s.w = Bits()
            dc.put_stored(s.w, keep[1][:NOISE], 0)
            dc.put_dynamic_header(s.w, 1, 286, len(d2), dc.rle_lengths(l2 + d2))
            dc.put_tokens(s.w, keep[0], l2, [0, 0, 0, 1])
            s.out = bytearray(keep[1])
            facts = dict(oversubscribed=dc.kraft(d2) > 32768)
        c.add(name, "dist", s.w.getvalue(), s.out, facts, valid=valid)


def g_several_blocks(c, rng):
    """One BGZF block, five DEFLATE blocks that share the LDS: the table build must take nothing over from the one before it."""
    deep_l = spread(286, list(range(1, 10)) + [10, 11, 12, 13, 14, 15, 15], rng, keep=(256, 257))
    deep_d = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 11][::-1]
    flat_l = lengths(286, complete({}, [256, 258, 259] + rng.sample(LITS, 14)))
    flat_d = [2, 2, 2, 2]
    third_l, third_d = small_code(rng)
    for name, first, second in (("deep_first", (deep_l, deep_d), (flat_l, flat_d)), ("flat_first", (flat_l, flat_d), (deep_l, deep_d))):
        s = Stream(rng)
        ta, _, _ = s.dynamic(*first, final=0)
        s.fixed([65, 67, (5, 2), 200, 71], 0)
        tb, _, _ = s.dynamic(*second, final=0)
        s.stored(bytes(rng.randrange(256) for _ in range(23)))
        tc, _, _ = s.dynamic(third_l, third_d, final=1)
        need = lambda code: (dc.subtable_need(code[0], 9)[0], dc.subtable_need(code[1], 8)[0])
        c.add("several_blocks_" + name, "several", s.w.getvalue(), s.out,
              dict(every_code=uses_every_code(ta, *first) and uses_every_code(tb, *second) and uses_every_code(tc, third_l, third_d),
                   deep_needs_sub_tables=min(need((deep_l, deep_d))) > 0, flat_needs_none=need((flat_l, flat_d)) == (0, 0), third_needs_none=need((third_l, third_d)) == (0, 0),
                   order_as_named=(need(first)[0] > 0) == (name == "deep_first")))


GROUPS = (g_code_length_code, g_runs, g_alphabet_sizes, g_ranks, g_sub_tables, g_distance_codes, g_several_blocks)
REPEATS = 8                                                            # every group under eight seeds: other symbols, other codes


@functools.lru_cache(maxsize=None)
def corpus(seed=20250911):
    """(file bytes, records): one record per BGZF block; the invalid blocks stand between valid ones, whose bytes must come back intact."""
    c = Cases()
    for rep in range(REPEATS):
        for k, g in enumerate(GROUPS):
            n0 = len(c.entries)
            g(c, random.Random(seed * 1000 + rep * 10 + k))
            for e in c.entries[n0:]:
                e["name"] += "_seed%d" % rep
    valid, invalid = [e for e in c.entries if e["valid"]], [e for e in c.entries if not e["valid"]]
    assert len(valid) > len(invalid) + 1
    order = []
    for k, e in enumerate(invalid):
        order += [valid[k], e]
    order += valid[len(invalid):]
    parts, recs, off = [], [], 0
    for e in order:
        recs.append(dict(name=e["name"], group=e["group"], valid=e["valid"], payload=e["payload"], offset=off, facts=e["facts"]))
        parts.append(e["blk"])
        off += len(e["blk"])
    assert recs[0]["valid"] and recs[-1]["valid"] and len({r["name"] for r in recs}) == len(recs)
    return b"".join(parts), recs


# ---- the tests -----------------------------------------------------------------------------------------------------------------
def test_every_case_is_what_it_is_named_for():
    _, recs = corpus()
    wrong = {r["name"]: [k for k, v in r["facts"].items() if v is not True] for r in recs}
    wrong = {n: ks for n, ks in wrong.items() if ks}
    assert not wrong, wrong
    assert all(r["facts"] for r in recs)
    assert all("every_code" in r["facts"] for r in recs if r["valid"])


def test_the_corpus_holds_every_case_of_the_list():
    _, recs = corpus()
    names = {r["name"] for r in recs}
    want = ["cl_hclen19", "cl_seven_bit_code", "cl_hclen4_only_runs_all_zero", "cl_two_symbols", "cl_incomplete", "cl_oversubscribed",
            "run_valid_twin", "run16_is_the_first_symbol", "run16_crosses_the_hlit_border", "run17_ends_at_hlit_plus_hdist", "run17_ends_one_past",
            "run18_ends_at_hlit_plus_hdist", "run18_ends_one_past", "run18_of_138", "runs_nearly_only", "runs_none_316_single_lengths",
            "size_hlit257_hdist1", "size_hlit286_hdist30", "size_hlit_field_30", "size_hlit_field_31", "size_hdist_field_30", "size_hdist_field_31",
            "size_no_end_of_block_code", "rank_one_length_in_all_five_chunks", "rank_first_and_last_symbol_share_a_length", "rank_all_15_lengths_at_once",
            "sub_largest_need", "sub_over_budget_incomplete_distance_code", "sub_one_prefix_two_lengths", "sub_one_prefix_one_length", "dist_all_30_lengths_zero", "dist_single_code",
            "dist_oversubscribed", "several_blocks_deep_first", "several_blocks_flat_first"]
    for rep in range(REPEATS):
        assert {"%s_seed%d" % (n, rep) for n in want} <= names
    assert 200 <= len(recs) <= 400
    invalid = [r["name"].rsplit("_seed", 1)[0] for r in recs if not r["valid"]]
    assert sorted(set(invalid)) == sorted(["cl_hclen4_only_runs_all_zero", "cl_incomplete", "cl_oversubscribed", "run16_is_the_first_symbol", "run17_ends_one_past", "run18_ends_one_past",
                                           "size_hlit_field_30", "size_hlit_field_31", "size_hdist_field_30", "size_hdist_field_31", "size_no_end_of_block_code", "dist_oversubscribed", "sub_over_budget_incomplete_distance_code"])


def test_no_code_needs_more_sub_table_than_the_budget():
    """The largest needs, and what they are held against (the search is largest_need's; the witness is in the corpus)."""
    assert largest_need(D_LIT_TB, 286)[0] <= D_LIT_MAX - 512 and largest_need(D_DIST_TB, 30)[0] <= D_DIST_MAX - 256
    for root, n in ((D_LIT_TB, 286), (D_DIST_TB, 30)):
        need, lens = largest_need(root, n)
        assert lens == sorted(lens) and len(lens) <= n and dc.kraft(lens) == 32768 and dc.subtable_need(lens, root)[0] == need
        for n15 in range(2, n, 2):                                     # no code of fill_lengths' family needs more
            try:
                assert dc.subtable_need(dc.fill_lengths(n, n15, 15), root)[0] <= need
            except AssertionError as e:
                if "too few symbols" not in str(e) and "cannot place" not in str(e):
                    raise


def test_zlib_reads_the_file_block_by_block_as_intended():
    data, recs = corpus()
    blocks = dc.bgzf_blocks(data)
    assert len(blocks) == len(recs)
    for (off, raw, isize), r in zip(blocks, recs):
        assert off == r["offset"] and isize == len(r["payload"])
        ok, out = dc.zlib_verdict(raw, isize)
        assert ok == r["valid"], r["name"]
        if ok:
            assert out == r["payload"], r["name"]
    for i, r in enumerate(recs):                                       # every invalid block has valid neighbours
        if not r["valid"]:
            assert recs[i - 1]["valid"] and recs[i + 1]["valid"], r["name"]
