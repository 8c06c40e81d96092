"""The corpus of tests/test_inflate_streams_host.py and tests/test_gpu_inflate_streams.py: a few hundred named BGZF blocks written
by tests/deflate_craft.py - the parts of DEFLATE that zlib's compressor never uses and that the decoders of csrc/inflate_dev.hip and
csrc/inflate_fast.h have exact-boundary logic for - plus about twenty streams that are wrong in one place each.  Every stream is held
against zlib's inflate when it is made (deflate_craft.check).  `corpus()` returns the file's bytes and one record per BGZF block."""
import functools
import random

import deflate_craft as dc
from deflate_craft import Bits

# Valid blocks a decoder may leave to its fallback by design, by name, with the reason next to the block's definition.  (Empty: a
# complete code never exceeds the device's sub-table budget - DESIGN.md section 6 - and nothing else makes it decline a valid stream.)
MAY_BE_LEFT = frozenset()


# ---- payloads ------------------------------------------------------------------------------------------------------------
def bam_like(rng, n):
    out = bytearray()
    i = rng.randrange(100000)
    while len(out) < n:
        out += b"%04d\0read%06d\0" % (i % 7919, i) + bytes(rng.randrange(4) * 17 for _ in range(20)) + rng.choice((b"IIIIFFFF", b"FFFF,,::")) * 5
        out += b"CBZ" + bytes(rng.choice(b"ACGT") for _ in range(8)) + b"-1\0UBZACGTACGTAC\0"
        i += 1
    return bytes(out[:n])


def acgt(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def rand_bytes(rng, n):
    # (65536 bytes of full-range noise do not fit a BGZF block whatever the writer does: the largest size draws from 64 values)
    return bytes(rng.randrange(256 if n <= 20000 else 64) for _ in range(n))


def short_period(rng, n):
    p = rng.choice((1, 2, 3, 5, 7, 64, 259))
    unit = bytes(rng.randrange(256) for _ in range(p))
    out = bytearray((unit * (n // p + 1))[:n])
    for _ in range(n // 500):                                         # a few breaks, so that the parse is not one match
        out[rng.randrange(n)] = rng.randrange(256)
    return bytes(out)


KINDS = (("bam", bam_like), ("acgt", acgt), ("rand", rand_bytes), ("period", short_period))
SIZES = (1, 2, 5, 63, 64, 65, 300, 4000, 20000, 65536)


class Corpus:
    def __init__(self):
        self.entries = []                                             # dicts: name, group, blk, payload, valid, want_a
        self.parse_payloads = []                                      # (name, payload) of the random-parse group

    def add(self, name, group, raw, payload, valid=True, want_a=None):
        payload = bytes(payload)
        dc.check(raw, payload, valid)
        assert len(payload) > 0, name                                  # (an empty block never reaches a decoder)
        self.entries.append(dict(name=name, group=group, blk=dc.bgzf(raw, payload), payload=payload, valid=valid, want_a=want_a))


def _dyn(tokens, litlens, distlens, final=1, w=None, **kw):
    w = Bits() if w is None else w
    dc.put_dynamic(w, tokens, final, litlens, distlens, **kw)
    return w


def _assign(n_sym, lengths, short_first):
    """A length array over n_sym symbols: the ascending `lengths` go to the symbols of `short_first` in its order, the rest after."""
    order = list(short_first) + [s for s in range(n_sym) if s not in set(short_first)]
    out = [0] * n_sym
    for s, l in zip(order, lengths):
        out[s] = l
    return out


def _random_tokens(rng, n, literals, lengths, dists, p_match=0.5, start=()):
    """Tokens drawn from the given literals / match lengths / distances (a distance that reaches before the start becomes a literal)."""
    toks, pos = list(start), sum(dc.token_lengths(start))
    for _ in range(n):
        d = rng.choice(dists)
        if rng.random() < p_match and d <= pos:
            t = (rng.choice(lengths), d)
            pos += t[0]
        else:
            t = rng.choice(literals)
            pos += 1
        toks.append(t)
    return toks


# ---- the groups ----------------------------------------------------------------------------------------------------------
def g_random_parse(c, rng):
    """Random parses of four kinds of data at ten sizes, cut into 1 .. ~400 DEFLATE blocks of mixed type per BGZF block."""
    for kname, gen in KINDS:
        for size in SIZES:
            payload = gen(rng, size)
            c.parse_payloads.append(("%s_%d" % (kname, size), payload))
            cuts = (1, 2, 5, 40, 400) if size >= 4000 else (1, 2, 5) if size >= 63 else (1, 2) if size > 1 else (1,)
            for nb in cuts:
                raw = dc.deflate_random_fit(payload, rng, nb)
                c.add("parse_%s_%d_x%d" % (kname, size, nb), "parse", raw, payload)


def g_headers(c, rng):
    text = bytes(rng.choice(b"ACGTN\n\t!#IF:,0123456789abcdefXYZxyz-_=+*") for _ in range(3000))
    # a run of code 16 across the border: the last literal/length lengths and the first distance lengths are equal and not zero
    for k, (n15, x) in enumerate(((2, None), (20, None), (64, None))):
        ll_set, dl_set = dc.fill_lengths(286, n15 + 20, 15, rng), dc.fill_lengths(30, 2, 9 + k, rng)
        x = max(set(ll_set) & set(dl_set), key=lambda v: min(ll_set.count(v), dl_set.count(v)))
        assert ll_set.count(x) >= 3 and dl_set.count(x) >= 3, (ll_set, dl_set)
        ll_rest, dl_rest = list(ll_set), list(dl_set)
        for _ in range(3):
            ll_rest.remove(x)
            dl_rest.remove(x)
        rng.shuffle(ll_rest)
        rng.shuffle(dl_rest)
        ll, dl = ll_rest + [x] * 3, [x] * 3 + dl_rest
        toks = dc.tokenize(text, rng)
        syms = dc.rle_lengths(ll + dl)
        at = 0
        crossing = []
        for s, xv, nb in syms:
            n = 1 if s < 16 else xv + (3 if s < 18 else 11)
            if at < 286 < at + n:
                crossing.append(s)
            at += n
        assert crossing == [16], crossing
        c.add("hdr_run16_crosses_border_%d" % k, "header", _dyn(toks, ll, dl).getvalue(), text)
    # runs of zeros across the border (codes 17 and 18), the longest of them ending exactly at HLIT + HDIST.  (A run of 138 cannot
    # end there in a valid stream: the end-of-block symbol 256 has a code and HLIT + HDIST <= 316, so at most 59 lengths follow it.
    # The 138-run is inside the literals instead, and "hdr_run18_to_tot" has the 59.)
    low = bytes(rng.randrange(32, 100) for _ in range(2000))
    toks = list(low)
    lf = [0] * 286
    for b in range(32, 100):
        lf[b] = 1 + rng.randrange(50)
    lf[256] = 1
    ll = dc.huffman_lengths(lf, 9)
    syms = dc.rle_lengths(ll + [0] * 30)
    assert syms[-1] == (18, 59 - 11, 7) and (18, 138 - 11, 7) in syms, syms[-4:]
    c.add("hdr_run18_to_tot", "header", _dyn(toks, ll, [0] * 30).getvalue(), low)
    # zeros across the border with code 17: the last 4 length symbols and the first 4 distance symbols are unused
    toks = dc.tokenize(text, rng, min_dist=5, max_len=114)
    lf, _ = dc.frequencies(toks)
    ll = dc.huffman_lengths([f + 1 for f in lf[:282]], 15) + [0] * 4
    dl = dc.huffman_lengths([0] * 4 + [1 + rng.randrange(9) for _ in range(26)], 15)
    syms = dc.rle_lengths(ll + dl)
    assert (17, 8 - 3, 3) in syms and dc.kraft(dl) == 32768 and dc.kraft(ll) == 32768
    c.add("hdr_run17_crosses_border", "header", _dyn(toks, ll, dl).getvalue(), text)
    # HLIT = 257 with HDIST = 1 of length 0: no distance code at all
    ll, _ = dc.auto_lengths(list(text))
    assert len(ll) == 257
    c.add("hdr_literals_only_hdist1_len0", "header", _dyn(list(text), ll, [0]).getvalue(), text)
    # one distance code of length 1 (the incomplete code zlib permits): distance 1 only
    runs = b"".join(bytes([rng.randrange(256)]) * rng.randrange(1, 40) for _ in range(300))
    toks = dc.tokenize(runs, rng, max_dist=1, p_near=1.0)
    assert any(type(t) is tuple for t in toks)
    ll, dl = dc.auto_lengths(toks)
    assert dl == [1]
    c.add("hdr_one_distance_code_len1", "header", _dyn(toks, ll, dl).getvalue(), runs)
    # the same with the single code on distance symbol 29 (HDIST = 30): distances 24577 .. 32768 only
    far = bytes(rng.getrandbits(8) for _ in range(25000))
    far = far + far[:12000] + far[8000:12000]
    toks = dc.tokenize(far, rng, min_dist=24577, p_match=1.0, p_longest=0.6)
    assert sum(1 for t in toks if type(t) is tuple) > 50
    ll, dl = dc.auto_lengths(toks)
    assert dl == [0] * 29 + [1]
    w = Bits()
    dc.put_stored(w, far[:10000], 0)
    k = 10000
    assert all(type(t) is int for t in toks[:k])                       # (no match before position 24577)
    c.add("hdr_one_distance_code_sym29", "header", _dyn(toks[k:], ll, dl, w=w).getvalue(), far)
    # HLIT = 286 and HDIST = 30 with every symbol coded; HCLEN = 19 although fewer would do; a run-length coding cut at random
    toks = dc.tokenize(text, rng)
    ll, dl = dc.auto_lengths(toks, full=True)
    ll = dc.huffman_lengths([1 << (15 - l) if l else 1 for l in ll], 15)
    dl = dc.huffman_lengths([1 << (15 - l) if l else 1 for l in dl], 15)
    assert min(ll) > 0 and min(dl) > 0 and len(ll) == 286 and len(dl) == 30
    c.add("hdr_hlit286_hdist30_all_coded", "header", _dyn(toks, ll, dl).getvalue(), text)
    c.add("hdr_hclen19", "header", _dyn(toks, ll, dl, hclen=19).getvalue(), text)
    c.add("hdr_random_rle", "header", _dyn(toks, ll, dl, rng=rng).getvalue(), text)
    # the smallest HCLEN of a valid stream.  (HCLEN = 4 reaches only the code-length symbols 16, 17, 18 and 0: every length would
    # be zero, the end-of-block code among them - that header is in the invalid group.)  HCLEN = 5 adds symbol 8: 256 codes of 8 bits.
    vals = list(range(255))
    payload = bytes(rng.choice(vals) for _ in range(1500))
    ll = [8] * 255 + [0, 8]
    w = Bits()
    cl = dc.put_dynamic_header(w, 1, 257, 1, dc.rle_lengths(ll + [0]))
    assert max(k for k in range(19) if cl[dc.CL_ORDER[k]]) == 4
    dc.put_tokens(w, list(payload), ll, [0])
    c.add("hdr_hclen5_minimum", "header", w.getvalue(), payload)
    # a code-length code with 7-bit codes
    toks = dc.tokenize(text, rng)
    ll, dl = dc.auto_lengths(toks, rng, 15, 15)
    w = Bits()
    cl = dc.put_dynamic_header(w, 1, len(ll), len(dl), [(v, 0, 0) for v in ll + dl], cl_skew=True)
    assert max(cl) == 7, cl
    dc.put_tokens(w, toks, ll, dl)
    c.add("hdr_code_length_code_7_bits", "header", w.getvalue(), text)


def g_deep(c, rng):
    """Codes at the 15-bit limit: the tail of the code space, spread over as many first-level prefixes as a complete code can."""
    for n15 in (2, 66, 130, 194, 258, 270):
        ll_sorted = dc.fill_lengths(286, n15, 15, rng if n15 % 4 else None)
        syms = list(range(286))
        rng.shuffle(syms)
        ll = _assign(286, ll_sorted, syms)
        need, prefixes = dc.subtable_need(ll, 9)
        assert need <= 768, need
        if n15 >= 258:
            assert prefixes >= 5, prefixes
        dl = _assign(30, dc.fill_lengths(30, 2, 15, rng), rng.sample(range(30), 30))
        dneed, _ = dc.subtable_need(dl, 8)
        assert dneed <= 256
        toks = list(bytes(rng.randrange(256) for _ in range(300)))
        toks = _random_tokens(rng, 6000, list(range(256)), [dc.LEN_BASE[k] + rng.randrange(1 << dc.LEN_EXTRA[k]) for k in range(29)] * 3,
                              [dc.DIST_BASE[k] + rng.randrange(1 << dc.DIST_EXTRA[k]) for k in range(30)] * 3, 0.1, toks)
        payload = dc.detok(toks)
        assert len(payload) <= 65536
        c.add("deep_lit15_%d_codes_%d_prefixes_need_%d" % (n15, prefixes, need), "deep", _dyn(toks, ll, dl).getvalue(), payload)
    chain = list(range(1, 15)) + [15, 15]
    variants = [("chain", chain + [0] * 14), ("chain_reversed", [0] * 14 + chain[::-1])]
    for k in range(6):
        variants.append(("fill%d" % k, _assign(30, dc.fill_lengths(30, 2 + 2 * k, 15, rng), rng.sample(range(30), 30))))
    for name, dl in variants:
        dneed, dpre = dc.subtable_need(dl, 8)
        assert dneed <= 256, dneed
        dists = [dc.DIST_BASE[k] + rng.randrange(1 << dc.DIST_EXTRA[k]) for k in range(30) if dl[k]] * 3
        toks = _random_tokens(rng, 4000, list(b"ACGTNacgtn"), [3, 4, 5, 6, 9, 17, 40], dists, 0.5, list(acgt(rng, 300)))
        ll, _ = dc.auto_lengths(toks)
        payload = dc.detok(toks)
        assert len(payload) <= 65536
        c.add("deep_dist_%s_need_%d_in_%d" % (name, dneed, dpre), "deep", _dyn(toks, ll, trim_dist(dl)).getvalue(), payload)


def trim_dist(dl):
    return dc.trim(list(dl), 1)


def g_longest(c, rng):
    """Matches of 48 bits: a 15-bit length code + 5 extra bits + a 15-bit distance code + 13 extra bits, hundreds in a row, 0 .. 7
    short literals between them.  Such a match makes at least 131 bytes from at least 16385 bytes back, so one 64 KiB BGZF block
    holds a few hundred of them, not 500: the 500 are spread over three blocks."""
    lits = [65, 67, 71, 84]
    # lengths 131 .. 258 are symbols 281 .. 285; all of 277 .. 285 and the two last distance symbols get 15-bit codes
    deep_l = [281, 282, 283, 284, 285, 277, 278, 279, 280, 270]
    ll = _assign(286, dc.fill_lengths(286, 10, 15), lits + [256] + [s for s in range(286) if s not in lits + [256] + deep_l] + deep_l)
    assert all(ll[s] == 15 for s in deep_l[:5]) and all(ll[s] <= 4 for s in lits), [ll[s] for s in lits]
    dl = _assign(30, dc.fill_lengths(30, 2, 15), [s for s in range(28)] + [28, 29])
    assert dl[28] == dl[29] == 15
    total = 0
    for name, preface, alt in (("at_32768", 32768, False), ("a", 16385, True), ("b", 20011, False), ("c", 16390, True)):
        out = bytearray(rng.getrandbits(8) for _ in range(preface))
        w = Bits()
        dc.put_stored(w, bytes(out), 0)
        toks, pos = [], preface
        if preface == 32768:
            toks.append((258, 32768))                                  # output position 32768, distance 32768: the block's byte 0
            pos += 258
        while True:
            l = rng.choice((131, 131, 132, 140, 163, 200, 257, 258))
            d = rng.randint(16385, min(32768, pos))
            extra = [rng.choice(lits) for _ in range(rng.randrange(8))]
            if pos + l + len(extra) > 65536:
                break
            toks += [(l, d)] + extra
            pos += l + len(extra)
        assert sum(1 for t in toks if t == (258, 32768) or type(t) is tuple and t[0] == 258) >= 3   # 258 as code 285 (43 bits) or, alt, as 284 + 31 (48)
        bits = dc.put_dynamic(w, toks, 1, ll, dl, l258_alt=alt)[0]
        assert not alt or sum(1 for t, b in zip(toks, bits) if type(t) is tuple and t[0] == 258 and b == 48) >= 3
        n48 = sum(1 for b in bits if b == 48)                          # (length 258 as code 285 has no extra bits: 43)
        assert n48 >= 150 and all(b >= 43 for t, b in zip(toks, bits) if type(t) is tuple), n48
        total += n48
        payload = dc.detok(toks, out)
        assert len(payload) == pos
        c.add("longest_48bit_%s_%d_matches" % (name, n48), "longest", w.getvalue(), payload)
    assert total >= 500, total


def round_view(tokens, bits, op0):
    """What the device's first 64-offset round of a DEFLATE block holds: the symbols that start in its first 64 bits.  Returns the
    sum of its match lengths, whether a later match reads what an earlier one of the round writes (the kernel's dependency test:
    source end > first match's destination), and whether some later match's source ends exactly at that destination."""
    pos, off, ms = 0, op0, []
    for t, b in zip(tokens, bits):
        if pos >= 64:
            break
        if type(t) is tuple:
            ms.append((off, t[0], t[1]))
        off += 1 if type(t) is int else t[0]
        pos += b
    first = ms[0][0] if ms else None
    ends = [o - d + min(l, d) for o, l, d in ms if o != first]
    return dict(n=len(ms), mtot=sum(m[1] for m in ms), dep=any(e > first for e in ends), touch=any(e == first for e in ends),
                lits_before=first is not None and first > op0)


def g_batching(c, rng):
    """The batched match copy of the device (all matches of a 64-offset round in one load / store pair when their lengths sum to at
    most 64 and none reads what an earlier one writes): every scenario is the first round of a DEFLATE block of its own, behind a
    stored block of noise to copy from; short codes, so that a round holds many symbols.  round_view() asserts what each round is."""
    F = 20                                                             # filler literals after a scenario: the round holds nothing else
    far = lambda k: 70 + k                                             # a distance no match of the same round can depend on
    scen = {
        "sum_64": ([(18, far(0)), (18, far(1)), (18, far(2)), (5, far(3)), (5, far(4))], dict(mtot=64, dep=False, n=5)),
        "sum_65": ([(18, far(0)), (18, far(1)), (18, far(2)), (5, far(3)), (6, far(4))], dict(mtot=65, dep=False, n=5)),
        "sum_63": ([(18, far(0)), (18, far(1)), (18, far(2)), (5, far(3)), (4, far(4))], dict(mtot=63, dep=False, n=5)),
        # the second match's source ends exactly at the first one's destination: not a dependency by the kernel's own test ...
        "source_ends_at_first_dst": ([(10, far(0)), (5, 15), (4, far(2))], dict(dep=False, touch=True, n=3)),
        "source_ends_at_first_dst_lit_between": ([(10, far(0)), 65, (5, 16), (4, far(2))], dict(dep=False, touch=True, n=3)),
        # ... and one byte further it is one
        "source_one_past_first_dst": ([(10, far(0)), (5, 14), (4, far(2))], dict(dep=True, n=3)),
        "source_one_past_first_dst_lit_between": ([(10, far(0)), 65, (5, 15), (4, far(2))], dict(dep=True, n=3)),
        "source_is_previous_match": ([(10, far(0)), (10, 10), (10, 20), (10, 5)], dict(dep=True, n=4)),
        # a match that reads literals stored in the same round
        "reads_literals_of_the_round": ([65, 67, 71, (6, 3), (4, far(1))], dict(dep=False, n=2, lits_before=True)),
        "reads_literal_dist1": ([(5, far(0)), 84, (9, 1), 65, (3, 2)], dict(dep=True, n=3)),
        # overlapping matches (distance < length) in a batch: as the first match they are batched, later ones depend
        "overlap_d1_first": ([71, (18, 1), (5, far(1)), (5, far(2))], dict(dep=False, n=3, lits_before=True)),
        "overlap_d2_first": ([65, 67, (17, 2), (6, far(1)), (3, far(2))], dict(dep=False, n=3, lits_before=True)),
        "overlap_d3_first": ([65, 67, 71, (10, 3), (10, far(1))], dict(dep=False, n=2, lits_before=True)),
        "overlap_later": ([(6, far(0)), (9, 1), (9, 2), (9, 3)], dict(dep=True, n=4)),
        "overlap_alone_64": ([84, (40, 1), (24, 3)], dict(dep=True, mtot=64, n=2)),
    }
    names = sorted(scen)
    alltoks = [t for n in names for t in scen[n][0]] + [65, 67, 71, 84]
    ll, dl = dc.auto_lengths(alltoks)
    assert max(ll) <= 6 and max(dl) <= 6, (max(ll), max(dl))       # (the codes of what the scenarios use most are 1 - 3 bits)
    for rep in range(3):                                               # three blocks: the scenarios in another order, at other positions
        order = names[:]
        rng.shuffle(order)
        out = bytearray(rand_bytes(rng, 150 + 37 * rep))
        w = Bits()
        dc.put_stored(w, bytes(out), 0)
        for k, n in enumerate(order):
            toks, want = scen[n]
            toks = toks + [rng.choice((65, 67, 71, 84)) for _ in range(F)]
            op0 = len(out)
            bits = dc.put_dynamic(w, toks, int(k == len(order) - 1), ll, dl)[0]
            view = round_view(toks, bits, op0)
            for key, v in want.items():
                assert view[key] == v, (n, key, view)
            dc.detok(toks, out)
        c.add("batch_scenarios_%d" % rep, "batching", w.getvalue(), out)
    # the same alphabet at random: thousands of rounds, their edges met by chance (and counted)
    for rep in range(4):
        start = list(rand_bytes(rng, 100))
        toks = _random_tokens(rng, 6000, [65, 67, 71, 84], [3, 5, 6, 9, 10, 17, 18], [1, 2, 3, 14, 15, 16] + [70, 71, 72, 90] * 4, 0.8, start)
        ll2, dl2 = dc.auto_lengths(toks[100:])
        w = Bits()
        dc.put_fixed(w, toks[:100], 0)
        bits = dc.put_dynamic(w, toks[100:], 1, ll2, dl2)[0]
        # walk the rounds as the kernel does
        seen, i, op, body = set(), 0, 100, toks[100:]
        while i < len(body):
            j, pos = i, 0
            while j < len(body) and pos < 64:
                pos += bits[j]
                j += 1
            v = round_view(body[i:j], bits[i:j], op)
            if v["n"] >= 2 and not v["dep"]:
                seen.add("mtot%d" % v["mtot"] if v["mtot"] in (63, 64, 65) else "batched")
                if v["touch"]:
                    seen.add("touch")
            op += sum(dc.token_lengths(body[i:j]))
            i = j
        assert {"mtot64", "mtot65", "touch", "batched"} <= seen, seen
        payload = dc.detok(toks)
        assert len(payload) <= 65536
        c.add("batch_random_%d" % rep, "batching", w.getvalue(), payload)
    # a match whose distance is its own output position: it reaches byte 0 of the block
    for k in (1, 2, 3, 4, 63, 64, 65, 300):
        toks = list(rand_bytes(rng, k)) + [(min(258, 3 + k), k)] + [65, (5, k + 1)]
        ll, dl = dc.auto_lengths(toks)
        c.add("match_reaches_byte_0_after_%d" % k, "batching", _dyn(toks, ll, dl).getvalue(), dc.detok(toks))


STORED_LENS = (0, 1, 2, 3, 4, 1023, 1024, 1025)


def g_stored(c, rng):
    """Stored blocks behind Huffman blocks that end at each of the 8 bit phases, of the lengths at which the hand-back of the bit
    position changes, each at every alignment A of the stream's address."""
    for a in range(4):
        phases = set()
        for j in range(8):
            w, out = Bits(), bytearray()

            def fixed(n_hi, n_lo, final=0):
                toks = [rng.randrange(144, 256) for _ in range(n_hi)] + [rng.randrange(144) for _ in range(n_lo)]
                rng.shuffle(toks)
                dc.put_fixed(w, toks, final)
                out.extend(toks)

            def stored(n, final=0, after_huffman=False):
                if after_huffman:
                    phases.add(w.total % 8)                            # the bit phase at which the Huffman block before it ends
                data = rand_bytes(rng, n)
                dc.put_stored(w, data, final)
                out.extend(data)
            fixed(j, 2)
            stored(STORED_LENS[j], after_huffman=True)
            fixed(0, 1)
            stored(STORED_LENS[(j + 3) % 8])
            if j % 2 == 0:
                for _ in range(3):
                    stored(0)                                          # several empty stored blocks in a row, none final
            if j % 4 == 1:                                             # a dynamic block between stored ones
                seg = bytes(out[-64:]) * 2
                toks = dc.tokenize(seg, rng)
                ll, dl = dc.auto_lengths(toks)
                dc.put_dynamic(w, toks, 0, ll, dl)
                out.extend(seg)
                stored(STORED_LENS[(j + 5) % 8])
            if j < 4:
                stored(STORED_LENS[7 - j] or 7, 1)                     # a final stored block
            else:
                fixed(j, 3, 1)                                         # stored, then fixed
            c.add("stored_A%d_phase%d" % (a, j), "stored", w.getvalue(), out, want_a=a)
        assert len(phases) == 8, phases
        # stored, fixed, stored
        w, out = Bits(), bytearray()
        for n, final in ((5, 0), (None, 0), (9, 1)):
            if n is None:
                toks = list(rand_bytes(rng, 11))
                dc.put_fixed(w, toks, final)
                out.extend(toks)
            else:
                data = rand_bytes(rng, n)
                dc.put_stored(w, data, final)
                out.extend(data)
        c.add("stored_fixed_stored_A%d" % a, "stored", w.getvalue(), out, want_a=a)


def g_ends(c, rng):
    text = acgt(rng, 500)
    for a in range(4):
        # the last symbol is a match that ends exactly at ISIZE
        toks = dc.tokenize(text + text[100:400], rng, p_match=0.5)
        toks = [t for t in toks]
        while type(toks[-1]) is int:
            toks.pop()
        payload = dc.detok(toks)
        ll, dl = dc.auto_lengths(toks, rng)
        c.add("end_match_ends_at_isize_A%d" % a, "ends", _dyn(toks, ll, dl).getvalue(), payload, want_a=a)
        # the end-of-block code is the last bit of the last byte
        for n_hi in range(8):
            w = Bits()
            toks = list(text[:40]) + [200] * n_hi
            dc.put_fixed(w, toks, 1)
            if w.total % 8 == 0:
                break
        assert w.total % 8 == 0
        c.add("end_eob_is_last_bit_A%d" % a, "ends", w.getvalue(), bytes(toks), want_a=a)
        # bytes after the final block, inside the BGZF data length
        raw = dc.deflate_random(text, rng, 3)
        for extra in (b"\0", b"\xff\xff\xff", bytes(rng.randrange(256) for _ in range(40))):
            c.add("end_trailing_%d_bytes_A%d" % (len(extra), a), "ends", raw + extra, text, want_a=a)


def g_invalid(c, rng):
    """Streams with one thing wrong each: zlib refuses them, and so must both decoders.  (They can only be refused, not crash: every
    store of the decoders is bounded by ISIZE, every load by the stream's length - and none of them is the file's first or last block.)"""
    text = bytes(rng.choice(b"ACGTN\n\t!#IF:,0123456789") for _ in range(1200))
    toks = dc.tokenize(text, rng)
    ll, dl = dc.auto_lengths(toks, full=True)
    ll = dc.huffman_lengths([1 << (15 - l) if l else 1 for l in ll], 15)       # every symbol coded: no trailing run of zeros
    dl = [4] * 2 + [5] * 28
    good = dc.rle_lengths(ll + dl)
    c.add("valid_twin_of_the_invalid_headers", "header", _dyn(toks, ll, dl).getvalue(), text)

    def header_variant(name, syms, hlit=286, hdist=30, **kw):
        w = Bits()
        dc.put_dynamic_header(w, 1, hlit, hdist, syms, **kw)
        dc.put_tokens(w, toks, ll, dl)
        c.add(name, "invalid", w.getvalue(), text, valid=False)
    # code 16 (repeat the previous length) as the first length symbol
    assert good[0][0] < 16
    header_variant("bad_code16_first", [(16, 0, 2)] + good)
    # a run that overruns HLIT + HDIST: the last lengths replaced by a run one too long - a decoder that lets it pass decodes the rest
    assert dl[-4:] == [dl[-1]] * 4
    header_variant("bad_run_overruns_tot", dc.rle_lengths((ll + dl)[:-3]) + [(16, 1, 2)])   # a repeat of 4 where 3 are left
    # HLIT = 287
    header_variant("bad_hlit_287", dc.rle_lengths(ll + [0] + dl), hlit=287)
    # over-subscribed codes
    ll_over = list(ll)
    ll_over[ll.index(max(ll))] = 1
    w = Bits()
    dc.put_dynamic_header(w, 1, 286, 30, dc.rle_lengths(ll_over + dl))
    dc.put_tokens(w, toks, ll, dl)
    c.add("bad_oversubscribed_literal_code", "invalid", w.getvalue(), text, valid=False)
    dl_over = list(dl)
    dl_over[dl.index(max(dl))] = 1
    w = Bits()
    dc.put_dynamic_header(w, 1, 286, 30, dc.rle_lengths(ll + dl_over))
    dc.put_tokens(w, toks, ll, dl)
    c.add("bad_oversubscribed_distance_code", "invalid", w.getvalue(), text, valid=False)
    # no end-of-block code
    ll_noeob = list(ll)
    ll_noeob[256] = 0
    w = Bits()
    dc.put_dynamic_header(w, 1, 286, 30, dc.rle_lengths(ll_noeob + dl))
    dc.put_tokens(w, toks, ll, dl)
    c.add("bad_no_end_of_block_code", "invalid", w.getvalue(), text, valid=False)
    # HCLEN = 4: only zeros can be written, the end-of-block code among them
    w = Bits()
    dc.put_dynamic_header(w, 1, 257, 1, [(18, 127, 7), (18, 120 - 11, 7)], hclen=4, cl_lens=[1 if s in (0, 18) else 0 for s in range(19)])
    w.put(0, 32)
    c.add("bad_hclen4_all_lengths_zero", "invalid", w.getvalue(), text, valid=False)
    # BTYPE 3
    w = Bits()
    dc.put_fixed(w, list(text[:100]), 0)
    w.put(0, 1)
    w.put(3, 2)
    w.put(0, 64)
    c.add("bad_btype_3", "invalid", w.getvalue(), text[:100] + b"x", valid=False)
    # stored: LEN / NLEN mismatch; a length that runs past the input
    for name, kw, cut in (("bad_stored_nlen", dict(nlen_field=(300 ^ 0xffff) ^ 0x0100), 0), ("bad_stored_len_past_input", dict(), 7)):
        w = Bits()
        dc.put_fixed(w, list(text[:50]), 0)
        dc.put_stored(w, text[50:350], 1, **kw)
        raw = w.getvalue()
        c.add(name, "invalid", raw[:len(raw) - cut], text[:350], valid=False)
    # a distance one larger than the output position
    t2 = list(text[:20]) + [(5, 21)] + list(text[25:60])
    l2, d2 = dc.auto_lengths(t2)
    c.add("bad_distance_past_start", "invalid", _dyn(t2, l2, d2).getvalue(), text[:60], valid=False)
    t2 = [(3, 1)] + list(text[:60])
    l2, d2 = dc.auto_lengths(t2)
    c.add("bad_distance_at_position_0", "invalid", _dyn(t2, l2, d2).getvalue(), text[:63], valid=False)
    # the stream makes one byte more / one byte less than ISIZE says (last symbol a literal, and a match)
    raw = dc.deflate_random(text, rng, 2)
    c.add("bad_isize_plus_1", "invalid", raw, text[:-1], valid=False)
    c.add("bad_isize_minus_1", "invalid", raw, text + b"A", valid=False)
    t2 = dc.tokenize(text + text[:300], rng, p_match=0.6)
    while type(t2[-1]) is int or t2[-1][0] < 4:
        t2.pop()
    l2, d2 = dc.auto_lengths(t2)
    p2 = bytes(dc.detok(t2))
    c.add("bad_isize_plus_1_match", "invalid", _dyn(t2, l2, d2).getvalue(), p2[:-1], valid=False)
    c.add("bad_isize_minus_1_match", "invalid", _dyn(t2, l2, d2).getvalue(), p2 + b"A", valid=False)
    # cut inside the last symbol: the fixed end-of-block code is seven zero bits, which zeros behind the input would complete
    for n_hi in range(8):
        w = Bits()
        t2 = list(text[:40]) + [200] * n_hi
        dc.put_fixed(w, t2, 1)
        if w.total % 8 == 4:
            break
    raw = w.getvalue()
    assert w.total % 8 == 4 and raw[-1] == 0
    c.add("bad_truncated_in_end_of_block", "invalid", raw[:-1], bytes(t2), valid=False)
    raw = _dyn(toks, ll, dl).getvalue()
    c.add("bad_truncated_last_byte", "invalid", raw[:-1], text, valid=False)
    c.add("bad_truncated_half", "invalid", raw[:len(raw) // 2], text, valid=False)
    # symbols that have codes but no meaning: literal/length 286 and distance 30 of the fixed code
    for name, tok in (("bad_fixed_symbol_286", [("L", 286)]), ("bad_fixed_symbol_287", [("L", 287)]),
                      ("bad_fixed_distance_30", [("L", 257), ("D", 30)]), ("bad_fixed_distance_31", [("L", 257), ("D", 31)])):
        w = Bits()
        dc.put_fixed(w, list(text[:30]) + tok + list(text[33:60]), 1)
        c.add(name, "invalid", w.getvalue(), text[:60], valid=False)


def libdeflate():
    """libdeflate, if this machine has it (htslib's usual compressor; no dependency: without it the group is absent)."""
    import ctypes
    try:
        lib = ctypes.CDLL("libdeflate.so.0")
    except OSError:
        return None
    lib.libdeflate_alloc_compressor.restype = ctypes.c_void_p
    lib.libdeflate_alloc_compressor.argtypes = [ctypes.c_int]
    lib.libdeflate_deflate_compress.restype = ctypes.c_size_t
    lib.libdeflate_deflate_compress.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    lib.libdeflate_free_compressor.argtypes = [ctypes.c_void_p]
    return lib


def g_libdeflate(c, rng):
    """Optional, and no part of what the corpus must hold: the random-parse payloads of 300 bytes and more as libdeflate writes them."""
    import ctypes
    lib = libdeflate()
    if lib is None:
        return
    for level in (1, 6, 12):
        comp = lib.libdeflate_alloc_compressor(level)
        assert comp
        for name, payload in c.parse_payloads:
            if len(payload) >= 300:
                buf = ctypes.create_string_buffer(dc.BGZF_MAX_RAW)
                n = lib.libdeflate_deflate_compress(comp, payload, len(payload), buf, dc.BGZF_MAX_RAW)
                if n:                                                  # (0: it does not fit a BGZF block)
                    c.add("libdeflate_%d_%s" % (level, name), "libdeflate", buf.raw[:n], payload)
        lib.libdeflate_free_compressor(comp)


GROUPS = (g_random_parse, g_headers, g_deep, g_longest, g_batching, g_stored, g_ends, g_invalid, g_libdeflate)
ALIGNED_GROUPS = ("stored", "ends")                                   # every block of these exists once per alignment A = 0 .. 3


@functools.lru_cache(maxsize=None)
def corpus(seed=20240611):
    """(file bytes, records): one record per BGZF block of the file, in file order - name, group, valid, payload, offset of the
    block, A = residue modulo 4 of its stream's offset in the file.  Pad blocks (group "pad") put the blocks that ask for it at
    their alignment; the invalid blocks come after the first third, so that none is the file's first or last block."""
    c = Corpus()
    for k, g in enumerate(GROUPS):
        g(c, random.Random(seed * 100 + k))
    # every code the writer made fits the device decoder's sub-table budget (csrc/inflate_dev.hip: D_LIT_MAX, D_DIST_MAX), so no valid
    # block can be declined for its tables.  (The over-subscribed codes of the invalid group go through put_dynamic_header alone.)
    assert 0 < dc.MAX_NEED[0] <= 768 and 0 < dc.MAX_NEED[1] <= 256, dc.MAX_NEED
    valid = [e for e in c.entries if e["valid"]]
    invalid = [e for e in c.entries if not e["valid"]]
    third = len(valid) // 3
    order = valid[:third] + invalid + valid[third:]
    rng, parts, recs, off = random.Random(seed), [], [], 0
    for e in order:
        if e["want_a"] is not None:
            blk, payload = dc.pad_block(off, e["want_a"], rng)
            recs.append(dict(name="pad_before_" + e["name"], group="pad", valid=True, payload=payload, offset=off, A=(off + 18) % 4))
            parts.append(blk)
            off += len(blk)
        assert e["want_a"] is None or (off + 18) % 4 == e["want_a"]
        recs.append(dict(name=e["name"], group=e["group"], valid=e["valid"], payload=e["payload"], offset=off, A=(off + 18) % 4))
        parts.append(e["blk"])
        off += len(e["blk"])
    assert recs[0]["valid"] and recs[-1]["valid"] and len({r["name"] for r in recs}) == len(recs)
    return b"".join(parts), recs
