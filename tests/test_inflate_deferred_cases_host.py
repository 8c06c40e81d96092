"""The corpus of tests/test_gpu_inflate_deferred.py, and the proof - on the CPU - that every one of its streams is what it is named for.

csrc/inflate_dev.hip decodes 64 bit offsets per round; a round's batched match copy (lengths sum to at most 64, no match reads what
an earlier one of the round writes) LOADS in its round and STORES in the next one ("pending" in between), fill() loads a 1 KB input
window with one wait, and a lane reads 64 stream bits at once.  The streams here are the smallest at which each of the three can go
wrong.  For every stream: zlib accepts or refuses it as intended (deflate_craft.check, when it is made), and a Python model of the
rounds - `rounds()` below, the round rule restated: a round ends after 64 offsets or at the end of the block; its first round is held
against deflate_corpus.round_view - shows that the situation occurs.  Otherwise the GPU test could pass without meeting the code."""
import collections
import functools
import random

import deflate_craft as dc
from deflate_corpus import round_view, rand_bytes
from deflate_craft import Bits

IN_WIN, WIN_MARGIN = 1024, 32                                          # csrc/inflate_dev.hip
LIT = (65, 67, 71, 84)                                                 # 8-bit literals of the fixed code
HI = (200, 201, 222, 250)                                              # 9-bit ones


# ---- the model -------------------------------------------------------------------------------------------------------------
def rounds(blk):
    """The 64-offset rounds of one Huffman block: a symbol belongs to the round in whose first 64 bits it STARTS; the end-of-block
    code ends the last one.  -> dicts: start (stream bit), syms [(token, start bit, bits, output offset)], eob."""
    out, pos, off, cur = [], blk["bit0"], blk["op0"], None
    for t, b in list(zip(blk["toks"], blk["bits"])) + [("EOB", blk["eob"])]:
        if cur is None or pos - cur["start"] >= 64:
            cur = dict(start=pos, syms=[], eob=False)
            out.append(cur)
        cur["syms"].append((t, pos, b, off))
        if t == "EOB":
            cur["eob"] = True
        else:
            off += 1 if type(t) is int else t[0]
        pos += b
    return out


def view(r):
    """A round's matches by the kernel's own tests: batched = one load / store pair, whose store is deferred to the next round."""
    ms = [(off, t[0], t[1]) for t, _, _, off in r["syms"] if type(t) is tuple]
    first = ms[0][0] if ms else None
    mtot = sum(l for _, l, _ in ms)
    dep = any(o != first and o - d + min(l, d) > first for o, l, d in ms)
    return dict(n=len(ms), mtot=mtot, dep=dep, first=first, batched=bool(ms) and mtot <= 64 and not dep,
                dst=[(o, o + l) for o, l, _ in ms], src=[(o - d, o - d + min(l, d)) for o, l, d in ms],
                lits=[off for t, _, _, off in r["syms"] if type(t) is int], bad=any(d > o for o, _, d in ms),
                total=sum(1 if type(t) is int else t[0] for t, _, _, _ in r["syms"] if t != "EOB"))


def reads(srcs, dsts):
    return any(a < d1 and d0 < b for a, b in srcs for d0, d1 in dsts)


def windows(blk, A, wlo):
    """(round, the input window's first coordinate while it is decoded) - the refill rule of the symbol loop, in coordinates of the
    4-byte aligned buffer (stream byte s sits at s + A)."""
    out = []
    for r in rounds(blk):
        byte0 = (8 * A + r["start"]) >> 3
        if byte0 < wlo or byte0 + WIN_MARGIN > wlo + IN_WIN:
            wlo = byte0 & ~3
        out.append((r, wlo))
    return out


class Stream:
    """A raw DEFLATE stream in the making, with what the model needs of every Huffman block."""

    def __init__(self):
        self.w, self.out, self.blocks, self.stored_at = Bits(), bytearray(), [], []

    def _rec(self, toks, bits, eob, hdr_bit):
        self.blocks.append(dict(toks=list(toks), bits=bits, eob=eob, bit0=self.w.total - sum(bits) - eob, op0=len(self.out), hdr_bit=hdr_bit))
        return self.blocks[-1]

    def stored(self, data, final=0):
        self.stored_at.append(dict(phase=self.w.total % 8, op0=len(self.out), n=len(data)))
        dc.put_stored(self.w, data, final)
        self.out += data
        self.stored_at[-1]["end_byte"] = self.w.total // 8

    def fixed(self, toks, final=0, detok=True):
        b = self.w.total
        blk = self._rec(toks, dc.put_fixed(self.w, toks, final), 7, b)
        if detok:
            dc.detok(toks, self.out)
        return blk

    def dynamic(self, toks, ll, dl, final=0, **kw):
        b = self.w.total
        bits = dc.put_dynamic(self.w, toks, final, ll, dl, **kw)[0]
        blk = self._rec(toks, bits, ll[256], b)
        dc.detok(toks, self.out)
        return blk


# ---- the cases -------------------------------------------------------------------------------------------------------------
class Cases:
    def __init__(self):
        self.entries = []

    def add(self, name, group, raw, payload, facts, valid=True, want_a=None):
        payload = bytes(payload)
        dc.check(raw, payload, valid)
        assert len(payload) > 0, name
        self.entries.append(dict(name=name, group=group, blk=dc.bgzf(raw, payload), payload=payload, valid=valid, want_a=want_a, facts=facts))


def _lits(rng, n, pool=LIT):
    return [rng.choice(pool) for _ in range(n)]


NOISE = 200                                                            # bytes of a stored block in front: something to copy from


def _prefix(rng):
    s = Stream()
    s.stored(rand_bytes(rng, NOISE))
    return s


def _pending_then(s, rng, match_last):
    """Round 0 of a fixed block: one match of 10 bytes from far back - a batch, so its store is pending when round 1 begins - and six
    literals, the match first or last.  -> (tokens, the match's destination, the output position behind the round)."""
    m = (10, 100)
    toks = _lits(rng, 6) + [m] if match_last else [m] + _lits(rng, 6)
    d0 = len(s.out) + (6 if match_last else 0)
    return toks, (d0, d0 + 10), len(s.out) + 16


def g_dependent_rounds(c, rng):
    """A match in round r (pending) and a match in round r + 1 whose source begins at the first byte, ends at the last byte, or
    straddles the end of the pending destination - plain and overlapping itself (distance 1 and 3, length 40)."""
    def case(name, match_last, m2, relation):
        s = _prefix(rng)
        t0, dst, op1 = _pending_then(s, rng, match_last)
        blk = s.fixed(t0 + [m2] + _lits(rng, 12), 1)
        rs = [view(r) for r in rounds(blk)]
        rv = round_view(blk["toks"], blk["bits"], blk["op0"])
        src = (op1 - m2[1], op1 - m2[1] + min(m2))
        facts = dict(round0_is_a_batch=rs[0]["batched"] and rs[0]["dst"] == [dst] and rv["n"] == 1 and not rv["dep"] and rv["mtot"] == 10,
                     round1_starts_with_the_match=rs[1]["dst"][:1] == [(op1, op1 + m2[0])] and rs[1]["src"][:1] == [src],
                     round1_reads_pending=reads(rs[1]["src"], rs[0]["dst"]), relation=relation(src, dst),
                     overlap_as_named=(m2[1] < m2[0]) == ("overlap" in name))
        c.add("dep_rounds_" + name, "dependent", s.w.getvalue(), s.out, facts)
    case("source_begins_at_first_byte", False, (5, 16), lambda s, d: s[0] == d[0])
    case("source_ends_at_last_byte", False, (5, 11), lambda s, d: s[1] == d[1])
    case("source_straddles_the_end", False, (5, 8), lambda s, d: s[0] < d[1] < s[1])
    case("source_is_the_whole_destination", True, (10, 10), lambda s, d: s == d)
    case("source_straddles_the_start", True, (5, 12), lambda s, d: s[0] < d[0] < s[1])
    case("overlap_d1_len40", True, (40, 1), lambda s, d: s == (d[1] - 1, d[1]))
    case("overlap_d3_len40", True, (40, 3), lambda s, d: s == (d[1] - 3, d[1]))
    case("overlap_len40_begins_at_first_byte", False, (40, 16), lambda s, d: s[0] == d[0] and s[1] > d[1])   # (distance 16 < 40: overlapping, across the literals too)
    case("overlap_len40_straddles_the_end", False, (40, 9), lambda s, d: s[0] < d[1] < s[1])


def g_slow_path(c, rng):
    """A pending copy followed by a round that cannot be batched - match lengths that sum to 65 or more; an in-round dependency -
    and reads the bytes the pending copy writes."""
    for name, nxt, want in (("mtot_72", [(18, 10), (18, 100), (18, 101), (18, 102)], dict(mtot=72, dep=False)),
                            ("mtot_65", [(17, 10), (16, 100), (16, 101), (16, 102)], dict(mtot=65, dep=False)),
                            ("in_round_dependency", [(10, 10), (5, 5)], dict(mtot=15, dep=True))):
        s = _prefix(rng)
        t0, dst, op1 = _pending_then(s, rng, True)
        blk = s.fixed(t0 + nxt + _lits(rng, 14), 1)
        rs = [view(r) for r in rounds(blk)]
        facts = dict(round0_is_a_batch=rs[0]["batched"] and rs[0]["dst"] == [dst], round1_is_not=not rs[1]["batched"] and rs[1]["n"] == len(nxt),
                     as_named=all(rs[1][k] == v for k, v in want.items()), round1_reads_pending=reads(rs[1]["src"], rs[0]["dst"]))
        c.add("pending_then_slow_" + name, "slow", s.w.getvalue(), s.out, facts)


def _last_round_pending(s, rng, j, final=0):
    """A fixed block of j 9-bit literals (they move the bit phase), then a fixed block of ONE round: literal, match, end of block."""
    s.fixed(_lits(rng, j, HI) + _lits(rng, 2))
    blk = s.fixed(_lits(rng, 1) + [(10, 100)], final)
    rs = rounds(blk)
    return len(rs) == 1 and rs[0]["eob"] and view(rs[0])["batched"], view(rs[0])["dst"]


def g_block_end(c, rng):
    """The pending copy belongs to the last round of a DEFLATE block; behind it, in the same BGZF block: a stored block (at each bit
    phase) whose bytes a later match reads, a fixed block, a dynamic block with new tables, or nothing."""
    phases = set()
    for j in range(8):
        s = _prefix(rng)
        ok, dst = _last_round_pending(s, rng, j)
        s.stored(rand_bytes(rng, 20))
        phases.add(s.stored_at[-1]["phase"])
        blk = s.fixed([(30, 30)] + _lits(rng, 9), 1)                   # the stored bytes and, before them, the pending copy's
        v = view(rounds(blk)[0])
        st = s.stored_at[-1]
        facts = dict(pending_at_block_end=ok, stored_follows=st["op0"] == dst[0][1],
                     match_reads_stored=reads(v["src"][:1], [(st["op0"], st["op0"] + 20)]), match_reads_pending=reads(v["src"][:1], dst))
        c.add("block_end_then_stored_phase%d" % st["phase"], "block_end", s.w.getvalue(), s.out, facts)
    assert phases == set(range(8)), phases
    s = _prefix(rng)
    ok, dst = _last_round_pending(s, rng, 3)
    v = view(rounds(s.fixed([(10, 10)] + _lits(rng, 9), 1))[0])
    c.add("block_end_then_fixed", "block_end", s.w.getvalue(), s.out, dict(pending_at_block_end=ok, next_reads_pending=v["src"][:1] == dst))
    s = _prefix(rng)
    ok, dst = _last_round_pending(s, rng, 5)
    toks = [(10, 10)] + list(b"new tables, other codes: 0123456789 abcdefghijklmnopqrstuvwxyz") + [(7, 40), (3, 1)]
    ll, dl = dc.auto_lengths(toks)
    v = view(rounds(s.dynamic(toks, ll, dl, 1))[0])
    c.add("block_end_then_dynamic", "block_end", s.w.getvalue(), s.out, dict(pending_at_block_end=ok, next_reads_pending=v["src"][:1] == dst, new_tables=max(ll) > 5))
    for j in (0, 4):                                                   # nothing follows: the epilogue (CRC, copy-out) reads the bytes back
        s = _prefix(rng)
        ok, dst = _last_round_pending(s, rng, j, 1)
        c.add("block_end_then_nothing_%d" % j, "block_end", s.w.getvalue(), s.out, dict(pending_at_block_end=ok, match_is_the_last_bytes=dst[0][1] == len(s.out)))


def g_one_round(c, rng):
    """A BGZF block that is one round: its only match starts at output offset 1 or above and reads the round's own literals."""
    for name, toks in (("offset1_d1", [65, (5, 1)]), ("offset3_d3", [65, 67, 71, (6, 3)]), ("offset2_d1_overlap", [84, 65, (40, 1)]), ("offset4_d2", [65, 67, 71, 84, (9, 2)])):
        s = Stream()
        blk = s.fixed(toks, 1)
        rs = rounds(blk)
        v, rv = view(rs[0]), round_view(blk["toks"], blk["bits"], 0)
        facts = dict(one_round=len(rs) == 1 and rs[0]["eob"], one_match=v["n"] == 1 and v["batched"] and rv["n"] == 1 and rv["lits_before"],
                     starts_at_1_or_above=v["first"] >= 1, reads_this_rounds_literals=all(o in v["lits"] for o in range(*v["src"][0])))
        c.add("one_round_" + name, "one_round", s.w.getvalue(), s.out, facts)


def g_invalid(c, rng):
    """Wrong in the round AFTER a pending copy (round 0: seven literals and a match of three), or cut off while it is pending."""
    head = _lits(rng, 7) + [(3, 2)]                                    # 56 + 12 bits: the next symbol starts round 1; 10 bytes
    claim = bytes(rng.choice(LIT) for _ in range(30))
    # a distance that reaches before the block's first byte
    s = Stream()
    blk = s.fixed(head + [(5, 11)] + _lits(rng, 3), 1, detok=False)
    rs = [view(r) for r in rounds(blk)]
    c.add("bad_distance_after_pending", "invalid", s.w.getvalue(), claim, dict(round0_is_a_batch=rs[0]["batched"], round1_reaches_before_the_start=rs[1]["bad"] and not rs[0]["bad"]), valid=False)
    # more output than ISIZE, in that round
    s = Stream()
    blk = s.fixed(head + [(18, 5)] + _lits(rng, 3), 1)
    rs = [view(r) for r in rounds(blk)]
    for isize in (11, 27):
        facts = dict(round0_is_a_batch=rs[0]["batched"], round0_fits=rs[0]["total"] == 10, round1_overruns=10 + rs[1]["total"] > isize)
        c.add("bad_output_overrun_after_pending_isize%d" % isize, "invalid", s.w.getvalue(), bytes(s.out[:isize]), facts, valid=False)
    # the stream ends where round 1 would begin: zeros behind it read as the fixed code's end of block
    s = Stream()
    blk = s.fixed(head + _lits(rng, 12), 1)
    rs = rounds(blk)
    raw = s.w.getvalue()
    cut = (rs[1]["start"] + 7) // 8
    for name, payload in (("isize_of_round0", s.out[:10]), ("isize_of_the_whole", s.out)):
        facts = dict(round0_is_a_batch=view(rs[0])["batched"], cut_is_behind_round0=rs[1]["start"] <= 8 * cut < rs[1]["start"] + 8, stream_goes_on=cut < len(raw))
        c.add("bad_truncated_while_pending_" + name, "invalid", raw[:cut], payload, facts, valid=False)


def _border_stream(rng, A, target_len, cut=0):
    """A fixed block (rounds of seven literals and a match: a pending copy in every round) whose stream is target_len + cut bytes,
    cut off at target_len."""
    unit = lambda: _lits(rng, 7) + [(10, 20)]
    s = Stream()
    toks = _lits(rng, 24)
    n_units = max(0, (target_len + cut - 40) * 8 // 71 - 1)
    assert n_units >= 4
    for _ in range(n_units - 3):
        toks += unit()
    total = 3 + 8 * 24 + 71 * n_units + 7
    have = (total + 7) // 8
    assert have <= target_len + cut, (have, target_len)
    toks += _lits(rng, target_len + cut - have)                        # (every 8-bit literal is one more byte)
    for _ in range(3):                                                 # ... and matches again up to the end
        toks += unit()
    blk = s.fixed(toks, 1)
    raw = s.w.getvalue()
    assert len(raw) == target_len + cut, (len(raw), target_len, cut)
    return s, blk, raw[:target_len]


def g_window_borders(c, rng):
    """The stream's last byte 0 .. 8 bytes on either side of the first and the second border of the 1 KB input window, at every
    alignment A; valid streams and twins cut off at the same place (behind them the window reads as zero: they must be refused)."""
    for A in range(4):
        # where the second window begins: the first round that no longer has WIN_MARGIN bytes of the first one
        _, blk, _ = _border_stream(rng, A, 3000)
        wl = sorted({w for _, w in windows(blk, A, 0)})
        assert wl[0] == 0 and 992 <= wl[1] <= 1004 and wl[1] % 4 == 0, wl
        for k, border in ((1, IN_WIN), (2, wl[1] + IN_WIN)):
            for delta in list(range(-9, 0)) + list(range(0, 9)):       # last byte at border + delta: -1 = the window's last byte, 0 = the next one's first
                n = border + delta - A + 1                             # stream bytes: the last one at coordinate A + n - 1
                for cut in (0, 6):
                    s, blk, raw = _border_stream(rng, A, n, cut)
                    ws = windows(blk, A, 0)
                    borders = sorted({w + IN_WIN for _, w in ws})
                    facts = dict(last_byte_at=A + len(raw) - 1 == border + delta, border_is_real=border in borders,
                                 pending_near_the_end=view(ws[-1][0])["batched"] or view(ws[-2][0])["batched"], cut_as_named=(len(s.w.getvalue()) - len(raw)) == cut)
                    name = "window%d_A%d_last_byte_%s%d%s" % (k, A, "minus" if delta < 0 else "plus", abs(delta), "_truncated" if cut else "")
                    c.add(name, "window", raw, s.out, facts, valid=not cut, want_a=A)
        # a dynamic header across the first window's border: the fixed block before it ends in the first window's last bytes, past its
        # middle (so the header code moves the window), and the header - every length coded on its own - ends behind coordinate 1024
        s = Stream()
        before = s.fixed(_lits(rng, 968 + 4 * A))
        text = bytes(rng.choice(b"ACGTN\n\t!#IF:,0123456789") for _ in range(400))
        toks = dc.tokenize(text, rng)
        ll, dl = dc.auto_lengths(toks, full=True)
        ll = dc.huffman_lengths([1 << (15 - l) if l else 1 for l in ll], 15)
        dl = dc.huffman_lengths([1 << (15 - l) if l else 1 for l in dl], 15)
        b = s.w.total
        dc.put_dynamic_header(s.w, 1, 286, 30, [(v, 0, 0) for v in ll + dl], cl_skew=True)
        bits = dc.put_tokens(s.w, toks, ll, dl)
        blk = s._rec(toks, bits, ll[256], b)
        dc.detok(toks, s.out)
        h0, h1 = A + b // 8, A + blk["bit0"] // 8
        facts = dict(first_window_still_there=all(w == 0 for _, w in windows(before, A, 0)) and IN_WIN - 512 + 8 < h0 <= IN_WIN - 16,
                     header_ends_behind_the_border=h1 > IN_WIN + 8, header_fits_a_window=h1 - h0 < 500,
                     tables_fit=dc.subtable_need(ll, 9)[0] <= 768 and dc.subtable_need(dl, 8)[0] <= 256)
        c.add("window_dynamic_header_crosses_border_A%d" % A, "window", s.w.getvalue(), s.out, facts, want_a=A)


def _deep_code():
    """tests/deflate_corpus.py g_longest's code: lengths 131 .. 258 and distances from 16385 on have 15-bit codes, four literals short ones."""
    lits = [65, 67, 71, 84]
    deep_l = [281, 282, 283, 284, 285, 277, 278, 279, 280, 270]
    order = lits + [256] + [x for x in range(286) if x not in lits + [256] + deep_l] + deep_l
    ll = [0] * 286
    for x, l in zip(order, dc.fill_lengths(286, 10, 15)):
        ll[x] = l
    dl = dc.fill_lengths(30, 2, 15)
    assert all(ll[x] == 15 for x in deep_l[:5]) and dl[28] == dl[29] == 15 and all(ll[x] <= 4 for x in lits)
    return lits, ll, dl


def g_wide_read(c, rng):
    """Length + distance pairs of 48 bits (15 + 5 and 15 + 13) that start at every bit phase 0 .. 31 of the aligned buffer; and one
    that starts in the last dword in which a lane's code may start before the window is refilled."""
    lits, ll, dl = _deep_code()
    lbits = sorted({ll[x] for x in lits})
    by_bits = {ll[x]: x for x in lits}
    pair = lambda pos: (rng.choice((131, 140, 163, 200, 257)), rng.randint(16385, min(32768, pos)))
    sums = {0: []}                                                     # a sum of literal sizes for every number of bits up to 63
    for tot in range(1, 64):
        sums[tot] = next(sums[tot - b] + [b] for b in reversed(lbits) if tot - b in sums)

    def symbols_begin(s):                                              # the stream bit behind the dynamic header (which the tokens do not change)
        probe = Stream()
        probe.w.total, probe.out = s.w.total, bytearray(s.out)
        return probe.dynamic([65], ll, dl, 1)["bit0"]
    for A in range(4):
        s = Stream()
        s.stored(rand_bytes(rng, 16400 + A))
        first_bit = symbols_begin(s)
        toks, pos, bit = [], len(s.out), 8 * A + first_bit
        for k in range(140):                                           # literals of 1 .. 4 bits put match k at phase 5 k mod 32
            for b in sums[(5 * k - bit) % 32]:
                toks.append(by_bits[b])
                bit += b
                pos += 1
            t = pair(pos)
            toks.append(t)
            bit += 48
            pos += t[0]
        blk = s.dynamic(toks, ll, dl, 1)
        phases = {(8 * A + p) % 32 for t, p, b, _ in (x for r in rounds(blk) for x in r["syms"]) if type(t) is tuple and b == 48}
        n48 = sum(1 for t, b in zip(blk["toks"], blk["bits"]) if type(t) is tuple and b == 48)
        c.add("wide_48bit_every_phase_A%d" % A, "wide", s.w.getvalue(), s.out, dict(all_matches_are_48_bits=n48 == 140, every_phase=phases == set(range(32))), want_a=A)
        # ... and steered: literals until a round starts in the window's last admissible byte, then literals up to its last offsets
        s = Stream()
        s.stored(rand_bytes(rng, 16400 + A))
        wlo = (A + s.stored_at[-1]["end_byte"]) & ~3                   # the stored-block code leaves the window here
        first_bit = symbols_begin(s)
        toks, pos, rstart, out_pos = [], 8 * A + first_bit, 8 * A + first_bit, len(s.out)
        goal_lo = 8 * (wlo + IN_WIN - WIN_MARGIN) + 1                  # a round that starts at bit 1 .. 7 of that byte is not refilled
        def put(t, b):
            nonlocal pos, rstart, out_pos
            if pos - rstart >= 64:
                rstart = pos
            toks.append(t)
            pos += b
            out_pos += 1 if type(t) is int else t[0]
        while pos < goal_lo - 1600:                                  # (literal rounds advance by 64 .. 67 bits: from 22 rounds on every bit is in reach)
            put(pair(out_pos), 48)
            for _ in range(rng.randrange(4)):
                put(by_bits[lbits[0]], lbits[0])
        # breadth-first over literal sizes: reach a symbol boundary at goal_lo .. goal_lo + 6 that begins a round
        seen, queue, found = {(pos, rstart): None}, collections.deque([(pos, rstart)]), None
        while queue and not found:
            p, r = queue.popleft()
            if goal_lo <= p <= goal_lo + 6 and p - r >= 64:
                found = (p, r)
                break
            if p > goal_lo + 6:
                continue
            r2 = p if p - r >= 64 else r
            for b in lbits:
                if (p + b, r2) not in seen:
                    seen[(p + b, r2)] = ((p, r), b)
                    queue.append((p + b, r2))
        assert found, "no path to the window's last admissible round start"
        path, k = [], found
        while seen[k]:
            k, b = seen[k]
            path.append(b)
        for b in reversed(path):
            put(by_bits[b], b)
        round_at = pos
        need = 8 * (wlo + IN_WIN - WIN_MARGIN + 8) - round_at          # offsets up to the dword lane 63 begins in
        assert need <= 63
        for b in sums[need]:
            put(by_bits[b], b)
        assert need <= pos - round_at <= 63
        m_at = pos
        put(pair(out_pos), 48)
        for _ in range(30):
            put(by_bits[lbits[-1]], lbits[-1])
        blk = s.dynamic(toks, ll, dl, 1)
        hit = [(r, w) for r, w in windows(blk, A, wlo) for t, p, b, _ in r["syms"] if type(t) is tuple and b == 48 and 8 * A + p == m_at]
        facts = dict(model_agrees_on_the_start=blk["bit0"] == first_bit and len(hit) == 1,
                     round_is_not_refilled=bool(hit) and hit[0][1] == wlo and ((8 * A + hit[0][0]["start"]) >> 3) == wlo + IN_WIN - WIN_MARGIN,
                     code_starts_in_the_last_dword=bool(hit) and ((m_at >> 5) << 2) - wlo == IN_WIN - WIN_MARGIN + 8,
                     reads_end_inside_the_window=((m_at >> 5) << 2) - wlo + 12 <= IN_WIN,
                     header_leaves_the_window_alone=(first_bit >> 3) - s.stored_at[-1]["end_byte"] < IN_WIN - 512 - 16)
        c.add("wide_48bit_in_the_last_dword_A%d" % A, "wide", s.w.getvalue(), s.out, facts, want_a=A)


GROUPS = (g_dependent_rounds, g_slow_path, g_block_end, g_one_round, g_invalid, g_window_borders, g_wide_read)


@functools.lru_cache(maxsize=None)
def corpus(seed=20250317):
    """(file bytes, records) as tests/deflate_corpus.py corpus() gives them: one record per BGZF block, pad blocks in front of the
    blocks that ask for an alignment; the invalid blocks stand between valid ones, whose bytes must come back intact."""
    c = Cases()
    for k, g in enumerate(GROUPS):
        g(c, random.Random(seed * 100 + k))
    valid = [e for e in c.entries if e["valid"] and e["want_a"] is None]
    aligned = [e for e in c.entries if e["want_a"] is not None]
    invalid = [e for e in c.entries if not e["valid"] and e["want_a"] is None]
    order = []
    for k, e in enumerate(invalid):                                    # valid, invalid, valid, invalid, ...
        order += [valid[k], e]
    order += valid[len(invalid):] + aligned + valid[:1]
    rng, parts, recs, off, seen = random.Random(seed), [], [], 0, {}
    for e in order:
        n = seen.get(e["name"], 0)
        seen[e["name"]] = n + 1
        name = e["name"] if not n else "%s_again%d" % (e["name"], n)
        if e["want_a"] is not None:
            blk, payload = dc.pad_block(off, e["want_a"], rng)
            recs.append(dict(name="pad_before_" + name, group="pad", valid=True, payload=payload, offset=off, A=(off + 18) % 4, facts={}))
            parts.append(blk)
            off += len(blk)
            assert (off + 18) % 4 == e["want_a"]
        recs.append(dict(name=name, group=e["group"], valid=e["valid"], payload=e["payload"], offset=off, A=(off + 18) % 4, facts=e["facts"]))
        parts.append(e["blk"])
        off += len(e["blk"])
    assert recs[0]["valid"] and recs[-1]["valid"] and len({r["name"] for r in recs}) == len(recs)
    return b"".join(parts), recs


# ---- the tests -------------------------------------------------------------------------------------------------------------
def test_every_case_is_what_it_is_named_for():
    _, recs = corpus()
    wrong = {r["name"]: [k for k, v in r["facts"].items() if v is not True] for r in recs}
    wrong = {n: ks for n, ks in wrong.items() if ks}
    assert not wrong, wrong
    assert all(r["facts"] for r in recs if r["group"] != "pad")


def test_the_corpus_holds_every_group_of_the_list():
    _, recs = corpus()
    names = {r["name"] for r in recs}
    count = lambda g: sum(1 for r in recs if r["group"] == g)
    assert count("dependent") >= 9 and count("slow") == 3 and count("block_end") >= 12 and count("one_round") >= 4 and count("invalid") == 5
    assert {"block_end_then_stored_phase%d" % p for p in range(8)} <= names
    for A in range(4):
        for k in (1, 2):
            for d in ["minus%d" % x for x in range(1, 10)] + ["plus%d" % x for x in range(9)]:
                assert {"window%d_A%d_last_byte_%s" % (k, A, d), "window%d_A%d_last_byte_%s_truncated" % (k, A, d)} <= names
        assert {"window_dynamic_header_crosses_border_A%d" % A, "wide_48bit_every_phase_A%d" % A, "wide_48bit_in_the_last_dword_A%d" % A} <= names
    assert all(r["A"] == int(r["name"].split("_A")[1][0]) for r in recs if "_A" in r["name"] and r["group"] != "pad")


def test_zlib_reads_the_file_block_by_block_as_intended():
    """(deflate_craft.check held every stream against zlib when it was made; this is the same through the BGZF framing.)"""
    data, recs = corpus()
    blocks = dc.bgzf_blocks(data)
    assert len(blocks) == len(recs)
    for (off, raw, isize), r in zip(blocks, recs):
        assert off == r["offset"] and isize == len(r["payload"])
        ok, out = dc.zlib_verdict(raw, isize)
        assert ok == r["valid"], r["name"]
        if ok:
            assert out == r["payload"], r["name"]
    assert not recs[0]["group"] == "invalid" and not recs[-1]["group"] == "invalid"
    for i, r in enumerate(recs):                                       # every invalid block has valid neighbours
        if not r["valid"]:
            assert recs[i - 1]["valid"] and recs[i + 1]["valid"], r["name"]
