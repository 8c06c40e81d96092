"""A test-side DEFLATE writer (RFC 1951) for the streams zlib's compressor never emits: any parse of the data (non-longest, far,
length-3 and overlapping matches), dynamic headers written from explicit code lengths with the run-length coding over the combined
literal/length + distance array, HLIT / HDIST / HCLEN above their minimum, codes at any length limit, stored / fixed / dynamic blocks in
any mix, BGZF framing - and streams that are wrong on purpose.  A writer only: the reference for every stream is zlib's inflate, and
`check()` holds every stream against it when it is made, so a bug here fails on the CPU before a decoder under test sees the stream.

Pure Python + numpy, deterministic from the seeds given.  Used by tests/test_inflate_streams_host.py (csrc/inflate_fast.h) and
tests/test_gpu_inflate_streams.py (csrc/inflate_dev.hip)."""
import bisect
import heapq
import random
import struct
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_SYM = [0] * 259                                                   # match length -> index into LEN_BASE
for _l in range(3, 259):
    LEN_SYM[_l] = bisect.bisect_right(LEN_BASE, _l) - 1
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
BGZF_MAX_RAW = 65536 - 26                                             # the largest DEFLATE stream a BGZF block holds


# ---- bits ----------------------------------------------------------------------------------------------------------------
class Bits:
    """Values of up to 16 bits, least significant bit first; packed by numpy in one go."""

    def __init__(self):
        self.v, self.n, self.total = [], [], 0

    def put(self, v, n):
        if n:
            self.v.append(v)
            self.n.append(n)
            self.total += n

    def align(self):
        self.put(0, -self.total & 7)

    def raw(self, data):
        assert self.total % 8 == 0
        self.v.extend(data)
        self.n.extend([8] * len(data))
        self.total += 8 * len(data)

    def getvalue(self):
        if not self.v:
            return b""
        v, n = np.asarray(self.v, dtype=np.uint32), np.asarray(self.n, dtype=np.int64)
        start = np.cumsum(n) - n
        k = np.arange(self.total, dtype=np.int64) - np.repeat(start, n)
        return np.packbits(((np.repeat(v, n) >> k.astype(np.uint32)) & 1).astype(np.uint8), bitorder="little").tobytes()


# ---- codes ---------------------------------------------------------------------------------------------------------------
def _rev(c, l):
    return int(format(c, "0%db" % l)[::-1], 2) if l else 0


def canonical(lens):
    """The canonical code of every symbol, bit-reversed (so that Bits.put sends its first bit first).  Lengths that over-subscribe
    the code space (the streams that are wrong on purpose) get codes cut to their length."""
    cnt = [0] * 17
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, c = [0] * 17, 0
    for l in range(1, 16):
        c = (c + cnt[l - 1]) << 1
        nxt[l] = c
    out = []
    for l in lens:
        if l:
            out.append(_rev(nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
        else:
            out.append(0)
    return out


def kraft(lens):
    """Code space used, in units of 2^-15: 32768 = complete."""
    return sum(1 << (15 - l) for l in lens if l)


def huffman_lengths(freqs, limit=15):
    """Huffman code lengths for the symbols with freq > 0, none longer than `limit`; complete whenever two or more symbols are used
    (one symbol alone gets the 1-bit code zlib permits)."""
    n = len(freqs)
    used = [i for i in range(n) if freqs[i] > 0]
    lens = [0] * n
    if len(used) < 2:
        for i in used:
            lens[i] = 1
        return lens
    assert len(used) <= 1 << limit
    heap = [(freqs[s], k) for k, s in enumerate(used)]
    heapq.heapify(heap)
    parent, nid = {}, len(used)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        parent[a[1]] = parent[b[1]] = nid
        heapq.heappush(heap, (a[0] + b[0], nid))
        nid += 1
    depth = {nid - 1: 0}
    for k in range(nid - 2, -1, -1):
        depth[k] = depth[parent[k]] + 1
    cnt = [0] * (limit + 1)
    for k in range(len(used)):
        cnt[min(depth[k], limit)] += 1
    total = sum(cnt[l] << (limit - l) for l in range(1, limit + 1))
    while total != 1 << limit:                                        # over-subscribed by the cut: lengthen a code, one unit at a time
        cnt[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if cnt[l]:
                cnt[l] -= 1
                cnt[l + 1] += 2
                break
        total -= 1
    order = sorted(range(len(used)), key=lambda k: (depth[k], -freqs[used[k]]))
    l = 1
    for k in order:
        while not cnt[l]:
            l += 1
        cnt[l] -= 1
        lens[used[k]] = l
    return lens


def fill_lengths(n_sym, n_deep, maxlen=15, rng=None):
    """The lengths (ascending) of a complete code of `n_sym` symbols of which exactly `n_deep` (even) are `maxlen` bits long: the
    rest of the code space is written in binary and codes are split until the count is right - the longest first, or at random."""
    assert n_deep % 2 == 0 and 0 < n_deep < n_sym
    rest, m = (1 << maxlen) - n_deep, n_sym - n_deep
    items = [maxlen - k for k in range(maxlen + 1) if (rest >> k) & 1]
    assert len(items) <= m, "too few symbols for %d codes of %d bits" % (n_deep, maxlen)
    while len(items) < m:
        cand = [i for i, l in enumerate(items) if l < maxlen - 1]
        assert cand, "cannot place %d symbols" % n_sym
        i = rng.choice(cand) if rng else max(cand, key=lambda i: items[i])
        l = items.pop(i)
        items += [l + 1, l + 1]
    out = sorted(items) + [maxlen] * n_deep
    assert kraft(out) == 32768
    return out


def subtable_need(lens, root):
    """Second-level table entries a decoder with a `root`-bit first level needs, by the rule of csrc/inflate_dev.hip (build_table):
    every first-level prefix that carries longer codes gets a sub-table of 2^(its longest code - root) entries."""
    need = {}
    for l, c in zip(lens, canonical(lens)):
        if l > root:
            p = c & ((1 << root) - 1)
            need[p] = max(need.get(p, 0), l - root)
    return sum(1 << b for b in need.values()), len(need)


# ---- tokens --------------------------------------------------------------------------------------------------------------
# A token is a literal (int 0..255), a match (length, distance), or raw material for the streams that are wrong on purpose:
# ("L", symbol) a literal/length code alone, ("D", symbol) a distance code alone, ("X", value, bits) plain bits.
def detok(tokens, out=None):
    out = bytearray() if out is None else out
    for t in tokens:
        if type(t) is int:
            out.append(t)
        elif t[0] not in ("L", "D", "X"):
            l, d = t
            assert 1 <= d <= len(out), (t, len(out))
            if d >= l:
                out += out[len(out) - d:len(out) - d + l]
            else:
                seg = bytes(out[len(out) - d:])
                out += (seg * (l // d + 1))[:l]
    return out


POLICY = dict(p_match=0.85, p_longest=0.3, p_len3=0.15, p_near=0.3, min_dist=1, max_dist=32768, max_len=258)


def tokenize(data, rng, **kw):
    """A random parse: at every position, with p_match, one of the earlier occurrences of the next three bytes (the nearest with
    p_near, else any inside the window - far ones included) and a length between 3 and what matches there (the longest with
    p_longest, 3 with p_len3, else any) - so non-longest, far, length-3-at-any-distance and overlapping matches all occur."""
    p = dict(POLICY, **kw)
    n = len(data)
    if n < 4:
        return list(data)
    d = np.frombuffer(data, dtype=np.uint8).astype(np.int64)
    keys = ((d[:-2] << 16) | (d[1:-1] << 8) | d[2:]).tolist()
    table, toks, i, rnd = {}, [], 0, rng.random
    p_match, p_near, p_longest, p_len3, min_d, max_d, max_l = (p[k] for k in ("p_match", "p_near", "p_longest", "p_len3", "min_dist", "max_dist", "max_len"))
    while i < n:
        l = 0
        if i + 3 <= n:
            lst = table.get(keys[i])
            if lst and rnd() < p_match:
                j = lst[-1] if rnd() < p_near else lst[int(rnd() * len(lst))]
                if i - j > max_d:
                    j = lst[-1]
                if min_d <= i - j <= max_d:
                    lim = min(max_l, n - i)
                    l = 3
                    while l < lim and data[j + l] == data[i + l]:
                        l += 1
                    r = rnd()
                    if r >= p_longest and l > 3:
                        l = 3 if r < p_longest + p_len3 else 3 + int(rnd() * (l - 2))
                    toks.append((l, i - j))
        if not l:
            toks.append(data[i])
            l = 1
        for k in range(i, min(i + min(l, 16), n - 2)):                # (the first positions of a long match are enough to find it again)
            table.setdefault(keys[k], []).append(k)
        i += l
    return toks


def token_lengths(tokens):
    """Output bytes per token."""
    return [1 if type(t) is int else (t[0] if t[0] not in ("L", "D", "X") else 0) for t in tokens]


def frequencies(tokens, l258_alt=False):
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in tokens:
        if type(t) is int:
            lf[t] += 1
        elif t[0] == "L":
            lf[min(t[1], 285)] += 1
        elif t[0] == "D":
            df[min(t[1], 29)] += 1
        elif t[0] != "X":
            lf[257 + (27 if l258_alt and t[0] == 258 else LEN_SYM[t[0]])] += 1
            df[bisect.bisect_right(DIST_BASE, t[1]) - 1] += 1
    return lf, df


# ---- block writers -------------------------------------------------------------------------------------------------------
def put_stored(w, data, final, len_field=None, nlen_field=None):
    w.put(final, 1)
    w.put(0, 2)
    w.align()
    l = len(data) if len_field is None else len_field
    w.put(l, 16)
    w.put(l ^ 0xffff if nlen_field is None else nlen_field, 16)
    w.raw(data)


def put_tokens(w, tokens, litlens, distlens, l258_alt=False, eob=True):
    """The tokens and the end-of-block code; returns the bits every token took.  l258_alt: length 258 goes as code 284 + 31."""
    lc, dc, bits = canonical(litlens), canonical(distlens), []
    put = w.put
    for t in tokens:
        b0 = w.total
        if type(t) is int:
            assert litlens[t], "literal %d has no code" % t
            put(lc[t], litlens[t])
        elif t[0] == "L":
            put(lc[t[1]], litlens[t[1]])
        elif t[0] == "D":
            put(dc[t[1]], distlens[t[1]])
        elif t[0] == "X":
            put(t[1], t[2])
        else:
            l, d = t
            ls = 27 if l258_alt and l == 258 else LEN_SYM[l]
            ds = bisect.bisect_right(DIST_BASE, d) - 1
            assert litlens[257 + ls] and distlens[ds], ("no code for", t)
            put(lc[257 + ls], litlens[257 + ls])
            put(l - LEN_BASE[ls], LEN_EXTRA[ls])
            put(dc[ds], distlens[ds])
            put(d - DIST_BASE[ds], DIST_EXTRA[ds])
        bits.append(w.total - b0)
    if eob:
        put(lc[256], litlens[256])
    return bits


def put_fixed(w, tokens, final, **kw):
    w.put(final, 1)
    w.put(1, 2)
    return put_tokens(w, tokens, FIXED_LIT, FIXED_DIST, **kw)


def rle_lengths(arr, rng=None):
    """The run-length coding of a code-length array as (symbol, extra value, extra bits).  Greedy, or with `rng` a random choice of
    where runs are cut and whether they are used at all.  The array is the combined one, so runs cross the HLIT/HDIST border."""
    out, i, n = [], 0, len(arr)
    while i < n:
        v, j = arr[i], i
        while j < n and arr[j] == v:
            j += 1
        run = j - i
        if rng and rng.random() < 0.2:
            run = 1 + int(rng.random() * run)
        if v == 0 and run >= 3:
            r = min(run, 138)
            if rng and rng.random() < 0.5:
                r = 3 + int(rng.random() * (r - 2))
            out.append((17, r - 3, 3) if r <= 10 else (18, r - 11, 7))
            i += r
        elif v and run >= 4:
            out.append((v, 0, 0))
            r = min(run - 1, 6)
            if rng and rng.random() < 0.5:
                r = 3 + int(rng.random() * (r - 2))
            out.append((16, r - 3, 2))
            i += 1 + r
        elif i and arr[i - 1] == v and run >= 3 and v:                # a run that goes on after a cut
            r = min(run, 6)
            out.append((16, r - 3, 2))
            i += r
        else:
            out.append((v, 0, 0))
            i += 1
    return out


def put_dynamic_header(w, final, hlit, hdist, cl_syms, hclen=None, cl_skew=False, cl_lens=None):
    """BFINAL, BTYPE 2, HLIT, HDIST, HCLEN, the code-length code and `cl_syms` (what rle_lengths returns, or any list of the kind)."""
    if cl_lens is None:
        f = [0] * 19
        for s, _, _ in cl_syms:
            f[s] += 1
        if cl_skew:                                                    # a code-length code as deep as it gets: weights that fall by halves
            for r, s in enumerate(sorted((s for s in range(19) if f[s]), key=lambda s: -f[s])):
                f[s] = 1 << max(0, 12 - 2 * r)
        if sum(1 for x in f if x) == 1:                                # (zlib wants the code-length code complete)
            f[[s for s in (0, 1) if not f[s]][0]] = 1
        cl_lens = huffman_lengths(f, 7)
    need = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
    hclen = need if hclen is None else hclen
    assert 4 <= hclen <= 19
    w.put(final, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_lens[CL_ORDER[k]], 3)
    cc = canonical(cl_lens)
    for s, x, nb in cl_syms:
        w.put(cc[s], cl_lens[s])
        w.put(x, nb)
    return cl_lens


MAX_NEED = [0, 0]                                                     # the largest sub-table need put_dynamic has seen: literal (9-bit root), distance (8-bit)


def put_dynamic(w, tokens, final, litlens, distlens, rng=None, hclen=None, cl_skew=False, **kw):
    """A dynamic block from explicit length arrays (len(litlens) = HLIT, len(distlens) = HDIST)."""
    assert 257 <= len(litlens) and 1 <= len(distlens)
    for k, (lens, root) in enumerate(((litlens, 9), (distlens, 8))):
        if max(lens) > root:
            MAX_NEED[k] = max(MAX_NEED[k], subtable_need(lens, root)[0])
    cl = put_dynamic_header(w, final, len(litlens), len(distlens), rle_lengths(list(litlens) + list(distlens), rng), hclen, cl_skew)
    return put_tokens(w, tokens, litlens, distlens, **kw), cl


def trim(lens, minimum):
    n = len(lens)
    while n > minimum and lens[n - 1] == 0:
        n -= 1
    return lens[:n]


def auto_lengths(tokens, rng=None, limit_l=15, limit_d=15, l258_alt=False, full=False):
    """Code lengths for the tokens.  With `rng` the frequencies are scaled at random (codes far from optimal, deeper than zlib makes
    them) and some unused symbols get codes; full: HLIT = 286 and HDIST = 30 whatever is used."""
    lf, df = frequencies(tokens, l258_alt)
    if rng:
        for f in (lf, df):
            for s in range(len(f)):
                if f[s]:
                    f[s] *= rng.choice((1, 1, 1, 4, 30, 500))
                elif rng.random() < 0.05:
                    f[s] = 1
    used_l, used_d = sum(1 for x in lf if x), sum(1 for x in df if x)
    ll, dl = huffman_lengths(lf, max(limit_l, (used_l - 1).bit_length())), huffman_lengths(df, max(limit_d, (used_d - 1).bit_length()))
    return (ll, dl) if full else (trim(ll, 257), trim(dl, 1))


def deflate_random(payload, rng, n_blocks=1, tight=False, **policy):
    """`payload` as a raw DEFLATE stream of `n_blocks` DEFLATE blocks: one random parse (matches reach across the block borders),
    cut at random tokens; every piece is a stored, a fixed or a dynamic block with a length limit drawn from 7 .. 15 and frequencies
    scaled at random.  tight: dynamic blocks with the true frequencies only (for data that would not fit a BGZF block otherwise)."""
    toks = tokenize(payload, rng, **policy)
    cuts = sorted(int(rng.random() * (len(toks) + 1)) for _ in range(n_blocks - 1))
    w, at, pos = Bits(), 0, 0
    for k, c in enumerate(cuts + [len(toks)]):
        seg, final = toks[at:c], k == n_blocks - 1
        nbytes = sum(token_lengths(seg))
        kind = rng.random()
        if kind < 0.2 and not tight and nbytes < 65536:
            put_stored(w, payload[pos:pos + nbytes], final)
        elif kind < 0.4 and not tight:
            put_fixed(w, seg, final)
        else:
            lf, df = frequencies(seg)
            n_l, n_d = sum(1 for x in lf if x), sum(1 for x in df if x)
            lo_l, lo_d = max(7, (n_l + 15).bit_length()), max(7, (n_d + 2).bit_length())   # (room for the unused symbols auto_lengths adds)
            ll, dl = auto_lengths(seg, None if tight else rng, rng.randint(min(lo_l, 15), 15), rng.randint(min(lo_d, 15), 15), full=rng.random() < 0.1)
            put_dynamic(w, seg, final, ll, dl, rng if rng.random() < 0.5 else None, hclen=19 if rng.random() < 0.1 else None)
        at, pos = c, pos + nbytes
    assert pos == len(payload)
    return w.getvalue()


def deflate_random_fit(payload, rng, n_blocks=1, **policy):
    """deflate_random, tried again with fewer stored blocks / DEFLATE blocks until the stream fits a BGZF block."""
    for attempt in range(6):
        raw = deflate_random(payload, rng, max(1, n_blocks >> max(0, attempt - 2)), tight=attempt >= 2, **policy)
        if len(raw) <= BGZF_MAX_RAW:
            return raw
    raise AssertionError("payload of %d bytes does not fit a BGZF block" % len(payload))


# ---- checking and framing ------------------------------------------------------------------------------------------------
def zlib_verdict(raw, isize):
    """zlib's inflate of a raw stream, as the harnesses ask it: True = it ends inside the input with exactly isize bytes."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw, isize + 1)
    except zlib.error:
        return False, None
    return d.eof and len(out) == isize, out


def check(raw, payload, valid):
    ok, out = zlib_verdict(raw, len(payload))
    if valid:
        assert ok and out == payload, "the writer made a stream zlib does not read back"
    else:
        assert not ok, "zlib accepts a stream that was meant to be wrong"
    return raw, payload, valid


def bgzf(raw, payload):
    """One BGZF block; CRC and ISIZE are those of `payload` (for a stream that is wrong on purpose: what the footer claims)."""
    assert len(raw) <= BGZF_MAX_RAW, len(raw)
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(raw) + 25) + raw
            + struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def pad_block(offset, a, rng):
    """A BGZF block of one stored DEFLATE block with 1 .. 4 payload bytes, after which (at file offset `offset`) the next block's
    DEFLATE stream starts at an address with residue `a` modulo 4."""
    k = 1 + (a - (offset + 31 + 1 + 18)) % 4
    payload = bytes(rng.randrange(256) for _ in range(k))
    w = Bits()
    put_stored(w, payload, 1)
    blk = bgzf(w.getvalue(), payload)
    assert (offset + len(blk) + 18) % 4 == a
    return blk, payload


def bgzf_blocks(data):
    """(offset, raw stream, isize) of every BGZF block of a file."""
    out, o = [], 0
    while o + 18 <= len(data):
        bs = struct.unpack_from("<H", data, o + 16)[0] + 1
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        out.append((o, data[o + 12 + xlen:o + bs - 8], struct.unpack_from("<I", data, o + bs - 4)[0]))
        o += bs
    assert o == len(data)
    return out


def redeflate_bgzf(data, rng):
    """A BGZF file block by block through zlib's inflate and deflate_random: the same payload boundaries (virtual offsets stay
    valid), other streams - 1 .. 6 DEFLATE blocks of mixed type per BGZF block."""
    out = []
    for _, raw, isize in bgzf_blocks(data):
        payload = zlib.decompress(raw, -15)
        assert len(payload) == isize
        new = deflate_random_fit(payload, rng, rng.randint(1, 6)) if isize else raw
        check(new, payload, True)
        out.append(bgzf(new, payload))
    return b"".join(out)
