"""The inputs and the two statements of the base-quality rule that tests/test_gpu_min_baseq.py compares the engine with
(tests/baseq_cases.py), held against the pinned oracle on the CPU: at Q = 0 the wrapped model is the oracle on every case; under the
case's Q the model with the masked lookup (E1) equals the UNCHANGED oracle on the reads whose masked bases were turned into one-base
deletions (E2); and every case has a masked pair that changes a matrix, which is what makes the GPU tests fail where the floor is not
applied.  Also the configuration checks that need no device: struct sizes, the XCK_E_ARG table, the knob parser, header and symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import baseq_cases as B
import oracle as O
import umi_consensus_model as UM
import util
from xcltk_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATS = ("ad", "dp", "oth")


def _oracle(c, batches):
    f = dict(B.FILT); f.update(c.filt)
    cfg, keep = O.make_config(capi.XCK_MODE_BAF, c.names, c.regions, c.snps, c.n_cells, flags=c.flags, **f)
    return O.run_oracle(cfg, [util.batch_from_dict(d)[0] for d in batches])


def _mats(m):
    return m if isinstance(m, dict) else {k: getattr(m, k) for k in MATS}


def _same(a, b):
    a, b = _mats(a), _mats(b)
    return all(np.array_equal(a[k][j], b[k][j]) for k in MATS for j in range(3))


@pytest.mark.parametrize("name", B.CASES)
def test_without_a_floor_the_model_is_the_oracle(name):
    c = B.case(name)
    m = B.model(c, 0)
    assert _same(m, _oracle(c, c.batches))
    assert m.stats["pairs_masked"] == 0 and _same(m, UM.model(c.names, c.regions, c.snps, c.batches, c.filt, "first"))


@pytest.mark.parametrize("name", B.CASES)                          # (every case: none is left out of the E2 comparison)
def test_masked_lookup_equals_the_oracle_on_the_rewritten_reads(name):
    c = B.case(name)
    rw = B.rewritten(c, c.q)
    m = B.model(c, c.q)
    assert _same(m, _oracle(c, rw)), "E1 and E2 disagree under the default rule"
    assert _same(B.model(c, c.q, "consensus"), UM.model(c.names, c.regions, c.snps, rw, c.filt, "consensus")), "E1 and E2 disagree under consensus"
    # the rewrite moved no read across min_len, and it holds the same accepted pairs: only allele codes change
    f = dict(B.FILT); f.update(c.filt)
    for d0, d1 in zip(c.batches, rw):
        assert [r.ok for r in B.JT._read_summary(d0, f)] == [r.ok for r in B.JT._read_summary(d1, f)]
    assert UM.molecules(c.names, c.snps, rw, c.filt)[1] == m.pairs == B.model(c, 0).pairs


@pytest.mark.parametrize("name", B.CASES)
def test_every_case_has_a_masked_pair_that_changes_a_matrix(name):
    c = B.case(name)
    m0, m = B.model(c, 0), B.model(c, c.q)
    print(name, c.q, m.stats, "nnz", [len(getattr(m, k)[0]) for k in MATS], "kept", m0.kept.tolist(), "->", m.kept.tolist())
    assert m.stats["pairs_masked"] >= 1 and m.stats["pairs_with_base"] == m0.stats["pairs_with_base"]
    assert not _same(m0, m), "no matrix differs between Q = 0 and Q = %d" % c.q
    assert not np.array_equal(m0.tally, m.tally)
    assert sum(len(getattr(m, k)[0]) for k in MATS) > 0
    assert sum(len(g) for g in c.reads) <= 40 and len(c.snps) <= 6 and c.n_cells == 3


def test_what_the_cases_cover():
    f = lambda name: B.case(name)
    # lengths 1, 2, odd, even; the SNP at qi = 0, L - 1 and both parities
    seen = set()
    for r in f("lengths").reads[0]:
        L, qi = len(r["seq"]), 1000 - r["pos"]
        seen.add((L, qi))
    assert {(1, 0), (2, 0), (2, 1), (5, 0), (5, 4), (5, 2), (5, 3), (6, 0), (6, 5), (6, 2), (6, 3)} <= seen
    # soft clip / insertion: the query offset differs from the reference offset
    c = f("offsets"); fl = dict(B.FILT)
    assert any(B.query_offset(r, 2000) not in (None, 2000 - r.pos) for r in B.JT._read_summary(c.batches[0], fl))
    # both walks in one tile, masked on both
    c = f("paths"); rs = B.JT._read_summary(c.batches[0], fl)
    at = {(bi, i) for bi, i, _ in B.model(c, c.q).masked_at}
    assert any(rs[i].simple for _, i in at) and any(not rs[i].simple for _, i in at)
    # `*` qualities, l_seq = 0, the pad byte
    c = f("stored")
    assert any(r["qual"] is None and r["seq"] for r in c.reads[0]) and any(r["seq"] == "" for r in c.reads[0])
    assert any(len(r["seq"]) & 1 and sum(l for _, l in r["cig"]) == len(r["seq"]) + 1 for r in c.reads[0])
    assert int(B.model(c, c.q).tally[0][4]) == 1                     # the pad nibble, shown: under N
    # the molecule rules part where a masked read comes first
    c = f("umi")
    assert not _same(B.model(c, c.q), B.model(c, c.q, "consensus"))
    # the filters flip at their ties
    assert B.model(f("min_count"), 0).kept.tolist() == [1, 1] and B.model(f("min_count"), 13).kept.tolist() == [0, 1]
    assert B.model(f("min_maf"), 0).kept.tolist() == [1, 0] and B.model(f("min_maf"), 13).kept.tolist() == [1, 1]
    # the second contig's batch is a window: its offsets do not start at 0
    c = f("contigs")
    assert int(c.batches[1]["seq_off"][0]) > 0 and int(c.batches[1]["cig_off"][0]) > 0 and int(c.batches[0]["seq_off"][0]) == 0
    # Q in {1, 13, 93}, 128-bit keys, the replay knobs
    assert {B.case(n).q for n in B.CASES} == {1, 13, 93} and any(B.case(n).flags & capi.XCK_F_FORCE_KEY128 for n in B.CASES)
    assert B.case("replay").env == {"XCK_HIT_CAP0": "64", "XCK_HIT_SLACK": "0"} and B.model(B.case("replay"), 13).pairs == 240


def test_written_bam_holds_the_case(tmp_path):
    """write_bam / record_quals / qual_column: the qualities of the written file, read back, are the case's columns"""
    import pybam
    for name in ("stored", "contigs", "lengths"):
        c = B.case(name)
        fn = str(tmp_path / (name + ".bam"))
        n = B.write_bam(c, fn)
        refs, recs = pybam.read_bam(fn)
        quals = B.record_quals(fn)
        assert n == len(recs) == len(quals) == sum(len(g) for g in c.reads)
        at = 0
        for bi, d in enumerate(c.batches):
            k = len(d["pos"])
            col = B.qual_column(quals[at:at + k], d["seq_off"])
            assert np.array_equal(col, c.quals[bi]), (name, bi)
            assert [r.pos for r in recs[at:at + k]] == d["pos"].tolist()
            at += k


# ----------------------------------------------------------------------------- configuration, no device
def _create(lib, size=None, mode=capi.XCK_MODE_BAF, flags=capi.XCK_F_DECODE_ONLY, min_baseq=0):
    cfg = capi.Config()
    cfg.struct_size = C.sizeof(capi.Config) if size is None else size
    cfg.mode, cfg.n_cells, cfg.flags, cfg.min_baseq = mode, 1, flags, min_baseq
    h = C.c_void_p()
    rc = lib.xck_create(C.byref(cfg), C.byref(h))
    err = lib.xck_last_error(None).decode() if rc else ""
    if rc == 0:
        lib.xck_destroy(h)
    return rc, err


@pytest.fixture
def lib(monkeypatch):
    monkeypatch.delenv("XCK_MIN_BASEQ", raising=False)
    return capi.load()


def test_struct_sizes(lib):
    """min_baseq fills what was the tail padding of xck_config: the size is what it was, sizeof - 4 (where the field begins) is refused
    as before, and the field's bytes are read only under XCK_F_MIN_BASEQ - an old caller's padding may hold anything"""
    assert C.sizeof(capi.Config) == 176 and capi.Config.MIN_BASEQ_OFFSET == 172 == capi.Config.filter_value.offset + 4
    assert capi.XCK_F_MIN_BASEQ == 512
    assert _create(lib)[0] == 0
    for size in (172, 180, 184, 0):
        rc, err = _create(lib, size=size)
        assert rc == capi.XCK_E_ARG and "struct_size" in err, size
    # the property sets the bit with the value and clears it with 0
    cfg = capi.Config(); cfg.flags = capi.XCK_F_DECODE_ONLY
    cfg.min_baseq = 13
    assert cfg.min_baseq == 13 and cfg.flags == capi.XCK_F_DECODE_ONLY | capi.XCK_F_MIN_BASEQ and bytes(cfg)[172:176] == b"\x0d\0\0\0"
    cfg.min_baseq = 0
    assert cfg.flags == capi.XCK_F_DECODE_ONLY
    # garbage in the padding of a caller that does not know the field: not read (with the bit, 0x7f7f7f7f is XCK_E_ARG; so is 13 on this decode-only handle)
    for junk in (0x7f7f7f7f, 13, -1):
        cfg = capi.Config(); cfg.struct_size = 176; cfg.mode, cfg.n_cells, cfg.flags = capi.XCK_MODE_BAF, 1, capi.XCK_F_DECODE_ONLY
        C.c_int32.from_buffer(cfg, 172).value = junk
        h = C.c_void_p()
        assert lib.xck_create(C.byref(cfg), C.byref(h)) == 0, junk
        lib.xck_destroy(h)
        cfg.flags |= capi.XCK_F_MIN_BASEQ
        assert lib.xck_create(C.byref(cfg), C.byref(h)) == capi.XCK_E_ARG, junk
    # a shorter struct cannot carry the field: the bit on it is refused, not ignored; without the bit it is accepted as ever
    for size in (capi.Config.filter_tag.offset, capi.Config.n_excl_pairs.offset):
        cfg = capi.Config(); cfg.struct_size = size; cfg.mode, cfg.n_cells = capi.XCK_MODE_BAF, 1
        cfg.flags = capi.XCK_F_DECODE_ONLY | capi.XCK_F_MIN_BASEQ
        h = C.c_void_p()
        assert lib.xck_create(C.byref(cfg), C.byref(h)) == capi.XCK_E_ARG and b"XCK_F_MIN_BASEQ" in lib.xck_last_error(None), size
        cfg.flags = capi.XCK_F_DECODE_ONLY
        assert lib.xck_create(C.byref(cfg), C.byref(h)) == 0, size
        lib.xck_destroy(h)
    # with the bit, the XCK_E_ARG table holds on the field: 0 and 1 .. 93 pass the range check (93 then fails as any floor does on this
    # decode-only handle), 94 and negatives do not
    for q, text in ((0, None), (93, "XCK_F_DECODE_ONLY"), (94, "outside 0 .. 93"), (-5, "outside 0 .. 93")):
        cfg = capi.Config(); cfg.struct_size = 176; cfg.mode, cfg.n_cells = capi.XCK_MODE_BAF, 1
        cfg.flags = capi.XCK_F_DECODE_ONLY | capi.XCK_F_MIN_BASEQ
        C.c_int32.from_buffer(cfg, 172).value = q
        h = C.c_void_p()
        rc = lib.xck_create(C.byref(cfg), C.byref(h))
        assert (rc == 0) if text is None else (rc == capi.XCK_E_ARG and text.encode() in lib.xck_last_error(None)), q
        if rc == 0:
            lib.xck_destroy(h)


def test_create_refuses(lib):
    for kw, text in ((dict(min_baseq=94, flags=0), "outside 0 .. 93"), (dict(min_baseq=-1, flags=0), "outside 0 .. 93"),
                     (dict(min_baseq=13, mode=capi.XCK_MODE_BASEFC, flags=0), "no BAF pipeline"),
                     (dict(min_baseq=13), "XCK_F_DECODE_ONLY"), (dict(min_baseq=13, mode=capi.XCK_MODE_BOTH), "XCK_F_DECODE_ONLY")):
        rc, err = _create(lib, **kw)
        assert rc == capi.XCK_E_ARG and text in err, (kw, err)


@pytest.mark.parametrize("text,ok", [("13", True), ("0", True), ("93", True), ("1", True), ("94", False), ("abc", False), ("-1", False), (" 13", False),
                                     ("13 ", False), ("1e1", False), ("0x0d", False), ("1000", False)])
def test_knob_parser(text, ok, monkeypatch):
    monkeypatch.setenv("XCK_MIN_BASEQ", text)
    lib = capi.load()
    # decode-only and basefc-only handles ignore a well-formed knob; a malformed one fails every create and is quoted
    for kw in (dict(), dict(mode=capi.XCK_MODE_BASEFC)):
        rc, err = _create(lib, **kw)
        if ok:
            assert rc == 0, err
        else:
            assert rc == capi.XCK_E_ARG and "XCK_MIN_BASEQ" in err and '"%s"' % text in err, err


def test_header_struct_and_symbols():
    with open(os.path.join(ROOT, "include", "xck.h")) as fp:
        h = fp.read()
    body = re.search(r"typedef struct xck_baseq_stats \{(.*?)\} xck_baseq_stats;", h, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|int32_t|int64_t)\s+(\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in capi.BaseqStats._fields_] and C.sizeof(capi.BaseqStats) == 24
    body = re.search(r"typedef struct xck_config \{(.*?)\} xck_config;", h, re.S).group(1)
    assert re.findall(r"^\s*\w+\s+(\w+);\s*$", body, re.M)[-2:] == ["filter_value", "min_baseq"]
    assert int(re.search(r"#define XCK_F_MIN_BASEQ\s+(\d+)", h).group(1)) == capi.XCK_F_MIN_BASEQ
    assert "int  xck_push_batch_q(xck_engine* e, const xck_batch* b, const uint8_t* qual);" in h
    assert "int  xck_get_baseq_stats(xck_engine* e, xck_baseq_stats* out);" in h and "XCK_MIN_BASEQ=<Q>" in h
    assert ("xck_push_batch_q", C.c_int, [C.c_void_p, C.POINTER(capi.Batch), C.POINTER(C.c_uint8)]) in capi.SYMBOLS
    assert ("xck_get_baseq_stats", C.c_int, [C.c_void_p, C.POINTER(capi.BaseqStats)]) in capi.SYMBOLS
    assert "#define XCK_ABI_VERSION 3" in h
