"""The opt-in tag filter (xck_config.filter_tag / XCK_TAG_FILTER, include/xck.h) in the HOST parser, without a GPU: decode-only handles
through Engine.decode_bam over the crafted file of tests/tag_filter_cases.py.  The verdict per record is Python's, on the records as
oracle/pybam.py reads them: the cell column must be XCK_CELL_FILTERED exactly there and the unfiltered decode's everywhere else, every
other column must not change, and xck_decode_stats.tag_filtered must be the predicted number.  Also the knob's grammar, the XCK_E_ARG
cases, and the two grown structs against the C header."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tag_filter_cases as T
from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    c = T.craft(str(tmp_path_factory.mktemp("tag_filter")))
    c["tables"] = T.tables(c)
    return c


@pytest.fixture(autouse=True)
def _no_knob(monkeypatch):
    monkeypatch.delenv("XCK_TAG_FILTER", raising=False)
    monkeypatch.delenv("XCK_CHUNK_BYTES", raising=False)


def _engine(c, mode=capi.XCK_MODE_BAF, n_threads=1, **kw):
    names, regions, snps, barcodes = c["tables"]
    return Engine(mode, names, regions, len(barcodes), snps=snps if mode & capi.XCK_MODE_BAF else (), barcodes=barcodes, cell_tag="CB", umi_tag="UB",
                  decode_only=True, n_threads=n_threads, **kw)


def _decode(c, n_threads=1, **kw):
    """-> (columns of the whole file, concatenated over its batches; tag_filtered; the engine's tag_filter)"""
    eng = _engine(c, n_threads=n_threads, **kw)
    try:
        got = list(eng.decode_bam(c["bam"], n_threads=n_threads))
        st = eng.decode_stats()
        tf = eng.tag_filter
    finally:
        eng.close()
    cols = {k: np.concatenate([g[k] for g in got]) for k in ("pos", "flag", "mapq", "cell", "umi")}
    cols["ordinal"] = np.concatenate([g["ordinal_base"] + np.arange(g["n_reads"], dtype=np.uint64) for g in got])
    cols["contig"] = np.concatenate([np.full(g["n_reads"], g["contig"], np.int32) for g in got])
    for off, dat in (("cig_off", "cigar"), ("seq_off", "seq")):
        cols[dat] = [bytes(g[dat][g[off][i]:g[off][i + 1]].tobytes()) for g in got for i in range(g["n_reads"])]
    return cols, int(st["tag_filtered"]), tf


def _check(c, full, filt, n_filtered, value, mask, umi_bits=None):
    names = c["tables"][0]
    recs, ok, wanted = T.verdicts(c["bam"], names, value, mask)
    fail = ~ok[wanted]                                                      # per record that reaches a batch, in file order
    assert len(fail) == len(full["cell"]) == len(filt["cell"])
    assert np.array_equal(filt["cell"][fail], np.full(int(fail.sum()), capi.XCK_CELL_FILTERED, np.int32))
    assert np.array_equal(filt["cell"][~fail], full["cell"][~fail])
    assert (full["cell"] >= -1).all()                                       # the unfiltered decode knows no -2
    for k in ("pos", "flag", "mapq", "ordinal", "contig"):
        assert np.array_equal(filt[k], full[k]), k
    assert filt["cigar"] == full["cigar"] and filt["seq"] == full["seq"]
    # keys: the 2-bit coded ones and XCK_UMI_NONE are equal; an interned one (the UMIs with N) is interned in both decodes
    hi = np.uint64(1) << np.uint64(63)
    interned = lambda u: ((u & hi) != 0) & (u != np.uint64(capi.XCK_UMI_NONE))
    assert np.array_equal(interned(filt["umi"]), interned(full["umi"])) and int(interned(full["umi"]).sum()) == len(T.N_UMI_AT)
    assert np.array_equal(filt["umi"][~interned(full["umi"])], full["umi"][~interned(full["umi"])])
    assert n_filtered == int(fail.sum())
    return int(fail.sum())


@pytest.mark.parametrize("how", ["config", "knob"])
@pytest.mark.parametrize("pred", sorted(T.PREDICATES))
def test_host_parse_marks_exactly_the_failing_records(crafted, pred, how, monkeypatch):
    value, mask = T.PREDICATES[pred]
    full, n0, tf0 = _decode(crafted, flags=capi.XCK_F_FORCE_KEY128)         # (64-bit key codes: an interned id has the top bit)
    assert n0 == 0 and tf0 is None
    if how == "config":
        filt, n, tf = _decode(crafted, flags=capi.XCK_F_FORCE_KEY128, tag_filter=(T.TAG, value, mask) if mask != T.ALL else (T.TAG, value))
    else:
        monkeypatch.setenv("XCK_TAG_FILTER", "%s:%d" % (T.TAG, value) if mask == T.ALL else "%s:0x%x/%d" % (T.TAG, value, mask))
        filt, n, tf = _decode(crafted, flags=capi.XCK_F_FORCE_KEY128)
    assert tf == (T.TAG, value, mask)
    n_fail = _check(crafted, full, filt, n, value, mask)
    print("tag filter %s (%s): %d of %d records in batches filtered" % (pred, how, n_fail, len(full["cell"])))
    if pred == "none":
        assert n_fail == len(full["cell"])
    else:
        assert 0 < n_fail < len(full["cell"])


@pytest.mark.parametrize("n_threads", [1, 3])
def test_host_parse_over_many_chunks_and_threads(crafted, n_threads, monkeypatch):
    value, mask = T.PREDICATES["exact"]
    monkeypatch.setenv("XCK_CHUNK_BYTES", str(T.SMALL_CHUNK_BYTES))
    full, n0, _ = _decode(crafted, n_threads=n_threads, flags=capi.XCK_F_FORCE_KEY128)
    filt, n, _ = _decode(crafted, n_threads=n_threads, flags=capi.XCK_F_FORCE_KEY128, tag_filter=(T.TAG, value))
    assert n0 == 0
    _check(crafted, full, filt, n, value, mask)


def test_config_fields_win_over_the_knob(crafted, monkeypatch):
    monkeypatch.setenv("XCK_TAG_FILTER", "xf:8/8")
    full, _, _ = _decode(crafted, flags=capi.XCK_F_FORCE_KEY128, tag_filter=("zz", 0, 0))    # (no record has zz: everything is filtered)
    assert (full["cell"] == capi.XCK_CELL_FILTERED).all()
    monkeypatch.delenv("XCK_TAG_FILTER")
    plain, _, _ = _decode(crafted, flags=capi.XCK_F_FORCE_KEY128)
    filt, n, tf = _decode(crafted, flags=capi.XCK_F_FORCE_KEY128, tag_filter=(T.TAG, 25))
    monkeypatch.setenv("XCK_TAG_FILTER", "xf:8/8")
    filt2, n2, tf2 = _decode(crafted, flags=capi.XCK_F_FORCE_KEY128, tag_filter=(T.TAG, 25))
    assert tf2 == tf == (T.TAG, 25, T.ALL) and n2 == n and np.array_equal(filt2["cell"], filt["cell"])
    _check(crafted, plain, filt2, n2, 25, T.ALL)


def test_counter_is_summed_over_the_readers_of_a_handle(crafted):
    eng = _engine(crafted, tag_filter=(T.TAG, 25))
    try:
        for _ in eng.decode_bam(crafted["bam"]):
            pass
        n = eng.decode_stats()["tag_filtered"]
        for _ in eng.decode_bam(crafted["bam"]):                             # summed over readers
            pass
        assert n > 0 and eng.decode_stats()["tag_filtered"] == 2 * n
    finally:
        eng.close()


@pytest.mark.parametrize("text,want", [("xf:25", ("xf", 25, T.ALL)), ("xf:8/8", ("xf", 8, 8)), ("xf:0x19", ("xf", 25, T.ALL)), ("xf:0x19/0xFF", ("xf", 25, 255)),
                                        ("xf:0/0", ("xf", 0, 0)), ("XF:4294967295", ("XF", T.ALL, T.ALL)), ("x1:025", ("x1", 25, T.ALL))])
def test_knob_grammar_accepts(crafted, text, want, monkeypatch):
    monkeypatch.setenv("XCK_TAG_FILTER", text)
    eng = _engine(crafted)
    try:
        assert eng.tag_filter == want
        got = np.concatenate([g["cell"] for g in eng.decode_bam(crafted["bam"])])
        n = eng.decode_stats()["tag_filtered"]
    finally:
        eng.close()
    names = crafted["tables"][0]
    _, ok, wanted = T.verdicts(crafted["bam"], names, want[1], want[2], want[0])
    assert np.array_equal(got == capi.XCK_CELL_FILTERED, ~ok[wanted]) and n == int((~ok[wanted]).sum())


@pytest.mark.parametrize("text", ["xf", "xf:", "xf25", "x:25", "xfx:25", "xf:25/", "xf:/8", "xf:-1", "xf:4294967296", "xf:25/0x1FFFFFFFF", "xf:abc", "xf:25 ", "xf:0x",
                                  "xf:1e3", "xf:25/8/8",
                                  "xf:9/8",                                  # value outside the mask: nothing could pass
                                  "x\x01:25",                                # not printable
                                  "CB:1", "UB:1"])                           # the handle's own tags
def test_malformed_knob_fails_create_and_is_quoted(crafted, text, monkeypatch):
    monkeypatch.setenv("XCK_TAG_FILTER", text)
    with pytest.raises(XckError) as ei:
        _engine(crafted)
    assert ei.value.code == capi.XCK_E_ARG
    if text not in ("xf:9/8", "x\x01:25", "CB:1", "UB:1"):                  # (well-formed, refused for what they say)
        assert '"%s"' % text in str(ei.value)
    assert "XCK_TAG_FILTER" in str(ei.value)


@pytest.mark.parametrize("tf", [("x", 1), ("x\x7f", 1), (" f", 1), ("CB", 1), ("UB", 1), ("xf", 9, 8), ("xf", 1, 0)])
def test_config_fields_that_are_refused(crafted, tf):
    if len(tf[0]) != 2:
        with pytest.raises(ValueError):
            _engine(crafted, tag_filter=tf)
        return
    with pytest.raises(XckError) as ei:
        _engine(crafted, tag_filter=tf)
    assert ei.value.code == capi.XCK_E_ARG and "filter" in str(ei.value)


def test_one_character_tag_through_the_abi_is_refused(lib):
    cfg = capi.Config()
    cfg.struct_size = C.sizeof(capi.Config)
    cfg.mode = 1; cfg.n_cells = 1; cfg.flags = capi.XCK_F_DECODE_ONLY
    cfg.filter_tag = b"x"; cfg.filter_mask = T.ALL; cfg.filter_value = 1
    h = C.c_void_p()
    assert lib.xck_create(C.byref(cfg), C.byref(h)) == capi.XCK_E_ARG
    assert b"two printable" in lib.xck_last_error(None)
    cfg.filter_tag = b"xfz"                                                 # three characters
    assert lib.xck_create(C.byref(cfg), C.byref(h)) == capi.XCK_E_ARG


def test_well_mode_handle_may_filter_on_any_tag(lib):
    """without barcodes / a UMI tag the handle has no cell_tag / umi_tag to collide with"""
    eng = Engine(capi.XCK_MODE_BASEFC, ["1"], [("1", 1, 100, "g")], 1, decode_only=True, tag_filter=("CB", 1))
    assert eng.tag_filter == ("CB", 1, T.ALL)
    eng.close()


def _header_numbers(tmp_path, struct_name, fields):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "xck.h"\nint main(void) { printf("%%zu", sizeof(%s));\n' % struct_name
                   + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct_name, n) for n in fields) + 'printf(" %d", XCK_CELL_FILTERED); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


@pytest.mark.parametrize("mirror,struct_name", [(capi.Config, "xck_config"), (capi.DecodeStats, "xck_decode_stats")])
def test_grown_struct_mirrors_match_the_header(mirror, struct_name, tmp_path):
    fields = [n for n, _ in mirror._fields_]
    got = _header_numbers(tmp_path, struct_name, fields)
    assert got[0] == C.sizeof(mirror)
    assert got[1:-1] == [getattr(mirror, n).offset for n in fields]
    assert got[-1] == capi.XCK_CELL_FILTERED == -2
    assert fields[-3:] == ["filter_tag", "filter_mask", "filter_value"] if mirror is capi.Config else fields[-1] == "tag_filtered"


def test_shorter_structs_are_still_accepted(crafted, lib):
    names, regions, snps, barcodes = crafted["tables"]
    sizes = (capi.Config.n_excl_pairs.offset, capi.Config.filter_tag.offset, C.sizeof(capi.Config))
    assert len(set(sizes)) == 3 and C.sizeof(capi.Config) - 4 not in sizes
    eng = _engine(crafted)                                                  # (its tables back the raw structs below)
    try:
        for size in sizes:
            cfg = capi.Config.from_buffer_copy(bytes(eng.cfg))
            cfg.struct_size = size
            cfg.filter_tag = b"xf"; cfg.filter_mask = 9; cfg.filter_value = 8   # (fields beyond a shorter struct_size: not read)
            h = C.c_void_p()
            assert lib.xck_create(C.byref(cfg), C.byref(h)) == 0, size
            try:
                # a short xck_decode_stats gets the fields it knows; the byte behind it is not written
                for n_fields, last in ((10, "gpu_path_given_up"), (12, "gpu_parse_fallbacks"), (15, "gpu_names_host_chunks"), (16, "tag_filtered")):
                    st = capi.DecodeStats()
                    C.memset(C.byref(st), 0x5A, C.sizeof(st))
                    st.struct_size = getattr(capi.DecodeStats, last).offset + 8
                    assert lib.xck_get_decode_stats(h, C.byref(st)) == 0
                    raw = bytes(st)
                    assert raw[st.struct_size:] == b"\x5A" * (C.sizeof(st) - st.struct_size), (size, last)
                    assert getattr(st, last) == 0
            finally:
                lib.xck_destroy(h)
    finally:
        eng.close()
