"""Host-side checks of the read assignment summary (no GPU): the ctypes mirror of xck_read_fate against the header text, the flag
rules that xck_create can decide without a device, the text of read_summary.tsv, and the fixtures themselves."""
import ctypes as C
import os
import re

import pytest

import read_fate_util as R
from xcltk_amd import capi
from xcltk_amd import fc_common as fcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "xck.h")) as fp:
        return fp.read()


def test_struct_mirrors_the_header():
    h = _header()
    body = re.search(r"typedef struct xck_read_fate \{(.*?)\} xck_read_fate;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    ctypes_of = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int64_t": C.c_int64}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(capi.ReadFate._fields_)
    assert C.sizeof(capi.ReadFate) == 8 + 8 * 14
    assert [n for n, _ in fields[2:]] == list(R.FIELDS) == list(capi.READ_FATE_FIELDS)
    assert capi.READ_FATE_CLASSES == R.CLASSES
    assert int(re.search(r"#define XCK_F_READ_FATE\s+(\d+)", h).group(1)) == capi.XCK_F_READ_FATE == 32
    assert int(re.search(r"#define XCK_ABI_VERSION (\d+)", h).group(1)) == 3          # additive: the ABI version stays
    assert "XCK_READ_FATE=1" in h.split("#ifndef XCK_H")[0]                          # the environment list names the knob


def test_library_exports_the_entry_point(lib):
    assert lib.xck_abi_version() == 3
    assert ("xck_get_read_fate", C.c_int, [C.c_void_p, C.c_int, C.POINTER(capi.ReadFate)]) in capi.SYMBOLS
    assert lib.xck_get_read_fate.argtypes == [C.c_void_p, C.c_int, C.POINTER(capi.ReadFate)]


def test_flag_is_refused_on_decode_only_handles(lib, monkeypatch):
    from xcltk_amd.engine import Engine, XckError
    monkeypatch.delenv("XCK_READ_FATE", raising=False)
    with pytest.raises(XckError) as ei:
        Engine(capi.XCK_MODE_BASEFC, ["1"], [("1", 1, 100, "g")], 1, flags=capi.XCK_F_READ_FATE, decode_only=True)
    assert ei.value.code == capi.XCK_E_ARG
    # a decode-only handle has no summary: XCK_E_STATE through the C-ABI, None from Engine.read_fate() - with and without the
    # environment knob, which such handles ignore (Dist.plan() probes BAM indexes through one in every multi-GPU run)
    for env in (None, "1"):
        if env:
            monkeypatch.setenv("XCK_READ_FATE", env)
        with Engine(capi.XCK_MODE_BASEFC, ["1"], [("1", 1, 100, "g")], 1, decode_only=True) as eng:
            rf = capi.ReadFate()
            rf.struct_size = C.sizeof(capi.ReadFate)
            assert lib.xck_get_read_fate(eng.h, capi.XCK_MODE_BASEFC, C.byref(rf)) == capi.XCK_E_STATE
            assert eng.read_fate() is None
            rf.struct_size = 8
            assert lib.xck_get_read_fate(eng.h, capi.XCK_MODE_BASEFC, C.byref(rf)) == capi.XCK_E_ARG
    assert lib.xck_get_read_fate(None, capi.XCK_MODE_BASEFC, None) == capi.XCK_E_ARG


def test_summary_text():
    fate = {k: i * 7 for i, k in enumerate(R.FIELDS)}
    one = fcc.read_summary_text(fate)
    assert one == "".join("%s\t%d\n" % (k, i * 7) for i, k in enumerate(R.FIELDS))
    assert one.splitlines()[0] == "n_reads\t0" and one.splitlines()[-1] == "pairs\t%d" % (7 * 13)
    many = fcc.read_summary_text(fate, n_ranks=4, cut_contigs=2)
    assert many == "#ranks=4 cut_contigs=2\n" + one
    assert fcc.read_summary_text(fate, n_ranks=1, cut_contigs=0) == one


def test_summary_writer_without_the_flag_writes_nothing(tmp_path):
    class Off(object):
        def read_fate(self, mode=None):
            return None
    fn = str(tmp_path / "read_summary.tsv")
    assert fcc.write_read_summary(Off(), None, fn) is None
    assert not os.path.exists(fn)

    class On(object):
        def read_fate(self, mode=None):
            return {k: 3 for k in R.FIELDS}
    assert fcc.write_read_summary(On(), None, fn)["pairs"] == 3
    with open(fn) as fp:
        assert fp.read() == fcc.read_summary_text({k: 3 for k in R.FIELDS})


@pytest.mark.parametrize("name", R.list_fixtures())
def test_fixture_classes_sum_to_the_records(name):
    """(I1) on the fixtures themselves, and the ranges the sums must keep"""
    fx = R.load_fixture(name)
    f = fx["fate"]
    assert sorted(f) == sorted(R.CLASSES + ("multi", "pairs"))
    assert sum(f[k] for k in R.CLASSES) + fx["outside_table"] == fx["records"]
    assert f["multi"] <= f["assigned"] and f["pairs"] >= f["assigned"] + f["multi"]
    if fx["mode"] == "baf":
        assert f["include_fail"] == 0
    for fn in fx["bam_fns"] + [fx["region_fn"]]:
        assert os.path.isfile(fn)


def test_the_issue_s_table_is_what_the_generator_wrote():
    """the figures quoted when the feature was specified (c1: 6 386 of 7 824 counted reads are assigned to more than one feature)"""
    want = {"c1_basefc": (1000, 268, 0, 405, 300, 0, 1, 202, 7824, 6386, 23455),
            "dense_basefc": (601, 177, 0, 382, 142, 0, 0, 13, 4685, 4384, 16170),
            "special_basefc": (1, 2, 1, 2, 1, 8, 0, 3, 22, 13, 35),
            "special_basefc_inc30": (1, 2, 1, 2, 1, 8, 0, 1, 24, 16, 40),
            "multibam_basefc": (517, 132, 0, 251, 125, 0, 4, 138, 3833, 2759, 8513),
            "well_basefc": (418, 172, 317, 0, 0, 0, 0, 6, 3887, 3805, 13851),
            "c1_baf": (1000, 268, 0, 405, 300, 0, 6971, 0, 1056, 654, 3503),
            "dense_baf": (601, 177, 0, 382, 142, 0, 3486, 0, 1212, 553, 9910),
            "special_baf": (1, 2, 1, 2, 1, 8, 6, 0, 19, 7, 28)}
    keys = ("low_mapq", "excl_flag", "orphan", "no_cell", "no_umi", "short_aligned", "no_target", "include_fail", "assigned", "multi", "pairs")
    for name, row in want.items():
        fx = R.load_fixture(name)
        assert tuple(fx["fate"][k] for k in keys) == row, name
        assert fx["fate"]["incl_flag"] == 0 and fx["fate"]["not_joined"] == 0
        assert fx["outside_table"] == (1 if fx["dataset"] == "special" else 0)
    assert R.load_fixture("dense_basefc_incl16")["fate"]["incl_flag"] > 0
    assert R.load_fixture("special_baf_regions_un")["fate"]["not_joined"] > 0
