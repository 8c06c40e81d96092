"""Host-side checks of the per-feature / per-SNP tables (no GPU): the ctypes mirror of xck_feature_summary against the header text, the
flag rules xck_create decides without a device, the text of feature_summary.tsv and snp_summary.tsv, the fixtures themselves, and
the plain-Python restatement against every fixture."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feature_summary_util as F
import read_fate_util as R
from xcltk_amd import capi
from xcltk_amd import fc_common as fcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASEFC, BAF = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF


def test_struct_mirrors_the_header():
    with open(os.path.join(ROOT, "include", "xck.h")) as fp:
        h = fp.read()
    body = re.search(r"typedef struct xck_feature_summary \{(.*?)\} xck_feature_summary;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, name = decl.rsplit(None, 1)
            fields.append((name, " ".join(ctype.split())))
    ctypes_of = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "const int64_t*": C.POINTER(C.c_int64)}
    assert [(n, ctypes_of[t]) for n, t in fields] == list(capi.FeatureSummary._fields_)
    assert capi.FEATURE_READ_COLS == F.READ_COLS and capi.SNP_COLS == F.SNP_COLS
    assert capi.FEATURE_MATRIX_COLS == {BASEFC: F.MATRIX_COLS["basefc"], BAF: F.MATRIX_COLS["baf"]}
    assert int(re.search(r"#define XCK_F_FEATURE_SUMMARY\s+(\d+)", h).group(1)) == capi.XCK_F_FEATURE_SUMMARY == 128
    assert int(re.search(r"#define XCK_ABI_VERSION (\d+)", h).group(1)) == 3          # additive: the ABI version stays
    env = h.split("#ifndef XCK_H")[0]
    assert "XCK_FEATURE_SUMMARY=1" in env and "XCK_CELL_SUMMARY_SLOTS" in env


def test_library_exports_the_entry_point(lib):
    assert lib.xck_abi_version() == 3
    assert lib.xck_get_feature_summary.argtypes == [C.c_void_p, C.c_int, C.POINTER(capi.FeatureSummary)]


def test_flag_is_refused_on_decode_only_handles(lib, monkeypatch):
    from xcltk_amd.engine import Engine, XckError
    monkeypatch.delenv("XCK_FEATURE_SUMMARY", raising=False)
    with pytest.raises(XckError) as ei:
        Engine(BASEFC, ["1"], [("1", 1, 100, "g")], 1, flags=capi.XCK_F_FEATURE_SUMMARY, decode_only=True)
    assert ei.value.code == capi.XCK_E_ARG
    for env in (None, "1"):                                    # decode-only handles ignore the environment knob
        if env:
            monkeypatch.setenv("XCK_FEATURE_SUMMARY", env)
        with Engine(BASEFC, ["1"], [("1", 1, 100, "g")], 1, decode_only=True) as eng:
            fs = capi.FeatureSummary()
            fs.struct_size = C.sizeof(capi.FeatureSummary)
            assert lib.xck_get_feature_summary(eng.h, BASEFC, C.byref(fs)) == capi.XCK_E_STATE
            assert eng.feature_summary() is None
            fs.struct_size = 8
            assert lib.xck_get_feature_summary(eng.h, BASEFC, C.byref(fs)) == capi.XCK_E_ARG
    assert lib.xck_get_feature_summary(None, BASEFC, None) == capi.XCK_E_ARG


REGIONS = [("1", 101, 200, "geneB"), ("2", 5, 9, "geneA")]


def test_feature_summary_text():
    reads = np.array([[1, 10, 4], [0, 0, 0]], dtype=np.int64)
    matrix = np.array([[7, 3], [0, 0]], dtype=np.int64)
    one = fcc.feature_summary_text(REGIONS, reads, matrix, BASEFC)
    assert one == ("chrom\tstart\tend\tname\tfetched\tinclude_fail\tpairs\tshared\tumis\tcells\n"
                   "1\t101\t200\tgeneB\t11\t1\t10\t4\t7\t3\n"
                   "2\t5\t9\tgeneA\t0\t0\t0\t0\t0\t0\n")
    assert fcc.feature_summary_text(REGIONS, reads, matrix, BASEFC, n_ranks=2, cut_contigs=1) == "#ranks=2 cut_contigs=1\n" + one
    assert fcc.feature_summary_text(REGIONS, reads, matrix, BASEFC, n_ranks=1) == one
    assert fcc.feature_summary_text(REGIONS, reads, None, BASEFC).splitlines()[1] == "1\t101\t200\tgeneB\t11\t1\t10\t4\t0\t0"
    baf = fcc.feature_summary_text(REGIONS, None, np.array([[3, 2, 5, 9, 1, 4], [0, 0, 0, 0, 0, 0]]), BAF)
    assert baf == ("chrom\tstart\tend\tname\tsnps\tsnps_kept\tad\tdp\toth\tcells\n"
                   "1\t101\t200\tgeneB\t3\t2\t5\t9\t1\t4\n"
                   "2\t5\t9\tgeneA\t0\t0\t0\t0\t0\t0\n")


def test_snp_summary_text():
    snps = [("1", 120, "A", "G", 0, 1), ("2", 7, "N", "T", 1, 0)]
    table = np.array([[9, 4, 0, 2, 1, 1, 1, 2], [3, 0, 0, 0, 1, 2, 0, 0]], dtype=np.int64)
    one = fcc.snp_summary_text(snps, table)
    assert one == ("chrom\tpos\tref\talt\tref_hap\talt_hap\treads\tA\tC\tG\tT\tN\ttotal\tref_umis\talt_umis\tkept\tregions\n"
                   "1\t120\tA\tG\t0\t1\t9\t4\t0\t2\t1\t1\t8\t4\t2\t1\t2\n"
                   "2\t7\tN\tT\t1\t0\t3\t0\t0\t0\t1\t2\t3\t2\t1\t0\t0\n")
    assert fcc.snp_summary_text(snps, table, n_ranks=3, cut_contigs=0) == "#ranks=3 cut_contigs=0\n" + one


def test_writers_on_off_and_method_absent(tmp_path):
    fn = str(tmp_path / "sub" / "feature_summary.tsv")

    class Off(object):
        mode = BASEFC

        def feature_summary(self, mode=None):
            return None

    class Absent(object):
        mode = BAF

    for eng in (Off(), Absent()):
        assert fcc.write_feature_summary(eng, None, fn, REGIONS) is None and fcc.write_snp_summary(eng, None, fn, []) is None
        assert not os.path.exists(fn)

    reads = np.array([[1, 10, 4], [0, 0, 0]], dtype=np.int64)

    class On(object):
        mode = BASEFC

        def feature_summary(self, mode=None):
            return dict(reads=reads, matrix=None, snp=None, has_matrix=False, read_cols=F.READ_COLS, matrix_cols=F.MATRIX_COLS["basefc"], snp_cols=F.SNP_COLS)
    got = fcc.write_feature_summary(On(), None, fn, REGIONS)
    assert np.array_equal(got["reads"], reads) and not got["matrix"].any()
    with open(fn) as fp:
        assert fp.read() == fcc.feature_summary_text(REGIONS, reads, None, BASEFC)
    assert fcc.write_snp_summary(On(), None, fn + ".snp", []) is None and not os.path.exists(fn + ".snp")


def test_writer_on_a_handle_without_regions(tmp_path):
    """no region: the getter hands out no array, the file is its header line"""
    fn = str(tmp_path / "feature_summary.tsv")

    class Empty(object):
        mode = BASEFC

        def feature_summary(self, mode=None):
            return dict(reads=None, matrix=None, snp=None, has_matrix=False, read_cols=F.READ_COLS, matrix_cols=F.MATRIX_COLS["basefc"], snp_cols=F.SNP_COLS)
    got = fcc.write_feature_summary(Empty(), None, fn, [])
    assert got["reads"].shape == (0, 3) and got["matrix"].shape == (0, 2)
    with open(fn) as fp:
        assert fp.read() == "chrom\tstart\tend\tname\tfetched\tinclude_fail\tpairs\tshared\tumis\tcells\n"


def _tables(fx):
    regions = fcc.load_region_from_txt(fx["region_fn"])
    snps = fcc.load_snp_from_tsv(os.path.join(fx["ddir"], "snps.tsv")) if fx["mode"] == "baf" else ()
    return regions, list(snps), fcc.contig_table(regions, snps)


def test_fixtures_are_consistent():
    names = F.list_fixtures()
    assert len(names) >= 13 and set(R.list_fixtures()) <= set(names)
    dropped = 0
    for name in names:
        fx, gx = F.load_fixture(name)
        regions, snps, _ = _tables(fx)
        tab = F.fixture_table(gx, regions, snps)
        assert os.path.getsize(os.path.join(F.FDIR, name + ".json")) < 100 * 1024
        if gx["mode"] == "basefc":
            assert tuple(gx["columns"]) == F.READ_COLS
            assert int(tab[:, F.PAIRS].sum()) == fx["fate"]["pairs"], name
            assert (tab[:, F.SHARED] <= tab[:, F.PAIRS]).all() and int(tab[:, F.SHARED].sum()) >= 2 * fx["fate"]["multi"]
        else:
            assert tuple(gx["columns"]) == F.SNP_COLS[:6] + ("ret",)
            assert int(tab[:, 0].sum()) == fx["fate"]["pairs"], name
            assert set(tab[:, 6].tolist()) <= {0, 3, 5}
            p = gx["params"]
            for s, row in zip(snps, tab):
                if row[6] == 3:
                    assert row[1:6].sum() < p["min_count"]
                assert F.verdict(row[1:6], s[2], s[3], p["min_count"], p["min_maf"]) == (1 if row[6] == 0 else 0), (name, s, row)
                assert row[1:6].sum() <= row[0]                  # a (cell, UMI) that shows a base is one of the reads
            dropped += int((tab[:, 6] == 5).sum())
    assert dropped > 0                                           # the two filter cases drop SNPs for their allele balance too


@pytest.mark.parametrize("name", F.list_fixtures())
def test_restatement_reproduces_the_fixture(name):
    """the per-pair restatement the GPU tests compare with, on the records oracle/pybam.py reads from the dataset"""
    fx, gx = F.load_fixture(name)
    regions, snps, names = _tables(fx)
    barcodes = None
    if fx["params"]["cell_tag"]:
        with open(os.path.join(fx["ddir"], fx["ds"]["barcodes"])) as fp:
            barcodes = sorted(x.strip() for x in fp)
    p = fx["params"]
    filt = {k: p[k] for k in ("min_mapq", "min_len", "excl_flag", "incl_flag", "no_orphan", "min_include")}
    want = F.fixture_table(gx, regions, snps)
    got, multi = F.restate(names, regions, snps, F.bam_batches(fx, names, barcodes), filt, gx["mode"] == "basefc")
    assert multi == fx["fate"]["multi"]
    if gx["mode"] == "basefc":
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:10]
    else:
        assert np.array_equal(got, want[:, 0]), np.flatnonzero(got != want[:, 0])[:10]
