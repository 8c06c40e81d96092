"""Host-side checks of the front-ends' output stage (no GPU, no library): the one skeleton of the four summary writers under a fake
multi-rank context, write_summaries' file names and order of collectives, the row selection of write_snp_summary, write_matrix_set
against row_map_from_rows / row_map_all, and run_logged."""
import logging
import os

import numpy as np
import pytest

from xcltk_amd import capi
from xcltk_amd import fc_common as fcc
from xcltk_amd.engine import XckError

BASEFC, BAF = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF
NAMES = ["cellB", "cellA"]
REGIONS = [("1", 101, 200, "geneB"), ("2", 5, 9, "geneA")]
SNPS = [("1", 100 + i, "ACGT"[i % 4], "CGTA"[i % 4], i % 2, 1 - i % 2) for i in range(8)]
FATE = {k: 3 * i + 1 for i, k in enumerate(capi.READ_FATE_FIELDS)}
CELL_FATE = np.arange(3 * 12, dtype=np.int64).reshape(3, 12) + 1
CELL_MATRIX = {BASEFC: np.array([[100, 7], [200, 9]], dtype=np.int64), BAF: np.array([[5, 9, 1, 4], [0, 2, 0, 1]], dtype=np.int64)}
FEAT_READS = np.array([[1, 10, 4], [2, 0, 0]], dtype=np.int64)
FEAT_MATRIX = {BASEFC: np.array([[7, 3], [1, 1]], dtype=np.int64), BAF: np.array([[3, 2, 5, 9, 1, 4], [1, 0, 0, 0, 0, 0]], dtype=np.int64)}
SNP_TABLE = np.arange(8 * 8, dtype=np.int64).reshape(8, 8) + 1


class On(object):
    """An engine-like object that keeps every table.  mode: the handle's; a BOTH handle answers for the pipeline it is asked about."""

    def __init__(self, mode=BAF):
        self.mode = mode
        self._snp = {"contig": np.zeros(len(SNPS), dtype=np.int32)}

    def read_fate(self, mode=None):
        return dict(FATE)

    def cell_summary(self, mode=None):
        mode = self.mode if mode is None else mode
        return dict(fate=CELL_FATE.copy(), matrix=CELL_MATRIX[mode].copy(), fate_cols=capi.CELL_FATE_COLS, matrix_cols=capi.CELL_MATRIX_COLS[mode])

    def feature_summary(self, mode=None):
        mode = self.mode if mode is None else mode
        return dict(reads=FEAT_READS.copy() if mode == BASEFC else None, matrix=FEAT_MATRIX[mode].copy(), snp=SNP_TABLE.copy() if mode == BAF else None,
                    has_matrix=True, read_cols=capi.FEATURE_READ_COLS, matrix_cols=capi.FEATURE_MATRIX_COLS[mode], snp_cols=capi.SNP_COLS)


class Off(object):
    mode = BAF

    def read_fate(self, mode=None):
        return None

    def cell_summary(self, mode=None):
        return None

    def feature_summary(self, mode=None):
        return None


class FakeDist(object):
    """Two ranks, one contig cut over them; the other rank counted what this one counted."""
    active, world, sharded_output = True, 2, False
    units = [dict(contig=0, window=(0, 500)), dict(contig=0, window=(500, 0)), dict(contig=1, window=None)]

    def __init__(self):
        self.calls = []

    def all_reduce_np(self, x, op="sum"):
        x = np.asarray(x)
        self.calls.append((x.shape, op))
        return 2 * x


def _fate2():
    return {k: 2 * v for k, v in FATE.items()}


# writer -> (call on (eng, dist, path), size of its tables, text of the file from doubled tables, the doubled table out of the return value)
WRITERS = {
    "read": (lambda e, d, fn: fcc.write_read_summary(e, d, fn), len(capi.READ_FATE_FIELDS),
             lambda: fcc.read_summary_text(_fate2(), 2, 1), lambda got: got == _fate2()),
    "cell": (lambda e, d, fn: fcc.write_cell_summary(e, d, fn, NAMES), CELL_FATE.size + CELL_MATRIX[BAF].size,
             lambda: fcc.cell_summary_text(NAMES, 2 * CELL_FATE, 2 * CELL_MATRIX[BAF], capi.CELL_FATE_COLS, capi.CELL_MATRIX_COLS[BAF], 2, 1),
             lambda got: np.array_equal(got["fate"], 2 * CELL_FATE) and np.array_equal(got["matrix"], 2 * CELL_MATRIX[BAF])),
    "feature": (lambda e, d, fn: fcc.write_feature_summary(e, d, fn, REGIONS), FEAT_MATRIX[BAF].size,
                lambda: fcc.feature_summary_text(REGIONS, None, 2 * FEAT_MATRIX[BAF], BAF, 2, 1),
                lambda got: got["reads"] is None and np.array_equal(got["matrix"], 2 * FEAT_MATRIX[BAF])),
    "snp": (lambda e, d, fn: fcc.write_snp_summary(e, d, fn, SNPS), SNP_TABLE.size,
            lambda: fcc.snp_summary_text(SNPS, 2 * SNP_TABLE, 2, 1), lambda got: np.array_equal(got, 2 * SNP_TABLE)),
}


@pytest.mark.parametrize("which", sorted(WRITERS))
def test_writer_sums_in_one_all_reduce_and_heads_the_file(which, tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    call, size, text, summed = WRITERS[which]
    dist, fn = FakeDist(), str(tmp_path / "sub" / "t.tsv")
    got = call(On(), dist, fn)
    assert dist.calls == [((size,), "sum")]                      # ONE collective, over all of the writer's tables
    with open(fn) as fp:
        body = fp.read()
    assert body.startswith("#ranks=2 cut_contigs=1\n") and body == text()    # (the *_text functions are pinned by their own tests)
    assert summed(got)


@pytest.mark.parametrize("which", sorted(WRITERS))
def test_writer_on_another_rank_joins_the_collective_and_writes_nothing(which, tmp_path, monkeypatch):
    monkeypatch.setenv("RANK", "1")
    call, size, _, summed = WRITERS[which]
    dist, fn = FakeDist(), str(tmp_path / "sub" / "t.tsv")
    got = call(On(), dist, fn)
    assert dist.calls == [((size,), "sum")] and summed(got)
    assert not os.path.exists(os.path.dirname(fn))


def test_basefc_feature_summary_sums_reads_and_matrix_together(tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    dist, fn = FakeDist(), str(tmp_path / "f.tsv")
    got = fcc.write_feature_summary(On(BASEFC), dist, fn, REGIONS)
    assert dist.calls == [((FEAT_READS.size + FEAT_MATRIX[BASEFC].size,), "sum")]
    assert np.array_equal(got["reads"], 2 * FEAT_READS) and np.array_equal(got["matrix"], 2 * FEAT_MATRIX[BASEFC])
    with open(fn) as fp:
        assert fp.read() == fcc.feature_summary_text(REGIONS, 2 * FEAT_READS, 2 * FEAT_MATRIX[BASEFC], BASEFC, 2, 1)


def test_snp_summary_zeroes_foreign_contigs_before_the_reduce(tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    eng, dist = On(), FakeDist()
    eng._snp["contig"][4:] = 1
    dist.contig_mask = np.array([True, False])                   # this rank streams contig 0 only
    got = fcc.write_snp_summary(eng, dist, str(tmp_path / "s.tsv"), SNPS)
    assert np.array_equal(got[:4], 2 * SNP_TABLE[:4]) and not got[4:].any()


SUMMARY_FILES = ("read_summary.tsv", "cell_summary.tsv", "feature_summary.tsv", "snp_summary.tsv")


@pytest.mark.parametrize("prefix", ["", "xcltk."])
def test_write_summaries_names_and_order(prefix, tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    d = str(tmp_path / "out")
    dist = FakeDist()
    fcc.write_summaries(On(), dist, os.path.join(d, prefix), NAMES, REGIONS, SNPS)
    assert sorted(os.listdir(d)) == sorted(prefix + f for f in SUMMARY_FILES)
    assert [c[0][0] for c in dist.calls] == [WRITERS[k][1] for k in ("read", "cell", "feature", "snp")]   # read, cell, feature, SNP
    with open(os.path.join(d, prefix + "snp_summary.tsv")) as fp:
        assert fp.read() == fcc.snp_summary_text(SNPS, 2 * SNP_TABLE, 2, 1)


def test_write_summaries_without_a_snp_file(tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    # a basefc handle; the basefc pipeline of a fused handle; the pileup pipeline without a SNP list
    for k, (eng, snps, mode) in enumerate(((On(BASEFC), SNPS, None), (On(capi.XCK_MODE_BOTH), SNPS, BASEFC), (On(BAF), None, None))):
        d, dist = str(tmp_path / ("o%d" % k)), FakeDist()
        fcc.write_summaries(eng, dist, os.path.join(d, ""), NAMES, REGIONS, snps, mode)
        assert sorted(os.listdir(d)) == sorted(SUMMARY_FILES[:3]) and len(dist.calls) == 3
    d, dist = str(tmp_path / "both"), FakeDist()                 # the pileup pipeline of a fused handle writes all four
    fcc.write_summaries(On(capi.XCK_MODE_BOTH), dist, os.path.join(d, ""), NAMES, REGIONS, SNPS, BAF)
    assert sorted(os.listdir(d)) == sorted(SUMMARY_FILES) and len(dist.calls) == 4


def test_write_summaries_on_a_handle_that_keeps_nothing(tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    for eng in (Off(), object()):
        d, dist = str(tmp_path / "out"), FakeDist()
        fcc.write_summaries(eng, dist, os.path.join(d, "xcltk."), NAMES, REGIONS, SNPS)
        assert dist.calls == [] and not os.path.exists(d)


def test_snp_summary_row_selection(tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    rows = np.array([5, 0, 3])
    chosen = [SNPS[i] for i in rows]
    fn = str(tmp_path / "missing" / "dir" / "xcltk.snp_summary.tsv")
    got = fcc.write_snp_summary(On(), None, fn, chosen, rows=rows)
    assert np.array_equal(got, SNP_TABLE[[5, 0, 3]])
    with open(fn) as fp:
        assert fp.read() == fcc.snp_summary_text(chosen, SNP_TABLE[[5, 0, 3]])
    # the whole table in order is the selection that selects everything
    fcc.write_snp_summary(On(), None, fn, SNPS, rows=np.arange(8))
    with open(fn) as fp:
        assert fp.read() == fcc.snp_summary_text(SNPS, SNP_TABLE)
    dist = FakeDist()                                            # several ranks: the selected rows are what is summed
    fcc.write_snp_summary(On(), dist, fn, chosen, rows=rows)
    assert dist.calls == [((3 * 8,), "sum")]
    with open(fn) as fp:
        assert fp.read() == fcc.snp_summary_text(chosen, 2 * SNP_TABLE[[5, 0, 3]], 2, 1)


# ---- write_matrix_set ----------------------------------------------------------------------------------------------------------------
REG5 = [("1", 100 * i + 1, 100 * i + 50, "g%d" % i) for i in range(5)]


def _coo(rows):
    r = np.array(rows, dtype=np.int32)
    return (r, np.zeros(len(r), dtype=np.int32), np.ones(len(r), dtype=np.int32))


class MtxEngine(object):
    n_cells = 2

    def __init__(self):
        self.mtx, self.groups = [], []

    def write_mtx_arrays(self, path, coo_k, rm, n_rows_out, n_cols=None):
        self.mtx.append((path, coo_k, np.array(rm), n_rows_out, n_cols))

    def group_counts(self, cell_group, n_groups=0, source="result", copy=True):
        self.groups.append((np.array(cell_group), n_groups, source))
        return {k: _coo([]) for k in ("count", "ad", "dp", "oth")}


SETS = {   # the two front-end shapes: keys in file order, the keys that decide the rows, what touches which rows
    "basefc": (("count",), ("count",), {"count": _coo([1, 3, 3])}, [1, 3]),
    "baf": (("ad", "dp", "oth"), ("dp", "oth"), {"ad": _coo([]), "dp": _coo([0]), "oth": _coo([4])}, [0, 4]),
}


@pytest.mark.parametrize("all_reg", [False, True])
@pytest.mark.parametrize("which", sorted(SETS))
def test_matrix_set_rows_region_file_and_order(which, all_reg, tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    keys, presence, coo, touched = SETS[which]
    d = str(tmp_path)
    mtx_fns = {k: os.path.join(d, k + ".mtx") for k in keys}
    group_fns = {k: os.path.join(d, k + ".groups.mtx") for k in keys}
    groups = (["g0", "g1"], np.array([1, 0], dtype=np.int32))
    eng = MtxEngine()
    fcc.write_matrix_set(eng, None, REG5, coo, all_reg, os.path.join(d, "region.tsv"), mtx_fns, presence, groups, os.path.join(d, "groups.tsv"), group_fns)
    rm = fcc.row_map_all(5) if all_reg else fcc.row_map_from_rows(5, np.array(touched))
    n_rows = 5 if all_reg else 2
    with open(os.path.join(d, "region.tsv")) as fp:
        assert fp.read().splitlines() == ["%s\t%d\t%d\t%s" % r for r, k in zip(REG5, rm) if k > 0]
    cell, grp = eng.mtx[:len(keys)], eng.mtx[len(keys):]
    assert [c[0] for c in cell] == [mtx_fns[k] for k in keys] and [c[0] for c in grp] == [group_fns[k] for k in keys]
    for (_, coo_k, got_rm, got_rows, n_cols), k in zip(cell, keys):
        assert coo_k is coo[k] and np.array_equal(got_rm, rm) and got_rows == n_rows == int(rm.max()) and n_cols is None
    assert all(np.array_equal(g[2], rm) and g[3] == n_rows and g[4] == 2 for g in grp)
    assert len(eng.groups) == 1 and eng.groups[0][1:] == (2, "result") and np.array_equal(eng.groups[0][0], groups[1])
    with open(os.path.join(d, "groups.tsv")) as fp:
        assert fp.read() == "g0\ng1\n"


def test_matrix_set_without_groups_and_without_regions(tmp_path, monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    d = str(tmp_path)
    for all_reg in (False, True):
        eng = MtxEngine()
        fcc.write_matrix_set(eng, None, [], {"count": _coo([])}, all_reg, os.path.join(d, "features.tsv"), {"count": os.path.join(d, "matrix.mtx")},
                             ("count",), None, os.path.join(d, "groups.tsv"), {"count": os.path.join(d, "matrix.groups.mtx")})
        assert [(c[0], len(c[2]), c[3]) for c in eng.mtx] == [(os.path.join(d, "matrix.mtx"), 0, 0)]    # 0 rows, and groups=None: no group_counts call
        assert eng.groups == [] and os.path.getsize(os.path.join(d, "features.tsv")) == 0 and not os.path.exists(os.path.join(d, "groups.tsv"))


def test_matrix_set_on_another_rank_writes_no_region_file(tmp_path, monkeypatch):
    monkeypatch.setenv("RANK", "1")
    eng, d = MtxEngine(), str(tmp_path)
    fcc.write_matrix_set(eng, None, REG5, SETS["basefc"][2], False, os.path.join(d, "features.tsv"), {"count": os.path.join(d, "matrix.mtx")},
                         ("count",), (["g0"], np.zeros(2, dtype=np.int32)), os.path.join(d, "groups.tsv"), {"count": os.path.join(d, "matrix.groups.mtx")})
    assert os.listdir(d) == [] and len(eng.mtx) == 2


# ---- run_logged ----------------------------------------------------------------------------------------------------------------------
class Conf(object):
    argv = None


def test_run_logged_return_codes_and_log_lines(caplog):
    caplog.set_level(logging.INFO)
    seen = []
    assert fcc.run_logged(seen.append, Conf()) == 0 and len(seen) == 1
    texts = [r.getMessage() for r in caplog.records]
    assert texts[0].startswith("start time: ") and texts[1:2] == ["All Done!"] and texts[2].startswith("end time: ") and texts[3].startswith("time spent: ")
    for exc in (ValueError("errcode -2"), XckError("no GPU", 5)):
        caplog.clear()

        def core(conf, exc=exc):
            raise exc
        assert fcc.run_logged(core, Conf()) == -1
        errors = [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR]
        assert errors == [str(exc), "Running program failed.", "Quiting ..."]
    with pytest.raises(KeyError):                                 # anything else is not the front-end's to report
        fcc.run_logged(lambda conf: {}["x"], Conf())


def test_run_logged_repeats_the_command_line(caplog):
    caplog.set_level(logging.INFO)
    conf = Conf()
    conf.argv = ["xcltk", "basefc", "-O", "out"]
    assert fcc.run_logged(lambda c: None, conf) == 0
    assert [r.getMessage() for r in caplog.records].count("CMD: xcltk basefc -O out") == 2
