"""Helpers of the read assignment summary tests (tests/test_read_fate_host.py, tests/test_gpu_read_fate.py, the two-rank worker):
the fixtures under tests/golden/read_fate/ (written by tools/make_read_fate_goldens.py from the reference's own check_read /
sam_fetch / include code) and an Engine built the way the front-ends build theirs."""
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FDIR = os.path.join(GOLDEN, "read_fate")
# the classes that sum to n_reads, then the two sums over the assigned reads (the order of xck_read_fate)
CLASSES = ("not_joined", "low_mapq", "excl_flag", "incl_flag", "orphan", "no_cell", "no_umi", "short_aligned", "no_target",
           "include_fail", "assigned")
FIELDS = ("n_reads",) + CLASSES + ("multi", "pairs")


def list_fixtures():
    return sorted(f[:-5] for f in os.listdir(FDIR) if f.endswith(".json")) if os.path.isdir(FDIR) else []


def load_fixture(name):
    with open(os.path.join(FDIR, name + ".json")) as fp:
        fx = json.load(fp)
    fx["ddir"] = os.path.join(GOLDEN, "datasets", fx["dataset"])
    with open(os.path.join(fx["ddir"], "dataset.json")) as fp:
        fx["ds"] = json.load(fp)
    fx["bam_fns"] = [os.path.join(fx["ddir"], b) for b in fx["ds"]["bams"]]
    fx["region_fn"] = fx["params"]["region_fn"].replace("$D/", fx["ddir"] + "/").replace("$F/", FDIR + "/")
    return fx


def fixture_engine(fx, flags, mode=None):
    """Engine over the fixture's dataset with the fixture's filters; mode: the fixture's own, or XCK_MODE_BOTH."""
    from xcltk_amd import capi
    from xcltk_amd import fc_common as fcc
    from xcltk_amd.engine import Engine
    p = fx["params"]
    if mode is None:
        mode = capi.XCK_MODE_BASEFC if fx["mode"] == "basefc" else capi.XCK_MODE_BAF
    regions = fcc.load_region_from_txt(fx["region_fn"])
    snps = fcc.load_snp_from_tsv(os.path.join(fx["ddir"], "snps.tsv")) if mode & capi.XCK_MODE_BAF else ()
    names = fcc.contig_table(regions, snps)
    barcodes = None
    if p["cell_tag"]:
        with open(os.path.join(fx["ddir"], fx["ds"]["barcodes"])) as fp:
            barcodes = sorted(x.strip() for x in fp)
    n_cells = len(barcodes) if barcodes is not None else len(fx["bam_fns"])
    return Engine(mode, names, regions, n_cells, snps=snps, barcodes=barcodes, cell_tag=p["cell_tag"], umi_tag=p["umi_tag"],
                  min_mapq=p["min_mapq"], min_len=p["min_len"], incl_flag=p["incl_flag"], excl_flag=p["excl_flag"],
                  no_orphan=p["no_orphan"], min_include=p["min_include"], flags=flags)


def ingest_all(eng, fx):
    """-> records the ingest calls report (every record of the files, whether its reference is in the contig table or not)"""
    return sum(eng.ingest_bam(fn, sample=i, n_threads=2) for i, fn in enumerate(fx["bam_fns"]))


def check_invariants(rf, st_n_reads):
    """(I1): the classes of a pipeline sum to n_reads, which is xck_stats.n_reads; multi / pairs are consistent with assigned."""
    assert rf["n_reads"] == st_n_reads, (rf, st_n_reads)
    assert sum(rf[k] for k in CLASSES) == rf["n_reads"], rf
    assert all(rf[k] >= 0 for k in FIELDS), rf
    assert rf["multi"] <= rf["assigned"] <= rf["pairs"], rf
    assert rf["pairs"] >= rf["assigned"] + rf["multi"], rf
