"""The opt-in UMI consensus allele of the pileup fold (XCK_F_UMI_CONSENSUS / XCK_UMI_CONSENSUS=1) against the plain-Python model of
tests/umi_consensus_model.py, which tests/test_umi_consensus_model_host.py holds against the pinned oracle under the default rule:
matrices, the per-SNP tallies (xck_get_feature_summary) and the five agreement counters (xck_get_molecule_stats), on crafted run
shapes and run lengths through both key widths and both sorts, on the derived calls, on deep fuzz inputs and through afc_wrapper."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import umi_consensus_model as UM
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAF, F128 = capi.XCK_MODE_BAF, capi.XCK_F_FORCE_KEY128
MATS = ("ad", "dp", "oth")
KEYS = pytest.mark.parametrize("flags", [0, F128], ids=["key64", "key128"])
SORTS = pytest.mark.parametrize("sort", ["", "radix"], ids=["partition", "radix"])


def make(c, consensus=True, flags=0, mode=BAF):
    f = dict(UM.FILT); f.update(c.filt)
    return Engine(mode, c.names, c.regions, c.n_cells, snps=c.snps, flags=flags | capi.XCK_F_FEATURE_SUMMARY, umi_consensus=consensus, **f)


def feed(eng, c):
    for d in c.batches:
        eng.push(util.batch_from_dict(d)[0])
    return eng.finish()


def same(got, m, what=""):
    for k in MATS:
        for j, col in enumerate(("row", "col", "val")):
            e = getattr(m, k)[j] if not isinstance(m, dict) else m[k][j]
            assert np.array_equal(np.asarray(got[k][j]), e), "%s %s.%s differs from the model" % (what, k, col)


def check(eng, got, m, what=""):
    same(got, m, what)
    assert np.array_equal(eng.feature_summary(BAF)["snp"][:, 1:6], m.tally), "%s: the per-SNP tallies differ from the model" % what
    assert eng.molecule_stats() == m.counters, what


@KEYS
@SORTS
@pytest.mark.parametrize("name", ["shapes", "single", "walk", "long", "deep"])
def test_case_matches_the_model(name, flags, sort, monkeypatch):
    if sort:
        monkeypatch.setenv("XCK_PILEUP_SORT", sort)
    c = UM.case(name)
    m = UM.model(c.names, c.regions, c.snps, c.batches, c.filt, "consensus")
    with make(c, True, flags) as eng:
        got = feed(eng, c)
        st = eng.stats()
        print(name, flags, sort, eng.molecule_stats(), "sort path", st["pileup_sort_path"], "nnz", [len(got[k][0]) for k in MATS])
        check(eng, got, m, name)
        assert sum(len(got[k][0]) for k in MATS) > 0
        if name == "deep":                                   # one (SNP, cell) deeper than a work item: the radix sort takes over unforced
            assert st["pileup_sort_path"] == 2
        elif not flags:
            assert st["pileup_sort_path"] == (2 if sort else 1)


@KEYS
@SORTS
def test_acc_is_a_where_the_default_rules_and_c_under_consensus(flags, sort, monkeypatch):
    """reads A, C, C of one molecule, the A earliest: the default answers A, the vote C, and one molecule has changed"""
    if sort:
        monkeypatch.setenv("XCK_PILEUP_SORT", sort)
    c = UM.case("acc")
    with make(c, False, flags) as eng:
        got = feed(eng, c)
        assert eng.feature_summary(BAF)["snp"][0, 1:6].tolist() == [1, 0, 0, 0, 0] and eng.molecule_stats() is None
        same(got, UM.model(c.names, c.regions, c.snps, c.batches, c.filt, "first"), "default")
        assert len(got["ad"][0]) == 0 and got["dp"][2].tolist() == [1, 1, 1]          # (its own region, first20, all)
    with make(c, True, flags) as eng:
        got = feed(eng, c)
        assert eng.feature_summary(BAF)["snp"][0, 1:6].tolist() == [0, 1, 0, 0, 0]
        assert eng.molecule_stats() == dict(molecules=1, multi_read=1, discordant=1, tied=0, changed=1)
        assert got["ad"][2].tolist() == [1, 1, 1] and got["dp"][2].tolist() == [1, 1, 1]


@KEYS
def test_gap_read_first_silences_under_the_default_and_abstains_under_consensus(flags):
    c = UM.case("shapes")
    tallies = []
    for consensus, rule in ((False, "first"), (True, "consensus")):
        m = UM.model(c.names, c.regions, c.snps, c.batches, c.filt, rule)
        with make(c, consensus, flags) as eng:
            got = feed(eng, c)
            same(got, m, rule)
            t = eng.feature_summary(BAF)["snp"][:, 1:6]
            assert np.array_equal(t, m.tally), rule
            tallies.append(t)
    for k in (7, 9):                                            # gap read (N, D) first, then C
        assert tallies[0][k].sum() == 0 and tallies[1][k].tolist() == [0, 1, 0, 0, 0]
    assert tallies[0][8].sum() == 0 and tallies[1][8].sum() == 0   # gap reads only


@KEYS
def test_derived_calls_follow_the_rule(flags):
    c = UM.case("shapes")
    mols, _ = UM.molecules(c.names, c.snps, c.batches, c.filt)
    m = UM.fold(c.names, c.regions, c.snps, c.filt, mols, "consensus")
    with make(c, True, flags) as eng:
        check(eng, feed(eng, c), m)
        same(eng.snp_counts(), UM.snp_counts(c.snps, m.allele), "snp_counts")
        group = [0, 1, 0]
        g = eng.group_counts(group, source="result")
        same(g, {k: UM.group_sum(getattr(m, k), group) for k in MATS}, "group_counts")
        g = eng.group_counts(group, source="snp")
        same(g, {k: UM.group_sum(UM.snp_counts(c.snps, m.allele)[k], group) for k in MATS}, "group_counts snp")
        m2 = UM.fold(c.names, UM.REGIONS2, c.snps, c.filt, mols, "consensus")
        same(eng.refold(UM.REGIONS2), m2, "refold")
        assert np.array_equal(eng.feature_summary(BAF)["snp"][:, 1:6], m2.tally)
        mask = [False, True, True]                              # cell 0 holds the molecule A, C, C
        f3 = dict(c.filt, min_count=2)
        m3 = UM.fold(c.names, UM.REGIONS2, c.snps, f3, mols, "consensus", cell_enabled=mask)
        same(eng.refold(UM.REGIONS2, min_count=2, cell_enabled=mask), m3, "refold cells")
        assert np.array_equal(eng.feature_summary(BAF)["snp"][:, 1:6], m3.tally) and m3.tally[0].sum() == 0
        assert eng.molecule_stats() == m.counters               # the counters are the finish's
        eng.reset()
        assert eng.molecule_stats() is None
        # (the handle's regions and filters follow its last refold; a finish counts every cell)
        check(eng, feed(eng, c), UM.fold(c.names, UM.REGIONS2, c.snps, f3, mols, "consensus"), "after reset")


def _stats_rc(eng, size=None, null=False):
    out = capi.MoleculeStats()
    out.struct_size = C.sizeof(capi.MoleculeStats) if size is None else size
    return eng.lib.xck_get_molecule_stats(eng.h, None if null else C.byref(out))


def test_interface():
    c = UM.case("acc")
    with make(c, False) as eng:
        assert _stats_rc(eng) == capi.XCK_E_STATE
        feed(eng, c)
        assert _stats_rc(eng) == capi.XCK_E_STATE and b"XCK_F_UMI_CONSENSUS" in eng.lib.xck_last_error(eng.h)
    with make(c, True) as eng:
        assert _stats_rc(eng) == capi.XCK_E_STATE               # before a finish
        feed(eng, c)
        assert _stats_rc(eng) == 0 and _stats_rc(eng, size=40) == capi.XCK_E_ARG and _stats_rc(eng, null=True) == capi.XCK_E_ARG
        eng.reset()
        assert _stats_rc(eng) == capi.XCK_E_STATE
        eng.finish()                                            # a finish without reads: zeros
        assert eng.molecule_stats() == dict.fromkeys(UM.COUNTERS, 0)
    f = dict(UM.FILT)
    for kw in (dict(mode=capi.XCK_MODE_BASEFC), dict(mode=BAF, decode_only=True)):
        with pytest.raises(XckError) as ei:
            Engine(kw.pop("mode"), c.names, c.regions, c.n_cells, snps=c.snps, umi_consensus=True, **dict(f, **kw))
        assert ei.value.code == capi.XCK_E_ARG


def test_fused_handle_votes_in_its_baf_half_only():
    c = UM.case("shapes")
    m = UM.model(c.names, c.regions, c.snps, c.batches, c.filt, "consensus")
    res = []
    for consensus in (False, True):
        with make(c, consensus, mode=capi.XCK_MODE_BOTH) as eng:
            res.append(feed(eng, c))
            assert (eng.molecule_stats() == m.counters) if consensus else (eng.molecule_stats() is None)
    same(res[1], m, "fused")
    assert len(res[0]["count"][0]) > 0 and all(np.array_equal(a, b) for a, b in zip(res[0]["count"], res[1]["count"]))
    assert not all(np.array_equal(a, b) for a, b in zip(res[0]["ad"], res[1]["ad"]))


def _child(args, knob, tmp_path, **env_more):
    env = dict(os.environ, **env_more)
    env.pop("XCK_UMI_CONSENSUS", None)
    if knob:
        env["XCK_UMI_CONSENSUS"] = "1"
    r = subprocess.run([sys.executable] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)
    return r


def test_environment_knob_equals_the_flag(tmp_path):
    c = UM.case("shapes")
    m = UM.model(c.names, c.regions, c.snps, c.batches, c.filt, "consensus")
    dst = str(tmp_path / "out.json")
    r = _child([os.path.join(ROOT, "tests", "umi_consensus_worker.py"), "engine", "shapes", dst], True, tmp_path)
    assert "ENGINE_DONE" in r.stdout, r.stdout[-2000:]
    with open(dst) as fp:
        out = json.load(fp)
    same({k: [np.array(a, dtype=np.int32) for a in out[k]] for k in MATS}, m, "knob")
    assert out["stats"] == m.counters and out["tally"] == m.tally.tolist()


@pytest.mark.parametrize("seed", UM.FUZZ_SEEDS)
def test_fuzz_matches_the_model(seed):
    c = UM.fuzz_case(seed)
    m = UM.model(c.names, c.regions, c.snps, c.batches, c.filt, "consensus")
    with make(c, True, c.flags) as eng:
        got = feed(eng, c)
        print(seed, eng.molecule_stats(), "nnz", [len(got[k][0]) for k in MATS])
        check(eng, got, m, "seed %d" % seed)


# ----------------------------------------------------------------------------- through a front-end
GOLDEN_CASE = "special_baf"


def _model_files(case, out_dir):
    """what oracle.run_files does for a BAF case, with the model under the consensus rule in the oracle's place: the BAMs read by
    oracle/pybam.py, encoded by oracle.encode_bam -> the reference-format files in out_dir, the counters"""
    import oracle as O
    import pybam
    p = util.oracle_params(case)
    assert p.pop("mode") == BAF and "phase" not in p
    regions, snps = O.load_regions(p["region_fn"]), O.load_snps(p["snp_fn"])
    with open(p["barcode_fn"]) as fp:
        samples = sorted(x.strip() for x in fp)
    excl = p["excl_flag"] if p["excl_flag"] is not None and p["excl_flag"] >= 0 else (772 if p["umi_tag"] else 1796)
    names = O.contig_table(regions, snps)
    umi_bits = O.default_umi_bits(BAF, len(regions), len(snps), len(samples))
    cell_index, intern, batches = {s: i for i, s in enumerate(samples)}, {}, []
    for bi, fn in enumerate(p["bam_fns"]):
        refs, recs = pybam.read_bam(fn)
        t2c = O.resolve_contigs([n for n, _ in refs], names)
        batches += [UM.batch_dict(b, keep) for b, keep in O.encode_bam(recs, t2c, bi, cell_index, p["cell_tag"], p["umi_tag"], umi_bits, intern)]
    filt = dict(min_mapq=p["min_mapq"], min_len=p["min_len"], incl_flag=p["incl_flag"], excl_flag=excl, no_orphan=p["no_orphan"],
                min_count=p["min_count"], min_maf=p["min_maf"], no_dup_hap=p["no_dup_hap"])
    m = UM.model(names, regions, snps, batches, filt, "consensus")
    O.write_outputs(BAF, out_dir, regions, snps, samples, {k: getattr(m, k) for k in MATS}, p["output_all_reg"])
    return m.counters


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if not f.startswith(".")}


def test_afc_wrapper_with_the_knob(tmp_path):
    """afc_wrapper in a child process with XCK_UMI_CONSENSUS=1: its files are the model's, molecule_summary.tsv holds the model's
    counters; without the knob the same call still writes the committed golden bytes; two ranks on the one GPU (the existing
    tests/dist_worker.py, which ends by comparing with the golden directory and so reports a mismatch here: the extra file and the
    other rule - its files are compared with the one-rank files instead) write what one rank writes."""
    from xcltk_amd import fc_common as fcc
    worker = os.path.join(ROOT, "tests", "umi_consensus_worker.py")
    one = tmp_path / "one"; one.mkdir()
    r = _child([worker, "afc", GOLDEN_CASE, str(one)], True, tmp_path)
    assert "AFC_DONE" in r.stdout, r.stdout[-2000:]
    assert "UMI consensus: " in r.stdout
    got = _files(os.path.join(str(one), "out_" + GOLDEN_CASE))
    (tmp_path / "m").mkdir()
    case, _, _, exp_dir = util.load_case(GOLDEN_CASE, str(tmp_path / "m"))
    counters = _model_files(case, str(tmp_path / "model"))
    print(GOLDEN_CASE, counters)
    want = _files(str(tmp_path / "model"))
    want["xcltk.molecule_summary.tsv"] = fcc.molecule_summary_text(counters).encode()
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], "%s differs from the model's" % f
    assert counters["molecules"] > 0
    # without the knob: the golden bytes
    off = tmp_path / "off"; off.mkdir()
    r = _child([worker, "afc", GOLDEN_CASE, str(off)], False, tmp_path)
    assert "AFC_DONE" in r.stdout, r.stdout[-2000:]
    util.assert_dirs_equal(os.path.join(str(off), "out_" + GOLDEN_CASE), exp_dir)
    # two ranks sharing the GPU, with the knob
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    two = tmp_path / "two"; two.mkdir()
    r = _child(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", port,
                os.path.join(ROOT, "tests", "dist_worker.py"), GOLDEN_CASE, str(two)], True, tmp_path,
               XCK_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", XCK_DIST_GATHER="0", XCK_DEVICE="0")
    got2 = _files(os.path.join(str(two), "out_" + GOLDEN_CASE))
    assert sorted(got2) == sorted(got), r.stdout[-2000:]
    for f in got:
        if f == "xcltk.molecule_summary.tsv":                   # (the two-rank file starts with its `#ranks` line)
            assert got2[f].startswith(b"#ranks=2 cut_contigs=") and got2[f].split(b"\n", 1)[1] == got[f], got2[f]
        else:
            assert got2[f] == got[f], "%s: two ranks differ from one" % f
