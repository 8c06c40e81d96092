"""The opt-in unique-feature molecules of the basefc fold (XCK_F_UNIQUE_FEATURE / XCK_UMI_FEATURE=unique) against the model of
tests/umi_feature_cases.py, which tests/test_umi_feature_cases_host.py holds against the pinned oracle: the count matrix entry for entry
and the four counters (xck_get_umi_feature_stats) on the crafted and generated cases with 64- and 128-bit keys, under both fold knobs;
what the flag must leave alone (the BAF half of a fused handle, the read-level numbers); what follows the matrix (the summaries'
marginals, xck_group_counts); the handle's life cycle and the argument checks; the environment knob; fc_wrapper on one and on two ranks."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import umi_feature_cases as UF
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC, BAF, BOTH, F128 = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF, capi.XCK_MODE_BOTH, capi.XCK_F_FORCE_KEY128
KEYS = pytest.mark.parametrize("key_bits", [64, 128], ids=["key64", "key128"])
FOLDS = pytest.mark.parametrize("fold", ["", "sort"], ids=["default", "sort"])
SUMMARIES = capi.XCK_F_READ_FATE | capi.XCK_F_CELL_SUMMARY | capi.XCK_F_FEATURE_SUMMARY
WORKER = os.path.join(ROOT, "tests", "umi_feature_worker.py")
OVERLAP_REGIONS = os.path.join(util.GOLDEN, "umi_feature", "regions_overlap.tsv")


def make(c, umi_feature="unique", flags=0, mode=FC, snps=(), **kw):
    return Engine(mode, c.names, c.regions, c.n_cells, snps=snps, flags=flags | (F128 if c.key_bits == 128 else 0), umi_feature=umi_feature, **dict(UF.KW, **kw))


def feed(eng, c, flush_every=0):
    for i, d in enumerate(c.batches):
        eng.push(UF.batch_of(d)[0])
        if flush_every and i % flush_every == 0:
            eng.flush()
    return eng.finish()


def same(got, exp, what=""):
    for j, col in enumerate(("row", "col", "val")):
        assert np.array_equal(np.asarray(got[j]), exp[j]), "%s: count.%s differs from the model" % (what, col)


@KEYS
@FOLDS
@pytest.mark.parametrize("name", UF.ALL)
def test_case_matches_the_model(name, key_bits, fold, monkeypatch):
    if fold:
        monkeypatch.setenv("XCK_FOLD", fold)
    c, m = UF.case(name, key_bits), UF.case_model(name, key_bits)
    with make(c) as eng:
        got = feed(eng, c, flush_every=3 if name == "repeated_batches" else 0)
        st, us = eng.stats(), eng.umi_feature_stats()
        print(name, key_bits, fold, us, "nnz", len(got["count"][0]), "n_hits_unique", st["n_hits_unique"], "fold_path", st["fold_path"])
        same(got["count"], m.count, name)
        assert us == m.counters
        assert us["keys"] - us["keys_dropped"] == int(np.asarray(got["count"][2]).sum())
        assert (st["key_bits"], st["umi_bits"]) == (key_bits, c.umi_bits)
        assert st["n_hits_unique"] >= us["keys"]                      # the read-level number: keys that reached HBM, repeats included
        if name in ("tile_run", "repeated_batches"):
            assert st["n_hits_unique"] > us["keys"]                   # the repeats did reach the stage
        if us["keys"]:
            assert st["fold_path"] == 2                               # the survivors are counted by the radix-sort fold


@KEYS
@pytest.mark.parametrize("umi_feature", [None, "all"])
def test_off_is_the_plain_oracle(umi_feature, key_bits):
    c = UF.case("gen_s1", key_bits)
    with make(c, umi_feature) as eng:
        got = feed(eng, c)
        same(got["count"], UF.plain_oracle(c), "off")
        assert eng.umi_feature_stats() is None
        assert eng.stats()["fold_path"] in ((1, 2) if key_bits == 64 else (2,))


@KEYS
def test_fused_handle_drops_in_its_basefc_half_only(key_bits):
    c = UF.generated("gen_s2", key_bits, with_snps=True)
    m = UF.model(c)
    res = []
    for uf in (None, "unique"):
        with make(c, uf, mode=BOTH, snps=c.snps) as eng:
            res.append(feed(eng, c))
            assert (eng.umi_feature_stats() == m.counters) if uf else (eng.umi_feature_stats() is None)
    same(res[1]["count"], m.count, "fused")
    same(res[0]["count"], UF.plain_oracle(c), "fused, off")
    assert len(res[0]["dp"][0]) > 0
    for k in ("ad", "dp", "oth"):
        assert all(np.array_equal(a, b) for a, b in zip(res[0][k], res[1][k])), k


@KEYS
def test_read_numbers_stay_and_marginals_follow(key_bits):
    c, m = UF.case("gen_s3", key_bits), UF.case_model("gen_s3", key_bits)
    seen = []
    for uf in (None, "unique"):
        with make(c, uf, flags=SUMMARIES) as eng:
            got = feed(eng, c)
            st = eng.stats()
            seen.append(dict(count=got["count"], fate=eng.read_fate(), cs=eng.cell_summary(), fs=eng.feature_summary(), hits=(st["n_hits"], st["n_hits_unique"])))
    off, on = seen
    assert off["fate"] == on["fate"] and off["hits"] == on["hits"] and off["fate"]["multi"] > 0
    assert np.array_equal(off["cs"]["fate"], on["cs"]["fate"]) and np.array_equal(off["fs"]["reads"], on["fs"]["reads"])
    for s, coo in ((off, UF.plain_oracle(c)), (on, m.count)):
        same(s["count"], coo)
        row, col, val = coo
        cells = np.stack([np.bincount(col, weights=val, minlength=c.n_cells), np.bincount(col, minlength=c.n_cells)], axis=1).astype(np.int64)
        feats = np.stack([np.bincount(row, weights=val, minlength=len(c.regions)), np.bincount(row, minlength=len(c.regions))], axis=1).astype(np.int64)
        assert np.array_equal(s["cs"]["matrix"], cells) and np.array_equal(s["fs"]["matrix"], feats)
    assert not np.array_equal(off["cs"]["matrix"], on["cs"]["matrix"])


@KEYS
def test_group_counts_reset_and_second_finish(key_bits):
    c, m = UF.case("gen_s4", key_bits), UF.case_model("gen_s4", key_bits)
    group = [(i % 5) - 1 for i in range(c.n_cells)]                   # (group -1: left out)
    with make(c) as eng:
        got = feed(eng, c)
        same(got["count"], m.count)
        same(eng.group_counts(group, n_groups=4)["count"], UF.grouped(m.count, group, 4), "group_counts")
        again = eng.finish()                                          # a second finish: the same blocks
        same(again["count"], m.count, "second finish")
        assert eng.umi_feature_stats() == m.counters
        ptr, nnz = eng.result_device()["count"]
        assert nnz == len(m.count[0]) and ptr
        import torch
        from xcltk_amd import shard
        dev = torch.as_tensor(shard._DevArray(ptr, 3 * nnz), device="cuda:0").cpu().numpy()
        same((dev[:nnz], dev[nnz:2 * nnz], dev[2 * nnz:]), m.count, "get_result_device")
        eng.reset()
        assert eng.umi_feature_stats() is None
        same(feed(eng, c)["count"], m.count, "after reset")
        assert eng.umi_feature_stats() == m.counters


def _stats_rc(eng, size=None, null=False):
    out = capi.UmiFeatureStats()
    out.struct_size = C.sizeof(capi.UmiFeatureStats) if size is None else size
    return eng.lib.xck_get_umi_feature_stats(eng.h, None if null else C.byref(out))


def test_interface():
    c = UF.case("three_rows", 64)
    with make(c, None) as eng:
        assert _stats_rc(eng) == capi.XCK_E_STATE
        feed(eng, c)
        assert _stats_rc(eng) == capi.XCK_E_STATE and b"XCK_F_UNIQUE_FEATURE" in eng.lib.xck_last_error(eng.h)
    with make(c) as eng:
        assert _stats_rc(eng) == capi.XCK_E_STATE                     # before a finish
        feed(eng, c)
        assert _stats_rc(eng) == 0 and _stats_rc(eng, size=32) == capi.XCK_E_ARG and _stats_rc(eng, null=True) == capi.XCK_E_ARG
        eng.reset()
        assert _stats_rc(eng) == capi.XCK_E_STATE
        got = eng.finish()                                            # a finish without reads: zeros, an empty matrix
        assert eng.umi_feature_stats() == dict.fromkeys(capi.UMI_FEATURE_FIELDS, 0) and len(got["count"][0]) == 0
    for kw in (dict(mode=BAF), dict(mode=FC, decode_only=True)):
        with pytest.raises(XckError) as ei:
            Engine(kw.pop("mode"), c.names, c.regions, c.n_cells, umi_feature="unique", **dict(UF.KW, **kw))
        assert ei.value.code == capi.XCK_E_ARG
    with pytest.raises(ValueError):
        Engine(FC, c.names, c.regions, c.n_cells, umi_feature="plurality", **UF.KW)


def _child(args, knob, **env_more):
    env = dict(os.environ, **env_more)
    env.pop("XCK_UMI_FEATURE", None)
    if knob is not None:
        env["XCK_UMI_FEATURE"] = knob
    return subprocess.run([sys.executable] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)


def test_environment_knob(tmp_path):
    """unique: the handle made without the flag counts as with it; all and an empty value: off; anything else fails xck_create.  A
    BAF-only handle ignores the knob (in this process: the knob is read at xck_create)."""
    c, m = UF.case("shuffled_order", 64), UF.case_model("shuffled_order", 64)
    for knob, exp in (("unique", (m.count, m.counters)), ("all", (UF.plain_oracle(c), None)), ("", (UF.plain_oracle(c), None)), ("first", None)):
        dst = str(tmp_path / ("out_%s.json" % (knob or "empty")))
        r = _child([WORKER, "engine", "shuffled_order", "64", dst], knob)
        assert "ENGINE_DONE" in r.stdout, r.stdout[-2000:]
        with open(dst) as fp:
            out = json.load(fp)
        if exp is None:
            assert out["create_failed"] == capi.XCK_E_ARG and "XCK_UMI_FEATURE" in out["error"] and "first" in out["error"]
            continue
        same([np.array(a, dtype=np.int32) for a in out["count"]], exp[0], "knob " + knob)
        assert out["stats"] == exp[1]
    os.environ["XCK_UMI_FEATURE"] = "unique"
    try:
        with Engine(BAF, c.names, c.regions, c.n_cells, snps=[("1", 50, "A", "C", 0, 1)], **UF.KW) as eng:
            eng.finish()
            assert eng.umi_feature_stats() is None
    finally:
        del os.environ["XCK_UMI_FEATURE"]


# ----------------------------------------------------------------------------- through a front-end
def _model_files(out_dir):
    """What oracle.run_files does for the basefc run of the worker's `fc` call, with the model in the oracle's place: the BAMs read by
    oracle/pybam.py, encoded by oracle.encode_bam -> the reference-format files in out_dir, the counters"""
    import oracle as O
    import pybam
    import umi_consensus_model as UM
    from types import SimpleNamespace
    D = os.path.join(util.GOLDEN, "datasets", "multibam")
    regions = O.load_regions(OVERLAP_REGIONS)
    with open(os.path.join(D, "barcodes.tsv")) as fp:
        samples = sorted(x.strip() for x in fp)
    names = O.contig_table(regions)
    umi_bits = O.default_umi_bits(FC, len(regions), 0, len(samples))
    cell_index, intern, batches = {s: i for i, s in enumerate(samples)}, {}, []
    for bi in (0, 1):
        refs, recs = pybam.read_bam(os.path.join(D, "possorted_%d.bam" % bi))
        t2c = O.resolve_contigs([n for n, _ in refs], names)
        batches += [UM.batch_dict(b, keep) for b, keep in O.encode_bam(recs, t2c, bi, cell_index, "CB", "UB", umi_bits, intern, with_seq=False)]
    m = UF.model(SimpleNamespace(names=names, regions=regions, n_cells=len(samples), batches=batches))
    O.write_outputs(FC, out_dir, regions, [], samples, {"count": m.count}, True)
    return m


def _files(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if not f.startswith(".")}


def _torchrun(args, knob):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = str(sk.getsockname()[1])
    return _child(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", port] + args, knob,
                  XCK_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", XCK_DIST_GATHER="0", XCK_DEVICE="0")


def test_fc_wrapper_with_the_knob(tmp_path):
    """fc_wrapper in a child process with XCK_UMI_FEATURE=unique on the two-contig golden BAMs and a region file with overlapping rows:
    its files are the model's, plus umi_feature_summary.tsv with the model's counters; two ranks sharing the GPU, one contig each,
    write the same bytes (their summary starts with its `#ranks` line); a plan that gives each rank a piece of one contig is refused
    before the ingest, the message naming the knob and the contig."""
    from xcltk_amd import fc_common as fcc
    one = str(tmp_path / "one")
    r = _child([WORKER, "fc", OVERLAP_REGIONS, one], "unique")
    assert "FC_DONE 0" in r.stdout, r.stdout[-2000:]
    assert "unique-feature molecules: " in r.stdout and " molecules on two or more features dropped" in r.stdout
    m = _model_files(str(tmp_path / "model"))
    print(m.counters)
    want = _files(str(tmp_path / "model"))
    want["umi_feature_summary.tsv"] = fcc.umi_feature_summary_text(m.counters).encode()
    got = _files(one)
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], "%s differs from the model's" % f
    assert m.counters["multi_feature"] > 0 and m.counters["keys"] > m.counters["keys_dropped"]
    # two ranks
    two = str(tmp_path / "two")
    r = _torchrun([WORKER, "fc", OVERLAP_REGIONS, two], "unique")
    assert r.stdout.count("FC_DONE 0") == 2, r.stdout[-3000:]
    got2 = _files(two)
    assert sorted(got2) == sorted(got)
    for f in got:
        if f == "umi_feature_summary.tsv":
            assert got2[f].startswith(b"#ranks=2 cut_contigs=") and got2[f].split(b"\n", 1)[1] == got[f], got2[f]
        else:
            assert got2[f] == got[f], "%s: two ranks differ from one" % f
    # one contig over two ranks
    cut = str(tmp_path / "cut")
    r = _torchrun([WORKER, "fc_cut", os.path.join(util.GOLDEN, "datasets", "c1", "regions.tsv"), cut], "unique")
    assert r.stdout.count("FC_DONE -1") == 2, r.stdout[-3000:]
    assert "XCK_UMI_FEATURE=unique: the multi-GPU plan cuts contig 1 over ranks" in r.stdout
    assert "decoded and joined" not in r.stdout and not os.path.exists(os.path.join(cut, "matrix.mtx"))
