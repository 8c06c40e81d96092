"""The opt-in 1-mismatch UMI collapsing of the basefc fold (XCK_F_UMI_COLLAPSE / XCK_UMI_DEDUP=1mm_all) against the model of
tests/umi_dedup_cases.py, which tests/test_umi_dedup_cases_host.py holds against the pinned oracle: the count matrix entry for entry and
the six counters (xck_get_umi_dedup_stats) on the crafted and generated cases with 64- and 128-bit keys; the composition with
XCK_F_UNIQUE_FEATURE; what the flag must leave alone (the BAF half of a fused handle, the read-level numbers); what follows the matrix
(the summaries' marginals, xck_group_counts); the handle's life cycle and the argument checks; the environment knob; fc_wrapper on one
and on two ranks."""
import ctypes as C
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import umi_dedup_cases as UD
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine, XckError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FC, BAF, BOTH, F128 = capi.XCK_MODE_BASEFC, capi.XCK_MODE_BAF, capi.XCK_MODE_BOTH, capi.XCK_F_FORCE_KEY128
KEYS = pytest.mark.parametrize("key_bits", [64, 128], ids=["key64", "key128"])
SUMMARIES = capi.XCK_F_READ_FATE | capi.XCK_F_CELL_SUMMARY | capi.XCK_F_FEATURE_SUMMARY
WORKER = os.path.join(ROOT, "tests", "umi_dedup_worker.py")
MULTIBAM = os.path.join(util.GOLDEN, "datasets", "multibam")


def make(c, umi_dedup="1mm_all", flags=0, mode=FC, snps=(), **kw):
    return Engine(mode, c.names, c.regions, c.n_cells, snps=snps, flags=flags | (F128 if c.key_bits == 128 else 0), umi_dedup=umi_dedup, **dict(UD.KW, **kw))


def feed(eng, c, flush_every=0):
    for i, d in enumerate(c.batches):
        eng.push(UD.batch_of(d)[0])
        if flush_every and i % flush_every == 0:
            eng.flush()
    return eng.finish()


def same(got, exp, what=""):
    for j, col in enumerate(("row", "col", "val")):
        assert np.array_equal(np.asarray(got[j]), exp[j]), "%s: count.%s differs from the model" % (what, col)


@KEYS
@pytest.mark.parametrize("name", UD.ALL)
def test_case_matches_the_model(name, key_bits):
    c, m = UD.case(name, key_bits), UD.case_model(name, key_bits)
    with make(c) as eng:
        got = feed(eng, c, flush_every=3 if name == "repeated" else 0)
        st, us = eng.stats(), eng.umi_dedup_stats()
        print(name, key_bits, us, "nnz", len(got["count"][0]), "n_hits_unique", st["n_hits_unique"], "fold_path", st["fold_path"])
        same(got["count"], m.count, name)
        assert us == m.counters
        if c.literal is not None:
            assert UD.coo_dict(got["count"]) == c.literal[0] and us == c.literal[1]
        assert us["molecules"] == int(np.asarray(got["count"][2]).sum()) and us["groups"] == len(got["count"][0])
        assert (st["key_bits"], st["umi_bits"]) == (key_bits, c.umi_bits)
        assert st["n_hits_unique"] >= us["keys"]                      # the read-level number: keys that reached HBM, repeats included
        if name == "repeated":
            assert st["n_hits_unique"] > us["keys"]                   # the repeats did reach the stage
        if us["keys"]:
            assert st["fold_path"] == 2


@KEYS
@pytest.mark.parametrize("name", UD.WITH_UF + tuple(UD.GENERATED))
def test_unique_feature_runs_first(name, key_bits):
    """XCK_F_UNIQUE_FEATURE | XCK_F_UMI_COLLAPSE: the survivors of the unique-feature rule on exact UMIs are collapsed; both stats calls."""
    import umi_feature_cases as UF
    c, m = UD.case(name, key_bits), UD.case_model(name, key_bits, True)
    with make(c, umi_feature="unique") as eng:
        got = feed(eng, c)
        us, uf = eng.umi_dedup_stats(), eng.umi_feature_stats()
        print(name, key_bits, us, uf)
        same(got["count"], m.count, name)
        assert us == m.counters and uf == UF.model(c).counters
        if c.literal_uf is not None:
            assert UD.coo_dict(got["count"]) == c.literal_uf[0] and us == c.literal_uf[1]
        assert uf["keys"] - uf["keys_dropped"] == us["keys"]          # what the first stage kept is what the second one saw


@KEYS
@pytest.mark.parametrize("umi_dedup", [None, "exact"])
def test_off_is_the_plain_oracle(umi_dedup, key_bits):
    c = UD.case("gen_p3", key_bits)
    with make(c, umi_dedup) as eng:
        got = feed(eng, c)
        same(got["count"], UD.plain_oracle(c), "off")
        assert eng.umi_dedup_stats() is None
        assert eng.stats()["fold_path"] in ((1, 2) if key_bits == 64 else (2,))


@KEYS
def test_fused_handle_collapses_in_its_basefc_half_only(key_bits):
    c = UD.generated("gen_p4", key_bits, with_snps=True)
    m = UD.model(c)
    res = []
    for ud in (None, "1mm_all"):
        with make(c, ud, mode=BOTH, snps=c.snps) as eng:
            res.append(feed(eng, c))
            assert eng.stats()["umi_bits"] == c.umi_bits
            assert (eng.umi_dedup_stats() == m.counters) if ud else (eng.umi_dedup_stats() is None)
    same(res[1]["count"], m.count, "fused")
    same(res[0]["count"], UD.plain_oracle(c), "fused, off")
    assert len(res[0]["dp"][0]) > 0
    for k in ("ad", "dp", "oth"):
        assert all(np.array_equal(a, b) for a, b in zip(res[0][k], res[1][k])), k


@KEYS
def test_read_numbers_stay_and_marginals_follow(key_bits):
    c, m = UD.case("gen_p5", key_bits), UD.case_model("gen_p5", key_bits)
    seen = []
    for ud in (None, "1mm_all"):
        with make(c, ud, flags=SUMMARIES) as eng:
            got = feed(eng, c)
            st = eng.stats()
            seen.append(dict(count=got["count"], fate=eng.read_fate(), cs=eng.cell_summary(), fs=eng.feature_summary(), hits=(st["n_hits"], st["n_hits_unique"])))
    off, on = seen
    assert off["fate"] == on["fate"] and off["hits"] == on["hits"]
    assert np.array_equal(off["cs"]["fate"], on["cs"]["fate"]) and np.array_equal(off["fs"]["reads"], on["fs"]["reads"])
    for s, coo in ((off, UD.plain_oracle(c)), (on, m.count)):
        same(s["count"], coo)
        row, col, val = coo
        cells = np.stack([np.bincount(col, weights=val, minlength=c.n_cells), np.bincount(col, minlength=c.n_cells)], axis=1).astype(np.int64)
        feats = np.stack([np.bincount(row, weights=val, minlength=len(c.regions)), np.bincount(row, minlength=len(c.regions))], axis=1).astype(np.int64)
        assert np.array_equal(s["cs"]["matrix"], cells) and np.array_equal(s["fs"]["matrix"], feats)
    assert not np.array_equal(off["cs"]["matrix"], on["cs"]["matrix"])


@KEYS
def test_group_counts_reset_and_second_finish(key_bits):
    c, m = UD.case("gen_p4", key_bits), UD.case_model("gen_p4", key_bits)
    group = [(i % 5) - 1 for i in range(c.n_cells)]                   # (group -1: left out)
    with make(c) as eng:
        got = feed(eng, c)
        same(got["count"], m.count)
        same(eng.group_counts(group, n_groups=4)["count"], UD.grouped(m.count, group, 4), "group_counts")
        assert eng.umi_dedup_stats() == m.counters                    # (xck_group_counts does not change them)
        eng.reset()
        assert eng.umi_dedup_stats() is None
        same(feed(eng, c)["count"], m.count, "after reset")
        assert eng.umi_dedup_stats() == m.counters


def _stats_rc(eng, size=None, null=False):
    out = capi.UmiDedupStats()
    out.struct_size = C.sizeof(capi.UmiDedupStats) if size is None else size
    return eng.lib.xck_get_umi_dedup_stats(eng.h, None if null else C.byref(out))


def test_interface():
    c = UD.case("chain_abc", 64)
    with make(c, None) as eng:
        assert _stats_rc(eng) == capi.XCK_E_STATE
        feed(eng, c)
        assert _stats_rc(eng) == capi.XCK_E_STATE and b"XCK_F_UMI_COLLAPSE" in eng.lib.xck_last_error(eng.h)
    with make(c) as eng:
        assert _stats_rc(eng) == capi.XCK_E_STATE                     # before a finish
        feed(eng, c)
        assert _stats_rc(eng) == 0 and _stats_rc(eng, size=48) == capi.XCK_E_ARG and _stats_rc(eng, null=True) == capi.XCK_E_ARG
        eng.reset()
        assert _stats_rc(eng) == capi.XCK_E_STATE
        got = eng.finish()                                            # a finish without reads: zeros, an empty matrix
        assert eng.umi_dedup_stats() == dict.fromkeys(capi.UMI_DEDUP_FIELDS, 0) and len(got["count"][0]) == 0
    for kw in (dict(mode=BAF), dict(mode=FC, decode_only=True)):
        with pytest.raises(XckError) as ei:
            Engine(kw.pop("mode"), c.names, c.regions, c.n_cells, umi_dedup="1mm_all", **dict(UD.KW, **kw))
        assert ei.value.code == capi.XCK_E_ARG
    with pytest.raises(ValueError):
        Engine(FC, c.names, c.regions, c.n_cells, umi_dedup="directional", **UD.KW)


def _child(args, knob, **env_more):
    env = dict(os.environ, **env_more)
    env.pop("XCK_UMI_DEDUP", None)
    if knob is not None:
        env["XCK_UMI_DEDUP"] = knob
    return subprocess.run([sys.executable] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=env)


def test_environment_knob(tmp_path):
    """1mm_all: the handle made without the flag counts as with it; exact and an empty value: off; anything else fails xck_create.  A
    BAF-only handle ignores the knob (in this process: the knob is read at xck_create)."""
    c, m = UD.case("staircase", 64), UD.case_model("staircase", 64)
    for knob, exp in (("1mm_all", (m.count, m.counters)), ("exact", (UD.plain_oracle(c), None)), ("", (UD.plain_oracle(c), None)), ("directional", None)):
        dst = str(tmp_path / ("out_%s.json" % (knob or "empty")))
        r = _child([WORKER, "engine", "staircase", "64", dst], knob)
        assert "ENGINE_DONE" in r.stdout, r.stdout[-2000:]
        with open(dst) as fp:
            out = json.load(fp)
        if exp is None:
            assert out["create_failed"] == capi.XCK_E_ARG and "XCK_UMI_DEDUP" in out["error"] and "directional" in out["error"]
            continue
        same([np.array(a, dtype=np.int32) for a in out["count"]], exp[0], "knob " + knob)
        assert out["stats"] == exp[1]
    os.environ["XCK_UMI_DEDUP"] = "1mm_all"
    try:
        with Engine(BAF, c.names, c.regions, c.n_cells, snps=[("1", 50, "A", "C", 0, 1)], **UD.KW) as eng:
            eng.finish()
            assert eng.umi_dedup_stats() is None
    finally:
        del os.environ["XCK_UMI_DEDUP"]


# ----------------------------------------------------------------------------- through a front-end
def _model_files(out_dir):
    """What oracle.run_files does for the basefc run of the worker's `fc` call, with the model in the oracle's place: the BAMs read by
    oracle/pybam.py, encoded by oracle.encode_bam -> the reference-format files in out_dir, the model"""
    import oracle as O
    import pybam
    import umi_consensus_model as UM
    from types import SimpleNamespace
    regions = O.load_regions(os.path.join(MULTIBAM, "regions.tsv"))
    with open(os.path.join(MULTIBAM, "barcodes.tsv")) as fp:
        samples = sorted(x.strip() for x in fp)
    names = O.contig_table(regions)
    umi_bits = O.default_umi_bits(FC, len(regions), 0, len(samples))
    cell_index, intern, batches = {s: i for i, s in enumerate(samples)}, {}, []
    for bi in (0, 1):
        refs, recs = pybam.read_bam(os.path.join(MULTIBAM, "possorted_%d.bam" % bi))
        t2c = O.resolve_contigs([n for n, _ in refs], names)
        batches += [UM.batch_dict(b, keep) for b, keep in O.encode_bam(recs, t2c, bi, cell_index, "CB", "UB", umi_bits, intern, with_seq=False)]
    m = UD.model(SimpleNamespace(names=names, regions=regions, n_cells=len(samples), batches=batches, umi_bits=umi_bits))
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


def test_fc_wrapper_with_and_without_the_knob(tmp_path):
    """fc_wrapper in a child process on the two-contig golden BAMs.  With XCK_UMI_DEDUP=1mm_all its files are the model's, plus
    umi_dedup_summary.tsv with the model's counters, and one log line; two ranks sharing the GPU write the same bytes (their summary
    starts with its `#ranks` line).  Without the knob: the golden bytes and no summary."""
    from xcltk_amd import fc_common as fcc
    regions = os.path.join(MULTIBAM, "regions.tsv")
    one = str(tmp_path / "one")
    r = _child([WORKER, "fc", regions, one], "1mm_all")
    assert "FC_DONE 0" in r.stdout, r.stdout[-2000:]
    assert "UMI collapsing (1mm_all): " in r.stdout and " groups changed" in r.stdout
    m = _model_files(str(tmp_path / "model"))
    print(m.counters)
    want = _files(str(tmp_path / "model"))
    want["umi_dedup_summary.tsv"] = fcc.umi_dedup_summary_text(m.counters).encode()
    got = _files(one)
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], "%s differs from the model's" % f
    # two ranks
    two = str(tmp_path / "two")
    r = _torchrun([WORKER, "fc", regions, two], "1mm_all")
    assert r.stdout.count("FC_DONE 0") == 2, r.stdout[-3000:]
    got2 = _files(two)
    assert sorted(got2) == sorted(got)
    for f in got:
        if f == "umi_dedup_summary.tsv":
            assert got2[f].startswith(b"#ranks=2 cut_contigs=") and got2[f].split(b"\n", 1)[1] == got[f], got2[f]
        else:
            assert got2[f] == got[f], "%s: two ranks differ from one" % f
    # without the knob
    off = str(tmp_path / "off")
    r = _child([WORKER, "fc", regions, off], None)
    assert "FC_DONE 0" in r.stdout and "UMI collapsing" not in r.stdout, r.stdout[-2000:]
    golden = _files(os.path.join(util.GOLDEN, "cases", "multibam_basefc", "expected"))
    assert _files(off) == golden
