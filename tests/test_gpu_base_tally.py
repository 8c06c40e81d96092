"""The opt-in pseudo-bulk base tallies and candidate calls (XCK_F_BASE_TALLY, include/xck.h) through the engine,
against the model of tests/base_tally_cases.py, which tests/test_base_tally_cases_host.py holds against a walk through oracle/pybam.py.
Tallies are read through xck_get_base_tally over the whole tiny contig; counters and candidates are the model's, with 64-bit and
XCK_F_FORCE_KEY128 handles."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import base_tally_cases as BT
import baseq_cases as B
import util
from xcltk_amd import capi
from xcltk_amd.baf import discover
from xcltk_amd.baf.genotype import load_candidate_snps
from xcltk_amd.engine import Engine, XckError

pytestmark = pytest.mark.gpu
BAF = capi.XCK_MODE_BAF
KNOBS = ("XCK_MIN_BASEQ", "XCK_UMI_CONSENSUS", "XCK_GPU_INFLATE", "XCK_GPU_INFLATE_MIN_MB", "XCK_GPU_PARSE", "XCK_GPU_NAMES", "XCK_CHUNK_BYTES", "XCK_HIT_CAP0",
         "XCK_HIT_SLACK", "XCK_TAG_FILTER", "XCK_READ_FATE", "XCK_CELL_SUMMARY", "XCK_FEATURE_SUMMARY", "XCK_CELL_GROUPS", "WORLD_SIZE", "XCK_DIST_FORCE")
THRESHOLDS = ((1, 0), (2, 0.2))


def make(c, flags=0, regions=(), snps=(), tally=True, lens=True, **kw):
    f = dict(BT.FILT); f.update(c.filt); f.update(kw)
    return Engine(BAF, c.names, list(regions), c.n_cells, snps=list(snps), flags=c.flags | flags, min_baseq=c.q, base_tally=tally,
                  contig_len=c.lens if tally and lens else None, **f)


def feed(eng, c, device=False):
    keep = []
    for d, qual in zip(c.batches, c.quals):
        if device:
            import torch
            b = capi.Batch()
            b.contig, b.n_reads, b.ordinal_base = d["contig"], len(d["pos"]), d["ordinal_base"]
            for k, ct in (("pos", C.c_int32), ("flag", C.c_uint16), ("mapq", C.c_uint8), ("cell", C.c_int32), ("umi", C.c_uint64),
                          ("cig_off", C.c_uint32), ("cigar", C.c_uint32), ("seq_off", C.c_uint32), ("seq", C.c_uint8)):
                a = np.ascontiguousarray(d[k])
                t = torch.from_numpy(a.view(np.uint8) if a.size else np.zeros(8, dtype=np.uint8)).to("cuda:0")
                keep.append(t)
                setattr(b, k, C.cast(t.data_ptr(), C.POINTER(ct)))
            eng.push(b, device_resident=True)
        else:
            b, k = util.batch_from_dict(d)
            keep.append(k)
            if c.q:
                eng.push_batch(b, qual=qual)
            else:
                eng.push(b)
    return keep


def check_tallies(eng, c, m, what=""):
    for k, n in enumerate(c.lens):
        got = eng.base_tally(k, 0, n)
        assert got.shape == (n, 4) and np.array_equal(got, m.tally[k]), "%s: the tallies of contig %d differ from the model (%d vs %d bases)" % (what, k, got.sum(), m.tally[k].sum())
    assert eng.base_tally_stats() == m.stats, what


def check_candidates(eng, m, what=""):
    for mc, mf in THRESHOLDS:                                             # (twice, with different thresholds)
        got, want = eng.find_candidates(mc, mf), BT.candidates(m.tally, mc, mf)
        assert got["positions_covered"] == want["positions_covered"], what
        for k in ("contig", "pos", "ref", "alt", "count"):
            assert np.array_equal(got[k], want[k]), "%s: candidates.%s at (%s, %s)" % (what, k, mc, mf)


@pytest.mark.parametrize("flags", [0, capi.XCK_F_FORCE_KEY128], ids=["k64", "k128"])
@pytest.mark.parametrize("name", BT.CASES)
def test_case_matches_the_model(name, flags):
    c, m = BT.case(name), BT.expected(name)
    with make(c, flags) as eng:
        keep = feed(eng, c)
        check_tallies(eng, c, m, name)                                    # (before finish: the getter waits for the queued work)
        res = eng.finish()
        assert all(len(res[k][0]) == 0 for k in ("ad", "dp", "oth")) and eng.stats()["n_reads"] == sum(len(g) for g in c.groups)
        print(name, eng.base_tally_stats(), "launches", eng.stats()["n_join_launches"])
        check_tallies(eng, c, m, name + " after finish")
        check_candidates(eng, m, name)
        # reset, the same input again: the same answer (tables zeroed, lengths kept)
        eng.reset()
        assert eng.base_tally_stats() == dict.fromkeys(BT.STATS, 0) and int(eng.base_tally(0, 0, c.lens[0]).sum()) == 0
        keep = feed(eng, c)
        eng.finish()
        check_tallies(eng, c, m, name + " after reset")
        check_candidates(eng, m, name + " after reset")


@pytest.mark.parametrize("name", ["two_contigs", "far_exon", "tile_p1"])
def test_device_resident_batches(name):
    c, m = BT.case(name), BT.expected(name)
    with make(c) as eng:
        keep = feed(eng, c, device=True)
        eng.finish()
        check_tallies(eng, c, m, name)
        check_candidates(eng, m, name)


@pytest.mark.parametrize("stage", ["0", "1"])
@pytest.mark.parametrize("name", ["two_contigs", "shared", "far_exon", "baseq"])
def test_both_host_push_forms(name, stage, monkeypatch):
    """XCK_PUSH_STAGE=0: the caller's arrays copied column by column into a batch slot; 1: packed into one block and staged, as the
    decoder's chunks are (the default takes the staged form for batches this small)"""
    monkeypatch.setenv("XCK_PUSH_STAGE", stage)
    c, m = BT.case(name), BT.expected(name)
    with make(c) as eng:
        keep = feed(eng, c)
        eng.finish()
        check_tallies(eng, c, m, "%s stage %s" % (name, stage))
        check_candidates(eng, m, name)


def test_untouched_contig_reads_as_zeros_and_ranges_are_checked():
    c = BT.case("one")
    with Engine(BAF, ["1", "2"], [], c.n_cells, snps=[], base_tally=True, contig_len=[c.lens[0], 50], **BT.FILT) as eng:
        keep = feed(eng, c)
        assert int(eng.base_tally(1, 0, 50).sum()) == 0 and eng.base_tally("1", 100, 10).sum() == 10
        out = (C.c_uint32 * 8)()
        for args in ((2, 0, 1), (0, -1, 1), (1, 49, 2), (0, 0, -1)):
            assert eng.lib.xck_get_base_tally(eng.h, *args, out) == capi.XCK_E_ARG, args
        st = capi.BaseTallyStats(); st.struct_size = 8
        assert eng.lib.xck_get_base_tally_stats(eng.h, C.byref(st)) == capi.XCK_E_ARG


# ----------------------------------------------------------------------------- beside SNPs and regions
@pytest.mark.parametrize("name", ["paths", "offsets", "contigs"])
def test_handle_with_snps_and_regions(name):
    """a handle that also has SNPs and regions: AD / DP / OTH byte for byte those of the same handle without the flag, tallies those of the
    zero-SNP handle (and of the model)"""
    bc = B.case(name)
    lens = [20000] * len(bc.names)
    c = type(bc)(**dict(vars(bc), lens=lens, q=0, groups=bc.reads))
    m = BT.model(c.batches, None, lens, c.filt)
    res = {}
    for tally in (False, True):
        with make(c, regions=bc.regions, snps=bc.snps, tally=tally) as eng:
            keep = feed(eng, c)
            res[tally] = eng.finish()
            if tally:
                check_tallies(eng, c, m, name + " with SNPs")
                check_candidates(eng, m, name + " with SNPs")
            else:
                assert eng.base_tally_stats() is None
    assert sum(len(res[False][k][0]) for k in ("ad", "dp", "oth")) > 0
    for k in ("ad", "dp", "oth"):
        for a, b in zip(res[False][k], res[True][k]):
            assert a.tobytes() == b.tobytes(), k
    with make(c) as eng:                                                 # no SNP anywhere
        keep = feed(eng, c)
        eng.finish()
        check_tallies(eng, c, m, name + " zero-SNP")


def test_fused_handle_tallies_in_its_baf_half():
    bc = B.case("paths")
    lens = [20000]
    c = type(bc)(**dict(vars(bc), lens=lens, q=0, groups=bc.reads))
    m = BT.model(c.batches, None, lens, c.filt)
    res = {}
    for tally in (False, True):
        f = dict(BT.FILT); f.update(c.filt, min_include=0)
        with Engine(capi.XCK_MODE_BOTH, c.names, bc.regions, c.n_cells, snps=bc.snps, base_tally=tally, contig_len=lens if tally else None, **f) as eng:
            keep = feed(eng, c)
            res[tally] = eng.finish()
            if tally:
                check_tallies(eng, c, m, "fused")
    for k in ("count", "ad", "dp", "oth"):
        assert len(res[False]["count"][0]) > 0 and all(a.tobytes() == b.tobytes() for a, b in zip(res[False][k], res[True][k])), k


# ----------------------------------------------------------------------------- the floor
@pytest.mark.parametrize("name", ["lengths", "stored", "offsets"])
def test_base_quality_floor_through_push_batch_q(name):
    """the cases of tests/baseq_cases.py under their floor: bases_masked is the model's, 0xff qualities are kept"""
    bc = B.case(name)
    lens = [20000] * len(bc.names)
    c = type(bc)(**dict(vars(bc), lens=lens, groups=bc.reads))
    m, m0 = BT.model(c.batches, c.quals, lens, c.filt, c.q), BT.model(c.batches, None, lens, c.filt)
    assert m.stats["bases_masked"] > 0 and m.stats["bases_masked"] + m.stats["bases_tallied"] + m.stats["bases_other"] == m0.stats["bases_tallied"] + m0.stats["bases_other"]
    with make(c) as eng:
        keep = feed(eng, c)
        eng.finish()
        check_tallies(eng, c, m, name)
        check_candidates(eng, m, name)


# ----------------------------------------------------------------------------- state errors
def test_state_errors():
    c = BT.case("one")
    b, keep = util.batch_from_dict(c.batches[0])
    ln = (C.c_int64 * 1)(c.lens[0])
    with make(c, lens=False) as eng:
        lib, h = eng.lib, eng.h
        # no lengths set: every push says which call is missing
        for fn in (lib.xck_push_batch, lib.xck_push_batch_device):
            assert fn(h, C.byref(b)) == capi.XCK_E_STATE and b"xck_set_contig_lengths" in lib.xck_last_error(h)
        assert lib.xck_push_batch_q(h, C.byref(b), None) == capi.XCK_E_STATE and b"xck_set_contig_lengths" in lib.xck_last_error(h)
        assert eng.stats()["n_reads"] == 0
        # bad lengths
        assert lib.xck_set_contig_lengths(h, ln, 2) == capi.XCK_E_ARG and lib.xck_set_contig_lengths(h, (C.c_int64 * 1)(0), 1) == capi.XCK_E_ARG
        assert lib.xck_set_contig_lengths(h, (C.c_int64 * 1)(1 << 31), 1) == capi.XCK_E_ARG and lib.xck_set_contig_lengths(h, None, 1) == capi.XCK_E_ARG
        assert lib.xck_set_contig_lengths(h, ln, 1) == 0 and lib.xck_set_contig_lengths(h, ln, 1) == 0
        assert lib.xck_push_batch(h, C.byref(b)) == 0
        # lengths set after a push
        assert lib.xck_set_contig_lengths(h, ln, 1) == capi.XCK_E_STATE
        # find_candidates before finish
        cfg = capi.CandidateConfig(); cfg.struct_size = C.sizeof(capi.CandidateConfig); cfg.min_count, cfg.min_maf = 1, 0
        out = capi.Candidates()
        assert lib.xck_find_candidates(h, C.byref(cfg), C.byref(out)) == capi.XCK_E_STATE and b"xck_finish" in lib.xck_last_error(h)
        eng.finish()
        assert lib.xck_find_candidates(h, C.byref(cfg), C.byref(out)) == 0 and out.n == 0 and out.positions_covered == 10
        cfg.struct_size = 8
        assert lib.xck_find_candidates(h, C.byref(cfg), C.byref(out)) == capi.XCK_E_ARG
        eng.reset()
        cfg.struct_size = C.sizeof(capi.CandidateConfig)
        assert lib.xck_find_candidates(h, C.byref(cfg), C.byref(out)) == capi.XCK_E_STATE
        assert lib.xck_set_contig_lengths(h, ln, 1) == 0                   # after a reset the lengths may be given again
    with make(c, tally=False) as eng:                                    # the getters on a handle without the flag
        lib, h = eng.lib, eng.h
        assert lib.xck_set_contig_lengths(h, ln, 1) == capi.XCK_E_STATE and b"XCK_F_BASE_TALLY" in lib.xck_last_error(h)
        assert lib.xck_get_base_tally(h, 0, 0, 1, (C.c_uint32 * 4)()) == capi.XCK_E_STATE
        st = capi.BaseTallyStats(); st.struct_size = C.sizeof(capi.BaseTallyStats)
        assert lib.xck_get_base_tally_stats(h, C.byref(st)) == capi.XCK_E_STATE
        cfg = capi.CandidateConfig(); cfg.struct_size = C.sizeof(capi.CandidateConfig)
        assert lib.xck_find_candidates(h, C.byref(cfg), C.byref(capi.Candidates())) == capi.XCK_E_STATE
        assert lib.xck_push_batch(h, C.byref(b)) == 0                      # ... which pushes as it always did


# ----------------------------------------------------------------------------- end to end
def _env(monkeypatch, path):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if path == "host":
        monkeypatch.setenv("XCK_GPU_INFLATE", "0")
    else:
        monkeypatch.setenv("XCK_GPU_INFLATE", "100")
        monkeypatch.setenv("XCK_GPU_INFLATE_MIN_MB", "0")


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("name", ["two_bam", "mixed", "past_end_bam"])
def test_discover_snps_end_to_end(name, path, tmp_path, monkeypatch):
    """discover_snps on a written BAM, no SNP anywhere on the handle, with the host inflate and through the device inflate and parse: the
    model's VCF text, the model's counters; pileup() then takes the file"""
    _env(monkeypatch, path)
    c, m = BT.case(name), BT.expected(name)
    bam, bc, vcf = str(tmp_path / "in.bam"), str(tmp_path / "barcodes.tsv"), str(tmp_path / ("cand.vcf" + (".gz" if path == "device" else "")))
    BT.write_bam(c, bam)
    with open(bc, "w") as fp:
        fp.write("".join(b + "\n" for b in B.BARCODES))
    f = dict(BT.FILT); f.update(c.filt)
    n, stats = discover.discover_snps(sam_fn=bam, barcode_fn=bc, out_vcf_fn=vcf, min_count=1, min_maf=0, min_mapq=f["min_mapq"], min_len=f["min_len"],
                                      incl_flag=f["incl_flag"], excl_flag=f["excl_flag"], no_orphan=f["no_orphan"], ncores=2)
    want = BT.candidates(m.tally, 1, 0)
    raw = open(vcf, "rb").read()
    text = gzip.decompress(raw).decode() if vcf.endswith(".gz") else raw.decode()
    print(name, path, n, stats)
    assert text == BT.vcf_text(["chr" + x for x in c.names], want)
    assert n == len(want["pos"]) and stats == dict(m.stats, positions_covered=want["positions_covered"])
    # the same file through a handle of the test's own: which decoder fed the pass, and the tables behind the VCF
    with Engine(BAF, ["chr" + x for x in c.names], [], c.n_cells, snps=[], barcodes=B.BARCODES, cell_tag="CB", umi_tag="UB", n_threads=2, base_tally=True, **f) as eng:
        assert eng.ingest_bam(bam) == sum(len(g) for g in c.groups) and list(eng.contig_len) == c.lens
        ds = eng.decode_stats()
        assert (ds["gpu_parse_chunks"] >= 1) if path == "device" else (ds["gpu_inflate_chunks"] == 0)
        check_tallies(eng, c, m, "%s %s" % (name, path))
    if name == "two_bam" and path == "host":
        from xcltk_amd.baf.genotype import pileup
        assert n > 0 and len(load_candidate_snps(vcf)) == n
        out_dir = str(tmp_path / "pileup")
        fn, n_raw, n_kept = pileup(sam_fn=bam, barcode_fn=bc, snp_vcf_fn=vcf, out_dir=out_dir, min_count=1, min_maf=0, ncores=2)
        assert os.path.isfile(fn) and 0 < n_kept <= n_raw <= n


def test_golden_10x_input(monkeypatch):
    """the dense golden dataset through Engine.ingest_bam (contig lengths from the BAM header): tallies over a sampled window and the
    candidate list equal the model fed by oracle/pybam.py"""
    _env(monkeypatch, "host")
    d = os.path.join(util.GOLDEN, "datasets", "dense")
    bam = os.path.join(d, "possorted.bam")
    with open(os.path.join(d, "barcodes.tsv")) as fp:
        barcodes = sorted(x.strip() for x in fp)
    refs = capi.bam_references(bam)
    names, lens = [n for n, _ in refs], [l for _, l in refs]
    filt = dict(min_mapq=20, min_len=30, excl_flag=772)
    m = BT.brute(bam, names, lens, filt, barcodes)
    assert m.stats["bases_tallied"] > 100000
    f = dict(BT.FILT); f.update(filt)
    with Engine(BAF, names, [], len(barcodes), snps=[], barcodes=barcodes, cell_tag="CB", umi_tag="UB", n_threads=2, base_tally=True, **f) as eng:
        assert eng.contig_len is None
        eng.ingest_bam(bam)
        assert list(eng.contig_len) == lens
        eng.finish()
        assert eng.base_tally_stats() == m.stats
        p0 = int(np.flatnonzero(m.tally[0].sum(axis=1))[0])
        for a, n in ((p0, 4096), (0, 100), (lens[0] - 4096, 4096), (150000, 20000)):
            assert np.array_equal(eng.base_tally(0, a, n), m.tally[0][a:a + n]), (a, n)
        for mc, mf in ((20, 0.1), (5, 0.25)):
            got, want = eng.find_candidates(mc, mf), BT.candidates(m.tally, mc, mf)
            print("golden", mc, mf, len(want["pos"]), want["positions_covered"])
            assert got["positions_covered"] == want["positions_covered"]
            for k in ("contig", "pos", "ref", "alt", "count"):
                assert np.array_equal(got[k], want[k]), k
