"""The genome's sequence on a tally handle and the candidates oriented by it (xck_set_contig_ref, xck_get_contig_ref,
xck_get_base_tally_contigs, xck_find_candidates_ref, include/xck.h) through the engine, against the models of
tests/refseq_cases.py, which tests/test_refseq_cases_host.py holds against a plain parse and against the plain candidate rule.
Every comparison is exact."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import base_tally_cases as BT
import baseq_cases as B
import refseq_cases as RS
import util
from test_gpu_base_tally import KNOBS, feed, make
from xcltk_amd import capi
from xcltk_amd.baf import discover
from xcltk_amd.engine import Engine
from xcltk_amd.utils import csp_io

pytestmark = pytest.mark.gpu
BAF = capi.XCK_MODE_BAF
THRESHOLDS = ((1, 0), (2, 0.2))
LISTS = ("contig", "pos", "ref", "alt", "count")


def tally_handle(lens, **kw):
    return Engine(BAF, ["c%d" % k for k in range(len(lens))], [], 3, snps=[], base_tally=True, contig_len=list(lens), **dict(BT.FILT, **kw))


def set_ref(eng, contig, raw, lb, lw, n_raw=None):
    buf = C.create_string_buffer(bytes(raw), len(raw))
    return eng.lib.xck_set_contig_ref(eng.h, contig, buf, len(raw) if n_raw is None else n_raw, lb, lw)


def load_genome(eng, contig, letters, lb=60, eol="\n"):
    text, fai = RS.fasta_text([("g", letters)], lb, eol)
    rc = set_ref(eng, contig, RS.raw_span(text, fai[0]), fai[0][3], fai[0][4])
    assert rc == 0, eng.lib.xck_last_error(eng.h)


# ----------------------------------------------------------------------------- pack
@pytest.mark.parametrize("chunk", [None, "64"], ids=["default_chunk", "chunk64"])
def test_pack_equals_the_model_over_the_grid(chunk, monkeypatch):
    """every geometry of the grid as a contig of one handle: the letters read back are the model's.  At 64 bytes a chunk the 2049-base
    contigs take more than 30 chunks each (tests/test_refseq_cases_host.py asserts that, and where the cuts fall, from the model)"""
    monkeypatch.delenv("XCK_REF_CHUNK_BYTES", raising=False)
    if chunk:
        monkeypatch.setenv("XCK_REF_CHUNK_BYTES", chunk)
    grid = RS.grid()
    assert min(len(RS.chunks(2049, lb, lb + len(eol), RS.MIN_CHUNK)) for lb in RS.line_bases_of(2049) for eol in RS.EOLS) > 30
    with tally_handle([g[0] for g in grid]) as eng:
        for c, (length, lb, eol, fin, place) in enumerate(grid):
            text, fai, k, want = RS.three(length, lb, eol, fin, place)
            raw = RS.raw_span(text, fai[k])
            assert set_ref(eng, c, raw, fai[k][3], fai[k][4]) == 0, (grid[c], eng.lib.xck_last_error(eng.h))
            got = eng.contig_ref(c, 0, length)
            assert got == RS.packed_letters(raw, length, fai[k][3], fai[k][4]) == "".join(RS.code_letter(ord(x)) for x in want), grid[c]
        assert eng.contig_ref(len(grid) - 1, 2040, 9) == RS.packed_letters(raw, length, fai[k][3], fai[k][4])[2040:] and eng.contig_ref(0, 0, 0) == ""
        assert eng.contig_ref(len(grid) - 1, 1001, 2) == RS.packed_letters(raw, length, fai[k][3], fai[k][4])[1001:1003]     # (an odd start)
        assert eng.tally_contigs() == []


def test_every_letter_and_every_byte_that_reads_as_n():
    body = bytes(range(33, 256))
    for lb in (len(body), 16):
        with tally_handle([len(body)]) as eng:
            raw = b"\n".join(body[a:a + lb] for a in range(0, len(body), lb))
            assert set_ref(eng, 0, raw, lb, lb + 1) == 0
            got = eng.contig_ref(0, 0, len(body))
            assert got == "".join(RS.code_letter(b) for b in body)
            assert set(got) == set(RS.LETTERS[1:]) and sum(x != "N" for x in got) == 2 * 14 and got[ord("=") - 33] == "N"


def test_replacing_a_sequence_and_a_stale_geometry():
    n = 500
    a, b = RS.seq_letters(n, 1, "ACGT"), RS.seq_letters(n, 2, "TGCAN")
    with tally_handle([n, n]) as eng:
        load_genome(eng, 0, a)
        load_genome(eng, 1, a, lb=7, eol="\r\n")
        assert eng.contig_ref(0, 0, n) == a == eng.contig_ref(1, 0, n)
        load_genome(eng, 0, b, lb=13)
        assert eng.contig_ref(0, 0, n) == b and eng.contig_ref(1, 0, n) == a
        # a stale index: the file was wrapped at 60, the index says 61 (and a line width to match)
        text, fai = RS.fasta_text([("g", a)], 60)
        raw = text[fai[0][2]:]
        assert len(raw) >= RS.offset(n - 1, 61, 62) + 1
        assert set_ref(eng, 0, raw, 61, 62) == capi.XCK_E_ARG and b"the FASTA line geometry does not match its index" in eng.lib.xck_last_error(eng.h)
        assert eng.lib.xck_get_contig_ref(eng.h, 0, 0, 1, C.create_string_buffer(2)) == capi.XCK_E_STATE
        assert eng.contig_ref(1, 0, n) == a                                # the other contig keeps its sequence
        load_genome(eng, 0, a)
        assert eng.contig_ref(0, 0, n) == a


# ----------------------------------------------------------------------------- orientation
def check_oriented(eng, m, genomes, what):
    for mc, mf in THRESHOLDS:
        want = RS.candidates_ref(m.tally, genomes, mc, mf)
        got = eng.find_candidates(mc, mf, use_ref=True)
        plain = eng.find_candidates(mc, mf, use_ref=False)
        again = eng.find_candidates(mc, mf, use_ref=True)
        assert "ref_stats" not in plain and got["ref_stats"] == want["ref_stats"] == again["ref_stats"], (what, mc, mf, got["ref_stats"], want["ref_stats"])
        assert got["positions_covered"] == want["positions_covered"] == plain["positions_covered"]
        for k in LISTS:
            assert np.array_equal(got[k], want[k]) and np.array_equal(got[k], again[k]), "%s: candidates.%s at (%s, %s)" % (what, k, mc, mf)
            assert np.array_equal(plain[k], BT.candidates(m.tally, mc, mf)[k]), (what, k)
        st = got["ref_stats"]
        assert sum(st.values()) == len(plain["pos"]) and st["ref_major"] + st["ref_minor"] == len(got["pos"]), (what, mc, mf)


@pytest.mark.parametrize("name,flags", [(n, 0) for n in BT.CASES] + [(n, capi.XCK_F_FORCE_KEY128) for n in ("codes", "two_contigs", "baseq")],
                         ids=[n + "-k64" for n in BT.CASES] + [n + "-k128" for n in ("codes", "two_contigs", "baseq")])
def test_oriented_candidates_match_the_model(name, flags):
    c, m = BT.case(name), BT.expected(name)
    with make(c, flags) as eng:
        keep = feed(eng, c)
        eng.finish()
        for kind in RS.GENOMES:
            genomes = {k: RS.genome(t, kind) for k, t in m.tally.items()}
            for k, g in genomes.items():
                load_genome(eng, k, g, lb=61 if kind == "mix" else 60)
            assert eng.contig_ref(0, 0, c.lens[0]) == genomes[0].upper()
            check_oriented(eng, m, genomes, "%s %s" % (name, kind))
        # after reset the sequence is still there and there are no candidates
        eng.reset()
        assert eng.contig_ref(0, 0, c.lens[0]) == genomes[0].upper()
        eng.finish()
        got = eng.find_candidates(1, 0, use_ref=True)
        assert len(got["pos"]) == 0 and got["positions_covered"] == 0 and got["ref_stats"] == dict.fromkeys(RS.CLASSES, 0)


def test_a_contig_without_a_sequence_counts_as_unknown():
    c, m = BT.case("two_contigs"), BT.expected("two_contigs")
    with make(c) as eng:
        keep = feed(eng, c)
        assert eng.tally_contigs() == [0, 1]
        eng.finish()
        check_oriented(eng, m, {}, "no sequence at all")
        g1 = RS.genome(m.tally[1], "second")
        load_genome(eng, 1, g1)
        check_oriented(eng, m, {1: g1}, "the second contig alone")
        n1 = len(BT.candidates({1: m.tally[1]}, 1, 0)["pos"])
        st = eng.find_candidates(1, 0, use_ref=True)["ref_stats"]
        assert n1 > 0 and st["ref_minor"] == n1 and st["ref_unknown"] == len(BT.candidates({0: m.tally[0]}, 1, 0)["pos"]) > 0


def test_set_reference_from_a_file(tmp_path):
    """Engine.set_reference: chr tolerance, only the contigs with a table after pushes, the wrong-build guard, use_ref's default"""
    c, m = BT.case("contention"), BT.expected("contention")
    g0 = RS.genome(m.tally[0], "second")
    assert len(BT.candidates(m.tally, 1, 0)["pos"]) == 1
    text, fai = RS.fasta_text([("chrX", "ACGT" * 10), ("chr1", g0), ("chr2", "ACGTN" * 10)], 50)
    fn = str(tmp_path / "genome.fa")
    with open(fn, "wb") as fp:
        fp.write(text)
    bad = str(tmp_path / "other_build.fa")
    with open(bad, "wb") as fp:
        fp.write(RS.fasta_text([("1", g0[:-1]), ("2", "ACGTN" * 10)], 50)[0])
    f = dict(BT.FILT); f.update(c.filt)
    with Engine(BAF, ["1", "2", "3"], [], c.n_cells, snps=[], base_tally=True, contig_len=[c.lens[0], 50, 9], **f) as eng:
        assert eng.set_reference(fn) == dict(loaded=["1", "2"], missing=["3"])              # before pushes: every contig
        assert eng.contig_ref("2", 0, 50) == "ACGTN" * 10 and eng.contig_ref(0, 0, c.lens[0]) == g0
    for with_fai in (False, True):
        if with_fai:
            with open(fn + ".fai", "w") as fp:
                fp.write(RS.fai_text(fai))
        with Engine(BAF, ["1", "2", "3"], [], c.n_cells, snps=[], base_tally=True, contig_len=[c.lens[0], 50, 9], **f) as eng:
            keep = feed(eng, c)
            eng.finish()
            assert "ref_stats" not in eng.find_candidates(1, 0)
            with pytest.raises(ValueError) as ei:
                eng.set_reference(bad)
            assert "'1'" in str(ei.value) and str(c.lens[0]) in str(ei.value) and str(c.lens[0] - 1) in str(ei.value)
            assert eng.set_reference(fn) == dict(loaded=["1"], missing=[])                  # after pushes: the contigs with a table
            assert eng.lib.xck_get_contig_ref(eng.h, 1, 0, 1, C.create_string_buffer(2)) == capi.XCK_E_STATE
            got, want = eng.find_candidates(1, 0), RS.candidates_ref(m.tally, {0: g0}, 1, 0)
            assert got["ref_stats"] == want["ref_stats"] and all(np.array_equal(got[k], want[k]) for k in LISTS)
            assert eng.set_reference(fn, names=["2", "3"]) == dict(loaded=["2"], missing=["3"])


# ----------------------------------------------------------------------------- state and argument errors
def test_state_and_argument_errors():
    c = BT.case("one")
    E_ARG, E_STATE = capi.XCK_E_ARG, capi.XCK_E_STATE
    raw = b"ACGTACGTAC\nACGTACGTAC\n" * 1000
    out = C.create_string_buffer(64)
    cfg = capi.CandidateConfig(); cfg.struct_size = C.sizeof(capi.CandidateConfig); cfg.min_count, cfg.min_maf = 1, 0
    st = capi.CandidateRefStats(); st.struct_size = C.sizeof(capi.CandidateRefStats)
    with make(c, lens=False) as eng:                                      # no lengths set
        lib, h = eng.lib, eng.h
        assert set_ref(eng, 0, raw, 10, 11) == E_STATE and b"xck_set_contig_lengths" in lib.xck_last_error(h)
        assert lib.xck_get_contig_ref(h, 0, 0, 1, out) == E_STATE
        assert lib.xck_get_base_tally_contigs(h, (C.c_uint8 * 1)(), 1) == 0
    with make(c) as eng:
        lib, h = eng.lib, eng.h
        n = c.lens[0]
        need = RS.offset(n - 1, 10, 11) + 1
        assert len(raw) >= need
        assert set_ref(eng, 1, raw, 10, 11) == E_ARG and set_ref(eng, -1, raw, 10, 11) == E_ARG
        assert set_ref(eng, 0, raw, 0, 11) == E_ARG and set_ref(eng, 0, raw, 10, 9) == E_ARG and set_ref(eng, 0, raw, -1, -1) == E_ARG
        assert set_ref(eng, 0, raw, 10, 11, n_raw=need - 1) == E_ARG and lib.xck_set_contig_ref(h, 0, None, need, 10, 11) == E_ARG
        assert lib.xck_get_contig_ref(h, 0, 0, 1, out) == E_STATE         # no sequence yet
        assert set_ref(eng, 0, raw, 10, 11, n_raw=need) == 0              # before any push
        assert set_ref(eng, 0, raw, 10, 10) == E_ARG and b"does not match its index" in lib.xck_last_error(h)   # (line_width == line_bases over a text with line ends)
        assert lib.xck_get_contig_ref(h, 0, 0, 1, out) == E_STATE
        assert set_ref(eng, 0, raw, 10, 11) == 0
        for args in ((1, 0, 1), (0, -1, 1), (0, n - 1, 2), (0, 0, -1)):
            assert lib.xck_get_contig_ref(h, *args, out) == E_ARG, args
        assert lib.xck_get_contig_ref(h, 0, n - 1, 1, out) == 0 and lib.xck_get_contig_ref(h, 0, 5, 0, None) == 0
        assert lib.xck_get_base_tally_contigs(h, (C.c_uint8 * 2)(), 2) == E_ARG and lib.xck_get_base_tally_contigs(h, None, 1) == E_ARG
        has = (C.c_uint8 * 1)(7)
        assert lib.xck_get_base_tally_contigs(h, has, 1) == 0 and has[0] == 0
        cand = capi.Candidates()
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(cand), C.byref(st)) == E_STATE and b"xck_finish" in lib.xck_last_error(h)
        keep = feed(eng, c)
        assert lib.xck_get_base_tally_contigs(h, has, 1) == 0 and has[0] == 1
        assert set_ref(eng, 0, raw, 10, 11) == 0                          # after a push
        eng.finish()
        assert set_ref(eng, 0, raw, 10, 11) == 0                          # after finish
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(cand), C.byref(st)) == 0 and cand.positions_covered == 10
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(cand), None) == E_ARG and lib.xck_find_candidates_ref(h, None, C.byref(cand), C.byref(st)) == E_ARG
        st.struct_size = 8
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(cand), C.byref(st)) == E_ARG
        st.struct_size = C.sizeof(capi.CandidateRefStats); cfg.struct_size = 8
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(cand), C.byref(st)) == E_ARG
        cfg.struct_size = C.sizeof(capi.CandidateConfig)
        eng.reset()
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(cand), C.byref(st)) == E_STATE
        assert eng.contig_ref(0, 0, 12) == "ACGTACGTACAC"
        # new lengths after a reset: a contig whose length changes loses its sequence, one that keeps it does not
        eng.set_contig_lengths([n])
        assert eng.contig_ref(0, 0, 4) == "ACGT"
        eng.set_contig_lengths([n - 1])
        assert lib.xck_get_contig_ref(h, 0, 0, 1, out) == E_STATE
    with make(c, tally=False) as eng:                                     # a handle without the flag
        lib, h = eng.lib, eng.h
        assert set_ref(eng, 0, raw, 10, 11) == E_STATE and b"XCK_F_BASE_TALLY" in lib.xck_last_error(h)
        assert lib.xck_get_contig_ref(h, 0, 0, 1, out) == E_STATE and lib.xck_get_base_tally_contigs(h, (C.c_uint8 * 1)(), 1) == E_STATE
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(capi.Candidates()), C.byref(st)) == E_STATE


# ----------------------------------------------------------------------------- end to end
def _env(monkeypatch, path):
    for k in KNOBS + ("XCK_REF_CHUNK_BYTES",):
        monkeypatch.delenv(k, raising=False)
    if path == "host":
        monkeypatch.setenv("XCK_GPU_INFLATE", "0")
    else:
        monkeypatch.setenv("XCK_GPU_INFLATE", "100")
        monkeypatch.setenv("XCK_GPU_INFLATE_MIN_MB", "0")


def _read(fn):
    raw = open(fn, "rb").read()
    return gzip.decompress(raw).decode() if fn.endswith(".gz") else raw.decode()


@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("name", ["two_bam", "mixed", "past_end_bam"])
def test_discover_snps_with_a_reference_end_to_end(name, path, tmp_path, monkeypatch):
    """discover_snps(refseq_fn=) on a written BAM through the host and the device decoder: the model's VCF text and counters, only the
    contigs with reads loaded; pileup() then counts the same molecules under either orientation"""
    _env(monkeypatch, path)
    c, m = BT.case(name), BT.expected(name)
    bam, bc = str(tmp_path / "in.bam"), str(tmp_path / "barcodes.tsv")
    vcf, vcf0 = (str(tmp_path / (x + (".gz" if path == "device" else ""))) for x in ("oriented.vcf", "plain.vcf"))
    BT.write_bam(c, bam)
    with open(bc, "w") as fp:
        fp.write("".join(b + "\n" for b in B.BARCODES))
    genomes = {k: RS.e2e_genome(t, 1, 0) for k, t in m.tally.items()}
    fa = str(tmp_path / "genome.fa")
    with open(fa, "wb") as fp:                                             # the FASTA names the contigs without chr, and one contig more
        fp.write(RS.fasta_text([(x, genomes[k]) for k, x in enumerate(c.names)] + [("unplaced", "ACGT" * 30)], 60)[0])
    f = dict(BT.FILT); f.update(c.filt)
    kw = dict(sam_fn=bam, barcode_fn=bc, min_count=1, min_maf=0, min_mapq=f["min_mapq"], min_len=f["min_len"], incl_flag=f["incl_flag"], excl_flag=f["excl_flag"],
              no_orphan=f["no_orphan"], ncores=2)
    n, stats = discover.discover_snps(out_vcf_fn=vcf, refseq_fn=fa, **kw)
    n0, stats0 = discover.discover_snps(out_vcf_fn=vcf0, **kw)
    touched = sorted({int(d["contig"]) for d in c.batches})
    want = RS.candidates_ref(m.tally, {k: genomes[k] for k in touched}, 1, 0)
    plain = BT.candidates(m.tally, 1, 0)
    chroms = ["chr" + x for x in c.names]
    print(name, path, n, stats)
    assert _read(vcf) == RS.vcf_text_ref(chroms, want, fa) and _read(vcf0) == BT.vcf_text(chroms, plain)
    assert n == len(want["pos"]) and n0 == len(plain["pos"]) and stats0 == dict(m.stats, positions_covered=plain["positions_covered"])
    assert stats == dict(stats0, ref_contigs=[chroms[k] for k in touched], ref_contigs_missing=[], **want["ref_stats"])
    if name == "two_bam":
        assert want["ref_stats"]["ref_minor"] > 0 and want["ref_stats"]["ref_major"] > 0 and want["ref_stats"]["ref_unknown"] > 0
    if name == "two_bam" and path == "host":
        from xcltk_amd.baf.genotype import pileup
        d = {}
        for key, v in (("oriented", vcf), ("plain", vcf0)):
            out_dir = str(tmp_path / key)
            pileup(sam_fn=bam, barcode_fn=bc, snp_vcf_fn=v, out_dir=out_dir, min_count=0, min_maf=0, ncores=2)
            d[key] = csp_io.load_data(os.path.join(out_dir, "raw"))
        a, b = d["oriented"], d["plain"]
        where = {(str(ch), int(p)): j for j, (ch, p) in enumerate(zip(b.chrom, b.pos))}
        same = swapped = 0
        for i, (ch, p) in enumerate(zip(a.chrom, a.pos)):
            j = where[(str(ch), int(p))]                                   # (the oriented list is a subset of the plain one)
            ad, dp, oth = (np.asarray(x[:, i].todense()).ravel() for x in (a.AD, a.DP, a.OTH))
            ad0, dp0, oth0 = (np.asarray(x[:, j].todense()).ravel() for x in (b.AD, b.DP, b.OTH))
            if (a.ref[i], a.alt[i]) == (b.ref[j], b.alt[j]):
                same += 1
                assert np.array_equal(ad, ad0) and np.array_equal(dp, dp0) and np.array_equal(oth, oth0), (ch, p)
            elif (a.ref[i], a.alt[i]) == (b.alt[j], b.ref[j]):
                swapped += 1
                assert np.array_equal(ad, dp0 - ad0) and np.array_equal(dp, dp0) and np.array_equal(oth, oth0), (ch, p)
        assert same > 0 and swapped > 0


def test_discover_command_line_takes_refseq(tmp_path, monkeypatch):
    _env(monkeypatch, "host")
    c, m = BT.case("two_bam"), BT.expected("two_bam")
    bam, bc, vcf, fa = (str(tmp_path / x) for x in ("in.bam", "barcodes.tsv", "out.vcf", "genome.fa"))
    BT.write_bam(c, bam)
    with open(bc, "w") as fp:
        fp.write("".join(b + "\n" for b in B.BARCODES))
    g = {k: RS.genome(t, "second") for k, t in m.tally.items()}
    with open(fa, "wb") as fp:
        fp.write(RS.fasta_text([("chr1", g[0]), ("chr2", g[1])], 70, "\r\n")[0])
    f = dict(BT.FILT); f.update(c.filt)
    argv = ["xcltk", "discover", "-s", bam, "-b", bc, "-O", vcf, "--refseq", fa, "--minCOUNT", "1", "--minMAF", "0", "--minMAPQ", str(f["min_mapq"]),
            "--minLEN", str(f["min_len"]), "--exclFLAG", str(f["excl_flag"]), "-p", "2"]
    assert discover.discover_main(argv) == 0
    want = RS.candidates_ref(m.tally, g, 1, 0)
    assert len(want["pos"]) > 0 and _read(vcf) == RS.vcf_text_ref(["chr1", "chr2"], want, fa)


def test_golden_10x_input_with_a_reference(monkeypatch, tmp_path):
    """the dense golden dataset: candidates oriented by a genome made from the model's tallies equal the model fed by oracle/pybam.py"""
    _env(monkeypatch, "host")
    d = os.path.join(util.GOLDEN, "datasets", "dense")
    bam = os.path.join(d, "possorted.bam")
    with open(os.path.join(d, "barcodes.tsv")) as fp:
        barcodes = sorted(x.strip() for x in fp)
    refs = capi.bam_references(bam)
    names, lens = [n for n, _ in refs], [l for _, l in refs]
    filt = dict(min_mapq=20, min_len=30, excl_flag=772)
    m = BT.brute(bam, names, lens, filt, barcodes)
    covered = [c for c, t in m.tally.items() if t.any()]
    genomes = {c: RS.e2e_genome(m.tally[c], 5, 0.25) for c in covered}
    fa = str(tmp_path / "genome.fa")
    with open(fa, "wb") as fp:
        fp.write(RS.fasta_text([(names[c], genomes[c]) for c in covered], 60)[0])
    f = dict(BT.FILT); f.update(filt)
    with Engine(BAF, names, [], len(barcodes), snps=[], barcodes=barcodes, cell_tag="CB", umi_tag="UB", n_threads=2, base_tally=True, **f) as eng:
        eng.ingest_bam(bam)
        eng.finish()
        assert eng.set_reference(fa) == dict(loaded=[names[c] for c in covered], missing=[])
        p0 = int(np.flatnonzero(m.tally[covered[0]].sum(axis=1))[0])
        assert eng.contig_ref(covered[0], p0, 4096) == genomes[covered[0]][p0:p0 + 4096]
        for mc, mf in ((20, 0.1), (5, 0.25)):
            got, want, plain = eng.find_candidates(mc, mf), RS.candidates_ref(m.tally, genomes, mc, mf), eng.find_candidates(mc, mf, use_ref=False)
            print("golden", mc, mf, len(want["pos"]), want["ref_stats"])
            assert got["ref_stats"] == want["ref_stats"] and got["positions_covered"] == want["positions_covered"]
            for k in LISTS:
                assert np.array_equal(got[k], want[k]), k
            assert sum(got["ref_stats"].values()) == len(plain["pos"]) and got["ref_stats"]["ref_major"] + got["ref_stats"]["ref_minor"] == len(got["pos"])
        assert want["ref_stats"]["ref_minor"] > 0 and want["ref_stats"]["ref_unknown"] > 0
