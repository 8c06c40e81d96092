"""The reference sequence of a tally handle without a GPU: the offset formula and the packing model of
tests/refseq_cases.py against a plain line-by-line parse over every line geometry, utils/fasta.py's in-memory index against literal .fai
lines and its rejections, the rule that orients a candidate by the genome's base with literals, at its ties and through its two
identities on every case of tests/base_tally_cases.py, the VCF text with a reference, the name and length matching of
Engine.set_reference, the new calls' state errors on a handle without the flag, and csrc/ref_geom.h - the arithmetic the pack kernel
shares with the host - under AddressSanitizer in a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import base_tally_cases as BT
import refseq_cases as RS
from xcltk_amd import capi
from xcltk_amd.baf import discover
from xcltk_amd.baf.genotype import VCF_HEADER, load_candidate_snps
from xcltk_amd.engine import Engine
from xcltk_amd.utils import fasta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- geometry
def test_offset_formula_and_packing_model_equal_a_plain_parse():
    n = 0
    for length, lb, eol, fin, place in RS.grid():
        text, fai, k, want = RS.three(length, lb, eol, fin, place)
        assert RS.plain_parse(text)["s%d" % k] == want
        name, ln, off, b, w = fai[k]
        assert (ln, b, w) == (length, lb, lb + len(eol))
        raw = RS.raw_span(text, fai[k])
        assert len(raw) == RS.offset(length - 1, b, w) + 1 and off + len(raw) <= len(text)
        assert RS.packed_letters(raw, length, b, w) == "".join(RS.code_letter(ord(x)) for x in want)
        assert all(raw[RS.offset(p, b, w)] == ord(want[p]) for p in (0, length // 2, length - 1))
        n += 1
    assert n == len(RS.LENGTHS) * 2 * 2 * 3 * 6 - 2 * 2 * 3 * sum(6 - len(RS.line_bases_of(x)) for x in RS.LENGTHS)


def test_code_letters():
    for k, x in enumerate(RS.LETTERS[1:]):
        assert RS.code_letter(ord(x)) == x and RS.code_letter(ord(x.lower())) == x
    for x in "=*-.U7u \n\rEZ":
        assert RS.code_letter(ord(x)) == "N", x
    assert RS.code_letter(200) == "N"
    assert set(RS.ALPHABET) >= set(RS.LETTERS[1:]) | set(RS.LETTERS[1:].lower()) | set("=*-.U7")


def test_chunks_cover_the_contig_and_end_on_every_kind_of_byte():
    """the staging chunks of the 2049-base contig at the smallest chunk size: more than 30.  A chunk is a range of positions, so its bytes
    begin and end on a base; the cut behind it falls in front of a base of the same line, in front of a \\n and in front of a \\r\\n"""
    kinds = set()
    for lb in RS.line_bases_of(2049):
        for eol in RS.EOLS:
            text, fai, k, _ = RS.three(2049, lb, eol, True, 1)
            raw = text[fai[k][2]:]
            ch = RS.chunks(2049, lb, lb + len(eol), RS.MIN_CHUNK)
            assert len(ch) > 30 and ch[0][0] == 0 and ch[-1][1] == 2049
            for (p0, p1, a, b), nxt in zip(ch, ch[1:] + [None]):
                assert p0 % 8 == 0 and p0 < p1 and (nxt is None or (nxt[0] == p1 and p1 % 8 == 0)) and b - a <= max(RS.MIN_CHUNK, 8 * (lb + len(eol)))
                if nxt is not None:                                       # the byte behind the chunk's last one: what the next copy does not start with
                    nb = raw[b:b + 1]
                    kinds.add("base" if nb not in (b"\r", b"\n") else "crlf" if nb == b"\r" else "lf")
    assert kinds == {"base", "lf", "crlf"}
    for lb in (1, 3, 60):                                                 # no chunk begins or ends on a byte of a line end
        text, fai, k, _ = RS.three(2049, lb, "\r\n", True, 1)
        raw = text[fai[k][2]:]
        assert all(raw[a] not in b"\r\n" and raw[b - 1] not in b"\r\n" for _, _, a, b in RS.chunks(2049, lb, lb + 2, RS.MIN_CHUNK))


# ----------------------------------------------------------------------------- utils/fasta.py
def test_in_memory_index_equals_the_literal_fai(tmp_path):
    for lb, eol, fin in ((60, "\n", True), (7, "\r\n", False), (1, "\n", False), (200, "\r\n", True)):
        seqs = [("chr1", RS.seq_letters(130, 1)), ("2", RS.seq_letters(61, 2)), ("chrM", RS.seq_letters(7, 3)), ("x", RS.seq_letters(lb, 4))]
        text, fai = RS.fasta_text(seqs, lb, eol, fin)
        got = fasta.build_index(text)
        want = [fasta.FaiEntry(*e) for e in fai]
        # (a sequence of one line: samtools records the line as it stands)
        for g, w, (_, s) in zip(got, want, seqs):
            assert g[:3] == w[:3]
            if len(s) > lb:
                assert g == w
            assert RS.packed_letters(text[g.offset:], g.length, g.line_bases, g.line_width) == RS.packed_letters(text[w.offset:], w.length, w.line_bases, w.line_width)
        fn = str(tmp_path / ("g%d.fa" % lb))
        with open(fn, "wb") as fp:
            fp.write(text)
        before = sorted(os.listdir(str(tmp_path)))
        with fasta.Fasta(fn) as fa:
            assert fa.entries == got
        assert sorted(os.listdir(str(tmp_path))) == before               # nothing is written next to the input
        with open(fn + ".fai", "w") as fp:
            fp.write(RS.fai_text(fai))
        assert fasta.read_fai(fn + ".fai") == want
        with fasta.Fasta(fn) as fa:
            assert fa.entries == want
            addr, n_raw, b, w = fa.span(fa.entries[1])
            assert C.string_at(addr, n_raw) == RS.raw_span(text, fai[1]) and (b, w) == (lb, lb + len(eol))
    assert fasta.build_index(b">a\nACGT\n>b desc\n\n>c\nAC\nGT\nA") == [("a", 4, 3, 4, 5), ("b", 0, 16, 0, 0), ("c", 5, 20, 2, 3)]


def test_ragged_lines_and_compressed_files_are_rejected(tmp_path):
    for text in (b">a\nACGT\nAC\nACGT\n", b">a\nACGT\nACGTA\n", b">a\nACGT\n\nACGT\n", b">a\nACGT\r\nACGT\nAC\n"):
        with pytest.raises(ValueError, match="different line length in sequence 'a'"):
            fasta.build_index(text)
    assert fasta.build_index(b">a\nACGT\nAC\n\n\n")[0][:2] == ("a", 6)            # a shorter last line, empty lines behind it
    with pytest.raises(ValueError, match="in front of the first"):
        fasta.build_index(b"ACGT\n>a\nAC\n")
    import gzip
    for name, data in (("g.fa.gz", gzip.compress(b">a\nACGT\n")), ("h.fa", gzip.compress(b">a\nACGT\n")), ("i.fa.gz", b">a\nACGT\n")):
        fn = str(tmp_path / name)
        with open(fn, "wb") as fp:
            fp.write(data)
        with pytest.raises(ValueError, match="decompress it first"):
            fasta.Fasta(fn)


def test_name_and_length_matching():
    e = [fasta.FaiEntry("chr1", 100, 6, 60, 61), fasta.FaiEntry("2", 50, 120, 60, 61), fasta.FaiEntry("chrM", 9, 200, 60, 61)]
    pairs, missing = fasta.match_contigs(e, ["1", "chr2", "3", "M"], [100, 50, 70, 9])
    assert [(c, x.name) for c, x in pairs] == [(0, "chr1"), (1, "2"), (3, "chrM")] and missing == ["3"]
    pairs, missing = fasta.match_contigs(e, ["1", "chr2", "3", "M"], [100, 51, 70, 9], want=[0, 2])
    assert [(c, x.name) for c, x in pairs] == [(0, "chr1")] and missing == ["3"]    # (the contig of another length was not asked for)
    with pytest.raises(ValueError) as ei:
        fasta.match_contigs(e, ["1", "chr2"], [100, 51])
    assert "'chr2'" in str(ei.value) and "51" in str(ei.value) and "50" in str(ei.value) and "'2'" in str(ei.value)


# ----------------------------------------------------------------------------- the rule
def test_orientation_rule_literals():
    c = (6, 4, 0, 0)
    assert RS.orient(c, "A", 4, 0.25) == ("ref_major", "A", "C")
    assert RS.orient(c, "C", 4, 0.25) == ("ref_minor", "C", "A")
    assert RS.orient(c, "G", 4, 0.25) == ("ref_unsupported", None, None)
    assert RS.orient(c, "N", 4, 0.25) == ("ref_unknown", None, None) and RS.orient(c, "R", 4, 0.25)[0] == "ref_unknown"
    assert RS.orient((5, 3, 3, 0), "G", 4, 0.25) == ("ref_minor", "G", "A") and BT.candidate((5, 3, 3, 0), 4, 0.25) == (True, "A", "C")
    assert RS.orient((0, 9, 1, 0), "G", 4, 0.1) == ("ref_minor", "G", "C")
    assert RS.orient((0, 9, 1, 0), "A", 4, 0.1) == ("ref_unsupported", None, None)
    assert RS.orient((2, 18, 0, 0), "A", 20, 0.1) == ("ref_minor", "A", "C")        # the tie 2 == 20 * 0.1 passes
    assert RS.orient((1, 19, 0, 0), "A", 20, 0.1) == (None, None, None) and not BT.candidate((1, 19, 0, 0), 20, 0.1)[0]
    assert RS.orient((0, 0, 0, 0), "A", 0, 0) == (None, None, None) and RS.orient((7, 0, 0, 0), "N", 0, 0) == (None, None, None)
    assert RS.orient((3, 3, 3, 3), "T", 1, 0) == ("ref_minor", "T", "A") and RS.orient((3, 3, 3, 3), "A", 1, 0) == ("ref_major", "A", "C")


TIES = [((9, 1, 0, 0), 0.1), ((27, 3, 0, 0), 0.1), ((2, 1, 0, 0), 0.333333), ((93, 7, 0, 0), 0.07), ((85, 15, 0, 0), 0.15), ((35, 15, 0, 0), 0.3), ((0, 2, 1, 0), 1 / 3), ((43, 0, 6, 0), 6 / 49), ((1, 0, 0, 1), 0.5)]


def test_orientation_rule_at_ties():
    """the ties of tests/test_base_tally_cases_host.py with the genome's base the minority base: the threshold now meets c[REF], and the
    verdict is that of !((double)m < (double)n * f)"""
    for c, f in TIES:
        n = sum(c)
        order = sorted(range(4), key=lambda b: (-c[b], b))
        major, minor = BT.BASES[order[0]], BT.BASES[order[1]]
        want = not (float(c[order[1]]) < float(n) * f)
        for g, cls in ((minor, "ref_minor"), (major, "ref_major")):
            got = RS.orient(c, g, 1, f)
            assert (got[0] == cls) == want and (got[0] is None) == (not want), (c, f, g)
            assert got[0] is None or (got[1] == g and got[2] == (major if g == minor else minor))
    assert RS.orient((93, 7, 0, 0), "C", 1, 0.07)[0] is None and RS.orient((85, 15, 0, 0), "C", 1, 0.15)[0] == "ref_minor"
    c = (8, 4, 0, 0)                                                       # min_count at n
    assert RS.orient(c, "C", 12.0, 0)[0] == "ref_minor" and RS.orient(c, "C", 12.000001, 0)[0] is None and RS.orient(c, "C", 11.5, 0)[0] == "ref_minor"


@pytest.mark.parametrize("name", BT.CASES)
def test_identities_on_every_case(name):
    m = BT.expected(name)
    for mc, mf in ((1, 0), (2, 0.2)):
        plain = BT.candidates(m.tally, mc, mf)
        for kind in RS.GENOMES:
            g = {c: RS.genome(t, kind) for c, t in m.tally.items()}
            got = RS.candidates_ref(m.tally, g, mc, mf)
            st = got["ref_stats"]
            assert sum(st.values()) == len(plain["pos"]) and st["ref_major"] + st["ref_minor"] == len(got["pos"]), (kind, mc, mf)
            assert got["positions_covered"] == plain["positions_covered"]
            assert set(zip(got["contig"].tolist(), got["pos"].tolist())) <= set(zip(plain["contig"].tolist(), plain["pos"].tolist()))
            if kind == "major":
                assert st == dict(ref_major=len(plain["pos"]), ref_minor=0, ref_unsupported=0, ref_unknown=0)
                assert all(np.array_equal(got[k], plain[k]) for k in ("contig", "pos", "ref", "alt", "count"))
            if kind == "second":
                assert st["ref_major"] == 0 and st["ref_unknown"] == 0 and st["ref_minor"] == len(plain["pos"])
                assert np.array_equal(got["ref"], plain["alt"]) and np.array_equal(got["alt"], plain["ref"])
            if kind == "N":
                assert st["ref_unknown"] == len(plain["pos"]) and len(got["pos"]) == 0


def test_the_cases_reach_every_class():
    tot = dict.fromkeys(RS.CLASSES, 0)
    for name in BT.CASES:
        m = BT.expected(name)
        st = RS.candidates_ref(m.tally, {c: RS.genome(t, "mix") for c, t in m.tally.items()}, 1, 0)["ref_stats"]
        for k in RS.CLASSES:
            tot[k] += st[k]
    print(tot)
    assert all(v > 0 for v in tot.values())


# ----------------------------------------------------------------------------- the VCF text
def test_vcf_text_with_a_reference(tmp_path):
    m = BT.expected("two_bam")
    g = {c: RS.e2e_genome(t, 1, 0) for c, t in m.tally.items()}
    cand = RS.candidates_ref(m.tally, g, 1, 0)
    st = cand["ref_stats"]
    assert st["ref_major"] > 0 and st["ref_minor"] > 0 and st["ref_unknown"] > 0
    chroms = ["chr1", "chr2"]
    fn = str(tmp_path / "cand.vcf")
    assert discover.write_candidate_vcf(fn, chroms, cand, "/some/genome.fa") == len(cand["pos"])
    text = open(fn).read()
    assert text == RS.vcf_text_ref(chroms, cand, "/some/genome.fa")
    assert text.startswith(VCF_HEADER + "##reference=/some/genome.fa\n#CHROM\t") and text.count("##reference=") == 1
    assert discover.candidate_vcf_text(chroms, cand) == BT.vcf_text(chroms, cand)            # without the option: the plain text
    assert load_candidate_snps(fn) == [(chroms[int(c)], int(p), str(r), str(a)) for c, p, r, a in zip(cand["contig"], cand["pos"], cand["ref"], cand["alt"])]
    # INFO by the written orientation, on a line the plain rule writes the other way round
    plain = BT.candidates(m.tally, 1, 0)
    where = {(int(c), int(p)): i for i, (c, p) in enumerate(zip(plain["contig"], plain["pos"]))}
    i = next(i for i in range(len(cand["pos"])) if cand["ref"][i] != plain["ref"][where[(int(cand["contig"][i]), int(cand["pos"][i]))]])
    cnt = [int(x) for x in cand["count"][i]]
    r, a = cnt[BT.BASES.index(cand["ref"][i])], cnt[BT.BASES.index(cand["alt"][i])]
    assert r <= a and "\t%s\t%s\t.\tPASS\tAD=%d;DP=%d;OTH=%d\n" % (cand["ref"][i], cand["alt"][i], a, r + a, sum(cnt) - r - a) in text


def test_discover_knows_the_option():
    assert "--refseq" in discover.USAGE and "-f," in discover.USAGE


# ----------------------------------------------------------------------------- state errors that need no GPU
def test_new_calls_on_a_handle_without_the_flag_are_state_errors():
    with Engine(capi.XCK_MODE_BAF, ["1"], [], 3, snps=[], decode_only=True, **BT.FILT) as eng:
        lib, h = eng.lib, eng.h
        raw = C.create_string_buffer(b"ACGT")
        assert lib.xck_set_contig_ref(h, 0, raw, 4, 4, 5) == capi.XCK_E_STATE and b"XCK_F_BASE_TALLY" in lib.xck_last_error(h)
        assert lib.xck_get_contig_ref(h, 0, 0, 1, C.create_string_buffer(2)) == capi.XCK_E_STATE
        assert lib.xck_get_base_tally_contigs(h, (C.c_uint8 * 1)(), 1) == capi.XCK_E_STATE
        cfg = capi.CandidateConfig(); cfg.struct_size = C.sizeof(capi.CandidateConfig)
        st = capi.CandidateRefStats(); st.struct_size = C.sizeof(capi.CandidateRefStats)
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(capi.Candidates()), C.byref(st)) == capi.XCK_E_STATE
        st.struct_size = 8
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(capi.Candidates()), C.byref(st)) == capi.XCK_E_ARG
        assert lib.xck_find_candidates_ref(h, C.byref(cfg), C.byref(capi.Candidates()), None) == capi.XCK_E_ARG
        with pytest.raises(ValueError, match="lengths"):
            eng.set_reference("/nowhere.fa")


# ----------------------------------------------------------------------------- the shared arithmetic under the sanitizers
def test_pack_arithmetic_is_sound_under_asan():
    """tools/asan/ref_geom_check.cpp: csrc/ref_geom.h over the grid, every chunk in a block of exactly its size"""
    asan = os.path.join(ROOT, "tools", "asan")
    r = subprocess.run(["make", "-C", asan, "ref_geom_check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and ("cannot find -lasan" in r.stdout or "cannot find -lubsan" in r.stdout):
        pytest.skip("no sanitizer runtime on this machine")
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([os.path.join(asan, "ref_geom_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "geometry sound" in r.stdout and "ERROR" not in r.stderr, r.stdout
