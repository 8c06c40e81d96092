"""What the reference-sequence tests share (tests/test_refseq_cases_host.py on the CPU, tests/test_gpu_refseq.py on the GPU): FASTA texts
of every line geometry, a second statement of where a position lies in them and of what the device packs (xck_set_contig_ref,
csrc/ref_geom.h), and a second statement of the rule that orients a candidate by the genome's base
(xck_find_candidates_ref, csrc/base_tally.h bt_candidate_ref).

  fasta_text() / plain_parse()   a FASTA file of several sequences with its literal .fai lines; the same text read line by line
  offset() / packed_letters()    the offset formula and the letters xck_get_contig_ref must return, read through the formula alone
  chunks()                       the staging chunks of a contig under a chunk size (rg_chunk_end), with what their last byte is
  orient() / candidates_ref()    the rule on one position; model tallies + genome letters -> what Engine.find_candidates(use_ref=True) returns
  genome()                       five genomes made from tallies: the majority base, the second base, a third base, all N, a mix
Nothing here calls the product library."""
import numpy as np

import base_tally_cases as BT

LETTERS = "=ACMGRSVTWYHKDBN"
BASES = BT.BASES
CLASSES = ("ref_major", "ref_minor", "ref_unsupported", "ref_unknown")
MIN_CHUNK = 64

LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 2049)
EOLS = ("\n", "\r\n")
# every letter in both cases, and bytes that must read as N
ALPHABET = "ACGTN" + "acgtn" + "MRSVWYHKDB" + "mrsvwyhkdb" + "=*-.U7"


def line_bases_of(length):
    return sorted({1, 3, 8, 60, length, length + 5})


def grid():
    """(length, line_bases, eol, final newline, place of the contig among three) of every pack case"""
    return [(n, lb, eol, fin, place) for n in LENGTHS for lb in line_bases_of(n) for eol in EOLS for fin in (False, True) for place in (0, 1, 2)]


# ----------------------------------------------------------------------------- FASTA text
def seq_letters(n, seed=0, alphabet=ALPHABET):
    return "".join(alphabet[(7 * p + seed) % len(alphabet)] for p in range(n))


def fasta_text(seqs, line_bases, eol="\n", final_newline=True):
    """seqs: [(name, letters)] -> (bytes of the file, [(name, length, offset, line_bases, line_width)] as a .fai holds them)"""
    out, fai = b"", []
    for k, (name, s) in enumerate(seqs):
        out += (">%s some description%s" % (name, eol)).encode()
        fai.append((name, len(s), len(out), line_bases, line_bases + len(eol)))
        lines = [s[a:a + line_bases] for a in range(0, len(s), line_bases)]
        out += eol.join(lines).encode()
        if k + 1 < len(seqs) or final_newline:
            out += eol.encode()
    return out, fai


def fai_text(fai):
    return "".join("%s\t%d\t%d\t%d\t%d\n" % e for e in fai)


def plain_parse(text):
    """{name: letters} of FASTA bytes, line by line"""
    out, name = {}, None
    for line in text.decode().split("\n"):
        line = line.rstrip("\r")
        if line.startswith(">"):
            name = line[1:].split()[0]
            out[name] = ""
        elif name is not None:
            out[name] += line
    return out


def three(length, line_bases, eol, final_newline, place, seed=0):
    """the grid's file: three sequences, the one under test (`length` letters) at `place` -> (text, fai, index of the contig, its letters)"""
    seqs = []
    for k in range(3):
        n = length if k == place else (11, 70, 23)[k]
        seqs.append(("s%d" % k, seq_letters(n, seed + k + length)))
    text, fai = fasta_text(seqs, line_bases, eol, final_newline)
    return text, fai, place, seqs[place][1]


# ----------------------------------------------------------------------------- the geometry
def offset(p, line_bases, line_width):
    return (p // line_bases) * line_width + p % line_bases


def code_letter(byte):
    """the letter the packed sequence holds for a FASTA byte: one of the 15 letters behind '=' in upper case, else N"""
    c = chr(byte).upper() if byte < 128 else "?"
    return c if c in LETTERS[1:] else "N"


def packed_letters(raw, length, line_bases, line_width):
    """raw: the file's bytes from the contig's first base on"""
    return "".join(code_letter(raw[offset(p, line_bases, line_width)]) for p in range(length))


def raw_span(text, entry):
    """the bytes xck_set_contig_ref takes for a .fai entry: first base through last base"""
    _, length, off, lb, lw = entry
    return text[off:off + offset(length - 1, lb, lw) + 1]


def chunks(length, line_bases, line_width, chunk_bytes):
    """[(p0, p1, first raw offset, one past the last)] of the staging chunks: a chunk starts at a multiple of 8 and takes the positions whose
    bytes fit into chunk_bytes, cut down to a multiple of 8 unless the contig ends there (at least 8 positions)"""
    def pos_below(r):
        return (r // line_width) * line_bases + min(r % line_width, line_bases)
    out, p0 = [], 0
    while p0 < length:
        p1 = pos_below(offset(p0, line_bases, line_width) + chunk_bytes)
        if p1 >= length:
            p1 = length
        else:
            p1 &= ~7
            if p1 <= p0:
                p1 = min(p0 + 8, length)
        out.append((p0, p1, offset(p0, line_bases, line_width), offset(p1 - 1, line_bases, line_width) + 1))
        p0 = p1
    return out


# ----------------------------------------------------------------------------- the rule
def orient(c, g, min_count, min_maf):
    """counts (A, C, G, T), the genome's letter -> (class or None, ref letter, alt letter).  ref_major / ref_minor are written."""
    c = [int(x) for x in c]
    g = g.upper()                                                         # (lower case packs as upper case)
    parent, pref, _ = BT.candidate(c, min_count, min_maf)
    if g not in BASES:
        return ("ref_unknown" if parent else None), None, None
    ref = BASES.index(g)
    alt = max((b for b in range(4) if b != ref), key=lambda b: (c[b], -b))
    n, m = sum(c), min(c[ref], c[alt])
    if m > 0 and not (float(n) < float(min_count)) and not (float(m) < float(n) * float(min_maf)):
        return ("ref_major" if BASES[ref] == pref else "ref_minor"), BASES[ref], BASES[alt]
    return ("ref_unsupported" if parent else None), None, None


def candidates_ref(tally, genomes, min_count, min_maf):
    """model tallies {contig: [len, 4]}, genomes {contig: letters, or None: no sequence loaded} -> Engine.find_candidates(use_ref=True)'s dict"""
    out = dict(contig=[], pos=[], ref=[], alt=[], count=[])
    st = dict.fromkeys(CLASSES, 0)
    covered = 0
    for c in sorted(tally):
        t, g = tally[c], genomes.get(c)
        for p in np.flatnonzero(t.sum(axis=1)).tolist():
            covered += 1
            cls, ref, alt = orient(t[p], g[p] if g is not None else "N", min_count, min_maf)
            if cls:
                st[cls] += 1
            if cls in ("ref_major", "ref_minor"):
                out["contig"].append(c); out["pos"].append(p + 1); out["ref"].append(ref); out["alt"].append(alt); out["count"].append(t[p].tolist())
    return dict(contig=np.array(out["contig"], np.int32), pos=np.array(out["pos"], np.int32), ref=np.array(out["ref"], dtype="U1"),
                alt=np.array(out["alt"], dtype="U1"), count=np.array(out["count"], np.uint32).reshape(-1, 4), positions_covered=covered, ref_stats=st)


GENOMES = ("major", "second", "third", "N", "mix")


def _ranked(t):
    """per position the four bases by (count descending, A C G T): [:, 0] the plain rule's ref, [:, 1] its alt"""
    return np.argsort(-np.asarray(t, dtype=np.int64).reshape(-1, 4), axis=1, kind="stable")


def genome(t, kind):
    """letters for a contig from its model tally [len, 4].  major: the base with the largest count; second: the plain rule's alt; third:
    the base with the smallest count (below the second, or absent); N; mix: those four by pos % 4, with lower case and an IUPAC letter"""
    r = _ranked(t)
    p = np.arange(len(r))
    col = {"major": np.zeros_like(p), "second": np.ones_like(p), "third": np.full_like(p, 3), "N": np.full_like(p, -1), "mix": np.array([0, 1, 3, -1])[p % 4]}[kind]
    x = np.where(col < 0, "N", np.array(list(BASES))[r[p, np.maximum(col, 0)]])
    if kind == "mix":
        x = np.where(p % 8 == 7, "R", np.where(p % 3 == 0, np.char.lower(x), x))
    return "".join(x.tolist())


def e2e_genome(t, min_count, min_maf):
    """the end-to-end tests' genome: the majority base at the plain rule's candidates of even rank, the second base at those of odd rank,
    N at every seventh; the majority base elsewhere"""
    t = np.asarray(t, dtype=np.int64).reshape(-1, 4)
    r = _ranked(t)
    n, m = t.sum(axis=1), np.take_along_axis(t, r[:, 1:2], axis=1)[:, 0]
    cand = (m > 0) & ~(n.astype(np.float64) < float(min_count)) & ~(m.astype(np.float64) < n.astype(np.float64) * float(min_maf))
    k = np.cumsum(cand) - 1                                               # the candidate's rank
    col = np.where(cand, k % 2, 0)
    x = np.array(list(BASES))[r[np.arange(len(r)), col]]
    x = np.where(cand & (k % 7 == 3), "N", x)
    return "".join(x.tolist())


def vcf_text_ref(chroms, cand, fasta_fn):
    """the VCF discover_snps(refseq_fn=) writes: the plain file's header with one more line, INFO by the written orientation"""
    return BT.vcf_text(chroms, cand).replace("#CHROM", "##reference=%s\n#CHROM" % fasta_fn, 1)
