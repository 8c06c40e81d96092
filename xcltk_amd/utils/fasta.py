"""fasta.py - a reference FASTA as the engine takes it (Engine.set_reference, xck_set_contig_ref): the file is
mapped, never parsed - the device packs the text as it lies in the file, driven by the line geometry of the FASTA index.

The index is `<fasta>.fai` when it is there (the five columns of `samtools faidx`: name, length, offset of the first base, bases a line,
bytes a line); otherwise build_index() makes the same five columns in memory by one scan over the line ends.  Nothing is written next
to the input.  Like `samtools faidx` the scan rejects a sequence whose inner lines differ in length: only a sequence's last line may be
shorter.  Compressed input is refused: decompress it first.
"""
import mmap
import os
from collections import namedtuple

import numpy as np

FaiEntry = namedtuple("FaiEntry", "name length offset line_bases line_width")
SCAN_BLOCK = 64 << 20


def offset_of(pos, line_bases, line_width):
    """offset of 0-based position pos from the sequence's first base"""
    return (pos // line_bases) * line_width + pos % line_bases


def read_fai(fai_fn):
    """the entries of a .fai (further columns, as of a FASTQ index, are ignored)"""
    out = []
    with open(fai_fn) as fp:
        for k, line in enumerate(fp):
            f = line.rstrip("\n").split("\t")
            if len(f) < 5:
                if not line.strip():
                    continue
                raise ValueError("%s line %d: a FASTA index line has five columns" % (fai_fn, k + 1))
            out.append(FaiEntry(f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])))
    return out


def build_index(buf):
    """The .fai columns of FASTA text (bytes, or a uint8 array / map of the file), by one scan over its line ends.  ValueError for text in
    front of the first header, a header without a name and a sequence whose lines differ in length other than a shorter last one."""
    buf = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf
    size = len(buf)
    if size == 0:
        return []
    nl = np.concatenate([a + np.flatnonzero(buf[a:a + SCAN_BLOCK] == 10) for a in range(0, size, SCAN_BLOCK)]).astype(np.int64)
    ends = nl if len(nl) and nl[-1] == size - 1 else np.append(nl, size)           # (a last line without a line end)
    starts = np.concatenate([[0], ends[:-1] + 1]).astype(np.int64)
    width = np.minimum(ends + 1, size) - starts
    bases = ends - starts
    bases = bases - ((bases > 0) & (buf[np.maximum(ends - 1, 0)] == 13))           # \r\n
    heads = np.flatnonzero(buf[starts] == ord(">"))
    if len(heads) == 0 or bases[:heads[0]].any():
        raise ValueError("FASTA text in front of the first '>' header")
    out = []
    for k, h in enumerate(heads.tolist()):
        words = bytes(buf[starts[h] + 1:starts[h] + 1 + bases[h]]).split()
        if not words or buf[starts[h] + 1] in (32, 9):
            raise ValueError("a FASTA header without a sequence name at offset %d" % starts[h])
        name = words[0].decode()
        a, b = h + 1, (int(heads[k + 1]) if k + 1 < len(heads) else len(starts))
        nz = np.flatnonzero(bases[a:b])
        if len(nz) == 0:
            out.append(FaiEntry(name, 0, int(starts[a]) if a < len(starts) else size, 0, 0))
            continue
        b = a + int(nz[-1]) + 1                                                    # (empty lines behind the sequence are no part of it)
        lb, lw = int(bases[a]), int(width[a])
        if (bases[a:b - 1] != lb).any() or (width[a:b - 1] != lw).any() or bases[b - 1] > lb:
            raise ValueError("different line length in sequence '%s'" % name)
        out.append(FaiEntry(name, int(bases[a:b].sum()), int(starts[a]), lb, lw))
    return out


def _other_name(x):
    return x[3:] if x.startswith("chr") else "chr" + x


def match_contigs(entries, contig_names, contig_len, want=None):
    """FASTA entries against a handle's contigs, with the chr tolerance of the BAM mapping (the name, then the name with 'chr' added /
    removed).  want: indices of the contigs asked for (None: all).  -> (pairs [(contig index, entry)], missing [contig names] the FASTA
    lacks).  ValueError when a matched contig's length differs from the handle's - another genome build - naming the contig and both."""
    by_name = {}
    for e in entries:
        by_name.setdefault(e.name, e)
    pairs, missing = [], []
    for c in (range(len(contig_names)) if want is None else want):
        x = contig_names[c]
        e = by_name.get(x) or by_name.get(_other_name(x))
        if e is None:
            missing.append(x)
            continue
        if int(e.length) != int(contig_len[c]):
            raise ValueError("contig '%s' has %d positions on the handle and '%s' has %d in the FASTA: another genome build?"
                             % (x, int(contig_len[c]), e.name, int(e.length)))
        pairs.append((int(c), e))
    return pairs, missing


class Fasta:
    """A mapped FASTA file with its index.  span(entry) -> (address, n_raw, line_bases, line_width) of the entry's raw bytes, as
    xck_set_contig_ref takes them; the address is valid until close()."""

    def __init__(self, fasta_fn):
        self.fn = fasta_fn
        with open(fasta_fn, "rb") as fp:
            magic = fp.read(2)
            if magic == b"\x1f\x8b" or fasta_fn.endswith((".gz", ".bgz")):
                raise ValueError("'%s' is compressed: decompress it first (the device packs the FASTA text as it lies in the file)" % fasta_fn)
            if not magic:
                raise ValueError("'%s' is empty" % fasta_fn)
            self.mm = mmap.mmap(fp.fileno(), 0, access=mmap.ACCESS_READ)
        self.buf = np.frombuffer(self.mm, dtype=np.uint8)
        fai = fasta_fn + ".fai"
        self.entries = read_fai(fai) if os.path.isfile(fai) else build_index(self.buf)

    def span(self, e):
        if e.length < 1 or e.line_bases < 1:
            raise ValueError("sequence '%s' of '%s' is empty" % (e.name, self.fn))
        n_raw = min(offset_of(e.length - 1, e.line_bases, e.line_width) + 1, len(self.buf) - e.offset)
        if e.offset < 0 or n_raw < 1:
            raise ValueError("sequence '%s' starts behind the end of '%s': a stale index?" % (e.name, self.fn))
        return self.buf.ctypes.data + e.offset, n_raw, e.line_bases, e.line_width

    def close(self):
        if getattr(self, "mm", None) is not None:
            self.buf = None
            self.mm.close()
            self.mm = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
