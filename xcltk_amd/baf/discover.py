"""discover.py - candidate SNPs from the BAMs alone: the first half of cellsnp-lite's "mode 2b" on the engine.

Every BAF path starts from a SNP list: pileup() of genotype.py needs `snp_vcf_fn`, the reference hands the question to
`cellsnp-lite -R <panel VCF>`.  Without a panel the usual way is to pile up every covered position of the pseudo-bulk and keep the
positions that pass minCOUNT / minMAF.  discover_snps() does that with one BAF handle that has no SNPs and no regions and keeps base
tallies (Engine(base_tally=True), XCK_F_BASE_TALLY): the BAMs are streamed once, every aligned base of every read that passes the read
filter adds to the A / C / G / T counters of its reference position, and xck_find_candidates picks the positions.  The VCF it writes is
what pileup(snp_vcf_fn=...) takes, and that step then applies the molecule-level counts and filter_snps to the candidates.

Reads are counted here, not molecules (UMIs): a genome-wide molecule dedup would need a sort of every aligned base.  Without a reference
genome REF of a line is the base with the largest count and ALT the largest of the others (ties: the earliest of A, C, G, T).  With one
(refseq_fn, -f / --refseq: cellsnp-lite's -f) the sequence of the contigs that have reads is packed on the device
and REF is the genome's base, as phasing against a reference panel needs it: ALT is the largest of the other three, a position whose
genome base is N or whose genome base the reads do not support is not written, and the log says how many lines that turned round.
Memory: 16 bytes of device memory per position of every contig that has reads, half a byte more with a reference.  Single GPU only.
"""
import argparse
import sys
from logging import info

import numpy as np

from .. import fc_common as fcc
from ..capi import XCK_E_CAPACITY, XCK_F_FORCE_KEY128, XCK_MODE_BAF, bam_references
from ..engine import Engine, XckError
from ..utils.zfile import ZF_F_BGZIP, zopen
from .genotype import VCF_HEADER

BASES = "ACGT"


def candidate_vcf_text(names, cand, refseq_fn=None):
    """The VCF text of a candidate list: names[contig] as the BAM names them, cand = dict(contig, pos, ref, alt, count [n, 4]) in
    (contig, pos) order.  INFO: AD = the ALT count, DP = REF + ALT, OTH = the other two bases.  refseq_fn: the reference the
    candidates were oriented by, named in one more header line."""
    lines = []
    count = np.asarray(cand["count"], dtype=np.int64).reshape(-1, 4)
    for i in range(len(cand["pos"])):
        ref, alt = str(cand["ref"][i]), str(cand["alt"][i])
        r, a, n = int(count[i, BASES.index(ref)]), int(count[i, BASES.index(alt)]), int(count[i].sum())
        lines.append("%s\t%d\t.\t%s\t%s\t.\tPASS\tAD=%d;DP=%d;OTH=%d\n" % (names[int(cand["contig"][i])], int(cand["pos"][i]), ref, alt, a, r + a, n - r - a))
    return VCF_HEADER + ("##reference=%s\n" % refseq_fn if refseq_fn else "") + "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n" + "".join(lines)


def write_candidate_vcf(out_vcf_fn, names, cand, refseq_fn=None):
    """candidate_vcf_text() to a file, bgzip-compressed when the name ends in .gz -> number of lines written"""
    text = candidate_vcf_text(names, cand, refseq_fn)
    gz = out_vcf_fn.endswith(".gz")
    with zopen(out_vcf_fn, "wb" if gz else "w", ZF_F_BGZIP if gz else None, is_bytes=gz) as fp:
        fp.write(text.encode("utf8") if gz else text)
    return len(cand["pos"])


def discover_snps(sam_fn=None, sam_list_fn=None, barcode_fn=None, sample_id_fn=None, out_vcf_fn=None, min_count=20, min_maf=0.1,
                  cell_tag="CB", umi_tag="UB", min_mapq=20, min_len=30, incl_flag=0, excl_flag=-1, no_orphan=True, ncores=1, refseq_fn=None):
    """Candidate SNPs of the pseudo-bulk of one BAM (sam_fn; several with commas) or a list file (sam_list_fn), cells from barcode_fn
    (droplet) or sample_id_fn (one BAM per cell), written to out_vcf_fn.  A read counts when it passes the read filter the other
    commands use (min_mapq, min_len, flags, orphans, a listed cell, a UMI where umi_tag is set); min_count / min_maf as
    Engine.find_candidates().  excl_flag < 0: the command's default for the UMI setting.  Returns (#candidates, stats) with stats =
    Engine.base_tally_stats() + positions_covered.  refseq_fn: a reference FASTA (indexed by <fasta>.fai, or scanned); the sequence
    of the contigs that have reads is loaded behind the pass (Engine.set_reference), the candidates are oriented by it
    (Engine.find_candidates(use_ref=True)), the VCF names it in a ##reference line, and stats gains ref_major, ref_minor,
    ref_unsupported, ref_unknown, ref_contigs (loaded) and ref_contigs_missing.  ValueError for invalid inputs, a reference of another
    genome build (a contig's length differs) and under a multi-GPU context."""
    if fcc.dist_requested():
        raise ValueError("discover_snps runs on one GPU: with contigs cut over ranks the reads near a cut are fed to both neighbours and would be "
                         "tallied twice; run it as a single process.")
    if not out_vcf_fn:
        raise ValueError("out_vcf_fn is needed")
    conf = type("DiscoverConf", (), {})()
    conf.sam_fn, conf.sam_list_fn, conf.barcode_fn, conf.sample_id_fn, conf.sample_id_str = sam_fn, sam_list_fn, barcode_fn, sample_id_fn, None
    conf.cell_tag = None if str(cell_tag) == "None" else cell_tag
    conf.umi_tag = None if str(umi_tag) == "None" else umi_tag
    conf.excl_flag, conf.debug, conf.nproc = int(excl_flag), 0, ncores
    conf.use_barcodes = lambda: conf.cell_tag is not None
    conf.use_umi = lambda: conf.umi_tag is not None
    conf.defaults = type("D", (), dict(UMI_TAG_BC="UB"))()
    if fcc.resolve_inputs(conf) < 0 or fcc.resolve_tags(conf) < 0:
        raise ValueError("invalid discover inputs")
    # contigs as the first BAM names them (the other BAMs are mapped by name, with the usual chr tolerance)
    refs = bam_references(conf.sam_fn_list[0])
    names, lengths = [n for n, _ in refs], [max(1, int(l)) for _, l in refs]
    if not names:
        raise ValueError("'%s' names no reference sequence" % conf.sam_fn_list[0])
    flags = 0
    while True:
        eng = Engine(XCK_MODE_BAF, names, [], len(conf.samples), snps=[], barcodes=conf.barcodes if conf.use_barcodes() else None,
                     cell_tag=conf.cell_tag, umi_tag=conf.umi_tag, min_mapq=min_mapq, min_len=min_len, incl_flag=incl_flag,
                     excl_flag=conf.excl_flag, no_orphan=no_orphan, n_threads=max(0, int(ncores)), flags=flags, base_tally=True, contig_len=lengths)
        try:
            try:
                n_rec = eng.ingest_bams(list(conf.sam_fn_list))
            except XckError as e:                                     # ids of non-ACGT keys outgrew the 64-bit layout: once more with 128-bit keys
                if getattr(e, "code", 0) == XCK_E_CAPACITY and not flags & XCK_F_FORCE_KEY128:
                    flags |= XCK_F_FORCE_KEY128
                    continue
                raise
            eng.finish()
            ref = eng.set_reference(refseq_fn) if refseq_fn else None
            cand = eng.find_candidates(min_count, min_maf, use_ref=bool(refseq_fn))
            stats = dict(eng.base_tally_stats(), positions_covered=cand["positions_covered"])
            if ref is not None:
                stats.update(cand["ref_stats"], ref_contigs=ref["loaded"], ref_contigs_missing=ref["missing"])
        finally:
            eng.close()
        break
    n = write_candidate_vcf(out_vcf_fn, names, cand, refseq_fn)
    info("[discover] %d BAM record(s), %d read(s) tallied, %d aligned base(s) on %d position(s): %d candidate SNP(s) (min_count %s, min_maf %s) -> %s"
         % (n_rec, stats["reads_tallied"], stats["bases_tallied"], stats["positions_covered"], n, min_count, min_maf, out_vcf_fn))
    if refseq_fn:
        info("[discover] oriented by %s: REF is the majority base at %d, the minority base at %d; left out: %d not supported by the reads, %d with no A/C/G/T in the reference"
             % (refseq_fn, stats["ref_major"], stats["ref_minor"], stats["ref_unsupported"], stats["ref_unknown"]))
    return n, stats


USAGE = """
Usage:   xcltk discover [options]

Candidate SNPs from the BAMs alone (pseudo-bulk pileup of every covered position, reads counted): the VCF that
`xcltk baf` / pileup() take as their SNP list.  Single GPU.

Options:
  -s, --sam FILE         Comma separated indexed BAM file(s).
  -S, --samList FILE     A list file containing BAM files, each per line.
  -b, --barcode FILE     A plain file listing all effective cell barcodes (droplet data).
  -i, --sampleList FILE  A list file containing sample IDs, each per line (one BAM per cell).
  -O, --outVCF FILE      Output VCF (bgzip-compressed when the name ends in .gz).
  -f, --refseq FILE      Reference genome FASTA (plain text; FILE.fai is used when it is there): REF of every line is the
                         genome's base.  Without it REF is the base with the largest count.
  --minCOUNT INT         Minimum aggregated count of a position [20]
  --minMAF FLOAT         Minimum minor allele fraction of a position [0.1]
  --cellTAG STR          Tag for cell barcodes, set to None when using sample IDs [CB]
  --UMItag STR           Tag for UMI, set to None when reads only [UB]
  --minMAPQ INT          Minimum MAPQ for read filtering [20]
  --minLEN INT           Minimum mapped length for read filtering [30]
  --inclFLAG INT         Required flags: skip reads with all mask bits unset [0]
  --exclFLAG INT         Filter flags: skip reads with any mask bits set [772 with UMIs, 1796 without]
  --countORPHAN          If use, do not skip anomalous read pairs.
  -p, --ncores INT       Number of decoder threads [1]
  -h, --help             Print this message and exit.
"""


def discover_main(argv):
    """`xcltk discover`: argv as sys.argv (program, command, options)"""
    if len(argv) <= 2 or argv[2] in ("-h", "--help"):
        sys.stdout.write(USAGE)
        sys.exit(0)
    ap = argparse.ArgumentParser(prog="xcltk discover", add_help=False)
    ap.add_argument("-s", "--sam"); ap.add_argument("-S", "--samList"); ap.add_argument("-b", "--barcode"); ap.add_argument("-i", "--sampleList")
    ap.add_argument("-O", "--outVCF", required=True); ap.add_argument("-f", "--refseq")
    ap.add_argument("--minCOUNT", type=float, default=20); ap.add_argument("--minMAF", type=float, default=0.1)
    ap.add_argument("--cellTAG", default="CB"); ap.add_argument("--UMItag", default="UB")
    ap.add_argument("--minMAPQ", type=int, default=20); ap.add_argument("--minLEN", type=int, default=30)
    ap.add_argument("--inclFLAG", type=int, default=0); ap.add_argument("--exclFLAG", type=int, default=-1)
    ap.add_argument("--countORPHAN", action="store_true"); ap.add_argument("-p", "--ncores", type=int, default=1)
    a = ap.parse_args(argv[2:])
    try:
        n, _ = discover_snps(sam_fn=a.sam, sam_list_fn=a.samList, barcode_fn=a.barcode, sample_id_fn=a.sampleList, out_vcf_fn=a.outVCF,
                             min_count=a.minCOUNT, min_maf=a.minMAF, cell_tag=a.cellTAG, umi_tag=a.UMItag, min_mapq=a.minMAPQ, min_len=a.minLEN,
                             incl_flag=a.inclFLAG, excl_flag=a.exclFLAG, no_orphan=not a.countORPHAN, ncores=a.ncores, refseq_fn=a.refseq)
    except (ValueError, XckError) as e:
        sys.stderr.write("Error: %s\n" % e)
        return 1
    sys.stdout.write("%d candidate SNP(s) written to %s\n" % (n, a.outVCF))
    return 0
