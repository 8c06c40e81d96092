"""`xcltk baf` from ONE pass over the BAMs (opt-in: XCK_BAF_ONE_PASS=1; baf/pipeline.py pipeline_wrapper).

The default pipeline reads every BAM twice: step 1 (genotype.pileup) counts the candidate SNPs per cell on a handle of one-base
features, step 3 (afc_wrapper) makes a second handle and streams the same reads again - same read filters, same cells, a subset
of the same SNP positions.  Here one BAF engine is made with the step-3 regions and the candidate SNPs as its SNP table (alleles of
the candidate VCF, REF on haplotype 0, ALT on 1, as genotype.py counts them), the BAMs are streamed once, and after finish()
  - Engine.snp_counts() gives the SNP x cell matrices of step 1 (xck_snp_counts), written with genotype._write_pileup_dirs;
  - step 3's prepare_config / phased_tables run on that directory (local phasing on the host, or on the device with XCK_DEVICE_PHASING=1);
  - Engine.refold() recounts under the phased list - its entries mapped into the candidates, the others disabled - and the result
    is written by the writers afc_wrapper uses.
Both directories hold what the two-pass pipeline writes.

fallback_reason() names the cases in which the two-pass path runs instead; pipeline_wrapper then carries on as if the switch were off.
"""
import os
from logging import error, info

from .. import fc_common as fcc
from ..capi import XCK_MODE_BAF
from ..engine import XckError
from ..utils.grange import format_chrom

SUMMARY_KNOBS = ("XCK_READ_FATE", "XCK_CELL_SUMMARY", "XCK_FEATURE_SUMMARY")
# what both steps resolve from their arguments and must agree on: one pass serves both only then
SHARED = ("sam_fn_list", "samples", "barcodes", "cell_tag", "umi_tag", "min_mapq", "min_len", "incl_flag", "excl_flag", "no_orphan")


def shared_settings(conf):
    """The read filters, tags, cells and BAM list a resolved configuration counts with."""
    return {k: getattr(conf, k) for k in SHARED}


def fallback_reason(dist_requested, snp_vcf_fn, phased_snp_fn, cand=None, phased=None, step1=None, step3=None, env=None):
    """Why `xcltk baf` cannot run from one pass, or None.  Pure: dist_requested (bool: a multi-GPU environment), the two file names,
    cand / phased (sequences of (chrom, pos, ...), chromosome names stripped of 'chr'; None = not loaded yet), step1 / step3
    (shared_settings() of the two steps; None = not resolved yet), env (a mapping, os.environ by default)."""
    env = os.environ if env is None else env
    if dist_requested:
        return "a multi-GPU environment (SNP rows have no owner rank across a contig cut)"
    if snp_vcf_fn is None:
        return "no candidate SNP VCF (snp_vcf_fn is None): there is no step 1"
    if phased_snp_fn is None:
        return "no phased SNP list: there is no step 3"
    for k in SUMMARY_KNOBS:
        if env.get(k, "0") not in ("", "0"):
            return "%s is on: step 1's summaries describe a handle of one-base features" % k
    if cand is not None:
        seen = set()
        for s in cand:
            if (s[0], s[1]) in seen:
                return "%s:%d appears twice in the candidate SNPs" % (s[0], s[1])
            seen.add((s[0], s[1]))
        if phased is not None:
            for s in phased:
                if (s[0], s[1]) not in seen:
                    return "phased SNP %s:%d is not among the candidate SNPs" % (s[0], s[1])
    if step1 is not None and step3 is not None:
        for k in SHARED:
            if step1.get(k) != step3.get(k):
                return "steps 1 and 3 resolve different %s" % ("cell lists" if k in ("samples", "barcodes") else "BAM lists" if k == "sam_fn_list" else "read filters / tags (%s)" % k)
    return None


def run(sam_fn, sam_list_fn, barcode_fn, sample_id_fn, sample_id, mode, snp_vcf_fn, cell_tag, umi_tag, min_count, min_maf, ncores, step3):
    """The pipeline of pipeline_wrapper from one pass; step3 = the keyword arguments pipeline_wrapper gives afc_wrapper
    (pipeline.step3_arguments: regions, phased list, the two directories, step 3's fixed filters).  -> its return code (0 / -1), or
    None when the two-pass path has to run: one `info` line then names the reason, and nothing has been written."""
    region_fn, phased_snp_fn, fc_dir, pileup_dir = step3["region_fn"], step3["phased_snp_fn"], step3["out_dir"], step3["cellsnp_dir"]
    from . import genotype as G
    from .fc import main as M
    from .fc.variants import plan_tables, refold_plan

    def fall_back(reason):
        info("one-pass baf: falling back to the two-pass pipeline: %s." % reason)
        return None
    reason = fallback_reason(fcc.dist_requested(), snp_vcf_fn, phased_snp_fn)
    if reason:
        return fall_back(reason)
    for fn in (snp_vcf_fn, phased_snp_fn, region_fn):
        if not fn or not os.path.isfile(fn):
            return fall_back("input file '%s' does not exist" % fn)
    try:
        conf1 = G.pileup_conf(sam_fn, sam_list_fn, barcode_fn, sample_id_fn, sample_id, mode, cell_tag, umi_tag, ncores)
    except ValueError as e:
        return fall_back("step 1 does not resolve its inputs (%s)" % e)
    conf3 = M.afc_conf(**step3)                                            # step 3 exactly as pipeline_wrapper calls it
    if fcc.resolve_inputs(conf3) < 0 or fcc.resolve_tags(conf3) < 0:
        return fall_back("step 3 does not resolve its inputs")
    cand = G.load_candidate_snps(snp_vcf_fn)
    loader = fcc.load_snp_from_vcf if fcc.is_vcf_name(phased_snp_fn) else fcc.load_snp_from_tsv
    phased = loader(phased_snp_fn, verbose=False)
    regions = fcc.load_region_from_txt(region_fn, verbose=False)
    if not cand or not phased or not regions:
        return fall_back("an input table is empty or does not load")
    table = [(format_chrom(c), p, r, a, 0, 1) for c, p, r, a in cand]      # REF on haplotype 0, ALT on 1, as genotype.pileup counts
    reason = fallback_reason(False, snp_vcf_fn, phased_snp_fn, table, list(phased), shared_settings(conf1), shared_settings(conf3))
    if reason:
        return fall_back(reason)
    info("one-pass baf: %d candidate SNPs, %d phased SNPs, %d regions, %d cells." % (len(table), len(phased), len(regions), len(conf3.samples)))
    conf3.reg_list = regions
    try:
        groups = fcc.load_cell_groups(conf3.samples, "[onepass]")          # (XCK_CELL_GROUPS only; a bad file ends the run before any BAM is opened)
    except ValueError as e:
        error("one-pass baf: %s" % e)
        return -1
    try:
        eng, _, dist = fcc.make_and_count(conf3, XCK_MODE_BAF, regions, table, log_prefix="[onepass]")
    except (ValueError, XckError) as e:
        error("one-pass baf: counting failed: %s" % e)
        return -1
    try:
        # step 1: the SNP x cell matrices of the pass, into the directories genotype.pileup writes
        coo = eng.snp_counts()
        if groups is not None:                                            # the same blocks summed per cell group, while they are in HBM
            groups = (groups[0], eng.group_counts(groups[1], n_groups=max(len(groups[0]), 1), source="snp"))
        vcf, p_raw, p_new = G._write_pileup_dirs(pileup_dir, cand, conf1.samples, coo, min_count, min_maf, groups)
        info("pileup #SNP raw=%d; post-filtering=%d." % (p_raw, p_new))
        info("pileup VCF is '%s'." % vcf)
        # step 3: its own preparation on that directory, then the recount under the phased list
        info("BAF feature counting ...")
        if M.prepare_config(conf3) < 0:
            raise ValueError("errcode -2")
        plan = plan_tables(table, conf3)
        coo = refold_plan(eng, plan)
        M.write_matrices(conf3, eng, dist, plan["regions"], coo)
        info("feature BAFs are at '%s'." % fc_dir)
    except (ValueError, IOError, OSError, XckError) as e:
        error("one-pass baf failed: %s" % e)
        return -1
    finally:
        eng.close()
    return 0
