"""Several runs of the allele-specific feature counting over the same reads, from ONE pass over the BAMs.

Step 3 of `xcltk baf` is rarely run once: the same reads are counted under two phasings, a few min_count / min_maf settings,
no_dup_hap on and off, genes and then bins.  Nothing up to the per-molecule alleles depends on any of that, so `afc_variants`
makes one engine, streams the BAMs once, takes the first variant from finish() and every other one from Engine.refold()
(xck_refold: the region stage of the pileup fold again, under new tables), and writes each variant's directory with the writers
`afc_wrapper` uses.  Every directory holds what `afc_wrapper` would have written for that variant.

Single GPU only: a multi-GPU plan places its region masks and contig cuts at ONE table's region boundaries.
"""

import os
from logging import info

import numpy as np

from ... import fc_common as fcc
from ...capi import XCK_MODE_BAF
from .config import Config
from .main import phased_tables, prepare_config, regions_with_snps, write_matrices

# what all variants share (arguments of afc_wrapper), and what a variant may set
COMMON_KEYS = ("sam_fn", "sam_list_fn", "barcode_fn", "sample_ids", "sample_id_fn", "phased_snp_fn", "debug_level", "ncores", "cell_tag",
               "umi_tag", "min_mapq", "min_len", "incl_flag", "excl_flag", "no_orphan")
VARIANT_KEYS = ("out_dir", "region_fn", "phased_snp_fn", "cellsnp_dir", "ref_cell_fn", "min_count", "min_maf", "output_all_reg", "no_dup_hap")


def map_to_universe(universe, snps):
    """Where the SNPs of a variant's own list sit in the universe: -> (index into `universe` per SNP of `snps`, bool per SNP of the
    universe: listed by the variant).  Both are sequences of (chrom, pos, ...).  ValueError when the universe or the variant holds
    a (chrom, pos) twice, or the variant names one the universe does not have."""
    at = {}
    for i, s in enumerate(universe):
        if at.setdefault((s[0], s[1]), i) != i:
            raise ValueError("the SNP universe holds %s:%d twice" % (s[0], s[1]))
    idx = np.zeros(len(snps), dtype=np.int64)
    enabled = np.zeros(len(universe), dtype=bool)
    for k, s in enumerate(snps):
        i = at.get((s[0], s[1]))
        if i is None:
            raise ValueError("SNP %s:%d of a variant is not in the SNP universe" % (s[0], s[1]))
        if enabled[i]:
            raise ValueError("a variant lists SNP %s:%d twice" % (s[0], s[1]))
        idx[k] = i
        enabled[i] = True
    return idx, enabled


def plan_tables(universe, conf):
    """What one prepared Config (prepare_config) counts with on an engine whose SNP table is `universe`: its regions, its own SNP
    list after local phasing, where those SNPs sit in the universe, which of the universe it lists, the universe with this list's
    alleles and haplotype indices, and the exclusion pairs in the universe's numbering.  ValueError as map_to_universe."""
    regions, snps = conf.reg_list, list(conf.snp_list)
    u_idx, enabled = map_to_universe(universe, snps)
    snps, excl = phased_tables(conf, regions, snps, regions_with_snps(regions, snps))
    table = list(universe)
    for i, s in zip(u_idx.tolist(), snps):
        table[i] = tuple(s)
    if excl is not None:
        excl = (np.asarray(excl[0], dtype=np.int32), u_idx[np.asarray(excl[1], dtype=np.int64)].astype(np.int32))
    return dict(conf=conf, regions=regions, snps=snps, u_idx=u_idx, enabled=enabled, table=table, excl=excl)


def refold_plan(eng, p, copy=False):
    """Engine.refold under the tables of one plan_tables() result."""
    conf = p["conf"]
    return eng.refold(p["regions"], snps=p["table"], snp_enabled=None if p["enabled"].all() else p["enabled"],
                      min_count=conf.min_count, min_maf=conf.min_maf, no_dup_hap=conf.no_dup_hap, excl_pairs=p["excl"], copy=copy)


def _variant_conf(common, var):
    for k in common:
        if k not in COMMON_KEYS:
            raise ValueError("afc_variants: '%s' is not an argument all variants share" % k)
    for k in var:
        if k not in VARIANT_KEYS:
            raise ValueError("afc_variants: a variant cannot set '%s'" % k)
    if "region_fn" not in var or "out_dir" not in var:
        raise ValueError("afc_variants: every variant needs out_dir and region_fn")
    conf = Config()
    conf.sam_fn, conf.sam_list_fn = common.get("sam_fn"), common.get("sam_list_fn")
    conf.barcode_fn = common.get("barcode_fn")
    conf.sample_id_str, conf.sample_id_fn = common.get("sample_ids"), common.get("sample_id_fn")
    conf.debug, conf.nproc = common.get("debug_level", 0), common.get("ncores", 1)
    conf.cell_tag, conf.umi_tag = common.get("cell_tag", "CB"), common.get("umi_tag", "UB")
    conf.min_mapq, conf.min_len = common.get("min_mapq", 20), common.get("min_len", 30)
    conf.incl_flag = common.get("incl_flag", 0)
    conf.excl_flag = -1 if common.get("excl_flag") is None else common["excl_flag"]
    conf.no_orphan = common.get("no_orphan", True)
    conf.region_fn, conf.out_dir = var["region_fn"], var["out_dir"]
    conf.snp_fn = var.get("phased_snp_fn", common.get("phased_snp_fn"))
    conf.cellsnp_dir, conf.ref_cell_fn = var.get("cellsnp_dir"), var.get("ref_cell_fn")
    conf.min_count, conf.min_maf = var.get("min_count", 1), var.get("min_maf", 0)
    conf.output_all_reg, conf.no_dup_hap = var.get("output_all_reg", False), var.get("no_dup_hap", True)
    return conf


def afc_variants(common, variants):
    """common: the arguments of afc_wrapper that all variants share (COMMON_KEYS: the BAMs, barcodes / sample IDs, tags, the read
    filters, and phased_snp_fn - the universe of SNPs).  variants: dicts of out_dir and region_fn plus any of VARIANT_KEYS; a
    variant's own phased_snp_fn may be a subset of the universe by (chrom, pos), with its own REF / ALT / haplotype columns - the SNPs
    it leaves out do not count for it.  Raises ValueError before any counting for a position outside the universe, a position the
    universe holds twice, or a multi-GPU environment.  Returns 0."""
    if fcc.dist_requested():
        raise ValueError("afc_variants runs on one GPU: a multi-GPU plan cuts at one table's region boundaries (WORLD_SIZE > 1 or XCK_DIST_FORCE is set)")
    if not variants:
        raise ValueError("afc_variants: no variant given")
    if not common.get("phased_snp_fn"):
        raise ValueError("afc_variants: common['phased_snp_fn'] (the universe of SNPs) is needed")
    loader = fcc.load_snp_from_vcf if fcc.is_vcf_name(common["phased_snp_fn"]) else fcc.load_snp_from_tsv
    universe = loader(common["phased_snp_fn"], verbose=True)
    if not universe:
        raise ValueError("afc_variants: failed to load the SNP universe")
    universe = list(universe)
    plans = []
    for var in variants:
        conf = _variant_conf(common, var)
        if prepare_config(conf) < 0:
            raise ValueError("errcode -2")
        plans.append(plan_tables(universe, conf))
    # the engine is made with the variant that has the most regions: the row field of its keys then fits every table
    first = max(range(len(plans)), key=lambda i: len(plans[i]["regions"]))
    order = [first] + [i for i in range(len(plans)) if i != first]
    p0 = plans[first]
    eng, coo, dist = fcc.make_and_count(p0["conf"], XCK_MODE_BAF, p0["regions"], p0["table"], excl_pairs=p0["excl"])
    try:
        for i in order:
            p = plans[i]
            conf = p["conf"]
            if i != first or not p["enabled"].all():       # (the engine was made with the whole universe enabled)
                coo = refold_plan(eng, p)
                info("[engine] variant %d recounted under its own tables (%d regions)" % (i, len(p["regions"])))
            pre = os.path.join(conf.out_dir, conf.out_prefix)
            fcc.write_summaries(eng, dist, pre, conf.samples, p["regions"])
            # (the variant's own SNPs, in its order: rows of the universe's table)
            fcc.write_snp_summary(eng, dist, pre + "snp_summary.tsv", p["snps"], rows=p["u_idx"])
            write_matrices(conf, eng, dist, p["regions"], coo)
    finally:
        eng.close()
    return 0
