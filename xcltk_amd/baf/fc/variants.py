"""Several runs of the allele-specific feature counting over the same reads, from ONE pass over the BAMs.

Step 3 of `xcltk baf` is rarely run once: the same reads are counted under two phasings, a few min_count / min_maf settings,
no_dup_hap on and off, genes and then bins.  Nothing up to the per-molecule alleles depends on any of that, so `afc_variants`
makes one engine, streams the BAMs once, takes the first variant from finish() and every other one from Engine.refold()
(xck_refold: the region stage of the pileup fold again, under new tables), and writes each variant's directory with the writers
`afc_wrapper` uses.  Every directory holds what `afc_wrapper` would have written for that variant.

A variant may also count a subset of the cells (its own barcode_fn or sample_id_fn: the cells that pass QC, one sample of a pooled
run, one clone).  That is a recount too, not a column selection: min_count / min_maf are decided on the allele tallies over the
variant's cells (Engine.refold(cell_enabled=...)).  The engine keeps the common list's columns; renumber_columns() maps them to the
variant's own list, so the directory is the one `afc_wrapper` writes when that list is its barcode file.

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
VARIANT_KEYS = ("out_dir", "region_fn", "phased_snp_fn", "cellsnp_dir", "ref_cell_fn", "min_count", "min_maf", "output_all_reg", "no_dup_hap",
                "barcode_fn", "sample_id_fn")


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


def subset_columns(common, subset):
    """Where the cells of a variant's own list sit in the common one: -> int64 array, per name of `subset` its column in `common`.
    ValueError for a name the common list does not have, or one the subset holds twice."""
    at = {c: i for i, c in enumerate(common)}
    idx = np.zeros(len(subset), dtype=np.int64)
    seen = set()
    for k, c in enumerate(subset):
        if c not in at:
            raise ValueError("afc_variants: cell '%s' of a variant is not in the common barcode / sample list" % c)
        if c in seen:
            raise ValueError("afc_variants: a variant lists cell '%s' twice" % c)
        seen.add(c)
        idx[k] = at[c]
    return idx


def renumber_columns(coo_k, cell_idx, n_cells):
    """One matrix (row, col, val), sorted by (row, col), from the columns of the common cell list to those of a subset of it.
    cell_idx: per cell of the subset its column in the common list (subset_columns); n_cells: the length of the common list.
    Entries of cells outside the subset are dropped (a masked recount holds none).  Where the subset follows the order of the
    common list - always for barcodes, which both runs sort - the map is monotone and the order of the entries stays; otherwise
    the entries are sorted again within their rows.  -> (row, col, val), int32, sorted by (row, col)."""
    cell_idx = np.asarray(cell_idx, dtype=np.int64)
    new_col = np.full(int(n_cells), -1, dtype=np.int32)
    new_col[cell_idx] = np.arange(len(cell_idx), dtype=np.int32)
    row, col, val = (np.asarray(a) for a in coo_k)
    c = new_col[col]
    keep = c >= 0
    row, c, val = row[keep].astype(np.int32), c[keep], val[keep].astype(np.int32)
    if len(cell_idx) > 1 and not (np.diff(cell_idx) > 0).all():
        o = np.lexsort((c, row))
        row, c, val = row[o], c[o], val[o]
    return row, c, val


def _variant_cells(var):
    """The cell list a variant names for itself, in the column order `afc_wrapper` gives it (resolve_inputs: barcodes sorted, sample
    IDs in file order), or None."""
    if var.get("barcode_fn") and var.get("sample_id_fn"):
        raise ValueError("afc_variants: a variant cannot set barcode_fn and sample_id_fn together")
    fn = var.get("barcode_fn") or var.get("sample_id_fn")
    if not fn:
        return None
    if not os.path.isfile(fn):
        raise ValueError("afc_variants: cell list '%s' of a variant does not exist" % fn)
    with fcc.zopen(fn, "rt") as fp:
        names = [x.strip() for x in fp]
    return sorted(names) if var.get("barcode_fn") else names


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
    """Engine.refold under the tables of one plan_tables() result, over the plan's cells (p["cell_idx"], set by afc_variants for a
    variant with a cell list of its own) - the matrices then come back in the columns of that list."""
    conf = p["conf"]
    cell_idx = p.get("cell_idx")
    cell_enabled = None
    if cell_idx is not None:
        cell_enabled = np.zeros(eng.n_cells, dtype=bool)
        cell_enabled[cell_idx] = True
    coo = eng.refold(p["regions"], snps=p["table"], snp_enabled=None if p["enabled"].all() else p["enabled"],
                     min_count=conf.min_count, min_maf=conf.min_maf, no_dup_hap=conf.no_dup_hap, excl_pairs=p["excl"], copy=copy,
                     cell_enabled=cell_enabled)
    if cell_idx is not None:
        coo = {k: renumber_columns(v, cell_idx, eng.n_cells) for k, v in coo.items()}
    return coo


def _variant_conf(common, var):
    for k in common:
        if k not in COMMON_KEYS:
            raise ValueError("afc_variants: '%s' is not an argument all variants share" % k)
    for k in var:
        if k not in VARIANT_KEYS:
            raise ValueError("afc_variants: a variant cannot set '%s'" % k)
    # (the Config carries the COMMON cells: the engine is made with them, and local phasing checks its inputs against them.  A
    #  variant's own cell list is resolved by afc_variants, into the plan.)
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
    it leaves out do not count for it.  A variant's own barcode_fn / sample_id_fn is a subset of the common cells: its directory
    holds what afc_wrapper writes when given that list (and, for sample IDs, the BAMs of those samples) - samples.tsv in the
    subset's order, the columns numbered by it, min_count / min_maf decided over its cells.  Its opt-in cell_summary.tsv is not
    written (the read counters of the handle are those of the common list); local phasing (cellsnp_dir, ref_cell_fn) is checked
    against the common cells, as without a list of its own.  Raises ValueError before any counting for a position outside the
    universe, a position the universe holds twice, a cell outside the common list, or a multi-GPU environment.  Returns 0."""
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
        p = plan_tables(universe, conf)
        cells = _variant_cells(var)
        if cells is not None:
            p["cells"], p["cell_idx"] = cells, subset_columns(conf.samples, cells)
            if fcc.is_writer_rank():
                fcc.write_samples(conf.out_sample_fn, cells)       # (prepare_config wrote the common list)
            groups = fcc.load_cell_groups(cells)                   # XCK_CELL_GROUPS: as a run with this list numbers them, over the engine's columns
            if groups is not None:
                full = np.full(len(conf.samples), -1, dtype=np.int32)
                full[p["cell_idx"]] = groups[1]
                conf.cell_groups = (groups[0], full)
        plans.append(p)
    # the engine is made with the variant that has the most regions: the row field of its keys then fits every table
    first = max(range(len(plans)), key=lambda i: len(plans[i]["regions"]))
    order = [first] + [i for i in range(len(plans)) if i != first]
    p0 = plans[first]
    eng, coo, dist = fcc.make_and_count(p0["conf"], XCK_MODE_BAF, p0["regions"], p0["table"], excl_pairs=p0["excl"])
    try:
        for i in order:
            p = plans[i]
            conf = p["conf"]
            subset = p.get("cell_idx") is not None
            if i != first or not p["enabled"].all() or subset:     # (the engine was made with the whole universe and every cell enabled)
                coo = refold_plan(eng, p)
                info("[engine] variant %d recounted under its own tables (%d regions%s)" %
                     (i, len(p["regions"]), ", %d of %d cells" % (len(p["cells"]), eng.n_cells) if subset else ""))
            pre = os.path.join(conf.out_dir, conf.out_prefix)
            if subset:
                fcc.write_read_summary(eng, dist, pre + "read_summary.tsv")
                fcc.write_feature_summary(eng, dist, pre + "feature_summary.tsv", p["regions"])
            else:
                fcc.write_summaries(eng, dist, pre, conf.samples, p["regions"])
            # (the variant's own SNPs, in its order: rows of the universe's table)
            fcc.write_snp_summary(eng, dist, pre + "snp_summary.tsv", p["snps"], rows=p["u_idx"])
            write_matrices(conf, eng, dist, p["regions"], coo, n_cols=len(p["cells"]) if subset else None)
    finally:
        eng.close()
    return 0
