"""Allele-specific feature counting (pileup at phased het SNPs) on the MI355X engine.

Drop-in for xcltk/baf/fc/main.py: `afc_wrapper` keeps the reference signature (:32-77) and
produces xcltk.region.tsv, xcltk.samples.tsv, xcltk.{AD,DP,OTH}.mtx (:373-379).  The per-SNP
pysam pileup of plp_snp()/fc_fet1() (baf/fc/core.py:143-247) runs as HIP kernels
(csrc/engine.hip) behind the C-ABI of include/xck.h.

Region-wise local phasing from a cellsnp-lite pileup (`cellsnp_dir` / `ref_cell_fn`,
baf/fc/main.py:107-153) runs on the host before the counting (baf/fc/phasing.py, baf/localphase.py):
it changes the haplotype index of SNP alleles and drops uncovered SNPs from region lists; the
engine then counts with that phase.  XCK_DEVICE_PHASING=1 phases the regions on the GPU instead (baf/fc/phasing_dev.py).
"""

import os
import sys
from logging import error, info
from logging import warning as warn

import numpy as np

from ... import fc_common as fcc
from ...capi import XCK_MODE_BAF
from .config import Config


def afc_wrapper(sam_fn, barcode_fn, region_fn, phased_snp_fn, out_dir, sam_list_fn=None,
                sample_ids=None, sample_id_fn=None, debug_level=0, ncores=1, cellsnp_dir=None,
                ref_cell_fn=None, cell_tag="CB", umi_tag="UB", min_count=1, min_maf=0,
                output_all_reg=False, no_dup_hap=True, min_mapq=20, min_len=30, incl_flag=0,
                excl_flag=None, no_orphan=True):
    conf = afc_conf(sam_fn=sam_fn, barcode_fn=barcode_fn, region_fn=region_fn, phased_snp_fn=phased_snp_fn, out_dir=out_dir,
                    sam_list_fn=sam_list_fn, sample_ids=sample_ids, sample_id_fn=sample_id_fn, debug_level=debug_level, ncores=ncores,
                    cellsnp_dir=cellsnp_dir, ref_cell_fn=ref_cell_fn, cell_tag=cell_tag, umi_tag=umi_tag, min_count=min_count,
                    min_maf=min_maf, output_all_reg=output_all_reg, no_dup_hap=no_dup_hap, min_mapq=min_mapq, min_len=min_len,
                    incl_flag=incl_flag, excl_flag=excl_flag, no_orphan=no_orphan)
    return fcc.run_logged(afc_core, conf)


def afc_conf(sam_fn, barcode_fn, region_fn, phased_snp_fn, out_dir, sam_list_fn=None, sample_ids=None, sample_id_fn=None, debug_level=0,
             ncores=1, cellsnp_dir=None, ref_cell_fn=None, cell_tag="CB", umi_tag="UB", min_count=1, min_maf=0, output_all_reg=False,
             no_dup_hap=True, min_mapq=20, min_len=30, incl_flag=0, excl_flag=None, no_orphan=True):
    """The Config of one afc_wrapper call, not yet resolved (prepare_config)."""
    conf = Config()
    conf.sam_fn, conf.sam_list_fn = sam_fn, sam_list_fn
    conf.barcode_fn, conf.region_fn, conf.snp_fn = barcode_fn, region_fn, phased_snp_fn
    conf.sample_id_str, conf.sample_id_fn = sample_ids, sample_id_fn
    conf.out_dir, conf.debug = out_dir, debug_level
    conf.cellsnp_dir, conf.ref_cell_fn = cellsnp_dir, ref_cell_fn
    conf.cell_tag, conf.umi_tag = cell_tag, umi_tag
    conf.nproc = ncores
    conf.min_count, conf.min_maf = min_count, min_maf
    conf.output_all_reg, conf.no_dup_hap = output_all_reg, no_dup_hap
    conf.min_mapq, conf.min_len = min_mapq, min_len
    conf.incl_flag = incl_flag
    conf.excl_flag = -1 if excl_flag is None else excl_flag
    conf.no_orphan = no_orphan
    return conf


def prepare_config(conf):
    if fcc.resolve_inputs(conf) < 0:
        return -1
    if not conf.out_dir:
        error("out dir needed!")
        return -1
    os.makedirs(conf.out_dir, exist_ok=True)          # every rank may get here first in a multi-GPU run
    pre = os.path.join(conf.out_dir, conf.out_prefix)
    conf.out_region_fn, conf.out_sample_fn = pre + "region.tsv", pre + "samples.tsv"
    conf.out_ad_fn, conf.out_dp_fn, conf.out_oth_fn = pre + "AD.mtx", pre + "DP.mtx", pre + "OTH.mtx"
    if not conf.region_fn:
        error("region file needed!")
        return -1
    if not os.path.isfile(conf.region_fn):
        error("region file '%s' does not exist." % conf.region_fn)
        return -1
    conf.reg_list = fcc.load_region_from_txt(conf.region_fn, verbose=True)
    if not conf.reg_list:
        error("failed to load region file.")
        return -1
    info("count %d regions in %d single cells." % (len(conf.reg_list), len(conf.samples)))
    if not conf.snp_fn:
        error("SNP file needed!")
        return -1
    if not os.path.isfile(conf.snp_fn):
        error("snp file '%s' does not exist." % conf.snp_fn)
        return -1
    loader = fcc.load_snp_from_vcf if fcc.is_vcf_name(conf.snp_fn) else fcc.load_snp_from_tsv
    conf.snp_list = loader(conf.snp_fn, verbose=True)
    if not conf.snp_list:
        error("failed to load snp file.")
        return -1
    info("%d SNPs loaded." % len(conf.snp_list))
    conf.snp_csp, conf.ref_cells = None, None
    if conf.cellsnp_dir is not None:
        # the per-SNP x cell pileup that local phasing works on (baf/fc/main.py:419-454)
        from ...utils.csp_io import load_data as csp_load_data
        from ...utils.grange import format_chrom
        if not os.path.isdir(conf.cellsnp_dir):
            error("cellsnp dir '%s' does not exist." % conf.cellsnp_dir)
            return -1
        try:
            csp = csp_load_data(conf.cellsnp_dir)
        except (IOError, OSError, ValueError) as e:
            error("failed to load cellsnp dir '%s': %s" % (conf.cellsnp_dir, e))
            return -1
        info("cellsnp SNP adata shape = %s." % str(csp.shape))
        if len(conf.samples) != csp.shape[0] or not set(conf.samples) <= set(csp.cells):
            error("cells of the cellsnp pileup do not match the barcodes / sample IDs.")
            return -1
        if csp.shape[1] != len(conf.snp_list):
            warn("n_snp: snp_adata=%d; snp_set=%d!" % (csp.shape[1], len(conf.snp_list)))
            if csp.shape[1] < len(conf.snp_list):
                error("the cellsnp pileup holds fewer SNPs than the phased SNP list.")
                return -1
        known = set((s[0], s[1]) for s in conf.snp_list)
        keep = [i for i in range(csp.shape[1]) if (format_chrom(str(csp.chrom[i])), int(csp.pos[i])) in known]
        if len(keep) < csp.shape[1]:                          # SNPs that were filtered in phasing
            csp = csp.subset_snps(keep)
            info("SNP adata shape after subset: %s." % str(csp.shape))
        conf.snp_csp = csp
    if conf.ref_cell_fn is not None:
        if not os.path.isfile(conf.ref_cell_fn):
            error("ref cell file '%s' does not exist." % conf.ref_cell_fn)
            return -1
        with open(conf.ref_cell_fn) as fp:
            conf.ref_cells = [x.rstrip("\n").split("\t")[0] for x in fp if x.strip()]
        if len(conf.ref_cells) > len(conf.samples) or not set(conf.ref_cells) <= set(conf.samples):
            error("reference cells are not a subset of the barcodes / sample IDs.")
            return -1
    if fcc.resolve_tags(conf) < 0:
        return -1
    conf.cell_groups = fcc.load_cell_groups(conf.samples)     # (XCK_CELL_GROUPS only; ValueError for a bad file, before any BAM is opened)
    if fcc.is_writer_rank():
        fcc.write_samples(conf.out_sample_fn, conf.samples)
    return 0


def regions_with_snps(regions, snps):
    """Boolean per region: at least one SNP with start <= pos <= end on the same (stripped)
    chromosome - the IntervalTree fetch of baf/fc/main.py:92-101."""
    import bisect
    from ...snptable import SnpTable
    if isinstance(snps, SnpTable):
        by_chrom = snps.positions_by_chrom()
    else:
        by_chrom = {}
        for s in snps:
            by_chrom.setdefault(s[0], []).append(s[1])
        for v in by_chrom.values():
            v.sort()
    out = []
    for ch, s, e, _ in regions:
        pos = by_chrom.get(ch)
        if pos is None or len(pos) == 0 or e < s:
            out.append(False)
            continue
        k = bisect.bisect_left(pos, s)
        out.append(bool(k < len(pos) and pos[k] <= e))
    return out


def _device_phasing_or_host(host_fn):
    """local_phasing() as XCK_DEVICE_PHASING says: unset / 0 -> the host loop (the default and the specification); 1 -> the regions are
    phased on the GPU (phasing_dev.py, csrc/local_phase.hip).  Without a usable device the host loop runs and the log says why; any
    other failure of the device path raises."""
    if os.environ.get("XCK_DEVICE_PHASING", "0") != "1":
        return host_fn
    from ... import capi
    n_dev = capi.load().xck_device_count()
    device = int(os.environ.get("XCK_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if n_dev <= 0:
        warn("XCK_DEVICE_PHASING=1 but no usable HIP device: local phasing runs on the host.")
        return host_fn
    if device >= n_dev:
        device = 0
    from .phasing_dev import local_phasing_dev
    return lambda *a: local_phasing_dev(*a, device=device)


def phased_tables(conf, regions, snps, has_snp):
    """-> (the SNP list the engine counts with, (region indices, SNP indices) left out of the SNP -> region join or None): the
    input as it is without local phasing; otherwise region-wise local phasing (baf/fc/main.py:107-153) gives new haplotype indices
    for flipped SNPs, and the SNPs without coverage in the pileup leave the SNP list of the region that was phased."""
    if not conf.use_local_phasing():
        return snps, None
    from .phasing import local_phasing
    from ...snptable import SnpTable
    phase_regions = regions if conf.output_all_reg else [r for r, h in zip(regions, has_snp) if h]
    phase_index = list(range(len(regions))) if conf.output_all_reg else [i for i, h in enumerate(has_snp) if h]
    rh, ah, ex_r, ex_s, _ = _device_phasing_or_host(local_phasing)(phase_regions, snps, conf.snp_csp, conf.ref_cells, conf.debug)
    ex_r = np.array([phase_index[i] for i in ex_r.tolist()], dtype=np.int32)
    if isinstance(snps, SnpTable):
        snps = SnpTable(snps.names, snps.chrom_id, snps.pos, snps.ref, snps.alt, rh, ah)
    else:
        snps = [(s[0], s[1], s[2], s[3], int(r), int(a)) for s, r, a in zip(snps, rh.tolist(), ah.tolist())]
    conf.snp_csp = conf.ref_cells = None
    return snps, (ex_r, ex_s)


def write_matrices(conf, eng, dist, regions, coo, n_cols=None):
    """xcltk.region.tsv and the three .mtx files of one counted table (afc_wrapper, afc_variants and the one-pass `xcltk baf` write
    through here), and with XCK_CELL_GROUPS their sums per cell group.  Only regions that wrote a DP or OTH line keep a row (baf/fc/core.py:101-113), unless output_all_reg.
    n_cols: the column count of the cell matrices' headers when `coo` is numbered by a subset of the engine's cells (afc_variants); None = the engine's cells."""
    pre = os.path.join(conf.out_dir, conf.out_prefix)
    fcc.write_matrix_set(eng, dist, regions, coo, conf.output_all_reg, conf.out_region_fn, {"ad": conf.out_ad_fn, "dp": conf.out_dp_fn, "oth": conf.out_oth_fn},
                         ("dp", "oth"), getattr(conf, "cell_groups", None), pre + "groups.tsv",
                         {"ad": pre + "AD.groups.mtx", "dp": pre + "DP.groups.mtx", "oth": pre + "OTH.groups.mtx"}, n_cols=n_cols)


def afc_core(conf):
    if prepare_config(conf) < 0:
        raise ValueError("errcode -2")
    info("program configuration:")
    conf.show(fp=sys.stderr, prefix="\t")
    regions, snps = conf.reg_list, conf.snp_list
    has_snp = regions_with_snps(regions, snps)
    info("#regions: total=%d; with_snps=%d." % (len(regions), sum(has_snp)))
    snps, excl = phased_tables(conf, regions, snps, has_snp)
    eng, coo, dist = fcc.make_and_count(conf, XCK_MODE_BAF, regions, snps, excl_pairs=excl)
    try:
        # (XCK_READ_FATE=1 / XCK_CELL_SUMMARY=1 / XCK_FEATURE_SUMMARY=1 only)
        fcc.write_summaries(eng, dist, os.path.join(conf.out_dir, conf.out_prefix), conf.samples, regions, snps)
        if coo is not None:                               # the only process / rank 0 after a gather / every rank (sharded output)
            write_matrices(conf, eng, dist, regions, coo)
        if conf.debug > 0:
            info("engine stats: %s" % eng.stats())
    finally:
        eng.close()
