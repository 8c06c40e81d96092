"""phasing_dev.py - region-wise local phasing on the device (XCK_DEVICE_PHASING=1).

The host path (phasing.py, ../localphase.py) stays the default and the specification.  This module chooses and pairs the SNPs
of every region exactly as local_phasing() does - the same eligibility tests, the position-sorted SNP list, zip()'s pairing
of the list with the pileup columns of the region - and writes the outcome down as SLOTS: (pileup column or -1, index of the
SNP in the phased list, position).  xck_local_phase (csrc/local_phase.hip) then runs reg_local_phasing / snp_local_phasing
for all regions on the GPU, and local_phasing_dev() turns its answer into the 5-tuple of local_phasing(), log lines included.
"""
from logging import debug, info
from logging import warning as warn

import numpy as np

from ...utils.grange import format_chrom
from .phasing import RLP_MIN_GAP, RLP_MIN_LEN, RLP_MIN_N_SNPS


def pileup_csc(csp, ref_cells=None):
    """The cell x SNP counts of a CellSnpData as the library takes them: (col_ptr, cell, ad, dp, cell_enabled or None).
    Entries are the non-zeros of DP; the reference cells stay in the table and are switched off by the mask."""
    DP = csp.DP.tocsc().astype(np.int64)
    DP.sum_duplicates()
    DP.eliminate_zeros()
    DP.sort_indices()
    AD = csp.AD.tocsc().astype(np.int64)
    ADm = AD.multiply(DP != 0).tocsc()                                   # AD where there is depth, on DP's pattern below
    if int(ADm.sum()) != int(AD.sum()) or int(abs(AD).sum()) != int(AD.sum()):
        raise ValueError("the cellsnp pileup has AD counts without depth, or negative ones")
    n_cells, n_cols = DP.shape
    key_dp = np.repeat(np.arange(n_cols, dtype=np.int64), np.diff(DP.indptr)) * n_cells + DP.indices
    ADm.sum_duplicates()
    ADm.eliminate_zeros()
    ADm.sort_indices()
    key_ad = np.repeat(np.arange(n_cols, dtype=np.int64), np.diff(ADm.indptr)) * n_cells + ADm.indices
    ad = np.zeros(len(key_dp), dtype=np.int64)
    ad[np.searchsorted(key_dp, key_ad)] = ADm.data
    enabled = None
    if ref_cells is not None:
        enabled = (~np.isin(np.array(csp.cells, dtype=object), np.array(list(ref_cells), dtype=object))).astype(np.uint8)
    return DP.indptr.astype(np.int64), DP.indices.astype(np.int32), ad, DP.data, enabled


def build_slots(regions, snps, csp, ref_cells=None):
    """-> dict: reg_ptr, slot_col, slot_snp, slot_pos (the CSR of slots); region (index into `regions` of every phased region);
    short (bool per slot: the list's tail beyond a pileup with fewer columns, which leaves the region first); csc (the pileup as
    pileup_csc() returns it).  Raises the ValueError of local_phasing() for a pileup with covered columns beyond the list's length."""
    s_chrom = [s[0] for s in snps]
    s_pos = np.array([s[1] for s in snps], dtype=np.int64)
    by_chrom = {}
    for j, ch in enumerate(s_chrom):
        by_chrom.setdefault(ch, []).append(j)
    for ch, idx in by_chrom.items():
        idx = np.array(idx, dtype=np.int64)
        by_chrom[ch] = idx[np.argsort(s_pos[idx], kind="stable")]       # the region's SNP list is sorted by position
    col_ptr, cell, ad, dp, enabled = pileup_csc(csp, ref_cells)
    # depth of every pileup column in the enabled cells (the covered test of the surplus case)
    on = np.ones(len(cell), dtype=bool) if enabled is None else enabled[cell].astype(bool)
    col_depth = np.add.reduceat(np.append(np.where(on, dp, 0), 0), col_ptr[:-1])[:len(col_ptr) - 1] if len(col_ptr) > 1 else np.zeros(0, dtype=np.int64)
    col_depth = np.where(np.diff(col_ptr) > 0, col_depth, 0)
    c_chrom = np.array([format_chrom(str(c)) for c in csp.chrom], dtype=object)
    c_pos = np.asarray(csp.pos, dtype=np.int64)
    cols_of = {}                                                         # chrom -> (column indices, their positions, sorted?)

    def region_cols(ch, start, end):
        if ch not in cols_of:
            idx = np.flatnonzero(c_chrom == ch)
            p = c_pos[idx]
            cols_of[ch] = (idx, p, bool(np.all(p[1:] >= p[:-1])))
        idx, p, is_sorted = cols_of[ch]
        if is_sorted:
            return idx[np.searchsorted(p, start, "left"):np.searchsorted(p, end + 1, "left")]
        return idx[(p >= start) & (p < end + 1)]                         # column order, whatever the positions do

    reg_ptr, slot_col, slot_snp, short, region = [0], [], [], [], []
    for g, (ch, start, end, name) in enumerate(regions):
        if end + 1 - start < RLP_MIN_LEN:
            continue
        cand = by_chrom.get(ch)
        if cand is None:
            continue
        lo, hi = np.searchsorted(s_pos[cand], start, "left"), np.searchsorted(s_pos[cand], end, "right")
        lst = cand[lo:hi]
        if len(lst) < max(1, RLP_MIN_N_SNPS):
            continue
        if s_pos[lst[-1]] - s_pos[lst[0]] + 1 < RLP_MIN_GAP:
            continue
        cols = region_cols(ch, start, end)
        if len(cols) > len(lst):
            covered = col_depth[cols] > 0
            if int(covered.sum()) != int(covered[:len(lst)].sum()):
                raise ValueError("region '%s': %d SNPs in the phased list but %d in the cellsnp pileup, %d of them covered beyond the list's length"
                                 % (name, len(lst), len(cols), int(covered[len(lst):].sum())))
            cols = cols[:len(lst)]                                       # (the columns beyond the list are empty: zip() never reaches them)
        sc = np.full(len(lst), -1, dtype=np.int64)
        sc[:len(cols)] = cols                                            # fewer columns: zip() pairs them with the FIRST SNPs of the list
        slot_col.append(sc); slot_snp.append(lst); short.append(np.arange(len(lst)) >= len(cols))
        reg_ptr.append(reg_ptr[-1] + len(lst))
        region.append(g)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)
    slot_snp = cat(slot_snp, np.int32)
    return dict(reg_ptr=np.array(reg_ptr, dtype=np.int64), slot_col=cat(slot_col, np.int32), slot_snp=slot_snp,
                slot_pos=s_pos[slot_snp].astype(np.int64), short=cat(short, bool), region=np.array(region, dtype=np.int64),
                csc=(col_ptr, cell, ad, dp, enabled))


def region_levels(reg_ptr, slot_snp):
    """Level of every region: 0 when it shares no SNP with an earlier region, otherwise 1 + the highest level among the earlier
    regions it shares a SNP with (the library makes the same levels and launches once per level)."""
    last = {}
    levels = np.zeros(len(reg_ptr) - 1, dtype=np.int64)
    for r in range(len(reg_ptr) - 1):
        sn = slot_snp[reg_ptr[r]:reg_ptr[r + 1]].tolist()
        lv = max([last.get(s, -1) for s in sn], default=-1) + 1
        for s in sn:
            last[s] = lv
        levels[r] = lv
    return levels


def tuple_from_result(regions, slots, kept, flip, status, ref_hap, alt_hap, debug_level=0):
    """The 5-tuple of local_phasing() and its log lines from per-slot kept / flip and per-region status (1 = phased)."""
    reg_ptr, slot_snp, short = slots["reg_ptr"], slots["slot_snp"], slots["short"]
    excl_region, excl_snp = [], []
    n_rlp = n_failed = n_slp = n_flipped = 0
    for r, g in enumerate(slots["region"].tolist()):
        a, b = int(reg_ptr[r]), int(reg_ptr[r + 1])
        sn, sh, kp = slot_snp[a:b], short[a:b], kept[a:b].astype(bool)
        for j in sn[sh].tolist():                                        # the tail of the list beyond a short pileup leaves first
            excl_region.append(g); excl_snp.append(j)
        for j in sn[~sh & ~kp].tolist():
            excl_region.append(g); excl_snp.append(j)
        name = regions[g][3]
        if not status[r]:
            warn("local phasing for region '%s' failed!" % name)
            n_failed += 1
        else:
            nf = int(flip[a:b][kp].sum())
            n_flipped += nf
            if debug_level > 1:
                debug("region '%s': #SNPs - total=%d; flipped=%d" % (name, int(kp.sum()), nf))
        n_slp += int(kp.sum())
        n_rlp += 1
    info("#regions: total=%d; local_phasing=%d; local_phasing_failed=%d." % (len(regions), n_rlp, n_failed))
    info("#SNPs: local_phasing=%d; local_phasing_flipped=%d." % (n_slp, n_flipped))
    return (np.asarray(ref_hap, dtype=np.int64), np.asarray(alt_hap, dtype=np.int64), np.array(excl_region, dtype=np.int32),
            np.array(excl_snp, dtype=np.int32), dict(n_rlp=n_rlp, n_failed=n_failed, n_slp=n_slp, n_flipped=n_flipped))


def local_phasing_dev(regions, snps, csp, ref_cells=None, debug_level=0, device=0):
    """local_phasing() of phasing.py with the regions phased on the GPU: same arguments, same 5-tuple."""
    from ...capi import local_phase
    slots = build_slots(regions, snps, csp, ref_cells)
    col_ptr, cell, ad, dp, enabled = slots["csc"]
    ref_hap = np.array([s[4] for s in snps], dtype=np.int64)
    alt_hap = np.array([s[5] for s in snps], dtype=np.int64)
    res = local_phase(csp.DP.shape[0], col_ptr, cell, ad, dp, ref_hap, alt_hap, slots["reg_ptr"], slots["slot_col"], slots["slot_snp"],
                      slots["slot_pos"], cell_enabled=enabled, device=device)
    ms = res["ms"]
    info("device local phasing: %d regions in %d levels; ms prepare=%.2f h2d=%.2f kernel=%.2f d2h=%.2f"
         % (len(slots["region"]), res["n_levels"], ms["prepare"], ms["h2d"], ms["kernel"], ms["d2h"]))
    return tuple_from_result(regions, slots, res["kept"], res["flip"], res["status"], res["ref_hap"], res["alt_hap"], debug_level)


def host_phase_slots(n_cells, col_ptr, cell, ad, dp, ref_hap, alt_hap, reg_ptr, slot_col, slot_snp, slot_pos, cell_enabled=None, cell_perm=None):
    """The problem of xck_local_phase answered by the host path, region after region (reg_local_phasing of phasing.py): the
    reference the device is compared with.  Slots without a column must be the tail of their region.  cell_perm: the rows of the
    dense matrices in another order, which changes nothing but the order of the float sums.  -> dict as capi.local_phase()."""
    from scipy import sparse
    from .phasing import reg_local_phasing
    n_cols = len(col_ptr) - 1
    AD = sparse.csc_matrix((np.asarray(ad, dtype=np.int64), np.asarray(cell), np.asarray(col_ptr)), shape=(n_cells, n_cols))
    DP = sparse.csc_matrix((np.asarray(dp, dtype=np.int64), np.asarray(cell), np.asarray(col_ptr)), shape=(n_cells, n_cols))
    rows = np.arange(n_cells) if cell_enabled is None else np.flatnonzero(np.asarray(cell_enabled))
    if cell_perm is not None:
        rows = rows[np.asarray(cell_perm)]
    ref_hap, alt_hap = np.array(ref_hap, dtype=np.int64), np.array(alt_hap, dtype=np.int64)
    n_slots = int(reg_ptr[-1])
    kept_all, flip_all = np.zeros(n_slots, dtype=np.uint8), np.zeros(n_slots, dtype=np.uint8)
    status = np.zeros(len(reg_ptr) - 1, dtype=np.uint8)
    for r in range(len(reg_ptr) - 1):
        a, b = int(reg_ptr[r]), int(reg_ptr[r + 1])
        n_with = int(np.sum(np.asarray(slot_col[a:b]) >= 0))
        assert np.all(np.asarray(slot_col[a:a + n_with]) >= 0)
        cols, lst = np.asarray(slot_col[a:a + n_with]), np.asarray(slot_snp[a:a + n_with])
        A, D = AD[:, cols].toarray()[rows], DP[:, cols].toarray()[rows]
        kept, flip = reg_local_phasing(ref_hap[lst], A, D, np.asarray(slot_pos[a:a + n_with]))
        kept_all[a:a + n_with] = kept
        if flip is not None:
            status[r] = 1
            flip_all[a:a + n_with][kept] = flip
            sel = lst[kept][flip == 1]
            ref_hap[sel], alt_hap[sel] = 1 - ref_hap[sel], 1 - alt_hap[sel]
    return dict(kept=kept_all, flip=flip_all, status=status, ref_hap=ref_hap.astype(np.int8), alt_hap=alt_hap.astype(np.int8),
                n_levels=int(region_levels(reg_ptr, np.asarray(slot_snp)).max()) + 1 if len(reg_ptr) > 1 else 0)
