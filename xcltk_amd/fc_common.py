"""fc_common.py - host logic shared by `basefc` and the BAF feature counting front-ends.

The reference duplicates this logic in xcltk/rdr/fc/main.py:305-431 and
xcltk/baf/fc/main.py:298-499 (prepare_config) and in the two utils.py (loaders, merge_mtx).
Here it lives once; behaviour (defaults, error messages, file formats, return codes) follows
those lines.  The compute itself is delegated to the HIP engine (engine.Engine).
"""

import ctypes as C
import os
import sys
import time
from logging import error, info
from logging import warning as warn

import numpy as np

from .capi import XCK_MODE_BASEFC
from .engine import Engine, XckError
from .snptable import SnpTable
from .utils.grange import format_chrom
from .utils.zfile import zopen

EXCL_FLAG_UMI = 772       # reference DefaultConfig, rdr/fc/config.py:108-109
EXCL_FLAG_XUMI = 1796


# ----------------------------------------------------------------------------- input resolution
def resolve_inputs(conf):
    """BAM list, barcodes / sample ids, tags, default exclude flag.  Returns 0 or -1 and
    logs the reference's messages (rdr/fc/main.py:323-373,401-429)."""
    if conf.sam_fn:
        if conf.sam_list_fn:
            error("should not specify 'sam_fn' and 'sam_list_fn' together.")
            return -1
        conf.sam_fn_list = conf.sam_fn.split(",")
    else:
        if not conf.sam_list_fn:
            error("one of 'sam_fn' and 'sam_list_fn' should be specified.")
            return -1
        with open(conf.sam_list_fn, "r") as fp:
            conf.sam_fn_list = [x.rstrip() for x in fp.readlines()]
    for fn in conf.sam_fn_list:
        if not os.path.isfile(fn):
            error("sam file '%s' does not exist." % fn)
            return -1

    if conf.barcode_fn:
        conf.sample_ids = None
        if conf.sample_id_str or conf.sample_id_fn:
            error("should not specify barcodes and sample IDs together.")
            return -1
        if not os.path.isfile(conf.barcode_fn):
            error("barcode file '%s' does not exist." % conf.barcode_fn)
            return -1
        with zopen(conf.barcode_fn, "rt") as fp:
            conf.barcodes = sorted(x.strip() for x in fp)       # column j = j-th SORTED barcode
        if len(set(conf.barcodes)) != len(conf.barcodes):
            error("duplicate barcodes!")
            return -1
    else:
        conf.barcodes = None
        if conf.sample_id_str and conf.sample_id_fn:
            error("should not specify 'sample_id_str' and 'sample_fn' together.")
            return -1
        if conf.sample_id_str:
            conf.sample_ids = conf.sample_id_str.split(",")
        elif conf.sample_id_fn:
            with zopen(conf.sample_id_fn, "rt") as fp:
                conf.sample_ids = [x.strip() for x in fp]
        else:
            warn("use default sample IDs ...")
            conf.sample_ids = ["Sample%d" % i for i in range(len(conf.sam_fn_list))]
        if len(conf.sample_ids) != len(conf.sam_fn_list):
            error("numbers of sam files and sample IDs are different.")
            return -1
    conf.samples = conf.barcodes if conf.barcodes else conf.sample_ids
    return 0


def resolve_tags(conf):
    """'None' strings, barcode/tag consistency, UMI 'Auto', default exclude flag."""
    if conf.cell_tag and conf.cell_tag.upper() == "NONE":
        conf.cell_tag = None
    if (not conf.cell_tag) ^ (not conf.barcodes):
        error("should not specify cell_tag or barcodes alone.")
        return -1
    if conf.umi_tag:
        up = conf.umi_tag.upper()
        if up == "AUTO":
            conf.umi_tag = None if conf.barcodes is None else conf.defaults.UMI_TAG_BC
        elif up == "NONE":
            conf.umi_tag = None
    if conf.excl_flag < 0:
        conf.excl_flag = EXCL_FLAG_UMI if conf.use_umi() else EXCL_FLAG_XUMI
    for tag, what in ((conf.cell_tag, "cell"), (conf.umi_tag, "UMI")):
        if tag and len(tag) != 2:
            error("%s tag '%s' is not a 2-character BAM tag." % (what, tag))
            return -1
    return 0


def load_region_from_txt(fn, sep="\t", verbose=False):
    """Header-free TSV: chrom, start, end (1-based inclusive), name -> list of
    (chrom_stripped, start, end_incl, name) in file order, or None (rdr/fc/utils.py:10-45)."""
    func = "load_region_from_txt"
    out = []
    if verbose:
        sys.stderr.write("[I::%s] start to load regions from file '%s' ...\n" % (func, fn))
    with zopen(fn, "rt") as fp:
        for nl, line in enumerate(fp, 1):
            parts = line.rstrip().split(sep)
            if len(parts) < 4:
                if verbose:
                    sys.stderr.write("[E::%s] too few columns of line %d.\n" % (func, nl))
                return None
            out.append((format_chrom(parts[0]), int(parts[1]), int(parts[2]), parts[3]))
    return out


_BASES = frozenset("ACGTN")


def _snp_from_fields(chrom, pos, ref, alt, a1, a2):
    ref, alt = ref.upper(), alt.upper()
    if len(ref) != 1 or ref not in "ACGTN":
        return "invalid REF base"
    if len(alt) != 1 or alt not in "ACGTN":
        return "invalid ALT base"
    if not ((a1 == "0" and a2 == "1") or (a1 == "1" and a2 == "0")):
        return "invalid GT"
    return (format_chrom(chrom), int(pos), ref, alt, int(a1), int(a2))


_REJ_TSV = {1: "too few columns of", 2: "invalid REF base of", 3: "invalid ALT base of", 7: "invalid GT of"}
_REJ_VCF = {1: "too few columns of", 2: "invalid REF base", 3: "invalid ALT base", 4: "GT not in", 5: "len(fields) != len(values) in",
            6: "invalid delimiter of", 7: "invalid GT of"}


def _load_snps_native(fn, is_vcf, verbose=False, func=""):
    """The library's parser (csrc/snptext.cpp): same list as the loops below for plain-ASCII files, about 4x sooner for a
    million SNPs; None when the file is outside what it reproduces exactly (or XCK_PY_LOADERS=1): the caller then loops.
    verbose: the per-line warnings of the loops, printed from the parser's list of rejected lines."""
    if os.environ.get("XCK_PY_LOADERS") == "1":
        return None
    from . import capi
    lib = capi.load()
    t = C.POINTER(capi.SnpText)()
    rc = lib.xck_parse_snp_text(fn.encode(), 1 if is_vcf else 0, C.byref(t))
    if rc != 0:
        return None                              # 1 = not eligible; I/O errors surface from the generic loader with Python's own message
    try:
        v = t.contents
        n, nr = int(v.n), int(v.n_rejected)
        if verbose and nr:
            text = _REJ_VCF if is_vcf else _REJ_TSV
            lines = np.ctypeslib.as_array(v.rej_line, shape=(nr,)).tolist()
            codes = np.ctypeslib.as_array(v.rej_code, shape=(nr,)).tolist()
            sys.stderr.write("".join("[W::%s] %s line %d.\n" % (func, text[c], l) for l, c in zip(lines, codes)))
        if n == 0:
            return []
        names = [v.chroms[i].decode("ascii") for i in range(v.n_chroms)]
        col = lambda p, dt: np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True)     # the library frees its own arrays
        return SnpTable(names, col(v.chrom_id, np.int32), col(v.pos, np.int64),
                        np.frombuffer(C.string_at(v.ref, n), dtype=np.uint8), np.frombuffer(C.string_at(v.alt, n), dtype=np.uint8),
                        col(v.ref_hap, np.int8), col(v.alt_hap, np.int8))
    finally:
        lib.xck_free_snp_text(t)


def load_snp_from_tsv(fn, verbose=False):
    """TSV with header: chrom pos ref alt ref_hap alt_hap (baf/fc/utils.py:51-110)."""
    func = "load_snp_from_tsv"
    snps = []
    if verbose:
        sys.stderr.write("[I::%s] start to load SNPs from tsv '%s' ...\n" % (func, fn))
    native = _load_snps_native(fn, False, verbose, func)
    if native is not None:
        return native
    with zopen(fn, "rt") as fp:
        for nl, line in enumerate(fp, 1):
            if nl == 1:
                continue
            parts = line.rstrip().split("\t")
            if len(parts) < 6:
                if verbose:
                    sys.stderr.write("[W::%s] too few columns of line %d.\n" % (func, nl))
                continue
            # inlined common case of _snp_from_fields (a million-SNP panel is a million calls)
            ref, alt, a1, a2 = parts[2], parts[3], parts[4], parts[5]
            if ref in _BASES and alt in _BASES and ((a1 == "0" and a2 == "1") or (a1 == "1" and a2 == "0")):
                snps.append((format_chrom(parts[0]), int(parts[1]), ref, alt, int(a1), int(a2)))
                continue
            s = _snp_from_fields(parts[0], parts[1], parts[2], parts[3], parts[4], parts[5])
            if isinstance(s, str):
                if verbose:
                    sys.stderr.write("[W::%s] %s of line %d.\n" % (func, s, nl))
                continue
            snps.append(s)
    return snps


def load_snp_from_vcf(fn, verbose=False):
    """Phased VCF, first sample column; GT must be 0|1, 1|0, 0/1 or 1/0 (baf/fc/utils.py:114-193)."""
    func = "load_snp_from_vcf"
    snps = []
    if verbose:
        sys.stderr.write("[I::%s] start to load SNPs from vcf '%s' ...\n" % (func, fn))
    native = _load_snps_native(fn, True, verbose, func)
    if native is not None:
        return native
    with zopen(fn, "rt") as fp:
        for nl, line in enumerate(fp, 1):
            if line[0] in ("#", "\n"):
                continue
            parts = line.rstrip().split("\t")
            if len(parts) < 10:
                if verbose:
                    sys.stderr.write("[W::%s] too few columns of line %d.\n" % (func, nl))
                continue
            msg = None
            fields = parts[8].split(":")
            values = parts[9].split(":")
            ref, alt = parts[3].upper(), parts[4].upper()
            if len(ref) != 1 or ref not in "ACGTN":
                msg = "invalid REF base"
            elif len(alt) != 1 or alt not in "ACGTN":
                msg = "invalid ALT base"
            elif "GT" not in fields:
                msg = "GT not in"
            elif len(values) != len(fields):
                msg = "len(fields) != len(values) in"
            else:
                gt = values[fields.index("GT")]
                sepc = "|" if "|" in gt else ("/" if "/" in gt else None)
                if sepc is None:
                    msg = "invalid delimiter of"
                else:
                    a1, a2 = gt.split(sepc)[:2]
                    s = _snp_from_fields(parts[0], parts[1], ref, alt, a1, a2)
                    if isinstance(s, str):
                        msg = s + " of"
                    else:
                        snps.append(s)
            if msg and verbose:
                sys.stderr.write("[W::%s] %s line %d.\n" % (func, msg, nl))
    return snps


def is_vcf_name(fn):
    return fn.endswith(".vcf") or fn.endswith(".vcf.gz") or fn.endswith(".vcf.bgz")


# ----------------------------------------------------------------------------- outputs
def contig_table(regions, snps=()):
    names, seen = [], set()
    for ch in [r[0] for r in regions] + (snps.chroms() if isinstance(snps, SnpTable) else [s[0] for s in snps]):
        if ch not in seen:
            seen.add(ch)
            names.append(ch)
    return names


def row_map_all(n):
    return np.arange(1, n + 1, dtype=np.int32)


def row_map_from_rows(n, *row_arrays):
    """Rows are numbered over the regions that produced at least one output line
    (k_reg bookkeeping, rdr/fc/core.py:118-124 and baf/fc/core.py:101-113)."""
    keep = np.zeros(n, dtype=bool)
    for r in row_arrays:
        keep[r] = True
    rm = np.zeros(n, dtype=np.int32)
    rm[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    return rm


def write_region_tsv(path, regions, rm):
    with open(path, "w") as fp:
        fp.write("".join("%s\t%d\t%d\t%s\n" % (ch, s, e, name)
                         for (ch, s, e, name), r in zip(regions, rm) if r > 0))


def is_writer_rank():
    """True in a single-process run and on rank 0 of a multi-GPU run (the only rank that writes files)."""
    return int(os.environ.get("RANK", "0")) == 0


def write_samples(path, samples):
    with open(path, "w") as fp:
        fp.write("".join(smp + "\n" for smp in samples))


def output_row_map(dist, n, all_reg, *row_arrays):
    """Output row of every region (0 = no row).  With sharded output the regions that wrote a line are known only jointly:
    one all-reduce of a presence vector (collective call)."""
    if all_reg:
        return row_map_all(n)
    if dist is not None and dist.active and dist.sharded_output:
        keep = np.zeros(n, dtype=np.int32)
        for r in row_arrays:
            keep[r] = 1
        keep = dist.all_reduce_np(keep, "max") > 0
        rm = np.zeros(n, dtype=np.int32)
        rm[keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
        return rm
    return row_map_from_rows(n, *row_arrays)


def write_mtx(eng, dist, path, coo_k, rm, n_rows_out, n_cols=None):
    """One matrix file: written by this process, or - sharded output - by all ranks together, each the lines of its own rows
    (shard.write_mtx_sharded; collective call).  n_cols: the column count of the header; None = the engine's cells."""
    if dist is not None and dist.active and dist.sharded_output:
        from .shard import write_mtx_sharded
        write_mtx_sharded(path, coo_k, rm, dist.row_owner, n_rows_out, eng.n_cells if n_cols is None else int(n_cols), dist.rank, dist.all_reduce_np,
                          dist.barrier, eng.lib)
    else:
        eng.write_mtx_arrays(path, coo_k, rm, n_rows_out, n_cols=n_cols)


# ----------------------------------------------------------------------------- cell groups (XCK_CELL_GROUPS)
def parse_cell_groups(lines, cells):
    """The group file of XCK_CELL_GROUPS as a pure function.  lines: an iterable of `name<TAB>group` lines without a header (blank
    lines are skipped); cells: the run's barcodes or sample ids in column order.  Groups are numbered by first appearance in the
    file, whether or not the line names a cell of the run, so a file numbers its groups the same way for every run; names that
    are not among `cells` are ignored and counted; cells the file does not name get -1.  -> (group names in column order, int32
    array [len(cells)] of group indices, number of ignored names).  ValueError for a line without two fields, a name with two
    different groups, or more than XCK_GROUP_MAX groups."""
    from .capi import XCK_GROUP_MAX
    col = {c: i for i, c in enumerate(cells)}
    names, gidx, seen = [], {}, {}
    cell_group = np.full(len(cells), -1, dtype=np.int32)
    n_ignored = 0
    for nl, line in enumerate(lines, 1):
        line = line.rstrip("\r\n")
        if not line.strip():
            continue
        parts = line.split("\t")
        if len(parts) < 2 or not parts[0] or not parts[1]:
            raise ValueError("cell group file: line %d is not name<TAB>group" % nl)
        name, grp = parts[0], parts[1]
        if name in seen:
            if seen[name] != grp:
                raise ValueError("cell group file: '%s' is in two groups ('%s' and '%s')" % (name, seen[name], grp))
            continue
        seen[name] = grp
        if grp not in gidx:
            gidx[grp] = len(names)
            names.append(grp)
            if len(names) > XCK_GROUP_MAX:
                raise ValueError("cell group file: more than %d groups" % XCK_GROUP_MAX)
        if name in col:
            cell_group[col[name]] = gidx[grp]
        else:
            n_ignored += 1
    return names, cell_group, n_ignored


def load_cell_groups(cells, log_prefix="[engine]"):
    """(group names, cell -> group array) of the file XCK_CELL_GROUPS names, or None when the knob is unset.  ValueError as
    parse_cell_groups, or when the file does not exist - raised where the front-ends resolve their inputs, before a BAM is opened."""
    fn = os.environ.get("XCK_CELL_GROUPS", "")
    if not fn:
        return None
    if not os.path.isfile(fn):
        raise ValueError("cell group file '%s' does not exist." % fn)
    with zopen(fn, "rt") as fp:
        names, cell_group, n_ignored = parse_cell_groups(fp, list(cells))
    info("%s cell groups: %d groups, %d of %d cells grouped, %d names ignored (not cells of this run)" %
         (log_prefix, len(names), int((cell_group >= 0).sum()), len(cell_group), n_ignored))
    return names, cell_group


def group_output_off(dist, log_prefix="[engine]"):
    """True (and one log line) where a multi-GPU run gathers its result on one rank: that form writes no group files."""
    if dist is not None and dist.active and not dist.sharded_output:
        info("%s XCK_CELL_GROUPS: the gathered output form (XCK_DIST_GATHER=1 / gather=True) writes no group files." % log_prefix)
        return True
    return False


def write_group_matrices(eng, dist, groups, names_fn, mtx_fns, rm, n_rows_out, source="result", log_prefix="[engine]"):
    """The engine's matrices summed per cell group (Engine.group_counts) -> names_fn (group names, one per line) and mtx_fns
    ({"count": path} or {"ad": .., "dp": .., "oth": ..}), in the rows `rm` gives the cell files.  groups: load_cell_groups() - None
    (XCK_CELL_GROUPS unset): nothing is launched or written.  Sharded output: a collective call, every rank sums its own rows."""
    if groups is None or group_output_off(dist, log_prefix):
        return
    names, cell_group = groups
    got = eng.group_counts(cell_group, n_groups=max(len(names), 1), source=source, copy=False)
    if is_writer_rank():
        write_samples(names_fn, names)
    for k, fn in mtx_fns.items():
        write_mtx(eng, dist, fn, got[k], rm, n_rows_out, n_cols=len(names))


def write_matrix_set(eng, dist, regions, coo, all_reg, region_fn, mtx_fns, presence, groups, group_names_fn, group_mtx_fns, log_prefix="[engine]", n_cols=None):
    """One matrix set: the region file (writer rank), the .mtx files of mtx_fns (an ordered {key of coo: path}), and with XCK_CELL_GROUPS
    the same rows summed per cell group (write_group_matrices).  A region keeps a row when a matrix named in `presence` wrote a line
    for it - ("count",) for basefc (rdr/fc/core.py:118-124), ("dp", "oth") for BAF (baf/fc/core.py:101-113) - or, all_reg, always:
    its row is then its input line number.  n_cols: the column count of the cell matrices' headers (None = the engine's cells).
    Sharded output: collective calls, on every rank."""
    rm = output_row_map(dist, len(regions), all_reg, *[coo[k][0] for k in presence])
    n_rows_out = int(rm.max()) if len(rm) else 0
    if is_writer_rank():
        write_region_tsv(region_fn, regions, rm)
    for k, fn in mtx_fns.items():
        write_mtx(eng, dist, fn, coo[k], rm, n_rows_out, n_cols=n_cols)
    write_group_matrices(eng, dist, groups, group_names_fn, group_mtx_fns, rm, n_rows_out, log_prefix=log_prefix)


def read_summary_text(fate, n_ranks=1, cut_contigs=0):
    """Text of read_summary.tsv: one `name\\tcount` line per counter of xck_read_fate, in the struct's order; runs of several
    ranks start with `#ranks=N cut_contigs=K`."""
    from .capi import READ_FATE_FIELDS
    head = "#ranks=%d cut_contigs=%d\n" % (n_ranks, cut_contigs) if n_ranks > 1 else ""
    return head + "".join("%s\t%d\n" % (k, int(fate[k])) for k in READ_FATE_FIELDS)


def _summary_ranks(dist):
    """(ranks, contigs cut over ranks) for the `#ranks` line of a summary file"""
    if dist is None or not dist.active:
        return 1, 0
    return dist.world, len(set(u["contig"] for u in getattr(dist, "units", ()) if u["window"] is not None))


def _write_summary(dist, path, arrays, text, log):
    """What every summary writer does with its table: the int64 `arrays` are summed over the ranks in ONE all-reduce (concatenated,
    reduced, split, reshaped; a collective call), log(summed arrays) is logged, and the writer rank creates the directory and writes
    text(summed arrays, n_ranks, cut_contigs) to `path`.  Returns the summed arrays."""
    arrays = [np.asarray(a, dtype=np.int64) for a in arrays]
    n_ranks, cut = _summary_ranks(dist)
    if dist is not None and dist.active:
        v = dist.all_reduce_np(np.concatenate([a.ravel() for a in arrays]))
        ends = np.cumsum([a.size for a in arrays]).tolist()
        arrays = [v[e - a.size:e].reshape(a.shape) for a, e in zip(arrays, ends)]
    info(log(arrays))
    if is_writer_rank():
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fp:
            fp.write(text(arrays, n_ranks, cut))
    return arrays


def write_read_summary(eng, dist, path, mode=None, log_prefix="[engine]"):
    """Read assignment summary of one pipeline (Engine.read_fate) -> `path`, when the handle counts it (XCK_READ_FATE=1 in the
    environment, or XCK_F_READ_FATE): nothing happens otherwise.  Multi-GPU: a collective call - the counters are summed over the
    ranks and the writer rank writes the file.  Where a contig is cut over ranks (cut_contigs > 0) the reads that straddle a cut
    are decoded by both neighbours and so counted twice, and each rank judges `no_target` against the regions it owns: the sums
    then describe the ranks' work, not the file.  Returns the (summed) dict or None."""
    from .capi import READ_FATE_FIELDS
    read_fate = getattr(eng, "read_fate", None)                # (an engine-like object without the method counts nothing)
    fate = read_fate(mode) if read_fate else None
    if fate is None:
        return None
    as_dict = lambda a: dict(zip(READ_FATE_FIELDS, a[0].tolist()))
    return as_dict(_write_summary(dist, path, [[fate[k] for k in READ_FATE_FIELDS]], lambda a, n_ranks, cut: read_summary_text(as_dict(a), n_ranks, cut),
                                  lambda a: "%s read summary: %s" % (log_prefix, " ".join("%s=%d" % kv for kv in as_dict(a).items()))))


def cell_summary_text(names, fate, matrix, fate_cols, matrix_cols, n_ranks=1, cut_contigs=0):
    """Text of cell_summary.tsv: header `cell reads <fate columns> <matrix columns>`, one line per matrix column in column order
    named by `names`, and a last line `*` for the reads without a listed cell (0 in the matrix columns).  `reads` is the sum of the
    class columns (everything but multi and pairs).  Runs of several ranks start with `#ranks=N cut_contigs=K`."""
    fate = np.asarray(fate, dtype=np.int64)
    n = len(names)
    assert fate.shape == (n + 1, len(fate_cols))
    matrix = np.zeros((n, len(matrix_cols)), dtype=np.int64) if matrix is None else np.asarray(matrix, dtype=np.int64)
    assert matrix.shape == (n, len(matrix_cols))
    n_cls = len(fate_cols) - 2
    head = "#ranks=%d cut_contigs=%d\n" % (n_ranks, cut_contigs) if n_ranks > 1 else ""
    lines = [head, "\t".join(("cell", "reads") + tuple(fate_cols) + tuple(matrix_cols)) + "\n"]
    for i in range(n + 1):
        m = matrix[i] if i < n else np.zeros(len(matrix_cols), dtype=np.int64)
        vals = [int(fate[i, :n_cls].sum())] + [int(x) for x in fate[i]] + [int(x) for x in m]
        lines.append((names[i] if i < n else "*") + "\t" + "\t".join("%d" % v for v in vals) + "\n")
    return "".join(lines)


def write_cell_summary(eng, dist, path, names, mode=None, log_prefix="[engine]"):
    """Per-cell table of one pipeline (Engine.cell_summary, after finish()) -> `path`, when the handle keeps it (XCK_CELL_SUMMARY=1 in
    the environment, or XCK_F_CELL_SUMMARY): nothing happens otherwise.  `names`: the matrix columns in order (barcodes or sample
    ids).  Multi-GPU: a collective call - the two arrays are summed over the ranks in one all-reduce and the writer rank writes
    the file; the caveat of write_read_summary about cut contigs holds per cell.  Returns the (summed) dict or None."""
    cell_summary = getattr(eng, "cell_summary", None)          # (an engine-like object without the method keeps nothing)
    cs = cell_summary(mode) if cell_summary else None
    if cs is None:
        return None
    fate, matrix = np.asarray(cs["fate"]), cs["matrix"]
    if matrix is None:
        matrix = np.zeros((fate.shape[0] - 1, len(cs["matrix_cols"])), dtype=np.int64)
    fate, matrix = _write_summary(
        dist, path, [fate, matrix], lambda a, n_ranks, cut: cell_summary_text(list(names), a[0], a[1], cs["fate_cols"], cs["matrix_cols"], n_ranks, cut),
        lambda a: "%s cell summary: %d cells with reads, %d reads without a listed cell" %
        (log_prefix, int((a[0][:-1].sum(axis=1) > 0).sum()), int(a[0][-1, :len(cs["fate_cols"]) - 2].sum())))
    return dict(cs, fate=fate, matrix=matrix)


def feature_summary_text(regions, reads, matrix, mode, n_ranks=1, cut_contigs=0):
    """Text of feature_summary.tsv: header, then one line per input region in input order (regions that got no output row too): the
    four fields of the features.tsv / region.tsv line, then the counters - basefc `fetched include_fail pairs shared umis cells`
    (fetched = pairs + include_fail), BAF `snps snps_kept ad dp oth cells`.  Runs of several ranks start with
    `#ranks=N cut_contigs=K`."""
    from .capi import FEATURE_READ_COLS, FEATURE_MATRIX_COLS, XCK_MODE_BASEFC
    n = len(regions)
    mcols = FEATURE_MATRIX_COLS[mode]
    matrix = np.zeros((n, len(mcols)), dtype=np.int64) if matrix is None else np.asarray(matrix, dtype=np.int64)
    assert matrix.shape == (n, len(mcols))
    if mode == XCK_MODE_BASEFC:
        reads = np.asarray(reads, dtype=np.int64)
        assert reads.shape == (n, len(FEATURE_READ_COLS))
        fail, pairs = FEATURE_READ_COLS.index("include_fail"), FEATURE_READ_COLS.index("pairs")
        table = np.concatenate([(reads[:, pairs] + reads[:, fail])[:, None], reads, matrix], axis=1)
        cols = ("fetched",) + tuple(FEATURE_READ_COLS) + tuple(mcols)
    else:
        table, cols = matrix, tuple(mcols)
    head = "#ranks=%d cut_contigs=%d\n" % (n_ranks, cut_contigs) if n_ranks > 1 else ""
    lines = [head, "\t".join(("chrom", "start", "end", "name") + cols) + "\n"]
    for (ch, s, e, name), row in zip(regions, table.tolist()):
        lines.append("%s\t%d\t%d\t%s\t%s\n" % (ch, s, e, name, "\t".join("%d" % v for v in row)))
    return "".join(lines)


def write_feature_summary(eng, dist, path, regions, mode=None, log_prefix="[engine]"):
    """Per-feature table of one pipeline (Engine.feature_summary, after finish()) -> `path`, when the handle keeps it
    (XCK_FEATURE_SUMMARY=1 in the environment, or XCK_F_FEATURE_SUMMARY): nothing happens otherwise.  `regions`: the input regions
    (chrom, start, end, name) in input order.  Multi-GPU: a collective call - one summing all-reduce, and the writer rank writes
    the file.  Every rank counts only the regions of its region_mask and a region belongs to exactly one rank, so the file is
    exact even where a contig is cut over ranks.  Returns the (summed) dict or None."""
    from .capi import FEATURE_READ_COLS
    feature_summary = getattr(eng, "feature_summary", None)    # (an engine-like object without the method keeps nothing)
    fs = feature_summary(mode) if feature_summary else None
    if fs is None:
        return None
    mode = eng.mode if mode is None else mode
    basefc = mode == XCK_MODE_BASEFC
    n = len(regions)                                           # (a handle without a region hands out no array: an empty table of the same columns)
    reads = np.zeros((n, len(FEATURE_READ_COLS) if basefc else 0), dtype=np.int64) if fs["reads"] is None or not basefc else fs["reads"]
    matrix = np.zeros((n, len(fs["matrix_cols"])), dtype=np.int64) if fs["matrix"] is None else fs["matrix"]
    reads, matrix = _write_summary(
        dist, path, [reads, matrix],
        lambda a, n_ranks, cut: feature_summary_text(list(regions), a[0] if basefc else None, a[1], mode, n_ranks, cut),
        lambda a: "%s feature summary: %d of %d regions with an entry" % (log_prefix, int((a[1][:, -1] > 0).sum()), n))
    return dict(fs, reads=reads if basefc else None, matrix=matrix)


def snp_summary_text(snps, table, n_ranks=1, cut_contigs=0):
    """Text of snp_summary.tsv: header `chrom pos ref alt ref_hap alt_hap reads A C G T N total ref_umis alt_umis kept regions`, then
    one line per SNP of the list in input order.  `snps`: (chrom, pos, ref, alt, ref_hap, alt_hap); `table`: the `snp` array of
    Engine.feature_summary (columns capi.SNP_COLS).  total = A + C + G + T + N; ref_umis / alt_umis = the tally of the SNP's REF /
    ALT base (N for a base outside ACGT).  Runs of several ranks start with `#ranks=N cut_contigs=K`."""
    table = np.asarray(table, dtype=np.int64)
    assert table.shape == (len(snps), 8)
    head = "#ranks=%d cut_contigs=%d\n" % (n_ranks, cut_contigs) if n_ranks > 1 else ""
    lines = [head, "chrom\tpos\tref\talt\tref_hap\talt_hap\treads\tA\tC\tG\tT\tN\ttotal\tref_umis\talt_umis\tkept\tregions\n"]
    idx = {"A": 0, "C": 1, "G": 2, "T": 3}
    for (ch, pos, ref, alt, rh, ah), row in zip(snps, table.tolist()):
        tally = row[1:6]
        lines.append("%s\t%d\t%s\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%d\n" % (
            ch, pos, ref, alt, rh, ah, row[0], "\t".join("%d" % v for v in tally), sum(tally),
            tally[idx.get(ref, 4)], tally[idx.get(alt, 4)], row[6], row[7]))
    return "".join(lines)


def write_snp_summary(eng, dist, path, snps, mode=None, log_prefix="[engine]", rows=None):
    """Per-SNP table of the pileup pipeline (Engine.feature_summary, after finish()) -> `path`, when the handle keeps it: nothing
    happens otherwise.  `snps`: the list to print, tuples (chrom, pos, ref, alt, ref_hap, alt_hap) or a SnpTable - the engine's own
    SNPs in input order, or with `rows` (an index array into the engine's SNP table, one per SNP of `snps`) a selection of them in
    any order.  Multi-GPU: a collective call - a rank zeroes the rows of the SNPs on contigs it does not stream, one summing
    all-reduce, and the writer rank writes the file.  Where a contig is cut over ranks (cut_contigs > 0 in the `#ranks` line) both neighbours see the reads
    and count the tallies of the SNPs near the cut, and `kept` is then the number of ranks that kept the SNP: those rows describe
    the ranks' work, not the file; nothing corrects for it.  `kept` (and `snps_kept` of feature_summary.tsv) is the verdict under
    the min_count / min_maf the ENGINE was made with: baf.genotype.pileup() makes its engine with 1 / 0 and applies the caller's
    thresholds to the summed matrices afterwards (filter_snps), so there `kept` says "some molecule showed a base", not "survived
    pileup's filter".  Returns the (summed) array or None."""
    from .capi import XCK_MODE_BAF
    feature_summary = getattr(eng, "feature_summary", None)
    fs = feature_summary(XCK_MODE_BAF) if feature_summary and eng.mode & XCK_MODE_BAF else None
    if fs is None or fs["snp"] is None:
        return None
    table = np.asarray(fs["snp"], dtype=np.int64)
    mask = getattr(dist, "contig_mask", None) if dist is not None and dist.active else None
    if mask is not None and len(table):
        table[~np.asarray(mask, dtype=bool)[eng._snp["contig"]]] = 0
    if rows is not None:
        table = table[np.asarray(rows, dtype=np.int64)]
    snps = list(snps)
    return _write_summary(dist, path, [table], lambda a, n_ranks, cut: snp_summary_text(snps, a[0], n_ranks, cut),
                          lambda a: "%s SNP summary: %d of %d SNPs kept" % (log_prefix, int((a[0][:, 6] > 0).sum()), len(a[0])))[0]


def molecule_summary_text(stats, n_ranks=1, cut_contigs=0):
    """Text of molecule_summary.tsv: one `name\\tcount` line per counter of xck_molecule_stats, in the struct's order; runs of several
    ranks start with `#ranks=N cut_contigs=K`."""
    from .capi import MOLECULE_FIELDS
    head = "#ranks=%d cut_contigs=%d\n" % (n_ranks, cut_contigs) if n_ranks > 1 else ""
    return head + "".join("%s\t%d\n" % (k, int(stats[k])) for k in MOLECULE_FIELDS)


def write_molecule_summary(eng, dist, path, log_prefix="[engine]"):
    """How the reads of the molecules of the pileup agree (Engine.molecule_stats, after finish()) -> `path`, when the handle decides a
    molecule's base by vote (XCK_UMI_CONSENSUS=1 in the environment, or XCK_F_UMI_CONSENSUS): nothing happens otherwise.  Multi-GPU:
    a collective call - the counters are summed over the ranks and the writer rank writes the file.  Where a contig is cut over
    ranks (cut_contigs > 0) a molecule with reads on both sides of a cut is counted by both neighbours: the sums then describe the
    ranks' work, not the file.  Returns the (summed) dict or None."""
    from .capi import MOLECULE_FIELDS
    molecule_stats = getattr(eng, "molecule_stats", None)      # (an engine-like object without the method votes nowhere)
    st = molecule_stats() if molecule_stats else None
    if st is None:
        return None
    as_dict = lambda a: dict(zip(MOLECULE_FIELDS, a[0].tolist()))
    return as_dict(_write_summary(dist, path, [[st[k] for k in MOLECULE_FIELDS]], lambda a, n_ranks, cut: molecule_summary_text(as_dict(a), n_ranks, cut),
                                  lambda a: "%s UMI consensus: %d of %d molecules changed" % (log_prefix, as_dict(a)["changed"], as_dict(a)["molecules"])))


def umi_feature_summary_text(stats, n_ranks=1, cut_contigs=0):
    """Text of umi_feature_summary.tsv: one `name\\tcount` line per counter of xck_umi_feature_stats, in the struct's order; runs of
    several ranks start with `#ranks=N cut_contigs=K`."""
    from .capi import UMI_FEATURE_FIELDS
    head = "#ranks=%d cut_contigs=%d\n" % (n_ranks, cut_contigs) if n_ranks > 1 else ""
    return head + "".join("%s\t%d\n" % (k, int(stats[k])) for k in UMI_FEATURE_FIELDS)


def write_umi_feature_summary(eng, dist, path, log_prefix="[engine]"):
    """What the unique-feature rule of the basefc fold dropped (Engine.umi_feature_stats, after finish()) -> `path`, when the handle
    counts unique-feature molecules only (XCK_UMI_FEATURE=unique in the environment, or XCK_F_UNIQUE_FEATURE): nothing happens
    otherwise.  Multi-GPU: a collective call - the counters are summed over the ranks and the writer rank writes the file; the ranks
    own whole contigs (make_engine refuses a plan that gives the pieces of one to several ranks) and a molecule lives on one contig, so the sums are
    the one-GPU run's.  Returns the (summed) dict or None."""
    from .capi import UMI_FEATURE_FIELDS
    umi_feature_stats = getattr(eng, "umi_feature_stats", None)   # (an engine-like object without the method drops nothing)
    st = umi_feature_stats() if umi_feature_stats else None
    if st is None:
        return None
    as_dict = lambda a: dict(zip(UMI_FEATURE_FIELDS, a[0].tolist()))
    return as_dict(_write_summary(dist, path, [[st[k] for k in UMI_FEATURE_FIELDS]], lambda a, n_ranks, cut: umi_feature_summary_text(as_dict(a), n_ranks, cut),
                                  lambda a: "%s unique-feature molecules: %d of %d molecules on two or more features dropped" %
                                  (log_prefix, as_dict(a)["multi_feature"], as_dict(a)["molecules"])))


def umi_dedup_summary_text(stats, n_ranks=1, cut_contigs=0):
    """Text of umi_dedup_summary.tsv: one `name\\tcount` line per counter of xck_umi_dedup_stats, in the struct's order; runs of
    several ranks start with `#ranks=N cut_contigs=K`."""
    from .capi import UMI_DEDUP_FIELDS
    head = "#ranks=%d cut_contigs=%d\n" % (n_ranks, cut_contigs) if n_ranks > 1 else ""
    return head + "".join("%s\t%d\n" % (k, int(stats[k])) for k in UMI_DEDUP_FIELDS)


def write_umi_dedup_summary(eng, dist, path, log_prefix="[engine]"):
    """What the 1-mismatch UMI collapsing of the basefc fold merged (Engine.umi_dedup_stats, after finish()) -> `path`, when the handle
    collapses (XCK_UMI_DEDUP=1mm_all in the environment, or XCK_F_UMI_COLLAPSE): nothing happens otherwise.  Multi-GPU: a collective
    call - the ranks own disjoint rows of the region table, a (row, cell) group never spans two of them, so the counters are summed
    over the ranks (max_group: the largest - every rank's value travels in a slot of its own through the same all-reduce) and the
    writer rank writes the file; the result is the one-GPU run's.  Returns the dict or None."""
    from .capi import UMI_DEDUP_FIELDS
    umi_dedup_stats = getattr(eng, "umi_dedup_stats", None)       # (an engine-like object without the method merges nothing)
    st = umi_dedup_stats() if umi_dedup_stats else None
    if st is None:
        return None
    n_ranks, rank = (dist.world, dist.rank) if dist is not None and dist.active else (1, 0)
    slots = [0] * n_ranks
    slots[rank] = st["max_group"]
    def as_dict(a):
        d = dict(zip(UMI_DEDUP_FIELDS, a[0].tolist()))
        d["max_group"] = int(max(a[1].tolist()))
        return d
    return as_dict(_write_summary(dist, path, [[st[k] for k in UMI_DEDUP_FIELDS], slots], lambda a, n_ranks, cut: umi_dedup_summary_text(as_dict(a), n_ranks, cut),
                                  lambda a: "%s UMI collapsing (1mm_all): %d of %d keys merged away, %d of %d groups changed" %
                                  (log_prefix, as_dict(a)["keys"] - as_dict(a)["molecules"], as_dict(a)["keys"], as_dict(a)["groups_changed"], as_dict(a)["groups"])))


def write_summaries(eng, dist, prefix, samples, regions, snps=None, mode=None, log_prefix="[engine]"):
    """The opt-in tables of one pipeline next to its matrices: `prefix` + read_summary.tsv (XCK_READ_FATE=1), cell_summary.tsv
    (XCK_CELL_SUMMARY=1), feature_summary.tsv (XCK_FEATURE_SUMMARY=1), - `snps` given, the pileup pipeline - snp_summary.tsv and - the
    pileup pipeline under XCK_UMI_CONSENSUS=1 - molecule_summary.tsv and - the basefc pipeline under XCK_UMI_FEATURE=unique -
    umi_feature_summary.tsv and - the basefc pipeline under XCK_UMI_DEDUP=1mm_all - umi_dedup_summary.tsv, each only when the handle keeps it.  `prefix` is a path
    prefix: a directory with its separator, or e.g. <dir>/xcltk. ; mode names the pipeline of a XCK_MODE_BOTH handle.  Multi-GPU: the
    writers' collective calls, in this order on every rank."""
    from .capi import XCK_MODE_BAF
    if getattr(eng, "mode", 0) & XCK_MODE_BASEFC and (mode is None or mode & XCK_MODE_BASEFC):
        write_umi_feature_summary(eng, dist, prefix + "umi_feature_summary.tsv", log_prefix)
        write_umi_dedup_summary(eng, dist, prefix + "umi_dedup_summary.tsv", log_prefix)
    write_read_summary(eng, dist, prefix + "read_summary.tsv", mode, log_prefix)
    write_cell_summary(eng, dist, prefix + "cell_summary.tsv", samples, mode, log_prefix)
    write_feature_summary(eng, dist, prefix + "feature_summary.tsv", regions, mode, log_prefix)
    if snps is not None and (mode is None or mode & XCK_MODE_BAF):
        write_snp_summary(eng, dist, prefix + "snp_summary.tsv", snps, mode, log_prefix)
    if getattr(eng, "mode", 0) & XCK_MODE_BAF and (mode is None or mode & XCK_MODE_BAF):
        write_molecule_summary(eng, dist, prefix + "molecule_summary.tsv", log_prefix)


# ----------------------------------------------------------------------------- engine driver
def make_engine(conf, mode, regions, snps=(), device=None, **extra):
    """Build the per-GPU engine from a resolved Config."""
    names = contig_table(regions, snps)
    if device is None:
        device = int(os.environ.get("XCK_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    kw = dict(min_mapq=conf.min_mapq, min_len=conf.min_len, incl_flag=conf.incl_flag,
              excl_flag=conf.excl_flag, no_orphan=conf.no_orphan, n_threads=max(0, int(conf.nproc)))
    if mode == XCK_MODE_BASEFC:
        kw["min_include"] = conf.min_include
    else:
        kw.update(min_count=conf.min_count, min_maf=conf.min_maf, no_dup_hap=conf.no_dup_hap)
    kw.update(extra)
    dist = Dist()
    if dist.active:                                   # multi-GPU: this rank counts the regions of its contigs (or contig pieces)
        dist.plan(conf, regions, snps)
        kw["region_mask"] = dist.region_mask
        # unique-feature molecules: a molecule is judged on the keys of its whole contig, so the pieces of a contig must be one rank's
        if mode & XCK_MODE_BASEFC and (kw.get("umi_feature") == "unique" or os.environ.get("XCK_UMI_FEATURE", "") == "unique"):
            owners = {}
            for u, r in zip(dist.units, dist.unit_owner.tolist()):
                owners.setdefault(u["contig"], set()).add(r)
            cut = [names[c] for c in sorted(owners) if len(owners[c]) > 1]
            if cut:
                raise XckError("XCK_UMI_FEATURE=unique: the multi-GPU plan cuts contig %s over ranks, and a molecule with keys on both sides of "
                               "a cut would be judged by two ranks; run with fewer ranks or without the knob." % ", ".join(cut))
    eng = Engine(mode, names, regions, len(conf.samples), snps=snps,
                 barcodes=conf.barcodes if conf.use_barcodes() else None,
                 cell_tag=conf.cell_tag, umi_tag=conf.umi_tag, device=device, **kw)
    eng.dist = dist
    return eng


def dist_requested():
    """True when the environment asks for a multi-GPU run (several ranks, or XCK_DIST_FORCE): what makes a Dist active, asked
    without making one."""
    return int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("XCK_DIST_FORCE", "0") not in ("", "0")


class Dist(object):
    """Multi-GPU context (one process per GPU).  With WORLD_SIZE > 1 every
    rank builds the full tables, streams only the contigs it owns (LPT on .bai record counts,
    contig lengths as fallback; an over-weight contig is cut at region boundaries).  The results meet in one of two ways:
    every rank writes the lines of its own rows into the shared output files (default: one all-reduce of text sizes per
    file), or - XCK_DIST_GATHER=1 - the per-rank sparse blocks are concatenated on rank 0 by one all-gatherv.  RCCL over
    xGMI with the nccl backend; gloo when XCK_DIST_BACKEND=gloo."""

    def __init__(self):
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.backend = None
        self.device = "cpu"
        # XCK_DIST_FORCE=1: take the multi-rank code path with ONE rank as well (communicator, collectives, gather and the sharded
        # writer all run, over a world of one) - how the one-GPU test box exercises the RCCL backend
        self.forced = self.world == 1 and os.environ.get("XCK_DIST_FORCE", "0") not in ("", "0")
        # how the ranks' results meet: every rank writes the lines of its own rows into the shared output files (default; the
        # ranks of one node see the same directory), or XCK_DIST_GATHER=1: the sparse blocks are gathered on rank 0, which writes
        self.sharded_output = False
        if self.world > 1 or self.forced:
            import torch
            import torch.distributed as dist
            self.backend = os.environ.get("XCK_DIST_BACKEND", "nccl")
            if not dist.is_initialized():
                if self.forced:
                    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                    os.environ.setdefault("MASTER_PORT", "29533")
                kw = dict(rank=self.rank, world_size=self.world) if self.forced else {}
                if self.backend == "nccl":
                    torch.cuda.set_device(self.local_rank)
                    dist.init_process_group("nccl", device_id=torch.device("cuda", self.local_rank), **kw)
                else:
                    dist.init_process_group(self.backend, **kw)
            if self.backend == "nccl":
                self.device = "cuda:%d" % self.local_rank
            self.sharded_output = os.environ.get("XCK_DIST_GATHER", "0") in ("", "0")
            # Ranks that SHARE a GPU (fewer devices than ranks on this node: test rehearsals, oversubscribed nodes) keep the BGZF inflate on the
            # host: the device decoder's launches run for tens of milliseconds, and the GPU time-slices between processes at that grain - the
            # other rank's join kernels then wait behind them (measured on one GPU with two ranks: 40 M reads/s host-only, 4.8 M with the
            # device share).  One GPU per rank - the deployment - is not affected.  (The engine reads the knob at xck_create.)
            try:
                # (ranks on THIS node: torchrun says so; without it, a rendezvous on this host means all ranks are here - otherwise unknown, no guess)
                one_node = os.environ.get("MASTER_ADDR", "") in ("127.0.0.1", "localhost", "::1")
                local_world = int(os.environ["LOCAL_WORLD_SIZE"]) if "LOCAL_WORLD_SIZE" in os.environ else (self.world if one_node else 0)
                if self.world > 1 and torch.cuda.device_count() < local_world:
                    os.environ.setdefault("XCK_GPU_INFLATE", "0")
            except Exception:
                pass

    @property
    def active(self):
        return self.world > 1 or self.forced

    def plan(self, conf, regions, snps=(), names=None):
        """Who counts what (identical on every rank): contigs by longest-processing-time on the .bai record counts; a contig
        that outweighs 1 / world of the reads is cut at region boundaries (shard.plan_units).  Sets contig_mask (contigs this
        rank streams), windows ({contig: (beg0, end0)} for the cut ones), region_mask (regions this rank counts) and
        row_owner (rank per region, for stitching the gathered blocks)."""
        from .shard import plan_units
        if names is None:
            names = contig_table(regions, snps)
        probe = Engine(XCK_MODE_BASEFC, names, [], 1, decode_only=True)
        try:
            weights = np.zeros(len(names), dtype=np.float64)
            for fn in conf.sam_fn_list:
                c = probe.contig_record_counts(fn)
                if c is None:                           # no index: every contig weighs the same
                    weights[:] = 1.0
                    break
                weights += c
            heavy = [c for c in range(len(names)) if weights.sum() > 0 and weights[c] > weights.sum() / self.world * 1.02]
            profiles = {}
            for c in heavy:                            # byte profile of the first BAM that has one (cuts are positions, valid for every BAM)
                for fn in conf.sam_fn_list:
                    pr = probe.contig_byte_profile(fn, c)
                    if pr is not None:
                        profiles[c] = pr
                        break
        finally:
            probe.close()
        cidx = {n: i for i, n in enumerate(names)}
        units, owner = plan_units(weights + 1e-9, self.world, regions, cidx, profiles)
        self.units, self.unit_owner, self.contig_weights = units, owner, weights
        self.contig_mask = np.zeros(len(names), dtype=bool)
        self.region_mask = np.zeros(len(regions), dtype=bool)
        self.row_owner = np.full(len(regions), -1, dtype=np.int32)
        self.windows = {}
        for u, r in zip(units, owner.tolist()):
            self.row_owner[u["regions"]] = r
            if r != self.rank:
                continue
            self.contig_mask[u["contig"]] = True
            self.region_mask[u["regions"]] = True
            if u["window"] is not None:
                if u["contig"] in self.windows:          # two pieces of one contig on this rank: their hull
                    b0, e0 = self.windows[u["contig"]]
                    nb, ne = u["window"]
                    self.windows[u["contig"]] = (min(b0, nb), 0 if (e0 == 0 or ne == 0) else max(e0, ne))
                else:
                    self.windows[u["contig"]] = u["window"]
        # a rank that holds pieces next to whole contigs: whole contigs have no window (decoded entirely)
        return self

    # -- the collectives the sharded writer needs (tiny tensors; RCCL with the nccl backend, gloo in the shared-GPU tests)
    def all_reduce_np(self, x, op="sum"):
        import torch
        import torch.distributed as td
        t = torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        td.all_reduce(t, op=td.ReduceOp.MAX if op == "max" else td.ReduceOp.SUM)
        return t.cpu().numpy()

    def barrier(self):
        import torch.distributed as td
        td.barrier()

    def gather(self, eng, regions):
        """all-gatherv of the per-rank sparse blocks to rank 0, straight from HBM (xck_get_result_device): one
        all-gather of sizes + one padded gather (RCCL over xGMI; host tensors over gloo).  Ranks own whole contigs,
        hence disjoint rows: rank 0 stitches the row runs together without sorting.  -> coo dict on rank 0, else None."""
        import torch
        from .shard import BlockGatherer, merge_row_blocks
        nccl = self.backend == "nccl"
        dev = torch.device(self.device) if nccl else torch.device("cuda", int(os.environ.get("XCK_DEVICE", self.local_rank if torch.cuda.device_count() > self.local_rank else 0)))
        blocks = eng.result_device()
        g = BlockGatherer(self.world, self.rank, dev, names=tuple(blocks), backend_is_nccl=nccl)
        g.start(blocks)
        res = g.wait()
        if self.rank != 0:
            return None
        return {k: merge_row_blocks([b.cpu().numpy() for b in res[k]], self.row_owner) for k in res}


def stream_bams(eng, conf, log_prefix="[engine]", contig_mask=None, windows=None):
    """One streaming pass over every BAM, in list order (= the reference's fetch order)."""
    t0 = time.time()
    n_tot = 0
    def per_file(i, fn, n):
        if conf.debug > 0:
            info("%s %s: %d records" % (log_prefix, fn, n))
    # (the next file reads ahead while this one is parsed and joined: Engine.ingest_bams)
    n_tot = eng.ingest_bams(list(conf.sam_fn_list), contig_mask=contig_mask, use_index=contig_mask is not None, windows=windows or None, on_file=per_file)
    dt = max(time.time() - t0, 1e-9)
    info("%s %d BAM record(s) decoded and joined in %.2fs (%.0f reads/s)" % (log_prefix, n_tot, dt, n_tot / dt))
    return n_tot


def log_tag_filter(eng, dist, log_prefix="[engine]"):
    """One log line when the handle filters its reads on a tag (Engine(tag_filter=...), or XCK_TAG_FILTER in the environment): the
    predicate and the records it rejected, summed over the ranks of a multi-GPU run (then a collective call).  Returns the number or None."""
    tf = getattr(eng, "tag_filter", None)
    if not tf:
        return None
    n = np.array([eng.decode_stats()["tag_filtered"]], dtype=np.int64)
    if dist is not None and dist.active:
        n = dist.all_reduce_np(n)
    info("%s tag filter %s: (value & 0x%X) == %d: %d record(s) filtered out" % (log_prefix, tf[0], tf[2], tf[1], int(n[0])))
    return int(n[0])


def log_min_baseq(eng, dist, log_prefix="[engine]"):
    """One log line when the handle's pileup runs with a base-quality floor (Engine(min_baseq=...), or XCK_MIN_BASEQ in the environment):
    the floor, the (read, SNP) pairs in which the read stores a base and those of them the floor masked, summed over the ranks of a
    multi-GPU run (then a collective call; where a contig is cut over ranks both neighbours count the reads at the cut).  Returns
    the (summed) dict or None."""
    baseq_stats = getattr(eng, "baseq_stats", None)            # (an engine-like object without the method masks nothing)
    st = baseq_stats() if baseq_stats and getattr(eng, "min_baseq", 0) else None
    if st is None:
        return None
    n = np.array([st["pairs_with_base"], st["pairs_masked"]], dtype=np.int64)
    if dist is not None and dist.active:
        n = dist.all_reduce_np(n)
    info("%s min base quality %d: %d (read, SNP) pair(s) with a base, %d masked" % (log_prefix, st["min_baseq"], int(n[0]), int(n[1])))
    return dict(st, pairs_with_base=int(n[0]), pairs_masked=int(n[1]))


def make_and_count(conf, mode, regions, snps=(), log_prefix="[engine]", gather=None, **extra):
    """Build the engine, stream every BAM (this rank's contigs when running multi-GPU), fold, gather.  Keys that are not ACGT strings (IUPAC UMIs, integer tags, read names in UMI-less runs) are
    interned on the host and take one id each; when the ids outgrow the UMI field of a 64-bit key the decoder stops with
    XCK_E_CAPACITY - the run is then repeated once with 128-bit keys (XCK_F_FORCE_KEY128), on every rank of a multi-GPU run.
    Multi-GPU: by default every rank gets ITS OWN rows back (dist.sharded_output) and the ranks write the files together
    (output_row_map / write_mtx below are then collective calls); gather=True, or XCK_DIST_GATHER=1, gathers the blocks on
    rank 0 instead (coo is None on the other ranks).
    Returns (engine - the caller closes it, coo or None, Dist)."""
    from .capi import XCK_E_CAPACITY, XCK_F_FORCE_KEY128
    flags = int(extra.pop("flags", 0))
    while True:
        eng = make_engine(conf, mode, regions, snps, flags=flags, **extra)
        dist, overflow, failure = eng.dist, 0, None
        try:
            stream_bams(eng, conf, log_prefix, dist.contig_mask if dist.active else None, dist.windows if dist.active else None)
        except XckError as e:
            failure = e
            overflow = int(getattr(e, "code", 0) == XCK_E_CAPACITY and not flags & XCK_F_FORCE_KEY128)
        except BaseException:
            eng.close()
            raise
        if dist.active:                                   # the ranks agree: one overflow sends all of them round again
            import torch
            import torch.distributed as td
            t = torch.tensor([overflow, int(failure is not None)], dtype=torch.int64, device=dist.device)
            td.all_reduce(t, op=td.ReduceOp.MAX)
            overflow, any_failure = int(t[0]), int(t[1])
            if any_failure and not overflow and failure is None:
                failure = XckError("another rank failed")
        if overflow:
            eng.close()
            warn("%s key ids exceed the 64-bit key layout; counting again with 128-bit keys." % log_prefix)
            flags |= XCK_F_FORCE_KEY128
            continue
        if failure is not None:
            eng.close()
            raise failure
        log_tag_filter(eng, dist, log_prefix)
        log_min_baseq(eng, dist, log_prefix)
        try:
            coo = eng.finish(copy=False)
            if gather is not None:
                dist.sharded_output = dist.active and not gather
            if dist.active and not dist.sharded_output:
                coo = dist.gather(eng, conf.reg_list)              # rank 0: merged matrices; other ranks: None
        except BaseException:
            eng.close()
            raise
        return eng, coo, dist


def run_logged(core, conf):
    """core(conf) between the reference's start / CMD / end log lines (rdr/fc/main.py:270-302, baf/fc/main.py:262-294): 0, or -1
    with the error logged when it raises ValueError or XckError."""
    ret = -1
    cmdline = None
    start_time = time.time()
    info("start time: %s." % time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(start_time)))
    if conf.argv is not None:
        cmdline = " ".join(conf.argv)
        info("CMD: %s" % cmdline)
    try:
        core(conf)
    except (ValueError, XckError) as e:
        error(str(e))
        error("Running program failed.")
        error("Quiting ...")
        ret = -1
    else:
        info("All Done!")
        ret = 0
    finally:
        if conf.argv is not None:
            info("CMD: %s" % cmdline)
        end_time = time.time()
        info("end time: %s" % time.strftime("%Y-%m-%d %H:%M:%S", time.localtime(end_time)))
        info("time spent: %.2fs" % (end_time - start_time))
    return ret
