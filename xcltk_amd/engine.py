"""engine.py - Python handle on the HIP counting engine (libxck.so) through the C-ABI.

One `Engine` drives one GPU.  It owns the region / SNP tables, the decoder settings
(barcode list, tag names) and the device-side hit accumulators; BAM files are streamed
through it once (`ingest_bam`) or record batches are pushed directly (`push`), and
`finish()` returns the sparse matrices as COO triplets.

There is no CPU compute path here: constructing an Engine without a usable HIP device
raises (the only exception is `decode_only=True`, which gives access to the host BAM
decoder alone and refuses push/finish).
"""

import ctypes as C
import os
from logging import info

import numpy as np

from . import capi
from .snptable import SnpTable
from .capi import XCK_MODE_BAF, XCK_MODE_BASEFC


class XckError(RuntimeError):
    """Engine / decoder failure; `code` holds the C-ABI error code (include/xck.h XCK_E_*) when there is one."""
    def __init__(self, msg, code=0):
        RuntimeError.__init__(self, msg)
        self.code = code


def resolve_contigs(bam_refs, contig_names):
    """tid -> engine contig id, with the reference's chr-prefix tolerance
    (sam_fetch, xcltk/utils/sam.py:105-118: try the name, then the name with 'chr'
    added / removed)."""
    tid_of = {}
    for i, n in enumerate(bam_refs):
        tid_of.setdefault(n, i)
    t2c = np.full(len(bam_refs), -1, dtype=np.int32)
    for ci, x in enumerate(contig_names):
        if x in tid_of:
            t2c[tid_of[x]] = ci
        else:
            y = x[3:] if x.startswith("chr") else "chr" + x
            if y in tid_of:
                t2c[tid_of[y]] = ci
    return t2c


def _parse_tag_filter(text):
    """(tag, value, mask) of an XCK_TAG_FILTER value TAG:VALUE[/MASK] (include/xck.h), or None where xck_create will refuse it"""
    num = lambda x: int(x, 16) if x[:2].lower() == "0x" else int(x, 10)
    try:
        value, _, mask = text[3:].partition("/")
        return (text[:2], num(value), num(mask) if mask else 0xFFFFFFFF) if text[2:3] == ":" else None
    except ValueError:
        return None


def region_array(regions, cidx, strict=True):
    """xck_region records of (chrom, start1, end1_incl[, name]) tuples; strict=False: a chrom outside cidx becomes contig -1."""
    # column-wise fills (a per-row structured assignment costs ~1.5 us: 1.5 s for 1 M SNPs)
    reg = np.zeros(len(regions), dtype=capi.REGION_DTYPE)
    if len(regions):
        reg["contig"] = [cidx[r[0]] for r in regions] if strict else [cidx.get(r[0], -1) for r in regions]
        reg["start"] = [r[1] for r in regions]
        reg["end"] = [r[2] for r in regions]
    return reg


def snp_array(snps, cidx):
    """xck_snp records of a SnpTable or of (chrom, pos1, ref, alt, ref_hap, alt_hap) tuples."""
    snp = np.zeros(len(snps), dtype=capi.SNP_DTYPE)
    if isinstance(snps, SnpTable):
        if len(snps):
            if int(snps.pos.max()) > 2 ** 31 - 1 or int(snps.pos.min()) < -2 ** 31:
                raise OverflowError("SNP position does not fit the engine's int32 coordinate")
            snp["contig"] = np.array([cidx[n] for n in snps.names], dtype=np.int32)[snps.chrom_id]
            snp["pos"] = snps.pos
            snp["ref"] = snps.ref
            snp["alt"] = snps.alt
            snp["ref_hap"] = snps.ref_hap
            snp["alt_hap"] = snps.alt_hap
    elif len(snps):
        snp["contig"] = [cidx[s[0]] for s in snps]
        snp["pos"] = [s[1] for s in snps]
        snp["ref"] = [ord(s[2]) for s in snps]
        snp["alt"] = [ord(s[3]) for s in snps]
        snp["ref_hap"] = [s[4] for s in snps]
        snp["alt_hap"] = [s[5] for s in snps]
    return snp


class Engine(object):
    def __init__(self, mode, contig_names, regions, n_cells, snps=(), barcodes=None,
                 cell_tag=None, umi_tag=None, device=0, min_mapq=20, min_len=30,
                 incl_flag=0, excl_flag=772, no_orphan=True, min_include=0.9, min_count=1,
                 min_maf=0, no_dup_hap=True, n_threads=0, flags=0, decode_only=False, excl_pairs=None, region_mask=None, tag_filter=None,
                 umi_consensus=False, min_baseq=0, umi_feature=None, umi_dedup=None, base_tally=False, contig_len=None):
        """regions: iterable of (chrom, start1, end1_incl[, name]); snps: iterable of
        (chrom, pos1, ref, alt, ref_hap, alt_hap); chrom names must already be stripped of
        'chr' and present in contig_names.  excl_pairs = (region indices, snp indices): pairs left out of the SNP -> region
        join (region-wise local phasing, xck_config.excl_*).  region_mask (bool per region): regions that are False keep
        their row index but are not counted by this engine (multi-GPU: another rank owns them).  tag_filter = (tag, value) or
        (tag, value, mask): only records whose first `tag` is an integer v >= 0 with (v & mask) == value count (xck_config.filter_tag;
        mask defaults to 0xFFFFFFFF; ("xf", 25) keeps what Cell Ranger counted); None leaves it to XCK_TAG_FILTER in the environment.
        self.tag_filter is the (tag, value, mask) the handle applies, or None.  umi_consensus=True (XCK_F_UMI_CONSENSUS; needs a BAF
        pipeline): the base of a molecule is a plurality vote over its reads instead of its first read's, reads that span the SNP
        in a gap abstain, and molecule_stats() says how often the reads of a molecule disagree; XCK_UMI_CONSENSUS=1 in the
        environment does the same for every handle with a BAF pipeline.  min_baseq=Q (1 .. 93, xck_config.min_baseq; needs a BAF
        pipeline; set together with XCK_F_MIN_BASEQ): a base whose quality is below Q (and stored: not 0xff) is not shown at its SNP, as `samtools mpileup -Q` / pysam's
        min_base_quality do; the qualities come from ingest_bam() or push_batch(..., qual=), and baseq_stats() counts what was masked;
        XCK_MIN_BASEQ in the environment supplies it where it is 0.  self.min_baseq is the floor the handle runs with.
        umi_feature="unique" (XCK_F_UNIQUE_FEATURE; needs a basefc pipeline): a molecule (contig, cell, UMI) counts only when exactly
        one region of its contig accepted its reads - one that two or more regions hold is dropped from all of them - and
        umi_feature_stats() says how many were; None and "all" count every (region, cell, UMI), the default;
        XCK_UMI_FEATURE=unique in the environment does the same for every handle with a basefc pipeline.
        umi_dedup="1mm_all" (XCK_F_UMI_COLLAPSE; needs a basefc pipeline): within one (region, cell) UMIs joined by chains of single-base
        substitutions count as one molecule (STARsolo's 1MM_All, UMI-tools' cluster), and umi_dedup_stats() says what was merged; with
        umi_feature="unique" that rule runs first, on exact UMIs; None and "exact" count every distinct UMI, the default;
        XCK_UMI_DEDUP=1mm_all in the environment does the same for every handle with a basefc pipeline.
        base_tally=True (XCK_F_BASE_TALLY; needs a BAF pipeline): the handle keeps pseudo-bulk A / C / G / T counters per reference
        position of every contig that receives reads (16 bytes a position), read by base_tally(), base_tally_stats() and
        find_candidates().  contig_len: one length per contig (xck_set_contig_lengths); omitted, ingest_bam() / ingest_bams() take the
        lengths from the first BAM's header, and push() needs set_contig_lengths() first."""
        self.lib = capi.load()
        self.mode = mode
        self.contig_names = list(contig_names)
        cidx = {n: i for i, n in enumerate(self.contig_names)}
        regions = list(regions)
        if not isinstance(snps, SnpTable):
            snps = list(snps)
        self._reg = region_array(regions, cidx)
        if regions and region_mask is not None:
            self._reg["contig"][~np.asarray(region_mask, dtype=bool)] = -1
        self._snp = snp_array(snps, cidx)
        cfg = capi.Config()
        cfg.struct_size = C.sizeof(capi.Config)
        cfg.mode = mode
        cfg.device = device
        cfg.min_mapq = float(min_mapq)
        cfg.min_len = int(min_len)
        cfg.incl_flag = int(incl_flag)
        cfg.excl_flag = int(excl_flag)
        cfg.no_orphan = 1 if no_orphan else 0
        cfg.min_include = float(min_include)
        cfg.min_count = float(min_count)
        cfg.min_maf = float(min_maf)
        cfg.no_dup_hap = 1 if no_dup_hap else 0
        cfg.n_cells = int(n_cells)
        cfg.n_contigs = len(self.contig_names)
        cfg.n_regions = len(regions)
        cfg.regions = self._reg.ctypes.data_as(C.POINTER(capi.Region))
        cfg.n_snps = len(snps)
        cfg.snps = self._snp.ctypes.data_as(C.POINTER(capi.Snp))
        self._bc = None
        if barcodes is not None:
            assert len(barcodes) == n_cells
            self._bc = (C.c_char_p * len(barcodes))(*[b.encode("ascii") for b in barcodes])
            cfg.barcodes = C.cast(self._bc, C.POINTER(C.c_char_p))
            if not cell_tag or len(cell_tag) != 2:
                raise ValueError("cell_tag must be a 2-character tag when barcodes are given")
            cfg.cell_tag = cell_tag.encode("ascii")
        if umi_tag:
            if len(umi_tag) != 2:
                raise ValueError("umi_tag must be a 2-character tag")
            cfg.umi_tag = umi_tag.encode("ascii")
        self._excl = None
        if excl_pairs is not None and len(excl_pairs[0]):
            er = np.ascontiguousarray(excl_pairs[0], dtype=np.int32)
            es = np.ascontiguousarray(excl_pairs[1], dtype=np.int32)
            assert len(er) == len(es)
            self._excl = (er, es)
            cfg.n_excl_pairs = len(er)
            cfg.excl_region = er.ctypes.data_as(C.POINTER(C.c_int32))
            cfg.excl_snp = es.ctypes.data_as(C.POINTER(C.c_int32))
        self.tag_filter = None
        if tag_filter is not None:
            if len(tag_filter) not in (2, 3) or not isinstance(tag_filter[0], str):
                raise ValueError("tag_filter must be (tag, value) or (tag, value, mask)")
            tag, value = tag_filter[0], int(tag_filter[1])
            mask = int(tag_filter[2]) if len(tag_filter) == 3 else 0xFFFFFFFF
            if len(tag) != 2:
                raise ValueError("tag_filter: the tag must be a 2-character tag")
            if not (0 <= value <= 0xFFFFFFFF and 0 <= mask <= 0xFFFFFFFF):
                raise ValueError("tag_filter: value and mask must fit 32 bits")
            cfg.filter_tag = tag.encode("latin-1")
            cfg.filter_mask, cfg.filter_value = mask, value
            self.tag_filter = (tag, value, mask)
        elif os.environ.get("XCK_TAG_FILTER"):                      # (xck_create checks the knob: a malformed one fails below)
            self.tag_filter = _parse_tag_filter(os.environ["XCK_TAG_FILTER"])
        cfg.n_threads = int(n_threads)
        self.min_baseq = int(min_baseq)
        if not self.min_baseq and not decode_only and (mode & XCK_MODE_BAF):     # (xck_create checks the knob: a malformed one fails below)
            knob = os.environ.get("XCK_MIN_BASEQ", "")
            self.min_baseq = int(knob) if knob.isdigit() else 0
        if umi_feature not in (None, "all", "unique"):
            raise ValueError("umi_feature must be None, 'all' or 'unique'")
        if umi_dedup not in (None, "exact", "1mm_all"):
            raise ValueError("umi_dedup must be None, 'exact' or '1mm_all'")
        cfg.flags = (int(flags) | (capi.XCK_F_DECODE_ONLY if decode_only else 0) | (capi.XCK_F_UMI_CONSENSUS if umi_consensus else 0)
                     | (capi.XCK_F_UNIQUE_FEATURE if umi_feature == "unique" else 0) | (capi.XCK_F_UMI_COLLAPSE if umi_dedup == "1mm_all" else 0)
                     | (capi.XCK_F_BASE_TALLY if base_tally else 0))
        cfg.min_baseq = int(min_baseq)                              # (behind the flags: a non-zero value sets XCK_F_MIN_BASEQ beside it)
        self.cfg = cfg
        self.n_cells = int(n_cells)
        self.n_regions = len(regions)
        h = C.c_void_p()
        rc = self.lib.xck_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise XckError("xck_create failed (%d): %s" % (rc, self.lib.xck_last_error(None).decode()), rc)
        self.h = h
        self.umi_bits = self.lib.xck_umi_bits(self.h)
        self._result = None
        self.base_tally_on = bool(cfg.flags & capi.XCK_F_BASE_TALLY)
        self.contig_len = None
        self.ref_loaded = False                                     # set_reference() has loaded a sequence: find_candidates() orients by it
        if contig_len is not None:
            self.set_contig_lengths(contig_len)

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "h", None):
            self.lib.xck_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise XckError("%s failed (%d): %s" % (what, rc, self.lib.xck_last_error(self.h).decode()), rc)

    # ------------------------------------------------------------------ data path
    def push(self, batch, device_resident=False):
        fn = self.lib.xck_push_batch_device if device_resident else self.lib.xck_push_batch
        self._check(fn(self.h, C.byref(batch)), "xck_push_batch")

    def push_batch(self, batch, qual=None):
        """push(), with the reads' base qualities for a handle with min_baseq (xck_push_batch_q): qual is a uint8 array of
        2 * (seq_off[n] - seq_off[0]) bytes, the quality of query offset qi of read i at 2 * (seq_off[i] - seq_off[0]) + qi, the pad
        byte of an odd-length read 0xff (0xff: no quality stored).  A handle without a floor ignores it."""
        if qual is None:
            return self.push(batch)
        q = np.ascontiguousarray(qual, dtype=np.uint8)
        n = int(batch.n_reads)
        if n > 0 and bool(batch.seq_off):
            need = 2 * (int(batch.seq_off[n]) - int(batch.seq_off[0]))
            if len(q) < need:
                raise ValueError("qual holds %d bytes, the batch needs %d" % (len(q), need))
        self._check(self.lib.xck_push_batch_q(self.h, C.byref(batch), q.ctypes.data_as(C.POINTER(C.c_uint8))), "xck_push_batch_q")

    def flush(self):
        self._check(self.lib.xck_flush(self.h), "xck_flush")

    def reset(self):
        self._check(self.lib.xck_reset(self.h), "xck_reset")
        self._result = None

    def set_contig_lengths(self, contig_len):
        """The contigs' lengths of a base_tally handle (xck_set_contig_lengths): one per contig, each in 1 .. 2^31 - 1, before the
        first push since the constructor or reset()."""
        v = np.ascontiguousarray(contig_len, dtype=np.int64)
        self._check(self.lib.xck_set_contig_lengths(self.h, capi.np_ptr(v, C.c_int64), len(v)), "xck_set_contig_lengths")
        self.contig_len = v.copy()

    def _lengths_from_bam(self, b, refs):
        """a base_tally handle without lengths: those of the open BAM's header, through the contig mapping (a contig the BAM does
        not name gets length 1: no read can reach it)"""
        if not self.base_tally_on or self.contig_len is not None:
            return
        v = np.ones(len(self.contig_names), dtype=np.int64)
        for tid, c in enumerate(resolve_contigs(refs, self.contig_names).tolist()):
            if c >= 0:
                v[c] = max(1, int(self.lib.xck_bam_ref_len(b, tid)))
        self.set_contig_lengths(v)

    def _open(self, path, n_threads=0):
        b = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = self.lib.xck_bam_open(path.encode(), n_threads, C.byref(b), err, 512)
        if rc != 0:
            raise XckError("xck_bam_open failed (%d): %s" % (rc, err.value.decode()), rc)
        refs = [self.lib.xck_bam_ref_name(b, i).decode() for i in range(self.lib.xck_bam_n_refs(b))]
        return b, refs

    def _opts(self, refs, sample, max_records=0, contig_mask=None, use_index=False, windows=None):
        """windows: {engine contig id: (beg0, end0)} - only the records of that contig from the first one overlapping beg0 up to
        the last one starting before end0 (0 / None = open end) are decoded (needs use_index and a .bai with a linear index)."""
        t2c = resolve_contigs(refs, self.contig_names)
        if contig_mask is not None:                     # multi-GPU: this rank only owns some contigs
            keep = np.asarray(contig_mask, dtype=bool)
            t2c = np.where((t2c >= 0) & keep[np.maximum(t2c, 0)], t2c, -1).astype(np.int32)
        o = capi.IngestOpts()
        o.struct_size = C.sizeof(capi.IngestOpts)
        o.sample = sample
        o.tid_to_contig = t2c.ctypes.data_as(C.POINTER(C.c_int32))
        o.max_records = max_records
        o.use_index = 1 if use_index else 0
        if windows:
            beg = np.zeros(len(refs), dtype=np.int32); end = np.zeros(len(refs), dtype=np.int32)
            for tid, c in enumerate(t2c.tolist()):
                if c >= 0 and c in windows:
                    beg[tid], end[tid] = int(windows[c][0] or 0), int(windows[c][1] or 0)
            o.tid_beg = beg.ctypes.data_as(C.POINTER(C.c_int32)); o.tid_end = end.ctypes.data_as(C.POINTER(C.c_int32))
            o._keep = (beg, end)
        return o, t2c

    def contig_record_counts(self, path):
        """Records per engine contig from the BAM's .bai (None if there is no usable index)."""
        b, refs = self._open(path, 1)
        try:
            t2c = resolve_contigs(refs, self.contig_names)
            out = np.zeros(len(self.contig_names), dtype=np.int64)
            m, u = C.c_int64(0), C.c_int64(0)
            for tid, c in enumerate(t2c.tolist()):
                if c < 0:
                    continue
                if self.lib.xck_bam_ref_records(b, tid, C.byref(m), C.byref(u)) != 0:
                    return None
                out[c] += m.value + u.value
            return out
        finally:
            self.lib.xck_bam_close(b)

    def contig_byte_profile(self, path, contig):
        """Compressed file offset of the first record overlapping every 16 kb window of one engine contig (from the .bai linear
        index; None without one): differences weigh the reads between two positions."""
        b, refs = self._open(path, 1)
        try:
            t2c = resolve_contigs(refs, self.contig_names)
            tids = [t for t, c in enumerate(t2c.tolist()) if c == contig]
            if not tids:
                return None
            n, ptr = C.c_int64(0), C.POINTER(C.c_uint64)()
            if self.lib.xck_bam_linear_index(b, tids[0], C.byref(n), C.byref(ptr)) != 0 or n.value == 0:
                return None
            v = np.ctypeslib.as_array(ptr, shape=(n.value,)).copy()
            return (v >> np.uint64(16)).astype(np.int64)
        finally:
            self.lib.xck_bam_close(b)

    def ingest_bam(self, path, sample=0, n_threads=0, max_records=0, contig_mask=None, use_index=False, windows=None):
        """Decode one BAM file and run the join kernels on every batch. Returns #records decoded.
        contig_mask (bool per engine contig) restricts the pass to the contigs this rank owns;
        with use_index the .bai is used to inflate only their byte ranges."""
        b, refs = self._open(path, n_threads or self.cfg.n_threads)
        try:
            self._lengths_from_bam(b, refs)
            o, keep = self._opts(refs, sample, max_records, contig_mask, use_index, windows)
            n = C.c_int64(0)
            self._check(self.lib.xck_ingest_bam(self.h, b, C.byref(o), C.byref(n)), "xck_ingest_bam")
            return int(n.value)
        finally:
            self.lib.xck_bam_close(b)

    def ingest_bams(self, paths, n_threads=0, contig_mask=None, use_index=False, windows=None, on_file=None, ahead=2):
        """ingest_bam() over a list of files, sample = position in the list, with the next `ahead` files already open and reading
        ahead (xck_bam_prefetch: scanner + inflate, on the host pool or the GPU) while this one is parsed and joined - what pays with
        many small files (per-cell BAMs).  on_file(i, path, n_records) is called after each file.  Returns the total number of records."""
        total, queue, nxt_i = 0, [], 0                             # queue: [(b, opts, keep-alive)] of files nxt_i - len(queue) .. nxt_i - 1

        def prepare(i):
            b, refs = self._open(paths[i], n_threads or self.cfg.n_threads)
            try:
                self._lengths_from_bam(b, refs)
                o, keep = self._opts(refs, i, 0, contig_mask, use_index, windows)
            except Exception:
                self.lib.xck_bam_close(b)
                raise
            return (b, o, keep)

        try:
            for i, path in enumerate(paths):
                while nxt_i < len(paths) and nxt_i <= i + max(0, int(ahead)):
                    queue.append(prepare(nxt_i))
                    if nxt_i > i:
                        self.lib.xck_bam_prefetch(self.h, queue[-1][0], C.byref(queue[-1][1]))   # (best effort: an error shows up when the file is ingested)
                    nxt_i += 1
                cur = queue.pop(0)
                try:
                    n = C.c_int64(0)
                    self._check(self.lib.xck_ingest_bam(self.h, cur[0], C.byref(cur[1]), C.byref(n)), "xck_ingest_bam")
                finally:
                    self.lib.xck_bam_close(cur[0])
                total += int(n.value)
                if on_file:
                    on_file(i, path, int(n.value))
        finally:
            for q in queue:
                self.lib.xck_bam_close(q[0])
        return total

    def open_stream(self, path, sample=0, n_threads=0, contig_mask=None, use_index=False, windows=None):
        """Resumable ingest of one BAM: -> BamStream whose advance(n) decodes and joins about n further
        records (whole decode chunks) and returns (records so far, done)."""
        return BamStream(self, path, sample, n_threads, contig_mask, use_index, windows)

    def decode_bam(self, path, sample=0, n_threads=0, max_records=0, contig_mask=None, use_index=False, windows=None):
        """Pull-style decode (tests / inspection): yields dicts of numpy copies per batch."""
        b, refs = self._open(path, n_threads or self.cfg.n_threads)
        try:
            o, keep = self._opts(refs, sample, max_records, contig_mask, use_index, windows)
            bt = capi.Batch()
            while True:
                rc = self.lib.xck_bam_next_batch(self.h, b, C.byref(o), C.byref(bt))
                if rc == 0:
                    break
                if rc < 0:
                    self._check(rc, "xck_bam_next_batch")
                n = bt.n_reads
                as_np = np.ctypeslib.as_array
                d = dict(contig=bt.contig, n_reads=n, ordinal_base=int(bt.ordinal_base),
                         pos=as_np(bt.pos, (n,)).copy(), flag=as_np(bt.flag, (n,)).copy(),
                         mapq=as_np(bt.mapq, (n,)).copy(), cell=as_np(bt.cell, (n,)).copy(),
                         umi=as_np(bt.umi, (n,)).copy(), cig_off=as_np(bt.cig_off, (n + 1,)).copy())
                c_hi = int(d["cig_off"][-1])
                d["cigar"] = as_np(bt.cigar, (max(c_hi, 1),)).copy()
                if bt.seq_off:
                    d["seq_off"] = as_np(bt.seq_off, (n + 1,)).copy()
                    d["seq"] = as_np(bt.seq, (max(int(d["seq_off"][-1]), 1),)).copy()
                yield d
        finally:
            self.lib.xck_bam_close(b)

    def finish_async(self):
        """Run the fold on the GPU and enqueue the copy-out of the matrices without waiting for it."""
        self._check(self.lib.xck_finish_async(self.h), "xck_finish_async")

    def finish(self, copy=True):
        """-> {"count": (row, col, val)} or {"ad": .., "dp": .., "oth": ..}; rows are 0-based
        region indices (input order), cols 0-based cell indices, sorted by (row, col).
        copy=False returns views of the engine's pinned result buffers."""
        res = capi.Result()
        self._check(self.lib.xck_finish(self.h, C.byref(res)), "xck_finish")
        self._result = res
        out = {}
        if self.mode & XCK_MODE_BASEFC:
            out["count"] = res.count.to_numpy(copy)
        if self.mode & XCK_MODE_BAF:
            out.update(ad=res.ad.to_numpy(copy), dp=res.dp.to_numpy(copy), oth=res.oth.to_numpy(copy))
        return out

    def refold(self, regions, snps=None, snp_enabled=None, min_count=1, min_maf=0, no_dup_hap=True, excl_pairs=None, copy=True, cell_enabled=None):
        """Recount the pileup of the last finish() under new tables and filters, without the reads (xck_refold): returns what
        finish() returns, as a fresh engine would that was made with these tables and fed the same reads.  regions as for the
        constructor (a chrom outside contig_names gives an empty row); snps=None keeps the engine's, otherwise the same SNPs index
        by index with their own ref / alt / haplotype columns; snp_enabled (bool per SNP): False feeds no region; excl_pairs =
        (region indices into the NEW regions, snp indices).  cell_enabled (bool per cell of the engine; ValueError for another length):
        the recount is over these cells only - the matrices AND the per-SNP tallies min_count / min_maf are decided on - and equals
        what a fresh engine returns that saw the same reads with cell = -1 for the others; columns keep the engine's numbering.  The
        mask holds for this call: the next refold() without one counts every cell again, and snp_counts() always does.  Valid
        between finish() and reset(), as often as wanted."""
        if cell_enabled is not None:
            cen = np.ascontiguousarray(np.asarray(cell_enabled, dtype=bool).astype(np.uint8))
            if cen.ndim != 1 or len(cen) != self.n_cells:
                raise ValueError("cell_enabled needs one entry per cell of the engine (%d), got %s" % (self.n_cells, cen.shape))
        cidx = {n: i for i, n in enumerate(self.contig_names)}
        regions = list(regions)
        reg = region_array(regions, cidx, strict=False)
        cfg = capi.RefoldConfig()
        cfg.struct_size = C.sizeof(capi.RefoldConfig)
        cfg.n_regions = len(regions)
        cfg.regions = reg.ctypes.data_as(C.POINTER(capi.Region))
        keep = [reg]
        if snps is not None:
            if not isinstance(snps, SnpTable):
                snps = list(snps)
            snp = snp_array(snps, cidx)
            cfg.n_snps = len(snp)
            cfg.snps = snp.ctypes.data_as(C.POINTER(capi.Snp))
            keep.append(snp)
        if snp_enabled is not None:
            en = np.ascontiguousarray(np.asarray(snp_enabled, dtype=bool).astype(np.uint8))
            if len(en) != len(self._snp):
                raise ValueError("snp_enabled needs one entry per SNP of the engine")
            cfg.snp_enabled = en.ctypes.data_as(C.POINTER(C.c_uint8))
            keep.append(en)
        if cell_enabled is not None:
            cfg.cell_enabled = cen.ctypes.data_as(C.POINTER(C.c_uint8))
            keep.append(cen)
        cfg.min_count = float(min_count)
        cfg.min_maf = float(min_maf)
        cfg.no_dup_hap = 1 if no_dup_hap else 0
        if excl_pairs is not None and len(excl_pairs[0]):
            er = np.ascontiguousarray(excl_pairs[0], dtype=np.int32)
            es = np.ascontiguousarray(excl_pairs[1], dtype=np.int32)
            assert len(er) == len(es)
            cfg.n_excl_pairs = len(er)
            cfg.excl_region = er.ctypes.data_as(C.POINTER(C.c_int32))
            cfg.excl_snp = es.ctypes.data_as(C.POINTER(C.c_int32))
            keep += [er, es]
        res = capi.Result()
        self._check(self.lib.xck_refold(self.h, C.byref(cfg), C.byref(res)), "xck_refold")
        self._result = res
        self.n_regions = len(regions)
        out = {}
        if self.mode & XCK_MODE_BASEFC:
            out["count"] = res.count.to_numpy(copy)
        out.update(ad=res.ad.to_numpy(copy), dp=res.dp.to_numpy(copy), oth=res.oth.to_numpy(copy))
        return out

    def snp_counts(self, copy=True):
        """The SNP x cell matrices of the last finish() (xck_snp_counts): {"ad": (row, col, val), "dp": .., "oth": ..} with row =
        index into the SNP list the engine was made with, col = cell, sorted by (row, col) - what an engine with one one-base region
        per SNP (REF on haplotype 0, ALT on 1, min_count 1, min_maf 0) would return.  Every SNP counts, whatever regions, mask and
        filters the engine or its last refold() carry; REF / ALT are the current ones.  Valid between finish() and reset(); it
        leaves the results of finish() / refold() / result_device() alone.  copy=False returns views of the engine's pinned
        buffers, valid until the next snp_counts(), reset() or close()."""
        res = capi.Result()
        self._check(self.lib.xck_snp_counts(self.h, C.byref(res)), "xck_snp_counts")
        return dict(ad=res.ad.to_numpy(copy), dp=res.dp.to_numpy(copy), oth=res.oth.to_numpy(copy))

    def group_counts(self, cell_group, n_groups=None, source="result", copy=True):
        """The engine's matrices with their columns summed per cell group (xck_group_counts): cell_group[c] is the group of cell c,
        -1 leaves the cell out; n_groups defaults to max(cell_group) + 1.  source="result": the matrices of the last finish() /
        refold() -> {"count": (row, col, val)} and / or {"ad": .., "dp": .., "oth": ..} like finish(); source="snp": the blocks of the
        last snp_counts() -> {"ad", "dp", "oth"} with row = SNP.  col = group, sorted by (row, col), no zero entries.  Valid between
        finish() and reset(); it leaves every other result alone.  copy=False returns views of the engine's pinned buffers, valid
        until the next group_counts(), reset() or close()."""
        src = {"result": capi.XCK_GROUP_SRC_RESULT, "snp": capi.XCK_GROUP_SRC_SNP}.get(source, source)
        cg = np.ascontiguousarray(cell_group, dtype=np.int32)
        if cg.ndim != 1 or len(cg) != self.n_cells:
            raise ValueError("cell_group needs one entry per cell of the engine")
        if n_groups is None:
            n_groups = int(cg.max()) + 1 if len(cg) else 0
            n_groups = max(n_groups, 1)
        cfg = capi.GroupConfig()
        cfg.struct_size = C.sizeof(capi.GroupConfig)
        cfg.source = int(src)
        cfg.n_groups = int(n_groups)
        cfg.cell_group = capi.np_ptr(cg, C.c_int32)
        res = capi.Result()
        self._check(self.lib.xck_group_counts(self.h, C.byref(cfg), C.byref(res)), "xck_group_counts")
        out = {}
        if src == capi.XCK_GROUP_SRC_RESULT and self.mode & XCK_MODE_BASEFC:
            out["count"] = res.count.to_numpy(copy)
        if src == capi.XCK_GROUP_SRC_SNP or self.mode & XCK_MODE_BAF:
            out.update(ad=res.ad.to_numpy(copy), dp=res.dp.to_numpy(copy), oth=res.oth.to_numpy(copy))
        return out

    def result_device(self):
        """Device-resident copy of the last finish(): {name: (device_ptr_of_[row|col|val], nnz)}."""
        res = capi.Result()
        self._check(self.lib.xck_get_result_device(self.h, C.byref(res)), "xck_get_result_device")
        names = (["count"] if self.mode & XCK_MODE_BASEFC else []) + (["ad", "dp", "oth"] if self.mode & XCK_MODE_BAF else [])
        out = {}
        for k in names:
            coo = getattr(res, k)
            out[k] = (C.cast(coo.row, C.c_void_p).value or 0, int(coo.nnz))
        return out

    def write_mtx(self, path, name, row_map, n_rows_out):
        """Write matrix `name` of the last finish() in the reference's exact text format."""
        if self._result is None:
            raise XckError("finish() first")
        coo = getattr(self._result, name)
        rm = np.ascontiguousarray(row_map, dtype=np.int32)
        rc = self.lib.xck_write_mtx(path.encode(), C.byref(coo), rm.ctypes.data_as(C.POINTER(C.c_int32)),
                                    int(n_rows_out), self.n_cells)
        if rc != 0:
            raise XckError("xck_write_mtx failed (%d)" % rc)

    def write_mtx_arrays(self, path, coo, row_map, n_rows_out, n_cols=None):
        """Same writer for (row, col, val) arrays that did not come from this engine's last
        finish() - e.g. the blocks gathered from all ranks.  n_cols: the column count of the header (None = the engine's cells)."""
        row, col, val = (np.ascontiguousarray(a, dtype=np.int32) for a in coo)
        c = capi.Coo()
        c.nnz = len(row)
        c.row, c.col, c.val = (capi.np_ptr(a, C.c_int32) for a in (row, col, val))
        rm = np.ascontiguousarray(row_map, dtype=np.int32)
        rc = self.lib.xck_write_mtx(path.encode(), C.byref(c), rm.ctypes.data_as(C.POINTER(C.c_int32)),
                                    int(n_rows_out), self.n_cells if n_cols is None else int(n_cols))
        if rc != 0:
            raise XckError("xck_write_mtx failed (%d)" % rc)

    def stats(self):
        st = capi.Stats()
        self._check(self.lib.xck_get_stats(self.h, C.byref(st)), "xck_get_stats")
        return {k: getattr(st, k) for k, _ in capi.Stats._fields_}

    def decode_stats(self):
        """The BAM decoder's counters since the last reset (xck_get_decode_stats): GPU share of the inflate, CRC checks, chunks
        walked and parsed on the device, read names interned on the device (XCK_GPU_NAMES), records the tag filter rejected
        (tag_filtered)."""
        st = capi.DecodeStats()
        st.struct_size = C.sizeof(capi.DecodeStats)
        self._check(self.lib.xck_get_decode_stats(self.h, C.byref(st)), "xck_get_decode_stats")
        return {k: getattr(st, k) for k, _ in capi.DecodeStats._fields_ if k not in ("struct_size", "reserved0")}

    def _summary(self, what, struct, mode):
        """What read_fate / cell_summary / feature_summary share: `mode` defaults to the handle's own pipeline (ValueError on a
        XCK_MODE_BOTH handle, which has two), xck_get_<what> fills a `struct` -> the struct, or None where the handle keeps no such
        table (XCK_E_STATE)."""
        if mode is None:
            if self.mode == capi.XCK_MODE_BOTH:
                raise ValueError("%s(): a XCK_MODE_BOTH handle has two pipelines, name one" % what)
            mode = self.mode
        out = struct()
        out.struct_size = C.sizeof(struct)
        rc = getattr(self.lib, "xck_get_" + what)(self.h, int(mode), C.byref(out))
        if rc == capi.XCK_E_STATE:
            return None
        self._check(rc, "xck_get_" + what)
        return out

    def read_fate(self, mode=None):
        """Where the reads of one pipeline went since the last reset (xck_get_read_fate): dict of the counters in the struct's
        order, or None on a handle made without XCK_F_READ_FATE (and without XCK_READ_FATE=1 in the environment).  mode names the
        pipeline: the handle's own by default, XCK_MODE_BASEFC or XCK_MODE_BAF on a XCK_MODE_BOTH handle.  Waits for queued work."""
        rf = self._summary("read_fate", capi.ReadFate, mode)
        if rf is None:
            return None
        return {k: int(getattr(rf, k)) for k in capi.READ_FATE_FIELDS}

    def cell_summary(self, mode=None):
        """The per-cell table of one pipeline since the last reset (xck_get_cell_summary): dict of `fate`, int64 [(n_cells + 1), 12]
        (row n_cells: the reads without a listed cell), `matrix`, int64 [n_cells, k] (None before finish()), and the column names
        `fate_cols`, `matrix_cols` - copies, not views; or None on a handle made without XCK_F_CELL_SUMMARY (and without
        XCK_CELL_SUMMARY=1 in the environment).  mode as for read_fate().  Waits for queued work."""
        cs = self._summary("cell_summary", capi.CellSummary, mode)
        if cs is None:
            return None
        n, k, km = int(cs.n_cells), int(cs.n_fate_cols), int(cs.n_matrix_cols)
        fate = np.ctypeslib.as_array(cs.fate, shape=((n + 1) * k,)).reshape(n + 1, k).copy()
        matrix = np.ctypeslib.as_array(cs.matrix, shape=(n * km,)).reshape(n, km).copy() if cs.has_matrix and cs.matrix else None
        return dict(fate=fate, matrix=matrix, fate_cols=capi.CELL_FATE_COLS, matrix_cols=capi.CELL_MATRIX_COLS[int(cs.mode)])

    def feature_summary(self, mode=None):
        """The per-feature and per-SNP tables of one pipeline since the last reset (xck_get_feature_summary), all in the input order
        of the regions / SNPs the engine was made with: dict of `reads`, int64 [n_regions, 3] (basefc; None for the BAF pipeline),
        `matrix`, int64 [n_regions, k] (None before finish()), `snp`, int64 [n_snps, 8] (BAF; None for basefc; the tallies and
        `kept` are zero before finish()), `has_matrix`, and the column names `read_cols`, `matrix_cols`, `snp_cols` - copies, not
        views; or None on a handle made without XCK_F_FEATURE_SUMMARY (and without XCK_FEATURE_SUMMARY=1 in the environment).
        mode as for read_fate().  Waits for queued work."""
        fs = self._summary("feature_summary", capi.FeatureSummary, mode)
        if fs is None:
            return None

        def table(p, rows, cols):
            if not p:
                return None
            return np.ctypeslib.as_array(p, shape=(rows * cols,)).reshape(rows, cols).copy() if rows * cols else np.zeros((rows, cols), dtype=np.int64)
        n = int(fs.n_regions)
        return dict(reads=table(fs.reads, n, int(fs.n_read_cols)),
                    matrix=table(fs.matrix, n, int(fs.n_matrix_cols)) if fs.has_matrix else None,
                    snp=table(fs.snp, int(fs.n_snps), int(fs.n_snp_cols)), has_matrix=bool(fs.has_matrix),
                    read_cols=capi.FEATURE_READ_COLS, matrix_cols=capi.FEATURE_MATRIX_COLS[int(fs.mode)], snp_cols=capi.SNP_COLS)

    def baseq_stats(self):
        """What the base-quality floor saw since the last reset (xck_get_baseq_stats): dict of min_baseq, pairs_with_base (the (read,
        SNP) pairs of the pileup in which the read stores a base), pairs_masked; None on a handle without a floor."""
        out = capi.BaseqStats()
        out.struct_size = C.sizeof(capi.BaseqStats)
        rc = self.lib.xck_get_baseq_stats(self.h, C.byref(out))
        if rc == capi.XCK_E_STATE:
            return None
        self._check(rc, "xck_get_baseq_stats")
        return dict(min_baseq=int(out.min_baseq), pairs_with_base=int(out.pairs_with_base), pairs_masked=int(out.pairs_masked))

    def base_tally(self, contig, start, n):
        """The A, C, G, T counters of positions [start, start + n) (0-based) of one contig (xck_get_base_tally; contig: index or name)
        -> uint32 [n, 4].  Waits for queued work; a contig no read touched reads as zeros."""
        c = self.contig_names.index(contig) if isinstance(contig, str) else int(contig)
        out = np.zeros((max(int(n), 0), 4), dtype=np.uint32)
        self._check(self.lib.xck_get_base_tally(self.h, c, int(start), int(n), capi.np_ptr(out, C.c_uint32)), "xck_get_base_tally")
        return out

    def base_tally_stats(self):
        """What the base tally pass saw since the last reset (xck_get_base_tally_stats): dict of reads_tallied, bases_tallied,
        bases_other, bases_masked, bases_out_of_range; None on a handle made without base_tally."""
        out = capi.BaseTallyStats()
        out.struct_size = C.sizeof(capi.BaseTallyStats)
        rc = self.lib.xck_get_base_tally_stats(self.h, C.byref(out))
        if rc == capi.XCK_E_STATE:
            return None
        self._check(rc, "xck_get_base_tally_stats")
        return {k: int(getattr(out, k)) for k in capi.BASE_TALLY_FIELDS}

    def tally_contigs(self):
        """indices of the contigs whose tally table exists, i.e. that a batch has reached (xck_get_base_tally_contigs)"""
        has = np.zeros(len(self.contig_names), dtype=np.uint8)
        self._check(self.lib.xck_get_base_tally_contigs(self.h, capi.np_ptr(has, C.c_uint8), len(has)), "xck_get_base_tally_contigs")
        return np.flatnonzero(has).tolist()

    def set_reference(self, fasta_fn, names=None):
        """The genome's sequence of a base_tally handle from a FASTA file (utils/fasta.py: mapped, indexed by <fasta>.fai or by one
        scan; xck_set_contig_ref packs the text on the device, 0.5 byte a position).  FASTA names are matched to the handle's contigs
        with the chr tolerance of the BAM mapping.  names: the contigs to load; None: after pushes the contigs that have a table,
        before them all.  ValueError when a matched contig's length differs from the handle's contig_len (another genome build), for a
        compressed file and without contig lengths.  -> dict(loaded=[contig names], missing=[asked-for contigs the FASTA lacks]);
        find_candidates() then orients by the reference, and a contig without a sequence counts as unknown."""
        from .utils.fasta import Fasta, match_contigs
        if self.contig_len is None:
            raise ValueError("set_reference needs the contigs' lengths (contig_len, set_contig_lengths() or an ingest) first")
        if names is not None:
            want = [self.contig_names.index(x) for x in names]
        else:
            want = self.tally_contigs() or None
        with Fasta(fasta_fn) as fa:
            pairs, missing = match_contigs(fa.entries, self.contig_names, self.contig_len, want)
            for c, e in pairs:
                addr, n_raw, lb, lw = fa.span(e)
                self._check(self.lib.xck_set_contig_ref(self.h, c, C.c_void_p(addr), n_raw, lb, lw), "xck_set_contig_ref")
        loaded = [self.contig_names[c] for c, _ in pairs]
        self.ref_loaded = self.ref_loaded or bool(loaded)
        info("[engine] reference %s: %d contig(s) loaded%s" % (fasta_fn, len(loaded), (", not in the FASTA: " + ", ".join(missing)) if missing else ""))
        return dict(loaded=loaded, missing=missing)

    def contig_ref(self, contig, start, n):
        """The letters of positions [start, start + n) (0-based) of a contig's packed sequence (xck_get_contig_ref) -> str"""
        c = self.contig_names.index(contig) if isinstance(contig, str) else int(contig)
        out = C.create_string_buffer(max(int(n), 0) + 1)
        self._check(self.lib.xck_get_contig_ref(self.h, c, int(start), int(n), out), "xck_get_contig_ref")
        return out.raw[:max(int(n), 0)].decode()

    def find_candidates(self, min_count=20, min_maf=0.1, use_ref=None):
        """The candidate SNP positions of the tallies (xck_find_candidates), in (contig, pos) order: dict of contig (int32 index),
        pos (int32, 1-based), ref, alt (str arrays of one letter), count (uint32 [n, 4]: A C G T), positions_covered - copies.
        ref is the base with the largest count, alt the largest of the others (ties: the earliest of A, C, G, T); a position is a
        candidate when alt > 0, not (n < min_count) and not (alt < n * min_maf).  Valid between finish() and reset().
        use_ref (None: when set_reference() has loaded a sequence): xck_find_candidates_ref - ref is the genome's base, alt the
        largest of the others, the smaller of the two counts takes the place of the alt count, positions whose genome base is not
        A C G T are left out - and the dict carries ref_stats: ref_major, ref_minor (written; ref is / is not the base the plain
        rule makes ref), ref_unsupported, ref_unknown (candidates of the plain rule that are not written)."""
        cfg = capi.CandidateConfig()
        cfg.struct_size = C.sizeof(capi.CandidateConfig)
        cfg.min_count, cfg.min_maf = float(min_count), float(min_maf)
        out = capi.Candidates()
        ref_stats = None
        if self.ref_loaded if use_ref is None else use_ref:
            st = capi.CandidateRefStats()
            st.struct_size = C.sizeof(capi.CandidateRefStats)
            self._check(self.lib.xck_find_candidates_ref(self.h, C.byref(cfg), C.byref(out), C.byref(st)), "xck_find_candidates_ref")
            ref_stats = {k: int(getattr(st, k)) for k in capi.CANDIDATE_REF_FIELDS}
        else:
            self._check(self.lib.xck_find_candidates(self.h, C.byref(cfg), C.byref(out)), "xck_find_candidates")
        n = int(out.n)
        take = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(k,)).astype(dt, copy=True) if k else np.zeros(0, dtype=dt)
        letters = lambda p: np.frombuffer(C.string_at(p, n), dtype="S1").astype("U1") if n else np.zeros(0, dtype="U1")
        res = dict(contig=take(out.contig, n, np.int32), pos=take(out.pos, n, np.int32), ref=letters(out.ref), alt=letters(out.alt),
                   count=take(out.count, 4 * n, np.uint32).reshape(n, 4), positions_covered=int(out.positions_covered))
        if ref_stats is not None:
            res["ref_stats"] = ref_stats
        return res

    def molecule_stats(self):
        """How the reads of the molecules of the last finish() agree (xck_get_molecule_stats): dict of molecules, multi_read,
        discordant, tied, changed in the struct's order, or None where the handle has nothing to say - made without umi_consensus /
        XCK_F_UMI_CONSENSUS (and without XCK_UMI_CONSENSUS=1 in the environment), before finish() or after reset().  refold(),
        snp_counts() and group_counts() do not change the counters."""
        out = capi.MoleculeStats()
        out.struct_size = C.sizeof(capi.MoleculeStats)
        rc = self.lib.xck_get_molecule_stats(self.h, C.byref(out))
        if rc == capi.XCK_E_STATE:
            return None
        self._check(rc, "xck_get_molecule_stats")
        return {k: int(getattr(out, k)) for k in capi.MOLECULE_FIELDS}

    def umi_feature_stats(self):
        """What the unique-feature rule of the last finish() saw (xck_get_umi_feature_stats): dict of molecules, multi_feature, keys,
        keys_dropped in the struct's order (keys - keys_dropped = the sum of the count matrix), or None where the handle has nothing
        to say - made without umi_feature="unique" / XCK_F_UNIQUE_FEATURE (and without XCK_UMI_FEATURE=unique in the environment),
        before finish() or after reset()."""
        out = capi.UmiFeatureStats()
        out.struct_size = C.sizeof(capi.UmiFeatureStats)
        rc = self.lib.xck_get_umi_feature_stats(self.h, C.byref(out))
        if rc == capi.XCK_E_STATE:
            return None
        self._check(rc, "xck_get_umi_feature_stats")
        return {k: int(getattr(out, k)) for k in capi.UMI_FEATURE_FIELDS}

    def umi_dedup_stats(self):
        """What the 1-mismatch UMI collapsing of the last finish() saw (xck_get_umi_dedup_stats): dict of keys, molecules, groups,
        groups_changed, opaque_keys, max_group in the struct's order (molecules = the sum of the count matrix, groups = its non-zeros),
        or None where the handle has nothing to say - made without umi_dedup="1mm_all" / XCK_F_UMI_COLLAPSE (and without
        XCK_UMI_DEDUP=1mm_all in the environment), before finish() or after reset()."""
        out = capi.UmiDedupStats()
        out.struct_size = C.sizeof(capi.UmiDedupStats)
        rc = self.lib.xck_get_umi_dedup_stats(self.h, C.byref(out))
        if rc == capi.XCK_E_STATE:
            return None
        self._check(rc, "xck_get_umi_dedup_stats")
        return {k: int(getattr(out, k)) for k in capi.UMI_DEDUP_FIELDS}


class BamStream(object):
    """One open BAM being streamed through an Engine in slices (xck_ingest_opts.pause_records)."""

    def __init__(self, eng, path, sample=0, n_threads=0, contig_mask=None, use_index=False, windows=None):
        self.eng = eng
        self.b, refs = eng._open(path, n_threads or eng.cfg.n_threads)
        eng._lengths_from_bam(self.b, refs)
        self.opts, self._keep = eng._opts(refs, sample, 0, contig_mask, use_index, windows)
        self.n_records = 0
        self.done = False

    def advance(self, n_records=0):
        """Decode and join at least n_records further records (0 = the rest of the file)."""
        if self.done:
            return self.n_records, True
        self.opts.pause_records = int(n_records)
        n = C.c_int64(0)
        rc = self.eng.lib.xck_ingest_bam(self.eng.h, self.b, C.byref(self.opts), C.byref(n))
        if rc < 0:
            self.eng._check(rc, "xck_ingest_bam")
        self.n_records = int(n.value)
        self.done = rc == 0
        return self.n_records, self.done

    def close(self):
        if self.b:
            self.eng.lib.xck_bam_close(self.b)
            self.b = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
