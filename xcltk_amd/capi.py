"""capi.py - ctypes mirror of include/xck.h and loader of libxck.so (the HIP engine).

There is no fallback: if the shared library is missing or cannot be loaded, every product
entry point raises.  (The CPU oracle under oracle/ is test infrastructure and is never
imported from here.)
"""

import ctypes as C
import os

import numpy as np

XCK_MODE_BASEFC = 1
XCK_MODE_BAF = 2
XCK_MODE_BOTH = 3
XCK_UMI_NONE = 0xFFFFFFFFFFFFFFFF
XCK_CELL_FILTERED = -2                 # cell of a record the handle's tag filter rejected; to the kernels the same as -1
XCK_F_FORCE_KEY128 = 1
XCK_F_VERIFY_CRC = 2
XCK_F_DECODE_ONLY = 4
XCK_F_LOW_PRIORITY = 8
XCK_F_DEVICE_CRC = 16
XCK_F_READ_FATE = 32
XCK_F_CELL_SUMMARY = 64
XCK_F_FEATURE_SUMMARY = 128
XCK_F_UMI_CONSENSUS = 256
XCK_F_MIN_BASEQ = 512
XCK_F_UNIQUE_FEATURE = 1024
XCK_F_UMI_COLLAPSE = 2048
XCK_F_BASE_TALLY = 4096
XCK_E_ARG, XCK_E_DEVICE, XCK_E_NOMEM, XCK_E_IO, XCK_E_STATE, XCK_E_CAPACITY = -1, -2, -3, -4, -5, -6

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libxck.so")


class Region(C.Structure):
    _fields_ = [("contig", C.c_int32), ("start", C.c_int32), ("end", C.c_int32)]


class Snp(C.Structure):
    _fields_ = [("contig", C.c_int32), ("pos", C.c_int32),
                ("ref", C.c_uint8), ("alt", C.c_uint8),
                ("ref_hap", C.c_uint8), ("alt_hap", C.c_uint8)]


REGION_DTYPE = np.dtype([("contig", "<i4"), ("start", "<i4"), ("end", "<i4")])
SNP_DTYPE = np.dtype([("contig", "<i4"), ("pos", "<i4"), ("ref", "u1"), ("alt", "u1"),
                      ("ref_hap", "u1"), ("alt_hap", "u1")])
assert REGION_DTYPE.itemsize == C.sizeof(Region) and SNP_DTYPE.itemsize == C.sizeof(Snp)


class Config(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("mode", C.c_int32), ("device", C.c_int32),
        ("min_mapq", C.c_double), ("min_len", C.c_int32),
        ("incl_flag", C.c_uint32), ("excl_flag", C.c_uint32), ("no_orphan", C.c_int32),
        ("min_include", C.c_double),
        ("min_count", C.c_double), ("min_maf", C.c_double), ("no_dup_hap", C.c_int32),
        ("n_cells", C.c_int32), ("n_contigs", C.c_int32),
        ("n_regions", C.c_int32), ("regions", C.POINTER(Region)),
        ("n_snps", C.c_int32), ("snps", C.POINTER(Snp)),
        ("barcodes", C.POINTER(C.c_char_p)),
        ("cell_tag", C.c_char * 4), ("umi_tag", C.c_char * 4),
        ("max_batch_reads", C.c_int64), ("n_threads", C.c_int32), ("flags", C.c_int32),
        ("n_excl_pairs", C.c_int32), ("excl_region", C.POINTER(C.c_int32)), ("excl_snp", C.POINTER(C.c_int32)),
        ("filter_tag", C.c_char * 4), ("filter_mask", C.c_uint32), ("filter_value", C.c_uint32),
    ]
    # xck_config.min_baseq lies in the four bytes behind filter_value that were the struct's tail padding (the size did not change); the
    # library reads them only when flags holds XCK_F_MIN_BASEQ.  Set through Config.min_baseq, which sets or clears the bit with it.
    MIN_BASEQ_OFFSET = 172

    @property
    def min_baseq(self):
        return C.c_int32.from_buffer(self, Config.MIN_BASEQ_OFFSET).value

    @min_baseq.setter
    def min_baseq(self, q):
        C.c_int32.from_buffer(self, Config.MIN_BASEQ_OFFSET).value = int(q)
        self.flags = (self.flags | XCK_F_MIN_BASEQ) if int(q) else (self.flags & ~XCK_F_MIN_BASEQ)


MIN_BASEQ_MAX = 93


class RefoldConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("n_regions", C.c_int32), ("regions", C.POINTER(Region)),
        ("n_snps", C.c_int32), ("snps", C.POINTER(Snp)), ("snp_enabled", C.POINTER(C.c_uint8)),
        ("min_count", C.c_double), ("min_maf", C.c_double), ("no_dup_hap", C.c_int32),
        ("n_excl_pairs", C.c_int32), ("excl_region", C.POINTER(C.c_int32)), ("excl_snp", C.POINTER(C.c_int32)),
        ("cell_enabled", C.POINTER(C.c_uint8)),          # appended: a struct_size that ends in front of it is still accepted
    ]


XCK_GROUP_SRC_RESULT, XCK_GROUP_SRC_SNP = 0, 1
XCK_GROUP_MAX = 4096


class GroupConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("source", C.c_int32), ("n_groups", C.c_int32), ("cell_group", C.POINTER(C.c_int32))]


class Batch(C.Structure):
    _fields_ = [
        ("contig", C.c_int32), ("n_reads", C.c_int32), ("ordinal_base", C.c_uint64),
        ("pos", C.POINTER(C.c_int32)), ("flag", C.POINTER(C.c_uint16)),
        ("mapq", C.POINTER(C.c_uint8)), ("cell", C.POINTER(C.c_int32)),
        ("umi", C.POINTER(C.c_uint64)), ("cig_off", C.POINTER(C.c_uint32)),
        ("cigar", C.POINTER(C.c_uint32)), ("seq_off", C.POINTER(C.c_uint32)),
        ("seq", C.POINTER(C.c_uint8)),
    ]


class Coo(C.Structure):
    _fields_ = [("nnz", C.c_int64), ("row", C.POINTER(C.c_int32)),
                ("col", C.POINTER(C.c_int32)), ("val", C.POINTER(C.c_int32))]

    def to_numpy(self, copy=True):
        """(row, col, val) int32 arrays; copy=False returns views of the engine-owned pinned
        buffers (valid until the next finish / reset / destroy of that engine)."""
        n = int(self.nnz)
        if n == 0:
            z = np.zeros(0, dtype=np.int32)
            return z, z.copy(), z.copy()
        out = tuple(np.ctypeslib.as_array(p, shape=(n,)) for p in (self.row, self.col, self.val))
        return tuple(a.copy() for a in out) if copy else out


class Result(C.Structure):
    _fields_ = [("count", Coo), ("ad", Coo), ("dp", Coo), ("oth", Coo)]


class Stats(C.Structure):
    _fields_ = [("n_batches", C.c_int64), ("n_reads", C.c_int64), ("n_hits", C.c_int64),
                ("n_hits_unique", C.c_int64), ("ms_h2d", C.c_double), ("ms_device", C.c_double),
                ("ms_join", C.c_double), ("ms_sort", C.c_double), ("ms_d2h", C.c_double),
                ("algo_bytes_join", C.c_int64), ("n_join_launches", C.c_int64), ("key_bits", C.c_int32), ("umi_bits", C.c_int32),
                ("fold_path", C.c_int32), ("fold_fallbacks", C.c_int32), ("pileup_sort_path", C.c_int32), ("fold_refinements", C.c_int32),
                ("pileup_sort2_path", C.c_int32), ("gpu_inflate_chunks", C.c_int32)]


class DecodeStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
                ("gpu_inflate_chunks", C.c_int64), ("gpu_inflate_blocks", C.c_int64), ("gpu_blocks_left_to_host", C.c_int64),
                ("crc_blocks_device", C.c_int64), ("crc_blocks_host", C.c_int64), ("crc_mismatch_device", C.c_int64),
                ("crc_device_host_disagree", C.c_int64), ("gpu_path_given_up", C.c_int64),
                ("gpu_parse_chunks", C.c_int64), ("gpu_parse_fallbacks", C.c_int64),
                ("gpu_names_interned", C.c_int64), ("gpu_names_distinct", C.c_int64), ("gpu_names_host_chunks", C.c_int64),
                ("tag_filtered", C.c_int64)]


class ReadFate(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32)] + [(k, C.c_int64) for k in (
        "n_reads", "not_joined", "low_mapq", "excl_flag", "incl_flag", "orphan", "no_cell", "no_umi", "short_aligned",
        "no_target", "include_fail", "assigned", "multi", "pairs")]


# the counters of xck_read_fate in the struct's order: n_reads, the classes that sum to it (READ_FATE_CLASSES), multi, pairs
READ_FATE_FIELDS = tuple(k for k, _ in ReadFate._fields_[2:])
READ_FATE_CLASSES = READ_FATE_FIELDS[1:-2]


class CellSummary(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("n_cells", C.c_int32), ("n_fate_cols", C.c_int32),
                ("fate", C.POINTER(C.c_int64)), ("has_matrix", C.c_int32), ("n_matrix_cols", C.c_int32),
                ("matrix", C.POINTER(C.c_int64))]


# the columns of xck_cell_summary.fate (the fields of xck_read_fate from low_mapq to pairs) and of .matrix per pipeline
CELL_FATE_COLS = READ_FATE_FIELDS[2:]
CELL_MATRIX_COLS = {XCK_MODE_BASEFC: ("umis", "features"), XCK_MODE_BAF: ("ad", "dp", "oth", "features")}


class FeatureSummary(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("n_regions", C.c_int32), ("n_read_cols", C.c_int32),
                ("reads", C.POINTER(C.c_int64)), ("has_matrix", C.c_int32), ("n_matrix_cols", C.c_int32),
                ("matrix", C.POINTER(C.c_int64)), ("n_snps", C.c_int32), ("n_snp_cols", C.c_int32), ("snp", C.POINTER(C.c_int64))]


# the columns of xck_feature_summary.reads (basefc), of .matrix per pipeline and of .snp (BAF)
FEATURE_READ_COLS = ("include_fail", "pairs", "shared")
FEATURE_MATRIX_COLS = {XCK_MODE_BASEFC: ("umis", "cells"), XCK_MODE_BAF: ("snps", "snps_kept", "ad", "dp", "oth", "cells")}
SNP_COLS = ("reads", "a", "c", "g", "t", "n", "kept", "regions")


class MoleculeStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("consensus", C.c_int32)] + [(k, C.c_int64) for k in (
        "molecules", "multi_read", "discordant", "tied", "changed")]


class BaseqStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_baseq", C.c_int32), ("pairs_with_base", C.c_int64), ("pairs_masked", C.c_int64)]


# the counters of xck_molecule_stats in the struct's order
MOLECULE_FIELDS = tuple(k for k, _ in MoleculeStats._fields_[2:])


class UmiFeatureStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(k, C.c_int64) for k in (
        "molecules", "multi_feature", "keys", "keys_dropped")]


# the counters of xck_umi_feature_stats in the struct's order
UMI_FEATURE_FIELDS = tuple(k for k, _ in UmiFeatureStats._fields_[2:])


class UmiDedupStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(k, C.c_int64) for k in (
        "keys", "molecules", "groups", "groups_changed", "opaque_keys", "max_group")]


# the counters of xck_umi_dedup_stats in the struct's order
UMI_DEDUP_FIELDS = tuple(k for k, _ in UmiDedupStats._fields_[2:])


class BaseTallyStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(k, C.c_int64) for k in (
        "reads_tallied", "bases_tallied", "bases_other", "bases_masked", "bases_out_of_range")]


# the counters of xck_base_tally_stats in the struct's order
BASE_TALLY_FIELDS = tuple(k for k, _ in BaseTallyStats._fields_[2:])


class CandidateConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("min_count", C.c_double), ("min_maf", C.c_double)]


class Candidates(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("pos", C.POINTER(C.c_int32)), ("ref", C.POINTER(C.c_char)),
                ("alt", C.POINTER(C.c_char)), ("count", C.POINTER(C.c_uint32)), ("positions_covered", C.c_int64)]


class CandidateRefStats(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] + [(k, C.c_int64) for k in (
        "ref_major", "ref_minor", "ref_unsupported", "ref_unknown")]


# the counters of xck_candidate_ref_stats in the struct's order
CANDIDATE_REF_FIELDS = tuple(k for k, _ in CandidateRefStats._fields_[2:])


class IngestOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sample", C.c_int32),
                ("tid_to_contig", C.POINTER(C.c_int32)), ("use_index", C.c_int32),
                ("max_records", C.c_int64), ("pause_records", C.c_int64),
                ("tid_beg", C.POINTER(C.c_int32)), ("tid_end", C.POINTER(C.c_int32))]


class PhaseProblem(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_cells", C.c_int32), ("n_cols", C.c_int32),
                ("col_ptr", C.POINTER(C.c_int64)), ("cell", C.POINTER(C.c_int32)), ("ad", C.POINTER(C.c_int32)), ("dp", C.POINTER(C.c_int32)),
                ("cell_enabled", C.POINTER(C.c_uint8)), ("n_snps", C.c_int32), ("n_regions", C.c_int32),
                ("ref_hap", C.POINTER(C.c_int8)), ("alt_hap", C.POINTER(C.c_int8)), ("reg_ptr", C.POINTER(C.c_int64)),
                ("slot_col", C.POINTER(C.c_int32)), ("slot_snp", C.POINTER(C.c_int32)), ("slot_pos", C.POINTER(C.c_int64))]


class PhaseResult(C.Structure):
    _fields_ = [("n_slots", C.c_int64), ("kept", C.POINTER(C.c_uint8)), ("flip", C.POINTER(C.c_uint8)),
                ("n_regions", C.c_int32), ("n_snps", C.c_int32), ("status", C.POINTER(C.c_uint8)),
                ("ref_hap", C.POINTER(C.c_int8)), ("alt_hap", C.POINTER(C.c_int8)), ("n_levels", C.c_int32), ("n_blocks", C.c_int32),
                ("ms_prepare", C.c_double), ("ms_h2d", C.c_double), ("ms_kernel", C.c_double), ("ms_d2h", C.c_double)]


XCK_PHASE_FAILED, XCK_PHASE_PHASED = 0, 1


# every symbol include/xck.h declares: (name, restype, argtypes)
_P = C.POINTER
class SnpText(C.Structure):
    _fields_ = [("n", C.c_int64), ("chrom_id", _P(C.c_int32)), ("pos", _P(C.c_int64)), ("ref", _P(C.c_char)), ("alt", _P(C.c_char)),
                ("ref_hap", _P(C.c_int8)), ("alt_hap", _P(C.c_int8)), ("n_chroms", C.c_int32), ("chroms", _P(C.c_char_p)),
                ("n_rejected", C.c_int64), ("rej_line", _P(C.c_int64)), ("rej_code", _P(C.c_int8))]


SYMBOLS = [
    ("xck_version", C.c_char_p, []),
    ("xck_abi_version", C.c_int, []),
    ("xck_device_count", C.c_int, []),
    ("xck_last_error", C.c_char_p, [C.c_void_p]),
    ("xck_create", C.c_int, [_P(Config), _P(C.c_void_p)]),
    ("xck_destroy", None, [C.c_void_p]),
    ("xck_umi_bits", C.c_int, [C.c_void_p]),
    ("xck_push_batch", C.c_int, [C.c_void_p, _P(Batch)]),
    ("xck_push_batch_device", C.c_int, [C.c_void_p, _P(Batch)]),
    ("xck_push_batch_q", C.c_int, [C.c_void_p, _P(Batch), _P(C.c_uint8)]),
    ("xck_flush", C.c_int, [C.c_void_p]),
    ("xck_finish", C.c_int, [C.c_void_p, _P(Result)]),
    ("xck_finish_async", C.c_int, [C.c_void_p]),
    ("xck_get_result_device", C.c_int, [C.c_void_p, _P(Result)]),
    ("xck_refold", C.c_int, [C.c_void_p, _P(RefoldConfig), _P(Result)]),
    ("xck_snp_counts", C.c_int, [C.c_void_p, _P(Result)]),
    ("xck_group_counts", C.c_int, [C.c_void_p, _P(GroupConfig), _P(Result)]),
    ("xck_reset", C.c_int, [C.c_void_p]),
    ("xck_get_stats", C.c_int, [C.c_void_p, _P(Stats)]),
    ("xck_get_decode_stats", C.c_int, [C.c_void_p, _P(DecodeStats)]),
    ("xck_get_read_fate", C.c_int, [C.c_void_p, C.c_int, _P(ReadFate)]),
    ("xck_get_cell_summary", C.c_int, [C.c_void_p, C.c_int, _P(CellSummary)]),
    ("xck_get_feature_summary", C.c_int, [C.c_void_p, C.c_int, _P(FeatureSummary)]),
    ("xck_get_molecule_stats", C.c_int, [C.c_void_p, _P(MoleculeStats)]),
    ("xck_get_baseq_stats", C.c_int, [C.c_void_p, _P(BaseqStats)]),
    ("xck_get_umi_feature_stats", C.c_int, [C.c_void_p, _P(UmiFeatureStats)]),
    ("xck_get_umi_dedup_stats", C.c_int, [C.c_void_p, _P(UmiDedupStats)]),
    ("xck_set_contig_lengths", C.c_int, [C.c_void_p, _P(C.c_int64), C.c_int32]),
    ("xck_get_base_tally", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, _P(C.c_uint32)]),
    ("xck_get_base_tally_stats", C.c_int, [C.c_void_p, _P(BaseTallyStats)]),
    ("xck_find_candidates", C.c_int, [C.c_void_p, _P(CandidateConfig), _P(Candidates)]),
    ("xck_set_contig_ref", C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32]),
    ("xck_get_contig_ref", C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_char_p]),
    ("xck_get_base_tally_contigs", C.c_int, [C.c_void_p, _P(C.c_uint8), C.c_int32]),
    ("xck_find_candidates_ref", C.c_int, [C.c_void_p, _P(CandidateConfig), _P(Candidates), _P(CandidateRefStats)]),
    ("xck_bam_open", C.c_int, [C.c_char_p, C.c_int, _P(C.c_void_p), C.c_char_p, C.c_size_t]),
    ("xck_bam_close", None, [C.c_void_p]),
    ("xck_bam_n_refs", C.c_int, [C.c_void_p]),
    ("xck_bam_ref_name", C.c_char_p, [C.c_void_p, C.c_int]),
    ("xck_bam_ref_len", C.c_int64, [C.c_void_p, C.c_int]),
    ("xck_bam_ref_records", C.c_int, [C.c_void_p, C.c_int, _P(C.c_int64), _P(C.c_int64)]),
    ("xck_bam_linear_index", C.c_int, [C.c_void_p, C.c_int, _P(C.c_int64), _P(_P(C.c_uint64))]),
    ("xck_ingest_bam", C.c_int, [C.c_void_p, C.c_void_p, _P(IngestOpts), _P(C.c_int64)]),
    ("xck_bam_prefetch", C.c_int, [C.c_void_p, C.c_void_p, _P(IngestOpts)]),
    ("xck_bam_next_batch", C.c_int, [C.c_void_p, C.c_void_p, _P(IngestOpts), _P(Batch)]),
    ("xck_write_mtx", C.c_int, [C.c_char_p, _P(Coo), _P(C.c_int32), C.c_int32, C.c_int32]),
    ("xck_mtx_part_size", C.c_int, [_P(Coo), _P(C.c_int32), _P(C.c_int64), _P(C.c_int64)]),
    ("xck_write_mtx_part", C.c_int, [C.c_char_p, C.c_int64, _P(Coo), _P(C.c_int32)]),
    ("xck_parse_snp_text", C.c_int, [C.c_char_p, C.c_int, _P(_P(SnpText))]),
    ("xck_free_snp_text", None, [_P(SnpText)]),
    ("xck_local_phase", C.c_int, [_P(PhaseProblem), _P(_P(PhaseResult))]),
    ("xck_free_phase_result", None, [_P(PhaseResult)]),
]

_lib = None


class XckLibraryError(RuntimeError):
    pass


def _preload_torch_hip():
    """PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64.so.1 (same sonames as /opt/rocm).
    Two HIP runtimes cannot share a process: whichever is loaded first serves both libxck.so and torch.
    If libxck.so pulled in the system runtime first, a later `import torch` finds "no ROCm-capable device".
    So when torch is installed, load ITS runtime before libxck.so (no `import torch` needed); the dynamic
    linker then binds libxck.so to the already loaded sonames."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.origin:
        return
    p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.isfile(p):
        try:
            C.CDLL(p, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load(path=None):
    """Load libxck.so (built by `make -C xcltk_amd/csrc` or __graft_entry__.build())."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    _preload_torch_hip()
    p = path or os.environ.get("XCK_LIB", LIB_PATH)
    if not os.path.isfile(p):
        raise XckLibraryError(
            "HIP engine library not found at %s - build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C xcltk_amd/csrc`. "
            "There is no CPU fallback." % p)
    try:
        lib = C.CDLL(p)
    except OSError as e:
        raise XckLibraryError("cannot load %s: %s (no CPU fallback)" % (p, e))
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.xck_abi_version() != 3:
        raise XckLibraryError("ABI mismatch")
    if path is None:
        _lib = lib
    return lib


def bam_references(path):
    """[(name, length)] of a BAM header, read by the engine's own decoder (xck_bam_open; no device needed)."""
    lib = load()
    b = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = lib.xck_bam_open(path.encode(), 1, C.byref(b), err, 512)
    if rc != 0:
        raise XckLibraryError("xck_bam_open failed (%d): %s" % (rc, err.value.decode()))
    try:
        return [(lib.xck_bam_ref_name(b, i).decode(), int(lib.xck_bam_ref_len(b, i))) for i in range(lib.xck_bam_n_refs(b))]
    finally:
        lib.xck_bam_close(b)


def np_ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def make_batch(contig, ordinal_base, pos, flag, mapq, cell, umi, cig_off, cigar,
               seq_off=None, seq=None):
    """Build a Batch struct over numpy arrays (kept alive by the returned holder tuple)."""
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    flag = np.ascontiguousarray(flag, dtype=np.uint16)
    mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
    cell = np.ascontiguousarray(cell, dtype=np.int32)
    umi = np.ascontiguousarray(umi, dtype=np.uint64)
    cig_off = np.ascontiguousarray(cig_off, dtype=np.uint32)
    cigar = np.ascontiguousarray(cigar, dtype=np.uint32)
    n = len(pos)
    assert len(flag) == n and len(mapq) == n and len(cell) == n and len(umi) == n
    assert len(cig_off) == n + 1 and (n == 0 or int(cig_off[-1]) <= len(cigar))
    b = Batch()
    b.contig = contig
    b.n_reads = n
    b.ordinal_base = ordinal_base
    b.pos = np_ptr(pos, C.c_int32)
    b.flag = np_ptr(flag, C.c_uint16)
    b.mapq = np_ptr(mapq, C.c_uint8)
    b.cell = np_ptr(cell, C.c_int32)
    b.umi = np_ptr(umi, C.c_uint64)
    b.cig_off = np_ptr(cig_off, C.c_uint32)
    b.cigar = np_ptr(cigar, C.c_uint32)
    keep = [pos, flag, mapq, cell, umi, cig_off, cigar]
    if seq_off is not None:
        seq_off = np.ascontiguousarray(seq_off, dtype=np.uint32)
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        assert len(seq_off) == n + 1 and (n == 0 or int(seq_off[-1]) <= len(seq))
        b.seq_off = np_ptr(seq_off, C.c_uint32)
        b.seq = np_ptr(seq, C.c_uint8)
        keep += [seq_off, seq]
    return b, keep


def local_phase(n_cells, col_ptr, cell, ad, dp, ref_hap, alt_hap, reg_ptr, slot_col, slot_snp, slot_pos, cell_enabled=None, device=0,
                struct_size=None):
    """xck_local_phase over numpy arrays (include/xck.h): -> dict(kept, flip: uint8 per slot; status: uint8 per region; ref_hap,
    alt_hap: int8 per SNP; n_levels, n_blocks, ms: dict of the stage times).  Raises engine.XckError with the library's code and text."""
    from .engine import XckError
    lib = load()
    arr = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    col_ptr, reg_ptr, slot_pos = arr(col_ptr, np.int64), arr(reg_ptr, np.int64), arr(slot_pos, np.int64)
    cell, ad, dp = arr(cell, np.int32), arr(ad, np.int32), arr(dp, np.int32)
    slot_col, slot_snp = arr(slot_col, np.int32), arr(slot_snp, np.int32)
    ref_hap, alt_hap = arr(ref_hap, np.int8), arr(alt_hap, np.int8)
    if len(col_ptr) < 1 or len(reg_ptr) < 1:
        raise ValueError("col_ptr / reg_ptr need at least one element")
    if not (len(cell) == len(ad) == len(dp)) or len(ref_hap) != len(alt_hap) or not (len(slot_col) == len(slot_snp) == len(slot_pos)):
        raise ValueError("parallel arrays differ in length")
    if (len(col_ptr) > 1 and int(col_ptr[-1]) > len(cell)) or (len(reg_ptr) > 1 and int(reg_ptr[-1]) > len(slot_col)):
        raise ValueError("a pointer array ends beyond its table")
    p = PhaseProblem()
    p.struct_size = C.sizeof(PhaseProblem) if struct_size is None else struct_size
    p.device, p.n_cells, p.n_cols = device, n_cells, len(col_ptr) - 1
    p.col_ptr, p.cell, p.ad, p.dp = np_ptr(col_ptr, C.c_int64), np_ptr(cell, C.c_int32), np_ptr(ad, C.c_int32), np_ptr(dp, C.c_int32)
    if cell_enabled is not None:
        cell_enabled = arr(cell_enabled, np.uint8)
        if len(cell_enabled) != n_cells:
            raise ValueError("cell_enabled needs one byte per cell")
        p.cell_enabled = np_ptr(cell_enabled, C.c_uint8)
    p.n_snps, p.n_regions = len(ref_hap), len(reg_ptr) - 1
    p.ref_hap, p.alt_hap = np_ptr(ref_hap, C.c_int8), np_ptr(alt_hap, C.c_int8)
    p.reg_ptr, p.slot_col, p.slot_snp, p.slot_pos = np_ptr(reg_ptr, C.c_int64), np_ptr(slot_col, C.c_int32), np_ptr(slot_snp, C.c_int32), np_ptr(slot_pos, C.c_int64)
    out = _P(PhaseResult)()
    rc = lib.xck_local_phase(C.byref(p), C.byref(out))
    if rc != 0:
        raise XckError("xck_local_phase failed (%d): %s" % (rc, (lib.xck_last_error(None) or b"").decode()), rc)
    try:
        r = out.contents
        take = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)
        return dict(kept=take(r.kept, int(r.n_slots), np.uint8), flip=take(r.flip, int(r.n_slots), np.uint8),
                    status=take(r.status, int(r.n_regions), np.uint8), ref_hap=take(r.ref_hap, int(r.n_snps), np.int8),
                    alt_hap=take(r.alt_hap, int(r.n_snps), np.int8), n_levels=int(r.n_levels), n_blocks=int(r.n_blocks),
                    ms=dict(prepare=r.ms_prepare, h2d=r.ms_h2d, kernel=r.ms_kernel, d2h=r.ms_d2h))
    finally:
        lib.xck_free_phase_result(out)
