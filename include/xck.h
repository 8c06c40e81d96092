/* xck.h - C-ABI of the MI355X-native cell x feature / cell x SNP counting engine (libxck.so).
 *
 * This is the drop-in boundary for the ONE hot path of hxj5/xcltk:
 *   - RDR `basefc`  : per-region UMI/read counting        (reference xcltk/rdr/fc/core.py:69-178)
 *   - BAF  pileup   : per-region allele-specific counting (reference xcltk/baf/fc/core.py:42-247)
 * The reference has no FFI; its seams are the Python functions fc_features()/fc_fet1()/plp_snp().
 * Each entry point below names the reference interface it replaces.  A reference-side binding
 * (ctypes) is shown in INTEGRATION.md.
 *
 * Conventions: plain C, plain pointers and sizes, no torch / HIP types.  Every call returns an
 * int status (0 = ok, <0 = error; xck_last_error() gives the text) unless stated otherwise.
 * One engine handle drives one GPU; calls on one handle must be serialised by the caller;
 * different handles may be used from different host threads.  No global state, no callbacks.
 * There is NO CPU fallback: if no HIP device is usable xck_create() fails.
 */
/* Environment.  A handle reads its knobs ONCE, at xck_create() (csrc/api.cpp Knobs::from_env): later changes of the
 * environment do not reach a live handle, and no push / finish call looks at the environment.  None of them changes a result.
 *   XCK_DEBUG_TIMING          (set)       stage timings and path decisions on stderr
 *   XCK_FOLD=sort                         basefc fold by radix sort instead of the partition fold (tests; xck_stats.fold_path says which ran)
 *   XCK_FOLD_C=<keys>                     page size of the partition folds (tests: small pages reach every path with small inputs)
 *   XCK_FOLD_LGG=<l>                      at most 2^l cell groups per row in the basefc fold (default 6, or one per cell up to 512 cells)
 *   XCK_FOLD_COPIES_LG=<l>                2^l copies of the level-1 counters / cursors (default 4)
 *   XCK_FOLD_BUCKET_BLOCKS, XCK_FOLD_OVERLAP=0|1, XCK_FOLD_OVERLAP_BLOCKS      grids of the work-item pass, its second stream
 *   XCK_FULL_SORT=1                       radix-sort fold over all key bits
 *   XCK_PILEUP_SORT=radix                 library radix sorts for both pileup stages (the fallback path, forced)
 *   XCK_PILEUP_HAP=sorted|values          region-level hits: sorted items + k_hap_class, or class in a value word instead of packed bits
 *   XCK_PILEUP_LGG=<l>                    at most 2^l cell groups per SNP in the pileup partitions (default 10)
 *   XCK_HIT_CAP0, XCK_HIT_SLACK           first capacity / head room of the hit accumulators (tests: reach the overflow-replay path)
 *   XCK_PUSH_STAGE=0|1, XCK_PUSH_STAGE_BYTES   xck_push_batch: packed one-copy form always / never / below this size (default 2 MB)
 *   XCK_GPU_INFLATE=auto|<percent>|0      share of the BGZF chunks that xck_ingest_bam inflates on the handle's GPU (csrc/inflate_dev.hip; the record
 *                                         walk and parse of these chunks: XCK_GPU_PARSE).  auto (the default): files of at least XCK_GPU_INFLATE_MIN_MB (96) compressed MB keep
 *                                         XCK_GPU_INFLATE_DEPTH (10) chunks on the device and leave the rest to the host pool, XCK_GPU_INFLATE_RING (12)
 *                                         chunks in flight in all; <percent>: a fixed share; 0 = host only.  XCK_GPU_INFLATE_FREE_CUS (32): CUs the
 *                                         inflate streams never use.  Bit-identical results either way (a block the kernel does not finish, and every
 *                                         chunk after a runtime error, is inflated by the host); off for handles without a device and with XCK_F_VERIFY_CRC
 *                                         alone (XCK_F_DEVICE_CRC keeps it on).
 *   XCK_GPU_PARSE=auto|0                  auto (the default): the records of the GPU-inflated chunks are walked and parsed on the device too
 *                                         (csrc/parse_dev.hip) and never visit the host - where the handle drives a GPU, the key is a UMI tag, every
 *                                         barcode is at most 18 bytes and the call sets no max_records.  A chunk the device cannot finish (a record that
 *                                         straddles blocks, a UMI that has to be interned, a damaged block, bytes carried in from the chunk before, a
 *                                         reader used through xck_bam_next_batch) takes the host path, which also reports every error; after four such
 *                                         chunks in a row the reader stops asking.  0: walk and parse on the host.  Bit-identical results either way;
 *                                         xck_decode_stats.gpu_parse_chunks / gpu_parse_fallbacks count them.
 *   XCK_GPU_NAMES=1                       (opt-in; unset or 0: nothing is allocated, launched or changed) device-names mode: a handle whose key is the
 *                                         read name (umi_tag == "") interns the names in a table in HBM (csrc/intern_dev.hip) instead of the host's, so
 *                                         its GPU-inflated chunks are walked and parsed on the device as those of a UMI handle are.  On for the life of
 *                                         a handle that drives a GPU, has an empty umi_tag and barcodes of at most 18 bytes (or none), with XCK_GPU_PARSE
 *                                         not 0 and the GPU share of the inflate not off (XCK_GPU_INFLATE=0, XCK_F_VERIFY_CRC alone); any other handle
 *                                         ignores the knob.  EVERY read name of xck_ingest_bam is then keyed by the device table: the chunks the host
 *                                         parses (pool-inflated chunks, the tail of a file, fallbacks, calls with max_records) send their names along
 *                                         with their columns, so a name has one key whichever side parsed its chunk.  The table is cleared where the
 *                                         host's is (xck_reset; per BAM without barcodes), grows between launches, and fails the ingest with
 *                                         XCK_E_CAPACITY when the id space of the key width is used up (as the host's does; XCK_TEST_INTERN_LIMIT
 *                                         applies), with XCK_E_NOMEM when it cannot grow.  xck_bam_next_batch keeps the host's table: on such a handle
 *                                         the two kinds of decode call do not mix between two clears - the second kind answers XCK_E_STATE.  Identical
 *                                         matrices either way; xck_decode_stats.gpu_names_* count.  With XCK_DEBUG_TIMING one line at xck_destroy.
 *   XCK_GPU_NAMES_SLOTS0=<slots>, XCK_GPU_NAMES_ARENA0=<bytes>   first sizes of that table (defaults 2^21 slots, 64 MB; tests: 64 and 4096 make a small
 *                                         file grow it several times).  XCK_TEST_NAMES_HASH_BITS=<n> (tests): the device table keeps only the low n bits of
 *                                         the hash - at 4 every probe chain holds thousands of names and the byte comparison has to decide.
 *   XCK_VERIFY_CRC=0|host|device          check the CRC32 of every BGZF block the record decoder inflates, as if the handle had been made with
 *                                         XCK_F_VERIFY_CRC (host: the GPU share of the inflate is off) or XCK_F_DEVICE_CRC (device: the GPU share checks
 *                                         its own blocks) - for front-ends and benchmarks whose calls do not carry the flags.  0 (the default) adds
 *                                         nothing to the flags; any other value means host.  Intact files give identical results either way; a damaged
 *                                         block fails the decode call with XCK_E_IO ("BGZF CRC mismatch", the file and the block's offset) instead
 *                                         of being counted.
 *   XCK_TAG_FILTER=TAG:VALUE[/MASK]       (opt-in; unset: no record is looked at twice and no result changes) the read filter of xck_config.filter_tag /
 *                                         filter_mask / filter_value for front-ends whose calls do not carry the fields: a record counts only when the first
 *                                         occurrence of the two-character TAG is an integer v with 0 <= v <= 0xFFFFFFFF and (v & MASK) == VALUE.  VALUE and
 *                                         MASK are decimal or 0x hex, MASK defaults to 0xFFFFFFFF: xf:25 keeps the reads Cell Ranger counted with the usual
 *                                         flags, xf:8/8 every read that is the one counted for its UMI.  Non-empty config fields win over the knob; a
 *                                         malformed value fails xck_create with XCK_E_ARG.  Decode-only handles honour it (the host parser applies it).
 *                                         A rejected record stays in its batch with cell = XCK_CELL_FILTERED; xck_decode_stats.tag_filtered counts them.
 *   XCK_READ_FATE=1                       every handle that drives a GPU counts where its reads went, as if made with XCK_F_READ_FATE (xck_get_read_fate) -
 *                                         for front-ends whose calls do not carry the flags: they then write read_summary.tsv next to their matrices.
 *                                         One small kernel more per join launch; off (the default, or 0) nothing is allocated or launched.  Decode-only
 *                                         handles ignore it.
 *   XCK_CELL_SUMMARY=1                    every handle that drives a GPU also keeps the per-cell table, as if made with XCK_F_CELL_SUMMARY
 *                                         (xck_get_cell_summary; implies XCK_READ_FATE=1): the front-ends then write cell_summary.tsv next to
 *                                         read_summary.tsv.  Off (the default, or 0) nothing is allocated or launched.  Decode-only handles ignore it.
 *   XCK_CELL_SUMMARY_SLOTS=<rows>         rows of the per-block LDS table of the per-cell accumulation (default and upper bound 512, rounded down to a
 *                                         power of two; tests: a small table reaches the path of the rows that do not fit with small inputs).  The same
 *                                         number governs the table of the per-feature / per-SNP accumulation (default and upper bound 1024 there)
 *   XCK_FEATURE_SUMMARY=1                 every handle that drives a GPU also keeps the per-feature and per-SNP tables, as if made with
 *                                         XCK_F_FEATURE_SUMMARY (xck_get_feature_summary): the front-ends then write feature_summary.tsv and, for the
 *                                         pileup, snp_summary.tsv next to their matrices.  One kernel more per join launch; does not imply XCK_READ_FATE.
 *                                         Off (the default, or 0) nothing is allocated or launched.  Decode-only handles ignore it.
 *   XCK_UMI_CONSENSUS=1                   every handle with a BAF pipeline that drives a GPU decides the base of a molecule by a plurality vote over its
 *                                         reads, as if made with XCK_F_UMI_CONSENSUS (xck_get_molecule_stats): the front-ends then write
 *                                         molecule_summary.tsv next to their BAF matrices, and step 1 and step 3 of one `xcltk baf` run use the same
 *                                         rule.  Off (the default, or 0) the reference's first-read rule holds and every output is byte-identical.
 *                                         Basefc-only and decode-only handles ignore it.
 *   XCK_MIN_BASEQ=<Q>                     (opt-in; 1 .. 93, unset or 0: off) every handle with a BAF pipeline that drives a GPU and whose
 *                                         xck_config.min_baseq is 0 runs with that base-quality floor, as if the field were set: the front-ends
 *                                         (afc_wrapper, afc_variants, pileup(), both `xcltk baf` paths) then log one line with the floor, the (read, SNP)
 *                                         pairs that showed a base and those the floor masked.  A value above 93 or one that is not a number fails
 *                                         xck_create with XCK_E_ARG.  Off, no quality byte is read, kept or copied and the default kernels run.
 *                                         Basefc-only and decode-only handles ignore it.
 *   XCK_UMI_FEATURE=unique|all            (opt-in; unset, empty or `all`: off) every handle with a basefc pipeline that drives a GPU counts a molecule
 *                                         (contig, cell, UMI) only when exactly one region of that contig accepted its reads, as if made with
 *                                         XCK_F_UNIQUE_FEATURE (xck_get_umi_feature_stats): the front-ends then write umi_feature_summary.tsv next to
 *                                         their count matrix.  Any other value fails xck_create with XCK_E_ARG.  Off, no kernel is added and every
 *                                         output is byte-identical.  BAF-only and decode-only handles ignore it.
 *   XCK_UMI_DEDUP=1mm_all|exact           (opt-in; unset, empty or `exact`: off) every handle with a basefc pipeline that drives a GPU counts, per
 *                                         (region, cell), the connected components of the graph that joins UMIs one substitution apart, as if made
 *                                         with XCK_F_UMI_COLLAPSE (xck_get_umi_dedup_stats): the front-ends then write umi_dedup_summary.tsv next
 *                                         to their count matrix.  Any other value fails xck_create with XCK_E_ARG.  Read once, at xck_create.  Off,
 *                                         no kernel is added and every output is byte-identical.  BAF-only and decode-only handles ignore it.
 *   XCK_GROUP_LONG_ROW=<entries>          xck_group_counts: a source row with at least this many entries is summed by one block with a table in
 *                                         LDS, a shorter one by one wave in registers (default and upper bound 64, at least 1; tests: a small value
 *                                         reaches the block shape with small inputs)
 *   XCK_REF_CHUNK_BYTES=<bytes>           xck_set_contig_ref: raw FASTA bytes per staging chunk (default 32 MiB, 64 .. 2^30; tests: 64 cuts a tiny
 *                                         contig into many chunks).  Read once, at xck_create
 *   XCK_CELL_GROUPS=<file>                (read by the Python front-ends, not by a handle) a TSV of name<TAB>group lines without a header, name = a
 *                                         barcode or a sample id; groups are numbered by first appearance, names that are not cells of the run are
 *                                         ignored (their number goes to the log), cells not named are left out.  The front-ends then write, next to
 *                                         their cell matrices, the same matrices summed per group (xck_group_counts): groups.tsv + matrix.groups.mtx
 *                                         (basefc), xcltk.groups.tsv + xcltk.{AD,DP,OTH}.groups.mtx (BAF step 3), cellSNP.groups.tsv +
 *                                         cellSNP.tag.{AD,DP,OTH}.groups.mtx (BAF step 1, raw and filtered).  A multi-GPU run that gathers its result
 *                                         on one rank (XCK_DIST_GATHER=1) logs one line and writes no group files.  Unset: nothing is allocated,
 *                                         launched or written.
 *   XCK_DEVICE_PHASING=1                  (read by the Python front-ends, not by a handle) region-wise local phasing before the allele-specific counting runs
 *                                         on the device (xck_local_phase below; xcltk_amd/baf/fc/phasing_dev.py) instead of the float64 host loop
 *                                         of baf/fc/phasing.py, which stays the default and the specification.  Covers afc_wrapper, afc_variants and the
 *                                         one-pass `xcltk baf`.  With no usable device the front-end says so in its log and runs the host loop.
 *   XCK_PHASE_WCAP=<snps>, XCK_PHASE_LDS_SNPS=<snps>, XCK_PHASE_BLOCKS=<n>   xck_local_phase, read at every call (tests: small values reach the other path with small regions):
 *                                         regions of at most WCAP SNPs (default and upper bound 512) keep their smoothing weights in the workgroup's HBM
 *                                         scratch slice, larger ones recompute them; regions of at most LDS_SNPS SNPs (default and upper bound 1024)
 *                                         keep their per-SNP state in LDS, larger ones in the slice; a launch has at most BLOCKS workgroups (default and upper
 *                                         bound 2048), which walk the regions of a level in a grid-stride loop.  None changes a result.
 *   XCK_WRITE_MAP=1                       (read at every xck_write_mtx; csrc/mtx_writer.h) the text is formatted straight into a MAP_SHARED mapping of the
 *                                         file, allocated at its final size first (regular files on file systems with fallocate; anything else, and a
 *                                         failed allocation, takes the default path).  Unset or 0, the default: threads format into a ring of buffers
 *                                         and the calling thread writes them in file order.  Identical bytes either way; the mapped path is the faster
 *                                         one on tmpfs and the slower one where a write fault costs more than the copy it saves (ext4, overlayfs).
 *                                         Either way a file that is already there is overwritten in place and cut to its new size, never emptied first.
 *   XCK_WRITE_CHUNK_ENTRIES=<entries>     (read at every xck_write_mtx / xck_mtx_part_size / xck_write_mtx_part) entries per unit of work of the writer's
 *                                         threads (default 262144, at most 2^24; tests: a small value cuts tiny matrices into many chunks)
 * Decoder (read when a BAM is opened or once per process): XCK_THREADS, XCK_NUMA=0, XCK_INFLATE=zlib, XCK_CHUNK_BYTES,
 * XCK_WRITE_THREADS (writer threads of xck_write_mtx, read at every call), XCK_TEST_INTERN_LIMIT (tests). */
#ifndef XCK_H
#define XCK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (XCK_F_DEVICE_CRC, xck_decode_stats and xck_get_decode_stats are additive: ABI 3 is unchanged, callers that do not use them see no difference) */
#define XCK_ABI_VERSION 3   /* 3: xck_stats.fold_path / fold_fallbacks / pileup_sort_path / fold_refinements / pileup_sort2_path; 2: xck_config.n_excl_pairs / excl_region / excl_snp, xck_ingest_opts.pause_records (older, shorter xck_config / xck_ingest_opts are still accepted: they carry struct_size.  xck_stats does not: xck_get_stats writes the whole ABI-3 struct, so its caller must be built against this header - check xck_abi_version() first) */

/* status codes */
#define XCK_OK            0
#define XCK_E_ARG        -1   /* invalid argument / configuration            */
#define XCK_E_DEVICE     -2   /* HIP runtime error, or no device             */
#define XCK_E_NOMEM      -3
#define XCK_E_IO         -4   /* file / BGZF / BAM format error              */
#define XCK_E_STATE      -5   /* call sequence error                         */
#define XCK_E_CAPACITY   -6   /* key space exhausted (too many interned UMIs)*/

/* counting modes */
#define XCK_MODE_BASEFC   1   /* feature x cell counts        (xcltk basefc)        */
#define XCK_MODE_BAF      2   /* feature x cell AD / DP / OTH (xcltk baf, step 3)   */
#define XCK_MODE_BOTH     3   /* both from ONE decode of the BAM */

/* UMI / read-name key code meaning "no usable key" (tag missing or empty string;
 * reference: check_read() -12, rdr/fc/mcount.py:41, baf/fc/mcount.py:116-117) */
#define XCK_UMI_NONE  0xFFFFFFFFFFFFFFFFull
/* cell column value of a record the handle's tag filter rejected (xck_config.filter_tag).  To every kernel it means what -1 means:
 * the join drops the read and xck_read_fate counts it under no_cell.  Callers of xck_push_batch may pass it themselves. */
#define XCK_CELL_FILTERED (-2)

/* A region ("feature"): 1-based inclusive start/end exactly as in the region TSV
 * (reference load_region_from_txt, rdr/fc/utils.py:10-45).  `contig` indexes the caller's
 * contig table (names with any leading "chr" stripped, utils/grange.py:263).
 * Output row index of a region == its index in this array. */
typedef struct xck_region {
    int32_t contig;
    int32_t start;      /* 1-based inclusive */
    int32_t end;        /* 1-based inclusive */
} xck_region;

/* A phased het SNP (reference SNP class, baf/fc/gfeature.py:8-39). ref/alt are upper-case
 * ASCII in "ACGTN"; ref_hap/alt_hap in {0,1} are the haplotype index of each allele. */
typedef struct xck_snp {
    int32_t contig;
    int32_t pos;        /* 1-based */
    uint8_t ref, alt;
    uint8_t ref_hap, alt_hap;
} xck_snp;

/* Engine configuration.  Replaces the fields of the reference Config objects that the hot
 * path reads (rdr/fc/config.py:5-41, baf/fc/config.py:8-60). */
typedef struct xck_config {
    uint32_t struct_size;       /* sizeof(xck_config), for ABI checking                      */
    int32_t  mode;              /* XCK_MODE_* (BOTH: every pushed batch feeds both pipelines) */
    int32_t  device;            /* HIP device ordinal                                        */
    /* read filter = check_read(), rdr/fc/core.py:46-62 == baf/fc/core.py:18-34 */
    double   min_mapq;          /* drop if mapq < min_mapq                                   */
    int32_t  min_len;           /* drop if #aligned (M/=/X) bases < min_len                  */
    uint32_t incl_flag;         /* if non-zero: drop unless flag & incl_flag                 */
    uint32_t excl_flag;         /* if non-zero: drop if flag & excl_flag                     */
    int32_t  no_orphan;         /* drop paired reads that are not proper pairs               */
    /* basefc include criterion, rdr/fc/core.py:160-165: 0 < v < 1 -> fraction (IEEE double
     * m/float(n) < v drops), otherwise length (m < v drops).                                */
    double   min_include;
    /* BAF: per-SNP filters (baf/fc/core.py:238-246) and haplotype rule (:181-192) */
    double   min_count;
    double   min_maf;
    int32_t  no_dup_hap;
    /* tables */
    int32_t  n_cells;           /* number of matrix columns (barcodes or sample ids)         */
    int32_t  n_contigs;
    int32_t  n_regions;
    const xck_region* regions;
    int32_t  n_snps;            /* BAF only                                                  */
    const xck_snp*    snps;
    /* decoder side (used only by xck_ingest_bam / xck_bam_next_batch) */
    const char* const* barcodes;  /* n_cells NUL-terminated barcodes, or NULL = well mode
                                     (column = sample index of the BAM)                      */
    char     cell_tag[4];       /* e.g. "CB"; "" when barcodes == NULL                       */
    char     umi_tag[4];        /* e.g. "UB"; "" = key is the read name                      */
    /* sizing */
    int64_t  max_batch_reads;   /* upper bound on reads per xck_push_batch (0 = default)     */
    int32_t  n_threads;         /* host decode threads (0 = the CPUs this process may use)   */
    int32_t  flags;             /* XCK_F_*                                                   */
    /* BAF: (region, SNP) pairs left OUT of the SNP -> region join although start <= pos <= end.  Region-wise
     * local phasing drops the SNPs without coverage in the cellsnp data from that region's list
     * (baf/fc/phasing.py:44-49; the SNP still counts in other regions that contain it).  Indices into
     * regions[] / snps[].  Read only when struct_size covers the fields.                      */
    int32_t  n_excl_pairs;
    const int32_t* excl_region;
    const int32_t* excl_snp;
    /* Opt-in read filter on an integer aux tag (10x: "xf"), applied by the decoder (xck_ingest_bam / xck_bam_next_batch, on the host
     * and in the device parse alike).  filter_tag = "" : off.  A record passes when the FIRST occurrence of the tag (htslib
     * bam_aux_get, as for cell_tag / umi_tag) has an integer type (c C s S i I), its value v widened to 64 bits lies in
     * 0 .. 0xFFFFFFFF and ((uint32_t)v & filter_mask) == filter_value.  Every other record - tag absent, of type A Z H f B, negative,
     * or behind an aux value that cannot be skipped - fails: it keeps its place in its batch (ordinals and every other column are
     * as without the filter) and its cell becomes XCK_CELL_FILTERED, whatever its barcode or sample.  The matrices are those of a
     * file from which the failing records were removed.  XCK_E_ARG: a tag that is not two printable characters or equals cell_tag /
     * umi_tag, or filter_value & ~filter_mask != 0 (nothing could pass).  Read only when struct_size covers the fields; the
     * environment's XCK_TAG_FILTER supplies them when filter_tag is empty.                                                  */
    char     filter_tag[4];
    uint32_t filter_mask;
    uint32_t filter_value;
    /* Opt-in minimum base quality of the pileup's allele calls (samtools mpileup -Q, pysam min_base_quality).  0 = off; 1 .. 93: a
     * (read, SNP) pair under an aligned block whose quality byte q at that query offset is not 0xff ("no quality stored", what BAM
     * writes for `*`) and is below min_baseq shows no base - exactly like a read that spans the SNP in a gap: under the default
     * molecule rule it still holds its (SNP, cell, UMI) key (a masked first read silences the molecule), under XCK_F_UMI_CONSENSUS it
     * abstains.  Only allele codes change: the read filter, the hits (xck_stats.n_hits), the summaries' read classes and the basefc half
     * of an XCK_MODE_BOTH handle are those of min_baseq = 0; tallies, min_count / min_maf, xck_refold, xck_snp_counts and
     * xck_group_counts follow.  The mask is applied by the join: a refold cannot change it.  The qualities reach the join through
     * xck_ingest_bam or xck_push_batch_q; xck_push_batch, xck_push_batch_device and xck_bam_next_batch answer XCK_E_STATE on such a
     * handle.  XCK_E_ARG: a value outside 0 .. 93, a basefc-only handle, XCK_F_DECODE_ONLY.  XCK_MIN_BASEQ supplies it when it is 0.
     * The field lies in what was the struct's tail padding, so sizeof(xck_config) is what it was and struct_size cannot tell a
     * caller that knows the field from one whose padding holds whatever was on its stack: the field is read ONLY when flags holds
     * XCK_F_MIN_BASEQ - a bit no earlier caller sets.  A C caller sets BOTH: `cfg.min_baseq = 13; cfg.flags |= XCK_F_MIN_BASEQ;`.
     * Without the bit the four bytes are never looked at (so neither a floor nor the XCK_E_ARG cases above come from them); the bit
     * on a struct whose struct_size ends before the field is XCK_E_ARG.  xck_get_baseq_stats answers XCK_E_STATE on a handle that
     * ended up without a floor, which is how a caller checks that its floor was taken. */
    int32_t  min_baseq;
} xck_config;

#define XCK_F_FORCE_KEY128   1  /* always use 128-bit sort keys (testing)                    */
#define XCK_F_VERIFY_CRC     2  /* verify BGZF CRC32 while decoding (on the host: the GPU share of the inflate is off) */
#define XCK_F_DEVICE_CRC    16  /* verify BGZF CRC32 while decoding, keeping the GPU share of the inflate: blocks inflated on the
                                   device are checked by the kernel (a block it finds damaged is inflated and checked again on the
                                   host), the others by the host.  Takes precedence over XCK_F_VERIFY_CRC.  Either flag: a block
                                   whose CRC32 differs from its footer's fails the decode call with XCK_E_IO                   */
#define XCK_F_LOW_PRIORITY   8  /* run this engine's kernels on a low-priority HIP stream: lets a second
                                   engine fill the GPU while the first one copies results out */
#define XCK_F_READ_FATE     32  /* count, on the device, which of the classes of xck_read_fate every pushed read falls into
                                   (xck_get_read_fate; one more small kernel behind every join launch).  Changes no result.
                                   XCK_E_ARG together with XCK_F_DECODE_ONLY                                              */
#define XCK_F_CELL_SUMMARY  64  /* per-cell table: the classes of xck_read_fate per cell, and after xck_finish the column marginals of
                                   the matrices (xck_get_cell_summary).  Implies XCK_F_READ_FATE (the global counters cost nothing
                                   extra): the per-cell instantiation of that kernel runs in its place.  Changes no result.
                                   XCK_E_ARG together with XCK_F_DECODE_ONLY                                              */
#define XCK_F_FEATURE_SUMMARY 128 /* per-feature and per-SNP tables: which regions lose reads to the include test or share them with an
                                   overlapping region, which SNPs the reads cover, and after xck_finish the row marginals of the
                                   matrices and the allele tallies and filter verdict of every SNP (xck_get_feature_summary; one more
                                   kernel behind every join launch).  Does not imply XCK_F_READ_FATE; combines freely with it and with
                                   XCK_F_CELL_SUMMARY.  Changes no result.  XCK_E_ARG together with XCK_F_DECODE_ONLY            */
#define XCK_F_UMI_CONSENSUS 256 /* pileup: the base a molecule (SNP, cell, UMI) shows is decided by a plurality vote over its reads that
                                   show a base there - buckets A / C / G / T, a tie goes to the bucket seen earliest in fetch order,
                                   a read that shows N abstains unless nothing else was seen - instead of by its first read, and a
                                   read that spans the SNP in an N / D gap abstains instead of silencing the molecule.  Everything
                                   downstream (tallies, min_count / min_maf, xck_refold, xck_snp_counts, xck_group_counts, the SNP
                                   table of xck_get_feature_summary) follows.  The same kernels count how often the reads of a
                                   molecule disagree (xck_get_molecule_stats).  Any handle with a BAF pipeline; on XCK_MODE_BOTH it
                                   affects the BAF half only.  XCK_E_ARG on a basefc-only handle and together with XCK_F_DECODE_ONLY */
#define XCK_F_MIN_BASEQ    512  /* xck_config.min_baseq holds a value (see there); without the bit the field's bytes are not read    */
#define XCK_F_UNIQUE_FEATURE 1024 /* basefc: a molecule - (contig of the region, cell, UMI key code), over all keys the join accepted since
                                   the last reset - counts only when exactly one row (entry of the region table) of that contig holds
                                   it; a molecule that two or more rows hold is dropped from all of them.  Two entries with the same
                                   interval are two rows: the molecules they share drop.  The same (cell, UMI) on two contigs is two
                                   molecules.  The read-level numbers (n_hits, n_hits_unique, xck_get_read_fate, the read columns of
                                   the summaries) describe the join and do not change; the matrix, its marginals in the summaries
                                   and xck_group_counts follow.  xck_get_umi_feature_stats counts what was dropped.  Any handle with
                                   a basefc pipeline; on XCK_MODE_BOTH the BAF half is untouched.  XCK_E_ARG on a BAF-only handle
                                   and together with XCK_F_DECODE_ONLY                                                          */
#define XCK_F_UMI_COLLAPSE 2048 /* basefc: 1-mismatch UMI collapsing (STARsolo's 1MM_All, UMI-tools' cluster).  Within one (row, cell) two
                                   of the distinct keys the join accepted since the last reset are adjacent when both UMI key codes
                                   are direct 2-bit codes (xck_umi_bits) of the same length that differ in exactly one base; the
                                   matrix value is the number of connected components of that graph instead of the number of keys.
                                   Interned codes (a UMI with N, an over-long UMI, a read name) are adjacent to nothing.  Cells and
                                   rows never interact; the result does not depend on read, batch or shard order.  With
                                   XCK_F_UNIQUE_FEATURE the unique-feature rule runs first, on exact UMIs, and its survivors are
                                   collapsed.  The read-level numbers (n_hits, n_hits_unique, xck_get_read_fate, the read columns of
                                   the summaries) describe the join and do not change; the matrix, its marginals in the summaries
                                   and xck_group_counts follow.  xck_get_umi_dedup_stats counts what was merged.  Any handle with a
                                   basefc pipeline; on XCK_MODE_BOTH the BAF half is untouched.  XCK_E_ARG on a BAF-only handle and
                                   together with XCK_F_DECODE_ONLY                                                              */
#define XCK_F_BASE_TALLY 0x1000 /* (= 4096) pileup: pseudo-bulk base tallies.  Per contig that received reads the handle keeps four 32-bit counters
                                   A, C, G, T per reference position (16 bytes per position: about 50 GB for every contig of a human
                                   genome; a contig's table is allocated and zeroed when its first batch is queued).  Every read that
                                   passes the read filter (mapq, flags, orphan, cell >= 0, UMI != XCK_UMI_NONE, min_len; regions and
                                   SNPs are not asked) adds, for every base of an M, = or X operation, one to the counter of the
                                   4-bit code 1, 2, 4 or 8 at that reference position; any other code (N, IUPAC, the pad nibble, a
                                   read without stored sequence) counts as bases_other, a base under the handle's base-quality floor
                                   as bases_masked, a base at or beyond the contig's length as bases_out_of_range.  Reads are
                                   counted, not molecules.  Needs xck_set_contig_lengths before the first push; with the flag a batch
                                   on a contig without SNPs is queued like any other.  xck_get_base_tally, xck_get_base_tally_stats
                                   and xck_find_candidates read the tables.  Any handle with a BAF pipeline; on XCK_MODE_BOTH the
                                   basefc half is untouched.  XCK_E_ARG on a basefc-only handle and together with XCK_F_DECODE_ONLY.
                                   No environment knob                                                                          */
#define XCK_F_DECODE_ONLY    4  /* handle drives the BAM decoder only: no GPU is touched, and
                                   xck_push_batch / xck_finish fail (used to run the host
                                   ingest on machines without a device; NOT a compute path)  */

/* One batch of decoded alignment records, structure-of-arrays, all reads on ONE contig,
 * in file order.  This is what the reference obtains record by record from
 * pysam.AlignmentFile.fetch() (utils/sam.py:85-118).  Host pointers (ideally pinned). */
typedef struct xck_batch {
    int32_t  contig;            /* engine contig id; <0 : batch is skipped                   */
    int32_t  n_reads;
    uint64_t ordinal_base;      /* fetch-order ordinal of read 0: (bam_index << 40) | record#;
                                   read i has ordinal_base + i  (baf/fc/mcount.py:118-119:
                                   first read of a UMI in fetch order decides the allele)    */
    const int32_t*  pos;        /* [n]   0-based leftmost reference coordinate               */
    const uint16_t* flag;       /* [n]   BAM FLAG                                            */
    const uint8_t*  mapq;       /* [n]                                                       */
    const int32_t*  cell;       /* [n]   column index; <0 = tag missing / not in list (-1), or
                                   XCK_CELL_FILTERED (-2): rejected by the handle's tag filter -
                                   callers may pass either, the kernels treat them alike      */
    const uint64_t* umi;        /* [n]   key code (see xck_umi_bits) or XCK_UMI_NONE         */
    const uint32_t* cig_off;    /* [n+1] offsets into cigar[]                                */
    const uint32_t* cigar;      /* BAM CIGAR words (len << 4 | op)                           */
    const uint32_t* seq_off;    /* [n+1] BYTE offsets into seq[] (BAF only, else NULL)       */
    const uint8_t*  seq;        /* BAM 4-bit packed bases, each read starts on a byte        */
} xck_batch;

/* Sparse result in coordinate form, sorted by (row, col), no zero entries.
 * row = region index (0-based, input order), col = cell index (0-based). Engine-owned
 * host memory, valid until xck_destroy(). */
typedef struct xck_coo {
    int64_t nnz;
    const int32_t* row;
    const int32_t* col;
    const int32_t* val;
} xck_coo;

typedef struct xck_result {
    xck_coo count;              /* XCK_MODE_BASEFC: matrix.mtx  (rdr/fc/core.py:109-116)     */
    xck_coo ad, dp, oth;        /* XCK_MODE_BAF: AD/DP/OTH.mtx  (baf/fc/core.py:84-99)       */
} xck_result;

typedef struct xck_stats {
    int64_t n_batches;
    int64_t n_reads;            /* records pushed (every decoded BAM record counts)          */
    int64_t n_hits;             /* (read,region) or (read,SNP) pairs accepted by the join    */
    int64_t n_hits_unique;      /* keys that reached HBM after the in-LDS de-duplication     */
    double  ms_h2d;             /* host-measured, cumulative                                 */
    double  ms_device;          /* HIP-event time of all kernels, cumulative                 */
    double  ms_join;            /* HIP-event time of the join/pileup kernels only            */
    double  ms_sort;            /* HIP-event time of sort + reduce kernels                   */
    double  ms_d2h;             /* HIP-event time of the result copy-out (copy stream)       */
    int64_t algo_bytes_join;    /* algorithmic bytes of the join kernels         */
    int64_t n_join_launches;    /* fused join kernel launches (device-resident batches are fused) */
    int32_t key_bits;           /* 64 or 128                                                 */
    int32_t umi_bits;
    int32_t fold_path;          /* basefc fold of the last xck_finish: 0 none yet, 1 partition fold (no sort), 2 radix-sort fold */
    int32_t fold_fallbacks;     /* finishes of this handle in which the partition fold handed over to the radix-sort fold   */
    int32_t pileup_sort_path;   /* pileup hits of the last xck_finish: 0 none yet, 1 row partition + LDS sort per item, 2 radix sort */
    int32_t fold_refinements;   /* partition fold of the last xck_finish: times the level-2 geometry had to be refined (uneven cells) */
    int32_t pileup_sort2_path;  /* pileup, region-level hits of the last xck_finish: 0 none, 1 partition + per-item hash classification (no sort), 2 radix sort, 3 partition + LDS sort per item */
    int32_t gpu_inflate_chunks; /* BGZF chunks (~740 blocks each) whose inflate ran on the GPU since the last xck_reset (XCK_GPU_INFLATE; was reserved0) */
} xck_stats;

/* What the BAM decoder of a handle did, since the last xck_reset, summed over the readers that fed it (xck_ingest_bam,
 * xck_bam_next_batch, xck_bam_prefetch; a reader's counts reach the handle at the end of each of these calls).  struct_size =
 * sizeof(xck_decode_stats), as for xck_config / xck_ingest_opts. */
typedef struct xck_decode_stats {
    uint32_t struct_size;
    uint32_t reserved0;
    int64_t gpu_inflate_chunks;       /* BGZF chunks inflated on the GPU (XCK_GPU_INFLATE; = xck_stats.gpu_inflate_chunks)        */
    int64_t gpu_inflate_blocks;       /* BGZF blocks of those chunks                                                              */
    int64_t gpu_blocks_left_to_host;  /* blocks of device chunks the host inflated: non-zero kernel status (INFLATE_ST_CRC included), or the whole chunk after a runtime error */
    int64_t crc_blocks_device;        /* non-empty blocks whose CRC32 the kernel checked and found right (XCK_F_DEVICE_CRC)       */
    int64_t crc_blocks_host;          /* non-empty blocks whose CRC32 the host checked and found right (either CRC flag)          */
    int64_t crc_mismatch_device;      /* blocks the kernel found with a CRC32 that differs from the footer's                      */
    int64_t crc_device_host_disagree; /* ... of which the host's check passed (the host's bytes are used; 0 unless the device erred) */
    int64_t gpu_path_given_up;        /* readers whose GPU share of the inflate was turned off by a runtime error or lack of memory */
    /* appended (a caller with the shorter struct gets the fields above): */
    int64_t gpu_parse_chunks;         /* GPU-inflated chunks whose records were walked and parsed on the device too (XCK_GPU_PARSE) */
    int64_t gpu_parse_fallbacks;      /* device-walked chunks that took the host path after all (straddling record, UMI to intern, ...) */
    /* appended after those (XCK_GPU_NAMES; a caller with a shorter struct gets the fields above): */
    int64_t gpu_names_interned;       /* read names looked up in the device table (directly codable and empty names need no table)  */
    int64_t gpu_names_distinct;       /* ids the device table handed out since its last clear, summed over the clears               */
    int64_t gpu_names_host_chunks;    /* host-parsed chunks (pool-inflated, tails, fallbacks, max_records) whose names were keyed on the device */
    /* appended after those (xck_config.filter_tag / XCK_TAG_FILTER; a caller with a shorter struct gets the fields above): */
    int64_t tag_filtered;             /* records that reached a batch with cell == XCK_CELL_FILTERED; a device-parsed chunk that fell back to the host counts once */
} xck_decode_stats;

/* Where the reads of ONE pipeline went, since the last xck_reset (handles made with XCK_F_READ_FATE; additive, ABI 3 is unchanged).
 * Every pushed record falls into exactly one class - the first that applies, in the order of the fields, which is the order of the
 * reference's check_read() (rdr/fc/core.py:46-62 == baf/fc/core.py:18-34) followed by fetch() and the include test:
 * n_reads == not_joined + low_mapq + ... + assigned.  struct_size = sizeof(xck_read_fate), as for xck_decode_stats. */
typedef struct xck_read_fate {
    uint32_t struct_size;
    int32_t  mode;              /* XCK_MODE_BASEFC or XCK_MODE_BAF: the pipeline these counters belong to                    */
    int64_t  n_reads;           /* = xck_stats.n_reads                                                                        */
    int64_t  not_joined;        /* reads of batches no kernel saw (counted on the host): batch contig < 0, or a contig without
                                   a region (basefc) / without a SNP (BAF) in this handle's tables                             */
    int64_t  low_mapq;          /* mapq < min_mapq                                    (check_read -2,  rdr/fc/core.py:47-48)  */
    int64_t  excl_flag;         /* excl_flag && (flag & excl_flag)                    (-3,  :49-50)                           */
    int64_t  incl_flag;         /* incl_flag && !(flag & incl_flag)                   (-4,  :51-52)                           */
    int64_t  orphan;            /* no_orphan, paired and not a proper pair            (-5,  :53-54)                           */
    int64_t  no_cell;           /* cell < 0: tag missing, empty, or barcode not in the list (-11, :55-56; rdr/fc/mcount.py push_read);
                                   includes the reads the handle's tag filter rejected (cell == XCK_CELL_FILTERED) that pass the four tests above */
    int64_t  no_umi;            /* key == XCK_UMI_NONE: tag missing or empty          (-12, :57-58)                           */
    int64_t  short_aligned;     /* aligned (M/=/X) bases < min_len                    (-21, :59-60)                           */
    int64_t  no_target;         /* basefc: no region with pos < end0 && endpos > start0 (the fetch() of utils/sam.py:85-118);
                                   BAF: no SNP of the list with pos <= p0 < endpos (whether the SNP lies in a region is not asked) */
    int64_t  include_fail;      /* basefc only: fetched by at least one region, none passes min_include (rdr/fc/core.py:160-165) */
    int64_t  assigned;          /* at least one region accepts the read / at least one SNP is covered                         */
    int64_t  multi;             /* ... of which two or more do (duplicate regions / SNPs count each, as in the join)           */
    int64_t  pairs;             /* accepted (read, region) / (read, SNP) pairs, summed over the assigned reads: = the pipeline's
                                   share of xck_stats.n_hits                                                                  */
} xck_read_fate;

/* The per-cell table of ONE pipeline, since the last xck_reset (handles made with XCK_F_CELL_SUMMARY; additive, ABI 3 is unchanged).
 * fate: what xck_read_fate counts, per cell - every read the pipeline's kernels saw adds 1 to its class in its row (its cell, or row
 * n_cells when cell < 0), an assigned read also its pairs, and 1 to multi when it has two or more.  The column sums equal the fields of
 * xck_read_fate from low_mapq to pairs.  not_joined stays global-only: those batches reach no kernel, so no row sees their reads.
 * matrix: column marginals of the result of xck_finish, computed on the device from its result blocks the first time the table is asked
 * for after the finish.  basefc: umis / pairs of a cell is the share of its accepted pairs that survived the UMI de-duplication.
 * The arrays are engine-owned host memory, valid until the next xck_get_cell_summary, xck_reset or xck_destroy on the handle. */
typedef struct xck_cell_summary {
    uint32_t struct_size;
    int32_t  mode;              /* XCK_MODE_BASEFC or XCK_MODE_BAF: the pipeline, as xck_read_fate.mode                          */
    int32_t  n_cells;           /* rows 0..n_cells-1 = the matrix columns; row n_cells = the reads with cell < 0               */
    int32_t  n_fate_cols;       /* 12: the fields of xck_read_fate from low_mapq to pairs, in that order                        */
    const int64_t* fate;        /* [(n_cells + 1) * n_fate_cols], row-major                                                     */
    int32_t  has_matrix;        /* 1 once xck_finish has run since the last xck_reset                                           */
    int32_t  n_matrix_cols;     /* basefc 2: umis (column sum of count), features (entries of the column);
                                   BAF 4: ad, dp, oth (column sums), features (entries of the DP column)                        */
    const int64_t* matrix;      /* [n_cells * n_matrix_cols], row-major; NULL while has_matrix == 0                             */
} xck_cell_summary;

/* The per-feature and per-SNP tables of ONE pipeline, since the last xck_reset (handles made with XCK_F_FEATURE_SUMMARY; additive, ABI 3 is
 * unchanged).  All arrays are row-major int64 in the caller's INPUT order of xck_config.regions / xck_config.snps (a region or SNP the
 * engine's tables leave out - contig outside the table, SNP position < 1 - keeps a row of zeros), engine-owned host memory, valid until
 * the next xck_get_feature_summary, xck_reset or xck_destroy on the handle.
 * reads (basefc only, available before xck_finish): over the (read, region) pairs of the reads that pass everything up to short_aligned in
 *   the classes of xck_read_fate - check_read, a listed cell, a non-empty key, min_len: include_fail = pairs that pass the fetch overlap
 *   (pos < end0 && endpos > start0) but fail min_include; pairs = pairs the join accepts (the column sums to the pipeline's share of
 *   xck_stats.n_hits); shared = accepted pairs whose read is accepted by two or more regions.  Duplicate regions each get their own numbers.
 * matrix (after xck_finish), computed on the device from the result blocks the first time the table is asked for after the finish:
 *   basefc  umis (row sum of count), cells (entries of the row);
 *   BAF     snps (SNPs of the list joined to the region, after excl_region / excl_snp), snps_kept (those that pass min_count / min_maf),
 *           ad, dp, oth (row sums), cells (entries of the DP row).
 * snp (BAF only): reads = filtered reads whose fetch span covers the SNP (pos <= p0 < endpos, a SNP inside an N gap included: the per-SNP
 *   split of xck_read_fate.pairs; available before xck_finish); a c g t n = the pseudo-bulk tallies of the fold, one count per
 *   (cell, UMI) that shows a base, the base being the one the handle's rule decides (the first read's, or the vote of XCK_F_UMI_CONSENSUS;
 *   the reference's MCount.tcount order); kept = verdict of the fold's own per-SNP filter (plp_snp,
 *   baf/fc/core.py:238-246) under xck_config.min_count / min_maf of THIS handle, 0 or 1 (a front-end that filters later, on sums of the
 *   matrices, creates the handle with 1 / 0: kept then only says that a molecule showed a base); regions = regions the SNP feeds.  Tallies and kept are zero while has_matrix == 0. */
typedef struct xck_feature_summary {
    uint32_t struct_size;
    int32_t  mode;              /* XCK_MODE_BASEFC or XCK_MODE_BAF: the pipeline, as xck_read_fate.mode                          */
    int32_t  n_regions;         /* rows of reads and matrix                                                                    */
    int32_t  n_read_cols;       /* basefc 3: include_fail, pairs, shared; BAF 0                                                */
    const int64_t* reads;       /* [n_regions * n_read_cols]; NULL for the BAF pipeline                                        */
    int32_t  has_matrix;        /* 1 once xck_finish has run since the last xck_reset                                          */
    int32_t  n_matrix_cols;     /* basefc 2, BAF 6 (see above)                                                                 */
    const int64_t* matrix;      /* [n_regions * n_matrix_cols]; NULL while has_matrix == 0                                     */
    int32_t  n_snps;            /* BAF: xck_config.n_snps; basefc 0                                                            */
    int32_t  n_snp_cols;        /* BAF 8: reads, a, c, g, t, n, kept, regions                                                  */
    const int64_t* snp;         /* [n_snps * n_snp_cols]; NULL for the basefc pipeline                                         */
} xck_feature_summary;

/* How the reads of the molecules of the last xck_finish agree (handles made with XCK_F_UMI_CONSENSUS; additive, ABI 3 is unchanged).  A
 * molecule is a (SNP, cell, UMI) with at least one read that shows a base at the SNP; reads that span the SNP in a gap are not looked
 * at.  Buckets are A, C, G, T and N (any other nibble).  struct_size = sizeof(xck_molecule_stats), as for xck_decode_stats. */
typedef struct xck_molecule_stats {
    uint32_t struct_size;
    int32_t  consensus;         /* 1: the handle votes (the only value a successful call returns)                               */
    int64_t  molecules;         /* molecules                                                                                   */
    int64_t  multi_read;        /* ... with two or more reads that show a base                                                 */
    int64_t  discordant;        /* ... whose reads fall into two or more buckets (N counts as a bucket here)                   */
    int64_t  tied;              /* ... where two or more of A / C / G / T share the largest number of reads                    */
    int64_t  changed;           /* ... whose winning bucket is not the bucket of the earliest read with a base: the molecules
                                   that the first-read rule would have called differently, gap reads aside                    */
} xck_molecule_stats;

/* What the unique-feature rule of the last xck_finish saw (handles made with XCK_F_UNIQUE_FEATURE; additive, ABI 3 is unchanged).  A
 * molecule is a (contig, cell, UMI) with at least one accepted (row, cell, UMI) key on that contig.  keys - keys_dropped is the sum of
 * the count matrix.  struct_size = sizeof(xck_umi_feature_stats), as for xck_decode_stats. */
typedef struct xck_umi_feature_stats {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t  molecules;         /* molecules with at least one key                                                             */
    int64_t  multi_feature;     /* ... that two or more rows of their contig hold: dropped from all of them                    */
    int64_t  keys;              /* distinct (row, cell, UMI) keys: what the fold counts without the flag                        */
    int64_t  keys_dropped;      /* ... of them the keys of the multi_feature molecules                                         */
} xck_umi_feature_stats;

/* What the 1-mismatch UMI collapsing of the last xck_finish saw (handles made with XCK_F_UMI_COLLAPSE; additive, ABI 3 is unchanged).
 * A group is one (row, cell) with at least one key.  struct_size = sizeof(xck_umi_dedup_stats), as for xck_decode_stats. */
typedef struct xck_umi_dedup_stats {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t  keys;              /* distinct exact (row, cell, UMI) keys entering the stage (behind the unique-feature rule, if set) */
    int64_t  molecules;         /* connected components: the sum of the count matrix                                           */
    int64_t  groups;            /* (row, cell) groups: the non-zeros of the count matrix                                       */
    int64_t  groups_changed;    /* ... whose value is smaller than their number of keys                                        */
    int64_t  opaque_keys;       /* keys with an interned UMI code: never merged                                                */
    int64_t  max_group;         /* keys of the largest group                                                                   */
} xck_umi_dedup_stats;

/* The pairs the base-quality floor saw (xck_config.min_baseq / XCK_MIN_BASEQ; xck_get_baseq_stats): (read, SNP) pairs of the pileup
 * pipeline's join since the last reset in which the read stores a base at the SNP, and those of them the floor masked.
 * struct_size = sizeof(xck_baseq_stats), as for xck_decode_stats. */
typedef struct xck_baseq_stats {
    uint32_t struct_size;
    int32_t  min_baseq;         /* the handle's floor                                         */
    int64_t  pairs_with_base;
    int64_t  pairs_masked;
} xck_baseq_stats;

/* The counters of the base tally pass since the last reset (handles made with XCK_F_BASE_TALLY; additive, ABI 3 is unchanged).
 * struct_size = sizeof(xck_base_tally_stats), as for xck_decode_stats. */
typedef struct xck_base_tally_stats {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t  reads_tallied;     /* reads that passed the read filter                                              */
    int64_t  bases_tallied;     /* aligned bases that added to A, C, G or T                                       */
    int64_t  bases_other;       /* aligned bases whose 4-bit code is not 1, 2, 4, 8 (or that have no stored code) */
    int64_t  bases_masked;      /* aligned bases under the handle's base-quality floor                            */
    int64_t  bases_out_of_range;/* aligned bases at or beyond the contig's length                                 */
} xck_base_tally_stats;

/* xck_find_candidates: thresholds, and the candidate positions it returns.  For a position with counts c[4] (A, C, G, T) and n their sum,
 * ref is the base with the largest count (the earliest of equals in A, C, G, T), alt the largest of the other three (same tie rule) with
 * count m; the position is a candidate when m > 0, !((double)n < min_count) and !((double)m < (double)n * min_maf) - the arithmetic of
 * the SNP filter of xck_finish with the alt count as the minor count. */
typedef struct xck_candidate_config {
    uint32_t struct_size;       /* sizeof(xck_candidate_config)                              */
    uint32_t reserved;
    double   min_count;
    double   min_maf;
} xck_candidate_config;
typedef struct xck_candidates {
    int64_t  n;                 /* candidates, in (contig, pos) order                        */
    const int32_t*  contig;     /* [n] engine contig id                                      */
    const int32_t*  pos;        /* [n] 1-based                                               */
    const char*     ref;        /* [n] ASCII                                                 */
    const char*     alt;        /* [n]                                                       */
    const uint32_t* count;      /* [n * 4] A C G T                                           */
    int64_t  positions_covered; /* positions of the allocated tables with n > 0              */
} xck_candidates;

typedef struct xck_engine xck_engine;     /* opaque: one per GPU */
typedef struct xck_bam    xck_bam;        /* opaque: one open BAM file */

/* -- library ------------------------------------------------------------------------------- */
const char* xck_version(void);
int         xck_abi_version(void);
int         xck_device_count(void);              /* number of usable HIP devices (0 if none) */
const char* xck_last_error(const xck_engine* e); /* e may be NULL: last error of the creating thread */

/* -- engine (replaces fc_features()/fc_fet1()/plp_snp(): the per-region fetch loops) -------- */
int  xck_create(const xck_config* cfg, xck_engine** out);
void xck_destroy(xck_engine* e);
/* number of bits available for a UMI / read-name key code in xck_batch.umi (26..64):
 *   ACGT-only key of L bases with 2L+1 <= bits-1  ->  (1 << 2L) | 2-bit packed bases (A0 C1 G2 T3)
 *   anything else                                   ->  (1 << (bits-1)) | interned id            */
int  xck_umi_bits(const xck_engine* e);
/* Copy one batch to the GPU (async, overlapped with kernels of the previous batch) and run
 * the join / pileup kernels on it.  The batch arrays may be reused once the call returns.
 * Batches of 2 MB and more cross PCIe straight from the caller's arrays (nine DMA copies, pinned or not: 0.86 - 1.05 G reads/s
 * measured); smaller ones are packed into one engine-owned pinned block and cross with ONE copy whose completion is an
 * event, not a wait (XCK_PUSH_STAGE_BYTES / XCK_PUSH_STAGE=0|1 override the rule).
 * The host arrays are checked first (one linear pass): cig_off / seq_off must not run backwards,
 * cell[i] < n_cells, contig < n_contigs, no null column - otherwise XCK_E_ARG and nothing is queued.
 * A negative cell[i] drops the read: -1 and XCK_CELL_FILTERED (-2, a read the caller's own tag filter rejected) mean the same. */
int  xck_push_batch(xck_engine* e, const xck_batch* b);
/* Same, but the arrays are DEVICE pointers already resident in HBM (benchmarks, pipelines
 * that decode on the GPU side); no copy is made and they must stay valid until xck_flush().
 * The contents cannot be checked from the host: the same invariants are the caller's word. */
int  xck_push_batch_device(xck_engine* e, const xck_batch* b);
/* xck_push_batch with the reads' base qualities, for a handle with a base-quality floor (xck_config.min_baseq): qual holds
 * 2 * (seq_off[n] - seq_off[0]) bytes, two per sequence byte - the quality of query offset qi of read i at
 * 2 * (seq_off[i] - seq_off[0]) + qi, the pad byte of an odd-length read 0xff, 0xff = "no quality stored" anywhere.  Checked and
 * copied as xck_push_batch does; the caller may reuse qual on return.  On a handle without a floor qual is ignored (it may be NULL)
 * and the call is xck_push_batch; with a floor a NULL qual is XCK_E_ARG unless the sequence range is empty. */
int  xck_push_batch_q(xck_engine* e, const xck_batch* b, const uint8_t* qual);
int  xck_flush(xck_engine* e);                    /* wait for all queued device work */
/* Fold all hits into the final sparse matrices (on the GPU: partition + one LDS pass per work item, radix sort
 * as the fallback) and copy them to engine-owned pinned host memory. */
int  xck_finish(xck_engine* e, xck_result* out);
/* Same fold, but returns as soon as the copy-out of the matrices has been ENQUEUED on the engine's copy
 * stream; a following xck_finish() waits for it and hands out the pointers.  Lets the caller run other
 * GPU work (e.g. a second engine) while the matrix crosses PCIe. */
int  xck_finish_async(xck_engine* e);
/* Same matrices as the last xck_finish(), but the pointers are DEVICE addresses ([row|col|val] in the
 * engine's workspace, valid until the next xck_finish / xck_reset): lets a multi-GPU driver exchange the
 * per-contig sparse blocks GPU-to-GPU (RCCL over xGMI) without a host round trip. */
int  xck_get_result_device(xck_engine* e, xck_result* out);
/* Recount the pileup under new tables without the reads (additive: ABI 3 is unchanged).  The read x SNP join and the first half of
 * the pileup fold - the sort of the hits, the base every (SNP, cell, UMI) shows under the handle's rule (its first read's, or the vote of XCK_F_UMI_CONSENSUS), the tallies per SNP - depend on
 * nothing but the reads, the read filters, the cells and the SNP positions; xck_finish keeps what they leave, and xck_refold runs the
 * second half again: the fan-out to the regions, REF / ALT and the haplotype indices, the exclusion pairs, min_count / min_maf and
 * no_dup_hap.  It returns the matrices a fresh handle would return that was created with these tables and filters and the original
 * read filters and cells and was fed the same reads, bit for bit.
 *   regions      the new feature table; output row = index, as in xck_config.  n_regions + 1 must fit the row field of the handle's key
 *                layout, which xck_create sized from max(n_regions, n_snps) + 1: XCK_E_ARG otherwise (create the handle with the
 *                largest table it will see).  Regions on a contig outside the handle's contig table keep empty rows.
 *   snps         NULL / 0 = keep the handle's; otherwise n_snps and every (contig, pos) must equal the list given to xck_create index
 *                by index; ref, alt, ref_hap, alt_hap may differ.
 *   snp_enabled  [n_snps of the handle] or NULL = all; a disabled SNP feeds no region (the handle then answers as one created with
 *                the list without it; in xck_feature_summary.snp its tallies and verdict stay, its regions are 0).
 *   excl_*       as in xck_config: indices into the NEW regions and the handle's SNP order.
 *   cell_enabled [n_cells of the handle], one byte per cell, or NULL = all; read only when struct_size covers the field (a caller built
 *                against the header without it passes the shorter struct and gets every cell, as before).  The call then returns, bit for
 *                bit, what a fresh handle returns that was fed the same reads with cell = -1 for every disabled cell, under the same
 *                tables and filters: the disabled cells' molecules are gone from the matrices AND from the pseudo-bulk tallies that
 *                min_count / min_maf are decided on, so a SNP may pass that failed over all cells, and the other way round.  Column
 *                indices stay the handle's own; a disabled cell simply has no entries.  The mask belongs to the call, as snp_enabled
 *                does: a later xck_refold without one answers for all cells again (the handle's own tallies are kept beside the masked
 *                ones).  xck_get_feature_summary's SNP table (a / c / g / t / n, kept) follows the tallies the last refold counted
 *                with; xck_snp_counts keeps answering for every cell; xck_group_counts with XCK_GROUP_SRC_RESULT sums what the call
 *                left.  A mask that enables every cell takes the same path as NULL; one that enables none gives XCK_OK and three
 *                empty matrices.  The basefc half of a XCK_MODE_BOTH handle is not recounted (its matrix under a cell subset is a
 *                column selection).
 * Valid on a handle with a BAF pipeline (XCK_MODE_BAF, or the BAF half of XCK_MODE_BOTH, whose out->count is the last finish's,
 * untouched), between a successful xck_finish and the next xck_reset, as often as wanted.  Pointers handed out by an earlier
 * xck_finish / xck_refold / xck_get_result_device die with the call, as at a second finish.  The handle's n_regions, filters and
 * tables follow the call, and xck_get_cell_summary / xck_get_feature_summary recompute their matrix halves, the kept and regions
 * columns of the SNP table included; the read-side counters do not change.
 * XCK_E_STATE before a finish, after a reset, on a decode-only handle, or when a fold of the handle has failed; XCK_E_ARG for a
 * basefc-only handle, a struct_size below XCK_REFOLD_CONFIG_SIZE_V1, an SNP list whose positions differ, exclusion pairs outside the tables, or too many
 * regions - the handle is then as it was.  A call that fails inside the fold leaves the handle failed, like a finish: xck_reset. */
typedef struct xck_refold_config {
    uint32_t struct_size;       /* sizeof(xck_refold_config); >= XCK_REFOLD_CONFIG_SIZE_V1   */
    int32_t  n_regions;
    const xck_region* regions;
    int32_t  n_snps;
    const xck_snp* snps;
    const uint8_t* snp_enabled;
    double   min_count, min_maf;
    int32_t  no_dup_hap;
    int32_t  n_excl_pairs;
    const int32_t* excl_region;
    const int32_t* excl_snp;
    const uint8_t* cell_enabled;   /* appended: everything above is the struct of the first header that had xck_refold */
} xck_refold_config;
#define XCK_REFOLD_CONFIG_SIZE_V1 ((uint32_t)offsetof(xck_refold_config, cell_enabled))   /* the struct without cell_enabled: still accepted */
int  xck_refold(xck_engine* e, const xck_refold_config* cfg, xck_result* out);
/* The SNP x cell matrices of the finished pileup (additive, as xck_refold is: ABI 3 is unchanged; a caller built against an older header
 * of ABI 3 does not see the symbol and loses nothing): out->ad / dp / oth with row = index of the SNP in the
 * list given to xck_create, col = cell, sorted by (row, col); out->count is empty.  Counted from what xck_finish keeps of the molecule
 * stage - the hits sorted by (SNP, cell, UMI) and the base every molecule shows under the handle's rule (its first read's, or the vote of XCK_F_UMI_CONSENSUS, under which no gap record claims) - without the reads, without a region
 * table and without a sort.  Per (SNP, cell): AD = molecules that show the SNP's ALT, DP = molecules that show REF or ALT (ALT wins when
 * REF == ALT), OTH = molecules that show another base; zero values are not emitted; a molecule that a gap record claims (an N / D
 * gap over the SNP earlier in fetch order) counts nowhere.  These are the matrices of a handle made with one one-base region per SNP,
 * REF on haplotype 0, ALT on haplotype 1, min_count 1, min_maf 0.  Every SNP of the handle's table and every cell counts, whatever snp_enabled or cell_enabled mask,
 * regions, exclusion pairs, haplotype indices, filters or no_dup_hap the handle or its last xck_refold carry; REF / ALT are the
 * handle's current ones (an xck_refold with other alleles is followed).
 * Valid where xck_refold is: on a handle with a BAF pipeline (a XCK_MODE_BOTH handle answers from it), between a successful
 * xck_finish and the next xck_reset, as often as wanted.  The call uses buffers of its own: it leaves the handle's tables and
 * results alone and does not invalidate what xck_finish / xck_refold / xck_get_result_device handed out, and a later xck_refold
 * does not invalidate its blocks, which are valid until the next xck_snp_counts, xck_reset or xck_destroy.
 * XCK_E_STATE before a finish, after a reset, on a decode-only handle, or when a fold of the handle has failed; XCK_E_ARG for a
 * basefc-only handle or a null out; XCK_E_CAPACITY when the sorted stream holds 2^32 hits or more (the call counts in 32 bits;
 * the split pileup fold has the same limit).  A handle without hits gives XCK_OK and three empty matrices.  An error leaves the handle as it
 * was: a failure inside the call (no memory for its own buffers) does not mark the handle failed. */
int  xck_snp_counts(xck_engine* e, xck_result* out);
/* Pseudo-bulk matrices per cell group (additive: ABI 3 is unchanged): the matrices the handle holds in device memory, with their columns
 * summed per group of cells under the mapping cell_group[n_cells of the handle] -> 0 .. n_groups - 1, or -1 = the cell is left out.
 *   Values    out->count / ad / dp / oth are COO with row = the source's row (a region in the handle's current order, a SNP in the
 *             caller's order) and col = group, sorted by (row, col), without zero entries.  Every value is exactly the sum, over the
 *             cells mapped to that group, of the source's values in that row.
 *   Filters   nothing is filtered again: the per-SNP filters, exclusions and no_dup_hap are those the source matrices were counted
 *             under; a group's AD / DP is the sum of its cells' AD / DP.
 *   Empty     a group without cells, and a row whose cells are all left out, produce no entries; all cells at -1, or a handle without
 *             hits, give XCK_OK and empty matrices.
 *   XCK_GROUP_SRC_RESULT   the matrices of the last xck_finish or xck_refold (after a refold: the refolded ones): a basefc handle fills
 *             count, a BAF handle ad / dp / oth, a XCK_MODE_BOTH handle all four (its count is the last finish's).
 *   XCK_GROUP_SRC_SNP      the blocks of the last xck_snp_counts since the last finish or reset: ad / dp / oth, count stays empty.
 * Valid between a successful xck_finish and the next xck_reset, as often as wanted.  The call uses buffers of its own (grow-only, freed
 * at xck_destroy): it invalidates nothing that xck_finish, xck_refold, xck_snp_counts or xck_get_result_device handed out, and none of
 * those invalidates its blocks, which live until the next xck_group_counts, xck_reset or xck_destroy.  A failure inside the call does
 * not mark the handle failed.
 * XCK_E_STATE before a finish, after a reset, on a decode-only handle, after a failed fold, or for source SNP when no xck_snp_counts
 * has run since the last finish or reset.  XCK_E_ARG for null pointers, a short struct_size, an unknown source, source SNP on a
 * basefc-only handle, n_groups outside 1 .. XCK_GROUP_MAX, or a cell_group entry outside -1 .. n_groups - 1: all found before the device
 * is touched, the handle stays as it was.  XCK_E_CAPACITY when a sum does not fit int32 (found, never wrapped) or a source matrix
 * holds 2^32 entries or more.  XCK_DEBUG_TIMING prints one `[xck] group_counts:` line. */
#define XCK_GROUP_SRC_RESULT 0   /* the matrices the handle holds now: last xck_finish or xck_refold */
#define XCK_GROUP_SRC_SNP    1   /* the blocks of the last xck_snp_counts */
#define XCK_GROUP_MAX     4096
typedef struct xck_group_config {
    uint32_t struct_size;       /* sizeof(xck_group_config)                                  */
    int32_t  source;            /* XCK_GROUP_SRC_*                                           */
    int32_t  n_groups;          /* 1 .. XCK_GROUP_MAX                                        */
    const int32_t* cell_group;  /* [n_cells of the handle]: group of every cell, or -1 = the cell is left out */
} xck_group_config;
int  xck_group_counts(xck_engine* e, const xck_group_config* cfg, xck_result* out);
/* Forget all pushed reads, keep tables and buffers (lets one engine be re-used per step). */
int  xck_reset(xck_engine* e);
int  xck_get_stats(const xck_engine* e, xck_stats* out);
/* The decoder's counters (xck_decode_stats; set out->struct_size first).  Works on decode-only handles too. */
int  xck_get_decode_stats(const xck_engine* e, xck_decode_stats* out);
/* The read assignment summary of one pipeline (set out->struct_size first): mode = XCK_MODE_BASEFC or XCK_MODE_BAF names it - the
 * handle's own mode, or either one on a XCK_MODE_BOTH handle, whose two pipelines keep their own counters (a contig may have
 * regions and no SNPs).  Waits for the handle's queued work as xck_flush does.  XCK_E_STATE on a handle made without
 * XCK_F_READ_FATE (XCK_F_CELL_SUMMARY implies it), XCK_E_ARG for a pipeline the handle does not have.  With contigs cut over several GPUs (xck_ingest_opts.tid_beg)
 * the reads that straddle a cut are seen by both neighbours, and no_target is relative to the regions of the handle that saw the read. */
int  xck_get_read_fate(xck_engine* e, int mode, xck_read_fate* out);
/* The per-cell table of one pipeline (set out->struct_size first); mode as for xck_get_read_fate.  Waits for the handle's queued work as
 * xck_flush does; after xck_finish the first call also runs the small kernel of the matrix columns.  XCK_E_STATE on a handle made
 * without XCK_F_CELL_SUMMARY, XCK_E_ARG for a pipeline the handle does not have or a short struct_size.  The caveat about cut contigs
 * of xck_get_read_fate holds per cell. */
int  xck_get_cell_summary(xck_engine* e, int mode, xck_cell_summary* out);
/* The per-feature / per-SNP tables of one pipeline (set out->struct_size first); mode as for xck_get_read_fate.  Waits for the handle's
 * queued work as xck_flush does; after xck_finish the first call also runs the small kernels of the matrix rows and the SNP verdicts, and
 * later calls return the same numbers.  XCK_E_STATE on a handle made without XCK_F_FEATURE_SUMMARY, XCK_E_ARG for a pipeline the handle
 * does not have or a short struct_size.  With contigs cut over several GPUs every handle counts the regions it was given; the SNPs
 * near a cut are seen by both neighbours. */
int  xck_get_feature_summary(xck_engine* e, int mode, xck_feature_summary* out);
/* The agreement counters of the handle's pileup pipeline (set out->struct_size first), as the molecule stage of the last xck_finish
 * counted them; xck_refold, xck_snp_counts and xck_group_counts do not change them, xck_reset clears them.  XCK_E_STATE on a handle
 * without XCK_F_UMI_CONSENSUS (and without XCK_UMI_CONSENSUS=1), before a successful xck_finish, after an xck_reset, or when a fold of
 * the handle has failed; XCK_E_ARG for a null pointer or a short struct_size.  With contigs cut over several GPUs every handle counts
 * the molecules of the reads it saw; a molecule whose reads straddle a cut is counted by both neighbours. */
int  xck_get_molecule_stats(xck_engine* e, xck_molecule_stats* out);
/* The counters of the unique-feature rule of the handle's basefc pipeline (set out->struct_size first), as the last xck_finish counted
 * them; xck_group_counts does not change them, xck_reset clears them.  XCK_E_STATE on a handle without XCK_F_UNIQUE_FEATURE (and
 * without XCK_UMI_FEATURE=unique), before a successful xck_finish, after an xck_reset, or when a fold of the handle has failed;
 * XCK_E_ARG for a null pointer or a short struct_size.  A run sharded by whole contigs sums its handles' counters to the one-GPU run's;
 * a molecule of a contig cut over several GPUs would be judged by each on its own part, which is why the front-ends refuse such a plan. */
int  xck_get_umi_feature_stats(xck_engine* e, xck_umi_feature_stats* out);
/* The counters of the 1-mismatch UMI collapsing of the handle's basefc pipeline (set out->struct_size first), as the last xck_finish
 * counted them; xck_group_counts does not change them, xck_reset clears them.  XCK_E_STATE on a handle without XCK_F_UMI_COLLAPSE (and
 * without XCK_UMI_DEDUP=1mm_all), before a successful xck_finish, after an xck_reset, or when a fold of the handle has failed; XCK_E_ARG
 * for a null pointer or a short struct_size.  The handles of a multi-GPU run own disjoint rows, a group never spans two of them, and
 * their counters add up to the one-GPU run's (max_group: the largest). */
int  xck_get_umi_dedup_stats(xck_engine* e, xck_umi_dedup_stats* out);
/* The pair counters of the handle's base-quality floor (set out->struct_size first).  Waits for the handle's queued work as xck_flush
 * does; xck_reset clears them, xck_finish and the derived calls do not change them.  A tile the join replays after an overflow counts
 * once.  XCK_E_STATE on a handle without a floor (and on a decode-only handle), XCK_E_ARG for a null pointer or a short struct_size. */
int  xck_get_baseq_stats(xck_engine* e, xck_baseq_stats* out);

/* -- pseudo-bulk base tallies (XCK_F_BASE_TALLY) -- */
/* The contigs' lengths, which bound the tables: n must equal the handle's n_contigs and every length lie in 1 .. 2^31 - 1 (XCK_E_ARG).
 * XCK_E_STATE on a handle without the flag and after the first push since xck_create / xck_reset; a push or an ingest on a tally handle
 * without lengths is XCK_E_STATE.  xck_reset keeps the lengths and zeroes the tables. */
int  xck_set_contig_lengths(xck_engine* e, const int64_t* len, int32_t n);
/* Copies the n * 4 counters (A C G T per position) of positions [pos0, pos0 + n) of a contig to out, after waiting for the queued work as
 * xck_flush does.  A contig no read touched reads as zeros.  XCK_E_ARG for a range outside the contig, XCK_E_STATE without the flag. */
int  xck_get_base_tally(xck_engine* e, int32_t contig, int32_t pos0, int32_t n, uint32_t* out);
/* The pass's counters since the last reset (set out->struct_size first); waits as xck_flush does.  XCK_E_STATE without the flag. */
int  xck_get_base_tally_stats(xck_engine* e, xck_base_tally_stats* out);
/* The candidate positions of every allocated table under cfg's thresholds: a count pass, a scan and an emit pass on the device.  Valid
 * between a successful xck_finish and the next xck_reset (XCK_E_STATE otherwise, and without the flag); may be called repeatedly with
 * other thresholds.  The arrays belong to the handle and are valid until the next xck_find_candidates / xck_reset / xck_destroy. */
int  xck_find_candidates(xck_engine* e, const xck_candidate_config* cfg, xck_candidates* out);

/* -- the genome's sequence on a tally handle (ref_seq.h; additive, ABI 3 is unchanged) -------- */
/* The sequence of one contig, packed on the device to 4 bits a position (BAM's codes =ACMGRSVTWYHKDBN; 0.5 byte a position).  raw is the
 * FASTA file's bytes from the contig's first base through its last one, line ends included; line_bases / line_width are the .fai's:
 * position p lies at raw[(p / line_bases) * line_width + p % line_bases].  Lower case reads as upper case; every byte that is not one of
 * the 15 letters (`=`, `*`, `-`, digits, ...) reads as N.  The bytes are staged in chunks of XCK_REF_CHUNK_BYTES (read at xck_create,
 * default 32 MiB, at least 64).  A byte below 33 where the geometry says a base must be - a stale index - fails the call with XCK_E_ARG
 * ("the FASTA line geometry does not match its index") and drops the contig's sequence.  XCK_E_STATE on a handle without
 * XCK_F_BASE_TALLY and before xck_set_contig_lengths; XCK_E_ARG for a contig out of range, line_bases < 1, line_width < line_bases and
 * n_raw smaller than the offset of the contig's last position + 1; XCK_E_NOMEM names the contig.  Valid before or after pushes and
 * xck_finish (it waits for the queued work); the sequence survives xck_reset, a second call for the contig replaces it, lengths that
 * xck_set_contig_lengths changes drop it, xck_destroy frees it. */
int  xck_set_contig_ref(xck_engine* e, int32_t contig, const char* raw, int64_t n_raw, int32_t line_bases, int32_t line_width);
/* The upper-case letters of positions [pos0, pos0 + n) of a contig's packed sequence (no terminator; tests and debugging).  The range
 * checks of xck_get_base_tally; XCK_E_STATE for a contig without a sequence. */
int  xck_get_contig_ref(xck_engine* e, int32_t contig, int32_t pos0, int32_t n, char* out);
/* has_table[c] = 1 for every contig whose table exists (a batch of it has been queued), else 0; n must be the handle's n_contigs. */
int  xck_get_base_tally_contigs(xck_engine* e, uint8_t* has_table, int32_t n);
/* xck_find_candidates oriented by the genome: with g the code of the position's base in the packed sequence,
 *   g not A, C, G or T (N, IUPAC, no sequence loaded for the contig): never written; counts under ref_unknown when xck_find_candidates'
 *     rule would have written it;
 *   otherwise ref = g, alt = the base other than ref with the largest count (the earliest of equals in A, C, G, T), m = min(c[ref],
 *     c[alt]); a candidate when m > 0, !((double)n < min_count) and !((double)m < (double)n * min_maf).  A written candidate counts
 *     under ref_major when ref is the base xck_find_candidates would have written as ref, else under ref_minor; a position that
 *     xck_find_candidates' rule accepts and this one rejects counts under ref_unsupported.
 * ref_major + ref_minor = out->n, and the four together = the n of xck_find_candidates under the same thresholds.  States, arrays and
 * positions_covered as xck_find_candidates; the lists of the two calls replace each other.  Set st->struct_size first. */
typedef struct xck_candidate_ref_stats {
    uint32_t struct_size;
    uint32_t reserved;
    int64_t  ref_major;
    int64_t  ref_minor;
    int64_t  ref_unsupported;
    int64_t  ref_unknown;
} xck_candidate_ref_stats;
int  xck_find_candidates_ref(xck_engine* e, const xck_candidate_config* cfg, xck_candidates* out, xck_candidate_ref_stats* st);

/* -- host ingest (replaces pysam.AlignmentFile + fetch(): own BGZF/BAM reader) --------------- */
/* n_threads = 0: the process's CPU share (affinity and cgroup quota; 1.5 threads per CPU behind a quota).  BAM only: CRAM / SAM text
 * are named in `err`.  On a multi-socket host the reader binds its threads - and, from the first xck_ingest_bam / xck_bam_next_batch
 * call until xck_bam_close, the CALLING thread - to the NUMA node of the engine's GPU (XCK_NUMA=0 in the environment turns that off). */
int  xck_bam_open(const char* path, int n_threads, xck_bam** out, char* err, size_t errlen);
void xck_bam_close(xck_bam* b);
int  xck_bam_n_refs(const xck_bam* b);
const char* xck_bam_ref_name(const xck_bam* b, int tid);
int64_t     xck_bam_ref_len(const xck_bam* b, int tid);
/* records per reference from the .bai next to the file (XCK_E_IO if there is no usable index);
 * used to balance contigs over GPUs */
int  xck_bam_ref_records(xck_bam* b, int tid, int64_t* n_mapped, int64_t* n_unmapped);
/* the .bai linear index of one reference: virtual offset of the first record overlapping every 16 kb window (SAMv1 5.1.3);
 * *n = 0 when the index has none.  The array belongs to the reader.  The compressed-byte distance between two windows
 * weighs the reads between them: used to cut an over-weight contig into position windows of equal work. */
int  xck_bam_linear_index(xck_bam* b, int tid, int64_t* n, const uint64_t** voffsets);

typedef struct xck_ingest_opts {
    uint32_t struct_size;
    int32_t  sample;            /* index of this BAM in the BAM list (ordinal high bits; column
                                   index in well mode)                                       */
    const int32_t* tid_to_contig; /* [n_refs] engine contig id per BAM tid, -1 = not used    */
    int32_t  use_index;         /* 1: decode only the virtual-offset ranges of the wanted tids
                                   (needs PATH.bai; silently decodes everything if absent)   */
    int64_t  max_records;       /* stop after this many records (0 = all)                    */
    int64_t  pause_records;     /* xck_ingest_bam only: return 1 ("paused") after the decode chunk in
                                   which at least this many further records were pushed by THIS call;
                                   the reader keeps its position and the next call continues
                                   (0 = run to the end of the file).  Read only when struct_size covers it. */
    /* Position windows (multi-GPU: ONE over-weight contig split at region boundaries): for BAM tid t only the
     * records from the first one that overlaps 0-based position tid_beg[t] (found through the .bai linear index; use_index = 1)
     * up to the last one that STARTS before tid_end[t] are decoded; records that start earlier but reach into the window are
     * included, so neighbouring windows share the reads that straddle the cut.  NULL = whole references.  tid_end[t] <= 0 =
     * no upper bound.  Read only when struct_size covers them. */
    const int32_t* tid_beg;
    const int32_t* tid_end;
} xck_ingest_opts;

/* Decode the BAM with the engine's decoder settings and push every batch; returns the number
 * of records decoded so far (over all calls on this reader) through *n_records.
 * Returns 0 at the end of the file, 1 when paused by pause_records, <0 on error. */
int  xck_ingest_bam(xck_engine* e, xck_bam* b, const xck_ingest_opts* o, int64_t* n_records);
/* Read ahead: the reader's threads start on the first chunks of the file (scanner, inflate - on the host pool or the GPU) and the call
 * returns at once; a later xck_ingest_bam / xck_bam_next_batch with the SAME options (which must stay valid until then) continues from
 * there.  For callers that count many small files one after the other (a plate of per-cell BAMs, the reference's
 * `for sam_fn in sam_fn_list` loops, rdr/fc/core.py:73-76): prefetch file k + 1 before ingesting file k, and the first inflate of the
 * next file overlaps the parse and the joins of this one.  Nothing of the engine is touched.  Returns 0, or <0 on error. */
int  xck_bam_prefetch(xck_engine* e, xck_bam* b, const xck_ingest_opts* o);
/* Pull-style decoding for tests / other consumers: fills *out with the next batch (arrays are
 * owned by the xck_bam and valid until the next call); returns 1 if a batch was produced,
 * 0 at end of file, <0 on error. */
int  xck_bam_next_batch(xck_engine* e, xck_bam* b, const xck_ingest_opts* o, xck_batch* out);

/* -- phased-SNP lists (fast path of load_snp_from_tsv / load_snp_from_vcf, baf/fc/utils.py:51-110, :114-193) --- */
/* The accepted SNPs of a TSV (header line, then chrom pos ref alt ref_hap alt_hap) or a phased VCF (first sample,
 * GT exactly 0|1, 1|0, 0/1, 1/0; single-base REF/ALT in ACGTN, upper-cased), in file order, chrom without a leading
 * "chr".  gzip / bgzip input is read through zlib.  Returns 0, or 1 when the file is outside what this parser
 * reproduces exactly (non-ASCII bytes, carriage returns, a position that is not plain decimal digits): the caller then
 * uses its generic loader.  <0 on I/O errors. */
typedef struct xck_snp_text {
    int64_t n;
    const int32_t* chrom_id;        /* [n] index into chroms[]                               */
    const int64_t* pos;             /* [n] 1-based                                           */
    const char*    ref;             /* [n]                                                   */
    const char*    alt;             /* [n]                                                   */
    const int8_t*  ref_hap;         /* [n] 0 / 1                                             */
    const int8_t*  alt_hap;         /* [n]                                                   */
    int32_t n_chroms;
    const char* const* chroms;      /* in order of first appearance                          */
    int64_t n_rejected;             /* lines the loaders warn about in verbose mode ...      */
    const int64_t* rej_line;        /* [n_rejected] 1-based line numbers, ascending          */
    const int8_t*  rej_code;        /* [n_rejected] XCK_SNP_REJ_*: the first check that failed */
} xck_snp_text;
#define XCK_SNP_REJ_COLUMNS     1   /* too few columns                                        */
#define XCK_SNP_REJ_REF         2   /* invalid REF base                                       */
#define XCK_SNP_REJ_ALT         3   /* invalid ALT base                                       */
#define XCK_SNP_REJ_NO_GT       4   /* VCF: no GT in FORMAT                                   */
#define XCK_SNP_REJ_FORMAT_LEN  5   /* VCF: FORMAT and sample column differ in length         */
#define XCK_SNP_REJ_DELIMITER   6   /* VCF: GT without | or /                                 */
#define XCK_SNP_REJ_GT          7   /* genotype is not 0|1 / 1|0 (0/1, 1/0)                   */
int  xck_parse_snp_text(const char* path, int is_vcf, xck_snp_text** out);
void xck_free_snp_text(xck_snp_text* t);

/* -- region-wise local phasing (replaces reg_local_phasing / snp_local_phasing, baf/fc/phasing.py:13-78, baf/localphase.py:14-343) -- */
/* Additive, ABI 3 is unchanged.  A stateless call: it needs no engine handle, allocates its own device buffers on `device` and frees them
 * before it returns.  It restates, in fp64 HIP (csrc/local_phase.hip), what xcltk_amd/baf/fc/phasing.py and xcltk_amd/baf/localphase.py
 * do on the host, region after region: the SNP and cell masks, the entry orientation of AD (ref_hap == 1 swaps AD with DP - AD), the rounds
 * of BAF filter (cells with 0.45 <= BAF <= 0.55 leave, for good) + two-haplotype EM with Gaussian smoothing (width 20000) + XOR of the
 * round's flip, and the majority rule.  The flips of a region's kept SNPs are applied to ref_hap / alt_hap (x -> 1 - x) before a later
 * region that shares a SNP reads them: regions are levelled on the host (level 0: shares no SNP with an earlier region; otherwise 1 + the
 * highest level among the earlier regions it shares a SNP with) and every level is one launch.  All sums run in a fixed order and no
 * floating-point atomic is used: the same problem gives the same bytes on every run and every device.
 *   pileup   cell x SNP counts as CSC by pileup column: col_ptr[n_cols + 1] (col_ptr[0] = 0, not decreasing), and per entry cell (strictly
 *            ascending inside a column), ad, dp with 0 <= ad <= dp.  An entry with dp = 0 counts as absent.
 *   cell_enabled   [n_cells] or NULL = all: a disabled cell is not seen at all (the --refcell subset).
 *   ref_hap / alt_hap   [n_snps], 0 / 1: the haplotype state at entry.
 *   regions  a CSR of slots, reg_ptr[n_regions + 1]; slot s pairs the pileup column slot_col[s] (or -1: the slot has no column and is never
 *            kept) with the SNP slot_snp[s] of the phased list, at position slot_pos[s] for the smoothing.  The slots of one region name
 *            distinct SNPs.  Regions are phased in the order given.
 * Result (library-owned host memory, until xck_free_phase_result): kept[s] = 1 when slot s has depth in the enabled cells (0: the (region,
 * SNP) pair leaves the region's list), flip[s] = 1 when the region flipped that SNP (after the majority rule; 0 for slots not kept and for
 * failed regions), status[r] = XCK_PHASE_PHASED or XCK_PHASE_FAILED (no informative cell left: nothing was flipped), the final ref_hap /
 * alt_hap, the number of levels (= launches), and host-measured milliseconds per stage.
 * XCK_E_ARG: null pointers, a short struct_size, pointers that run backwards, indices outside the tables, cells not strictly ascending
 * in a column, ad outside [0, dp], a haplotype index other than 0 / 1, a SNP twice in one region - all found before the device is touched.
 * XCK_E_DEVICE / XCK_E_NOMEM as elsewhere.  Nothing is returned on error (*out = NULL; xck_last_error(NULL) has the text). */
#define XCK_PHASE_FAILED 0
#define XCK_PHASE_PHASED 1
typedef struct xck_phase_problem {
    uint32_t struct_size;       /* sizeof(xck_phase_problem)                                 */
    int32_t  device;            /* HIP device ordinal                                        */
    int32_t  n_cells;
    int32_t  n_cols;
    const int64_t* col_ptr;     /* [n_cols + 1]                                              */
    const int32_t* cell;        /* [col_ptr[n_cols]]                                         */
    const int32_t* ad;
    const int32_t* dp;
    const uint8_t* cell_enabled;/* [n_cells] or NULL                                         */
    int32_t  n_snps;
    int32_t  n_regions;
    const int8_t*  ref_hap;     /* [n_snps]                                                  */
    const int8_t*  alt_hap;
    const int64_t* reg_ptr;     /* [n_regions + 1]                                           */
    const int32_t* slot_col;    /* [reg_ptr[n_regions]]                                      */
    const int32_t* slot_snp;
    const int64_t* slot_pos;
} xck_phase_problem;
typedef struct xck_phase_result {
    int64_t  n_slots;
    const uint8_t* kept;        /* [n_slots]                                                 */
    const uint8_t* flip;        /* [n_slots]                                                 */
    int32_t  n_regions;
    int32_t  n_snps;
    const uint8_t* status;      /* [n_regions] XCK_PHASE_*                                   */
    const int8_t*  ref_hap;     /* [n_snps]                                                  */
    const int8_t*  alt_hap;
    int32_t  n_levels;
    int32_t  n_blocks;          /* workgroups of the widest launch (each owns a scratch slice) */
    double   ms_prepare;        /* validation, levels, sizing (host)                         */
    double   ms_h2d;            /* allocation and copies to the device                       */
    double   ms_kernel;         /* all levels, launch to completion                          */
    double   ms_d2h;            /* copies back, frees                                        */
} xck_phase_result;
int  xck_local_phase(const xck_phase_problem* p, xck_phase_result** out);
void xck_free_phase_result(xck_phase_result* r);

/* -- output (replaces merge_mtx(), rdr/fc/utils.py:54-93) ------------------------------------ */
/* Write a MatrixMarket file byte-identical to the reference: header
 * "%%MatrixMarket matrix coordinate integer general\n%%\n{nrow}\t{ncol}\t{nnz}\n" then
 * "row\tcol\tval\n" lines (1-based).  row_map[r] gives the 1-based output row of region r
 * (0 = region not written). */
int  xck_write_mtx(const char* path, const xck_coo* m, const int32_t* row_map,
                   int32_t n_rows_out, int32_t n_cols);
/* The same file written by several processes (multi-GPU run on one node; no reference counterpart - its workers hand their
 * triplets to the parent, rdr/fc/main.py:232-262): every process owns some rows.  xck_mtx_part_size gives the bytes and lines
 * of the "row\tcol\tval\n" text of m (no header); after the sizes have been exchanged, xck_write_mtx_part writes that text at
 * byte `offset` of `path` (created if needed, never truncated).  The header line is the caller's. */
int  xck_mtx_part_size(const xck_coo* m, const int32_t* row_map, int64_t* n_bytes, int64_t* n_lines);
int  xck_write_mtx_part(const char* path, int64_t offset, const xck_coo* m, const int32_t* row_map);

#ifdef __cplusplus
}
#endif
#endif /* XCK_H */
