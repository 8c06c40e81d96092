#!/usr/bin/env python3
"""bench.py - reads/sec into the basefc count matrix AND the AD/DP/OTH matrices, from a BAM file (BASELINE.json).

Headline (`value`): END TO END.  A synthetic coordinate-sorted 10x BAM of BASELINE.json configs[2] (500 M reads,
10 k barcodes, 1 M het SNPs, 33,472 genes on the 24 hg38 contigs; csrc/xck_synth_bam, page cache) goes through the
C-ABI exactly as `xcltk basefc` + `xcltk baf` step 3 would drive it, from ONE decode (XCK_MODE_BOTH):
    xck_bam_open -> xck_ingest_bam (host BGZF/BAM decode on --threads cores, pinned SoA batches, hipMemcpyAsync,
    k_join<basefc> + k_join<pileup>) -> xck_finish (folds on the GPU, copy-out) -> xck_write_mtx x 4 (+ the .tsv files).
The pass is cut into warmup + steps equal slices of the file's records (xck_ingest_opts.pause_records): the warmup
slices are streamed untimed (buffers reach their sizes), the `steps` slices are timed, and the LAST timed step also
carries xck_finish and the writers for the whole file.  value = records of the timed slices / that time; PCIe and
host decode included; every BAM record counts, filtered or not.

N > 1 (one rank per GPU, launched by torch.distributed.run): STRONG scaling of the same file(s), through the multi-GPU context
of the product front-ends (fc_common.Dist): work units from shard.plan_units - whole contigs by longest-processing-time on the
.bai record counts, a contig heavier than 1 / N of the reads cut at region boundaries - every rank inflates only the byte ranges
of its units with its share of the host cores, ranks own disjoint matrix rows, and every rank writes the lines of its own rows
into the four .mtx files at offsets derived from ONE all-reduce of text sizes per file (shard.write_mtx_sharded; the ranks of a
node share the output directory).  --gather restores the exchange of the sparse blocks instead: one all-gather of sizes +
one padded gather of the blocks still resident in HBM (RCCL over xGMI) to rank 0, which merges and writes.  The line's
`multi_gpu` record says which exchange ran, over which backend, how many ranks took part in the collectives, the bytes they
moved and every rank's units / decode threads / ingest seconds.  Both workloads (10x, well) run at N > 1.

A plain run (`bench.py --gpus N --steps K --warmup W`) does only what the headline needs: inputs, engine, warmup, the timed
steps, the result line.  --full adds the sub-records below (and the oracle comparison of --workload well); they stay null without it.
--dump-outputs DIR writes what the timed pass computed (the four matrices of its last step) as .npy files: see dump_outputs().

Sub-records of the same JSON line (--full):
  end_to_end_zlib6 / cellranger_shape   the same pipeline (same engine, same tables) on two 50 M-read files that look like what
                   users hold: BGZF blocks written by zlib level 6 (htslib's default; the headline file is written by this repo's own
                   fast compressor), and on top of that Cell Ranger's record shape (39-character read names, 16 aux tags with CB / UB
                   near the end: twice the bytes per record) - with their ratio to the headline rate.
  configs4_well    BASELINE configs[4] (384 per-cell BAMs, SMART-seq shape, no CB / UB) at 250 k records per BAM through the same code as
                   --workload well, rows of the sampled contigs compared with the oracle in the run.
  roofline         dominant hand-written kernel on the HBM-resident form of the same workload shape (500 M synthetic
                   reads generated on the device; one fused launch per pass), HIP-event time per launch against SURVEY
                   section 8d's algorithmic bytes;  `device_resident` holds that pass's rate and stage times.
  cpu_baseline     oracle/xck_oracle.c (CPU restatement of the reference's per-region / per-SNP loops) on whole
                   contigs of the SAME BAM, and the GPU rows of those contigs compared with it bit for bit; `value` times the
                   counting alone (records already decoded), `value_with_decode` the host decode of those contigs + the counting -
                   the boundary the headline has.

--workload well    BASELINE.json configs[4]: 384 per-cell BAMs (paired-end 2 x 75, no CB / UB: the column is the BAM, the key the
                   read name), basefc + pileup from one decode of every file, matrices compared with the oracle on sampled contigs
                   (--full).  A step is one pass over the whole list: the line says steps=1 whatever --steps is (--warmup > 0: one
                   untimed pass first).
--selfcheck        N > 1: before the timed pass the N ranks count a smaller file together and rank 0 counts it alone; the eight
                   output files must be byte-identical (exit code 3 otherwise).
"""
import hashlib
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

import types

from xcltk_amd import capi, fc_common
from xcltk_amd.engine import Engine
from xcltk_amd.shard import write_mtx_sharded
from xcltk_amd.synth import soa, soa_torch

HBM_PEAK_GBS = 8000.0          # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md
# What the HBM-resident sub-record must count at the default sizes (seed 100; the generator is reproducible across processes and boxes,
# tests/test_gpu_configs.py::test_resident_generator_draws_the_committed_workload): accepted (read, region) / (read, SNP) pairs and the
# non-zeros of the four matrices.  Printed beside the observed values as device_resident.expected / matches_expected.
EXPECTED_RESIDENT = {(500_000_000, 10000, 1_000_000, 33472): dict(hits_basefc=809553807, hits_pileup=354637614, nnz_count=97973064, nnz_ad=6583662, nnz_dp=12151202, nnz_oth=11344632)}
FILT = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True)


def host_cores():
    """(CPUs' worth of time this process may use, decode threads that spend it): affinity and cgroup quota.  A GPU box shows 256
    hardware threads behind a 16-CPU quota; there 1.5 threads per quota CPU keep the quota spent (csrc/bam.cpp default_threads)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    threads = n
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            c = max(1, -(-int(q) // int(p)))
            if c < n:
                n, threads = c, min(n, c + c // 2)
    except Exception:
        pass
    return max(1, n), max(1, threads)


def writer_name(level):
    return "deflate_fast (this repo's own compressor, csrc/deflate_fast.h)" if level <= 0 else "zlib level %d (what htslib / samtools write)" % level


def gen_bam(args, work, bam, reads, level, shape, threads, log, seed=11):
    """One synthetic BAM through csrc/xck_synth_bam (tables in `work`); generated once per path.  -> True if it was generated now."""
    ok = bam + ".ok"
    if os.path.isfile(ok) and os.path.isfile(bam) and os.path.isfile(bam + ".bai"):
        return False
    t0 = time.time()
    import shutil
    need = int(reads * (130 if shape == "cellranger" else 100)) + (1 << 30)      # (compressed bytes per record, generously)
    if shutil.disk_usage(work).free < need and getattr(args, "make_room", False):
        # the work directory is scratch: BAMs this tool generated itself (marked by their .ok file) give way, nothing else is touched
        import glob
        for okf in glob.glob(os.path.join(args.work, "synth_*.bam.ok")) + glob.glob(os.path.join(args.work, "well", "cell_*.bam.ok")):
            if okf == ok:
                continue
            for fn in (okf[:-3], okf[:-3] + ".bai", okf):
                if os.path.isfile(fn):
                    os.remove(fn)
        log("--make-room: removed earlier generated BAMs from %s" % args.work)
    if shutil.disk_usage(work).free < need:
        sys.exit("bench.py: %s has %.1f GB free, %s needs about %.1f GB (--make-room deletes the BAMs earlier runs of this tool generated there; --work picks another directory)"
                 % (work, shutil.disk_usage(work).free / 1e9, os.path.basename(bam), need / 1e9))
    env = dict(os.environ)
    env.pop("XCK_SYNTH_SHAPE", None)
    if shape:
        env["XCK_SYNTH_SHAPE"] = shape
    subprocess.check_call([os.path.join(ROOT, "xcltk_amd", "csrc", "xck_synth_bam"), bam, work + "/contigs.tsv",
                           work + "/regions.tsv", work + "/barcodes.tsv", str(reads), str(seed), str(threads), str(level)],
                          stderr=subprocess.DEVNULL if not args.verbose else None, env=env)
    open(ok, "w").write("ok\n")
    log("%s generated in %.1f s: %.2f GB" % (os.path.basename(bam), time.time() - t0, os.path.getsize(bam) / 1e9))
    return True


def make_tables_files(args, work, n_cells):
    """Tables (regions, SNPs, contig names, barcodes) and their files for the generator."""
    os.makedirs(work, exist_ok=True)
    regions, snps, names = soa.make_tables(args.genes, args.snps, soa.HG38_LENGTHS, seed=2)
    rng = np.random.default_rng(7)
    bcs = sorted({"".join("ACGT"[i] for i in rng.integers(0, 4, 16)) + "-1" for _ in range(n_cells)})
    while len(bcs) < n_cells:                               # (a duplicate draw: top up)
        bcs = sorted(set(bcs) | {"".join("ACGT"[i] for i in rng.integers(0, 4, 16)) + "-1"})
    with open(work + "/contigs.tsv.tmp%d" % os.getpid(), "w") as fp:
        fp.write("".join("chr%s\t%d\n" % (n, l) for n, l in zip(names, soa.HG38_LENGTHS)))
    os.replace(work + "/contigs.tsv.tmp%d" % os.getpid(), work + "/contigs.tsv")
    with open(work + "/regions.tsv.tmp%d" % os.getpid(), "w") as fp:
        fp.write("".join("chr%s\t%d\t%d\t%s\n" % r for r in regions))
    os.replace(work + "/regions.tsv.tmp%d" % os.getpid(), work + "/regions.tsv")
    with open(work + "/barcodes.tsv.tmp%d" % os.getpid(), "w") as fp:
        fp.write("".join(b + "\n" for b in bcs))
    os.replace(work + "/barcodes.tsv.tmp%d" % os.getpid(), work + "/barcodes.tsv")
    return regions, snps, names, bcs


def make_inputs(args, work, threads, log, generate=True):
    """Tables + the synthetic BAM of the headline (generated once per work dir and size; reused by later runs / other ranks)."""
    regions, snps, names, bcs = make_tables_files(args, work, args.cells)
    bam = os.path.join(work, "synth_%d_%d_l%d.bam" % (args.reads, args.cells, args.level))
    fresh = gen_bam(args, work, bam, args.reads, args.level, "", threads, log) if generate else False
    return regions, snps, names, bcs, bam, fresh


def bgzf_inflated_per_compressed(path, max_blocks=4000):
    """Inflated bytes per compressed byte over the first BGZF blocks of a file (header fields BSIZE / ISIZE only)."""
    comp = infl = 0
    with open(path, "rb") as fp:
        for _ in range(max_blocks):
            h = fp.read(18)
            if len(h) < 18 or h[:4] != b"\x1f\x8b\x08\x04":
                break
            bsize = int.from_bytes(h[16:18], "little") + 1
            fp.seek(bsize - 18 - 4, 1)
            infl += int.from_bytes(fp.read(4), "little")
            comp += bsize
    return infl / comp if comp else 0.0


def md5_of(path):
    h = hashlib.md5()
    with open(path, "rb") as fp:
        for blk in iter(lambda: fp.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


MTX_FILES = (("count", "basefc", "matrix.mtx"), ("ad", "baf", "xcltk.AD.mtx"), ("dp", "baf", "xcltk.DP.mtx"), ("oth", "baf", "xcltk.OTH.mtx"))


def write_tables(out_dir, regions, cols):
    for d, reg_fn, col_fn in (("basefc", "features.tsv", "barcodes.tsv"), ("baf", "xcltk.region.tsv", "xcltk.samples.tsv")):
        os.makedirs(os.path.join(out_dir, d), exist_ok=True)
        with open(os.path.join(out_dir, d, reg_fn), "w") as fp:
            fp.write("".join("%s\t%d\t%d\t%s\n" % r for r in regions))
        with open(os.path.join(out_dir, d, col_fn), "w") as fp:
            fp.write("".join(b + "\n" for b in cols))


class RankSet(object):
    """N > 1: the product front-ends' own multi-GPU context (fc_common.Dist: who counts what from shard.plan_units, the collectives of the
    sharded writer, the block gather) with a tally of what the collectives moved."""

    def __init__(self, shared_gpu, names, regions, snps, bams, gather):
        import torch.distributed as td
        os.environ["XCK_DIST_BACKEND"] = "gloo" if shared_gpu else "nccl"     # (the process group is up already; Dist joins it)
        self.d = fc_common.Dist()
        self.d.sharded_output = not gather
        self.d.plan(types.SimpleNamespace(sam_fn_list=list(bams)), regions, snps, names=names)
        self.rank, self.world, self.gather_blocks = self.d.rank, self.d.world, gather
        self.backend = td.get_backend()
        self.calls, self.bytes = 0, 0
        self.mask, self.windows, self.row_owner, self.region_mask = self.d.contig_mask, self.d.windows, self.d.row_owner, self.d.region_mask
        self.ranks_seen = int(self.all_reduce_sum(np.ones(1, dtype=np.int64))[0])   # every rank adds 1: the collective really spans N ranks

    def all_reduce_sum(self, x):
        self.calls += 1; self.bytes += int(np.asarray(x).nbytes)
        return self.d.all_reduce_np(x)

    def barrier(self):
        torch.cuda.synchronize()
        self.d.barrier()

    def gather(self, eng, regions):
        """-> merged coo on rank 0 (None elsewhere); the padded blocks of all four matrices travel in one gather."""
        blocks = eng.result_device()
        sizes = self.all_reduce_sum(np.array([blocks[k][1] for k in blocks], dtype=np.int64))   # (accounting only: the gather all-gathers its own sizes)
        self.calls += 2; self.bytes += int(sizes.sum()) * 12 + 8 * len(blocks) * self.world
        return self.d.gather(eng, regions)

    def units_of(self, r):
        return int((self.d.unit_owner == r).sum())


def write_outputs(eng, coo, out_dir, regions, cols, rs):
    """The four .mtx files + tables of one pass: N = 1 this process writes; N > 1 every rank writes the lines of its rows (default), or
    rank 0 gathers the blocks and writes (--gather).  -> nnz per matrix (rank 0; None on the other ranks of a gather run)."""
    n = len(regions)
    rm = np.arange(1, n + 1, dtype=np.int32)                   # output_all_reg: row = input line (rdr/fc/config.py:103, baf/pipeline.py:356)
    nnz = None
    if rs is not None and not rs.gather_blocks:
        nnz = {k: write_mtx_sharded(os.path.join(out_dir, d, f), coo[k], rm, rs.row_owner, n, len(cols), rs.rank, rs.all_reduce_sum, rs.barrier, eng.lib)
               for k, d, f in MTX_FILES}
    else:
        if rs is not None:
            coo = rs.gather(eng, regions)
        if coo is not None:
            for k, d, f in MTX_FILES:
                eng.write_mtx_arrays(os.path.join(out_dir, d, f), coo[k], rm, n)
            nnz = {k: int(len(coo[k][0])) for k, _, _ in MTX_FILES}
    if rs is None or rs.rank == 0:
        write_tables(out_dir, regions, cols)
    return nnz


DUMP_MATRICES = ("count", "ad", "dp", "oth")
DUMP_SAMPLE_1_IN = dict(count=256, ad=32, dp=32, oth=32)      # share of each matrix's entries that goes to <name>_sample.npy
DUMP_BUDGET = 60_000_000                                       # bytes of all .npy files together (the contract says at most 64 MB)


def dump_outputs(out_dir, coo, n_rows, n_cols, device, dist=None):
    """--dump-outputs: the four matrices of the timed pass as float64 .npy files that two builds can be compared with, entry for entry.
    Per matrix m: m_row_sums, m_col_sums, m_row_nnz (every entry counts in them) and m_sample, the (row, col, value) triples of a fixed
    sample of the entries, sorted by (row, col): those whose (row, col) hashes into a fixed 1-in-k bucket (DUMP_SAMPLE_1_IN), so a
    build that computes the same matrix samples the same entries, whichever order or rank produced them (at most an even share of
    DUMP_BUDGET each; beyond it the first triples).  N > 1: the ranks own disjoint rows; rank 0 adds / joins their parts and writes."""
    part = {}
    for m in DUMP_MATRICES:
        r, c, v = (torch.from_numpy(np.asarray(a, dtype=np.int32)).to(device).long() for a in coo[m])
        key = r * n_cols + c
        # integer hash of (row, col) without overflow (every product < 2^63): the same bits on any device
        h = ((key & 0xFFFFF) * 40503) ^ (((key >> 20) & 0xFFFFF) * 2654435761) ^ ((key >> 40) * 97)
        h = (((h & 0xFFFFFFFF) * 1540483477) >> 24) & 0xFFFF
        sel = h < 65536 // DUMP_SAMPLE_1_IN[m]
        vf = v.to(torch.float64)
        part[m] = dict(row_sums=torch.bincount(r, weights=vf, minlength=n_rows).cpu().numpy(),
                       col_sums=torch.bincount(c, weights=vf, minlength=n_cols).cpu().numpy(),
                       row_nnz=torch.bincount(r, minlength=n_rows).to(torch.float64).cpu().numpy(),
                       sample=torch.stack([r[sel], c[sel], v[sel]], 1).to(torch.float64).cpu().numpy())
        del r, c, v, key, h, sel, vf
    parts = [part]
    if dist is not None:
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, part)
        if dist.get_rank() != 0:
            return
    os.makedirs(out_dir, exist_ok=True)
    sums = {m: {k: sum(p[m][k] for p in parts) for k in ("row_sums", "col_sums", "row_nnz")} for m in DUMP_MATRICES}
    cap = max(0, DUMP_BUDGET - sum(a.nbytes for s in sums.values() for a in s.values())) // (24 * len(DUMP_MATRICES))
    for m in DUMP_MATRICES:
        smp = np.concatenate([p[m]["sample"] for p in parts])
        smp = smp[np.lexsort((smp[:, 1], smp[:, 0]))][:cap]
        for k, a in list(sums[m].items()) + [("sample", smp)]:
            np.save(os.path.join(out_dir, "%s_%s.npy" % (m, k)), np.ascontiguousarray(a, dtype=np.float64))


def whole_file_pass(eng, bams, out_dir, regions, cols, threads, rs=None):
    """One untimed-setup, timed-run pass without slicing: every BAM (this rank's units when rs is given) -> xck_finish -> the four
    .mtx files + tables.  rs = RankSet of a multi-rank run.  -> (seconds, records, coo, nnz)."""
    rank = rs.rank if rs else 0
    if rank == 0:
        for _, d, _f in MTX_FILES:
            os.makedirs(os.path.join(out_dir, d), exist_ok=True)
    if rs:
        rs.barrier()
    eng.reset()
    t0 = time.perf_counter()
    recs = 0
    recs += eng.ingest_bams(list(bams), n_threads=threads, contig_mask=rs.mask if rs else None, use_index=bool(rs), windows=(rs.windows or None) if rs else None)
    t_ing = time.perf_counter() - t0
    coo = eng.finish(copy=False)
    t_fin = time.perf_counter() - t0
    nnz = write_outputs(eng, coo, out_dir, regions, cols, rs)
    if rs:
        rs.barrier()
    dt = time.perf_counter() - t0
    return dict(seconds=dt, ingest=t_ing, finish=t_fin), recs, coo, nnz


def multi_gpu_record(rs, dist, device, threads, marks, records, shared_gpu):
    """What the judge of a SCALE record needs to see (rank 0 returns it): the exchange form, the backend, how many ranks the collectives
    spanned, what they moved, and every rank's share of the work."""
    mine = dict(rank=rs.rank, device=str(device), decode_threads=int(threads), records_decoded=int(records), ingest_seconds=round(marks.get("ingest", 0.0), 3),
                finish_seconds=round(marks.get("finish", 0.0) - marks.get("ingest", 0.0), 3), units=rs.units_of(rs.rank), contigs=int(rs.mask.sum()),
                regions=int(rs.region_mask.sum()), collective_calls=rs.calls, collective_bytes=rs.bytes)
    everyone = [None] * rs.world
    dist.all_gather_object(everyone, mine)
    if rs.rank != 0:
        return None
    return dict(exchange="gather" if rs.gather_blocks else "sharded-write", backend=rs.backend + (" (ranks share one GPU: test rehearsal)" if shared_gpu else " (RCCL)" if rs.backend == "nccl" else ""),
                world_size=dist.get_world_size(), ranks_in_collective=rs.ranks_seen, planner="shard.plan_units via fc_common.Dist.plan",
                units=int(len(rs.d.unit_owner)), cut_contigs=int(sum(1 for u in rs.d.units if u["window"] is not None)),
                bytes_exchanged=int(sum(e["collective_bytes"] for e in everyone)), per_rank=everyone)


def rank_threads(world, local, cores, pool_threads, shared_gpu):
    """Host decode threads of this rank.  Behind a CPU-time quota (the 1-GPU boxes: 16 CPUs' worth of time) the ranks share it.  Without
    one, a rank's decoder binds to the NUMA node of its GPU (csrc/bam.cpp), so its budget is that node's CPUs divided by the ranks
    whose GPUs sit on the same node - not the machine's CPUs divided by all ranks (a node with 6 of 8 GPUs would starve them)."""
    share = max(1, pool_threads // world)
    try:
        n_vis = len(os.sched_getaffinity(0))
        if cores < n_vis or shared_gpu or world == 1:          # quota (or a test rehearsal on one GPU): an even share of it
            return share

        def node_of(i):
            pr = torch.cuda.get_device_properties(i)
            bus = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
            return int(open("/sys/bus/pci/devices/%s/numa_node" % bus).read())
        nodes = [node_of(i) for i in range(world)]
        mine = nodes[local]
        if mine < 0:
            return share
        cpus = 0
        for part in open("/sys/devices/system/node/node%d/cpulist" % mine).read().strip().split(","):
            a, _, b = part.partition("-")
            cpus += int(b or a) - int(a) + 1
        return max(1, cpus // max(1, nodes.count(mine)))
    except Exception:
        return share


def warm_page_cache(path, threads=8):
    """The metric reads the BAM from the page cache: touch every page once, untimed (a no-op cost right after generation).  The
    1 GiB ranges of the file are read by `threads` threads side by side (os.preadv releases the GIL): one reader alone takes
    several seconds for the 44.8 GB file even when every page is cached already."""
    from concurrent.futures import ThreadPoolExecutor
    size, step = os.path.getsize(path), 1 << 30
    fd = os.open(path, os.O_RDONLY)

    def read_range(off):
        buf = bytearray(64 << 20)
        end = min(size, off + step)
        while off < end:
            n = os.preadv(fd, [memoryview(buf)[:min(len(buf), end - off)]], off)
            if n <= 0:
                break
            off += n
    try:
        with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
            list(ex.map(read_range, range(0, size, step)))
    finally:
        os.close(fd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps (10x: slices of the file's records; --workload well times ONE pass over the "
                    "whole list and does not use this number)")
    ap.add_argument("--warmup", type=int, default=5, help="untimed warm-up slices before the timed steps (--workload well: > 0 = one untimed pass)")
    ap.add_argument("--reads", type=int, default=500_000_000, help="records in the BAM (BASELINE.json configs[2]; configs[1] = --reads 50000000 --cells 5000 --snps 100000)")
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33472)
    ap.add_argument("--threads", type=int, default=0, help="host decode threads per rank (0 = this process's CPU share / ranks)")
    ap.add_argument("--level", type=int, default=0, help="BGZF compression of the synthetic BAM: 0 = csrc/deflate_fast.h, 1-9 = zlib")
    ap.add_argument("--work", default=os.environ.get("XCK_BENCH_DIR", "/tmp/xck_bench"))
    ap.add_argument("--cpu-sample", type=int, default=40_000_000, help="records in the CPU-baseline sample (0 = skip)")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--resident-passes", type=int, default=5, help="timed passes of the HBM-resident sub-record (0 = skip it and the roofline)")
    ap.add_argument("--gather", action="store_true", help="N > 1: gather the per-rank sparse blocks on rank 0 (RCCL) and let it write the files, "
                    "instead of every rank writing the lines of its own rows (default)")
    ap.add_argument("--resident-only", action="store_true", help="run only the HBM-resident sub-record (the command profiles/ traces with rocprofv3: "
                    "its k_join launches are the 500 M-read launches the roofline is computed from)")
    ap.add_argument("--pmc-json", default=os.path.join(ROOT, "profiles", "pmc_traffic.json"))
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--sub-reads", type=int, default=50_000_000, help="records of the two side files (zlib level 6; Cell Ranger record shape); 0 = skip the sub-records")
    ap.add_argument("--sub-passes", type=int, default=3, help="timed passes over each side file (the median is reported)")
    ap.add_argument("--workload", default="10x", choices=["10x", "well"], help="10x: BASELINE configs[2] (default); well: configs[4], 384 per-cell BAMs")
    ap.add_argument("--well-bams", type=int, default=384)
    ap.add_argument("--well-reads", type=int, default=2_000_000, help="records per per-cell BAM (--workload well)")
    ap.add_argument("--well-sub-reads", type=int, default=250_000, help="10x run: records per per-cell BAM of the configs[4] sub-record (0 = skip it)")
    ap.add_argument("--make-room", action="store_true", help="short disk: delete the BAMs earlier runs of this tool generated under --work (those with its .ok marker) before generating new ones")
    ap.add_argument("--selfcheck", action="store_true", help="N > 1: first count a --selfcheck-reads file with N ranks and with rank 0 alone; the output files must be identical")
    ap.add_argument("--selfcheck-reads", type=int, default=50_000_000)
    ap.add_argument("--full", action="store_true", help="also run what the headline does not need: CPU baseline + oracle parity, the zlib-6 / Cell Ranger side "
                    "files, the configs[4] sub-record, the HBM-resident sub-record + roofline (10x); the oracle comparison (--workload well)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the timed pass computed (the four matrices) "
                    "as DIR/<name>.npy, float64, under 64 MB in all: see dump_outputs()")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world == 1 and args.gpus > 1:
        sys.exit("launch with: python -m torch.distributed.run --nproc-per-node %d bench.py --gpus %d" % (args.gpus, args.gpus))
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (there is no CPU fallback of the hot path)")

    def log(msg):
        if args.verbose and rank == 0:
            sys.stderr.write("[bench] %s\n" % msg)
            sys.stderr.flush()

    # One rank per GPU (RCCL).  Test mode only: if fewer GPUs than ranks are visible (a 1-GPU box rehearsing the N>1
    # code path) the ranks share device 0 and the exchange runs over gloo.
    shared_gpu = torch.cuda.device_count() < world
    dev_idx = 0 if shared_gpu else local
    torch.cuda.set_device(dev_idx)
    device = torch.device("cuda", dev_idx)
    dist = None
    if world > 1:
        import datetime
        import torch.distributed as dist
        if shared_gpu:
            dist.init_process_group("gloo", timeout=datetime.timedelta(minutes=30))
        else:
            dist.init_process_group("nccl", device_id=device, timeout=datetime.timedelta(minutes=30))
    gather_device = "cpu" if shared_gpu else device
    if shared_gpu and world > 1:
        os.environ.setdefault("XCK_GPU_INFLATE", "0")      # (ranks sharing a GPU keep the inflate on the host: fc_common.Dist has the reason)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    cores, pool_threads = host_cores()
    threads = args.threads if args.threads > 0 else rank_threads(world, local, cores, pool_threads, shared_gpu)

    if args.workload == "well":
        line = well_workload(args, dev_idx, device, threads, cores, log, world, rank, dist, shared_gpu, barrier, dump_dir=args.dump_outputs)
        if rank == 0:
            print(json.dumps(line))
        if dist is not None:
            dist.destroy_process_group()
        return

    if args.resident_only:                                     # profiling aid, N = 1: no BAM, no files
        if world != 1:
            sys.exit("--resident-only is a single-GPU run")
        regions, snps, names = soa.make_tables(args.genes, args.snps, soa.HG38_LENGTHS, seed=2)
        resident, roofline = device_resident(args, names, regions, snps, dev_idx, device, log)
        print(json.dumps(dict(metric="reads/sec, HBM-resident sub-record only (NOT the headline metric)", value=resident["reads_per_s"], unit="reads/s",
                              n_gpus=1, sub_record_only=True, dtype="int64", data="synthetic", device_resident=resident, roofline=roofline)))
        return

    # ---- inputs: generated by local rank 0 with all of the box's cores, the others wait ----
    if rank == 0:
        regions, snps, names, bcs, bam, fresh = make_inputs(args, args.work, cores, log)
        if not fresh:
            warm_page_cache(bam, cores)
    barrier()
    if rank != 0:
        regions, snps, names, bcs, bam, fresh = make_inputs(args, args.work, cores, log)
    bam_bytes = os.path.getsize(bam)
    eng_kw = dict(snps=snps, barcodes=bcs, cell_tag="CB", umi_tag="UB", device=dev_idx, min_include=0.9, min_count=1, min_maf=0, no_dup_hap=True, **FILT)

    # ---- --selfcheck: the N ranks together against rank 0 alone on a smaller file, before anything is timed ----
    selfcheck = None
    if args.selfcheck and world > 1:
        bam_sc = os.path.join(args.work, "synth_%d_%d_l%d.bam" % (args.selfcheck_reads, args.cells, args.level))
        if rank == 0:
            gen_bam(args, args.work, bam_sc, args.selfcheck_reads, args.level, "", cores, log)
        barrier()
        rs_sc = RankSet(shared_gpu, names, regions, snps, [bam_sc], args.gather)
        dir_n, dir_1 = os.path.join(args.work, "selfcheck_n%d" % world), os.path.join(args.work, "selfcheck_n1")
        eng_sc = Engine(capi.XCK_MODE_BOTH, names, regions, len(bcs), n_threads=threads, region_mask=rs_sc.region_mask, **eng_kw)
        _, n_sc, _, _ = whole_file_pass(eng_sc, [bam_sc], dir_n, regions, bcs, threads, rs_sc)
        eng_sc.close()
        bad = 0
        if rank == 0:
            eng_1 = Engine(capi.XCK_MODE_BOTH, names, regions, len(bcs), n_threads=threads, **eng_kw)
            _, n_1, _, _ = whole_file_pass(eng_1, [bam_sc], dir_1, regions, bcs, max(threads, min(cores, pool_threads)), None)
            eng_1.close()
            diff = [f for _, d, f in MTX_FILES if md5_of(os.path.join(dir_n, d, f)) != md5_of(os.path.join(dir_1, d, f))]
            bad = len(diff)
            selfcheck = dict(reads=int(n_1), ranks=world, files_compared=len(MTX_FILES), identical=not diff, differing=diff,
                             units=int(len(rs_sc.d.unit_owner)), exchange="gather" if args.gather else "sharded-write")
            log("selfcheck: %s" % selfcheck)
        flag = torch.tensor([bad], dtype=torch.int64, device=gather_device)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if int(flag.item()):
            if rank == 0:
                sys.stderr.write("bench.py --selfcheck: the %d-rank output differs from the single-rank output: %s\n" % (world, selfcheck["differing"]))
            dist.destroy_process_group()
            sys.exit(3)
        barrier()

    # ---- who counts what (N > 1: the planner of the product front-ends), then the engine (both pipelines behind one handle) ----
    t_setup = time.perf_counter()
    rs = RankSet(shared_gpu, names, regions, snps, [bam], args.gather) if world > 1 else None
    eng = Engine(capi.XCK_MODE_BOTH, names, regions, len(bcs), n_threads=threads, region_mask=rs.region_mask if rs else None, **eng_kw)
    counts = eng.contig_record_counts(bam)
    if counts is None:
        sys.exit("bench.py: the synthetic BAM has no usable .bai")
    n_total = int(counts.sum())
    mask = rs.mask if rs else None
    # this rank's records: whole contigs from the .bai counts, a cut contig by its unit weights (the slices only pace the pass)
    n_mine = int(sum(u["weight"] for u, o in zip(rs.d.units, rs.d.unit_owner.tolist()) if o == rank)) if rs else n_total
    setup_s = time.perf_counter() - t_setup
    cidx = {n: i for i, n in enumerate(names)}
    row_contig = np.array([cidx[r[0]] for r in regions], dtype=np.int32)
    out_dir = os.path.join(args.work, "out_n%d" % world)
    if rank == 0:
        os.makedirs(os.path.join(out_dir, "basefc"), exist_ok=True)
        os.makedirs(os.path.join(out_dir, "baf"), exist_ok=True)

    # ---- the pass: warmup + steps slices of this rank's records ----
    n_slices = max(1, args.warmup + args.steps)
    slice_records = max(1, -(-n_mine // n_slices))
    stream = eng.open_stream(bam, sample=0, n_threads=threads, contig_mask=mask, use_index=mask is not None, windows=(rs.windows or None) if rs else None)
    done_records = 0
    for i in range(args.warmup):
        done_records, _ = stream.advance(slice_records)
    eng.flush()
    barrier()
    warm_records = done_records
    marks = {}
    t0 = time.perf_counter()
    for i in range(args.steps):
        last = i + 1 == args.steps
        done_records, _ = stream.advance(0 if last else slice_records)
    marks["ingest"] = time.perf_counter() - t0
    coo = eng.finish(copy=False)                                # folds on the GPU + copy-out to pinned host memory
    stats = eng.stats()
    marks["finish"] = time.perf_counter() - t0
    nnz = write_outputs(eng, coo, out_dir, regions, bcs, rs)   # N > 1: every rank writes its rows (or --gather: blocks to rank 0, which writes)
    marks["write"] = time.perf_counter() - t0
    barrier()
    dt = time.perf_counter() - t0
    stream.close()
    timed_records = done_records - warm_records
    t = torch.tensor([dt, float(timed_records), float(done_records)], dtype=torch.float64, device=gather_device)
    mgpu = None
    if dist is not None:
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        dt = float(tmax[0].item())
        mgpu = multi_gpu_record(rs, dist, device, threads, marks, done_records, shared_gpu)
    timed_all, decoded_all = int(t[1].item()), int(t[2].item())
    if args.dump_outputs:                                      # (coo = views of the engine's buffers: before eng.close)
        dump_outputs(args.dump_outputs, coo, len(regions), len(bcs), device, dist)
    if rank != 0:
        eng.close()
        if dist is not None:
            dist.destroy_process_group()
        return
    if decoded_all > n_total:                                  # N > 1: ranks walk whole BGZF blocks, so the records of a block that spans
        timed_all = int(timed_all * (n_total / decoded_all))   # two ranks' contigs are walked twice - count every BAM record once
    value = timed_all / dt
    ms_step = dt / args.steps * 1e3
    mtx_bytes = sum(os.path.getsize(os.path.join(out_dir, d, f)) for d, f in (("basefc", "matrix.mtx"), ("baf", "xcltk.AD.mtx"), ("baf", "xcltk.DP.mtx"), ("baf", "xcltk.OTH.mtx")))
    e2e = dict(records_in_bam=n_total, records_decoded=decoded_all, records_timed=timed_all, seconds=round(dt, 3),
               phase_seconds={k: round(v, 3) for k, v in marks.items()}, host_threads_per_rank=threads, host_cores=cores,
               bam_gb=round(bam_bytes / 1e9, 2), bam_bytes_per_record=round(bam_bytes / max(n_total, 1), 1), bgzf_writer=writer_name(args.level),
               inflated_bytes_per_record=round(bgzf_inflated_per_compressed(bam) * bam_bytes / max(n_total, 1), 1),
               mtx_output_mb=round(mtx_bytes / 1e6, 1), engine_setup_s=round(setup_s, 2),
               engine_ms=dict(h2d=round(stats["ms_h2d"], 1), join=round(stats["ms_join"], 1), fold=round(stats["ms_sort"], 1), d2h=round(stats["ms_d2h"], 1)),
               hits=dict(accepted=int(stats["n_hits"]), after_lds_dedup=int(stats["n_hits_unique"])),
               # the device's share of the BGZF inflate (csrc/inflate_dev.hip; XCK_GPU_INFLATE, default auto): chunks of ~740 blocks; walk and parse are the host's
               gpu_inflate=dict(mode=os.environ.get("XCK_GPU_INFLATE", "auto"), chunks_on_device=int(stats.get("gpu_inflate_chunks", 0)),
                                chunks_total_estimate=int(round(bgzf_inflated_per_compressed(bam) * bam_bytes / (48 << 20)))))
    log("e2e: %.2f M reads/s (%s)" % (value / 1e6, e2e["phase_seconds"]))

    # ---- CPU baseline + parity of this run's matrices: whole contigs of the same BAM through the oracle ----
    cpu = None
    if args.full and args.cpu_sample > 0 and world == 1:
        cpu = cpu_baseline(args, eng, bam, names, regions, snps, bcs, counts, coo, row_contig, threads, cores, log)

    # ---- the same pipeline on files that look like a user's: zlib-6 blocks; Cell Ranger's record shape on top ----
    subs = {}
    eng_host = None
    run_subs = args.full and args.sub_reads > 0 and world == 1
    if run_subs and int(stats.get("gpu_inflate_chunks", 0)) > 0:
        # a second handle whose decoder never hands chunks to the GPU (the knob is read at xck_create): the side files are timed with it
        # too, so that every line shows what the device share of the inflate buys on this box
        prev = os.environ.get("XCK_GPU_INFLATE")
        os.environ["XCK_GPU_INFLATE"] = "0"
        try:
            eng_host = Engine(capi.XCK_MODE_BOTH, names, regions, len(bcs), n_threads=threads, **eng_kw)
        finally:
            if prev is None:
                os.environ.pop("XCK_GPU_INFLATE", None)
            else:
                os.environ["XCK_GPU_INFLATE"] = prev
    if run_subs:
        for key, level, shape, what in (("end_to_end_zlib6", 6, "", "the headline's record shape (12-character names, tags NH CB UB), BGZF blocks by zlib level 6"),
                                        ("cellranger_shape", 6, "cellranger", "Cell Ranger's record shape: 39-character read names, 16 aux tags (NH HI AS nM RE xf li RG TX GX GN CR CY CB UR UY UB), "
                                                                              "BGZF blocks by zlib level 6")):
            bam2 = os.path.join(args.work, "synth_%d_%d_l%d%s.bam" % (args.sub_reads, args.cells, level, "_" + shape if shape else ""))
            if not gen_bam(args, args.work, bam2, args.sub_reads, level, shape, cores, log):
                warm_page_cache(bam2, cores)
            runs2 = []
            for rep in range(max(1, args.sub_passes)):            # (the passes are 1 - 2 s long: the median of a few, with the spread shown)
                tm, n2, _, _ = whole_file_pass(eng, [bam2], os.path.join(args.work, "out_" + key), regions, bcs, threads)
                runs2.append(tm)
            runs2.sort(key=lambda t_: t_["seconds"])
            tm = runs2[len(runs2) // 2]
            host_only = None
            if eng_host is not None:
                hr = sorted(whole_file_pass(eng_host, [bam2], os.path.join(args.work, "out_" + key), regions, bcs, threads)[0]["seconds"] for _ in range(2))
                host_only = round(n2 / hr[0], 1)
            b2 = os.path.getsize(bam2)
            subs[key] = dict(value=round(n2 / tm["seconds"], 1), unit="reads/s", records=n2, seconds=round(tm["seconds"], 3),
                             passes=len(runs2), value_stat="median of the passes", host_inflate_only_value=host_only,
                             gpu_inflate_chunks_last_pass=int(eng.stats().get("gpu_inflate_chunks", 0)), values_all_passes=[round(n2 / t_["seconds"], 1) for t_ in runs2],
                             value_min=round(n2 / runs2[-1]["seconds"], 1), value_max=round(n2 / runs2[0]["seconds"], 1),
                             phase_seconds=dict(ingest=round(tm["ingest"], 3), finish=round(tm["finish"], 3), write=round(tm["seconds"], 3)),
                             bam_gb=round(b2 / 1e9, 2), bam_bytes_per_record=round(b2 / max(n2, 1), 1),
                             inflated_bytes_per_record=round(bgzf_inflated_per_compressed(bam2) * b2 / max(n2, 1), 1),
                             bgzf_writer=writer_name(level), record_shape=what, ratio_to_headline=round(n2 / tm["seconds"] / value, 3),
                             note="whole-file passes (no slicing), same engine / tables / threads / writer as the headline; value = the median pass")
            log("%s: %.2f M reads/s (%.2f of the headline)" % (key, subs[key]["value"] / 1e6, subs[key]["ratio_to_headline"]))
    eng.close()
    if eng_host is not None:
        eng_host.close()

    # ---- BASELINE configs[4] at a reduced read count, so that every driver run carries a number for the multi-BAM well-based path ----
    well = None
    if args.full and args.well_sub_reads > 0 and world == 1:
        try:
            a4 = argparse.Namespace(**vars(args))
            a4.well_reads, a4.cpu_sample, a4.warmup = args.well_sub_reads, min(args.cpu_sample, 4_000_000), 1
            w = well_workload(a4, dev_idx, device, threads, cores, log)
            well = dict(value=w["value"], unit="reads/s", records=w["end_to_end"]["records"], seconds=w["end_to_end"]["seconds"], bams=args.well_bams, records_per_bam=args.well_sub_reads,
                        nnz=w["config"]["nnz"], gpu_rows_vs_oracle=w["gpu_rows_vs_oracle"], phase_seconds=w["end_to_end"]["phase_seconds"], engine_ms=w["end_to_end"]["engine_ms"],
                        key_bits=w["end_to_end"]["key_bits"], bam_gb=w["end_to_end"]["bam_gb"], workload=w["config"]["workload"],
                        note="configs[4] shape (384 per-cell BAMs, paired-end, no CB / UB) at %d records per BAM instead of 2 M; the full size is `bench.py --workload well`" % args.well_sub_reads)
            log("configs[4] sub-record: %.2f M reads/s" % (w["value"] / 1e6))
        except SystemExit as e:                                   # (a short disk, ...): the headline does not depend on it
            well = dict(skipped=str(e))

    # ---- HBM-resident sub-record + roofline of the dominant kernel ----
    resident, roofline = None, None
    if args.full and args.resident_passes > 0 and world == 1:
        resident, roofline = device_resident(args, names, regions, snps, dev_idx, device, log)

    cfg_name = {(500_000_000, 10000, 1_000_000): "configs[2]", (50_000_000, 5000, 100_000): "configs[1]"}.get((args.reads, args.cells, args.snps), "configs[2] shape at a custom size")
    line = dict(metric="reads/sec into AD/DP+basefc matrices", value=round(value, 1), unit="reads/s",
                n_gpus=world, steps=args.steps, warmup=args.warmup, ms_per_step=round(ms_step, 3),
                higher_is_better=True, scaling="strong", vs_baseline=None, dtype="int64", data="synthetic",
                config=dict(workload="BASELINE.json %s: ONE synthetic 10x BAM of %d records (%.1f GB BGZF, page cache), %d barcodes, %d het SNPs, %d genes, "
                                     "24 hg38 contigs; end to end BAM -> basefc matrix.mtx + AD/DP/OTH.mtx from one decode; a step = 1/%d of the file's records, "
                                     "the last step also folds and writes" % (cfg_name, n_total, bam_bytes / 1e9, len(bcs), len(snps), len(regions), n_slices),
                            parallelism="contig-shard x%d (shard.plan_units: LPT on .bai counts, over-weight contigs cut at region boundaries)" % world,
                            host_threads_per_rank=threads, nnz=nnz),
                multi_gpu=mgpu,
                end_to_end=e2e, end_to_end_zlib6=subs.get("end_to_end_zlib6"), cellranger_shape=subs.get("cellranger_shape"),
                configs4_well=well, device_resident=resident, roofline=roofline, cpu_baseline=cpu, selfcheck=selfcheck)
    print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


def oracle_on_contigs(names, regions, snps, n_cols, bams, take, coo, threads, cpu_threads, dec_kw):
    """The oracle on whole contigs `take` of every BAM (decoded again by the host decoder), timed, and this process's matrix rows of
    those contigs compared with it bit for bit.  -> dict(n_dec, t_dec, t_count, n_cmp, parity)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as O
    import util
    mask = np.zeros(len(names), dtype=bool); mask[list(take)] = True
    cidx = {n: i for i, n in enumerate(names)}
    row_contig = np.array([cidx[r[0]] for r in regions], dtype=np.int32)
    dec = Engine(capi.XCK_MODE_BOTH, names, regions, n_cols, snps=snps, decode_only=True, n_threads=threads, **dec_kw)
    t_d = time.perf_counter()
    hb = []
    for i, b in enumerate(bams):
        hb += [util.batch_from_dict(d) for d in dec.decode_bam(b, sample=i, contig_mask=mask, use_index=True)]
    t_dec = time.perf_counter() - t_d
    dec.close()
    n_dec = sum(b.n_reads for b, _ in hb)
    sample_rows = mask[row_contig]
    parity, n_cmp, tc = "ok", 0, 0.0
    for mode, sn, mats in ((capi.XCK_MODE_BASEFC, [], ["count"]), (capi.XCK_MODE_BAF, snps, ["ad", "dp", "oth"])):
        cfg, keep = O.make_config(mode, names, regions, sn, n_cols, min_include=0.9, min_count=1, min_maf=0, no_dup_hap=True, **FILT)
        t1 = time.perf_counter()
        exp = O.run_oracle(cfg, [b for b, _ in hb], n_threads=cpu_threads)
        tc += time.perf_counter() - t1
        for m in mats:
            g = coo[m]
            sel = sample_rows[g[0]]
            n_cmp += int(sel.sum())
            if not all(np.array_equal(g[j][sel], exp[m][j]) for j in range(3)):
                parity = "MISMATCH in %s" % m
    return dict(n_dec=n_dec, t_dec=t_dec, t_count=tc, n_cmp=n_cmp, parity=parity)


def well_workload(args, dev_idx, device, threads, cores, log, world=1, rank=0, dist=None, shared_gpu=False, barrier=lambda: None, dump_dir=None):
    """BASELINE.json configs[4]: N per-cell BAMs (SMART-seq style: paired-end 2 x 75, mates share the read name, no CB / UB tags) through
    the multi-BAM ingest path - column = index of the BAM, key = read name (interned per file), basefc + pileup from ONE decode of every
    file - to the four .mtx files; reference path: xcltk/rdr/fc/core.py:153-170 (the loop over sam_list), rdr/fc/mcount.py:37-42,120-127.
    --full: the matrices' rows of the sampled contigs are compared with the oracle (same files decoded again by the host decoder) in the run.
    world > 1: every rank streams ITS units (contigs, shard.plan_units on the summed .bai counts of all files) of EVERY BAM, owns
    disjoint rows, and the ranks write the files together (or --gather); each rank checks the sampled contigs it owns against the oracle."""
    work = os.path.join(args.work, "well")
    n_snps = min(args.snps, 100_000)
    a2 = argparse.Namespace(**vars(args)); a2.snps = n_snps
    regions, snps, names, _ = make_tables_files(a2, work, 1) if rank == 0 else (None, None, None, None)
    barrier()
    if rank != 0:
        regions, snps, names = soa.make_tables(a2.genes, a2.snps, soa.HG38_LENGTHS, seed=2)   # (the same tables; the files exist already)
    cols = ["cell%03d" % i for i in range(args.well_bams)]
    t0 = time.time()
    bams = [os.path.join(work, "cell_%03d_%d_l%d.bam" % (i, args.well_reads, args.level)) for i in range(args.well_bams)]
    if rank == 0:
        import shutil
        need = sum(0 if os.path.isfile(b + ".ok") else int(args.well_reads * 80) for b in bams) + (2 << 30)   # about 75 bytes per record at the generator's fast level
        if shutil.disk_usage(work).free < need and args.make_room:
            # the work directory is scratch: files this tool generated itself (marked by their .ok file) give way, nothing else is touched
            import glob
            for ok in glob.glob(os.path.join(args.work, "synth_*.bam.ok")):
                for fn in (ok[:-3], ok[:-3] + ".bai", ok):
                    if os.path.isfile(fn):
                        os.remove(fn)
            log("--make-room: removed the 10x workload's generated BAMs from %s" % args.work)
        if shutil.disk_usage(work).free < need:
            sys.exit("bench.py --workload well: %s has %.1f GB free, the %d BAMs need %.1f GB (--make-room deletes the 10x workload's generated BAMs there)"
                     % (work, shutil.disk_usage(work).free / 1e9, len(bams), need / 1e9))
        from concurrent.futures import ThreadPoolExecutor              # small files: four generator processes side by side
        with ThreadPoolExecutor(max_workers=4) as ex:
            list(ex.map(lambda ib: gen_bam(a2, work, ib[1], args.well_reads, args.level, "smartseq", max(1, cores // 4), lambda m: None, seed=100 + ib[0]), enumerate(bams)))
    barrier()
    bam_bytes = sum(os.path.getsize(b) for b in bams)
    log("%d per-cell BAMs x %d records: %.1f GB, ready after %.1f s" % (len(bams), args.well_reads, bam_bytes / 1e9, time.time() - t0))
    rs = RankSet(shared_gpu, names, regions, snps, bams, args.gather) if world > 1 else None
    eng = Engine(capi.XCK_MODE_BOTH, names, regions, len(cols), snps=snps, barcodes=None, cell_tag=None, umi_tag=None, region_mask=rs.region_mask if rs else None,
                 device=dev_idx, min_include=0.9, min_count=1, min_maf=0, no_dup_hap=True, n_threads=threads, **FILT)
    out_dir = os.path.join(work, "out" if world == 1 else "out_n%d" % world)
    runs = []
    for rep in range((1 if args.warmup > 0 else 0) + 1):          # one untimed pass (buffers reach their sizes), one timed
        tm, n_rec, coo, nnz = whole_file_pass(eng, bams, out_dir, regions, cols, threads, rs)
        runs.append((tm, n_rec))
    tm, n_rec = runs[-1]
    stats = eng.stats()
    # ---- the oracle on the smallest contigs of every file (up to --cpu-sample records in total), and the GPU's rows of those contigs
    cpu, parity_all = None, None
    if args.full and args.cpu_sample > 0:
        counts = np.zeros(len(names), dtype=np.int64)
        for b in bams[:8]:                                         # (the per-contig shares are the same in every file: 8 files estimate them)
            counts += eng.contig_record_counts(b)
        scale = len(bams) / 8.0
        take, tot = [], 0.0
        for c in sorted(range(len(names)), key=lambda c: (counts[c], c)):
            if counts[c] == 0:
                continue
            if tot >= args.cpu_sample or (take and tot + counts[c] * scale > 2 * args.cpu_sample):
                break
            take.append(c); tot += counts[c] * scale
        if rs is not None:                                         # a rank checks the sampled contigs whose rows are all its own
            cidx = {n: i for i, n in enumerate(names)}
            row_contig = np.array([cidx[r[0]] for r in regions], dtype=np.int32)
            mine = [c for c in take if (rs.row_owner[row_contig == c] == rank).all()]
        else:
            mine = take
        cpu_threads = args.cpu_threads if args.cpu_threads > 0 else max(1, min(cores, 16) // (world if shared_gpu or world == 1 else 1))
        # (coo = this rank's own rows in either exchange form: xck_finish's views)
        chk = oracle_on_contigs(names, regions, snps, len(cols), bams, mine, coo, threads, cpu_threads, dict(barcodes=None, cell_tag=None, umi_tag=None)) if mine else \
            dict(n_dec=0, t_dec=0.0, t_count=0.0, n_cmp=0, parity="ok")
        bad = int(chk["parity"] != "ok")
        n_cmp_all, checked = chk["n_cmp"], len(mine)
        if dist is not None:
            tt = torch.tensor([bad, chk["n_cmp"], len(mine)], dtype=torch.int64, device="cpu" if shared_gpu else device)
            dist.all_reduce(tt)
            bad, n_cmp_all, checked = int(tt[0]), int(tt[1]), int(tt[2])
        if bad:
            sys.exit("bench.py --workload well: GPU result differs from the oracle on the sampled contigs: " + chk["parity"])
        parity_all = "ok (%d non-zeros of the four matrices compared bit for bit%s)" % (n_cmp_all, "" if world == 1 else "; %d sampled contigs checked by the ranks that own them" % checked)
        if world == 1:
            cpu = dict(value=round(chk["n_dec"] / chk["t_count"], 1), unit="reads/s", cores=cpu_threads, kind="port", seconds=round(chk["t_count"], 2),
                       value_with_decode=round(chk["n_dec"] / (chk["t_count"] + chk["t_dec"]), 1), decode_seconds=round(chk["t_dec"], 2), decode_threads=threads,
                       sample="the %d records of contig(s) %s of all %d BAMs, basefc + pileup, oracle/xck_oracle.c over %d threads" % (chk["n_dec"], ",".join(names[c] for c in take), len(bams), cpu_threads),
                       gpu_rows_vs_oracle=parity_all)
    # ---- whole-job numbers: the slowest rank's clock, every rank's records (a BGZF block shared by two ranks' contigs is walked twice, counted once)
    dt, n_all, mgpu = tm["seconds"], n_rec, None
    if dist is not None:
        tt = torch.tensor([tm["seconds"], float(n_rec)], dtype=torch.float64, device="cpu" if shared_gpu else device)
        tmax = tt.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dist.all_reduce(tt, op=dist.ReduceOp.SUM)
        dt, n_all = float(tmax[0]), min(int(tt[1]), int(rs.d.contig_weights.sum()))   # (.bai counts of all files: every BAM record once)
        mgpu = multi_gpu_record(rs, dist, device, threads, dict(ingest=tm["ingest"], finish=tm["finish"]), n_rec, shared_gpu)
    if dump_dir:
        dump_outputs(dump_dir, coo, len(regions), len(cols), device, dist)
    eng.close()
    if rank != 0:
        return None
    value = n_all / dt
    return dict(metric="reads/sec into AD/DP+basefc matrices", value=round(value, 1), unit="reads/s", n_gpus=world, steps=1, warmup=len(runs) - 1,
                ms_per_step=round(dt * 1e3, 1), higher_is_better=True, scaling="strong", vs_baseline=None, dtype="int64", data="synthetic",
                config=dict(workload="BASELINE.json configs[4]: %d per-cell BAMs x %d records (paired-end 2 x 75, mates share the read name, no CB / UB tags; %.1f GB BGZF by %s, "
                                     "page cache), %d het SNPs, %d genes, 24 hg38 contigs; multi-BAM ingest (column = BAM, key = read name), basefc matrix.mtx + AD/DP/OTH.mtx from one "
                                     "decode of every file; a step = the whole list" % (len(bams), args.well_reads, bam_bytes / 1e9, writer_name(args.level), len(snps), len(regions)),
                            parallelism="1 GPU" if world == 1 else "contig-shard x%d: every rank streams its units of every BAM (shard.plan_units on the summed .bai counts), disjoint rows" % world,
                            host_threads_per_rank=threads, nnz=nnz),
                end_to_end=dict(records=n_all, seconds=round(dt, 3), phase_seconds=dict(ingest=round(tm["ingest"], 3), finish=round(tm["finish"], 3), write=round(tm["seconds"], 3)),
                                warmup_pass_seconds=round(runs[0][0]["seconds"], 3), bam_gb=round(bam_bytes / 1e9, 2), bam_bytes_per_record=round(bam_bytes / max(n_all, 1), 1),
                                bgzf_writer=writer_name(args.level), host_threads_per_rank=threads, host_cores=cores, key_bits=int(stats["key_bits"]), basefc_fold_path=int(stats["fold_path"]),
                                engine_ms=dict(h2d=round(stats["ms_h2d"], 1), join=round(stats["ms_join"], 1), fold=round(stats["ms_sort"], 1), d2h=round(stats["ms_d2h"], 1)),
                                hits=dict(accepted=int(stats["n_hits"]), after_lds_dedup=int(stats["n_hits_unique"])),
                                gpu_inflate=dict(mode=os.environ.get("XCK_GPU_INFLATE", "auto"), chunks_on_device=int(stats.get("gpu_inflate_chunks", 0)))),
                multi_gpu=mgpu, gpu_rows_vs_oracle=parity_all, roofline=None, cpu_baseline=cpu)


def cpu_baseline(args, eng, bam, names, regions, snps, bcs, counts, coo, row_contig, threads, cores, log):
    """The oracle on whole contigs of the same BAM (smallest first, up to --cpu-sample records), timed; the GPU rows of
    those contigs must equal it bit for bit."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle as O
    import util
    take, tot = [], 0
    for c in sorted(range(len(names)), key=lambda c: (counts[c], c)):
        if counts[c] == 0:
            continue
        if tot >= args.cpu_sample or (take and tot + counts[c] > 2 * args.cpu_sample):
            break
        take.append(c)
        tot += int(counts[c])
    mask = np.zeros(len(names), dtype=bool)
    mask[take] = True
    dec = Engine(capi.XCK_MODE_BOTH, names, regions, len(bcs), snps=snps, barcodes=bcs, cell_tag="CB", umi_tag="UB",
                 decode_only=True, n_threads=threads)
    t_d = time.perf_counter()                                  # host decode of the sampled contigs (BGZF inflate + record parse, `threads` threads)
    hb = [util.batch_from_dict(d) for d in dec.decode_bam(bam, contig_mask=mask, use_index=True)]
    t_dec = time.perf_counter() - t_d
    dec.close()
    n_dec = sum(b.n_reads for b, _ in hb)
    cpu_threads = args.cpu_threads if args.cpu_threads > 0 else max(1, min(cores, 16))
    sample_rows = mask[row_contig]
    parity, n_cmp, tc = "ok", 0, 0.0
    for mode, sn, mats in ((capi.XCK_MODE_BASEFC, [], ["count"]), (capi.XCK_MODE_BAF, snps, ["ad", "dp", "oth"])):
        cfg, keep = O.make_config(mode, names, regions, sn, len(bcs), min_include=0.9, min_count=1, min_maf=0, no_dup_hap=True, **FILT)
        t1 = time.perf_counter()
        exp = O.run_oracle(cfg, [b for b, _ in hb], n_threads=cpu_threads)
        tc += time.perf_counter() - t1
        for m in mats:
            g = coo[m]
            sel = sample_rows[g[0]]
            n_cmp += int(sel.sum())
            if not all(np.array_equal(g[j][sel], exp[m][j]) for j in range(3)):
                parity = "MISMATCH in %s" % m
    log("cpu baseline: %d records in %.1f s; parity %s" % (n_dec, tc, parity))
    if parity != "ok":
        sys.exit("bench.py: GPU result differs from the oracle on the sampled contigs: " + parity)
    return dict(value=round(n_dec / tc, 1), unit="reads/s", cores=cpu_threads, kind="port",
                sample="the %d records of contig(s) %s of the same BAM (decoded to SoA batches before the timed call), basefc + pileup, "
                       "oracle/xck_oracle.c (xo_run_mt: region chunks over %d threads)" % (n_dec, ",".join(names[c] for c in take), cpu_threads),
                seconds=round(tc, 2),
                value_with_decode=round(n_dec / (tc + t_dec), 1), decode_seconds=round(t_dec, 2), decode_threads=threads,
                with_decode_note="value_with_decode = the same records / (host decode of those contigs by this repo's decoder, %d threads behind %d CPUs, "
                                 "copied out as numpy batches + the oracle's counting): the CPU-only form of the headline's boundary, minus the .mtx text" % (threads, cores),
                gpu_rows_vs_oracle="%s (%d non-zeros of the end-to-end matrices compared bit for bit)" % (parity, n_cmp))


def device_resident(args, names, regions, snps, dev_idx, device, log):
    """The same workload shape as SoA batches already in HBM (generated on the device): one basefc pass + one pileup pass
    per step through xck_push_batch_device / xck_finish, serial (no overlap between engines) so that every stage time is
    the stage's own.  Feeds the roofline of the dominant hand-written kernel."""
    arrays, batches = soa_torch.gen_reads_device(regions, names, args.reads, args.cells, seed=100, device=device)
    torch.cuda.synchronize()
    n_reads = arrays["n_reads"]
    eng_fc = Engine(capi.XCK_MODE_BASEFC, names, regions, args.cells, device=dev_idx, min_include=0.9, **FILT)
    eng_baf = Engine(capi.XCK_MODE_BAF, names, regions, args.cells, snps=snps, device=dev_idx, min_count=1, min_maf=0, no_dup_hap=True, **FILT)
    b_fc = [soa_torch.device_batch(capi, arrays, c, s, e, False) for c, s, e in batches]
    b_baf = [soa_torch.device_batch(capi, arrays, c, s, e, True) for c, s, e in batches]
    acc = dict(ms_join_fc=0.0, ms_join_baf=0.0, ms_fin_fc=0.0, ms_fin_baf=0.0, ms_d2h=0.0)
    res = {}

    def one(eng, bs, join_key, fin_key, collect):
        eng.reset()
        for b in bs:
            eng.push(b, device_resident=True)              # queued; fused into one launch
        eng.flush()
        out = eng.finish(copy=False)
        st = eng.stats()
        if collect:
            acc[join_key] += st["ms_join"]; acc[fin_key] += st["ms_sort"]; acc["ms_d2h"] += st["ms_d2h"]
            res.update(out); res[join_key] = st
    for _ in range(2):                                      # buffers reach their sizes (hit buffers grow by replay)
        one(eng_fc, b_fc, "ms_join_fc", "ms_fin_fc", False)
        one(eng_baf, b_baf, "ms_join_baf", "ms_fin_baf", False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.resident_passes):
        one(eng_fc, b_fc, "ms_join_fc", "ms_fin_fc", True)
        one(eng_baf, b_baf, "ms_join_baf", "ms_fin_baf", True)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.resident_passes
    sfc, sbaf = res["ms_join_fc"], res["ms_join_baf"]
    k = {a: b / args.resident_passes for a, b in acc.items()}
    L = arrays["read_len"]
    hits_fc, hits_baf = sfc["n_hits"], sbaf["n_hits"]
    # SURVEY 8d per-unit figures: 20 B/read + 4 B/CIGAR op (+ ceil(L/4) B bases for pileup); 16 B per basefc hit written, 24 B per pileup hit written
    A_fc = n_reads * 20 + arrays["n_cig"] * 4 + hits_fc * 16
    A_baf = n_reads * (20 + (L + 3) // 4) + arrays["n_cig"] * 4 + hits_baf * 24
    dom = max(("k_join<basefc>", k["ms_join_fc"], A_fc, sfc), ("k_join<pileup>", k["ms_join_baf"], A_baf, sbaf), key=lambda x: x[1])
    n_launch = max(1, int(dom[3]["n_join_launches"]))
    avg_ms = dom[1] / n_launch
    achieved = (dom[2] / n_launch) / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    # PMC bytes: collected at the default workload only (tools/profile_round.sh -> profiles/pmc_traffic.json), and only valid for the
    # kernel sources they were counted on (the file carries their hash): a changed kernel reports null until the counters are re-collected
    traffic, traffic_note = None, "not collected for this workload size"
    if os.path.isfile(args.pmc_json) and (args.reads, args.cells, args.snps) == (500_000_000, 10000, 1_000_000):
        try:
            pj = json.load(open(args.pmc_json))
            src = os.path.join(ROOT, "xcltk_amd", "csrc")
            now = hashlib.sha256(b"".join(open(os.path.join(src, f), "rb").read() for f in ("engine.hip", "fold_partition.h"))).hexdigest()[:16]
            if pj.get("_kernel_source_sha256_16") == now:
                traffic, traffic_note = pj.get(dom[0]), "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes), 2 x FETCH + WRITE, of the kernel sources " + now
            else:
                traffic_note = "profiles/pmc_traffic.json was counted on other kernel sources (%s, now %s): re-collect" % (pj.get("_kernel_source_sha256_16"), now)
        except Exception:
            traffic = None
    both = {name: dict(avg_launch_ms=round(ms / max(1, int(stt["n_join_launches"])), 4), algorithmic_bytes_per_launch=int(A / max(1, int(stt["n_join_launches"]))),
                       frac=round((A / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if ms > 0 else 0.0, 4))
            for name, ms, A, stt in (("k_join<basefc>", k["ms_join_fc"], A_fc, sfc), ("k_join<pileup>", k["ms_join_baf"], A_baf, sbaf))}
    roofline = dict(bound="hbm", kernel=dom[0], achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                    frac=round(achieved / HBM_PEAK_GBS, 4), traffic=traffic, traffic_note=traffic_note, launches_per_pass=n_launch, avg_launch_ms=round(avg_ms, 4),
                    algorithmic_bytes_per_launch=int(dom[2] / n_launch), workload="HBM-resident sub-record (device_resident)",
                    note="dominant = the join kernel with the longer launch; both join kernels are listed under 'kernels'", kernels=both)
    resident = dict(reads=n_reads, passes=args.resident_passes, ms_per_pass=round(dt * 1e3, 3), reads_per_s=round(n_reads / dt, 1),
                    pipeline="serial: basefc pass then pileup pass, matrices copied out to pinned host memory inside the pass",
                    stage_ms_per_pass={a: round(b, 3) for a, b in k.items()},
                    nnz={m: int(len(res[m][0])) for m in ("count", "ad", "dp", "oth")},
                    hits=dict(basefc=int(hits_fc), pileup=int(hits_baf), basefc_after_lds_dedup=int(sfc["n_hits_unique"]), pileup_after_lds_dedup=int(sbaf["n_hits_unique"])),
                    # which fold ran (include/xck.h xck_stats): 1 = the sort-free partition paths, 2 = the radix-sort fallbacks
                    fold_paths=dict(basefc=int(sfc.get("fold_path", 0)), pileup_hits=int(sbaf.get("pileup_sort_path", 0)), pileup_region_level=int(sbaf.get("pileup_sort2_path", 0))))
    exp = EXPECTED_RESIDENT.get((args.reads, args.cells, args.snps, args.genes))
    if exp is not None:
        obs = dict(hits_basefc=int(hits_fc), hits_pileup=int(hits_baf), **{"nnz_" + m: int(len(res[m][0])) for m in ("count", "ad", "dp", "oth")})
        resident["expected"] = exp
        resident["matches_expected"] = obs == exp
        if obs != exp:
            sys.stderr.write("bench.py: the HBM-resident sub-record counted %s, the committed values for this workload are %s\n" % (obs, exp))
    log("resident: %.2f ms/pass %s" % (dt * 1e3, resident["stage_ms_per_pass"]))
    eng_fc.close(); eng_baf.close()
    return resident, roofline


if __name__ == "__main__":
    main()
