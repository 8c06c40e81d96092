#!/usr/bin/env python
"""What pseudo-bulk matrices per cell group cost: xck_group_counts beside the host path it replaces - copy every per-cell block out
and sum its columns per group in numpy - on the same handle, in one process on one GPU.

The workload is the HBM-resident one of `bench.py --resident-only` (xcltk_amd/synth/soa_torch.py at BASELINE configs[2]: 500 M reads,
10 k cells, 1 M SNPs, 33 k genes), on a pileup handle, with 20 groups drawn at random over the cells (seed 7; one cell in twenty left
out).  One handle; the first pass and the first two rounds are not timed (they size the buffers).  Then `--repeats` rounds (at least
5), each of, for source RESULT (gene x cell AD / DP / OTH of the finish) and for source SNP (the SNP x cell blocks of xck_snp_counts):
  xck_group_counts   the library's own `[xck] group_counts:` line under XCK_DEBUG_TIMING: host clock to the compute stream's
                     synchronise, the stages by HIP events (row pointers, count pass + scans, emit pass) and the wait for the
                     copy-out; and the wall time of the whole call from Python;
  host path          finish(copy=True) / snp_counts(copy=True) followed by host_aggregate() below, wall time from the call to the
                     aggregated arrays.  host_aggregate is vectorised numpy (gather, stable argsort of row * n_groups + group,
                     add.reduceat): the way a user of the Python API would write it, not a tuned C loop.
The two results are asserted equal in every round.  Prints one JSON line with the medians and the spread (min, max) and the ratio of
the medians, and writes it to --out.  No threshold: the tool reports what comes out.
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

GC_RE = re.compile(r"\[xck\] group_counts: source (\w+), (\d+) groups: total ([0-9.]+) ms .*row pointers ([0-9.]+), count \+ scans ([0-9.]+), emit ([0-9.]+); "
                   r"wait for the copy-out ([0-9.]+); (\d+) entries")
GC_PARTS = ("total_ms", "row_pointers_ms", "count_scans_ms", "emit_ms", "copy_out_wait_ms")
MATS = ("ad", "dp", "oth")


def host_aggregate(coo, cell_group, n_groups):
    import numpy as np
    row, col, val = coo
    g = cell_group[col]
    keep = g >= 0
    key = row[keep].astype(np.int64) * n_groups + g[keep]
    v = val[keep].astype(np.int64)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    if not len(ks):
        z = np.zeros(0, np.int32)
        return z, z.copy(), z.copy()
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    sums = np.add.reduceat(v[order], starts)
    k = ks[starts]
    return (k // n_groups).astype(np.int32), (k % n_groups).astype(np.int32), sums.astype(np.int32)


def main():
    from refold_time import StderrCapture, stat
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500_000_000)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33472)
    ap.add_argument("--groups", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats: at least 5")
    os.environ["XCK_DEBUG_TIMING"] = "1"                       # (a handle reads its knobs at xck_create)
    import numpy as np
    import torch
    from xcltk_amd import capi
    from xcltk_amd.engine import Engine
    from xcltk_amd.synth import soa, soa_torch
    filt = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True)
    device = torch.device("cuda", 0)
    regions, snps, names = soa.make_tables(args.genes, args.snps, soa.HG38_LENGTHS, seed=2)
    arrays, batches = soa_torch.gen_reads_device(regions, names, args.reads, args.cells, seed=100, device=device)
    torch.cuda.synchronize()
    rng = np.random.default_rng(7)
    cg = rng.integers(0, args.groups, args.cells).astype(np.int32)
    cg[rng.random(args.cells) < 0.05] = -1
    cap = StderrCapture()
    eng = Engine(capi.XCK_MODE_BAF, names, regions, args.cells, snps=snps, device=0, min_count=1, min_maf=0, no_dup_hap=True, **filt)
    bs = [soa_torch.device_batch(capi, arrays, c, s, e, True) for c, s, e in batches]
    cap.start()
    for warm in range(2):                                      # (the first pass of a new handle sizes its hit buffers and workspaces)
        eng.reset()
        for b in bs:
            eng.push(b, device_resident=True)
        eng.flush()
        eng.finish(copy=False)
    eng.snp_counts(copy=False)
    cap.stop()
    acc = {s: dict(dev=[], dev_wall=[], host=[]) for s in ("result", "snp")}
    info = {}
    for rep in range(args.repeats + 2):                        # rounds 0 and 1 size the buffers
        for source in ("result", "snp"):
            cap.start()
            t0 = time.perf_counter()
            got = eng.group_counts(cg, args.groups, source=source, copy=False)
            dt_dev = (time.perf_counter() - t0) * 1e3
            text = cap.stop()
            cap.start()
            t0 = time.perf_counter()
            cells = eng.finish(copy=True) if source == "result" else eng.snp_counts(copy=True)
            host = {k: host_aggregate(cells[k], cg, args.groups) for k in MATS}
            dt_host = (time.perf_counter() - t0) * 1e3
            cap.stop()
            for k in MATS:
                for j in range(3):
                    assert np.array_equal(got[k][j], host[k][j]), "xck_group_counts and the host path differ in %s %s[%d]" % (source, k, j)
            m = GC_RE.search(text)
            assert m and m.group(1) == source, text
            info[source] = dict(source_entries=int(m.group(8)), source_bytes=int(m.group(8)) * 12, nnz={k: int(len(got[k][0])) for k in MATS})
            if rep < 2:
                continue
            acc[source]["dev"].append([float(x) for x in m.groups()[2:7]]); acc[source]["dev_wall"].append(dt_dev); acc[source]["host"].append(dt_host)
    eng.close()
    out = dict(tool="tools/group_counts_time.py", workload=dict(reads=args.reads, cells=args.cells, snps=args.snps, genes=args.genes, groups=args.groups),
               repeats=args.repeats, device=torch.cuda.get_device_name(0), results_equal=True)
    for source in ("result", "snp"):
        a = acc[source]
        d = dict(info[source], group_counts={p: stat([r[i] for r in a["dev"]]) for i, p in enumerate(GC_PARTS)},
                 group_counts_call_wall_ms=stat(a["dev_wall"]), host_copy_and_numpy_wall_ms=stat(a["host"]))
        d["host_over_device_call_wall"] = round(d["host_copy_and_numpy_wall_ms"]["median"] / max(d["group_counts_call_wall_ms"]["median"], 1e-9), 2)
        out[source] = d
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
