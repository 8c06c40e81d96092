#!/usr/bin/env python
"""What a recount costs beside a fresh count: xck_create, a fresh xck_finish of the pileup and xck_refold, in one process on one GPU.

The workload is the HBM-resident one of `bench.py --resident-only` (xcltk_amd/synth/soa_torch.py at BASELINE configs[2]: 500 M reads,
10 k cells, 1 M SNPs, 33 k genes).  After a warm-up round, `--repeats` rounds (at least 5), each on a new handle whose first pass and
first two refolds are not timed (they size the handle's buffers), of
  xck_create        wall time, and the share of it the host SNP -> region CSR loop of build_tables takes ([xck] create: ... under
                    XCK_DEBUG_TIMING);
  push + xck_finish the pileup's fold by HIP events (xck_stats.ms_sort);
  xck_refold        to the same tables: host clock ending in the stream synchronise, split into table upload, the two builder kernels +
                    scan (HIP events) and the region stage (HIP events) - the library's own `[xck] refold:` line;
  xck_refold        from the genes to 100 kb bins.
Prints one JSON line with the medians and the spread (min, max), and writes it to --out.  The library's debug lines are read from the
process's stderr, which is redirected to a file while the measured calls run.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class StderrCapture(object):
    """fd 2 goes to a file between start() and stop(); stop() returns what was written."""
    def __init__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = None

    def start(self):
        sys.stderr.flush()
        self.tmp.seek(0); self.tmp.truncate()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)

    def stop(self):
        sys.stderr.flush()
        os.dup2(self.saved, 2); os.close(self.saved)
        self.tmp.seek(0)
        return self.tmp.read().decode("utf-8", "replace")


def stat(xs):
    xs = sorted(xs)
    n = len(xs)
    med = xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])
    return dict(median=round(med, 4), min=round(xs[0], 4), max=round(xs[-1], 4), n=n)


REFOLD_RE = re.compile(r"\[xck\] refold: total ([0-9.]+) ms .*table upload ([0-9.]+), builder kernels \+ scan ([0-9.]+), region stage ([0-9.]+)")
CSR_RE = re.compile(r"\[xck\] create: host SNP -> region CSR loop ([0-9.]+) ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500_000_000)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33472)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bin", type=int, default=100_000, help="width of the fixed-size bins of the second refold")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats: at least 5")
    os.environ["XCK_DEBUG_TIMING"] = "1"                       # (a handle reads its knobs at xck_create)
    import torch
    from xcltk_amd import capi
    from xcltk_amd.engine import Engine
    from xcltk_amd.synth import soa, soa_torch
    filt = dict(min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True)
    device = torch.device("cuda", 0)
    regions, snps, names = soa.make_tables(args.genes, args.snps, soa.HG38_LENGTHS, seed=2)
    lengths = dict(zip(names, soa.HG38_LENGTHS))
    bins = [(c, s, min(s + args.bin - 1, int(lengths[c])), "%s_%d" % (c, s)) for c in names for s in range(1, int(lengths[c]) + 1, args.bin)]
    arrays, batches = soa_torch.gen_reads_device(regions, names, args.reads, args.cells, seed=100, device=device)
    torch.cuda.synchronize()
    cap = StderrCapture()
    acc = dict(create_ms=[], create_csr_loop_ms=[], finish_ms_sort=[], refold_same=[], refold_bins=[])
    eng = None
    for rep in range(args.repeats + 1):                        # round 0 warms up: buffers reach their sizes
        if eng is not None:
            eng.close()
        cap.start()
        t0 = time.perf_counter()
        eng = Engine(capi.XCK_MODE_BAF, names, regions, args.cells, snps=snps, device=0, min_count=1, min_maf=0, no_dup_hap=True, **filt)
        dt_create = (time.perf_counter() - t0) * 1e3
        text = cap.stop()
        bs = [soa_torch.device_batch(capi, arrays, c, s, e, True) for c, s, e in batches]
        for warm in range(2):                                  # (the first pass of a new handle sizes its hit buffers and workspaces)
            eng.reset()
            for b in bs:
                eng.push(b, device_resident=True)
            eng.flush()
            cap.start()
            first = eng.finish(copy=False)
            cap.stop()
        ms_sort = eng.stats()["ms_sort"]
        nnz = {k: int(len(first[k][0])) for k in ("ad", "dp", "oth")}
        cap.start()
        eng.refold(regions, copy=False); eng.refold(bins, copy=False)     # (likewise: the builder's buffers, the bins' workspace)
        cap.stop()
        cap.start()
        same = eng.refold(regions, copy=False)
        t_same = cap.stop()
        assert {k: int(len(same[k][0])) for k in nnz} == nnz, "a refold to the same tables changed the matrices' sizes"
        cap.start()
        eng.refold(bins, copy=False)
        t_bins = cap.stop()
        if rep == 0:
            continue
        acc["create_ms"].append(dt_create)
        acc["create_csr_loop_ms"].append(float(CSR_RE.search(text).group(1)))
        acc["finish_ms_sort"].append(ms_sort)
        acc["refold_same"].append([float(x) for x in REFOLD_RE.search(t_same).groups()])
        acc["refold_bins"].append([float(x) for x in REFOLD_RE.search(t_bins).groups()])
    eng.close()
    parts = ("total_ms", "table_upload_ms", "builder_kernels_scan_ms", "region_stage_ms")
    out = dict(tool="tools/refold_time.py", workload=dict(reads=args.reads, cells=args.cells, snps=args.snps, genes=args.genes, bins=len(bins), bin_width=args.bin),
               repeats=args.repeats, device=torch.cuda.get_device_name(0),
               xck_create_ms=stat(acc["create_ms"]), create_host_csr_loop_ms=stat(acc["create_csr_loop_ms"]),
               fresh_finish_ms_sort=stat(acc["finish_ms_sort"]),
               refold_same_tables={p: stat([r[i] for r in acc["refold_same"]]) for i, p in enumerate(parts)},
               refold_genes_to_bins={p: stat([r[i] for r in acc["refold_bins"]]) for i, p in enumerate(parts)})
    out["refold_cheaper_than_fresh_finish"] = out["refold_same_tables"]["total_ms"]["median"] < out["fresh_finish_ms_sort"]["median"]
    out["device_tables_cheaper_than_host_loop"] = (out["refold_same_tables"]["table_upload_ms"]["median"] + out["refold_same_tables"]["builder_kernels_scan_ms"]["median"]
                                                   < out["create_host_csr_loop_ms"]["median"])
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
