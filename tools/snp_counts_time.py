#!/usr/bin/env python
"""What the SNP x cell matrices of a finished pileup cost: xck_snp_counts beside the detour that gives the same matrices without it,
xck_refold to one one-base region per SNP - on the same handle, in one process on one GPU.

The workload is the HBM-resident one of `bench.py --resident-only` (xcltk_amd/synth/soa_torch.py at BASELINE configs[2]: 500 M reads,
10 k cells, 1 M SNPs, 33 k genes).  One handle; the first pass and the first two calls of each kind are not timed (they size the
buffers).  Then `--repeats` rounds (at least 5), each of
  xck_snp_counts   the library's own `[xck] snp_counts:` line under XCK_DEBUG_TIMING: host clock to the compute stream's synchronise,
                   the stages by HIP events (flags + long runs, scans + row bases, emit) and the wait for the copy-out; and the wall
                   time of the whole call;
  xck_refold       to the one-base regions (REF on haplotype 0, ALT on 1, min_count 1, min_maf 0): the library's `[xck] refold:` line -
                   host clock to the stream synchronise, table upload, builder kernels + scan, region stage - and the wall time of the
                   whole call (it ends with the same wait for the copy-out);
  xck_refold       back to the genes, so that every round starts from the same tables (not timed).
The two results are asserted equal in every round.  Prints one JSON line with the medians and the spread (min, max), and writes it
to --out.
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

SC_RE = re.compile(r"\[xck\] snp_counts: total ([0-9.]+) ms .*flags \+ long runs ([0-9.]+), scans \+ row bases ([0-9.]+), emit ([0-9.]+); wait for the copy-out ([0-9.]+); (\d+) entries")
SC_PARTS = ("total_ms", "flags_long_runs_ms", "scans_row_bases_ms", "emit_ms", "copy_out_wait_ms")
RF_PARTS = ("total_ms", "table_upload_ms", "builder_kernels_scan_ms", "region_stage_ms")


def main():
    from refold_time import REFOLD_RE, StderrCapture, stat
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500_000_000)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33472)
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
    snps = list(snps)
    if len({(s[0], s[1]) for s in snps}) != len(snps):
        sys.exit("the synthetic SNP table holds a position twice: the one-base regions would not be per SNP")
    onebase = [(s[0], s[1], s[1], "s%d" % i) for i, s in enumerate(snps)]
    snps01 = [(s[0], s[1], s[2], s[3], 0, 1) for s in snps]
    arrays, batches = soa_torch.gen_reads_device(regions, names, args.reads, args.cells, seed=100, device=device)
    torch.cuda.synchronize()
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
    cap.stop()
    acc = dict(sc=[], sc_wall=[], rf=[], rf_wall=[])
    entries, nnz = 0, None
    for rep in range(args.repeats + 2):                        # rounds 0 and 1 size the buffers of both calls
        cap.start()
        t0 = time.perf_counter()
        got = eng.snp_counts(copy=False)
        dt_sc = (time.perf_counter() - t0) * 1e3
        t_sc = cap.stop()
        cap.start()
        t0 = time.perf_counter()
        det = eng.refold(onebase, snps=snps01, min_count=1, min_maf=0, no_dup_hap=True, copy=False)
        dt_rf = (time.perf_counter() - t0) * 1e3               # (includes building the 10^6-row table in Python: reported, not compared)
        t_rf = cap.stop()
        for k in ("ad", "dp", "oth"):
            for j in range(3):
                assert np.array_equal(got[k][j], det[k][j]), "xck_snp_counts and the one-base refold differ in %s[%d]" % (k, j)
        nnz = {k: int(len(got[k][0])) for k in ("ad", "dp", "oth")}
        cap.start()
        eng.refold(regions, snps=snps, copy=False)
        cap.stop()
        if rep < 2:
            continue
        m = SC_RE.search(t_sc)
        entries = int(m.group(6))
        acc["sc"].append([float(x) for x in m.groups()[:5]]); acc["sc_wall"].append(dt_sc)
        acc["rf"].append([float(x) for x in REFOLD_RE.search(t_rf).groups()]); acc["rf_wall"].append(dt_rf)
    eng.close()
    out = dict(tool="tools/snp_counts_time.py", workload=dict(reads=args.reads, cells=args.cells, snps=args.snps, genes=args.genes),
               repeats=args.repeats, device=torch.cuda.get_device_name(0), stream_entries=entries, nnz=nnz,
               snp_counts={p: stat([r[i] for r in acc["sc"]]) for i, p in enumerate(SC_PARTS)},
               snp_counts_call_wall_ms=stat(acc["sc_wall"]),
               refold_to_one_base_regions={p: stat([r[i] for r in acc["rf"]]) for i, p in enumerate(RF_PARTS)},
               refold_call_wall_ms_with_python_tables=stat(acc["rf_wall"]), results_equal=True)
    out["snp_counts_not_slower_than_detour"] = out["snp_counts"]["total_ms"]["median"] <= out["refold_to_one_base_regions"]["total_ms"]["median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    assert out["snp_counts_not_slower_than_detour"], "xck_snp_counts is slower than the refold detour measured in the same run"


if __name__ == "__main__":
    main()
