#!/usr/bin/env python
"""What a recount for a subset of the cells costs: xck_refold with a cell mask beside the plain xck_refold and a fresh xck_finish, on one GPU.

The workload is the HBM-resident one of `bench.py --resident-only` and tools/refold_time.py (xcltk_amd/synth/soa_torch.py at BASELINE
configs[2]: 500 M reads, 10 k cells, 1 M SNPs, 33 k genes).  A session is one fresh process on one handle: two untimed passes size
the handle's buffers, then `--repeats` rounds (at least 5) of
  push + xck_finish          the pileup's fold by HIP events (xck_stats.ms_sort);
  xck_refold                 to the same tables, no mask: the library's own `[xck] refold:` line (host clock ending in the stream
                             synchronise; table upload, builder kernels + scan and region stage by HIP events);
  xck_refold(cell_enabled)   the same with a random 10 %, a random 50 % and all of the cells enabled (all: the call finds the mask full on
                             the host and takes the unmasked kernels), with the line's `cell mask` part: bit table upload, SNP bounds, masked tallies.
The first timed call of each kind follows an untimed one of the same kind.

With --parent-lib the sessions alternate between that library (the parent commit's libxck.so, which knows no mask: finish and the plain
refold only) and this tree's, `--sessions` of each in the order parent, tree, tree, parent, ...: the plain refold and the finish must not
have become slower.  The
bar is the parent's own [min, max] over all its rounds; the JSON says whether this tree's medians lie inside and gives both.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from refold_time import REFOLD_RE, StderrCapture, stat  # noqa: E402

MASK_RE = re.compile(r"cell mask ([0-9.]+)")
PARTS = ("total_ms", "table_upload_ms", "builder_kernels_scan_ms", "region_stage_ms")


def session(args):
    """One handle in this process, under whatever library XCK_LIB names.  -> dict of lists, one entry per timed round"""
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
    masks = {} if args.no_masks else {"10": rng.random(args.cells) < 0.1, "50": rng.random(args.cells) < 0.5, "100": np.ones(args.cells, bool)}
    cap = StderrCapture()
    acc = dict(finish_ms_sort=[], refold_plain=[], nnz_dp=[])
    for k in masks:
        acc["refold_mask_%s" % k] = []; acc["cell_mask_ms_%s" % k] = []; acc["nnz_dp_%s" % k] = []

    def timed_refold(**kw):
        cap.start()
        r = eng.refold(regions, copy=False, **kw)
        text = cap.stop()
        return [float(x) for x in REFOLD_RE.search(text).groups()], text, int(len(r["dp"][0]))

    eng = Engine(capi.XCK_MODE_BAF, names, regions, args.cells, snps=snps, device=0, min_count=1, min_maf=0, no_dup_hap=True, **filt)
    try:
        bs = [soa_torch.device_batch(capi, arrays, c, s, e, True) for c, s, e in batches]
        for rnd in range(-2, args.repeats):                    # (the first passes of a new handle size its hit buffers and workspaces)
            eng.reset()
            for b in bs:
                eng.push(b, device_resident=True)
            eng.flush()
            cap.start()
            eng.finish(copy=False)
            cap.stop()
            ms_sort = eng.stats()["ms_sort"]
            timed_refold()
            plain, _, nnz = timed_refold()
            got = {}
            for k, m in masks.items():
                timed_refold(cell_enabled=m)
                parts, text, z = timed_refold(cell_enabled=m)
                got[k] = (parts, float(MASK_RE.search(text).group(1)), z)
            if rnd < 0:
                continue
            acc["finish_ms_sort"].append(ms_sort); acc["refold_plain"].append(plain); acc["nnz_dp"].append(nnz)
            for k, (parts, ms, z) in got.items():
                acc["refold_mask_%s" % k].append(parts); acc["cell_mask_ms_%s" % k].append(ms); acc["nnz_dp_%s" % k].append(z)
        acc["device"] = torch.cuda.get_device_name(0)
        acc["cells_enabled"] = {k: int(m.sum()) for k, m in masks.items()}
    finally:
        eng.close()
    return acc


def parts_stat(rows):
    return {p: stat([r[i] for r in rows]) for i, p in enumerate(PARTS)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500_000_000)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=33472)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sessions", type=int, default=2, help="sessions per library when --parent-lib is given")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libxck.so: alternate its sessions with this tree's")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-masks", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats: at least 5")
    if args.worker:
        print("SESSION " + json.dumps(session(args)))
        return

    def run(lib, no_masks):
        env = dict(os.environ)
        if lib:
            env["XCK_LIB"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reads", str(args.reads), "--cells", str(args.cells), "--snps", str(args.snps),
               "--genes", str(args.genes), "--repeats", str(args.repeats)] + (["--no-masks"] if no_masks else [])
        p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit("a session failed (exit %d)" % p.returncode)      # (nothing more is started on the GPU)
        print("[refold_cells_time] session under %s done" % (lib or "this tree's library"), file=sys.stderr, flush=True)
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("SESSION ")][-1][len("SESSION "):])

    new, parent = [], []
    for i in range(args.sessions if args.parent_lib else 1):
        if args.parent_lib and i % 2 == 0:                      # parent, this tree, this tree, parent, ...: neither is always the second
            parent.append(run(args.parent_lib, True))
        new.append(run(None, False))
        if args.parent_lib and i % 2 == 1:
            parent.append(run(args.parent_lib, True))
    cat = lambda ss, k: [x for s in ss for x in s[k]]
    out = dict(tool="tools/refold_cells_time.py", workload=dict(reads=args.reads, cells=args.cells, snps=args.snps, genes=args.genes),
               repeats=args.repeats, sessions=len(new), device=new[0]["device"], cells_enabled=new[0]["cells_enabled"],
               fresh_finish_ms_sort=stat(cat(new, "finish_ms_sort")), refold_plain=parts_stat(cat(new, "refold_plain")), nnz_dp=new[0]["nnz_dp"][0])
    for k in new[0]["cells_enabled"]:
        out["refold_mask_%s_percent" % k] = dict(parts_stat(cat(new, "refold_mask_%s" % k)), cell_mask_ms=stat(cat(new, "cell_mask_ms_%s" % k)),
                                                 nnz_dp=new[0]["nnz_dp_%s" % k][0])
    if parent:
        pf, pr = stat(cat(parent, "finish_ms_sort")), parts_stat(cat(parent, "refold_plain"))
        out["parent"] = dict(fresh_finish_ms_sort=pf, refold_plain=pr)
        out["finish_median_within_parent_spread"] = out["fresh_finish_ms_sort"]["median"] <= pf["max"]
        out["plain_refold_median_within_parent_spread"] = out["refold_plain"]["total_ms"]["median"] <= pr["total_ms"]["max"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
