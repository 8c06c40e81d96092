#!/usr/bin/env python
"""What the 1-mismatch UMI collapsing costs: xck_finish of the basefc pipeline with XCK_F_UMI_COLLAPSE beside the same handle shape without
it, on this tree's library and - with --parent-lib - on a library built from the parent commit, each in a process of its own on one GPU.

The workload is the HBM-resident one of `bench.py --resident-only` (xcltk_amd/synth/soa_torch.py at BASELINE configs[2]: 500 M reads,
10 k cells, 33 k genes); --umi-len and --cells shrink the UMI pool and the number of cells, so that the (gene, cell) groups grow into the
classes of csrc/umi_collapse.h that the default workload hardly reaches.  A measuring process makes one handle; after a warm-up pass
(the first finish sizes the hit buffers and the workspaces) `--repeats` passes (at least 5) of reset, push of the device-resident
batches, flush and xck_finish are timed: the fold by HIP events (xck_stats.ms_sort: everything xck_finish runs on the compute stream
before the copy-out - under the flag the whole stage of csrc/umi_collapse.h, its count included) and the whole call on the host clock.
Under the flag the counters of xck_get_umi_dedup_stats and the library's `[xck] UMI collapsing:` line (the keys per size class) go along.

Without --role the tool starts the measuring processes one after the other, prints their JSON lines and a closing comparison, and
writes all of it to --out.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.refold_time import StderrCapture, stat  # noqa: E402

STAGE_RE = re.compile(r"\[xck\] UMI collapsing: n=(\d+) distinct=(\d+) components=(\d+) groups=(\d+) changed=(\d+) opaque=(\d+) max group=(\d+) larger groups=(\d+) keys medium=(\d+) giant=(\d+) sort bits=(\d+)")


def measure(args):
    os.environ["XCK_DEBUG_TIMING"] = "1"                       # (a handle reads its knobs at xck_create)
    os.environ.pop("XCK_UMI_DEDUP", None)
    from xcltk_amd import capi
    if args.lib:
        os.environ["XCK_LIB"] = args.lib
        capi._preload_torch_hip()                              # (as capi.load() does: the library binds to the HIP runtime torch ships)
        probe = C.CDLL(args.lib)                               # (a parent-commit library lacks the calls this commit adds: not bound)
        capi.SYMBOLS[:] = [s for s in capi.SYMBOLS if hasattr(probe, s[0])]
    import torch
    from xcltk_amd.engine import Engine
    from xcltk_amd.synth import soa, soa_torch
    device = torch.device("cuda", 0)
    regions, _, names = soa.make_tables(args.genes, 0, soa.HG38_LENGTHS, seed=2)
    arrays, batches = soa_torch.gen_reads_device(regions, names, args.reads, args.cells, seed=100, device=device, umi_len=args.umi_len, with_seq=False)
    torch.cuda.synchronize()
    on = args.role == "1mm_all"
    eng = Engine(capi.XCK_MODE_BASEFC, names, regions, args.cells, device=0, min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True,
                 min_include=0.9, **({"umi_dedup": "1mm_all"} if on else {}))   # (a parent-commit Engine has no such argument)
    bs = [soa_torch.device_batch(capi, arrays, c, s, e, False) for c, s, e in batches]
    cap = StderrCapture()
    ms_sort, ms_wall, text, nnz = [], [], "", 0
    for rep in range(args.repeats + 1):                        # pass 0 warms up
        eng.reset()
        for b in bs:
            eng.push(b, device_resident=True)
        eng.flush()
        torch.cuda.synchronize()
        cap.start()
        t0 = time.perf_counter()
        res = eng.finish(copy=False)
        dt = (time.perf_counter() - t0) * 1e3
        text = cap.stop()
        nnz = int(len(res["count"][0]))
        if rep:
            ms_sort.append(eng.stats()["ms_sort"]); ms_wall.append(dt)
    st = eng.stats()
    out = dict(role=args.role, lib=args.lib or "this tree", workload=dict(reads=args.reads, cells=args.cells, genes=args.genes, umi_len=args.umi_len), repeats=args.repeats,
               device=torch.cuda.get_device_name(0), keys_in_hbm=int(st["n_hits_unique"]), nnz=nnz, fold_path=int(st["fold_path"]),
               finish_ms_sort=stat(ms_sort), finish_wall_ms=stat(ms_wall))
    if on:
        us = out["umi_dedup_stats"] = eng.umi_dedup_stats()
        out["fraction_merged"] = round(1.0 - us["molecules"] / us["keys"], 6) if us["keys"] else 0.0
        m = STAGE_RE.search(text)
        if m:
            g = out["stage"] = dict(zip(("n", "distinct", "components", "groups", "changed", "opaque", "max_group", "larger_groups", "keys_medium", "keys_giant", "sort_bits"),
                                        (int(x) for x in m.groups())))
            nd = max(g["distinct"], 1)
            out["key_share"] = dict(small=round(1.0 - (g["keys_medium"] + g["keys_giant"]) / nd, 6), medium=round(g["keys_medium"] / nd, 6), giant=round(g["keys_giant"] / nd, 6))
    eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500_000_000)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=33472)
    ap.add_argument("--umi-len", type=int, default=12, help="bases per UMI: the pool is 4^L")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libxck.so built from the parent commit: measured without the flag, for the comparison")
    ap.add_argument("--out", default=None, help="also write what is printed to this file")
    ap.add_argument("--role", default=None, choices=["off", "1mm_all"], help="(internal) measure in this process")
    ap.add_argument("--lib", default=None, help="(internal) the library of a measuring process")
    args = ap.parse_args()
    if args.repeats < 5:
        sys.exit("--repeats: at least 5")
    if args.role:
        return measure(args)
    runs = ([("parent_off", "off", args.parent_lib)] if args.parent_lib else []) + [("new_off", "off", None), ("new_on", "1mm_all", None)]
    lines, got = [], {}
    for name, role, lib in runs:
        cmd = [sys.executable, os.path.abspath(__file__), "--role", role, "--reads", str(args.reads), "--cells", str(args.cells), "--genes", str(args.genes), "--umi-len", str(args.umi_len),
               "--repeats", str(args.repeats)] + (["--lib", lib] if lib else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:                                  # (nothing more is started on the GPU behind a process that failed)
            sys.exit("%s failed (%d):\n%s" % (name, r.returncode, r.stderr[-3000:]))
        got[name] = json.loads(r.stdout.strip().splitlines()[-1])
        lines.append("%s %s" % (name, json.dumps(got[name])))
        print(lines[-1]); sys.stdout.flush()
    med = {k: v["finish_ms_sort"]["median"] for k, v in got.items()}
    summary = dict(tool="tools/umi_dedup_time.py", finish_ms_sort_median=med, flag_adds_ms=round(med["new_on"] - med["new_off"], 3))
    if "parent_off" in med:
        summary["off_vs_parent_ms"] = round(med["new_off"] - med["parent_off"], 3)
        summary["parent_spread_ms"] = [got["parent_off"]["finish_ms_sort"]["min"], got["parent_off"]["finish_ms_sort"]["max"]]
    lines.append("summary %s" % json.dumps(summary))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
