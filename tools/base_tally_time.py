#!/usr/bin/env python
"""What the pseudo-bulk base tallies cost: the batches' kernel work of one BAF handle with XCK_F_BASE_TALLY beside the same handle without
it, on this tree's library and - with --parent-lib - on a library built from the parent commit, and the time of xck_find_candidates.

The workload is the HBM-resident one of `bench.py --resident-only` (xcltk_amd/synth/soa_torch.py: 500 M reads, 10 k cells, 1 M SNPs, the
contigs of hg38), sequences included.  A measuring process makes one handle and, after --warmup passes (2), times --repeats passes of
reset, push of the device-resident batches and flush: every batch's kernels (tile records, join, and under the flag the tally pass) on the
host clock from the first push to the end of the flush, and the join alone by HIP events (xck_stats.ms_join; the tally pass runs behind
the second event and is not in it).  Under the flag xck_finish and xck_find_candidates (min_count 20, min_maf 0.1) follow the last pass,
the latter --repeats times, and as often with a min_count that no position reaches (the count pass and the scan alone: nothing is emitted
or copied out).  The variants alternate: --rounds rounds of parent, off, on, each in a process of its own on one GPU;
rounds x repeats is at least 5 timed passes per variant.

Without --role the tool starts the measuring processes one after the other, prints their JSON lines and a closing comparison, and writes
all of it to --out.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.refold_time import stat  # noqa: E402


def measure(args):
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
    regions, snps, names = soa.make_tables(args.genes, args.snps, soa.HG38_LENGTHS, seed=2)
    arrays, batches = soa_torch.gen_reads_device(regions, names, args.reads, args.cells, seed=100, device=device)
    torch.cuda.synchronize()
    on = args.role == "on"
    lens = dict(zip(soa.HG38_NAMES, soa.HG38_LENGTHS))
    kw = dict(base_tally=True, contig_len=[lens[n] for n in names]) if on else {}   # (a parent-commit library has no such flag)
    eng = Engine(capi.XCK_MODE_BAF, names, regions, args.cells, snps=snps, device=0, min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True,
                 min_count=1, min_maf=0, **kw)
    bs = [soa_torch.device_batch(capi, arrays, c, s, e, True) for c, s, e in batches]
    ms_wall, ms_join = [], []
    for rep in range(args.warmup + args.repeats):
        eng.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in bs:
            eng.push(b, device_resident=True)
        eng.flush()
        dt = (time.perf_counter() - t0) * 1e3
        if rep >= args.warmup:
            ms_wall.append(dt); ms_join.append(eng.stats()["ms_join"])
    out = dict(role=args.role, lib=args.lib or "this tree", workload=dict(reads=args.reads, cells=args.cells, genes=args.genes, snps=args.snps, batches=len(bs)),
               warmup=args.warmup, repeats=args.repeats, device=torch.cuda.get_device_name(0), n_hits=int(eng.stats()["n_hits"]),
               pass_wall_ms=stat(ms_wall), pass_join_ms=stat(ms_join), pass_wall_ms_all=[round(x, 3) for x in ms_wall])
    if on:
        t0 = time.perf_counter()
        eng.finish(copy=False)
        out["finish_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        ms_fc = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            cand = eng.find_candidates(20, 0.1)
            ms_fc.append((time.perf_counter() - t0) * 1e3)
        out["find_candidates_wall_ms"] = stat(ms_fc)
        out["candidates"] = int(len(cand["pos"])); out["positions_covered"] = int(cand["positions_covered"])
        ms_fc0 = []                                            # a min_count no position reaches: the count pass and the scan alone, nothing emitted or copied
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            none = eng.find_candidates(1e12, 0.1)
            ms_fc0.append((time.perf_counter() - t0) * 1e3)
        assert len(none["pos"]) == 0
        out["find_candidates_no_candidate_wall_ms"] = stat(ms_fc0)
        out["base_tally_stats"] = eng.base_tally_stats()
        out["table_bytes"] = int(sum(16 * int(l) for l in eng.contig_len))
    eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500_000_000)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=33472)
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5, help="timed passes per measuring process")
    ap.add_argument("--rounds", type=int, default=1, help="rounds of (parent, off, on), each variant in a process of its own")
    ap.add_argument("--parent-lib", default=None, help="libxck.so built from the parent commit: measured without the flag, for the comparison")
    ap.add_argument("--out", default=None, help="also write what is printed to this file")
    ap.add_argument("--role", default=None, choices=["off", "on"], help="(internal) measure in this process")
    ap.add_argument("--lib", default=None, help="(internal) the library of a measuring process")
    args = ap.parse_args()
    if args.warmup < 2 or args.repeats * args.rounds < 5:
        sys.exit("at least two warm-up passes and five timed passes per variant (--repeats x --rounds)")
    if args.role:
        return measure(args)
    variants = ([("parent_off", "off", args.parent_lib)] if args.parent_lib else []) + [("new_off", "off", None), ("new_on", "on", None)]
    lines, wall, join, last = [], {}, {}, {}
    for rnd in range(args.rounds):
        for name, role, lib in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--role", role, "--reads", str(args.reads), "--cells", str(args.cells), "--genes", str(args.genes),
                   "--snps", str(args.snps), "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--rounds", str(args.rounds)] +(["--lib", lib] if lib else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:                              # (nothing more is started on the GPU behind a process that failed)
                sys.exit("%s failed (%d):\n%s" % (name, r.returncode, r.stderr[-3000:]))
            got = last[name] = json.loads(r.stdout.strip().splitlines()[-1])
            wall.setdefault(name, []).extend(got["pass_wall_ms_all"]); join.setdefault(name, []).append(got["pass_join_ms"]["median"])
            lines.append("round %d %s %s" % (rnd, name, json.dumps(got)))
            print(lines[-1]); sys.stdout.flush()
    summary = dict(tool="tools/base_tally_time.py", pass_wall_ms={k: stat(v) for k, v in wall.items()}, pass_join_ms_medians=join)
    summary["flag_adds_ms_per_pass"] = round(summary["pass_wall_ms"]["new_on"]["median"] - summary["pass_wall_ms"]["new_off"]["median"], 3)
    if "parent_off" in wall:
        p = summary["pass_wall_ms"]["parent_off"]
        summary["off_inside_parent_spread"] = bool(p["min"] <= summary["pass_wall_ms"]["new_off"]["median"] <= p["max"])
    for k in ("find_candidates_wall_ms", "find_candidates_no_candidate_wall_ms", "candidates", "positions_covered"):
        if k in last.get("new_on", {}):
            summary[k] = last["new_on"][k]
    lines.append("summary %s" % json.dumps(summary))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
