#!/usr/bin/env python
"""What the packed reference costs: xck_find_candidates on this tree's library beside a library built from the parent commit
(--parent-lib), xck_find_candidates_ref beside the plain call of the same process, and xck_set_contig_ref for chr1 beside a plain pinned
host-to-device copy of the same bytes.

The workload is that of tools/base_tally_time.py (the HBM-resident 500 M reads of `bench.py --resident-only`, hg38's contigs, one BAF handle
with XCK_F_BASE_TALLY).  A measuring process pushes the batches once, finishes, and then times, after --warmup calls (2), --repeats calls
of each of
  find_candidates at a min_count no position reaches   the count pass and the scan alone: nothing is emitted or copied out
  find_candidates at min_count 20 / min_maf 0.1        (--emit-repeats calls, one warm-up: the time is the copy-out of the lists)
and, on this tree's library, the same two through xck_find_candidates_ref under a genome of uniformly drawn A C G T at 60 bases a line,
loaded contig by contig with xck_set_contig_ref from pageable host memory; chr1's load is repeated --warmup + --repeats times and timed, and
so is a torch copy of the same bytes from a pinned tensor to the device - the floor of any staging scheme.
The variants alternate: --rounds rounds of parent, new, each in a process of its own; rounds x repeats is at least 6.

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

LINE = 60


def fasta_body(length, seed):
    """uint8 array: `length` uniformly drawn bases at LINE a line, from the first base through the last"""
    import numpy as np
    n_lines = (length + LINE - 1) // LINE
    a = np.empty((n_lines, LINE + 1), dtype=np.uint8)
    a[:, :LINE] = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, (n_lines, LINE), dtype=np.uint8)]
    a[:, LINE] = 10
    return a.reshape(-1)[:(length - 1) // LINE * (LINE + 1) + (length - 1) % LINE + 1]


def timed(fn, warmup, repeats):
    ms = []
    for k in range(warmup + repeats):
        t0 = time.perf_counter()
        out = fn()
        if k >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return ms, out


def measure(args):
    from xcltk_amd import capi
    new = args.role == "new"
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
    lens = dict(zip(soa.HG38_NAMES, soa.HG38_LENGTHS))
    eng = Engine(capi.XCK_MODE_BAF, names, regions, args.cells, snps=snps, device=0, min_mapq=20, min_len=30, incl_flag=0, excl_flag=772, no_orphan=True,
                 min_count=1, min_maf=0, base_tally=True, contig_len=[lens[n] for n in names])
    for c, s, e in batches:
        eng.push(soa_torch.device_batch(capi, arrays, c, s, e, True), device_resident=True)
    eng.finish(copy=False)
    plain = lambda mc: (lambda: eng.find_candidates(mc, 0.1)) if not new else (lambda: eng.find_candidates(mc, 0.1, use_ref=False))
    out = dict(role=args.role, lib=args.lib or "this tree", workload=dict(reads=args.reads, cells=args.cells, genes=args.genes, snps=args.snps),
               warmup=args.warmup, repeats=args.repeats, emit_repeats=args.emit_repeats, device=torch.cuda.get_device_name(0))
    ms, none = timed(plain(1e12), args.warmup, args.repeats)
    assert len(none["pos"]) == 0
    out["plain_no_candidate_ms"] = stat(ms); out["plain_no_candidate_ms_all"] = [round(x, 3) for x in ms]
    ms, cand = timed(plain(20), 1, args.emit_repeats)
    out["plain_emit_ms"] = stat(ms); out["candidates"] = int(len(cand["pos"])); out["positions_covered"] = int(cand["positions_covered"])
    del cand
    if new:
        t0 = time.perf_counter()
        raw_bytes = 0
        for c in eng.tally_contigs():
            body = fasta_body(int(eng.contig_len[c]), 7 + c)
            raw_bytes += len(body)
            eng._check(eng.lib.xck_set_contig_ref(eng.h, c, C.c_void_p(body.ctypes.data), len(body), LINE, LINE + 1), "xck_set_contig_ref")
        out["genome"] = dict(contigs=len(eng.tally_contigs()), raw_bytes=raw_bytes, generate_and_load_s=round(time.perf_counter() - t0, 2))
        ms, none = timed(lambda: eng.find_candidates(1e12, 0.1, use_ref=True), args.warmup, args.repeats)
        assert len(none["pos"]) == 0 and sum(none["ref_stats"].values()) == 0
        out["ref_no_candidate_ms"] = stat(ms); out["ref_no_candidate_ms_all"] = [round(x, 3) for x in ms]
        ms, cand = timed(lambda: eng.find_candidates(20, 0.1, use_ref=True), 1, args.emit_repeats)
        out["ref_emit_ms"] = stat(ms); out["ref_candidates"] = int(len(cand["pos"])); out["ref_stats"] = cand["ref_stats"]
        assert sum(cand["ref_stats"].values()) == out["candidates"]
        del cand
        # chr1 again, timed, beside the plain pinned copy of the same bytes
        c1 = max(eng.tally_contigs(), key=lambda c: int(eng.contig_len[c]))
        body = fasta_body(int(eng.contig_len[c1]), 7 + c1)
        ms, _ = timed(lambda: eng._check(eng.lib.xck_set_contig_ref(eng.h, c1, C.c_void_p(body.ctypes.data), len(body), LINE, LINE + 1), "xck_set_contig_ref"),
                      args.warmup, args.repeats)
        pinned = torch.from_numpy(body).pin_memory()
        dst = torch.empty(len(body), dtype=torch.uint8, device=device)

        def copy():
            dst.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize()
        ms0, _ = timed(copy, args.warmup, args.repeats)
        gbs = lambda v: round(len(body) * 1e-6 / v, 2)
        out["set_contig_ref"] = dict(contig=names[c1], positions=int(eng.contig_len[c1]), raw_bytes=len(body), ms=stat(ms), gb_per_s_median=gbs(stat(ms)["median"]),
                                     pinned_copy_ms=stat(ms0), pinned_copy_gb_per_s_median=gbs(stat(ms0)["median"]))
    eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=500_000_000)
    ap.add_argument("--cells", type=int, default=10000)
    ap.add_argument("--genes", type=int, default=33472)
    ap.add_argument("--snps", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3, help="timed calls per measuring process")
    ap.add_argument("--emit-repeats", type=int, default=2, help="timed calls at min_count 20 / min_maf 0.1 per measuring process (the copy-out dominates)")
    ap.add_argument("--rounds", type=int, default=2, help="rounds of (parent, new), each variant in a process of its own")
    ap.add_argument("--parent-lib", default=None, help="libxck.so built from the parent commit")
    ap.add_argument("--out", default=None, help="also write what is printed to this file")
    ap.add_argument("--role", default=None, choices=["parent", "new"], help="(internal) measure in this process")
    ap.add_argument("--lib", default=None, help="(internal) the library of a measuring process")
    args = ap.parse_args()
    if args.warmup < 2 or args.repeats * args.rounds < 6:
        sys.exit("at least two warm-up calls and six timed calls per variant (--repeats x --rounds)")
    if args.role:
        return measure(args)
    variants = ([("parent", args.parent_lib)] if args.parent_lib else []) + [("new", None)]
    lines, none, last = [], {}, {}
    for rnd in range(args.rounds):
        for name, lib in variants:
            cmd = [sys.executable, os.path.abspath(__file__), "--role", name, "--reads", str(args.reads), "--cells", str(args.cells), "--genes", str(args.genes),
                   "--snps", str(args.snps), "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--emit-repeats", str(args.emit_repeats),
                   "--rounds", str(args.rounds)] + (["--lib", lib] if lib else [])
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:                              # (nothing more is started on the GPU behind a process that failed)
                sys.exit("%s failed (%d):\n%s" % (name, r.returncode, r.stderr[-3000:]))
            got = last[name] = json.loads(r.stdout.strip().splitlines()[-1])
            none.setdefault(name, []).extend(got["plain_no_candidate_ms_all"])
            if name == "new":
                none.setdefault("new_ref", []).extend(got["ref_no_candidate_ms_all"])
            lines.append("round %d %s %s" % (rnd, name, json.dumps(got)))
            print(lines[-1]); sys.stdout.flush()
    summary = dict(tool="tools/refseq_time.py", no_candidate_ms={k: stat(v) for k, v in none.items()})
    if "parent" in none:
        p = summary["no_candidate_ms"]["parent"]
        summary["plain_inside_parent_spread"] = bool(p["min"] <= summary["no_candidate_ms"]["new"]["median"] <= p["max"])
    summary["ref_adds_ms"] = round(summary["no_candidate_ms"]["new_ref"]["median"] - summary["no_candidate_ms"]["new"]["median"], 3)
    for k in ("plain_emit_ms", "ref_emit_ms", "candidates", "ref_candidates", "ref_stats", "set_contig_ref", "genome"):
        if k in last.get("new", {}):
            summary[k] = last["new"][k]
    lines.append("summary %s" % json.dumps(summary))
    print(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
