#!/usr/bin/env python
"""local_phase_time.py - the fixture's 120 synthetic regions plus one region of 200 SNPs x 3000 cells through the device path
(xck_local_phase) and through the host path (baf/fc/phasing.py), each once; writes a JSON with the seconds per path, regions per
second, levels and the device's per-stage milliseconds.

Usage: python tools/local_phase_time.py out.json [--skip-host]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def problem():
    import local_phase_util as U
    from make_local_phase_fixture import dense_problem, draw_region
    args, _ = U.load_problem("synthetic")
    AD, DP, rh, pos = draw_region(np.random.RandomState(29), 3000, 200, 1.0, 0.25)
    big = dense_problem([(AD, DP, np.arange(200), pos)], 3000, ref_hap=rh)
    n_cols, n_snps, nnz, n_slots = len(args["col_ptr"]) - 1, len(args["ref_hap"]), len(args["cell"]), len(args["slot_col"])
    cat = np.concatenate
    return dict(n_cells=3000, cell_enabled=None,
                col_ptr=cat([args["col_ptr"], big["col_ptr"][1:] + nnz]), cell=cat([args["cell"], big["cell"]]).astype(np.int32),
                ad=cat([args["ad"], big["ad"]]).astype(np.int32), dp=cat([args["dp"], big["dp"]]).astype(np.int32),
                ref_hap=cat([args["ref_hap"], big["ref_hap"]]), alt_hap=cat([args["alt_hap"], big["alt_hap"]]),
                reg_ptr=cat([args["reg_ptr"], big["reg_ptr"][1:] + n_slots]), slot_col=cat([args["slot_col"], big["slot_col"] + n_cols]),
                slot_snp=cat([args["slot_snp"], big["slot_snp"] + n_snps]), slot_pos=cat([args["slot_pos"], big["slot_pos"]]))


def main(out_fn, skip_host):
    from xcltk_amd import capi
    from xcltk_amd.baf.fc.phasing_dev import host_phase_slots
    p = problem()
    n_regions = len(p["reg_ptr"]) - 1
    out = dict(n_regions=n_regions, shape="120 fixture regions (<= 130 SNPs, <= 400 cells) + 1 region of 200 SNPs x 3000 cells")
    capi.local_phase(**{k: (v[:2] if k == "reg_ptr" else v) for k, v in p.items()})      # (first call: runtime start-up, code object load)
    t = time.time()
    dev = capi.local_phase(**p)
    out["device_s"] = time.time() - t
    out["device_regions_per_s"] = n_regions / out["device_s"]
    out["levels"], out["blocks"], out["device_stage_ms"] = dev["n_levels"], dev["n_blocks"], dev["ms"]
    if not skip_host:
        t = time.time()
        host = host_phase_slots(**p)
        out["host_s"] = time.time() - t
        out["host_regions_per_s"] = n_regions / out["host_s"]
        out["speedup"] = out["host_s"] / out["device_s"]
        out["equal"] = bool(all(np.array_equal(dev[k], host[k]) for k in ("kept", "flip", "status", "ref_hap", "alt_hap")))
    with open(out_fn, "w") as fp:
        json.dump(out, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1], "--skip-host" in sys.argv[2:])
