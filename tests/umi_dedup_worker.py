"""Child process of tests/test_gpu_umi_dedup.py: what it runs sees XCK_UMI_DEDUP (or not) in its environment from the start, as a
front-end's user sets it.  Also the worker of its torch.distributed.run calls: every rank makes the same front-end call.
  engine <case> <key bits> <out.json>   a case of tests/umi_dedup_cases.py through a handle made WITHOUT the flag; a failed xck_create
                                        leaves {"create_failed": code, "error": text}
  fc <regions.tsv> <out dir>            fc_wrapper on the two-contig golden dataset `multibam` with the given region file"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import util  # noqa: E402

what = sys.argv[1]
if what == "engine":
    import umi_dedup_cases as UD
    from xcltk_amd import capi
    from xcltk_amd.engine import Engine, XckError
    name, key_bits, dst = sys.argv[2], int(sys.argv[3]), sys.argv[4]
    c = UD.case(name, key_bits)
    try:
        with Engine(capi.XCK_MODE_BASEFC, c.names, c.regions, c.n_cells, flags=capi.XCK_F_FORCE_KEY128 if key_bits == 128 else 0, **UD.KW) as eng:
            for d in c.batches:
                eng.push(UD.batch_of(d)[0])
            got = eng.finish()
            out = dict(stats=eng.umi_dedup_stats(), count=[a.tolist() for a in got["count"]])
    except XckError as e:
        out = dict(create_failed=e.code, error=str(e))
    with open(dst, "w") as fp:
        json.dump(out, fp)
    print("ENGINE_DONE")
else:
    import logging
    from xcltk_amd.rdr.fc.main import fc_wrapper
    logging.basicConfig(level=logging.INFO, stream=sys.stdout)       # (the front-end's one-line reports are logging.info)
    region_fn, out_dir = sys.argv[2], sys.argv[3]
    D = os.path.join(util.GOLDEN, "datasets", "multibam")
    sam = ",".join(os.path.join(D, "possorted_%d.bam" % i) for i in (0, 1))
    ret = fc_wrapper(sam_fn=sam, barcode_fn=os.path.join(D, "barcodes.tsv"), region_fn=region_fn, out_dir=out_dir)
    print("FC_DONE", ret)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        import torch.distributed as dist
        if dist.is_initialized():
            if ret == 0:
                dist.barrier()
            dist.destroy_process_group()
