"""Worker of test_gpu_group_counts_multirank.py: one golden case through its front-end with XCK_CELL_GROUPS set by the test, as a plain
single process or as one rank under torch.distributed.run.  Rank 0 checks the cell files against the reference's and prints
GROUPS_OK <name>; the test compares the group files of the runs."""
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import util  # noqa: E402

logging.basicConfig(level=logging.INFO, stream=sys.stdout, format="%(message)s")
name, tmp = sys.argv[1], sys.argv[2]
case, ddir, odir, exp = util.load_case(name, tmp)
from xcltk_amd.baf.fc.main import afc_wrapper  # noqa: E402
from xcltk_amd.rdr.fc.main import fc_wrapper  # noqa: E402
ret = fc_wrapper(**case["kwargs"]) if case["kind"] == "basefc" else afc_wrapper(**case["kwargs"])
assert ret == 0
multi = int(os.environ.get("WORLD_SIZE", "1")) > 1
if multi:
    import torch.distributed as dist  # noqa: E402
    dist.barrier()
if not multi or dist.get_rank() == 0:
    for f in os.listdir(exp):                              # the cell files are the reference's, group files or not
        assert open(os.path.join(odir, f), "rb").read() == open(os.path.join(exp, f), "rb").read(), f
    print("GROUPS_OK", name, flush=True)
if multi:
    dist.destroy_process_group()
