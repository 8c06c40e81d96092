"""Worker of tests/test_gpu_feature_summary.py, run under torch.distributed.run: every rank makes the same front-end call of a golden
case with XCK_FEATURE_SUMMARY=1 in its environment; the ranks sum their tables and rank 0 writes feature_summary.tsv (and, for the
pileup, snp_summary.tsv) next to the matrices."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import util  # noqa: E402

name, tmp = sys.argv[1], sys.argv[2]
assert os.environ.get("XCK_FEATURE_SUMMARY") == "1"
case, ddir, odir, exp = util.load_case(name, tmp)
from xcltk_amd.baf.fc.main import afc_wrapper  # noqa: E402
from xcltk_amd.rdr.fc.main import fc_wrapper  # noqa: E402
basefc = case["kind"] == "basefc"
ret = fc_wrapper(**case["kwargs"]) if basefc else afc_wrapper(**case["kwargs"])
assert ret == 0
import torch.distributed as dist  # noqa: E402
dist.barrier()
if dist.get_rank() == 0:
    for base in ["feature_summary.tsv"] if basefc else ["xcltk.feature_summary.tsv", "xcltk.snp_summary.tsv"]:
        assert os.path.isfile(os.path.join(odir, base)), base
    print("FEATURE_SUMMARY_DIST_OK %s WORLD %d" % (name, dist.get_world_size()))
dist.destroy_process_group()
