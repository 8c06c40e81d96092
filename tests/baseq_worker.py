"""Child process of tests/test_gpu_min_baseq.py: what it runs sees XCK_MIN_BASEQ (or not) in its environment from the start, as a
front-end's user sets it.
  afc <golden case> <tmp> [<dataset dir>]   afc_wrapper on a golden BAF case, its BAMs taken from <dataset dir> when given (a copy with
                                            rewritten qualities); the output directory is printed"""
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import util  # noqa: E402

what, name, dst = sys.argv[1:4]
assert what == "afc"
from xcltk_amd.baf.fc.main import afc_wrapper  # noqa: E402
logging.basicConfig(level=logging.INFO, stream=sys.stdout)           # (the front-end's one-line reports are logging.info)
case, ddir, odir, exp = util.load_case(name, dst, sys.argv[4] if len(sys.argv) > 4 else None)
assert afc_wrapper(**case["kwargs"]) == 0
print("AFC_DONE", odir)
