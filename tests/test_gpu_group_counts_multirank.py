"""XCK_CELL_GROUPS in a contig-sharded run of two ranks (sharing the one GPU of the test box, gloo): in the sharded output form every
rank sums its own rows and the ranks write the group files together - byte for byte the files of the single-process run, which
test_gpu_group_counts.py pins to the reference's matrices; the gather form writes none and says so once."""
import os
import subprocess
import sys

import numpy as np
import pytest

import group_util as G
import util
from test_gpu_multirank import _free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "group_counts_dist_worker.py")
GROUP_FILES = {"basefc": ["groups.tsv", "matrix.groups.mtx"], "baf": ["xcltk.groups.tsv"] + ["xcltk.%s.groups.mtx" % k for k in ("AD", "DP", "OTH")]}


def _group_file(tmp_path, name):
    case, ddir, _, _ = util.load_case(name, tmp_path)
    bcs = sorted(x.strip() for x in open(case["kwargs"]["barcode_fn"]))
    gn = ["c", "a", "b"]
    lines = ["%s\t%s\n" % (bc, gn[(3 * i + i // 4) % 3]) for i, bc in enumerate(bcs) if i % 6 != 2]
    fn = str(tmp_path / "cell_groups.tsv")
    open(fn, "w").write("".join(lines))
    return fn, case["kind"]


def _run(name, tmp, world, groups_fn, gather=False):
    """One child under its own time limit; -> its output.  Nothing further is started after a child that failed."""
    os.makedirs(str(tmp), exist_ok=True)
    env = dict(os.environ, XCK_CELL_GROUPS=groups_fn, XCK_DIST_BACKEND="gloo", XCK_DEVICE="0", MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0",
               XCK_DIST_GATHER="1" if gather else "0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "XCK_DIST_FORCE"):
        env.pop(k, None)
    cmd = [sys.executable, WORKER, name, str(tmp)] if world == 1 else \
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % world, "--master-addr", "127.0.0.1",
         "--master-port", _free_port(), WORKER, name, str(tmp)]
    r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    tb = [ln for ln in r.stdout.splitlines() if "Error" in ln or "error" in ln or "File \"/" in ln]
    assert r.returncode == 0 and "GROUPS_OK " + name in r.stdout, "rc %d\n%s" % (r.returncode, "\n".join(tb[-40:]) or r.stdout[-2000:])
    return r.stdout


@pytest.mark.parametrize("name", ["multibam_basefc", "multibam_baf"])
def test_two_ranks_write_the_single_process_group_files(name, tmp_path):
    fn, kind = _group_file(tmp_path, name)
    _run(name, tmp_path / "one", 1, fn)
    _run(name, tmp_path / "two", 2, fn)
    d1, d2 = (os.path.join(str(tmp_path / w), "out_" + name) for w in ("one", "two"))
    for f in GROUP_FILES[kind]:
        a, b = (open(os.path.join(d, f), "rb").read() for d in (d1, d2))
        assert a == b, f
    dims, coo = G.read_mtx(os.path.join(d2, GROUP_FILES[kind][1]))
    assert dims[1] == 3 and len(coo[0]) > 10 and len(np.unique(coo[1])) == 3


def test_gather_form_writes_no_group_files_and_says_so_once(tmp_path):
    name = "multibam_baf"
    fn, kind = _group_file(tmp_path, name)
    out = _run(name, tmp_path / "gather", 2, fn, gather=True)
    d = os.path.join(str(tmp_path / "gather"), "out_" + name)
    assert not [f for f in os.listdir(d) if "groups" in f]
    assert len([ln for ln in out.splitlines() if "writes no group files" in ln]) == 1, out[-2000:]
