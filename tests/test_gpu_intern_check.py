"""The device intern table alone (csrc/intern_dev.hip): xck_gpu_intern_check (tools/gpu_intern_check.hip) feeds name lists to the insert
routine both kernels of the ingest use - 64 copies of one name in one wave, 32 names twice in one wave, names of 1 to 254 bytes, names
that differ in their last byte or only in length, high and zero bytes, 20,000 random names with 4 hash bits kept - and checks on the
host that keys are equal exactly where the names are, that ids stay below the distinct names plus the launches' lanes, and that a
table grown from 64 slots gives the partition of one sized in advance.  Reference boundary: string equality on the host (std::map)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_intern_table_partitions_names_exactly():
    exe = os.path.join(ROOT, "xcltk_amd", "csrc", "xck_gpu_intern_check")
    r = subprocess.run(["timeout", "-k", "10", "120", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "all checks held" in r.stdout and r.stdout.count(": ok") == 6
