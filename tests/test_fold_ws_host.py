"""The fold workspaces (csrc/fold_ws.h: radix_fold_carve, molecule_carve, region_carve) without a GPU: tools/asan/fold_ws_check.cpp is
a stand-alone program built with -fsanitize=address,undefined that runs each carve function as the engine does - on an arena without
memory for the size, then on a malloc'ed block of exactly that size - over key sizes 8 and 16, split mode and the partition sort on
and off, 0 to 10^6 hits (2^32 - 1: sizes only), 0 and 1 SNPs, and sort / partition scratch sizes on both sides of each other.  Every
block must be non-null, aligned, inside the workspace and disjoint from the others, and is written over its stated extent; the blocks
taken after a read-back go to their remembered offsets.  The carved size never exceeds the hand-counted formula it replaced.
Reference boundary: none (the reference allocates per object); this pins the one statement of each workspace against its uses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_workspaces_carve_sound_blocks_under_asan():
    asan = os.path.join(ROOT, "tools", "asan")
    r = subprocess.run(["make", "-C", asan, "fold_ws_check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and ("cannot find -lasan" in r.stdout or "cannot find -lubsan" in r.stdout):
        pytest.skip("no sanitizer runtime on this machine")
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([os.path.join(asan, "fold_ws_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "workspaces sound" in r.stdout and "resident shapes" in r.stdout and "ERROR" not in r.stderr, r.stdout
