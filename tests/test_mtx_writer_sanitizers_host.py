"""The .mtx writer (csrc/mtx_writer.cpp) under sanitizers, without a GPU: tools/asan/mtx_writer_check.cpp is a stand-alone program that
writes random matrices at random chunk sizes and thread counts through the mapped path, through the pipeline and line by line with
snprintf, compares the three texts, and runs the fill against a mapping that ends in a PROT_NONE page - built once with
-fsanitize=address,undefined and once with -fsanitize=thread.  Nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("exe", ["mtx_writer_check", "mtx_writer_check_tsan"])
def test_both_paths_write_the_same_text_and_the_fill_stays_inside_it(exe):
    asan = os.path.join(ROOT, "tools", "asan")
    r = subprocess.run(["make", "-C", asan, exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and any(("cannot find -l" + n) in r.stdout for n in ("asan", "ubsan", "tsan")):
        pytest.skip("no sanitizer runtime on this machine")
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([os.path.join(asan, exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "three texts identical, guard page untouched" in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
