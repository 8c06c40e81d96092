"""The host logic of the device parse path (csrc/parse_dev.h summaries_to_batches: per-block summaries of the device's record walk ->
the chunk's batches) against the decoder's own layout (csrc/bam_records.cpp run_part + layout_chunk), without a GPU: tools/asan/
parse_layout_check.cpp is a stand-alone program built with -fsanitize=address,undefined that walks random chunks both ways - the
summaries come from a host restatement of the walk kernel - and compares batch lists, ordinals, totals, per-batch sizes and the last
record.  Reference boundary: none (the reference iterates records one by one); this pins two implementations of one layout."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_summaries_to_batches_equals_layout_chunk_under_asan():
    asan = os.path.join(ROOT, "tools", "asan")
    r = subprocess.run(["make", "-C", asan, "parse_layout_check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and ("cannot find -lasan" in r.stdout or "cannot find -lubsan" in r.stdout):
        pytest.skip("no sanitizer runtime on this machine")
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([os.path.join(asan, "parse_layout_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "batches identical" in r.stdout and "ERROR" not in r.stderr, r.stdout
