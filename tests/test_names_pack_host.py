"""The host code device-names mode adds to the decoder (csrc/bam_records.cpp: the walk's name byte counts, the trailer behind the SoA columns,
parse_part's packing of the names it no longer interns), without a GPU: tools/asan/names_pack_check.cpp is a stand-alone program
built with -fsanitize=address,undefined that lays out and parses random chunks with names of 0 to 254 bytes and checks that every
kept record's item is what the device table needs - length 0 exactly where the key is final, otherwise the name's own bytes, inside
the block, no two names overlapping - and that the host table stays empty.  Reference boundary: none (the reference keys a read by
pysam's query_name); this pins the hand-over between the two halves of one mode."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_name_trailer_is_packed_as_the_device_table_needs_it_under_asan():
    asan = os.path.join(ROOT, "tools", "asan")
    r = subprocess.run(["make", "-C", asan, "names_pack_check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and ("cannot find -lasan" in r.stdout or "cannot find -lubsan" in r.stdout):
        pytest.skip("no sanitizer runtime on this machine")
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([os.path.join(asan, "names_pack_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "names packed" in r.stdout and "ERROR" not in r.stderr, r.stdout
