"""The quality region a base-quality floor (xck_config.min_baseq) adds to a host-parsed chunk's SoA block (csrc/bam_records.cpp soa_reserve /
parse_record), without a GPU: tools/asan/qual_pack_check.cpp is a stand-alone program built with -fsanitize=address,undefined that lays
out and parses random chunks with and without qualities, with and without the name trailer, and checks that every kept record's bytes
and pad are where 2 * seq_off says, inside the block and disjoint; that the layout without qualities is the present one; and that the
name trailer is intact when both are on."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_quality_region_under_asan():
    asan = os.path.join(ROOT, "tools", "asan")
    r = subprocess.run(["make", "-C", asan, "qual_pack_check"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]                      # (a machine without the sanitizer runtime fails here: the check is part of the change)
    r = subprocess.run([os.path.join(asan, "qual_pack_check")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "the name trailer intact" in r.stdout and "ERROR" not in r.stderr, r.stdout
