"""The conditions the device-names GPU tests rest on (tests/test_gpu_device_names.py, tests/test_gpu_device_names_golden.py), checked on
the CPU with oracle/pybam.py and tests/reblock.py alone - nothing of the product's decoder or device code runs here: the files hold
the pairs and name shapes they claim, the two records of every pair of the shared-names file fall into different chunks, mates of
the one-SNP file straddle chunk boundaries, the tail chunk is too short for the device, and the re-cut golden files of the UMI-less
cases have chunks the device takes."""
import collections
import os

import pytest

import device_decode_cases as D
import device_names_cases as N
import pybam
import reblock
import util

GOLDEN_NOUMI = ("c1_basefc_noumi", "c1_baf_noumi", "well_basefc", "well_basefc_orphan", "well_baf")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("names_host"))
    out = dict(shared=os.path.join(tmp, "shared.bam"), packed=os.path.join(tmp, "packed.bam"), mates=os.path.join(tmp, "mates.bam"), shapes=os.path.join(tmp, "shapes.bam"))
    out["shared_recs"] = N.write_shared(out["shared"])
    N.write_shared(out["packed"], align=False)
    out["pair_of"] = N.write_mates(out["mates"])
    out["shape_at"] = N.write_shapes(out["shapes"])
    return out


def test_shared_names_file_holds_its_pairs_in_different_chunks(files):
    _, recs = pybam.read_bam(files["shared"])
    assert len(recs) == N.N
    for i in range(N.HALF):
        a, b = recs[i], recs[i + N.HALF]
        assert a.query_name == b.query_name == "r%07d" % i and a.get_tag("CB") == b.get_tag("CB") and a.pos == b.pos
    assert len({r.query_name for r in recs}) == N.HALF
    chunk, chunks = N.chunk_of_record(files["shared"])
    assert len(chunk) == N.N and 14 <= len(chunks) <= 24
    assert all(chunk[i] != chunk[i + N.HALF] for i in range(N.HALF))
    assert min(chunk[i + N.HALF] - chunk[i] for i in range(N.HALF)) >= 6
    assert all(n >= N.MIN_BLOCKS for n in chunks[:-1]) and chunks[-1] < N.MIN_BLOCKS        # the tail chunk is always host-parsed


def test_packed_file_holds_the_same_records_across_block_boundaries(files):
    _, a = pybam.read_bam(files["shared"])
    _, b = pybam.read_bam(files["packed"])
    assert [(r.query_name, r.pos, r.get_tag("CB")) for r in a] == [(r.query_name, r.pos, r.get_tag("CB")) for r in b]
    with pytest.raises(AssertionError):                                    # records straddle blocks: the device's walk cannot end at a block's end
        reblock.block_records(files["packed"])


def test_mates_lie_one_to_three_records_apart_and_straddle_chunks(files):
    _, recs = pybam.read_bam(files["mates"])
    where = collections.defaultdict(list)
    for i, r in enumerate(recs):
        where[r.query_name].append(i)
        assert r.pos < N.SNP_POS - 1 < r.pos + 60
    assert len(where) == N.HALF and all(len(v) == 2 for v in where.values())
    assert {v[1] - v[0] for v in where.values()} == {1, 2, 3}
    for v in where.values():
        a, b = recs[v[0]], recs[v[1]]
        assert a.get_tag("CB") == b.get_tag("CB")
    chunk, chunks = N.chunk_of_record(files["mates"])
    assert sum(chunk[v[0]] != chunk[v[1]] for v in where.values()) >= 4   # pairs with one mate in each of two chunks
    assert chunks[-1] < N.MIN_BLOCKS and all(n >= N.MIN_BLOCKS for n in chunks[:-1])


def test_shapes_file_holds_every_shape_in_both_parsers_reach(files):
    _, recs = pybam.read_bam(files["shapes"])
    at = files["shape_at"]
    assert len(recs) == N.N_SHAPES_FILE
    for i, (name, cell) in at.items():
        assert recs[i].query_name == name and recs[i].get_tag("CB") == N.BARCODES[cell]
    by = collections.Counter((recs[i].query_name, recs[i].get_tag("CB")) for i in at)
    for s in N.SHAPES:
        assert by[(s, N.BARCODES[0])] == (3 if s == "ACGT" else 2) and by[(s, N.BARCODES[1])] == 1
    assert {len(s) for s in N.SHAPES} >= {0, 1, 8, 9, 254}
    assert all(r.query_name.startswith("f") and r.get_tag("CB") in N.BARCODES[2:] for i, r in enumerate(recs) if i not in at)
    chunk, chunks = N.chunk_of_record(files["shapes"])
    assert len(chunks) >= 3 and chunks[0] >= N.MIN_BLOCKS and chunks[-1] < N.MIN_BLOCKS
    first = [i for i in at if i < 200]
    last = [i for i in at if i >= N.N_SHAPES_FILE - 60]
    assert {chunk[i] for i in first} == {0} and {chunk[i] for i in last} == {len(chunks) - 1}      # a device chunk and the host-parsed tail


@pytest.mark.parametrize("name", GOLDEN_NOUMI)
def test_recut_golden_files_have_device_chunks(name, tmp_path):
    case, ddir, odir, exp, chunk_bytes, info = D.recut_case(name, tmp_path)
    p = util.oracle_params(case)
    assert p["umi_tag"] is None or p["umi_tag"].upper() == "NONE"
    n_dev = 0
    for fn in p["bam_fns"]:
        n_dev += sum(n >= D.MIN_BLOCKS for n in reblock.plan_chunks(fn, chunk_bytes))
    assert n_dev >= 1
    pred = D.predict_run(p["bam_fns"], p["region_fn"], p["snp_fn"] if case["kind"] != "basefc" else None, p["barcode_fn"], p["cell_tag"], "ZZ", chunk_bytes)
    assert pred["device_chunks"] == n_dev and pred["cls"] in ("clean", "odd")
