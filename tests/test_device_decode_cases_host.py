"""The conditions the device-decode GPU tests rest on (tests/test_gpu_device_decode_golden.py, tests/test_gpu_device_decode_crafted.py),
checked where no GPU is needed and with nothing of the product's decoder: a golden BAM re-cut into small record-aligned BGZF blocks
(tests/reblock.py) holds, for an independent reader, the very records of the original - so what the unmodified reference wrote for the
original is what a run over the re-cut file must write -, the re-cut files have the block counts that send their chunks to the device,
the class each golden case is expected to fall into follows from its records, and the crafted files hold what they are meant to hold.
Reference boundary: the reference's recorded outputs (tests/golden/cases/*/expected) and pysam's record iteration and get_tag as
restated by oracle/pybam.py; the crafted files' expectations are the oracle's (oracle/xck_oracle.c) on pybam's records."""
import json
import os

import pytest

import device_decode_cases as D
import oracle as O
import pybam
import reblock
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine

DATASETS = os.path.join(util.GOLDEN, "datasets")
FIELDS = ("tid", "pos", "flag", "mapq", "query_name", "cigartuples", "seq_nibbles", "tags", "l_seq")
# every (dataset, schedule) a GPU test uses
USED = sorted(set((ds, plan[0], plan[1]) for ds, plan in D.DATASET_PLAN.items()) |
              set((D.dataset_of(name), sch, D.shape_chunk_bytes(D.dataset_of(name), sch)) for name in D.SHAPE_CASES for sch in D.SHAPES))


@pytest.fixture(scope="module")
def recut_dirs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("recut")
    out = {}
    for ds, sch, _ in USED:
        d = str(tmp / (ds + "_" + sch))
        out[ds, sch] = (d, reblock.recut_dataset(os.path.join(DATASETS, ds), d, D.recut(sch)))
    return out


def _bams(ds):
    with open(os.path.join(DATASETS, ds, "dataset.json")) as fp:
        return json.load(fp)["bams"]


@pytest.mark.parametrize("ds,sch,chunk_bytes", USED)
def test_recut_file_reads_as_the_original(ds, sch, chunk_bytes, recut_dirs):
    d, info = recut_dirs[ds, sch]
    for bam in _bams(ds):
        refs0, recs0 = pybam.read_bam(os.path.join(DATASETS, ds, bam))
        refs1, recs1 = pybam.read_bam(os.path.join(d, bam))
        assert refs0 == refs1 and len(recs0) == len(recs1) == info[bam][0] > 0
        for a, b in zip(recs0, recs1):
            for f in FIELDS:
                assert getattr(a, f) == getattr(b, f), (bam, a.ordinal, f)
        assert not os.path.exists(os.path.join(d, bam + ".bai"))


@pytest.mark.parametrize("ds,sch,chunk_bytes", USED)
def test_recut_file_has_the_blocks_the_device_path_needs(ds, sch, chunk_bytes, recut_dirs):
    d, info = recut_dirs[ds, sch]
    share = D.SCHEDULES[sch][1]
    for bam in _bams(ds):
        path = os.path.join(d, bam)
        n_rec, n_blocks, most = info[bam]
        first, skip, blocks = reblock.block_records(path)
        assert len(reblock.read_blocks(path)) == n_blocks and sum(len(b) for b in blocks) == n_rec and max(len(b) for b in blocks) == most
        assert (skip > 0) == share                                          # the first record starts inside a block, or at a block's start
        chunks = reblock.plan_chunks(path, chunk_bytes)
        # every chunk but the file's tail is an intended one (the tail may stay on the host); there is at least one
        intended = chunks[:-1] if len(chunks) > 1 and chunks[-1] < D.HEADROOM else chunks
        assert intended and min(intended) >= D.HEADROOM > D.MIN_BLOCKS, (bam, chunks)
        if sch == "many":
            assert most > 128                                               # three k_parse rounds of 64 records
        if sch in ("single", "single_empty"):
            assert set(len(b) for b in blocks) == {0, 1}
            assert sum(1 for b in blocks if not b) >= n_rec // D.SCHEDULES[sch][2]
        if sch == "ten":
            assert most <= 11 and len(chunks) == 1


# the class of every golden case: the cases without a UMI tag are inflate-only; the phasing dataset holds 10-base ACGT UMIs only; c1, dense
# and multibam are 10x-style data in which one UMI in a few hundred holds an N, and special holds a numeric UB (value 0) on a wanted contig
EXPECTED_CLASS = {name: ("inflate-only" if name.endswith("_noumi") or name.startswith("well_") else "clean" if name.startswith("phasing_") else "odd")
                  for name in util.list_cases()}


@pytest.mark.parametrize("name", util.list_cases())
def test_class_predicted_from_the_records(name, tmp_path, recut_dirs):
    ds = D.dataset_of(name)
    sch, chunk_bytes = D.DATASET_PLAN[ds]
    case, _, _, _ = util.load_case(name, tmp_path, recut_dirs[ds, sch][0])
    pred = D.predict_case(case, chunk_bytes)
    assert pred["cls"] == EXPECTED_CLASS[name] and pred["exact"] and pred["device_chunks"] >= len(_bams(ds))
    assert pred["parse_chunks"] + pred["fallbacks"] == (0 if pred["cls"] == "inflate-only" else pred["device_chunks"])


@pytest.mark.parametrize("sch", D.SHAPES)
@pytest.mark.parametrize("name", D.SHAPE_CASES)
def test_class_of_the_block_shape_cases(name, sch, tmp_path, recut_dirs):
    """c1 and dense hold UMIs with N (21 of 10,000 and 16 of 6,000 records), so a chunk with such a record falls back by design and only
    phasing is clean under every shape; every shape is parsed on the device in at least two of the three cases, and where a chunk is
    expected to fall back, fewer than four follow in a row, so the counts are exact."""
    ds = D.dataset_of(name)
    case, _, _, _ = util.load_case(name, tmp_path, recut_dirs[ds, sch][0])
    pred = D.predict_case(case, D.shape_chunk_bytes(ds, sch))
    assert pred["exact"] and pred["cls"] == ("clean" if ds == "phasing" else "odd")
    assert pred["parse_chunks"] > 0 or (ds == "dense" and sch != "single")


def test_indexed_recut_reads_as_the_original(tmp_path):
    src, dst = os.path.join(DATASETS, "c1", "possorted.bam"), str(tmp_path / "c1.bam")
    n = reblock.reblock_bam_indexed(src, dst)
    (refs0, recs0), (refs1, recs1) = pybam.read_bam(src), pybam.read_bam(dst)
    assert refs0 == refs1 and len(recs0) == len(recs1) == n
    assert all(getattr(a, f) == getattr(b, f) for a, b in zip(recs0, recs1) for f in FIELDS)
    assert os.path.getsize(dst + ".bai") > 1000
    assert min(reblock.plan_chunks(dst, D.INDEXED_CHUNK_BYTES)[:-1]) >= D.HEADROOM


# ----------------------------------------------------------------------------- crafted files
def _n_max(c, flags):
    names, regions, snps, barcodes = D.crafted_tables(c)
    with Engine(capi.XCK_MODE_BOTH, names, regions, len(barcodes), snps=snps, barcodes=barcodes, cell_tag="CB", umi_tag="UB", flags=flags,
                decode_only=True) as eng:
        return (eng.umi_bits - 2) // 2


@pytest.mark.parametrize("flags", [0, capi.XCK_F_FORCE_KEY128])
@pytest.mark.parametrize("odd", [False, True])
def test_crafted_files_meet_their_conditions(odd, flags, tmp_path, oracle_lib):
    n_max = _n_max(D.craft(str(tmp_path / "probe"), 12, odd), flags)       # (the tables, and with them the key layout, do not depend on n_max)
    assert n_max == (31 if flags else 23)
    c = D.craft(str(tmp_path / "c"), n_max, odd)
    exp = D.crafted_expected(c)
    D.check_crafted_conditions(c, exp)
    refs, recs = pybam.read_bam(c["bam"])
    assert len(recs) == c["n_records"] and [n for n, _ in refs] == [n for n, _ in D.REFS]
    by_name = {r.query_name: r for r in recs}
    # the records are what their names say
    assert by_name["edge_cb_type_A"].tags["CB"] == ("A", "Q") and by_name["edge_cb_type_H"].tags["CB"][0] == "H"
    r = by_name["edge_arrays_and_numbers_first"]
    assert [r.tags[t][0] for t in list(r.tags)[:10]] == ["B", "B", "B", "c", "C", "s", "S", "i", "I", "f"] and list(r.tags)[10:12] == ["CB", "UB"]
    assert not by_name["edge_cb_absent"].has_tag("CB") and not by_name["edge_ub_absent"].has_tag("UB")
    assert len(by_name["edge_cb_long_unlisted"].get_tag("CB")) > D.BC_SLOT
    assert by_name["edge_ub_empty"].tags["UB"] == ("Z", "") and by_name["edge_ub_type_A"].tags["UB"] == ("A", "G")
    assert [len(by_name["edge_" + k].get_tag("UB")) for k in ("umi_len_1", "umi_len_nmax_minus_1", "umi_len_nmax")] == [1, n_max - 1, n_max]
    assert by_name["edge_no_cigar"].cigartuples is None and by_name["edge_l_seq_0"].l_seq == 0 and by_name["edge_l_seq_odd"].l_seq % 2 == 1
    r = by_name["edge_long_cigar"]
    assert len(r.cigartuples) > 64 and r.l_seq == 1000 and {op for op, _ in r.cigartuples} >= {0, 1, 2, 3, 4}
    assert "" in by_name and max(len(q) for q in by_name) == 254
    assert all(r.tid == -1 and r.flag & 4 for r in recs[-D.N_UNMAPPED:]) and recs[-D.N_UNMAPPED - 1].tid == 3
    if odd:
        assert len(by_name["edge_umi_len_nmax_plus_1"].get_tag("UB")) == n_max + 1
        assert "N" in by_name["edge_umi_with_N"].get_tag("UB") and by_name["edge_umi_lowercase"].get_tag("UB").islower()
        assert by_name["edge_ub_numeric_0"].tags["UB"] == ("i", 0)
        assert [by_name["edge_ub_numeric_" + t].tags["UB"][0] for t in "cSif"] == list("cSif")
        assert all(by_name["edge_ub_numeric_" + t].get_tag("UB") for t in "cSif")
    # the blocks: a contig change inside a block; the block of more than 64 records whose first round of 64 holds wanted, unwanted
    # and wanted records; no block with more runs than the walk's summary holds
    names = D.crafted_tables(c)[0]
    t2c = O.resolve_contigs([n for n, _ in refs], names)
    assert t2c == [0, 1, -1, 2]
    _, skip, blocks = reblock.block_records(c["bam"])
    assert skip == 0 and max(D.contig_runs(b, t2c) for b in blocks) <= D.MAX_RUNS
    assert any({t for t, _ in b} == {0, 1} for b in blocks)
    big = [b for b in blocks if len(b) > 64]
    assert len(big) == 1 and [t2c[t] for t, _ in big[0][:64]] == [1] * D.ALT_EACH + [-1] * D.N_UNKNOWN + [2] * (64 - D.ALT_EACH - D.N_UNKNOWN)
    # the chunks: all of 64 blocks and more; the records the device cannot code sit in two of them, with clean chunks around
    chunks = reblock.plan_chunks(c["bam"], D.CHUNK_BYTES)
    assert min(chunks[:-1]) >= D.HEADROOM and chunks[-1] >= D.MIN_BLOCKS
    at, with_odd = 0, []
    for n in chunks:
        keys = {k for b in blocks[at:at + n] for k in b}
        with_odd.append(len(keys & set(c["odd_keys"])))
        at += n
    if odd:
        assert len(c["odd_keys"]) == 8 and sum(with_odd) == 8
        assert sum(1 for k in with_odd if k) >= 2 and sum(1 for k in with_odd if not k) >= 2
        assert not any(all(with_odd[k:k + 4]) for k in range(len(with_odd) - 3))      # never four fallbacks in a row: the reader keeps asking
    else:
        assert not c["odd_keys"]
    pred = D.predict_run([c["bam"]], c["region_fn"], c["snp_fn"], c["barcode_fn"], "CB", "UB", D.CHUNK_BYTES, n_max)
    assert pred["exact"] and (pred["device_chunks"], pred["fallbacks"]) == (len(chunks), sum(1 for k in with_odd if k))
