"""The three opt-in summaries (XCK_F_READ_FATE, XCK_F_CELL_SUMMARY, XCK_F_FEATURE_SUMMARY) of one handle across xck_reset: where the
reset's zeroing (summaries_reset), the passes behind the first join launch of a queue (launch_summaries) and the overflow replay of
the push pipeline meet.  A handle that has counted one run, was reset and has counted a DIFFERENT run must answer as a fresh handle
that has only seen the second: nothing of the first run - a counter, a tally, a cached matrix half - may survive the reset, and the
replay must not run a summary pass a second time.  Every comparison is exact."""
import numpy as np
import pytest

import read_fate_util as R
import util
from xcltk_amd import capi

pytestmark = pytest.mark.gpu
ALL3 = capi.XCK_F_READ_FATE | capi.XCK_F_CELL_SUMMARY | capi.XCK_F_FEATURE_SUMMARY
SLICE = 1000                   # reads per pushed batch: one join tile, so the first guess of the hit capacity is 78 per shard
MAPQ_SHIFT = 18                # second run: the fixtures' mapq values are 0, 1, 3 and 255, their min_mapq is 20


def _slices(batches, mapq_shift):
    """The decoded batches (Engine.decode_bam) cut into pieces of SLICE reads, mapq raised by mapq_shift (saturating).  A handle's
    min_mapq is fixed at xck_create, so the second run's different threshold is stated on the reads: mapq + 18 >= 20 is mapq >= 2."""
    out = []
    for d in batches:
        for a in range(0, d["n_reads"], SLICE):
            b = min(a + SLICE, d["n_reads"])
            g = dict(contig=d["contig"], ordinal_base=d["ordinal_base"] + a, cigar=d["cigar"], cig_off=d["cig_off"][a:b + 1])
            for k in ("pos", "flag", "cell", "umi"):
                g[k] = d[k][a:b]
            g["mapq"] = np.minimum(d["mapq"][a:b].astype(np.int64) + mapq_shift, 255).astype(np.uint8)
            if "seq_off" in d:
                g["seq_off"], g["seq"] = d["seq_off"][a:b + 1], d["seq"]
            out.append(util.batch_from_dict(g))
    return out


def _run(eng, pieces):
    """push, finish, read everything -> (matrices and the three summaries as a flat dict of arrays / dicts, join launches)"""
    for b, _ in pieces:
        eng.push(b)
    got = {"res." + k: v for k, v in eng.finish().items()}
    got["fate"] = eng.read_fate()
    cs, fs = eng.cell_summary(), eng.feature_summary()
    got.update({"cell.fate": cs["fate"], "cell.matrix": cs["matrix"], "feat.matrix": fs["matrix"],
                "feat.reads": fs["reads"] if fs["reads"] is not None else fs["snp"]})
    assert cs["matrix"] is not None and fs["has_matrix"]
    return got, eng.stats()["n_join_launches"]


def _assert_same(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if k == "fate":
            assert got[k] == want[k], (got[k], want[k])
        elif k.startswith("res."):
            for a, b, what in zip(got[k], want[k], ("row", "col", "val")):
                assert np.array_equal(a, b), (k, what)
        else:
            assert np.array_equal(got[k], want[k]), (k, np.flatnonzero((got[k] != want[k]).any(axis=1))[:10])


@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("name", ["c1_basefc", "c1_baf"])
def test_reset_then_a_different_run_equals_a_fresh_handle(name, replay, monkeypatch):
    fx = R.load_fixture(name)
    for k in ("XCK_HIT_CAP0", "XCK_HIT_SLACK"):
        monkeypatch.delenv(k, raising=False)
    if replay:                                                    # (read at xck_create; the knobs of test_overflow_replay_classifies_once)
        monkeypatch.setenv("XCK_HIT_CAP0", "64")
        monkeypatch.setenv("XCK_HIT_SLACK", "0")
    with R.fixture_engine(fx, ALL3) as eng:
        batches = [d for i, fn in enumerate(fx["bam_fns"]) for d in eng.decode_bam(fn, sample=i, n_threads=2)]
        first, second = _slices(batches, 0), _slices(batches, MAPQ_SHIFT)
        one, launches = _run(eng, first)
        print(name, "first run:", one["fate"], "launches", launches, "pushes", len(first))
        assert one["fate"]["pairs"] > 0 and one["fate"]["low_mapq"] > 0
        # replay: at least one launch of the first run is replayed (which one depends on the inputs alone: a batch is one tile, its hits
        # land in one shard, and the shard holds 128 entries for the first batch and cursor + 78 from then on)
        assert launches > len(first) if replay else launches == len(first), (launches, len(first))
        eng.reset()
        assert all(v == 0 for v in eng.read_fate().values())
        got, _ = _run(eng, second)                                # (the hit streams keep their grown capacity: no replay is asked of this run)
    with R.fixture_engine(fx, ALL3) as eng:
        want, launches = _run(eng, second)
        print(name, "second run, fresh handle:", want["fate"], "launches", launches)
        # (no replay is asked of this handle either: its buffers double ahead of the cursors, and whether a one-tile batch outruns
        # them depends on where the run's hits fall - c1_baf's second run never does)
        assert launches >= len(second) if replay else launches == len(second), (launches, len(second))
    # the second run is a different one: the reads with mapq 3 pass the mapq filter now
    assert want["fate"]["low_mapq"] < one["fate"]["low_mapq"] and not np.array_equal(want["cell.fate"], one["cell.fate"])
    _assert_same(got, want)
