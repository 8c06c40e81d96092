"""k_join at limit - 1, at the limit and at limit + 1 of everything it stages per tile (tests/join_tile_cases.py): the set-aside
list of spliced reads, the staged CIGAR words, regions / SNPs and SNP windows, the parked pairs of a wave, the LDS queues and the key
set, gap records, chunks of 64 regions, batch sizes.  Each case runs with 64- and with 128-bit keys against the CPU oracle, compared
exactly, and the accepted pairs the engine reports equal the tile model's.  tests/test_join_tile_cases_host.py shows on the CPU that
every read under test changes the expected matrices, i.e. that a lost pair cannot pass here."""
import pytest

import join_tile_cases as JT
import util

pytestmark = pytest.mark.gpu

MATS = {JT.FC: ["count"], JT.BAF: ["ad", "dp", "oth"]}


@pytest.mark.parametrize("flags", [0, JT.F128], ids=["key64", "key128"])
@pytest.mark.parametrize("name", JT.NAMES)
def test_join_tile_case(name, flags):
    c = JT.case(name)
    kw = dict(JT.FILT); kw.update(c.filt)
    batches = [util.batch_from_dict(d) for d in c.batches]
    got, exp, stats = util.engine_vs_oracle(c.mode, c.names, c.regions, c.snps, c.n_cells, batches, flags=flags, **kw)
    tiles, pairs = JT.model(c.mode, c.names, c.regions, c.snps, c.batches, c.filt, flags)
    print("%s flags=%d: crosses %s, nnz %s, n_hits %d (model %d)" % (name, flags, sorted(JT.crossed(c.mode, tiles)),
                                                                   [len(exp[m][0]) for m in MATS[c.mode]], stats["n_hits"], pairs))
    util.assert_coo_equal(got, exp, MATS[c.mode])
    assert sum(len(exp[m][0]) for m in MATS[c.mode]) > 0
    assert stats["n_hits"] == pairs
