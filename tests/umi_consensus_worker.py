"""Child process of tests/test_gpu_umi_consensus.py: what it runs sees XCK_UMI_CONSENSUS (or not) in its environment from the start,
as a front-end's user sets it.
  engine <case> <out.json>   a crafted case of tests/umi_consensus_model.py through a handle made WITHOUT the flag
  afc <golden case> <tmp>    afc_wrapper on a golden BAF case; the output directory is printed"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import util  # noqa: E402

what, name, dst = sys.argv[1:4]
if what == "engine":
    import umi_consensus_model as UM
    from xcltk_amd import capi
    from xcltk_amd.engine import Engine
    c = UM.case(name)
    f = dict(UM.FILT); f.update(c.filt)
    with Engine(capi.XCK_MODE_BAF, c.names, c.regions, c.n_cells, snps=c.snps, flags=capi.XCK_F_FEATURE_SUMMARY, **f) as eng:
        for d in c.batches:
            eng.push(util.batch_from_dict(d)[0])
        got = eng.finish()
        out = dict(stats=eng.molecule_stats(), tally=eng.feature_summary()["snp"][:, 1:6].tolist(), **{k: [a.tolist() for a in got[k]] for k in ("ad", "dp", "oth")})
    with open(dst, "w") as fp:
        json.dump(out, fp)
    print("ENGINE_DONE")
else:
    import logging
    from xcltk_amd.baf.fc.main import afc_wrapper
    logging.basicConfig(level=logging.INFO, stream=sys.stdout)       # (the front-end's one-line reports are logging.info)
    case, ddir, odir, exp = util.load_case(name, dst)
    assert afc_wrapper(**case["kwargs"]) == 0
    print("AFC_DONE", odir)
