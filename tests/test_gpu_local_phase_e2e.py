"""XCK_DEVICE_PHASING=1 end to end: the front-ends with the regions phased on the GPU (baf/fc/phasing_dev.py, csrc/local_phase.hip)
write, byte for byte, what the unmodified reference wrote (the phasing_baf_* golden cases, the short and the surplus pileup among
them) and what they write with the switch off (afc_variants, the one-pass `xcltk baf`)."""
import os

import pytest

import util

pytestmark = pytest.mark.gpu

CASES = ["phasing_baf_off", "phasing_baf_allreg", "phasing_baf_refcells", "phasing_baf_short_pileup", "phasing_baf_surplus_pileup"]
DS = os.path.join(util.GOLDEN, "datasets", "phasing")


@pytest.fixture
def device_calls(monkeypatch):
    """Switch the device path on; -> list that receives one entry per local_phasing_dev call."""
    from xcltk_amd.baf.fc import phasing_dev
    calls = []

    def counted(*a, _orig=phasing_dev.local_phasing_dev, **k):
        calls.append(len(a[0]))
        return _orig(*a, **k)
    monkeypatch.setattr(phasing_dev, "local_phasing_dev", counted)
    monkeypatch.setenv("XCK_DEVICE_PHASING", "1")
    for k in ("WORLD_SIZE", "XCK_DIST_FORCE"):
        monkeypatch.delenv(k, raising=False)
    return calls


@pytest.mark.parametrize("name", CASES)
def test_afc_wrapper_with_device_phasing_matches_the_reference_outputs(name, tmp_path, device_calls):
    from xcltk_amd.baf.fc.main import afc_wrapper
    case, ddir, odir, exp = util.load_case(name, tmp_path)
    assert afc_wrapper(**case["kwargs"]) == 0
    util.assert_dirs_equal(odir, exp)
    assert len(device_calls) == (1 if case["kwargs"].get("cellsnp_dir") else 0)      # (phasing_baf_off has no pileup: nothing to phase)


def _variants(tmp_path, sub):
    d = tmp_path / sub
    d.mkdir()
    common, variants, outs = None, [], []
    for name in CASES:
        case, ddir, odir, exp = util.load_case(name, d)
        kw = dict(case["kwargs"])
        common = {k: kw.pop(k) for k in ("sam_fn", "barcode_fn", "phased_snp_fn")}
        variants.append(kw); outs.append((odir, exp))
    return common, variants, outs


def test_afc_variants_with_device_phasing_equals_the_host_phasing(tmp_path, monkeypatch, device_calls):
    from xcltk_amd.baf.fc.variants import afc_variants
    common, variants, outs_dev = _variants(tmp_path, "dev")
    assert afc_variants(common, variants) == 0
    assert len(device_calls) == 4                                        # once per variant with a pileup
    monkeypatch.delenv("XCK_DEVICE_PHASING")
    common, variants, outs_host = _variants(tmp_path, "host")
    assert afc_variants(common, variants) == 0
    assert len(device_calls) == 4
    for (od, exp), (oh, _) in zip(outs_dev, outs_host):
        util.assert_dirs_equal(od, oh)
        util.assert_dirs_equal(od, exp)


def test_one_pass_baf_with_device_phasing_equals_the_host_phasing(tmp_path, monkeypatch, device_calls):
    from test_genotype import GT, _genotype_cases
    from xcltk_amd.baf.pipeline import pipeline_wrapper
    from xcltk_amd.utils import csp_io
    name, case = _genotype_cases()[0]
    covered = set(csp_io.load_data(os.path.join(GT, name)).pos.tolist())  # the phased list derives from the filtered pileup VCF: the SNPs it keeps
    lines = open(os.path.join(DS, "snps.tsv")).read().splitlines()
    snp_fn = str(tmp_path / "phased.tsv")
    open(snp_fn, "w").write("\n".join([lines[0]] + [l for l in lines[1:] if int(l.split("\t")[1]) in covered]) + "\n")
    monkeypatch.setenv("XCK_BAF_ONE_PASS", "1")
    outs = {}
    for how in ("dev", "host"):
        if how == "host":
            monkeypatch.delenv("XCK_DEVICE_PHASING")
        outs[how] = str(tmp_path / how)
        ret = pipeline_wrapper("smp", sam_fn=os.path.join(DS, "possorted.bam"), barcode_fn=os.path.join(DS, "barcodes.tsv"),
                               snp_vcf_fn=os.path.join(DS, "cellsnp", "cellSNP.base.vcf.gz"), region_fn=os.path.join(DS, "regions.tsv"),
                               out_dir=outs[how], phased_snp_fn=snp_fn, ref_cell_fn=os.path.join(DS, "ref_cells.tsv"),
                               min_count=case["min_count"], min_maf=case["min_maf"], ncores=2)
        assert ret == 0
    assert len(device_calls) == 1
    util.assert_dirs_equal(os.path.join(outs["dev"], "3_baf_fc"), os.path.join(outs["host"], "3_baf_fc"))
    assert os.path.getsize(os.path.join(outs["dev"], "3_baf_fc", "xcltk.DP.mtx")) > 200
