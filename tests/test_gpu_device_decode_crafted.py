"""Records the golden files do not hold, through the device-decoded ingest (k_walk -> k_scan -> k_parse -> engine_push_parsed): tags of
type A and H, B arrays and numbers of every width ahead of the wanted tags, tags given twice, absent and empty tags, unlisted and
over-long barcodes, UMIs at the bound of the 2-bit code, records without CIGAR or sequence, 200 CIGAR operations, the shortest and the
longest read name, contig changes and a contig the tables do not know inside one block of more than 64 records, unmapped records -
and, in a second file, the UMIs the device leaves to the host (too long, with N, lowercase, numeric).  Every such record is the only
read of its (region, cell) pair and lies on a SNP, so its fate is one entry of `count` and of `ad` / `dp` (tests/device_decode_cases.py
writes the files; tests/test_device_decode_cases_host.py checks on the CPU that they hold what they are meant to hold).
The expected matrices are NOT csrc/bam_records.cpp parse_record's, which k_parse restates line by line: they are the oracle's
(oracle/xck_oracle.c) on the records as oracle/pybam.py reads them.  Reference boundary: pysam's record iteration and get_tag
(first occurrence of a tag, str for Z / A / H, the value for numeric types), as restated by oracle/pybam.py."""
import pytest

import device_decode_cases as D
import util
from xcltk_amd import capi
from xcltk_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("flags", [0, capi.XCK_F_FORCE_KEY128])
@pytest.mark.parametrize("odd", [False, True])
def test_crafted_records_through_the_device_decoder(odd, flags, tmp_path, monkeypatch, oracle_lib):
    monkeypatch.setenv("XCK_GPU_INFLATE", "100")
    monkeypatch.setenv("XCK_GPU_INFLATE_MIN_MB", "0")
    monkeypatch.setenv("XCK_CHUNK_BYTES", str(D.CHUNK_BYTES))
    monkeypatch.delenv("XCK_GPU_PARSE", raising=False)
    names, regions, snps, barcodes = D.crafted_tables(D.craft(str(tmp_path / "tables"), 12, odd))     # (the tables do not depend on n_max)
    eng = Engine(capi.XCK_MODE_BOTH, names, regions, len(barcodes), snps=snps, barcodes=barcodes, cell_tag="CB", umi_tag="UB", n_threads=4, flags=flags)
    try:
        n_max = (eng.umi_bits - 2) // 2                                     # the longest UMI encode_key_direct codes in 2 bits
        c = D.craft(str(tmp_path / "c"), n_max, odd)
        assert D.crafted_tables(c) == (names, regions, snps, barcodes)
        exp = D.crafted_expected(c)
        D.check_crafted_conditions(c, exp)
        pred = D.predict_run([c["bam"]], c["region_fn"], c["snp_fn"], c["barcode_fn"], "CB", "UB", D.CHUNK_BYTES, n_max)
        n = eng.ingest_bam(c["bam"])
        got = eng.finish()
        st = D.sum_stats([eng.decode_stats()])
    finally:
        eng.close()
    print("device decode: crafted %s file, n_max %d: inflate chunks %d (predicted %d), parse chunks %d (%d), fallbacks %d (%d)" % (
        "odd" if odd else "clean", n_max, st["gpu_inflate_chunks"], pred["device_chunks"], st["gpu_parse_chunks"], pred["parse_chunks"],
        st["gpu_parse_fallbacks"], pred["fallbacks"]))
    assert n == c["n_records"]                                             # (every record is walked, wanted or not)
    util.assert_coo_equal(got, exp, ("count", "ad", "dp", "oth"))
    if odd:
        assert st["gpu_parse_fallbacks"] >= 1 and st["gpu_parse_chunks"] > 0
    else:
        assert st["gpu_parse_chunks"] > 0 and st["gpu_parse_fallbacks"] == 0
    assert pred["exact"] and pred["cls"] == ("odd" if odd else "clean")
    D.assert_stats(pred, st)
