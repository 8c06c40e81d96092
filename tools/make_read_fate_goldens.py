#!/opt/conda/bin/python3.9
"""make_read_fate_goldens.py - CONTAINER-ONLY generator of tests/golden/read_fate/*.json and tests/golden/cell_summary/*.json
(test infrastructure).

Expected values of the read assignment summary (xck_get_read_fate, include/xck.h), produced by the unmodified reference's own
code on the golden datasets.  Like oracle/refgen/run_reference.py - whose stand-in set-up it repeats - it imports the
reference in place (read-only tree, sys.dont_write_bytecode) with `pysam` -> oracle/pybam.py and `anndata` -> the minimal
stand-in; nothing of the reference is copied, only numbers are kept.

Per dataset and mode it calls
  * check_read() of rdr/fc/core.py / baf/fc/core.py on every record,
  * sam_fetch(sam, chrom, start, end - 1) per region with __get_include_frac / __get_include_len (rdr/fc/core.py:140-165),
  * sam_fetch(sam, chrom, pos, pos) per SNP of load_snp_from_tsv (BAF),
keys the records by their ordinal in the file, and gives each record the FIRST class that applies, in the order of
xck_read_fate.  A barcode MCount.push_read would reject, or an empty key, falls under no_cell / no_umi.  Records on references
Per cell (xck_get_cell_summary): the same class of every record, grouped by the record's row - its listed barcode, or the index of
its BAM where the cells are files; `*` collects the records without a listed barcode.  Records that are `not_joined` or outside
the table reach no kernel and so no row.  The rows are named in the engine's column order (sorted barcodes / sample ids) and
only the non-zero ones are kept, as 12 numbers in the order of FIELDS[1:].

Records on references outside the front-end's contig table (the regions' chromosomes, plus the SNPs' for BAF) are counted apart (`outside_table`: the
decoder may drop them or forward them as skipped batches); records on a table contig without targets are `not_joined`.

usage: make_read_fate_goldens.py [--check]      (--check: compare with the committed files instead of writing them)
"""
import collections
import json
import os
import sys
import types

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "refgen"))
REF = os.environ.get("XCLTK_REFERENCE", "/root/reference")
DATASETS = os.path.join(ROOT, "tests", "golden", "datasets")
OUT = os.path.join(ROOT, "tests", "golden", "read_fate")
OUT_CELL = os.path.join(ROOT, "tests", "golden", "cell_summary")

FIELDS = ("not_joined", "low_mapq", "excl_flag", "incl_flag", "orphan", "no_cell", "no_umi", "short_aligned", "no_target",
          "include_fail", "assigned", "multi", "pairs")
CHECK_CODE = {-2: "low_mapq", -3: "excl_flag", -4: "incl_flag", -5: "orphan", -11: "no_cell", -12: "no_umi", -21: "short_aligned"}

# (file stem, dataset, mode, overrides).  Defaults: MAPQ 20, min length 30, exclude 772 with UMIs / 1796 without, no orphans,
# min_include 0.9, tags CB / UB, the dataset's regions.tsv.  "$F/" = a file next to the fixtures.
CASES = [
    ("c1_basefc", "c1", "basefc", {}),
    ("dense_basefc", "dense", "basefc", {}),
    ("special_basefc", "special", "basefc", {}),
    ("special_basefc_inc30", "special", "basefc", {"min_include": 30}),
    ("multibam_basefc", "multibam", "basefc", {}),
    ("well_basefc", "well", "basefc", {"cell_tag": None, "umi_tag": None}),
    ("c1_baf", "c1", "baf", {}),
    ("dense_baf", "dense", "baf", {}),
    ("special_baf", "special", "baf", {}),
    # so that no class is empty everywhere:
    ("dense_basefc_incl16", "dense", "basefc", {"incl_flag": 16}),
    # the dataset's regions plus one on chrUn, which carries a read and no SNP -> that read is not_joined
    ("special_baf_regions_un", "special", "baf", {"region_fn": "$F/special_regions_un.tsv"}),
]


def install_standins():
    import pybam
    m = types.ModuleType("pysam")
    m.AlignmentFile = pybam.AlignmentFile
    m.BGZFile = pybam.BGZFile
    m.__version__ = "0.0-standin"
    sys.modules["pysam"] = m
    import anndata_standin
    a = types.ModuleType("anndata")
    a.AnnData = anndata_standin.AnnData
    sys.modules["anndata"] = a
    return pybam


class Conf(object):
    pass


def run_case(pybam, stem, dataset, mode, over):
    from xcltk.baf.fc import core as baf_core
    from xcltk.baf.fc.utils import load_snp_from_tsv
    from xcltk.rdr.fc import core as rdr_core
    from xcltk.rdr.fc.utils import load_region_from_txt
    from xcltk.utils.grange import format_chrom
    from xcltk.utils.sam import sam_fetch
    inc_frac = getattr(rdr_core, "__get_include_frac")
    inc_len = getattr(rdr_core, "__get_include_len")
    ddir = os.path.join(DATASETS, dataset)
    with open(os.path.join(ddir, "dataset.json")) as fp:
        ds = json.load(fp)
    p = dict(min_mapq=20, min_len=30, incl_flag=0, no_orphan=True, min_include=0.9, cell_tag="CB", umi_tag="UB",
             region_fn="$D/regions.tsv")
    p.update(over)
    p["excl_flag"] = over.get("excl_flag", 772 if p["umi_tag"] else 1796)
    c = Conf()
    for k in ("min_mapq", "min_len", "incl_flag", "excl_flag", "no_orphan", "min_include", "cell_tag", "umi_tag"):
        setattr(c, k, p[k])
    region_fn = p["region_fn"].replace("$D/", ddir + "/").replace("$F/", OUT + "/")
    regs = load_region_from_txt(region_fn)
    bc = None
    if p["cell_tag"]:
        with open(os.path.join(ddir, ds["barcodes"])) as fp:
            bc = set(line.strip() for line in fp)
    table = set(format_chrom(r.chrom) for r in regs)
    if mode == "basefc":
        targets = set(table)
        check_read = rdr_core.check_read
    else:
        snps = load_snp_from_tsv(os.path.join(ddir, "snps.tsv")).get_regions()
        targets = set(format_chrom(s.chrom) for s in snps)
        table |= targets
        check_read = baf_core.check_read
    fate = collections.Counter()
    rows = collections.defaultdict(collections.Counter)        # per-cell table: row name -> the same counters
    records = outside = 0
    for bam_index, b in enumerate(ds["bams"]):
        sam = pybam.AlignmentFile(os.path.join(ddir, b), "r")
        n_acc, fetched = collections.Counter(), set()          # per record ordinal: accepting regions / covered SNPs; fetched by any region
        if mode == "basefc":
            for reg in regs:
                itr = sam_fetch(sam, reg.chrom, reg.start, reg.end - 1)
                if not itr:
                    continue
                for r in itr:
                    fetched.add(r.ordinal)
                    if 0 < c.min_include < 1:
                        f = inc_frac(r.positions, reg.start - 1, reg.end - 2)
                        ok = f is not None and f >= c.min_include
                    else:
                        ok = inc_len(r.positions, reg.start - 1, reg.end - 2) >= c.min_include
                    if ok:
                        n_acc[r.ordinal] += 1
        else:
            for s in snps:
                itr = sam_fetch(sam, s.chrom, s.pos, s.pos)
                if not itr:
                    continue
                for r in itr:
                    n_acc[r.ordinal] += 1
        for r in sam.fetch():
            records += 1
            ch = format_chrom(sam.references[r.tid]) if r.tid >= 0 else None
            if ch not in table:
                outside += 1
                continue
            code = check_read(r, c)
            listed = True
            if bc is not None:
                listed = r.has_tag(p["cell_tag"]) and r.get_tag(p["cell_tag"]) in bc
            if p["umi_tag"]:
                key_ok = r.has_tag(p["umi_tag"]) and bool(r.get_tag(p["umi_tag"]))
            else:
                key_ok = bool(r.query_name)
            if ch not in targets:
                cls = "not_joined"
            elif code in (-2, -3, -4, -5):
                cls = CHECK_CODE[code]
            elif code == -11 or not listed:
                cls = "no_cell"
            elif code == -12 or not key_ok:
                cls = "no_umi"
            elif code == -21:
                cls = "short_aligned"
            elif code < 0:
                raise SystemExit("%s: check_read code %d has no class" % (stem, code))
            elif mode == "basefc" and r.ordinal not in fetched:
                cls = "no_target"
            elif n_acc[r.ordinal] == 0:
                cls = "include_fail" if mode == "basefc" else "no_target"
            else:
                cls = "assigned"
                fate["pairs"] += n_acc[r.ordinal]
                fate["multi"] += 1 if n_acc[r.ordinal] > 1 else 0
            fate[cls] += 1
            if cls != "not_joined":
                if bc is None:
                    row = ds["sample_ids"][bam_index]
                else:
                    row = r.get_tag(p["cell_tag"]) if listed else "*"
                rows[row][cls] += 1
                if cls == "assigned":
                    rows[row]["pairs"] += n_acc[r.ordinal]
                    rows[row]["multi"] += 1 if n_acc[r.ordinal] > 1 else 0
    out = dict(name=stem, dataset=dataset, mode=mode, records=records, outside_table=outside,
               params={k: p[k] for k in sorted(p)}, fate={k: int(fate[k]) for k in FIELDS},
               reference="hxj5/xcltk check_read / sam_fetch / include test via tools/make_read_fate_goldens.py (pysam/anndata stand-ins)")
    assert sum(out["fate"][k] for k in FIELDS[:-2]) + outside == records
    names = sorted(bc) if bc is not None else list(ds["sample_ids"])
    assert set(rows) <= set(names) | {"*"}
    cell = dict(name=stem, dataset=dataset, mode=mode, cells=names, columns=list(FIELDS[1:]),
                rows={k: [int(v[c]) for c in FIELDS[1:]] for k, v in sorted(rows.items())},
                reference=out["reference"])
    for j, c in enumerate(FIELDS[1:]):
        assert sum(v[j] for v in cell["rows"].values()) == out["fate"][c], c
    return out, cell


def main():
    check = "--check" in sys.argv[1:]
    pybam = install_standins()
    sys.path.insert(0, REF)
    import logging
    logging.disable(logging.CRITICAL)
    os.makedirs(OUT, exist_ok=True)
    os.makedirs(OUT_CELL, exist_ok=True)
    bad = 0
    for stem, dataset, mode, over in CASES:
        out, cell = run_case(pybam, stem, dataset, mode, over)
        text = json.dumps(out, indent=1, sort_keys=True) + "\n"
        fn = os.path.join(OUT, stem + ".json")
        f = out["fate"]
        print("%-24s records %5d outside %d  %s" % (stem, out["records"], out["outside_table"], " ".join("%s=%d" % (k, f[k]) for k in FIELDS)))
        if check:
            with open(fn) as fp:
                if fp.read() != text:
                    print("  DIFFERS from %s" % fn)
                    bad += 1
        else:
            with open(fn, "w") as fp:
                fp.write(text)
        # (one line per row: a thousand short lists read better, and diff better, than twelve thousand lines of digits)
        body = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(cell["rows"].items()))
        head = json.dumps({k: v for k, v in cell.items() if k != "rows"}, indent=1, sort_keys=True)
        text = head[:-2] + ',\n "rows": {\n' + body + "\n }\n}\n"
        assert json.loads(text) == cell
        fn = os.path.join(OUT_CELL, stem + ".json")
        print("%-24s rows %d (of %d cells)" % ("", len(cell["rows"]), len(cell["cells"])))
        if check:
            with open(fn) as fp:
                if fp.read() != text:
                    print("  DIFFERS from %s" % fn)
                    bad += 1
        else:
            with open(fn, "w") as fp:
                fp.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
