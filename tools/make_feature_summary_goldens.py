#!/opt/conda/bin/python3.9
"""make_feature_summary_goldens.py - CONTAINER-ONLY generator of tests/golden/feature_summary/*.json (test infrastructure).

Expected values of the per-feature and per-SNP tables (xck_get_feature_summary, include/xck.h), produced by the unmodified
reference's own code on the golden datasets, with the stand-in set-up of tools/make_read_fate_goldens.py (whose cases, and
install_standins(), it imports): the reference is imported in place, nothing of it is copied, only numbers are kept.

basefc, per region of load_region_from_txt: the records of sam_fetch(sam, chrom, start, end - 1) that pass check_read() and the
  barcode / key rule of MCount.push_read, split by __get_include_frac / __get_include_len into accepted (`pairs`) and not
  (`include_fail`); `shared` = accepted records that two or more regions accept (from the per-record accept counts).
BAF, per SNP of load_snp_from_tsv: plp_snp(snp, sam_list, mcnt, conf) itself - mcnt.tcount and the return code (0 kept, 3 below
  min_count, 5 below min_maf) - and the number of records of the same sam_fetch(sam, chrom, pos, pos) that pass the same rule.

Rows are keyed by the region's index in the file / by `chrom:pos:ref:alt#k` (k-th list entry with that text); only non-zero rows
are kept, one per line (BAF: a SNP without a read and without a tally that plp_snp drops with return code 3 has no row).  Per case the `pairs` / `reads` column must sum to `fate.pairs` of the committed
tests/golden/read_fate/<stem>.json (the per-SNP filters do not touch it: the two filter cases use their dataset's BAF file).

usage: make_feature_summary_goldens.py [--check]      (--check: compare with the committed files instead of writing them)
"""
import collections
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_read_fate_goldens as G   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "feature_summary")
# the 11 cases of the read-fate tool (per-SNP filters off: min_count 1, min_maf 0, the front-end's defaults), and two with
# filters that drop SNPs
CASES = [(stem, ds, mode, dict(over), stem) for stem, ds, mode, over in G.CASES] + [
    ("dense_baf_c3_m01", "dense", "baf", {"min_count": 3, "min_maf": 0.1}, "dense_baf"),
    ("special_baf_c3_m01", "special", "baf", {"min_count": 3, "min_maf": 0.1}, "special_baf"),
]
REGION_COLS = ("include_fail", "pairs", "shared")
SNP_COLS = ("reads", "a", "c", "g", "t", "n", "ret")


def run_case(pybam, stem, dataset, mode, over, fate_stem):
    from xcltk.baf.fc import core as baf_core
    from xcltk.baf.fc.mcount import MCount
    from xcltk.baf.fc.utils import load_snp_from_tsv
    from xcltk.rdr.fc import core as rdr_core
    from xcltk.rdr.fc.utils import load_region_from_txt
    from xcltk.utils.sam import sam_fetch
    inc_frac = getattr(rdr_core, "__get_include_frac")
    inc_len = getattr(rdr_core, "__get_include_len")
    ddir = os.path.join(G.DATASETS, dataset)
    with open(os.path.join(ddir, "dataset.json")) as fp:
        ds = json.load(fp)
    p = dict(min_mapq=20, min_len=30, incl_flag=0, no_orphan=True, min_include=0.9, cell_tag="CB", umi_tag="UB",
             region_fn="$D/regions.tsv", min_count=1, min_maf=0)
    p.update(over)
    p["excl_flag"] = over.get("excl_flag", 772 if p["umi_tag"] else 1796)
    c = G.Conf()
    for k in ("min_mapq", "min_len", "incl_flag", "excl_flag", "no_orphan", "min_include", "cell_tag", "umi_tag", "min_count", "min_maf"):
        setattr(c, k, p[k])
    c.use_barcodes = lambda: bool(p["cell_tag"])
    c.use_umi = lambda: bool(p["umi_tag"])
    c.debug = 0
    bc = None
    if p["cell_tag"]:
        with open(os.path.join(ddir, ds["barcodes"])) as fp:
            bc = set(line.strip() for line in fp)
    c.samples = sorted(bc) if bc is not None else list(ds["sample_ids"])
    check_read = rdr_core.check_read if mode == "basefc" else baf_core.check_read

    def passes(r):                                             # check_read, a listed cell, a non-empty key
        if check_read(r, c) < 0:
            return False
        if bc is not None and not (r.has_tag(p["cell_tag"]) and r.get_tag(p["cell_tag"]) in bc):
            return False
        return bool(r.get_tag(p["umi_tag"])) if p["umi_tag"] else bool(r.query_name)

    sams = [pybam.AlignmentFile(os.path.join(ddir, b), "r") for b in ds["bams"]]
    rows, keys = {}, []
    if mode == "basefc":
        region_fn = p["region_fn"].replace("$D/", ddir + "/").replace("$F/", G.OUT + "/")
        regs = load_region_from_txt(region_fn)
        cols = REGION_COLS
        acc = collections.defaultdict(list)                    # (bam, record ordinal) -> regions that accept it
        fail = collections.Counter()
        for g, reg in enumerate(regs):
            keys.append("%s:%d-%d" % (reg.chrom, reg.start, reg.end - 1))
            for bi, sam in enumerate(sams):
                itr = sam_fetch(sam, reg.chrom, reg.start, reg.end - 1)
                if not itr:
                    continue
                for r in itr:
                    if not passes(r):
                        continue
                    if 0 < c.min_include < 1:
                        f = inc_frac(r.positions, reg.start - 1, reg.end - 2)
                        ok = f is not None and f >= c.min_include
                    else:
                        ok = inc_len(r.positions, reg.start - 1, reg.end - 2) >= c.min_include
                    if ok:
                        acc[bi, r.ordinal].append(g)
                    else:
                        fail[g] += 1
        pairs, shared = collections.Counter(), collections.Counter()
        for gs in acc.values():
            for g in gs:
                pairs[g] += 1
                shared[g] += 1 if len(gs) >= 2 else 0
        for g in range(len(regs)):
            v = [fail[g], pairs[g], shared[g]]
            if any(v):
                rows[str(g)] = v
        total = sum(pairs.values())
    else:
        snps = load_snp_from_tsv(os.path.join(ddir, "snps.tsv")).get_regions()
        cols = SNP_COLS
        mcnt = MCount(c.samples, c)
        seen = collections.Counter()
        total = 0
        for s in snps:
            text = "%s:%d:%s:%s" % (s.chrom, s.pos, s.ref, s.alt)
            key = "%s#%d" % (text, seen[text])
            seen[text] += 1
            keys.append(key)
            n = 0
            for sam in sams:
                itr = sam_fetch(sam, s.chrom, s.pos, s.pos)
                if itr:
                    n += sum(1 for r in itr if passes(r))
            ret, mcnt = baf_core.plp_snp(s, sams, mcnt, c)
            if ret not in (0, 3, 5):
                raise SystemExit("%s: plp_snp returned %d for %s" % (stem, ret, key))
            v = [n] + [int(x) for x in mcnt.tcount] + [int(ret)]
            total += n
            if any(v[:-1]) or ret == 0:                       # (an absent row: no read, no tally, dropped for min_count - return code 3)
                rows[key] = v
            elif ret != 3:
                raise SystemExit("%s: %s has no count and return code %d" % (stem, key, ret))
    with open(os.path.join(G.OUT, fate_stem + ".json")) as fp:
        want = json.load(fp)["fate"]["pairs"]
    if total != want:
        raise SystemExit("%s: pairs %d, tests/golden/read_fate/%s.json has %d" % (stem, total, fate_stem, want))
    return dict(name=stem, dataset=dataset, mode=mode, fate=fate_stem, params={k: p[k] for k in sorted(p)}, columns=list(cols),
                keys=keys, rows=rows,
                reference="hxj5/xcltk check_read / sam_fetch / include test / plp_snp via tools/make_feature_summary_goldens.py (pysam/anndata stand-ins)")


def main():
    check = "--check" in sys.argv[1:]
    pybam = G.install_standins()
    sys.path.insert(0, G.REF)
    import logging
    logging.disable(logging.CRITICAL)
    os.makedirs(OUT, exist_ok=True)
    bad = 0
    for stem, dataset, mode, over, fate_stem in CASES:
        out = run_case(pybam, stem, dataset, mode, over, fate_stem)
        body = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in out["rows"].items())
        head = json.dumps({k: v for k, v in out.items() if k not in ("rows", "keys")}, indent=1, sort_keys=True)
        text = head[:-2] + ',\n "keys": ' + json.dumps(out["keys"]) + ',\n "rows": {\n' + body + "\n }\n}\n"
        assert json.loads(text) == out
        fn = os.path.join(OUT, stem + ".json")
        print("%-24s %-6s rows %d of %d, column sums %s" % (stem, mode, len(out["rows"]), len(out["keys"]),
                                                            [sum(v[j] for v in out["rows"].values()) for j in range(len(out["columns"]))]))
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
