#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (no GPU needed): tools/kernel_table.py BASE_DIR NEW_DIR

Each directory holds, for every HIP translation unit of the build, NAME.s and NAME.rpass made with
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I../../include --cuda-device-only -S NAME.hip -o DIR/NAME.s \
        -Rpass-analysis=kernel-resource-usage 2> DIR/NAME.rpass
Prints, per xck:: kernel: SGPRs, VGPRs, AGPRs, scratch, occupancy, LDS bytes, the instruction count of the body (lines between the
kernel's label and its .Lfunc_end; comments, labels and directives stripped) and whether the instruction text is the same once the
basic-block label numbers are taken out.  Then the kernels only one side has, and the same for the library (rocPRIM) kernels by
mangled name.  Exit status 1 if a kernel both sides have differs in any figure."""
import glob, hashlib, os, re, subprocess, sys

FIELDS = [("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds")]


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def read_dir(d):
    """{mangled name: {"unit", "res": {...}, "n_insn", "sha"}}; the same kernel in two units (a static kernel of a shared header) gets one entry per unit"""
    kernels = []
    for s_path in sorted(glob.glob(os.path.join(d, "*.s"))):
        unit = os.path.basename(s_path)[:-2]
        res, cur = {}, None
        for line in open(s_path[:-2] + ".rpass", errors="replace"):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = res.setdefault(m.group(1), {}); continue
            for label, key in FIELDS:
                m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
        names, body, inside = set(), {}, None
        for line in open(s_path, errors="replace"):
            t = line.strip()
            m = re.match(r"\.amdhsa_kernel (\S+)", t)
            if m:
                names.add(m.group(1)); continue
            if inside is None:
                m = re.match(r"(_Z\w+):", t)
                if m and not line[0].isspace():
                    inside = m.group(1); body[inside] = []
                continue
            if t.startswith(".Lfunc_end"):
                inside = None; continue
            t = t.split(";")[0].strip()
            if not t or t.endswith(":") or t.startswith("."):
                continue
            body[inside].append(re.sub(r"\.LBB\d+_", ".LBB_", t))
        for n in sorted(names):
            text = body.get(n, [])
            kernels.append({"name": n, "unit": unit, "res": res.get(n, {}), "n_insn": len(text), "calls": sum(1 for t in text if t.startswith("s_swappc") or t.startswith("s_call")),
                            "sha": hashlib.sha1("\n".join(text).encode()).hexdigest()[:12]})
    return kernels


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    base, new = read_dir(sys.argv[1]), read_dir(sys.argv[2])
    pretty = demangle(sorted({k["name"] for k in base + new}))
    # a static kernel has an internal-linkage name (_ZN3xckL...): compare it with the parent's external one
    key = lambda k: re.sub(r"^_ZN3xckL", "_ZN3xck", k["name"])
    is_xck = lambda k: k["name"].startswith("_ZN3xck")
    bx = {key(k): k for k in base if is_xck(k)}
    bad = 0
    print("%d kernels in %s (%d xck::), %d in %s (%d xck::)" % (len(base), sys.argv[1], len(bx), len(new), sys.argv[2], sum(map(is_xck, new))))
    print("calls in xck:: kernel bodies: base %d, new %d" % (sum(k["calls"] for k in base if is_xck(k)), sum(k["calls"] for k in new if is_xck(k))))
    print("\n%-8s %5s %5s %5s %7s %4s %6s %7s  %-10s %s" % ("unit", "sgpr", "vgpr", "agpr", "scratch", "occ", "lds", "insns", "vs base", "kernel"))
    seen = set()
    for k in sorted((k for k in new if is_xck(k)), key=lambda k: (k["unit"], pretty[k["name"]])):
        b = bx.get(key(k)); seen.add(key(k))
        r = k["res"]
        if b is None: verdict = "NEW"; bad += 1
        elif b["res"] != r or b["n_insn"] != k["n_insn"]:
            verdict = "DIFFERS (base: %s, %d insns)" % (" ".join("%s=%s" % (f, b["res"].get(f)) for _, f in FIELDS), b["n_insn"]); bad += 1
        else: verdict = "same" if b["sha"] == k["sha"] else "same-count"
        print("%-8s %5s %5s %5s %7s %4s %6s %7d  %-10s %s" % (k["unit"], r.get("sgpr"), r.get("vgpr"), r.get("agpr"), r.get("scratch"), r.get("occ"), r.get("lds"), k["n_insn"],
                                                          verdict, pretty[k["name"]].split("(")[0].replace("void ", "")))
    print("\nxck:: kernels of the base that the new build does not have:")
    for n in sorted(set(bx) - seen, key=lambda n: pretty[bx[n]["name"]]):
        print("   ", pretty[bx[n]["name"]].split("(")[0].replace("void ", ""))
    lb = {k["name"] for k in base if not is_xck(k)}; ln = {k["name"] for k in new if not is_xck(k)}
    per_unit = {}
    for k in new:
        if not is_xck(k): per_unit[k["unit"]] = per_unit.get(k["unit"], 0) + 1
    print("\nlibrary kernels (by mangled name): base %d, new %d (%s); only in base %d, only in new %d" %
          (len(lb), len(ln), ", ".join("%s %d" % u for u in sorted(per_unit.items())) or "none", len(lb - ln), len(ln - lb)))
    for n in sorted(lb ^ ln): print("   ", "-" if n in lb else "+", n)
    lib_b = {k["name"]: k for k in base if not is_xck(k)}
    lib_diff = [k["name"] for k in new if not is_xck(k) and k["name"] in lib_b and (lib_b[k["name"]]["res"], lib_b[k["name"]]["sha"]) != (k["res"], k["sha"])]
    print("library kernels whose resources or instruction text differ: %d" % len(lib_diff))
    for n in lib_diff: print("   ", n)
    sys.exit(1 if bad or lib_diff or (lb ^ ln) else 0)


if __name__ == "__main__":
    main()
