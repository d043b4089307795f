#!/usr/bin/env python3
"""Do two source trees compile to the same GPU kernels?  (no GPU needed)

Every .hip unit of lidar_imu_init_amd/csrc in both trees is compiled device-only to assembly with the flags of that tree's
Makefile (FLAGS and its per-object additions).  For every kernel symbol the two trees are compared on
  * the instruction stream - comments stripped, local labels (.L...) renumbered in order of appearance;
  * the .amdhsa_kernel descriptor block (VGPR / SGPR counts, LDS bytes, scratch, ...).
Whole streams are compared; a kernel may have moved to another unit.  One line per kernel, exit status 1 on any difference.

usage: kernel_isa_diff.py <tree A> <tree B> [--jobs N] [--keep DIR]
"""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join("lidar_imu_init_amd", "csrc")


def makefile_flags(csrc):
    """(common flags, {unit stem: extra flags}) as the Makefile gives them to hipcc"""
    text = open(os.path.join(csrc, "Makefile")).read()
    var = {"ARCH": "gfx950", "EXTRA": ""}
    m = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M)
    if m:
        var["ARCH"] = m.group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    flags = re.sub(r"\$\((\w+)\)", lambda v: var.get(v.group(1), ""), flags).split()
    per_unit = {}
    for stem, add in re.findall(r"^\$\(OBJ\)/(\w+)\.o:\s*FLAGS\s*\+=\s*(.*)$", text, re.M):
        per_unit.setdefault(stem, []).extend(add.split())
    return flags, per_unit


def compile_unit(hipcc, src, flags, out):
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stdout))
    return out


def strip_line(line):
    return re.sub(r"\s+", " ", line.split(";", 1)[0]).strip()


def kernels_of(asm_path):
    """{symbol: (instruction stream, descriptor block)} of one assembly file"""
    lines = [strip_line(l) for l in open(asm_path)]
    desc, start = {}, {}
    i = 0
    while i < len(lines):
        m = re.match(r"\.amdhsa_kernel (\S+)$", lines[i])
        if m:
            j = lines.index(".end_amdhsa_kernel", i)
            desc[m.group(1)] = [l for l in lines[i + 1:j] if l]
            i = j
        i += 1
    for i, l in enumerate(lines):
        if l.endswith(":") and l[:-1] in desc:
            start[l[:-1]] = i
    out = {}
    for sym, i in start.items():
        body, labels = [], {}
        for l in lines[i + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            if l:
                body.append(re.sub(r"\.L\w+", lambda v: labels.setdefault(v.group(0), ".L%d" % len(labels)), l))
        out[sym] = (body, desc[sym])
    missing = set(desc) - set(out)
    if missing:
        raise RuntimeError("%s: no code found for %s" % (asm_path, sorted(missing)))
    return out


def tree_kernels(tree, hipcc, jobs, keep):
    csrc = os.path.join(tree, CSRC)
    flags, per_unit = makefile_flags(csrc)
    units = sorted(glob.glob(os.path.join(csrc, "*.hip")))
    os.makedirs(keep, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        futs = {}
        for src in units:
            stem = os.path.splitext(os.path.basename(src))[0]
            futs[stem] = ex.submit(compile_unit, hipcc, src, flags + per_unit.get(stem, []), os.path.join(keep, stem + ".s"))
        found = {}
        for stem, f in futs.items():
            for sym, k in kernels_of(f.result()).items():
                if sym in found:
                    raise RuntimeError("%s: kernel %s is defined in %s and in %s" % (tree, sym, found[sym][0], stem))
                found[sym] = (stem,) + k
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--hipcc", default=os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    ap.add_argument("--keep", help="keep the assembly files under DIR/a and DIR/b")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        keep = a.keep or tmp
        ka = tree_kernels(a.tree_a, a.hipcc, a.jobs, os.path.join(keep, "a"))
        kb = tree_kernels(a.tree_b, a.hipcc, a.jobs, os.path.join(keep, "b"))
    bad = 0
    for sym in sorted(set(ka) | set(kb)):
        if sym not in ka or sym not in kb:
            verdict = "ONLY IN %s (%s)" % (("A", ka[sym][0]) if sym in ka else ("B", kb[sym][0]))
        else:
            (ua, ca, da), (ub, cb, db) = ka[sym], kb[sym]
            what = [w for w, x, y in (("code", ca, cb), ("descriptor", da, db)) if x != y]
            where = ua if ua == ub else "%s -> %s" % (ua, ub)
            verdict = ("DIFFERENT %s" % " + ".join(what) if what else "same %6d lines" % len(ca)) + "  " + where
        bad += not verdict.startswith("same")
        print("%-34s %s" % (verdict, sym))
    print("%d kernels, %d differ" % (len(set(ka) | set(kb)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
