"""Compare the gfx950 device assembly of csrc files between a parent revision and the working tree, kernel by kernel.

    python tools/asm_compare.py PARENT_REV file.hip [file.hip ...] [--title "..."] > profiles/<name>_asm.log

Each file is compiled at both trees with build.CXXFLAGS plus the file's EXTRA_FLAGS plus --cuda-device-only -S
-Rpass-analysis=kernel-resource-usage, once with VIP_BUILD_EXPERIMENTS=0 and once with =1.  Per kernel symbol the instruction text
(comments, directives and the function index in block labels stripped) and every line of the resource remark are compared:
identical = same text; reordered = the same multiset of lines in another order with an equal remark (the moved lines are printed,
for a reader to judge); changed = anything else (a short diff is printed).  The script only diffs text.
"""
import argparse
import collections
import difflib
import importlib.util
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "vip-cup-2022_amd"
_spec = importlib.util.spec_from_file_location("vip_build", os.path.join(ROOT, PKG, "build.py"))
build = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(build)


def compile_asm(tree, name, exp):
    """-> {demangled kernel: (instruction lines, remark lines)} of csrc/<name> in `tree`"""
    flags = [f for f in build.CXXFLAGS if not f.startswith(("-I", "-DVIP_BUILD_EXPERIMENTS"))]
    flags += [f"-Iinclude", f"-I{PKG}/csrc", f"-DVIP_BUILD_EXPERIMENTS={exp}", *build.EXTRA_FLAGS.get(name, [])]
    cmd = [build.HIPCC, *flags, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-x", "hip",
           f"{PKG}/csrc/{name}", "-o", "-"]
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {name} in {tree}:\n{r.stderr}")
    remarks, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = remarks.setdefault(text.split(":", 1)[1].strip(), [])
        elif cur is not None:
            cur.append(text)
    kernels = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", r.stdout, re.M)
    bodies = {}
    for sym in kernels:
        m = re.search(rf"^{re.escape(sym)}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", r.stdout, re.M | re.S)
        lines = []
        for line in m.group(1).splitlines():
            line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";", 1)[0]).strip()
            if line and (not line.startswith(".") or line.endswith(":")):
                lines.append(line)
        bodies[sym] = lines
    names = subprocess.run(["c++filt", *kernels], capture_output=True, text=True, check=True).stdout.splitlines() if kernels else []
    return {n: (bodies[s], remarks.get(s, [])) for s, n in zip(kernels, names)}


def compare(parent, head, out):
    counts = collections.Counter()
    for k in [k for k in head if k in parent]:
        (pl, pr), (hl, hr) = parent[k], head[k]
        if pl == hl and pr == hr:
            kind = "identical"
        elif collections.Counter(pl) == collections.Counter(hl) and pr == hr:
            kind = "reordered"
        else:
            kind = "changed"
        counts[kind] += 1
        print(f"{kind:<10} {k}  [{len(pl)} -> {len(hl)} lines]", file=out)
        print(f"    parent: {'; '.join(pr)}\n    head: {'; '.join(hr)}", file=out)
        if kind != "identical":
            diff = [d for d in difflib.unified_diff(pl, hl, "parent", "head", n=0, lineterm="") if not d.startswith(("---", "+++"))]
            for d in diff[:80]:
                print("    | " + d, file=out)
            if len(diff) > 80:
                print(f"    | ... {len(diff) - 80} more diff lines", file=out)
    return counts


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("files", nargs="+")
    ap.add_argument("--title", default="Device assembly")
    args = ap.parse_args()
    rev = subprocess.run(["git", "rev-parse", "--short", args.parent], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    print(f"{args.title}: {', '.join('csrc/' + f for f in args.files)}, parent commit ({rev}) against the working tree.\n"
          "Every translation unit compiled for gfx950 with the build's flags (build.CXXFLAGS + EXTRA_FLAGS), once with\n"
          "VIP_BUILD_EXPERIMENTS=0 and once with =1, plus --cuda-device-only -S -Rpass-analysis=kernel-resource-usage; compared per kernel\n"
          "symbol: instruction text (comments, directives and the function index in block labels stripped) and every line of the\n"
          "resource remark.\n"
          "identical = same instruction text; reordered = the same multiset of instructions in another order, resource remark equal;\n"
          "changed = anything else.\n")
    total = collections.Counter()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "archive", "--format=tar", args.parent, f"{PKG}/csrc", "include"], cwd=ROOT, capture_output=True,
                             check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        jobs = [(tree, f, exp) for exp in (0, 1) for f in args.files for tree in (tmp, ROOT)]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            res = dict(zip(jobs, ex.map(lambda j: compile_asm(*j), jobs)))
    for exp in (0, 1):
        for f in args.files:
            p, h = res[(tmp, f, exp)], res[(ROOT, f, exp)]
            print(f"== {f}, VIP_BUILD_EXPERIMENTS={exp}: {len(p)} kernels at parent, {len(h)} at head; same set: {set(p) == set(h)}")
            for k in sorted(set(p) ^ set(h)):
                print(f"only at {'parent' if k in p else 'head'}: {k}")
            total += compare(p, h, sys.stdout)
    print(f"\ntotal over both builds: {total['identical']} identical, {total['reordered']} reordered, {total['changed']} changed")
    return 1 if total["changed"] else 0


if __name__ == "__main__":
    sys.exit(main())
