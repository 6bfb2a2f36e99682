#!/usr/bin/env python3
"""isa_diff.py — show, without a GPU, that a change left the kernels' code as it was.

    tools/isa_diff.py OLD NEW kernels.hip shard_f32_kernels.hip ... [--rename OLD=NEW] [--out FILE]

OLD and NEW are two `tenstorrentallreduce_amd` directories (OLD: a `git worktree` or `git archive`
of the commit to compare against).  Every listed csrc/*.hip file is compiled in each tree that has
it with the Makefile's HIPFLAGS plus `--offload-device-only -S`; the kernels of a tree's files are
pooled, so a kernel may move between files.  The assembly is split per kernel, names demangled,
comments dropped and the basic-block label numbers (.LBB<n>_) normalised, and the two sides are
compared kernel by kernel: `identical`, or the number of differing lines and the first few, then
both sides' resource figures (VGPRs, SGPRs, LDS bytes, scratch bytes).  A diff and nothing else.
Exit status: 0 all identical, 1 some kernel differs, 2 a kernel is missing on one side.
"""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROCM = os.environ.get("ROCM", "/opt/rocm")
RESOURCES = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
             ("lds", ".amdhsa_group_segment_fixed_size"), ("scratch", ".amdhsa_private_segment_fixed_size"))


def split_kernels(asm):
    """{mangled name: [lines]} — a kernel's body from its label to .Lfunc_end, then its .amdhsa_kernel block."""
    out, kernels = {}, set()
    name, lines = None, None
    for line in asm.splitlines():
        s = line.strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            name, lines = m.group(1), out.setdefault(m.group(1), [])
            kernels.add(name)
            continue   # like the label below, the line holds the name: not part of what is compared
        if name is None:
            m = re.match(r"([A-Za-z_$][\w$.]*):", s)
            if m and not m.group(1).startswith(".L"):
                name, lines = m.group(1), out.setdefault(m.group(1), [])
                continue
        if name is not None:
            lines.append(line)
            if s.startswith(".Lfunc_end") or s == ".end_amdhsa_kernel":
                name = None
    return {k: v for k, v in out.items() if k in kernels}


def normalise(lines):
    """comments and blank lines dropped, white space collapsed, .LBB<n>_<m> -> .LBB_<m>"""
    out = []
    for line in lines:
        s = " ".join(line.split(";", 1)[0].split())
        if s:
            out.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", s)))
    return out


def resources(lines):
    got = {}
    for s in lines:
        for key, directive in RESOURCES:
            if s.startswith(directive + " "):
                got[key] = int(s.split()[1], 0)
    return got


def base_name(demangled):
    """`void ns::(anonymous namespace)::k<8, false>(args)` -> `k<8, false>`: no return type, scope or parameters"""
    depth, end = 0, len(demangled)
    for i, ch in enumerate(demangled):   # the parameter list opens at the first '(' outside <> that is no "(anonymous"
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0 and not demangled.startswith("(anonymous namespace)", i):
            end = i
            break
    head, depth, start = demangled[:end], 0, 0
    for i, ch in enumerate(head):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif depth == 0 and (ch == " " or head.startswith("::", i - 1)):
            start = i + 1
    return head[start:].replace("tsa::", "").replace("(anonymous namespace)::", "")


def rename(name, renames):
    for old, new in renames:
        m = re.match(re.escape(old) + r"(?![\w])", name)
        if m:
            return new + name[m.end():]
    return name


def pair(old, new, renames=()):
    """old, new: {name: normalised lines}.  -> [(old name, new name or None)], [new names without an old one]"""
    pairs, taken = [], set()
    for name in sorted(old):
        target = rename(name, renames)
        pairs.append((name, target if target in new else None))
        taken.add(target)
    return pairs, sorted(n for n in new if n not in taken)


def compare(a, b, show=6):
    """-> (number of differing lines, the first `show` of them as unified-diff lines)"""
    diff = [d for d in difflib.unified_diff(a, b, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---")]
    return len(diff), diff[:show]


def makefile_flags(tree):
    """HIPFLAGS of the tree's Makefile, its := / ?= variables expanded"""
    text = open(os.path.join(tree, "Makefile")).read()
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}

    def expand(s, depth=0):
        return re.sub(r"\$\((\w+)\)", lambda m: expand(var.get(m.group(1), ""), depth + 1), s) if depth < 8 else s
    return expand(var["HIPCC"]), expand(var["HIPFLAGS"]).split()


def assemble(tree, name):
    hipcc, flags = makefile_flags(tree)
    extra = []
    if name == "kernels.hip":
        subprocess.run(["make", "-s", "build/lo_dag_gen.inc"], cwd=tree, check=True, stdout=subprocess.DEVNULL)
        extra = ["-Ibuild"]
    r = subprocess.run([hipcc, *flags, *extra, "--offload-device-only", "-S", "-o", "-", os.path.join("csrc", name)],
                       cwd=tree, check=True, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
    return r.stdout


def demangle(names):
    """ROCm's llvm-cxxfilt where the installation has it, else the c++filt on PATH (both read Itanium names)"""
    names = list(names)
    tools = [os.path.join(ROCM, d, "llvm-cxxfilt") for d in ("lib/llvm/bin", "llvm/bin")]
    tool = next((t for t in tools if os.path.exists(t)), None) or shutil.which("llvm-cxxfilt") or "c++filt"
    r = subprocess.run([tool], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def tree_kernels(tree, files, jobs):
    here = [f for f in files if os.path.exists(os.path.join(tree, "csrc", f))]
    with ThreadPoolExecutor(jobs) as ex:
        texts = list(ex.map(lambda f: assemble(tree, f), here))
    out = {}
    for f, text in zip(here, texts):
        ks = split_kernels(text)
        names = demangle(ks)
        for mangled, lines in ks.items():
            out[base_name(names[mangled])] = normalise(lines)
    return out, here


def fmt(res):
    return "vgpr %3d  sgpr %3d  lds %6d  scratch %d" % tuple(res.get(k, -1) for k, _ in RESOURCES)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("files", nargs="+", help="names of .hip files under csrc/ (one missing in a tree is left out there)")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW", help="a kernel base name that changed")
    ap.add_argument("--show", type=int, default=6, help="differing lines printed per kernel")
    ap.add_argument("--out", help="write the report here as well")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in a.rename]
    old, old_files = tree_kernels(a.old, a.files, a.j)
    new, new_files = tree_kernels(a.new, a.files, a.j)
    pairs, extra = pair(old, new, renames)
    report = ["old: %s  (%d kernels)" % (" ".join(old_files), len(old)), "new: %s  (%d kernels)" % (" ".join(new_files), len(new))]
    same = differ = missing = 0
    for o, n in pairs:
        if n is None:
            missing += 1
            report.append("%s: MISSING in new" % o)
            continue
        count, first = compare(old[o], new[n], a.show)
        title = o if o == n else "%s -> %s" % (o, n)
        ro, rn = resources(old[o]), resources(new[n])
        if count == 0:
            same += 1
            report.append("%s: identical  (%d lines; %s)" % (title, len(old[o]), fmt(ro)))
        else:
            differ += 1
            report.append("%s: %d lines differ of %d / %d" % (title, count, len(old[o]), len(new[n])))
            report += ["    " + d for d in first]
            report += ["    old  " + fmt(ro), "    new  " + fmt(rn)]
    for n in extra:
        missing += 1
        report.append("%s: MISSING in old" % n)
    report.append("%d identical, %d differ, %d missing" % (same, differ, missing))
    text = "\n".join(report) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 2 if missing else 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
