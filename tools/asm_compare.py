#!/usr/bin/env python3
"""Compare two device-assembly listings of the same translation unit kernel by kernel.

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S chains.hip -o before.s      (at the parent)
    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S chains.hip -o after.s       (at the new tree)
    python tools/asm_compare.py before.s after.s [--all]

A kernel's text is its instruction lines with comments and the numbers of local labels stripped; its resources are what the
compiler prints behind it (VGPRs, SGPRs, LDS bytes, scratch bytes, occupancy - the figures of `make resources`). The script diffs
text and compares those figures; it looks for no particular instruction. Prints a markdown table: one line per kernel that differs
(--all: per kernel), then the counts. Exit status 1 when a kernel's LDS size, scratch size or occupancy differs, or a kernel is
missing on one side.
"""
import re
import subprocess
import sys

RES = {"vgpr": r"; NumVgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)", "lds": r"; LDSByteSize: (\d+)", "scratch": r"; ScratchSize: (\d+)",
       "occ": r"; Occupancy: (\d+)"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def kernels(path):
    """{mangled name: (instruction lines, resources)} of every .amdhsa kernel in the listing"""
    found, name, body = {}, None, []
    lines = open(path).read().split("\n")
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", ln)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None and ln.startswith(".Lfunc_end"):
            res, j = {}, i
            while j < len(lines) and len(res) < len(RES) and j < i + 400:
                for k, pat in RES.items():
                    mm = re.match(pat, lines[j])
                    if mm and k not in res:
                        res[k] = int(mm.group(1))
                j += 1
            found[name] = (body, res)
            name = None
        elif name is not None:
            t = ln.split(";")[0].strip()
            if t and not t.startswith("."):  # an instruction (directives and local labels start with a dot)
                body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", t))
        i += 1
    return found


def short(n):
    n = n.replace("void mldev::", "").replace("mldev::", "").replace("(ChainArgs)", "")
    return n


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    show_all = "--all" in sys.argv
    a, b = kernels(args[0]), kernels(args[1])
    names = demangle(sorted(set(a) | set(b)))
    same = differ = bad = 0
    print("| kernel | instructions | VGPRs | SGPRs | LDS | scratch | occupancy | text |")
    print("|---|---|---|---|---|---|---|---|")
    for mangled in sorted(names, key=lambda k: names[k]):
        if mangled not in a or mangled not in b:
            print("| `%s` | only in %s |" % (short(names[mangled]), "the first" if mangled in a else "the second"))
            bad += 1
            continue
        (ta, ra), (tb, rb) = a[mangled], b[mangled]
        identical = ta == tb and ra == rb
        same += identical
        differ += not identical
        if any(ra.get(k) != rb.get(k) for k in ("lds", "scratch", "occ")) or rb.get("scratch") != 0:
            bad += 1
        if identical and not show_all:
            continue

        def cell(k):
            return str(ra.get(k)) if ra.get(k) == rb.get(k) else "%s -> %s" % (ra.get(k), rb.get(k))

        n = str(len(ta)) if len(ta) == len(tb) else "%d -> %d" % (len(ta), len(tb))
        ops = lambda t: sorted(x.split()[0] for x in t)  # noqa: E731
        text = "identical" if ta == tb else ("the same operations in another order or other registers" if ops(ta) == ops(tb) else
                                             ("same count, other operations" if len(ta) == len(tb) else "%+d" % (len(tb) - len(ta))))
        print("| `%s` | %s | %s | %s | %s | %s | %s | %s |" % (short(names[mangled]), n, cell("vgpr"), cell("sgpr"), cell("lds"), cell("scratch"), cell("occ"), text))
    print()
    print("%d kernels: %d identical in text and resources, %d differ; %d with another LDS size, scratch or occupancy (or missing)" % (len(names), same, differ, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
