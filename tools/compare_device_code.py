#!/usr/bin/env python
"""Kernel-by-kernel comparison of the device code of two builds (no GPU needed):

    python tools/compare_device_code.py OLD_DIR NEW_DIR [--drop-template-arg KERNEL:INDEX ...]

OLD_DIR / NEW_DIR hold the gfx950 assembly `hipcc --save-temps` leaves beside the objects
(`*-hip-amdgcn-amd-amdhsa-gfx950.s`; build with `make CXXFLAGS="... --save-temps"`).  Every kernel's body is compared
with its labels normalised and comments stripped, and its descriptor (registers, scratch, LDS: the numbers
tools/resource_usage.py prints) line by line.  `--drop-template-arg esplit_pass:4` matches a kernel of OLD whose
template lost its argument 4 (counted from 0) with the kernel of NEW that has the remaining arguments.
Prints counts, the kernels only one side has, the name map of renamed kernels and every differing pair; exit status 1
if a matched pair differs or NEW has a kernel OLD lacks."""
import glob
import os
import re
import subprocess
import sys


def demangle(names):
    filt = "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([filt if os.path.exists(filt) else "c++filt"], input="\n".join(names), capture_output=True, text=True)
    return [re.sub(r"\(anonymous namespace\)::", "", ln).replace("void ", "", 1).split("(")[0] for ln in out.stdout.splitlines()]


def kernels(directory):
    """{demangled name: (normalised body lines, descriptor lines)} of every kernel in the directory's assembly."""
    found = {}
    for path in sorted(glob.glob(os.path.join(directory, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        text = open(path).read()
        unit = os.path.basename(path).split("-hip-")[0]
        for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, flags=re.S | re.M):
            name, desc = m.group(1), [ln.strip() for ln in m.group(2).splitlines()]
            start = text.index("\n%s:" % name)
            end = text.index("\n.Lfunc_end", start)
            body = []
            for ln in text[start:end].splitlines()[2:]:
                ln = ln.split(";")[0].rstrip()
                ln = re.sub(r"\.LBB\d+_", ".LBB_", ln).replace(name, "<self>")
                if ln.strip():
                    body.append(ln)
            found[(unit, name)] = (body, [d.replace(name, "<self>") for d in desc])
    keys = list(found)
    names = demangle([k[1] for k in keys])
    return {"%s: %s" % (k[0], n): found[k] for k, n in zip(keys, names)}


def drop_arg(name, kernel, index):
    m = re.match(r"^(\S+: %s)<(.*)>$" % re.escape(kernel), name)
    if not m:
        return name
    args = [a.strip() for a in m.group(2).split(",")]  # (integral and boolean arguments only: no nested commas)
    return "%s<%s>" % (m.group(1), ", ".join(a for i, a in enumerate(args) if i != index))


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    drops = [a.split(":") for a in sys.argv[4:]] if len(sys.argv) > 3 and sys.argv[3] == "--drop-template-arg" else []
    old, new = kernels(old_dir), kernels(new_dir)
    renamed, removed = {}, []
    for name in sorted(old):
        if name in new:
            continue
        cand = name
        for kernel, index in drops:
            cand = drop_arg(cand, kernel, int(index))
        if cand in new and cand not in old and cand not in renamed.values():
            renamed[name] = cand
        else:
            removed.append(name)
    added = sorted(n for n in new if n not in old and n not in renamed.values())
    pairs = [(n, n) for n in sorted(old) if n in new] + sorted(renamed.items())
    differing = []
    for o, n in pairs:
        if old[o][0] != new[n][0] or old[o][1] != new[n][1]:
            ops = lambda body: sorted(ln.split()[0] for ln in body if ln.startswith("\t") and not ln.strip().startswith("."))
            what = "same" if old[o][0] == new[n][0] else "DIFFERS (%d / %d lines, opcode multiset %s)" % (
                len(old[o][0]), len(new[n][0]), "same" if ops(old[o][0]) == ops(new[n][0]) else "differs")
            differing.append((o, n, what, [(a, b) for a, b in zip(old[o][1], new[n][1]) if a != b]))
    print("kernels: old %d, new %d; matched by name %d, matched after renaming %d, only in old %d, only in new %d"
          % (len(old), len(new), len(pairs) - len(renamed), len(renamed), len(removed), len(added)))
    print("matched pairs with identical body and descriptor: %d of %d" % (len(pairs) - len(differing), len(pairs)))
    print("\nonly in old (%d):" % len(removed))
    for n in removed:
        print("  " + n)
    print("\nonly in new (%d):" % len(added))
    for n in added:
        print("  " + n)
    print("\nrenamed (%d):" % len(renamed))
    for o, n in sorted(renamed.items()):
        print("  %s  ->  %s" % (o, n.split(": ", 1)[1]))
    print("\ndiffering pairs (%d):" % len(differing))
    for o, n, body, desc in differing:
        print("  %s%s: body %s, descriptor lines %s" % (o, "" if o == n else " -> " + n, body, desc or "same"))
    return 1 if differing or added else 0


if __name__ == "__main__":
    sys.exit(main())
