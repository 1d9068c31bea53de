#!/usr/bin/env python3
"""Do two builds of one translation unit give every kernel the same code?   python profiles/isa_diff.py OLD.s NEW.s [--map NAMES.map]

OLD.s / NEW.s: hipcc --cuda-device-only -S output of the same unit before and after a change.  Per kernel (matched by demangled name) the
instruction stream -- comments, directives and labels stripped, basic-block labels renumbered without the function's index -- and the
kernel descriptor (.amdhsa_* lines: registers, scratch, LDS) are compared line for line.  NAMES.map renames OLD's kernels first: lines of
`regex => replacement` applied to the demangled name (re.sub), for a change that renames kernels or their template parameters.
Prints one line per unit and the first differing line of each differing kernel; exit status 1 if any kernel differs, is missing or is new."""
import argparse
import os
import re
import subprocess
import sys


def kernels(path, cxxfilt):
    src = open(path).read().splitlines()
    desc, streams, i = {}, {}, 0
    while i < len(src):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", src[i])
        if m:
            j = next(k for k in range(i, len(src)) if src[k].strip() == ".end_amdhsa_kernel")
            desc[m.group(1)] = [l.strip() for l in src[i + 1:j]]
            i = j
        i += 1
    for i, l in enumerate(src):
        m = re.match(r"^(\S+):", l)
        if not m or m.group(1) not in desc:
            continue
        body = []
        for l2 in src[i + 1:]:
            t = l2.split(";")[0].strip()
            if t.startswith(".Lfunc_end"):
                break
            if t and not t.startswith(".") and not t.endswith(":"):
                body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", " ".join(t.split())))
        streams[m.group(1)] = body
    names = list(desc)
    dem = subprocess.run([cxxfilt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return {d: (streams[n], desc[n]) for n, d in zip(names, dem)}


ap = argparse.ArgumentParser()
ap.add_argument("old")
ap.add_argument("new")
ap.add_argument("--map")
ap.add_argument("--cxxfilt", default=os.environ.get("CXXFILT", "c++filt"))
args = ap.parse_args()
rules = []
for line in open(args.map) if args.map else []:
    if line.strip() and not line.startswith("#"):
        pat, rep = line.rstrip("\n").split(" => ")
        rules.append((re.compile(pat), rep))
old = {}
for name, v in kernels(args.old, args.cxxfilt).items():
    for pat, rep in rules:
        name = pat.sub(rep, name)
    old[name] = v
new = kernels(args.new, args.cxxfilt)
bad = 0
for name in sorted(set(old) | set(new)):
    if name not in old or name not in new:
        print(f"  only in {'NEW' if name in new else 'OLD'}: {name}")
        bad += 1
        continue
    for what, a, b in (("instructions", old[name][0], new[name][0]), ("descriptor", old[name][1], new[name][1])):
        if a != b:
            k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"  {what} differ in {name}: {len(a)} / {len(b)} lines, first at {k}: {a[k:k + 1]} | {b[k:k + 1]}")
            bad += 1
            break
print(f"{os.path.basename(args.new)}: {len(new)} kernels, {sum(len(v[0]) for v in new.values())} instructions, {bad} differing")
sys.exit(1 if bad else 0)
