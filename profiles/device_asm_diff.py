#!/usr/bin/env python3
"""Are two device-assembly files (hipcc --offload-arch=gfx950 ... --cuda-device-only -S -cuid=same) the same code in another order?
Usage: python profiles/device_asm_diff.py BEFORE.s AFTER.s   (exit code 0: the same).
hipcc emits kernels in instantiation order and numbers its labels by the function's ordinal in the file, so a host-side change that only moves
an instantiation renumbers `.LBB<n>_`, `.Lfunc_end<n>`, `.Ltmp<n>`, the `BB<n>_` in loop comments and the padding in front of those comments
in every function behind it.  This normalises exactly those, splits the file into the header, the per-kernel blocks and the metadata's
per-kernel entries, sorts the latter two by their text and compares."""
import re, sys, hashlib
def norm(path):
    lines = open(path).read().split('\n')
    # split into blocks at each ".section .text.<sym>" line; trailing metadata separately
    try:
        meta_i = next(i for i, l in enumerate(lines) if l.strip() == '.amdgpu_metadata')
    except StopIteration:
        meta_i = len(lines)
    body, meta = lines[:meta_i], lines[meta_i:]
    blocks, cur = [], []
    for l in body:
        if l.startswith('\t.section\t.text.') and cur:
            blocks.append(cur); cur = []
        cur.append(l)
    blocks.append(cur)
    def clean(b):
        t = '\n'.join(b)
        t = re.sub(r'BB\d+_', 'BBX_', t)
        t = re.sub(r'\.Lfunc_(end|begin)\d+', r'.Lfunc_\1X', t)
        t = re.sub(r'\.Ltmp\d+', '.LtmpX', t)
        t = re.sub(r'[ \t]+;', ' ;', t)      # (comment column: padded to the label's width)
        return t
    head, rest = blocks[0], sorted(clean(b) for b in blocks[1:])
    # metadata: kernel entries start with "  - .agpr_count" (first key of an entry)
    m = '\n'.join(meta)
    parts = re.split(r'\n(?=  - \.agpr_count)', m)
    mhead, ments = parts[0], parts[1:]
    tail = ''
    if ments:
        last = ments[-1]
        k = last.find('\namdhsa.target')
        if k >= 0:
            ments[-1], tail = last[:k], last[k:]
    return clean(head), rest, mhead, sorted(ments), tail
a, b = norm(sys.argv[1]), norm(sys.argv[2])
ok = a == b
print(sys.argv[1].split('/')[-1], 'kernel blocks', len(a[1]), len(b[1]), 'metadata entries', len(a[3]), len(b[3]), 'SAME AFTER SORT' if ok else 'DIFFERENT')
if not ok:
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y: print(' part', i, 'differs')
sys.exit(0 if ok else 1)
