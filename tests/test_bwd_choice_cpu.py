"""Which kernel the render backward runs, asked of the library without a GPU (vl3d_render_bwd_choice: the function the entry points call,
csrc/vl3d_render_bwd_choice.h): one named case per promise of include/vl3d.h and the chooser's comments, a sweep over variants x entries x
flags x sizes (the shape is a row of the table, the scratch holds it), the scratch size against the values recorded before the layout was
sized from the table, and the chooser's header on its own under plain g++ and the host sanitizers."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {(64, 16), (64, 8), (32, 16), (64, 12)}      # the region shapes (BWD_REGIONS); interiors are 2 less each way


@pytest.fixture(scope="module")
def R():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import render
    return render


def desc_of(T=50, scale=1.0, variant=0, spec="mpv", dtype=0, D=32, H=720, W=1280, uv=0, gcu=False, **spec_kw):
    from videoloop3d_amd.render import RenderSpec, _desc_dims
    s = RenderSpec.mpv(variant=variant, **spec_kw) if spec == "mpv" else RenderSpec(variant=variant, uv_noise_seed=0, **spec_kw)
    d = _desc_dims(D, T, int(H * scale), int(W * scale), H, W, s, dtype)
    d.uv_noise_seed = uv
    d.grad_flags = 1 if gcu else 0
    return d


def choice(R, d, entry="render", qk=False, reg=False, scratch_bytes=None):
    c = R.bwd_choice(d, entry, qk, reg, scratch_bytes)
    family = {0: "atomics", 1: "tile", 2: "pair", 3: "pair12"}[c.family]
    flags = "".join(n for n, v in (("REG ", c.reg), ("MASK ", c.mask), ("ADAM ", c.adam), ("CULL ", c.cull), ("F16 ", c.f16)) if v).strip()
    return (family, c.width, c.rows, flags)


# (name, descriptor arguments, call arguments, expected (family, width, rows, flags))
CASES = [
    ("cfg3 variant 0", dict(), dict(), ("pair12", 64, 12, "")),
    ("cfg3 variant 6", dict(variant=6), dict(), ("pair", 32, 16, "")),
    ("cfg3 variant 7", dict(variant=7), dict(), ("pair12", 64, 12, "")),
    ("cfg3 variant 3", dict(variant=3), dict(), ("tile", 64, 16, "")),
    ("cfg3 variant 4", dict(variant=4), dict(), ("tile", 64, 16, "")),
    ("cfg3 variant 1", dict(variant=1), dict(), ("atomics", 0, 0, "")),
    ("cfg3 short scratch", dict(), dict(scratch_bytes=1 << 20), ("atomics", 0, 0, "")),
    ("cfg3 no scratch", dict(), dict(scratch_bytes=0), ("atomics", 0, 0, "")),
    ("cfg3 uv noise", dict(uv=7), dict(), ("atomics", 0, 0, "")),
    ("1.1x stack", dict(scale=1.1), dict(), ("tile", 64, 16, "")),
    ("1.1x stack, regularisers", dict(scale=1.1), dict(reg=True), ("pair", 32, 16, "REG")),
    ("1.1x stack, regularisers, utils_mpi", dict(scale=1.1, spec="utils_mpi"), dict(reg=True), ("tile", 64, 16, "REG")),
    ("T = 1 variant 0", dict(T=1), dict(), ("tile", 64, 8, "")),
    ("T = 1 variant 3", dict(T=1, variant=3), dict(), ("tile", 64, 16, "")),
    ("T = 1 fp16 stack", dict(T=1, dtype=1), dict(), ("tile", 64, 16, "F16")),
    ("quad map without gcu", dict(), dict(qk=True), ("tile", 64, 16, "CULL")),
    ("quad map with gcu, variant 0", dict(gcu=True), dict(qk=True), ("tile", 32, 16, "CULL")),
    ("quad map with gcu, variant 3", dict(gcu=True, variant=3), dict(qk=True), ("tile", 64, 16, "REG CULL")),
    ("mask entry, default", dict(T=1), dict(entry="mask"), ("tile", 64, 8, "MASK")),
    ("mask entry, variant 3", dict(T=1, variant=3), dict(entry="mask"), ("tile", 64, 16, "MASK")),
    ("fused step, dense", dict(), dict(entry="adam"), ("pair", 32, 16, "ADAM")),
    ("fused step, culled", dict(), dict(entry="adam", qk=True), ("tile", 32, 16, "REG ADAM CULL")),
    ("fused step, culled, variant 3", dict(variant=3), dict(entry="adam", qk=True), ("tile", 64, 16, "REG ADAM CULL")),
    ("variant 6 with regularisers", dict(variant=6), dict(reg=True), ("tile", 64, 16, "REG")),
    ("variant 7 with regularisers", dict(variant=7), dict(reg=True), ("tile", 64, 16, "REG")),
    ("(none, sigmoid) activations", dict(rgb_act="none"), dict(), ("tile", 64, 16, "")),
    # ... and the rest of include/vl3d.h's variant paragraph
    ("cfg3 variant 2", dict(variant=2), dict(), ("tile", 64, 8, "")),
    ("cfg3 variant 5", dict(variant=5), dict(), ("tile", 32, 16, "")),
    ("variant 5, utils_mpi", dict(variant=5, spec="utils_mpi"), dict(), ("tile", 64, 16, "")),
    ("variant 2 with regularisers", dict(variant=2), dict(reg=True), ("tile", 64, 16, "REG")),
    ("variant 5, quad map with gcu", dict(variant=5, gcu=True), dict(qk=True), ("tile", 32, 16, "REG CULL")),
    ("cfg3 regularisers", dict(), dict(reg=True), ("pair", 32, 16, "REG")),
    ("fp16 stack at the frame's size", dict(dtype=1), dict(), ("pair12", 64, 12, "F16")),
    ("mask entry, variant 1", dict(T=1, variant=1), dict(entry="mask"), ("atomics", 0, 0, "")),
    ("mask entry, regularisers", dict(T=1), dict(entry="mask", reg=True), ("tile", 64, 8, "REG MASK")),
]


@pytest.mark.parametrize("name,dkw,ckw,want", CASES, ids=[c[0] for c in CASES])
def test_named_choice(R, name, dkw, ckw, want):
    assert choice(R, desc_of(**dkw), **ckw) == want


def test_gather_and_owner_table_switches(R):
    c = R.bwd_choice(desc_of(variant=4))
    assert (c.gather9, c.owner4) == (1, 0)
    assert [R.bwd_choice(desc_of(T=1, variant=v)).owner4 for v in (0, 2, 3, 4, 5)] == [1, 1, 0, 0, 1]      # four texels per thread: T = 1, not 3 / 4
    assert R.bwd_choice(desc_of(T=1), "mask").owner4 == 1 and R.bwd_choice(desc_of(T=2)).owner4 == 0
    assert R.bwd_choice(desc_of(), "adam", True).owner4 == 0


def test_refusals_are_the_entries(R):
    from videoloop3d_amd import _lib as L
    out = L.BwdChoice()

    def rc(d, entry, qk=0, fused=None, scratch=1 << 40):
        return L.lib().vl3d_render_bwd_choice(d, entry, qk, 0, scratch, int(entry == 2) if fused is None else fused, L.C.byref(out))
    assert rc(desc_of(), 0) == 0
    assert rc(desc_of(variant=0x10), 0) == 1                       # check_desc: ablation bits
    assert rc(desc_of(D=0), 0) == 1
    assert rc(desc_of(spec="utils_mpi", T=1), 1) == 3              # the mask channel's convention
    assert rc(desc_of(T=1), 2) == 3 and rc(desc_of(variant=5), 2) == 3 and rc(desc_of(variant=5), 2, qk=1) == 0      # the fused step's descriptors
    assert rc(desc_of(), 2, scratch=64) == 1                       # ... and its scratch
    planes = desc_of()
    planes.coord_mode = 2                                          # VL3D_COORD_AFFINE_PLANES: no tile culling, as check_cull says
    assert rc(planes, 0) == 0 and rc(planes, 0, qk=1) == 1
    unbuilt = desc_of()
    unbuilt.border_mode = 0                                        # (affine, zeros, post): no such convention, the dispatch's refusal
    assert rc(unbuilt, 0) == 3
    assert rc(desc_of(), 3) == 1 and rc(desc_of(), 0, fused=1) == 1 and rc(desc_of(), 2, fused=0) == 1
    assert L.lib().vl3d_render_bwd_choice(desc_of(), 0, 0, 0, 0, 0, None) == 1


def scratch_needed(D, H, W, Hs, Ws, width, rows):
    """bytes a backward in width x rows regions addresses in its scratch, from the layout alone: 16 header words + 12 per plane rounded up
    to 4 words, one 16-byte window per (tile, plane), the owner table behind them at the next 256 bytes, 2 bytes per (plane, texel) + the
    gather's prefetch padding of 16 rows + 64 texels"""
    tiles = -(-W // (width - 2)) * -(-H // (rows - 2))
    windows_end = ((16 + 12 * D + 3) & ~3) * 4 + tiles * D * 16
    return ((windows_end + 255) & ~255) + (D * Hs * Ws + 16 * Ws + 64) * 2


def test_sweep_shape_is_a_table_row_and_the_scratch_holds_it(R):
    from videoloop3d_amd import _lib as L
    seen = set()
    sizes = [(13, 61, 1.0), (33, 131, 1.0), (6, 61, 1.0), (200, 200, 1.1), (7, 29, 1.0), (720, 1280, 1.0)]
    for (H, W, scale), T, D in itertools.product(sizes, (1, 3), (1, 5)):
        for variant, entry, qk, reg, gcu, spec, dtype in itertools.product(range(16), ("render", "mask", "adam"), (False, True), (False, True),
                                                                         (False, True), ("mpv", "utils_mpi"), (0, 1)):
            d = desc_of(T=T, scale=scale, variant=variant, spec=spec, dtype=dtype, D=D, H=H, W=W, gcu=gcu)
            out = L.BwdChoice()
            need = int(L.lib().vl3d_render_bwd_scratch_bytes(d))
            rc = L.lib().vl3d_render_bwd_choice(d, L.BWD_ENTRY[entry], int(qk), int(reg), need, int(entry == "adam"), L.C.byref(out))
            if rc != 0:      # the entry refuses the descriptor (mask / fused step: the shipped convention; a quad map at the mask entry; ...)
                assert entry != "render"
                continue
            if out.family == 0:
                assert variant == 1 and (out.width, out.rows) == (0, 0)
                continue
            assert (out.width, out.rows) in SHAPES
            assert (out.family == 3) == ((out.width, out.rows) == (64, 12)) and (out.family != 2 or (out.width, out.rows) == (32, 16))
            assert scratch_needed(D, H, W, d.Hs, d.Ws, out.width, out.rows) <= need
            seen.add((out.family, out.width, out.rows, out.reg, out.mask, out.adam, out.cull, out.f16))
    assert {(s[1], s[2]) for s in seen} == SHAPES and {s[0] for s in seen} == {1, 2, 3}


def test_scratch_bytes_are_what_they_were(R):
    """vl3d_render_bwd_scratch_bytes is ABI (callers allocate by it; an entry takes the owner-computes path only when given that many): sized
    from the shape table it returns, for every frame of 1..200 x 1..200 pixels, the value recorded from the library of the commit before (the
    literal list of interiors; tests/golden/make_bwd_scratch_bytes.py is the recipe) -- tests/golden/bwd_scratch_bytes.npz: D = 1 and 32 with the stack at the frame's size, D = 32 with a stack of
    (ceil(1.1 H), W + 3) texels"""
    from videoloop3d_amd import _lib as L
    ref = np.load(os.path.join(ROOT, "tests", "golden", "bwd_scratch_bytes.npz"))
    f = L.lib().vl3d_render_bwd_scratch_bytes
    d = L.RenderDesc()
    d.T = 1
    for i, D in enumerate(int(v) for v in ref["D"]):
        got = np.zeros((200, 200), dtype=np.int64)
        big = np.zeros((200, 200), dtype=np.int64)
        for H in range(1, 201):
            for W in range(1, 201):
                d.D, d.H, d.W, d.Hs, d.Ws = D, H, W, H, W
                got[H - 1, W - 1] = f(d)
                if D == 32:
                    d.Hs, d.Ws = (H * 11 + 9) // 10, W + 3
                    big[H - 1, W - 1] = f(d)
        assert np.array_equal(got, ref["stack_is_frame"][i]), D
        if D == 32:
            assert np.array_equal(big, ref["stack_larger"])


def test_the_chooser_stands_alone_under_the_host_sanitizers(tmp_path):
    """the header compiles with plain g++ -std=c++17 (no HIP), and the stand-alone program of the named cases runs clean under
    -fsanitize=address,undefined"""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the build environment"
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "videoloop3d_amd", "csrc")]
    exe = str(tmp_path / "bwd_choice_cases")
    # (the sanitizers' runtimes linked statically: the program does not depend on the order of the process's shared libraries)
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan"] + inc + [os.path.join(ROOT, "tests", "bwd_choice_cases.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "0 failed" in p.stdout
