"""The five float render entries (vl3d_render_fwd, _fwd_frames, _fwd_reg, _reg_fwd, _bwd) off the device: each takes the quad map its
`_culled` twin took (header, library, binding; the twins are gone), refuses a malformed call with VL3D_EINVAL and a message that names it,
and reads a NULL map as a dense model whatever QH / QW say.  The refusals come before anything touches a device, so the pointers are
placeholders nothing reads -- which is why those tests do not run where a device exists: a refusal that went missing would launch a kernel
on them there, here it comes back as a HIP error code.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vl3d_render_fwd", "vl3d_render_fwd_frames", "vl3d_render_fwd_reg", "vl3d_render_reg_fwd", "vl3d_render_bwd"]
no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="placeholder addresses: a refusal that went missing would launch a kernel on them")
P = 64      # a non-null, aligned placeholder


def test_the_five_entries_take_a_quad_map_and_the_culled_twins_are_gone():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib as L
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vl3d.h")).read(), flags=re.S)
    lib = ctypes.CDLL(L.LIB_PATH)
    i32 = ctypes.c_int32
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported by the library"
        decl = re.sub(r"\s+", " ", re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header).group(1))
        # the map right behind homos, then its grid; the two forwards that plan with plane masks take their scratch behind it
        behind = r"const float \*homos, const uint8_t \*quad_keep, int32_t QH, int32_t QW,"
        assert re.search(behind + (r" void \*cull_scratch," if name in ENTRIES[:2] else r" (?!void \*cull_scratch)"), decl), decl
        argtypes, restype = L.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == decl.count(",") + 1
        k = 5 if name == "vl3d_render_fwd_frames" else 3      # (desc, stack, [frame0, T_alloc,] homos) in front
        assert argtypes[k:k + 3] == [ctypes.c_void_p, i32, i32]
        culled = name + "_culled"
        assert culled not in L.SIGNATURES and not hasattr(lib, culled) and not re.search(r"\b" + culled + r"\b", header), culled


def _desc(planar=True, **fields):
    """D 2, T 3, 8 x 8 texels, 4 x 6 pixels, fp32, sigmoid / sigmoid: the planar convention, or utils_mpi's"""
    from videoloop3d_amd import _lib as L
    d = L.RenderDesc()
    d.D, d.T, d.Hs, d.Ws, d.H, d.W = 2, 3, 8, 8, 4, 6
    d.coord_mode, d.border_mode, d.act_order = (L.COORD["affine"], L.BORDER["hardcut"], L.ACT_ORDER["post"]) if planar else (0, 0, 0)
    d.rgb_act = d.alpha_act = L.ACT["sigmoid"]
    d.pixel_center = 0.5 if planar else 0.0
    d.sx = d.sy = 1.0
    for k, v in fields.items():
        setattr(d, k, v)
    return d


# every pointer a placeholder, a dense model, a run of frames inside its clip, no regulariser gradient
DEFAULTS = dict(stack=P, homos=P, qk=None, QH=0, QW=0, cull=None, rgb=P, alpha=P, asum=None, sums=P, reg_state=P, frame0=1, T_alloc=5,
                g_rgb=P, g_alpha=None, g_reg=None, g_asum=None, g_stack=P, scratch=None, scratch_bytes=0)
OUTPUT = {"vl3d_render_fwd": "rgb", "vl3d_render_fwd_frames": "alpha", "vl3d_render_fwd_reg": "rgb", "vl3d_render_reg_fwd": "sums",
          "vl3d_render_bwd": "g_stack"}


def _call(entry, d, **over):
    from videoloop3d_amd import _lib as L
    a = dict(DEFAULTS, **over)
    qmap = (a["qk"], a["QH"], a["QW"])
    args = {"vl3d_render_fwd": (a["stack"], a["homos"], *qmap, a["cull"], a["rgb"], a["alpha"], a["asum"]),
            "vl3d_render_fwd_frames": (a["stack"], a["frame0"], a["T_alloc"], a["homos"], *qmap, a["cull"], a["rgb"], a["alpha"]),
            "vl3d_render_fwd_reg": (a["stack"], a["homos"], *qmap, a["rgb"], a["alpha"], a["asum"], a["sums"], a["reg_state"]),
            "vl3d_render_reg_fwd": (a["stack"], a["homos"], *qmap, a["sums"], a["reg_state"]),
            "vl3d_render_bwd": (a["stack"], a["homos"], *qmap, a["rgb"], a["alpha"], a["g_rgb"], a["g_alpha"], a["g_reg"], a["reg_state"],
                                a["g_asum"], a["g_stack"], a["scratch"], a["scratch_bytes"])}[entry]
    lib = L.lib()
    return getattr(lib, entry)(d, *args, None), lib.vl3d_last_error()


def _refusals():
    """(id, entry, descriptor fields, planar, call arguments, a fragment of the message)"""
    with_map = dict(qk=P, QH=2, QW=2, cull=P)
    cases = []
    for e in ENTRIES:
        for what in ("stack", "homos", OUTPUT[e]):
            cases.append((f"null-{what}", e, {}, True, {what: None}, b"null pointer"))
        cases.append(("map-under-affine-planes", e, dict(coord_mode=2), True, with_map, b"per-plane texel transforms"))
        cases.append(("grid-of-mixed-signs", e, {}, True, dict(with_map, QW=-2), b"bad quad grid"))
        cases.append(("grid-with-a-zero", e, {}, True, dict(with_map, QH=0), b"bad quad grid"))
        cases.append(("tile-exact-grid-of-ragged-tiles", e, {}, True, dict(with_map, QH=-3, QW=-2), b"whole tiles"))
        cases.append(("stack-window-outside-its-plane", e, dict(cull_row0=4, cull_Hs=8, cull_Ws=8), True, with_map, b"leaves the plane"))
        cases.append(("tile-exact-grid-under-utils-mpi", e, {}, False, dict(with_map, QH=-2, QW=-2), b"tile-exact layout: the planar"))
    for e in ENTRIES[:2]:
        cases.append(("map-without-cull-scratch", e, {}, True, dict(with_map, cull=None), b"vl3d_render_cull_scratch_bytes"))
    for e in ENTRIES[2:4]:
        cases.append(("129-planes", e, dict(D=129), True, {}, b"at most 128 planes"))
    cases.append(("grad-reg-without-reg-state", "vl3d_render_bwd", {}, True, dict(g_reg=P, reg_state=None), b"grad_reg needs the reg_state"))
    cases.append(("run-past-the-clip", "vl3d_render_fwd_frames", {}, True, dict(frame0=3), b"leaves the clip"))      # frames 3 .. 5 of 5
    cases.append(("run-before-the-clip", "vl3d_render_fwd_frames", {}, True, dict(frame0=-1), b"leaves the clip"))
    return [pytest.param(*c[1:], id=f"{c[1][5:]}-{c[0]}") for c in cases]


@no_device
@pytest.mark.parametrize("entry, fields, planar, args, fragment", _refusals())
def test_refusals_name_the_surviving_entry(entry, fields, planar, args, fragment):
    import __graft_entry__ as g
    g.build()
    rc, msg = _call(entry, _desc(planar, **fields), **args)
    assert rc == 1, (rc, msg)                                                   # VL3D_EINVAL
    assert msg.startswith(entry.encode() + b": ") and fragment in msg, msg


@no_device
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_null_map_is_a_dense_call_whatever_the_grid_says(entry):
    """quad_keep NULL with QH = 3, QW = 5 (no grid of 8 x 8 texels under the tile-exact rules, and no scratch): not a grid refusal -- the call
    gets as far as the device, which does not exist here"""
    import __graft_entry__ as g
    g.build()
    for QH, QW in ((3, 5), (-3, -5), (3, -5)):
        rc, msg = _call(entry, _desc(), qk=None, QH=QH, QW=QW, cull=None)
        assert not (rc == 1 and (b"grid" in msg or b"tile" in msg or b"cull" in msg)), (rc, msg)
