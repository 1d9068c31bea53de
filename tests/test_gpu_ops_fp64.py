"""The unfused drop-ins on the device -- utils_mpi.warp_homography, overcompose and overcomposeNto0 (csrc/vl3d_ops.hip), through the wrappers
callers use -- against tests/ops_statement.py: the reference's chain in fp64, the element-wise compositing bounds derived there
(2^-23 (D + C + 4) times the sum of the absolute terms, floor 2^-120) and the warp bound B = 4 max |oracle in fp32 - oracle in fp64| without a
floor.  Every bound and measured maximum is printed before it is asserted.  The refusals go through the C ABI on real buffers pre-filled
with a sentinel: a status, and nothing written."""
import pytest
import torch

import ops_statement as OS

pytestmark = pytest.mark.gpu

RAY_NAMES = sorted(OS.RAYS)
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


# ---- overcompose -----------------------------------------------------------------------------------------------------------------------------------------
def _overcompose(dev, case):
    """the wrapper on alpha [2,3,43,D], content [2,3,43,D,C] -> dict of COMP_OUTPUTS in canonical order, on the host"""
    from videoloop3d_amd.utils_mpi import overcompose
    P, D, C = case.dims
    a = case.a.reshape(OS.P_OVER + (D,)).to(dev).requires_grad_(True)
    c = case.c.reshape(OS.P_OVER + (D, C)).to(dev).requires_grad_(True)
    rgb, bw = overcompose(a, c)
    assert rgb.shape == OS.P_OVER + (C,) and bw.shape == a.shape and rgb.dtype == bw.dtype == torch.float32
    g_rgb = case.g_rgb.reshape(OS.P_OVER + (C,)).to(dev)
    if case.g_bw is None:
        ga, gc = torch.autograd.grad([rgb], [a, c], [g_rgb])
    else:
        ga, gc = torch.autograd.grad([rgb, bw], [a, c], [g_rgb, case.g_bw.reshape(a.shape).to(dev)])
    return dict(rgb=rgb.detach().cpu().reshape(P, C), bw=bw.detach().cpu().reshape(P, D), g_alpha=ga.cpu().reshape(P, D), g_content=gc.cpu().reshape(P, D, C))


@pytest.mark.parametrize("name", RAY_NAMES)
def test_overcompose_forward(dev, name):
    for C in (1, 3, 8):
        case, ref, bnd = OS.comp_statement(name, OS.P_OVER, C, True)
        OS.check(f"overcompose {name} D {case.dims[1]} C {C}", _overcompose(dev, case), ref, bnd, ("rgb", "bw"))


@pytest.mark.parametrize("name", RAY_NAMES)
def test_overcompose_gradient(dev, name):
    for C in (1, 3, 8):
        for with_bw in (True, False):
            case, ref, bnd = OS.comp_statement(name, OS.P_OVER, C, with_bw)
            OS.check(f"overcompose {name} D {case.dims[1]} C {C} g_bw {with_bw}", _overcompose(dev, case), ref, bnd, ("g_alpha", "g_content"))


@pytest.mark.parametrize("name", RAY_NAMES)
def test_overcompose_backward_null_g_bw(dev, name):
    """vl3d_overcompose_bwd with grad_bw = NULL (autograd materialises a zero tensor, so the wrapper never sends one)"""
    from videoloop3d_amd import _lib as L
    case, ref, bnd = OS.comp_statement(name, OS.P_OVER, 3, False)
    P, D, C = case.dims
    a, c, g = case.a.to(dev), case.c.to(dev), case.g_rgb.to(dev)
    ga, gc = torch.full_like(a, SENTINEL), torch.full_like(c, SENTINEL)
    L.check(L.lib().vl3d_overcompose_bwd(P, D, C, L.ptr(a), L.ptr(c), L.ptr(g), None, L.ptr(ga), L.ptr(gc), L.stream_ptr(dev)), "vl3d_overcompose_bwd")
    OS.check(f"vl3d_overcompose_bwd {name} D {D} C {C} grad_bw NULL", dict(g_alpha=ga.cpu(), g_content=gc.cpu()), ref, bnd, ("g_alpha", "g_content"))


# ---- overcomposeNto0 -------------------------------------------------------------------------------------------------------------------------------------
def _nto0(dev, case, blend, permuted):
    """the wrapper on mpi [2,D,4,7,37] (permuted: a non-contiguous view of a [2,7,37,D,4] tensor) -> (got, reference in fp64, bounds), in
    overcomposeNto0's layout: rgb, trans, g_alpha, g_content (and g_colour: mpi's colour channels under blend_content)"""
    from videoloop3d_amd.utils_mpi import overcomposeNto0
    mpi, bc, g_rgb = OS.nto0_inputs(case, blend=blend)
    ref = OS.reference_nto0(mpi, bc, g_rgb)
    b = OS.bounds(case)
    if permuted:
        leaf = mpi.permute(0, 3, 4, 1, 2).contiguous().to(dev).requires_grad_(True)
        m = leaf.permute(0, 3, 4, 1, 2)
        assert not m.is_contiguous() and m.shape == mpi.shape
    else:
        leaf = m = mpi.to(dev).requires_grad_(True)
    bcd = None if bc is None else bc.to(dev).requires_grad_(True)
    rgb, trans = overcomposeNto0(m, ret_mask=True, blend_content=bcd)
    assert rgb.shape == g_rgb.shape and trans.shape == mpi[:, :, 3].shape and not trans.requires_grad
    rgb_only = overcomposeNto0(m, blend_content=bcd)
    assert torch.equal(rgb_only, rgb)
    grads = torch.autograd.grad([rgb], [leaf] + ([bcd] if blend else []), [g_rgb.to(dev)])
    gm = grads[0].cpu()
    gm = gm.permute(0, 3, 4, 1, 2) if permuted else gm
    got = dict(rgb=rgb.detach().cpu(), trans=trans.cpu(), g_alpha=gm[:, :, 3], g_content=grads[1].cpu() if blend else gm[:, :, :3])
    want = dict(rgb=ref["rgb"], trans=ref["trans"], g_alpha=ref["g_mpi"][:, :, 3], g_content=ref["g_blend"] if blend else ref["g_mpi"][:, :, :3])
    bnd = dict(rgb=OS.rgb_to_nto0(b["rgb"]), trans=OS.to_nto0(b["trans"]), g_alpha=OS.to_nto0(b["g_alpha"]), g_content=OS.to_nto0(b["g_content"]))
    if blend:      # mpi's colour channels are not read: their gradient is exactly zero
        assert float(gm[:, :, :3].abs().max()) == 0.0
    return got, want, bnd


NTO0_VARIANTS = ((3, False, False), (1, True, False), (4, True, True), (8, True, False), (3, False, True))      # C, blend_content, permuted view


@pytest.mark.parametrize("name", RAY_NAMES)
def test_nto0_forward(dev, name):
    for C, blend, permuted in NTO0_VARIANTS:
        case = OS.comp_case(name, OS.P_NTO0, C, with_bw=False)
        got, want, bnd = _nto0(dev, case, blend, permuted)
        OS.check(f"overcomposeNto0 {name} D {case.dims[1]} C {C} blend_content {blend} permuted {permuted}", got, want, bnd, ("rgb", "trans"))


@pytest.mark.parametrize("name", RAY_NAMES)
def test_nto0_gradient(dev, name):
    for C, blend, permuted in NTO0_VARIANTS:
        case = OS.comp_case(name, OS.P_NTO0, C, with_bw=False)
        got, want, bnd = _nto0(dev, case, blend, permuted)
        OS.check(f"overcomposeNto0 {name} D {case.dims[1]} C {C} blend_content {blend} permuted {permuted}", got, want, bnd, ("g_alpha", "g_content"))


@pytest.mark.parametrize("name", ["uniform1_x32", "opaque_mid", "single_plane"])
def test_nto0_blendweight_short_circuit(dev, name):
    """a caller-supplied blendweight replaces the scan, as in the reference: rgb = sum_k content_k alpha_k blendweight_k.  D multiply-multiply-add
    terms: 2^-23 (D + C + 4) sum_k |content_k alpha_k blendweight_k| + 2^-120 holds for any order of the sum"""
    from videoloop3d_amd.utils_mpi import overcomposeNto0
    for C, blend in ((3, False), (4, True)):
        case = OS.comp_case(name, OS.P_NTO0, C, with_bw=False)
        P, D, _ = case.dims
        mpi, bc, _ = OS.nto0_inputs(case, blend=blend)
        given = OS.synth.hash_uniform(tuple(mpi[:, :, 3].shape), seed=91)
        want, same = OS.MO.overcomposeNto0(mpi.double(), blendweight=given.double(), ret_mask=True, blend_content=None if bc is None else bc.double())
        content = (mpi[:, :, :3] if bc is None else bc).double()
        bound = OS.EPS * (D + C + 4) * (content * (mpi[:, :, 3] * given).double().unsqueeze(2)).abs().sum(1) + OS.FLOOR
        gd = given.to(dev)
        rgb, back = overcomposeNto0(mpi.to(dev), blendweight=gd, ret_mask=True, blend_content=None if bc is None else bc.to(dev))
        assert back is gd and torch.equal(same, given.double())
        OS.check(f"overcomposeNto0 {name} D {D} C {C} blendweight given", dict(rgb=rgb.cpu()), dict(rgb=want), dict(rgb=bound), ("rgb",))
        assert torch.equal(overcomposeNto0(mpi.to(dev), blendweight=gd, blend_content=None if bc is None else bc.to(dev)), rgb)


# ---- warp_homography -------------------------------------------------------------------------------------------------------------------------------------
def _warp(dev, case, gout=None):
    from videoloop3d_amd.utils_mpi import warp_homography
    g = case.dims
    im = case.images.to(dev).requires_grad_(True)
    out = warp_homography(g["h"], g["w"], case.homos.to(dev), im)
    assert out.shape == case.gout.shape and out.dtype == torch.float32
    (gi,) = torch.autograd.grad([out], [im], [(case.gout if gout is None else gout).to(dev)])
    return out.detach().cpu(), gi.cpu()


@pytest.mark.parametrize("name", OS.WARP_ALL)
def test_warp(dev, name):
    st = OS.warp_statement(name)
    g = st.case.dims
    assert float(st.case.excluded.double().mean()) <= OS.EXCLUDED_CAP
    out, gi = _warp(dev, st.case)
    st.check(f"B x D = {g['B']} x {g['D']}, C = {g['C']}, {g['Hs']} x {g['Ws']} -> {g['h']} x {g['w']}", out, gi)
    if name == "shifted":      # whole rows and columns outside the texture: exactly 0, and they reach no texel
        lines = OS.outside_lines(st.case)
        assert int(lines.sum()) > 0 and float(out[lines.expand_as(out)].abs().max()) == 0.0
        _, gl = _warp(dev, st.case, gout=lines.expand_as(out).float())
        assert float(gl.abs().max()) == 0.0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse(dev):
    from videoloop3d_amd.utils_mpi import overcompose, overcomposeNto0, warp_homography
    a = torch.rand(2, 3, 5, 4, device=dev)
    with pytest.raises(RuntimeError, match="C <= 8"):
        overcompose(a, torch.rand(2, 3, 5, 4, 9, device=dev))
    for shape in ((2, 3, 5, 5, 3), (2, 3, 4, 4, 3), (3, 5, 4, 3)):
        with pytest.raises(RuntimeError, match="does not match"):
            overcompose(a, torch.rand(shape, device=dev))
    mpi = torch.rand(2, 4, 4, 3, 5, device=dev)
    with pytest.raises(RuntimeError, match="bad dims"):
        overcomposeNto0(mpi, blend_content=torch.rand(2, 4, 9, 3, 5, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        overcompose(a.cpu(), torch.rand(2, 3, 5, 4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        overcomposeNto0(mpi.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        warp_homography(4, 4, torch.eye(3).expand(1, 1, 3, 3), torch.rand(1, 1, 3, 4, 4))


def _abi_calls(dev):
    """entry point -> (argument list of a valid small call, indices of its dimensions, of its pointers that must not be NULL, every buffer, the
    index of the dimension limited to 65535 or None, the index of C or None).  The buffers are large enough for every mutation below (C = 9
    included), so a refusal that failed to refuse would still write inside them."""
    from videoloop3d_amd import _lib as L
    N, C, Hs, Ws, h, w = 2, 3, 5, 6, 4, 7
    P, D, HW, B = 70, 4, 35, 2
    big = lambda n: torch.full((n,), SENTINEL, device=dev)      # noqa: E731
    src = lambda n: torch.rand(n, device=dev)      # noqa: E731
    s = L.stream_ptr(dev)
    homos = torch.eye(3, device=dev).reshape(1, 9).repeat(N, 1).contiguous()
    t = dict(homos=homos, images=src(N * 9 * Hs * Ws), out=big(N * 9 * h * w), gout=src(N * 9 * h * w), gimg=big(N * 9 * Hs * Ws),
             alpha=src(P * D), content=src(P * D * 9), rgb=big(P * 9), bw=big(P * D), g_rgb=src(P * 9), g_bw=src(P * D), g_alpha=big(P * D),
             g_content=big(P * D * 9))
    p = {k: L.ptr(v) for k, v in t.items()}
    a_sb, a_sd, c_sb, c_sd, c_sc = D * HW, HW, D * 9 * HW, 9 * HW, HW      # B * HW = P: the same buffers
    calls = {
        "vl3d_warp_fwd": ([N, C, Hs, Ws, h, w, p["homos"], p["images"], p["out"], s], range(6), (6, 7, 8), 0, 1),
        "vl3d_warp_bwd": ([N, C, Hs, Ws, h, w, p["homos"], p["gout"], p["gimg"], s], range(6), (6, 7, 8), 0, 1),
        "vl3d_overcompose_fwd": ([P, D, C, p["alpha"], p["content"], p["rgb"], p["bw"], s], range(3), (3, 4, 5, 6), None, 2),
        "vl3d_overcompose_bwd": ([P, D, C, p["alpha"], p["content"], p["g_rgb"], p["g_bw"], p["g_alpha"], p["g_content"], s], range(3), (3, 4, 5, 7, 8), None, 2),
        "vl3d_overcompose_nto0_fwd": ([B, D, C, HW, p["alpha"], a_sb, a_sd, p["content"], c_sb, c_sd, c_sc, p["rgb"], p["bw"], s], range(4), (4, 7, 11), 0, 2),
        "vl3d_overcompose_nto0_bwd": ([B, D, C, HW, p["alpha"], a_sb, a_sd, p["content"], c_sb, c_sd, c_sc, p["g_rgb"], p["g_alpha"], p["g_content"], s],
                                      range(4), (4, 7, 11, 12, 13), 0, 2),
    }
    return calls, t


def test_abi_refusals_write_nothing(dev):
    """null pointers, non-positive dimensions, C = 9 for the compositing entries and N (B) > 65535: each is a status with a message, and no
    buffer changes.  The valid call of every entry point does write (so the sentinel would show it)."""
    from videoloop3d_amd import _lib as L
    calls, t = _abi_calls(dev)
    before = {k: v.clone() for k, v in t.items()}
    unchanged = lambda: all(torch.equal(before[k], t[k]) for k in t)      # noqa: E731
    n = 0
    for name, (args, dims, ptrs, limited, c_at) in calls.items():
        fn = getattr(L.lib(), name)
        bad = [(i, None) for i in ptrs] + [(i, v) for i in dims for v in (0, -1)]
        if limited is not None:
            bad.append((limited, 65536))
        if name.startswith("vl3d_overcompose"):
            bad.append((c_at, 9))
        for i, v in bad:
            mutated = list(args)
            mutated[i] = v
            rc = fn(*mutated)
            torch.cuda.synchronize()
            assert rc != 0 and L.lib().vl3d_last_error(), (name, i, v, rc)
            assert unchanged(), (name, i, v)
            n += 1
    print(f"{n} refusals over {len(calls)} entry points: a status each, every buffer untouched")
    for name, (args, *_rest) in calls.items():
        assert getattr(L.lib(), name)(*args) == 0, (name, L.lib().vl3d_last_error())
        torch.cuda.synchronize()
        assert not unchanged(), name
        for k in t:
            t[k].copy_(before[k])
