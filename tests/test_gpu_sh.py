"""Stage 1's view-dependent colour head on the MI355X (vl3d_render_sh_fwd / _bwd, render.render_planes_sh, MPMesh with rgb_mlp_type = 'rgb_sh',
direct2sh, the driver's direct2sh_epoch) against its float64 statement (tests/sh_statement.py on the oracle's public pieces).

Tolerances are the project's own (TOL = 1e-4 of tests/test_gpu_render.py): outputs <= 1e-4, gradients <= 1e-4 max(1, |g|max).  The backward sums
with float atomics, so gradients are compared within that tolerance, never bitwise.  Every case uses a rotated, off-axis camera, so that all
three components of the ray direction vary over the image."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import sh_statement as SH
from oracle import mpi_oracle as MO
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
MPV_KW = dict(pixel_center=0.5, coord_mode="affine", border="hardcut", act_order="post")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def maxabs(a, b):
    return float((a.detach().double().cpu() - torch.as_tensor(b).detach().double().cpu()).abs().max())


def rot(axis, deg):
    a = np.radians(deg)
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def camera(H, W):
    """a rotated, off-axis view: (E ref -> target [4,4], K [3,3]) float64 -- a wide field of view with the principal point off centre"""
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = rot((0.3, 0.9, 0.2), 21.0), (0.04, -0.02, 0.01)
    K = np.array([[0.8 * W, 0, 0.37 * W], [0, 0.75 * W, 0.61 * H], [0, 0, 1.0]])
    return torch.tensor(E), torch.tensor(K)


def fused_homos(D, Hs, Ws, H, W):
    """the homographies of tests/test_gpu_render.py test_fused_vs_oracle: strong parallax, in-plane rotation / zoom, frame mapped onto the plane"""
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    tar_e = tar_e.clone()
    tar_e[:3, 3] *= 4.0
    depths = make_depths(D, 1.0, 100.0).flip(0)
    homos = compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3), depths[None])[0]
    th = math.radians(3.0)
    Rz = torch.tensor([[math.cos(th) * 1.07, -math.sin(th), 2.0], [math.sin(th), math.cos(th) * 0.93, -1.5], [1e-4, -2e-4, 1.0]])
    S = torch.tensor([[Ws / W, 0, 0], [0, Hs / H, 0], [0, 0, 1.0]])
    return S @ (homos @ Rz)


def ragged_homos(D):
    homos = torch.tensor([[1.0, 0.01, 0.3], [-0.01, 1.0, 0.2], [0, 0, 1.0]]).repeat(D, 1, 1)
    homos[:, 0, 2] += torch.arange(D) * 0.7
    return homos


def texels(D, Hs, Ws, seed=11):
    stack = synth.make_plane_stack(D, 1, Hs, Ws, seed=seed)
    sh = (synth.hash_uniform((D, 1, Hs, Ws, 3, 4), seed=seed + 1) - 0.5) * 2.0
    sh[..., 3] = 0
    return stack, sh


def cotangents(H, W):
    return (synth.hash_uniform((1, H, W, 3), seed=5) - 0.5, synth.hash_uniform((1, H, W), seed=6) - 0.5,
            (synth.hash_uniform((1, H, W, 2), seed=7) - 0.5) * 0.1)


@functools.lru_cache(maxsize=None)
def statement(shape, acts, homos_kind, keep_frac=None, logit_hi=None):
    """the float64 statement of one case, computed once: inputs, outputs and both gradients"""
    D, Hs, Ws, H, W = shape
    stack, sh = texels(D, Hs, Ws)
    if logit_hi is not None:
        stack[..., 3] = synth.hash_uniform((D, 1, Hs, Ws), seed=24) * (logit_hi + 4.0) - 4.0
    homos = fused_homos(D, Hs, Ws, H, W) if homos_kind == "fused" else ragged_homos(D)
    E, K = camera(H, W)
    keep = None
    if keep_frac is not None:
        torch.manual_seed(3)
        keep = torch.rand(D, 4, 6) < keep_frac
    spec = MO.RenderSpec(rgb_act=acts[0], alpha_act=acts[1], **MPV_KW)
    s64, h64 = stack.double().requires_grad_(True), sh.double().requires_grad_(True)
    rgb, alpha, asum, _, _ = SH.render(s64, h64, homos.double(), SH.ray_matrix(E, K), H, W, spec, keep)
    g_rgb, g_a, g_s = cotangents(H, W)
    gs, gh = torch.autograd.grad([rgb, alpha, asum], [s64, h64], [g_rgb.double(), g_a.double(), g_s.double()])
    return types.SimpleNamespace(stack=stack, sh=sh, homos=homos, E=E, K=K, keep=keep, rgb=rgb.detach(), alpha=alpha.detach(), asum=asum.detach(),
                                 g_stack=gs, g_sh=gh)


def run(dev, st, acts, H, W, ray_scale=1.0, keep=None):
    from videoloop3d_amd.render import RenderSpec, render_planes_sh, sh_ray_matrix
    s, h = st.stack.to(dev).requires_grad_(True), st.sh.to(dev).requires_grad_(True)
    ray_m = (sh_ray_matrix(st.E, st.K) * ray_scale).to(dev)
    rgb, alpha, asum = render_planes_sh(s, h, st.homos.to(dev), ray_m, H, W, RenderSpec.mpv(rgb_act=acts[0], alpha_act=acts[1]),
                                        quad_keep=None if keep is None else keep.to(dev), with_alpha_sums=True)
    g_rgb, g_a, g_s = (t.to(dev) for t in cotangents(H, W))
    gs, gh = torch.autograd.grad([rgb, alpha, asum], [s, h], [g_rgb, g_a, g_s])
    return rgb, alpha, asum, gs, gh


def check(st, rgb, alpha, asum, gs, gh):
    assert tuple(rgb.shape) == tuple(st.rgb.shape) and tuple(alpha.shape) == tuple(st.alpha.shape) and tuple(asum.shape) == tuple(st.asum.shape)
    assert maxabs(rgb, st.rgb) <= TOL and maxabs(alpha, st.alpha) <= TOL and maxabs(asum, st.asum) <= TOL * max(1.0, float(st.asum.abs().max()))
    assert maxabs(gs, st.g_stack) <= TOL * max(1.0, float(st.g_stack.abs().max()))
    assert maxabs(gh, st.g_sh) <= TOL * max(1.0, float(st.g_sh.abs().max()))
    assert float(gh[..., 3].abs().max()) == 0.0                                          # the reserved lane: an exact 0
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gh).all())


# ---- 1, 2: forward and both gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acts", [("sigmoid", "sigmoid"), ("none", "sigmoid")])
@pytest.mark.parametrize("shape", [(8, 48, 64, 40, 56), (5, 33, 47, 61, 70), (3, 20, 24, 9, 130)])
def test_forward_and_both_gradients(dev, shape, acts):
    H, W = shape[3:]
    st = statement(shape, acts, "fused")
    rgb, alpha, asum, gs, gh = run(dev, st, acts, H, W)
    check(st, rgb, alpha, asum, gs, gh)
    assert float(st.g_sh.abs().sum()) > 0 and float(gh.abs().sum()) > 0                  # the view-dependent coefficients are reached
    # all three components of the direction vary over the image
    d = SH.ray_dirs(SH.ray_matrix(st.E, st.K), H, W)
    assert all(float(d[..., i].max() - d[..., i].min()) > 0.05 for i in range(3))


@pytest.mark.parametrize("shape", [(1, 4, 6, 3, 5), (2, 9, 70, 1, 66), (3, 17, 129, 16, 125)])
def test_ragged_sizes(dev, shape):
    """a single plane, frames narrower than a wave, a one-pixel row, tile size +- 1"""
    acts = ("sigmoid", "sigmoid")
    st = statement(shape, acts, "ragged")
    check(st, *run(dev, st, acts, *shape[3:]))


@pytest.mark.parametrize("acts", [("relu", "clamp"), ("abs", "none"), ("clamp", "relu")])
def test_other_activation_pairs_forward(dev, acts):
    """the rest of the activation table: forward against the statement (their gradients have kinks: checked where they are smooth, above)"""
    shape = (5, 33, 47, 61, 70)
    st = statement(shape, acts, "fused")
    rgb, alpha, asum, gs, gh = run(dev, st, acts, *shape[3:])
    assert maxabs(rgb, st.rgb) <= TOL * max(1.0, float(st.rgb.abs().max())) and maxabs(alpha, st.alpha) <= TOL * max(1.0, float(st.alpha.abs().max()))
    assert bool(torch.isfinite(gs).all()) and bool(torch.isfinite(gh).all()) and float(gh[..., 3].abs().max()) == 0.0


# ---- 3: against the shipped kernel ------------------------------------------------------------------------------------------------------------------
def test_zero_coefficients_equal_the_shipped_render(dev):
    """stack_sh = 0 and colour lanes r / C0: the picture of render_planes on r -- rgb to the one extra rounding of C0 (r / C0) under a slope
    <= 0.25, alpha and alpha_sums bit for bit (vl3d_render_fwd's), the alpha lane's gradient within the gradient tolerance"""
    import dataclasses
    from videoloop3d_amd.render import RenderSpec, render_planes, render_planes_sh, render_planes_with_regularisers, sh_ray_matrix
    D, Hs, Ws, H, W = 8, 48, 64, 40, 56
    r = synth.make_plane_stack(D, 1, Hs, Ws, seed=11)
    s = r.clone()
    s[..., :3] = r[..., :3] / np.float32(SH.C0)
    homos = fused_homos(D, Hs, Ws, H, W).to(dev)
    E, K = camera(H, W)
    spec = RenderSpec.mpv()
    g_rgb, g_a, _ = (t.to(dev) for t in cotangents(H, W))
    rd = r.to(dev).requires_grad_(True)
    rgb_p, alpha_p = render_planes(rd, homos, H, W, spec)
    (g_p,) = torch.autograd.grad([rgb_p, alpha_p], rd, [g_rgb, g_a])
    # (variant bits 12-15 = 1: the two-pass forward with regularisers, whose alpha_sums are vl3d_render_fwd's)
    _, alpha_q, _, asum_p = render_planes_with_regularisers(rd.detach(), homos, H, W, dataclasses.replace(spec, variant=0x1000))
    sd = s.to(dev).requires_grad_(True)
    zero = torch.zeros((D, 1, Hs, Ws, 3, 4), device=dev, requires_grad=True)
    rgb, alpha, asum = render_planes_sh(sd, zero, homos, sh_ray_matrix(E, K).to(dev), H, W, spec, with_alpha_sums=True)
    g_s, g_z = torch.autograd.grad([rgb, alpha], [sd, zero], [g_rgb, g_a])
    assert maxabs(rgb, rgb_p) <= 1e-5
    assert torch.equal(alpha, alpha_p) and torch.equal(alpha_q, alpha_p) and torch.equal(asum, asum_p)
    assert maxabs(g_s[..., 3], g_p[..., 3]) <= TOL * max(1.0, float(g_p.abs().max()))
    assert maxabs(g_s[..., :3], g_p[..., :3] * SH.C0) <= TOL * max(1.0, float(g_p.abs().max()))
    assert float(g_z[..., :3].abs().sum()) > 0 and float(g_z[..., 3].abs().max()) == 0.0


# ---- 4: normalisation ---------------------------------------------------------------------------------------------------------------------------------
def test_ray_matrix_scale_does_not_matter(dev):
    shape, acts = (5, 33, 47, 61, 70), ("sigmoid", "sigmoid")
    st = statement(shape, acts, "fused")
    a = run(dev, st, acts, *shape[3:])
    b = run(dev, st, acts, *shape[3:], ray_scale=2.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---- 5: tile culling --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_frac", [0.0, 0.3, 1.0])
def test_tile_culling(dev, keep_frac):
    from videoloop3d_amd import tiles
    shape, acts = (5, 60, 90, 50, 75), ("sigmoid", "sigmoid")
    D, Hs, Ws, H, W = shape
    st = statement(shape, acts, "fused", keep_frac=keep_frac)
    rgb, alpha, asum, gs, gh = run(dev, st, acts, H, W, keep=st.keep)
    check(st, rgb, alpha, asum, gs, gh)
    dead = ~tiles.quad_to_texel_mask(st.keep.to(dev), Hs, Ws)                             # texels no kept quad reads
    if bool(dead.any()):
        assert float(gs[:, 0][dead].abs().max()) == 0.0 and float(gh[:, 0][dead].abs().max()) == 0.0
    if keep_frac == 0.0:
        assert float(rgb.abs().max()) == 0.0 and float(alpha.abs().max()) == 0.0
    if keep_frac == 1.0:
        dense = run(dev, st, acts, H, W)
        assert torch.equal(rgb, dense[0]) and torch.equal(alpha, dense[1]) and torch.equal(asum, dense[2])
        # (the backward sums with atomics: within the tolerance, not bitwise)
        assert maxabs(gs, dense[3]) <= TOL * max(1.0, float(st.g_stack.abs().max())) and maxabs(gh, dense[4]) <= TOL * max(1.0, float(st.g_sh.abs().max()))


# ---- 6: near-opaque planes --------------------------------------------------------------------------------------------------------------------------
def test_nearly_opaque_planes_gradient_envelope(dev):
    """alpha logits up to +6 (a = 0.9975: the (S - P) / (1 - a) cancellation amplified 400x), the bound of tests/test_gpu_render.py's test of that name"""
    shape, acts = (12, 70, 90, 64, 80), ("sigmoid", "sigmoid")
    st = statement(shape, acts, "fused", logit_hi=6.0)
    assert float(st.stack[..., 3].max()) > 5.5
    check(st, *run(dev, st, acts, *shape[3:]))


# ---- 7: degenerate cases ------------------------------------------------------------------------------------------------------------------------------
def test_nothing_covered(dev):
    """every plane outside the frame, behind the camera (Z < 0) or at Z = 0: zeros, zero gradients, no NaN"""
    from videoloop3d_amd.render import RenderSpec, render_planes_sh, sh_ray_matrix
    D, Hs, Ws, H, W = 4, 20, 24, 9, 70
    stack, sh = texels(D, Hs, Ws)
    homos = torch.eye(3).repeat(D, 1, 1)
    homos[0, 0, 2] = 1e4                                                               # far outside
    homos[1, 1, 2] = -1e4
    homos[2, 2, 2] = -1.0                                                              # Z = -1: the plane point lies behind the camera
    homos[2, :2, 2] = 5.0
    homos[3, 2] = 0.0                                                                  # Z = 0
    E, K = camera(H, W)
    s, h = stack.to(dev).requires_grad_(True), sh.to(dev).requires_grad_(True)
    rgb, alpha, asum = render_planes_sh(s, h, homos.to(dev), sh_ray_matrix(E, K).to(dev), H, W, RenderSpec.mpv(), with_alpha_sums=True)
    g_rgb, g_a, g_s = (t.to(dev) for t in cotangents(H, W))
    gs, gh = torch.autograd.grad([rgb, alpha, asum], [s, h], [g_rgb, g_a, g_s])
    # (Z < 0 flips the plane point through the origin: (x + 5) / -1 is negative for the whole frame, so the plane is outside as well)
    for t in (rgb, alpha, asum, gs, gh):
        assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0


def test_entry_refusals(dev):
    """what vl3d_render_sh_fwd refuses, before any launch"""
    import dataclasses
    from videoloop3d_amd.render import RenderSpec, render_planes_sh, sh_ray_matrix
    D, Hs, Ws, H, W = 2, 8, 10, 6, 7
    stack, sh = (t.to(dev) for t in texels(D, Hs, Ws))
    homos = ragged_homos(D).to(dev)
    ray_m = sh_ray_matrix(*camera(H, W)).to(dev)
    ok = RenderSpec.mpv()
    render_planes_sh(stack, sh, homos, ray_m, H, W, ok)
    for bad in (dataclasses.replace(ok, uv_noise_seed=7), dataclasses.replace(ok, variant=1), RenderSpec(), dataclasses.replace(ok, act_order="pre"),
                dataclasses.replace(ok, border="zeros")):
        with pytest.raises(RuntimeError, match="vl3d_render_sh_fwd"):
            render_planes_sh(stack, sh, homos, ray_m, H, W, bad)
    with pytest.raises(RuntimeError, match="float32"):
        render_planes_sh(stack.half(), sh, homos, ray_m, H, W, ok)
    with pytest.raises(RuntimeError, match="stack_sh"):
        render_planes_sh(stack, sh[..., :2, :], homos, ray_m, H, W, ok)
    with pytest.raises(RuntimeError, match="tile-exact"):
        render_planes_sh(stack, sh, homos, ray_m, H, W, dataclasses.replace(ok, tile=(4, 5)), quad_keep=torch.ones(D, 2, 2, dtype=torch.bool, device=dev))
    with pytest.raises(RuntimeError, match="misaligned"):
        flat = torch.zeros(stack.numel() + 4, device=dev)
        render_planes_sh(flat[1:1 + stack.numel()].view(stack.shape), sh, homos, ray_m, H, W, ok)
    big = 130
    with pytest.raises(RuntimeError, match="128 planes"):
        render_planes_sh(torch.zeros(big, 1, 2, 2, 4, device=dev), torch.zeros(big, 1, 2, 2, 3, 4, device=dev), torch.eye(3, device=dev).repeat(big, 1, 1),
                         ray_m, 2, 2, ok)


# ---- 8, 9: the module -------------------------------------------------------------------------------------------------------------------------------
def _args(**kw):
    a = dict(mpi_h_scale=1.0, mpi_w_scale=1.0, mpi_d=4, atlas_grid_h=2, rgb_mlp_type="rgb_sh", rgb_activate="sigmoid", alpha_activate="sigmoid",
             bg_color="", learn_loop_mask=True, upsample_stage="", scale_invariant=True, sparsity_loss_weight=0.004, rgb_smooth_loss_weight=0.2,
             a_smooth_loss_weight=0.5, density_loss_weight=0.02, d_smooth_loss_weight=0.0, l_smooth_loss_weight=0.0, optimizer="adam", lrate=0.05,
             lrate_decay=100, N_iters=3, sparsify_epoch=-1, density_loss_epoch=0, patch_h_size=16, patch_w_size=20, patch_h_stride=8,
             patch_w_stride=12, vid2img_mode="average", add_intrin_noise=False, i_weights=1, mpi_h_verts=4, mpi_w_verts=5, add_uv_noise=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


MH, MW = 24, 32
MK = np.array([[0.9 * MW, 0, MW / 2 + 1.5], [0, 0.85 * MW, MH / 2 - 1.0], [0, 0, 1]], np.float64)


def _model(dev, **kw):
    from videoloop3d_amd.MPI import MPMesh
    m = MPMesh(_args(**kw), MH, MW, np.eye(4), MK, 1.0, 100.0).to(dev)
    with torch.no_grad():
        stack, sh = texels(*m.stack.shape[:1], *m.stack.shape[2:4], seed=5)
        m.stack.copy_(stack * 0.7)
        if hasattr(m, "stack_sh"):
            m.stack_sh.copy_(sh)
        if m.learn_loop_mask:
            m.stack_mask.copy_(synth.hash_uniform(tuple(m.stack_mask.shape), seed=6) * 3 - 2)
    return m


def _view():
    """a rotated target camera and a crop of it: (tar_extrin [1,4,4], crop intrinsics [1,3,3], h, w)"""
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = rot((0.2, 0.9, 0.3), 4.0), (0.05, -0.02, 0.01)
    Kc = MK.copy()
    Kc[0, 2] -= 5
    Kc[1, 2] -= 3
    return torch.tensor(E)[None], torch.tensor(Kc)[None], 20, 26


def _statement_of(m, ext, Kc, h, w):
    """the statement on the model's weights for the view (ref_extrin = identity: `ext` is the ref -> target extrinsic)"""
    homos = m.plane_homographies(ext, Kc).double()
    spec = MO.RenderSpec(rgb_act=m.args.rgb_activate, alpha_act=m.args.alpha_activate, scale=m.spec.scale, offset=m.spec.offset, **MPV_KW)
    s64 = m.stack.detach().cpu().double().requires_grad_(True)
    zero = torch.zeros(tuple(s64.shape[:4]) + (3, 4), dtype=torch.float64)
    h64 = (m.stack_sh.detach().cpu().double() if hasattr(m, "stack_sh") else zero).requires_grad_(True)
    rgb, alpha, asum, lay, cov = SH.render(s64, h64, homos, SH.ray_matrix(ext[0], Kc[0]), h, w, spec)
    return s64, h64, rgb, alpha, lay, cov


def test_module_eval_training_extras_gradients_and_label(dev):
    m = _model(dev)
    ext, Kc, h, w = _view()
    s64, h64, rgb_o, alpha_o, lay, cov = _statement_of(m, ext, Kc, h, w)
    m.eval()
    with torch.no_grad():
        rgbl, extra = m(h, w, ext, Kc)
    assert tuple(rgbl.shape) == (1, 4, h, w) and extra == {}
    assert maxabs(rgbl[:, :3].permute(0, 2, 3, 1), rgb_o) <= TOL
    # the label does not depend on colour: the bits of a `direct` model's two-pass label on the same alpha and mask
    d = _model(dev, rgb_mlp_type="direct", loop_mask_two_pass=True).eval()
    with torch.no_grad():
        d.stack[..., 3].copy_(m.stack[..., 3])
        assert torch.equal(d.stack_mask, m.stack_mask)
        rgbl_d, _ = d(h, w, ext, Kc)
    assert torch.equal(rgbl[:, 3], rgbl_d[:, 3]) and float(rgbl[:, 3].abs().max()) > 0
    # training: the regularisers against the reference's formulas on the statement's slot layers, and the gradient at both parameters
    m.train()
    rgbl, extra = m(h, w, ext, Kc)
    want = SH.extras(lay, cov, alpha_o, m.mpi_d)
    assert sorted(extra) == sorted(want)
    for k in want:
        assert abs(float(extra[k]) - float(want[k])) <= TOL * max(1.0, abs(float(want[k]))), k
    G = synth.hash_uniform((1, 3, h, w), seed=21) - 0.5
    wt = {k: getattr(m.args, f"{k}_loss_weight") * 25.0 for k in want}
    total = (rgbl[:, :3] * G.to(dev)).sum() + sum(wt[k] * extra[k].sum() for k in want)
    gs, gh = torch.autograd.grad(total, [m.stack, m.stack_sh])
    total_o = (rgb_o.permute(0, 3, 1, 2) * G.double()).sum() + sum(wt[k] * want[k] for k in want)
    gs_o, gh_o = torch.autograd.grad(total_o, [s64, h64])
    assert maxabs(gs, gs_o) <= TOL * max(1.0, float(gs_o.abs().max())) and maxabs(gh, gh_o) <= TOL * max(1.0, float(gh_o.abs().max()))
    assert float(gh_o.abs().sum()) > 0 and float(gh[..., 3].abs().max()) == 0.0
    # the driver's objective takes its generic spelling for such a model
    tgt = synth.hash_uniform((1, 3, h, w), seed=40, device=dev)
    tm = (synth.hash_uniform((1, h, w), seed=41, device=dev) > 0.5).float()
    loss, img, loop, ex = m.objective(h, w, ext, Kc, tgt, tm)
    assert loss.requires_grad and sorted(ex) == sorted(want) and bool(torch.isfinite(loss))


def test_direct2sh_on_the_device(dev):
    ext, Kc, h, w = _view()
    m = _model(dev, rgb_mlp_type="direct", learn_loop_mask=False).eval()
    with torch.no_grad():
        before, _ = m(h, w, ext, Kc)
    m.direct2sh(keep_picture=True)
    assert m.rgb_mlp_type == "rgb_sh" and m.stack_sh.device == m.stack.device
    with torch.no_grad():
        after, _ = m(h, w, ext, Kc)
    assert maxabs(after, before) <= 1e-5
    # the default is the reference's: the colours read C0 * stack.rgb, and the picture changes at the switch
    m2 = _model(dev, rgb_mlp_type="direct", learn_loop_mask=False).eval()
    m2.direct2sh()
    with torch.no_grad():
        got, _ = m2(h, w, ext, Kc)
    _, _, rgb_o, _, _, _ = _statement_of(m2, ext, Kc, h, w)
    assert maxabs(got.permute(0, 2, 3, 1), rgb_o) <= TOL and maxabs(got, before) > 1e-2
    opt = m2.get_optimizer()
    from videoloop3d_amd import tiles
    assert isinstance(opt, tiles.TileAdam) and sum(len(g["params"]) for g in opt.param_groups) == 2


# ---- 10: the driver ---------------------------------------------------------------------------------------------------------------------------------
def test_driver_switches_at_direct2sh_epoch(dev, tmp_path):
    from videoloop3d_amd import train_3d as drv
    from videoloop3d_amd.MPI import MPMesh
    V = 2
    poses = []
    for v in range(V):
        poses.append(np.concatenate([rot((0.1, 1.0, 0.2), 1.5 * (v + 1)), np.array([[0.03 * (v + 1)], [-0.01], [0.0]])], 1))
    poses = torch.tensor(np.stack(poses), dtype=torch.float32)
    intrins = torch.tensor(MK, dtype=torch.float32)[None].repeat(V, 1, 1)
    vids = [synth.hash_uniform((3, 3, MH, MW), seed=30 + v, device=dev) for v in range(V)]
    args = _args(rgb_mlp_type="direct", direct2sh_epoch=1, N_iters=3)
    model = MPMesh(args, MH, MW, np.eye(4), MK, 1.0, 100.0).to(dev).train()
    with torch.no_grad():
        model.stack.copy_(synth.make_plane_stack(*model.stack.shape[:4], seed=5) * 0.7)
    stack0 = model.stack.detach().clone()
    seen = []
    out = drv.train(model, args, vids, poses, intrins, MH, MW, device=dev, generator=torch.Generator().manual_seed(7), save_dir=str(tmp_path),
                    on_step=lambda e, i, loss, *r: seen.append((e, model.rgb_mlp_type, loss)))
    assert out["epochs"] == 3 and out["iters"] == len(seen) > 0
    assert {t for e, t, _ in seen if e < 1} == {"direct"} and {t for e, t, _ in seen if e >= 1} == {"rgb_sh"}
    assert all(bool(torch.isfinite(l)) for _, _, l in seen)
    # both parameters move, and the reserved lane stays 0
    assert float((model.stack.detach() - stack0).abs().max()) > 1e-3
    assert float(model.stack_sh.detach()[..., :3].abs().max()) > 1e-3 and float(model.stack_sh.detach()[..., 3].abs().max()) == 0.0
    # the checkpoint, loaded into a fresh `direct` model, gives the same forward bit for bit
    ck = torch.load(str(tmp_path / "epoch_0002.tar"), weights_only=False)
    assert ck["network_state_dict"]["self.rgb_mlp_type"] == "rgb_sh"
    fresh = MPMesh(_args(rgb_mlp_type="direct"), MH, MW, np.eye(4), MK, 1.0, 100.0).to(dev)
    fresh.init_from_mpi(ck["network_state_dict"])
    assert fresh.rgb_mlp_type == "rgb_sh"
    ext, Kc, h, w = _view()
    model.eval(), fresh.eval()
    with torch.no_grad():
        a, _ = model(h, w, ext, Kc)
        b, _ = fresh(h, w, ext, Kc)
    assert torch.equal(a, b)
