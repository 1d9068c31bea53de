"""Training under the bake rule on the MI355X (include/vl3d.h VL3D_ACT_BAKED; csrc/vl3d_render_c6_mpv_baked.hip): act_order="baked" renders the
picture the viewer package shows -- every tap activated, truncated to the byte vl3d_bake_rgba8 writes, decoded, then blended -- with the
activate-first gradient, the rounding straight-through.

  1  the picture is the shipped one: render_planes / render_frame_run under the rule against the baked render of bake_texels(stack)
  2  forward and gradient against the statement (tests/bake_rule_statement.py) with the DEVICE's bytes
  3  tile culling, shared-border and tile-exact
  4  the kernel families agree bit for bit under the new order
  5  fp16 stacks            6  the layer regularisers            7  what keeps refusing
  8  MPMeshVid.playback_rule_            9  evaluate_views(baked=...)

Bounds: 1e-5 on every pixel against the baked render (the bound tests/test_gpu_baked.py holds float-on-decoded against baked to), TOL = 1e-4 on
outputs and TOL * max(1, |g|max) on the stack gradient against the statement (tests/test_gpu_render.py)."""
import dataclasses
import math
import types

import numpy as np
import pytest
import torch

import baked_models as BM
import bake_rule_statement as ST
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-4
MPV_BAKED = dict(pixel_center=0.5, coord_mode="affine", border="hardcut", act_order="baked")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def maxabs(a, b):
    return float((a.detach().double().cpu() - torch.as_tensor(b).detach().double().cpu()).abs().max())


def _tile_ran():
    from videoloop3d_amd import render
    return int(render.LAST_BWD_SCRATCH[:1].view(torch.int32).item())


def bench_homos(D, H, W, near=1.0, far=100.0, scale=1.0):
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    tar_e = tar_e.clone()
    tar_e[:3, 3] *= scale
    depths = make_depths(D, near, far).flip(0)
    return compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3), depths[None])[0]


def device_bytes(stack, dev):
    """the bytes the bake kernel writes for `stack` (the rule the render shares, csrc/vl3d_bake_rule.h), on the host"""
    from videoloop3d_amd.baked import bake_texels
    return bake_texels(stack.to(dev), "sigmoid", "sigmoid").cpu()


# ---- 1. the picture is the shipped one ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixed(dev):
    """the fixed scenes of tests/baked_models.py as LOGITS: D = 4, 5 frames, 40 x 72 texels, 37 x 70 view, three cameras, the quad map of
    tests/test_gpu_baked.py; with the two ends of the rule (bytes 0 and 255) in view.  Computed once, never modified."""
    import baked_statement as BS
    from videoloop3d_amd.baked import bake_texels
    stack = synth.make_plane_stack(BM.D, BM.T_ALLOC, BM.HS, BM.WS, seed=7, device=dev, alpha_bias=-0.5)
    stack[0, :, 8:16, 8:24] = -30.0
    stack[1, :, 16:24, 30:50] = 30.0
    keep = synth.hash_uniform((BM.D, BM.QH, BM.QW), seed=11) < 0.5
    keep[2] = False
    baked = bake_texels(stack, "sigmoid", "sigmoid")
    assert int((baked == 0).sum()) > 0 and int((baked == 255).sum()) > 0
    return types.SimpleNamespace(stack=stack, baked=baked, keep=keep.to(torch.uint8).to(dev), homos=BS.cameras(BM.D, BM.H, BM.W).to(dev))


@pytest.mark.parametrize("run", [(1, 3), (3, 1), (1, 2)], ids=["run of 3", "run of 1", "run of 2"])
@pytest.mark.parametrize("layout", ["dense", "shared", "exact"])
def test_the_picture_is_the_shipped_one(dev, fixed, layout, run):
    from videoloop3d_amd.render import render_frame_run, render_frame_run_baked, render_planes
    f0, n = run
    spec_b = BM.specs()[layout]                                                  # what the baked render reads: geometry only
    spec = dataclasses.replace(spec_b, rgb_act="sigmoid", alpha_act="sigmoid", act_order="baked")
    qk = None if layout == "dense" else fixed.keep
    worst = 0.0
    for cam in range(3):
        rgb_s, alpha_s = render_frame_run_baked(fixed.baked, f0, n, fixed.homos[cam], BM.H, BM.W, spec_b, quad_keep=qk)
        rgb, alpha = render_planes(fixed.stack[:, f0:f0 + n].contiguous(), fixed.homos[cam], BM.H, BM.W, spec, quad_keep=qk)
        e = max(maxabs(rgb, rgb_s), maxabs(alpha, alpha_s))
        worst = max(worst, e)
        assert e <= 1e-5, (cam, e)
        # the frames read in place (vl3d_render_fwd_frames): the same kernels, the same bits
        rgb_r, alpha_r = render_frame_run(fixed.stack, f0, n, fixed.homos[cam], BM.H, BM.W, spec, quad_keep=qk)
        assert torch.equal(rgb_r, rgb) and torch.equal(alpha_r, alpha)
        assert float(alpha.max()) > 0.3
    # ... and not the float one
    rgb_p, _ = render_planes(fixed.stack[:, f0:f0 + n].contiguous(), fixed.homos[0], BM.H, BM.W, dataclasses.replace(spec, act_order="post"), quad_keep=qk)
    rgb_0, _ = render_planes(fixed.stack[:, f0:f0 + n].contiguous(), fixed.homos[0], BM.H, BM.W, spec, quad_keep=qk)
    print(f"{layout} run {run}: max |baked order - baked render| {worst:.3g}, max |baked order - post| {maxabs(rgb_0, rgb_p):.3g}")
    assert maxabs(rgb_0, rgb_p) > 1e-3


# ---- 2. forward and gradient against the statement ---------------------------------------------------------------------------------------
def _against_statement(dev, stack, homos, H, W, kw=None, keep=None, tile=(0, 0), variant=0):
    """render_planes under the rule against the statement with the device's bytes: outputs <= TOL, stack gradient <= TOL * max(1, |g|max)
    -> (rgb, alpha, gs) of the device, gs_o of the statement"""
    from videoloop3d_amd.render import RenderSpec, render_planes
    kw = dict(MPV_BAKED, **(kw or {}))
    T = stack.shape[1]
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5) - 0.5
    g_a = synth.hash_uniform((T, H, W), seed=6) - 0.5
    s_cpu = stack.clone().requires_grad_(True)
    rgb_o, alpha_o, _ = ST.render(s_cpu, device_bytes(stack, dev), homos, H, W, kw.get("scale", (1.0, 1.0)), kw.get("offset", (0.0, 0.0)), tile, keep)
    (gs_o,) = torch.autograd.grad([rgb_o, alpha_o], s_cpu, [g_rgb, g_a])
    s_gpu = stack.to(dev).requires_grad_(True)
    spec = dataclasses.replace(RenderSpec(variant=variant, **kw), tile=tuple(tile))
    rgb, alpha = render_planes(s_gpu, homos.to(dev), H, W, spec, quad_keep=None if keep is None else keep.to(dev))
    (gs,) = torch.autograd.grad([rgb, alpha], s_gpu, [g_rgb.to(dev), g_a.to(dev)])
    e = (maxabs(rgb, rgb_o), maxabs(alpha, alpha_o), maxabs(gs, gs_o), float(gs_o.abs().max()))
    print(f"baked vs statement: rgb {e[0]:.3g} alpha {e[1]:.3g} grad {e[2]:.3g} (|g|max {e[3]:.3g})")
    assert e[0] <= TOL and e[1] <= TOL
    assert e[2] <= TOL * max(1.0, e[3])
    assert float(gs.abs().sum()) > 0 and torch.isfinite(gs).all()
    return rgb, alpha, gs, gs_o, (g_rgb, g_a, s_gpu, spec)


@pytest.mark.parametrize("shape", [(8, 2, 48, 64, 40, 56), (5, 1, 33, 47, 61, 70), (3, 3, 20, 24, 9, 130)])
def test_forward_and_gradient_against_the_statement(dev, shape):
    """the three shapes of test_fused_vs_oracle with its rotated homographies and hash cotangents"""
    D, T, Hs, Ws, H, W = shape
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=11)
    homos = bench_homos(D, H, W, scale=4.0)
    th = math.radians(3.0)
    Rz = torch.tensor([[math.cos(th) * 1.07, -math.sin(th), 2.0], [math.sin(th), math.cos(th) * 0.93, -1.5], [1e-4, -2e-4, 1.0]])
    homos = torch.tensor([[Ws / W, 0, 0], [0, Hs / H, 0], [0, 0, 1.0]]) @ (homos @ Rz)
    _against_statement(dev, stack, homos, H, W)


# ---- 3. tile culling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep_frac", [0.3, 1.0])
def test_tile_culling_shared_borders(dev, keep_frac):
    """the scene of test_tile_culling_matches_oracle: culled texels get exactly 0 gradient, a map that keeps everything is the dense call"""
    from videoloop3d_amd import tiles
    from videoloop3d_amd.render import render_planes
    D, T, Hs, Ws, H, W = 7, 2, 150, 200, 139, 187
    QH, QW = 6, 9
    torch.manual_seed(3)
    keep = torch.rand(D, QH, QW) < keep_frac
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=13)
    th = math.radians(2.0)
    Rz = torch.tensor([[math.cos(th) * 1.05, -math.sin(th), 3.0], [math.sin(th), math.cos(th) * 0.96, 2.5], [2e-5, -3e-5, 1.0]])
    homos = bench_homos(D, H, W, scale=1.5) @ Rz
    rgb, alpha, gs, _, (g_rgb, g_a, s_gpu, spec) = _against_statement(dev, stack, homos, H, W, keep=keep)
    assert _tile_ran() == 1
    dead = ~tiles.quad_to_texel_mask(keep.to(dev), Hs, Ws)
    assert float(gs[dead[:, None].expand(D, T, Hs, Ws)].abs().max() if dead.any() else 0.0) == 0.0
    if keep_frac == 1.0:
        rgb_p, alpha_p = render_planes(s_gpu, homos.to(dev), H, W, spec)
        (gs_p,) = torch.autograd.grad([rgb_p, alpha_p], s_gpu, [g_rgb.to(dev), g_a.to(dev)])
        assert torch.equal(rgb, rgb_p) and torch.equal(alpha, alpha_p) and torch.equal(gs, gs_p)


def test_tile_culling_tile_exact(dev):
    """a scene built as tests/test_gpu_tile_exact.py builds its own (independent tiles of 14 x 13 texels, 9 x 13 quads, 35 % kept)"""
    from test_gpu_tile_exact import scene as tile_exact_scene
    from videoloop3d_amd import tiles
    D, T, th, tw, QH, QW = 6, 3, 14, 13, 9, 13
    H, W = int(QH * (th - 1) / 1.15), int(QW * (tw - 1) / 1.15)
    homos, scale, keep = tile_exact_scene(D, H, W, QH, QW, th, tw, keep_frac=0.35)
    Hs, Ws = QH * th, QW * tw
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=19)
    _, alpha, gs, _, _ = _against_statement(dev, stack, homos, H, W, kw=dict(scale=scale), keep=keep, tile=(th, tw))
    assert _tile_ran() == 1 and float(alpha.max()) > 0.3
    dead = ~tiles.quad_to_texel_mask(keep, Hs, Ws, (th, tw))
    assert dead.any() and float(gs.cpu()[dead[:, None].expand(D, T, Hs, Ws)].abs().max()) == 0.0


# ---- 4. the kernel families agree bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_fwd_frame_pair_kernel_equals_single_frame_kernel_bitwise(dev, T, dtype):
    from videoloop3d_amd.render import RenderSpec, render_planes_with_regularisers
    D, Hs, Ws, H, W = 5, 70, 150, 61, 139
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=31, device=dev, dtype=dtype)
    homos = bench_homos(D, H, W, scale=2.0).to(dev)
    outs = []
    for variant in (0, 0x600):
        rgb, alpha, sums, asum = render_planes_with_regularisers(stack, homos, H, W, RenderSpec(variant=variant, **MPV_BAKED))
        outs.append((rgb, alpha, asum))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert float(outs[0][0].abs().max()) > 0.01


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("stack_scale", [1.0, 1.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_bwd_frame_pair_kernels_equal_tile_kernel_bitwise(dev, stack_scale, T, dtype):
    """variant 0: the frame pairs as the choice takes them (64 x 12 regions where the stack fits, else the tile kernel), 6: pairs in 32 x 16
    regions, 7: pairs in 64 x 12 regions, 3: one frame per thread in 64 x 16 regions -- the same gradient bits"""
    from videoloop3d_amd import render as R
    from videoloop3d_amd.render import RenderSpec, render_planes
    D, H, W = 5, 150, 260
    Hs, Ws = int(H * stack_scale) - 5, int(W * stack_scale) - 9
    kw = dict(MPV_BAKED, scale=(stack_scale, stack_scale), offset=(-1.5, -2.5))
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=41, device=dev, dtype=dtype).requires_grad_(True)
    homos = bench_homos(D, H, W).to(dev)
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5, device=dev) - 0.5
    g_a = synth.hash_uniform((T, H, W), seed=6, device=dev) - 0.5
    out, fam = {}, {}
    for variant in (0, 3, 6, 7):
        rgb, alpha = render_planes(stack, homos, H, W, RenderSpec(variant=variant, **kw))
        (gs,) = torch.autograd.grad([rgb, alpha], stack, [g_rgb, g_a])
        assert _tile_ran() == 1
        out[variant], fam[variant] = gs, R.last_bwd_choice()[:3]
    # the choice describes the new order's calls as every other (vl3d_render_bwd_choice)
    assert fam[3] == ("tile", 64, 16)
    if stack_scale == 1.0:
        assert fam[0] == ("pair12", 64, 12) and fam[6] == ("pair", 32, 16) and fam[7] == ("pair12", 64, 12)
    assert all(torch.equal(out[v], out[3]) for v in (0, 6, 7))
    assert float(out[0].float().abs().max()) > 1e-3


@pytest.mark.parametrize("stack_scale", [1.0, 1.1])
def test_bwd_2x2_gather_equals_3x3_gather_bitwise(dev, stack_scale):
    from videoloop3d_amd.render import RenderSpec, render_planes
    D, T, H, W = 6, 2, 300, 500
    Hs, Ws = int(H * stack_scale) - 7, int(W * stack_scale) - 11
    kw = dict(MPV_BAKED, scale=(stack_scale, stack_scale), offset=(-2.0, -3.0))
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=21, device=dev).requires_grad_(True)
    homos = bench_homos(D, H, W).to(dev)
    g = synth.hash_uniform((T, H, W, 3), seed=5, device=dev) - 0.5
    out = {}
    for variant in (0, 4):
        rgb, _ = render_planes(stack, homos, H, W, RenderSpec(variant=variant, **kw))
        (gs,) = torch.autograd.grad(rgb, stack, g)
        assert _tile_ran() == 1
        out[variant] = gs
    assert torch.equal(out[0], out[4])
    assert float(out[0].abs().max()) > 1e-3


# ---- 5. fp16 stacks --------------------------------------------------------------------------------------------------------------------
def test_fp16_plane_stack(dev):
    """pattern and bounds of tests/test_gpu_render.py: test_fp16_plane_stack; the statement takes the device bytes of the fp16 texels"""
    from videoloop3d_amd.baked import bake_texels
    from videoloop3d_amd.render import RenderSpec, render_planes, render_planes_with_smoothness
    D, T, Hs, Ws, H, W = 6, 2, 100, 140, 93, 131
    stack16 = synth.make_plane_stack(D, T, Hs, Ws, seed=21).half()
    homos = bench_homos(D, H, W, scale=1.5)
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5) - 0.5
    u8 = bake_texels(stack16.to(dev), "sigmoid", "sigmoid").cpu()
    s_cpu = stack16.float().requires_grad_(True)
    rgb_o, alpha_o, _ = ST.render(s_cpu, u8, homos, H, W)
    (gs_o,) = torch.autograd.grad(rgb_o, s_cpu, g_rgb)
    s_gpu = stack16.to(dev).requires_grad_(True)
    rgb, alpha = render_planes(s_gpu, homos.to(dev), H, W, RenderSpec(**MPV_BAKED))
    (gs,) = torch.autograd.grad(rgb, s_gpu, g_rgb.to(dev))
    assert _tile_ran() == 1 and gs.dtype == torch.float16
    print(f"fp16 baked: rgb {maxabs(rgb, rgb_o):.3g} alpha {maxabs(alpha, alpha_o):.3g} grad {maxabs(gs.float(), gs_o):.3g} (|g|max {float(gs_o.abs().max()):.3g})")
    assert maxabs(rgb, rgb_o) <= TOL and maxabs(alpha, alpha_o) <= TOL
    assert maxabs(gs.float(), gs_o) <= 1e-3 * max(1e-3, float(gs_o.abs().max())) + 1e-6      # fp16 rounding of the returned gradient
    rgb_a, _ = render_planes(s_gpu, homos.to(dev), H, W, RenderSpec(variant=1, **MPV_BAKED))
    (gs_a,) = torch.autograd.grad(rgb_a, s_gpu, g_rgb.to(dev))
    assert _tile_ran() == 0 and gs_a.dtype == torch.float16
    assert maxabs(gs_a.float(), gs_o) <= 4e-3 * max(1e-3, float(gs_o.abs().max())) + 1e-5
    # bit-identical to the fp32 kernels on the same (rounded) values, including the fused regulariser sums
    s32 = stack16.float().to(dev).requires_grad_(True)
    rgb32, _, sums32 = render_planes_with_smoothness(s32, homos.to(dev), H, W, RenderSpec(**MPV_BAKED))
    rgb16, _, sums16 = render_planes_with_smoothness(s_gpu, homos.to(dev), H, W, RenderSpec(**MPV_BAKED))
    assert torch.equal(rgb16, rgb32) and torch.equal(sums16, sums32)


# ---- 6. the layer regularisers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("feasible", [True, False])
def test_fused_smoothness_regularisers(dev, feasible):
    """pattern and bounds of tests/test_gpu_render.py: test_fused_smoothness_regularisers, on the statement's layers"""
    from videoloop3d_amd.render import RenderSpec, render_planes_with_smoothness
    D, T, Hs, Ws, H, W = 5, 2, 90, 130, 83, 121
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=17) * 0.5
    if feasible:
        th = math.radians(1.5)
        Rz = torch.tensor([[math.cos(th) * 1.03, -math.sin(th), 3.0], [math.sin(th), math.cos(th) * 0.98, 2.0], [1e-5, -2e-5, 1.0]])
        homos = bench_homos(D, H, W, scale=1.5) @ Rz
    else:
        homos = torch.tensor([[0.5, 0, 10.0], [0, 0.5, 8.0], [0, 0, 1.0]]) @ bench_homos(D, H, W, scale=1.0)
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5) - 0.5
    coef = torch.tensor([0.7, -0.4, 1.3, 0.9])
    s_cpu = stack.clone().requires_grad_(True)
    rgb_o, alpha_o, _, L = ST.render(s_cpu, device_bytes(stack, dev), homos, H, W, return_layers=True)      # L: T,H,W,K,4
    sums_o = torch.stack([(L[:, :, :-1, :, :3] - L[:, :, 1:, :, :3]).abs().sum(), (L[:, :-1, :, :, :3] - L[:, 1:, :, :, :3]).abs().sum(),
                          (L[:, :, :-1, :, 3] - L[:, :, 1:, :, 3]).abs().sum(), (L[:, :-1, :, :, 3] - L[:, 1:, :, :, 3]).abs().sum()])
    loss_o = (rgb_o * g_rgb).sum() + (sums_o * coef).sum() * 1e-3
    (gs_o,) = torch.autograd.grad(loss_o, s_cpu)
    s_gpu = stack.to(dev).requires_grad_(True)
    rgb, alpha, sums = render_planes_with_smoothness(s_gpu, homos.to(dev), H, W, RenderSpec(**MPV_BAKED))
    loss = (rgb * g_rgb.to(dev)).sum() + (sums * coef.to(dev)).sum() * 1e-3
    (gs,) = torch.autograd.grad(loss, s_gpu)
    assert _tile_ran() == (1 if feasible else 0)
    diff = (gs.cpu() - gs_o).abs()
    scale = float(gs_o.abs().max())
    print(f"baked regularisers: sums {maxabs(sums, sums_o) / float(sums_o.abs().max()):.3g} rel, rgb {maxabs(rgb, rgb_o):.3g}, "
          f"grad max {float(diff.max()):.3g} of {scale:.3g}, share above 1e-4 {float((diff > 1e-4 * max(1.0, scale)).float().mean()):.3g}")
    assert maxabs(sums, sums_o) <= 2e-5 * float(sums_o.abs().max())
    assert maxabs(rgb, rgb_o) <= TOL
    assert float((diff > 1e-4 * max(1.0, scale)).float().mean()) <= 1e-4
    assert float(diff.max()) <= 5e-3 * max(1.0, scale)


# ---- 7. what keeps refusing --------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from videoloop3d_amd import render as R
    from videoloop3d_amd.render import RenderSpec, render_planes
    D, T, Hs, Ws, H, W = 3, 2, 24, 40, 20, 36
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=3, device=dev).requires_grad_(True)
    homos = bench_homos(D, H, W).to(dev)
    # another activation pair, another geometry: VL3D_EUNSUPPORTED (code 3) with a message that names what is built
    for spec in (RenderSpec(rgb_act="none", **MPV_BAKED), RenderSpec(act_order="baked"), RenderSpec(border="hardcut", act_order="baked")):
        with pytest.raises(RuntimeError, match=r"code 3.*built is \(affine, hardcut, baked\) with sigmoid / sigmoid"):
            render_planes(stack, homos, H, W, spec)
        with pytest.raises(RuntimeError, match=r"code 3.*built is \(affine, hardcut, baked\)"):
            R.bwd_choice(R._desc(stack, H, W, spec, 0, 0))
    spec = RenderSpec(**MPV_BAKED)
    # the loop-mask channel: the wrapper's sentence, and the entry's own (unchanged) check behind it
    mask = torch.zeros((D, T, Hs, Ws), device=dev)
    assert not R.mask_channel_supported(stack, spec)
    with pytest.raises(RuntimeError, match="loop-mask channel is not built for the bake rule"):
        R.render_planes_with_mask(stack, mask, homos, H, W, spec)
    with pytest.raises(RuntimeError, match=r"code 3.*loop-mask channel is built for"):
        R._RenderPlanesMask.apply(stack, mask, homos, H, W, spec, False)
    # the plane-rows band
    rows = torch.zeros(D, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="bake rule"):
        R.render_plane_rows(stack.detach(), homos, rows, H, W, Hs, spec)
    # the packed render
    from videoloop3d_amd.tiles import CULLED_ALPHA
    model, Hm, Wm, K = BM.pool_model(dev, "")
    model.pack_()
    hm = model.plane_homographies(torch.eye(4)[None], torch.tensor(K)[None].float()).to(dev)
    with pytest.raises(RuntimeError, match="bake rule"):
        R.render_planes_packed(model.packed, model.stack_pool.data, [0], hm, Hm, Wm, dataclasses.replace(model.spec, act_order="baked"), model.quad_keep,
                               CULLED_ALPHA)
    with pytest.raises(RuntimeError, match="packed"):
        model.playback_rule_()


CFG = dict(loss_name=["gpnn_lm"], loss_gain=torch.tensor([1.0]), macro_block=torch.tensor([65]), patch_size=torch.tensor([3]), stride=torch.tensor([2]),
           patcht_size=torch.tensor([3]), stridet=torch.tensor([1]), alpha=torch.tensor([10000.0]), dist_fn=["mse"], rou=["-2"], scaling=torch.tensor([0.1]))


def _view(K):
    tar = np.eye(4, dtype=np.float32)
    tar[:3, 3] = [0.03, 0.01, 0.0]
    return torch.tensor(tar)[None], torch.tensor(K.astype(np.float32))[None]


# ---- 8. the module -----------------------------------------------------------------------------------------------------------------------
def test_module_playback_rule(dev, monkeypatch):
    """a small tile-culled MPMeshVid (tests/baked_models.py: pool_model, tile-exact): eval frames are bake(model)'s, the training gradient at
    module.stack is render_planes' autograd under the same spec, and one optimiser step (two kernels: the fused backward + Adam step stands
    aside, fused_steps stays 0) moves dynamic texels and leaves culled ones alone."""
    import warnings
    from videoloop3d_amd import MPV, tiles
    from videoloop3d_amd.baked import bake
    model, Hm, Wm, K = BM.pool_model(dev, "")
    assert model.playback_rule_() is model and model.spec.act_order == "baked"
    tar_e, tar_k = _view(K)
    model.eval()
    shipped = bake(model)
    for ts in (torch.arange(model.frm_num), torch.tensor([1, 2, 3])):      # the whole clip (render_planes), a run read in place (render_frame_run)
        with torch.no_grad():
            frames, extra = model(Hm, Wm, tar_e, tar_k, ts=ts)
            want, _ = shipped.render(Hm, Wm, tar_e, tar_k, ts)
        assert extra == {} and frames.shape == want.shape == (len(ts), 3, Hm, Wm)
        print(f"module eval under the rule vs bake(model).render, {len(ts)} frames: {maxabs(frames, want):.3g}")
        assert maxabs(frames, want) <= 1e-5 and float(frames.std()) > 0.01
    # training: the gradient the module leaves at module.stack against render_planes called by hand with what the module passed and received
    model.train()
    seen = {}
    real = MPV.render_planes

    def spy(stack, homos, H, W, spec, **kw):
        rgb, alpha = real(stack, homos, H, W, spec, **kw)
        seen.update(homos=homos.detach().clone(), spec=spec, kw=kw, HW=(H, W))
        rgb.register_hook(lambda g: seen.__setitem__("g_rgb", g.detach().clone()))
        return rgb, alpha
    monkeypatch.setattr(MPV, "render_planes", spy)
    h, w = 24, 40
    res = synth.hash_uniform((1, 2 * model.frm_num + 1, 3, h, w), seed=8, device=dev)
    _, ex = model(h, w, tar_e, tar_k, res=res, losscfg=dict(CFG))
    ex["swd"].sum().backward()
    monkeypatch.setattr(MPV, "render_planes", real)
    assert seen["spec"].act_order == "baked" and seen["kw"]["quad_keep"] is not None and seen["HW"] == (h, w)
    leaf = model.stack.detach().clone().requires_grad_(True)
    rgb, _ = real(leaf, seen["homos"], h, w, seen["spec"], quad_keep=model.quad_keep)
    (g_hand,) = torch.autograd.grad(rgb, leaf, seen["g_rgb"])
    keep_t = tiles.quad_to_texel_mask(model.quad_keep, *model.stack.shape[2:4], model.tile_own)[:, None, :, :, None].expand_as(model.stack)
    g_mod = torch.where(keep_t, model.stack.grad, torch.zeros_like(model.stack.grad))      # (static texels: the tie hook sums the frames into frame 0)
    assert float(g_hand.abs().sum()) > 0
    dyn_t = tiles.quad_to_texel_mask(model.quad_dyn, *model.stack.shape[2:4], model.tile_own)[:, None, :, :, None].expand_as(model.stack)
    assert maxabs(g_mod[dyn_t], g_hand[dyn_t]) <= TOL * max(1.0, float(g_hand.abs().max()))
    # one optimiser step under the rule
    model.zero_grad(set_to_none=True)
    before = model.stack.detach().clone()
    opt = model.get_optimizer(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        opt.zero_grad(set_to_none=True)
        _, ex = model(h, w, tar_e, tar_k, res=res, losscfg=dict(CFG))
        assert opt.pending is not None and not opt.fuses(opt.pending[1], model.spec)
        ex["swd"].sum().backward()
        opt.step()
    assert getattr(opt, "fused_backward", False) and opt.fused_steps == 0
    after = model.state_dict()["stack"]      # (flushes the deferred updates)
    assert not torch.equal(after[dyn_t], before[dyn_t])
    assert torch.equal(after[~keep_t], before[~keep_t])


# ---- 9. scoring the playback model -----------------------------------------------------------------------------------------------------------
def _culled_model(dev, T):
    """tests/baked_models.py: pool_model (tile-exact) with a clip of T frames"""
    from videoloop3d_amd import tiles
    from videoloop3d_amd.MPV import MPMeshVid
    model, Hm, Wm, K = BM.pool_model(torch.device("cpu"), "")
    args = types.SimpleNamespace(**dict(vars(model.args), mpv_frm_num=T))
    qh, qw, th, tw = 4, 6, 8, 8
    big = MPMeshVid(args, Hm, Wm, np.eye(4), K, 1.0, 100.0)
    stack = synth.make_plane_stack(model.mpi_d, T, qh * th, qw * tw, seed=5, alpha_bias=0.0) * 0.8
    keep, dyn = model.quad_keep.cpu(), model.quad_dyn.cpu()
    stack = torch.where(tiles.quad_to_texel_mask(dyn, qh * th, qw * tw, (th, tw))[:, None, :, :, None], stack, stack[:, :1])
    stack = torch.where(tiles.quad_to_texel_mask(keep, qh * th, qw * tw, (th, tw))[:, None, :, :, None], stack, torch.tensor([0.0, 0.0, 0.0, tiles.CULLED_ALPHA]))
    big.init_from_mpi({"ref_extrin": big.ref_extrin, "ref_intrin": big.ref_intrin, "planedepth": big.planedepth, "stack": stack, "quad_keep": keep,
                       "quad_dyn": dyn, "self.is_sparse": True, "self.has_dyn": True, "self.tile_own": (th, tw), "self.tile_full": (th, tw)})
    return big.to(dev).eval(), K


@pytest.mark.parametrize("kind", ["BakedMPV", "BakedPool"])
def test_evaluate_views_scores_the_playback_model(dev, kind):
    """evaluate_views(..., baked=b) == view_image_metrics / nn_metrics by hand on b.render_display of the same cameras, as Python floats.
    2 views, frames of 56 x 72, crop 4 -- and a clip of 8 frames: the first patch configuration of the evaluation (5, 2, 7, 1) takes temporal
    patches of 7 frames, which a clip of 6 does not hold (vl3d_patchnn refuses it: "input smaller than one patch")."""
    from videoloop3d_amd import evaluations as E
    from videoloop3d_amd.baked import bake, bake_pool
    T, H, W, crop = 8, 56, 72, 4
    model, K = _culled_model(dev, T)
    b = bake(model) if kind == "BakedMPV" else bake_pool(model)
    assert type(b).__name__ == kind
    ext = np.tile(np.eye(4, dtype=np.float32)[None], (2, 1, 1))
    ext[1, :3, 3] = [0.03, 0.01, 0.0]
    Ks = np.tile(K.astype(np.float32)[None], (2, 1, 1))
    Ks[:, 0, 2] += (W - 64) / 2
    Ks[:, 1, 2] += (H - 36) / 2
    own = [b.render_display(H, W, torch.tensor(np.repeat(ext[v:v + 1], T, 0)), torch.tensor(np.repeat(Ks[v:v + 1], T, 0)), np.arange(T), channels=3)
           for v in range(2)]
    gts = []
    for v in range(2):
        noise = (synth.hash_uniform((T + 1, H, W, 3), 40 + v, device=dev) * 11).long() - 5
        gts.append((torch.cat([own[v], own[v][:1]]).long() + noise).clamp(0, 255).to(torch.uint8).cpu().numpy())
        assert float(own[v].float().std()) > 1.0
    res = E.evaluate_views(model, gts, ext, Ks, crop=crop, baked=b)
    plain = E.evaluate_views(model, gts, ext, Ks, crop=crop)
    c = slice(crop, -crop)
    for v, r in enumerate(res):
        gt = torch.as_tensor(gts[v]).to(dev)
        m = E.loop_static_mask(gt)
        psnr, ssim, dyn = E.view_image_metrics(gt[:, c, c], own[v][:, c, c], m[c, c])
        assert (r["psnr"], r["ssim"], r["dyn"]) == (psnr, ssim, dyn)
        comp, coh, loop = E.nn_metrics(gt[:, c, c].permute(3, 0, 1, 2)[None].float(), own[v][:, c, c].permute(3, 0, 1, 2)[None].float())
        for tag, vals in (("nnf", comp), ("nnb", coh), ("loop", loop)):
            assert [r[f"{tag}_{E._config_tag(cf)}"] for cf in E.EVAL_PATCH_CONFIGS] == vals
        assert r["psnr"] != plain[v]["psnr"]      # the float model's frames are another picture
