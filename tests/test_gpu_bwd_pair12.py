"""The frame-pair backward in 64 x 12-pixel regions (render_bwd_pair_k<..., BWD_64X12>, `variant` 7; the default wherever it measured faster) against the
frame-pair backward in 32 x 16-pixel regions (the same kernel's BWD_32X16 instantiation, `variant` 6): per frame the same arithmetic in the same order, so the
gradient has the SAME BITS -- over ragged and exact tile grids, frames smaller than one region, even and odd T, fp32 and fp16 stacks, stacks at
the frame's size and at the 1.07x edge of the pair dispatch, with and without an alpha gradient, in both coordinate conventions."""
import math

import pytest
import torch

from oracle import mpi_oracle as MO
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu

SPECS = {
    "utils_mpi": dict(),
    "mpv": dict(pixel_center=0.5, coord_mode="affine", border="hardcut", act_order="post"),
}
PAIRS_32x16, PAIRS_64x12, ONE_FRAME_64x16 = 6, 7, 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _homos(D, H, W, scale=1.0):
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    tar_e = tar_e.clone()
    tar_e[:3, 3] *= scale
    depths = make_depths(D, 1.0, 100.0).flip(0)
    return compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3), depths[None])[0]


def _plan_feasible():
    from videoloop3d_amd import render
    return int(render.LAST_BWD_SCRATCH.view(torch.int32)[0].item())


# what vl3d_render_bwd_choice reports for a dense call of T >= 2 frames without regularisers inside the pair dispatch (`fits`): (family, width,
# rows) -- variant 0 takes variant 7's kernel there, the other two are kernels of their own
CHOICE = {PAIRS_32x16: ("pair", 32, 16), PAIRS_64x12: ("pair12", 64, 12), 0: ("pair12", 64, 12), ONE_FRAME_64x16: ("tile", 64, 16)}


def _grads(dev, spec_name, H, W, stack_scale, T, dtype, with_alpha, variants, D=5, runs=1):
    """gradient of every variant for one scene: a 2-degree in-plane rotation with a little zoom and perspective (taps off the axes,
    plan feasible), the frame centred on a stack of stack_scale times its size"""
    from videoloop3d_amd.render import RenderSpec, last_bwd_choice, render_planes
    Hs, Ws = int(H * stack_scale), int(W * stack_scale)
    assert Hs * 100 <= H * 107 and Ws * 100 <= W * 107, "outside the pair dispatch (`fits`): the case would not reach the kernels under test"
    kw = SPECS[spec_name]
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=41, device=dev, dtype=dtype).requires_grad_(True)
    th = math.radians(2.0)
    Rz = torch.tensor([[math.cos(th) * 1.01, -math.sin(th), 1.0], [math.sin(th), math.cos(th) * 0.99, 0.5], [2e-5, -3e-5, 1.0]])
    homos = _homos(D, H, W) @ Rz
    if spec_name == "mpv":
        kw = dict(kw, scale=(stack_scale, stack_scale), offset=(-0.5, 0.25))
    else:
        homos = torch.diag(torch.tensor([Ws / W, Hs / H, 1.0])) @ homos
    homos = homos.to(dev)
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5, device=dev) - 0.5
    g_a = synth.hash_uniform((T, H, W), seed=6, device=dev) - 0.5
    out = {}
    for v in variants:
        for run in range(runs):
            rgb, alpha = render_planes(stack, homos, H, W, RenderSpec(variant=v, **kw))
            if with_alpha:
                (gs,) = torch.autograd.grad([rgb, alpha], stack, [g_rgb, g_a])
            else:
                (gs,) = torch.autograd.grad(rgb, stack, g_rgb)
            assert _plan_feasible() == 1
            # the kernel the variant names ran (equal bits from ONE kernel reached twice would prove nothing): no REG / MASK / ADAM / CULL
            assert last_bwd_choice() == CHOICE[v] + (False, False, False, False, dtype == torch.float16)
            out[(v, run)] = gs.clone()
    return out


# frames: ragged in both axes | exact multiples of the 62 x 10 owned pixels | one tile exactly | smaller than one region | one ragged column of tiles
FRAMES = [(150, 260), (40, 124), (10, 62), (7, 40), (93, 70)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("spec_name", ["mpv", "utils_mpi"])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_pair12_gradient_equals_the_32_wide_pairs_bitwise(dev, frame, spec_name, T, dtype):
    H, W = frame
    for stack_scale in (1.0, 1.07):          # the stack at exactly the frame's size | at the edge of `fits` (Hs * 100 <= H * 107)
        for with_alpha in (True, False):
            out = _grads(dev, spec_name, H, W, stack_scale, T, dtype, with_alpha, (PAIRS_32x16, PAIRS_64x12, 0, ONE_FRAME_64x16))
            ref = out[(PAIRS_32x16, 0)]
            assert float(ref.float().abs().max()) > 1e-3
            assert torch.isfinite(ref.float()).all()
            for v in (PAIRS_64x12, 0, ONE_FRAME_64x16):
                assert torch.equal(out[(v, 0)], ref), (v, stack_scale, with_alpha)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_pair12_is_deterministic(dev, dtype):
    """every texel is written once, in a fixed order: two runs give the same bits"""
    out = _grads(dev, "mpv", 150, 260, 1.0, 3, dtype, True, (PAIRS_64x12, 0), runs=2)
    assert torch.equal(out[(PAIRS_64x12, 0)], out[(PAIRS_64x12, 1)])
    assert torch.equal(out[(0, 0)], out[(0, 1)])
    assert torch.equal(out[(0, 0)], out[(PAIRS_64x12, 0)])


def test_pair12_against_the_oracle(dev):
    """... and directly against the CPU oracle (odd T: the tail frame is swept twice and stored once)"""
    from videoloop3d_amd.render import RenderSpec, render_planes
    D, T, H, W = 4, 3, 75, 131
    kw = SPECS["mpv"]
    stack = synth.make_plane_stack(D, T, H, W, seed=13)
    th = math.radians(2.0)
    homos = _homos(D, H, W, scale=1.5) @ torch.tensor([[math.cos(th), -math.sin(th), 2.0], [math.sin(th), math.cos(th), 1.5], [2e-5, -3e-5, 1.0]])
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5) - 0.5
    g_a = synth.hash_uniform((T, H, W), seed=6) - 0.5
    s_cpu = stack.clone().requires_grad_(True)
    rgb_o, alpha_o, _ = MO.render_planes(s_cpu, homos, H, W, MO.RenderSpec(**kw))
    (gs_o,) = torch.autograd.grad([rgb_o, alpha_o], s_cpu, [g_rgb, g_a])
    s_gpu = stack.to(dev).requires_grad_(True)
    rgb, alpha = render_planes(s_gpu, homos.to(dev), H, W, RenderSpec(variant=PAIRS_64x12, **kw))
    (gs,) = torch.autograd.grad([rgb, alpha], s_gpu, [g_rgb.to(dev), g_a.to(dev)])
    assert _plan_feasible() == 1
    from videoloop3d_amd.render import last_bwd_choice
    assert last_bwd_choice()[:3] == CHOICE[PAIRS_64x12]
    assert float((gs.cpu() - gs_o).abs().max()) <= 1e-4 * max(1.0, float(gs_o.abs().max()))


@pytest.mark.parametrize("variant", [0, PAIRS_32x16, PAIRS_64x12])
def test_pair12_infeasible_view_takes_the_atomics_fallback(dev, variant):
    """a view rotated 40 degrees about the optical axis: |J^-1|_inf = cos + sin = 1.41 > 1.4, the on-device plan says infeasible -- both pair
    kernels exit and the atomics kernel gives the result (no host synchronisation either way)"""
    from videoloop3d_amd.render import RenderSpec, render_planes
    D, T, H, W = 3, 2, 90, 140
    kw = SPECS["mpv"]
    stack = synth.make_plane_stack(D, T, H, W, seed=3)
    th = math.radians(40.0)
    c, s = math.cos(th), math.sin(th)
    cx, cy = W / 2.0, H / 2.0
    rot = torch.tensor([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [0.0, 0.0, 1.0]])
    homos = _homos(D, H, W) @ rot
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5) - 0.5
    s_cpu = stack.clone().requires_grad_(True)
    rgb_o, _, _ = MO.render_planes(s_cpu, homos, H, W, MO.RenderSpec(**kw))
    (gs_o,) = torch.autograd.grad(rgb_o, s_cpu, g_rgb)
    s_gpu = stack.to(dev).requires_grad_(True)
    rgb, _ = render_planes(s_gpu, homos.to(dev), H, W, RenderSpec(variant=variant, **kw))
    (gs,) = torch.autograd.grad(rgb, s_gpu, g_rgb.to(dev))
    assert _plan_feasible() == 0
    assert float(gs_o.abs().max()) > 1e-3
    assert float((gs.cpu() - gs_o).abs().max()) <= 1e-4 * max(1.0, float(gs_o.abs().max()))
