"""The 64 x 12 frame-pair backward WITHOUT the owner table (render_bwd_pair_k<..., BWD_64X12, OWNERLESS>, `variant` 8) against the two frame-pair kernels that read
the table (the same kernel without OWNERLESS in 64 x 12 regions, `variant` 7, and in 32 x 16 regions, `variant` 6).  The gather computes every texel's owner
pixel with the function the table pass uses, on the same inputs, so the partition of the texels -- and with it every bit of the gradient -- is
the table kernels': one tile / a ragged grid / a frame smaller than a region, even and odd T, fp32 and fp16 stacks, stacks at the frame's
size and at the 1.07x edge of the pair dispatch (windows wider and taller than the region: the strip and extra-row passes), a near-unit view
(3 x 3 gather with the ballot skip) and a magnifying one (every tile sets the "apart" bit: 2 x 2 gather), with and without an alpha gradient,
in both coordinate conventions.  Then: every texel is written exactly once, the table region of the scratch is never touched, and an
infeasible plan still leaves for the atomics kernel."""
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
PAIRS_32x16, PAIRS_64x12, OWNERLESS = 6, 7, 8
CHOICE = {PAIRS_32x16: ("pair", 32, 16), PAIRS_64x12: ("pair12", 64, 12), OWNERLESS: ("pair12", 64, 12), 0: ("pair12", 64, 12)}
# in-plane rotation (degrees), zoom, on top of the benchmark cameras' own 0.5-degree turn about y (J within 0.5 % of 1 across the frame).  At unit
# zoom the 2x2 test of the window pass stays undecided (J00 - |J01| <= 1.002 * 1.005 - 0.0087 = 0.998 < 1.001: the 3x3 gather, whose ballot skips
# the pixels no texel of the wave reaches); at zoom 1.10 pixels are at least 1.10 * 0.993 - 0.01 = 1.08 texels apart under the planar convention
# (the utils_mpi one scales by (Ws - 1) / Ws, (Hs - 1) / Hs: 0.86 for the 7-row frame -- no promise there)
VIEWS = {"half_degree": (0.5, 1.0), "apart": (0.5, 1.10)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _homos(D, H, W):
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    depths = make_depths(D, 1.0, 100.0).flip(0)
    return compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3), depths[None])[0]


def _scratch_words():
    from videoloop3d_amd import render
    return render.LAST_BWD_SCRATCH.view(torch.int32)


def _window_sizes(D, H, W):
    """the size words of the (62 x 10-pixel tile, plane) window records the last backward wrote (bwd_windows_k: width | height << 16, bit 30 =
    "pixels at least a texel apart")"""
    tiles = -(-W // 62) * -(-H // 10)
    off = (16 + 12 * D + 3) & ~3
    return _scratch_words()[off:off + tiles * D * 4].view(tiles * D, 4)[:, 2].cpu()


def _scene(dev, spec_name, H, W, stack_scale, T, dtype, view, D, shift=(0.0, 0.0)):
    """stack, homographies, output gradients and RenderSpec arguments: the frame centred on a stack of stack_scale times its size, seen under
    `view` with a little perspective (taps off the axes, plan feasible); shift: the frame's image moved by that many plane units"""
    Hs, Ws = int(H * stack_scale), int(W * stack_scale)
    assert Hs * 100 <= H * 107 and Ws * 100 <= W * 107, "outside the pair dispatch (`fits`): the case would not reach the kernels under test"
    kw = SPECS[spec_name]
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=41, device=dev, dtype=dtype)
    th, zoom = math.radians(VIEWS[view][0]), VIEWS[view][1]
    Rz = torch.tensor([[math.cos(th) * zoom * 1.002, -math.sin(th) * zoom, 1.0], [math.sin(th) * zoom, math.cos(th) * zoom * 0.998, 0.5],
                       [2e-5, -3e-5, 1.0]])
    homos = torch.tensor([[1.0, 0.0, shift[0]], [0.0, 1.0, shift[1]], [0.0, 0.0, 1.0]]) @ _homos(D, H, W) @ Rz
    if spec_name == "mpv":
        kw = dict(kw, scale=(stack_scale, stack_scale), offset=(-0.5, 0.25))
    else:
        homos = torch.diag(torch.tensor([Ws / W, Hs / H, 1.0])) @ homos
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5, device=dev) - 0.5
    g_a = synth.hash_uniform((T, H, W), seed=6, device=dev) - 0.5
    return stack, homos.to(dev), g_rgb, g_a, kw


def _grads(dev, spec_name, H, W, stack_scale, T, dtype, with_alpha, view, variants, D, runs=1):
    from videoloop3d_amd.render import RenderSpec, last_bwd_choice, render_planes
    stack, homos, g_rgb, g_a, kw = _scene(dev, spec_name, H, W, stack_scale, T, dtype, view, D)
    stack.requires_grad_(True)
    out = {}
    for v in variants:
        for run in range(runs):
            rgb, alpha = render_planes(stack, homos, H, W, RenderSpec(variant=v, **kw))
            if with_alpha:
                (gs,) = torch.autograd.grad([rgb, alpha], stack, [g_rgb, g_a])
            else:
                (gs,) = torch.autograd.grad(rgb, stack, g_rgb)
            assert int(_scratch_words()[0].item()) == 1      # the plan word: the owner-computes path ran
            assert last_bwd_choice() == CHOICE[v] + (False, False, False, False, dtype == torch.float16)
            out[(v, run)] = gs.clone()
    # the view is what its name says: at the stack's own size no tile of the near-unit view may take the 2x2 gather, every non-empty
    # one of the magnifying view must (variants 7 / 8 / 0 ran last: 62 x 10-pixel tiles)
    if variants[-1] != PAIRS_32x16:
        z = _window_sizes(D, H, W)
        z = z[(z & 0xffff) != 0]
        assert len(z) > 0
        if view == "apart" and spec_name == "mpv":
            assert bool(((z >> 30) & 1).all())
        elif view == "half_degree" and stack_scale == 1.0:
            assert not bool(((z >> 30) & 1).any())
        # windows beyond the 64 x 12 threads -- the strip and the extra-row passes run: a 62-pixel tile row at 1.07 texels per pixel is 66
        # texels + margins wide, a 10-pixel tile column at 1.07 x 1.10 is 11.8 + margins tall (stacks tall enough to hold it)
        if stack_scale > 1.0 and W >= 62:
            assert int((z & 0xffff).max()) > 64
        if stack_scale > 1.0 and view == "apart" and H >= 23 and spec_name == "mpv":
            assert int(((z >> 16) & 0x3fff).max()) > 12
    return out


# frames: one tile exactly | ragged 3 x 2 tile grid | smaller than a region | ragged 4 x 3 grid
FRAMES = [(10, 62), (23, 70), (7, 29), (33, 131)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("spec_name", ["mpv", "utils_mpi"])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
def test_ownerless_gradient_equals_the_table_kernels_bitwise(dev, frame, spec_name, T, dtype):
    H, W = frame
    D = 3 + FRAMES.index(frame) % 3
    for stack_scale in (1.0, 1.07):          # the stack at exactly the frame's size | at the edge of `fits` (Hs * 100 <= H * 107)
        for view in VIEWS:
            for with_alpha in (True, False):
                out = _grads(dev, spec_name, H, W, stack_scale, T, dtype, with_alpha, view, (PAIRS_32x16, PAIRS_64x12, OWNERLESS), D)
                got = out[(OWNERLESS, 0)]
                assert float(got.float().abs().max()) > 1e-3
                assert torch.isfinite(got.float()).all()
                for v in (PAIRS_64x12, PAIRS_32x16):
                    assert torch.equal(got, out[(v, 0)]), (v, stack_scale, view, with_alpha)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_ownerless_is_deterministic_and_the_default_path_equals_it(dev, dtype):
    """every texel is written once, in a fixed order: two runs give the same bits; variant 0 gives variant 8's"""
    out = _grads(dev, "mpv", 33, 131, 1.0, 3, dtype, True, "half_degree", (OWNERLESS, 0), 4, runs=2)
    assert torch.equal(out[(OWNERLESS, 0)], out[(OWNERLESS, 1)])
    assert torch.equal(out[(0, 0)], out[(OWNERLESS, 0)])
    out = _grads(dev, "utils_mpi", 23, 70, 1.07, 2, dtype, False, "apart", (OWNERLESS, 0), 3)
    assert torch.equal(out[(0, 0)], out[(OWNERLESS, 0)])


def _direct(dev, stack, homos, H, W, kw, variant, g_rgb, g_a):
    """one forward and one vl3d_render_bwd through the C ABI with caller-owned buffers: the gradient pre-filled with NaN, the scratch with the
    byte 0xA5 -> (gradient, scratch bytes as a uint8 tensor)"""
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd.render import RenderSpec, _desc
    T = stack.shape[1]
    desc = _desc(stack, H, W, RenderSpec(variant=variant, **kw), 0, 0)
    rgb = torch.empty((T, H, W, 3), dtype=torch.float32, device=dev)
    alpha = torch.empty((T, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        s = L.stream_ptr(dev)
        L.check(L.lib().vl3d_render_fwd(desc, L.ptr(stack), L.ptr(homos), None, 0, 0, None, L.ptr(rgb), L.ptr(alpha), None, s), "vl3d_render_fwd")
        n = int(L.lib().vl3d_render_bwd_scratch_bytes(desc))
        scratch = torch.full((n,), 0xA5, dtype=torch.uint8, device=dev)
        g_stack = torch.full(stack.shape, float("nan"), dtype=stack.dtype, device=dev)
        L.check(L.lib().vl3d_render_bwd(desc, L.ptr(stack), L.ptr(homos), None, 0, 0, L.ptr(rgb), L.ptr(alpha), L.ptr(g_rgb), L.ptr(g_a), None, None,
                                        None, L.ptr(g_stack), L.ptr(scratch), n, s), "vl3d_render_bwd")
    torch.cuda.synchronize()
    return g_stack, scratch


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_every_texel_is_written_exactly_once(dev, dtype):
    """the frame's image moved 20 texels right and 8 down on the stack: the texels left of / above it are in no tile's window (a window
    reaches 1.6 pixels past the frame), the pre-pass zero-fills them, and they are exactly 0; nothing of the NaN the gradient held survives;
    everything equals the table kernel's gradient"""
    D, T, H, W = 4, 3, 33, 131
    stack, homos, g_rgb, g_a, kw = _scene(dev, "mpv", H, W, 1.0, T, dtype, "half_degree", D, shift=(20.0, 8.0))
    got, _ = _direct(dev, stack, homos, H, W, kw, OWNERLESS, g_rgb, g_a)
    ref, _ = _direct(dev, stack, homos, H, W, kw, PAIRS_64x12, g_rgb, g_a)
    assert not torch.isnan(got.float()).any()
    assert float(got.float().abs().max()) > 1e-3
    # the nearest plane's parallax takes 4.5 texels (x) / 1 texel (y) of the shift back, 0.5 degrees over 131 columns / 33 rows move the
    # image's edge by at most 1.2 / 0.3 texels: 20 - 4.5 - 1.2 - 1.6 > 12, 8 - 1 - 0.3 - 1.6 > 5
    assert bool((got[:, :, :, :12] == 0).all()) and bool((got[:, :, :5] == 0).all())
    assert float(got[:, :, 12:, 24:].float().abs().max()) > 1e-3
    assert torch.equal(got, ref)


def test_the_owner_table_is_not_touched(dev):
    """caller-owned scratch full of 0xA5: after variant 8 the table region -- from the 256-byte aligned end of the window records to the end
    -- still holds 0xA5 everywhere, after variant 7 it does not; the header and the window records are written by both"""
    D, T, H, W = 3, 2, 23, 70
    stack, homos, g_rgb, g_a, kw = _scene(dev, "mpv", H, W, 1.0, T, torch.float32, "half_degree", D)
    table_bytes = (D * H * W + 16 * W + 64) * 2      # one uint16 per (plane, texel) + the prefetch padding (vl3d_render_bwd_scratch_bytes)
    win_off = ((16 + 12 * D + 3) & ~3) * 4
    win_bytes = -(-W // 62) * -(-H // 10) * D * 16
    grads = {}
    for v in (OWNERLESS, PAIRS_64x12):
        grads[v], scratch = _direct(dev, stack, homos, H, W, kw, v, g_rgb, g_a)
        table_off = scratch.numel() - table_bytes
        assert table_off % 256 == 0 and table_off >= win_off + win_bytes
        table = scratch[table_off:]
        if v == OWNERLESS:
            assert bool((table == 0xA5).all())
        else:
            assert int((table[:D * H * W * 2] != 0xA5).sum()) >= D * H * W      # every entry written (an entry's two bytes are never both 0xA5 by chance alone)
        words = scratch[:win_off + win_bytes].view(torch.int32)
        assert int(words[0].item()) == 1 and bool((words[1:16] == 0).all())      # the header: feasible, the rest cleared
        recs = words[win_off // 4:].view(-1, 4)
        assert bool((recs != -1515870811).all())      # (0xA5A5A5A5: no corner, size word or reciprocal width is that)
        assert bool(((recs[:, 2] & 0xffff) > 0).any())
    assert torch.equal(grads[OWNERLESS], grads[PAIRS_64x12])


@pytest.mark.parametrize("spec_name,dtype,table_free", [("mpv", torch.float32, True), ("mpv", torch.float16, False), ("utils_mpi", torch.float32, False),
                                                        ("utils_mpi", torch.float16, False)], ids=["mpv-f32", "mpv-f16", "utils_mpi-f32", "utils_mpi-f16"])
def test_which_kernel_the_default_runs(dev, spec_name, dtype, table_free):
    """the exported choice reads (pair12, 64, 12) for both 64 x 12 kernels, so the default (variant 0) is told apart by what it leaves in a
    scratch full of 0xA5: the table region untouched for fp32 stacks of the planar convention (the OWNERLESS kernel), every entry written
    for fp16 stacks and for the utils_mpi convention (the table kernel) -- csrc/vl3d_render_bwd_choice.h, BWD_PAIR12_AUTO_OWNERLESS_*"""
    D, T, H, W = 3, 2, 23, 70
    stack, homos, g_rgb, g_a, kw = _scene(dev, spec_name, H, W, 1.0, T, dtype, "half_degree", D)
    table_bytes = (D * H * W + 16 * W + 64) * 2
    got, scratch = _direct(dev, stack, homos, H, W, kw, 0, g_rgb, g_a)
    assert int(scratch[:4].view(torch.int32)[0].item()) == 1      # the owner-computes path ran
    table = scratch[scratch.numel() - table_bytes:]
    if table_free:
        assert bool((table == 0xA5).all())
    else:
        assert int((table[:D * H * W * 2] != 0xA5).sum()) >= D * H * W
    ref, _ = _direct(dev, stack, homos, H, W, kw, PAIRS_64x12, g_rgb, g_a)
    assert float(got.float().abs().max()) > 1e-3 and torch.equal(got, ref)


def test_ownerless_infeasible_view_takes_the_atomics_fallback(dev):
    """a view rotated 40 degrees about the optical axis: |J^-1|_inf = cos + sin = 1.41 > 1.4, the on-device plan says infeasible -- the
    kernel and its pre-pass exit and the atomics kernel gives the result (tolerance: tests/test_gpu_bwd_pair12.py's for the same fallback)"""
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
    rgb, _ = render_planes(s_gpu, homos.to(dev), H, W, RenderSpec(variant=OWNERLESS, **kw))
    (gs,) = torch.autograd.grad(rgb, s_gpu, g_rgb.to(dev))
    assert int(_scratch_words()[0].item()) == 0
    assert float(gs_o.abs().max()) > 1e-3
    assert float((gs.cpu() - gs_o).abs().max()) <= 1e-4 * max(1.0, float(gs_o.abs().max()))
