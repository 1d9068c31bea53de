"""The row-pair forward (render_fwd2r_k: two pixel rows per thread that share their middle tap row; the default of dense fp32 stacks with the
shipped activations and T >= 2) against the two kernels it must equal BIT FOR BIT: the frame pairs (forward variant 7) and the one-frame,
one-pixel kernel (forward variant 6).  rgb, alpha and the sparsity sums `asum` are compared through the C ABI's plain forward, which is where
the kernel is dispatched (a T = 1 call takes the one-frame kernel under every variant: those cases pin that this stays so).

Tripwire: a lane whose lower pixel's base tap is not exactly one texel row below the upper pixel's fetches its own two upper taps in a branch
of its own.  `own_lanes` restates make_taps' rule on the host (base tap = floor of the texel coordinate clamped to [0, S - 2]; rows 2k and
2k + 1 of the rendered window pair up) and every case asserts that SOME pairs take that branch and SOME do not -- neither path can pass by
never running.  A frame of one row has no pair at all: there the count of pairs is asserted to be 0 instead."""
import math

import pytest
import torch

from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu

MPV = dict(pixel_center=0.5, coord_mode="affine", border="hardcut", act_order="post")
CONVENTIONS = {"mpv": MPV, "utils_mpi": dict()}
FWD_DEFAULT, FWD_ONE_FRAME, FWD_PAIRS = 0, 0x600, 0x700
D = 5
SIZES = [(64, 16), (70, 17), (130, 1), (33, 47)]            # (W, H): one tile; ragged width, odd height; a single row; narrow and tall
STACKS = ["1.0x", "1.1x", "1.6x", "rot20"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def bench_homos(D, H, W):
    """the benchmark's camera (bench.py) at this frame size."""
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    return compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3),
                              make_depths(D, 1.0, 100.0).flip(0)[None])[0]


def scene(conv, kind, W, H, D=D):
    """(spec keywords, homos [D,3,3], Hs, Ws) of a frame under the benchmark's camera over a stack `kind`: 1.0x / 1.1x / 1.6x the frame
    (the planar convention scales texel coordinates, the utils_mpi one its homographies), or 1.0x seen rotated by 20 degrees."""
    kw = dict(CONVENTIONS[conv])
    homos = bench_homos(D, H, W)
    s = 1.0 if kind == "rot20" else float(kind[:-1])
    Hs, Ws = max(2, round(H * s)), max(2, round(W * s))      # (two texel rows under the single-row frame: one row covers nothing)
    if kind == "rot20":
        th, cx, cy = math.radians(20.0), W / 2.0, H / 2.0
        c, sn = math.cos(th), math.sin(th)
        homos = homos @ torch.tensor([[c, -sn, cx - c * cx + sn * cy], [sn, c, cy - sn * cx - c * cy], [0.0, 0.0, 1.0]])
    elif conv == "mpv":
        kw.update(scale=(Ws / W, Hs / H))
    else:
        homos = torch.diag(torch.tensor([Ws / W, Hs / H, 1.0])) @ homos
    return kw, homos, Hs, Ws


def own_lanes(kw, homos, H, W, Hs, Ws, window=(0, 0)):
    """(pairs that fetch their own taps, pairs) over all planes, by make_taps' rule in fp32 on the host."""
    pc = float(kw.get("pixel_center", 0.0))
    affine = kw.get("coord_mode", "utils_mpi") == "affine"
    sx, sy = kw.get("scale", (1.0, 1.0))
    ox, oy = kw.get("offset", (0.0, 0.0))
    px = (torch.arange(W, dtype=torch.float32) + float(window[1]) + pc)[None, :]
    py = (torch.arange(H, dtype=torch.float32) + float(window[0]) + pc)[:, None]
    own = pairs = 0
    for h in homos.to(torch.float32).reshape(-1, 9):
        Z = h[6] * px + h[7] * py + h[8]
        qx, qy = (h[0] * px + h[1] * py + h[2]) / Z, (h[3] * px + h[4] * py + h[5]) / Z
        tx = qx * sx + ox if affine else qx / (Ws / 2.0) * 0.5 * (Ws - 1)
        ty = qy * sy + oy if affine else qy / (Hs / 2.0) * 0.5 * (Hs - 1)
        x0 = tx.floor().clamp(0, max(Ws - 2, 0)).long()
        y0 = ty.floor().clamp(0, max(Hs - 2, 0)).long()
        off = y0 * Ws + x0
        up, lo = off[0:H - (H & 1):2], off[1::2]
        own += int((lo != up + (Ws if Hs > 1 else 0)).sum())
        pairs += up.numel()
    return own, pairs


def assert_both_paths(scenes, H, W, window=(0, 0)):
    """`scenes`: the (kw, homos, Hs, Ws) a case renders; over them, some pairs fetch their own taps and some share."""
    counts = [own_lanes(kw, homos, H, W, Hs, Ws, window) for kw, homos, Hs, Ws in scenes]
    own, pairs = sum(c[0] for c in counts), sum(c[1] for c in counts)
    if H == 1:
        assert pairs == 0
    else:
        assert 0 < own < pairs, f"own-taps pairs {own} of {pairs}: one of the two paths does not run in this case"
    return own, pairs


def fwd(stack, homos, H, W, kw, variant, window=(0, 0), quad_keep=None):
    """vl3d_render_fwd -> (rgb, alpha, asum); the outputs start as NaN, so a pixel a kernel does not write compares unequal."""
    from videoloop3d_amd import _lib as L, render as R
    spec = R.RenderSpec(variant=variant, **kw)
    T, dev = stack.shape[1], stack.device
    desc = R._desc(stack, H, W, spec, int(window[0]), int(window[1]))
    rgb = torch.full((T, H, W, 3), float("nan"), device=dev)
    alpha = torch.full((T, H, W), float("nan"), device=dev)
    asum = torch.full((T, H, W, 2), float("nan"), device=dev)
    homos = homos.to(dev).to(torch.float32).contiguous()
    with torch.cuda.device(dev):
        qk = None if quad_keep is None else R._quad_map(quad_keep.to(dev), stack.shape[0])
        cull = None if qk is None else R._cull_scratch(desc, dev)
        L.check(L.lib().vl3d_render_fwd(desc, L.ptr(stack), L.ptr(homos), *R._qmap(qk, spec), L.ptr(cull), L.ptr(rgb), L.ptr(alpha), L.ptr(asum),
                                        L.stream_ptr(dev)), "vl3d_render_fwd")
    return rgb, alpha, asum


def assert_three_kernels_equal(stack, homos, H, W, kw, window=(0, 0), quad_keep=None):
    ref = fwd(stack, homos, H, W, kw, FWD_DEFAULT, window, quad_keep)
    assert all(bool(torch.isfinite(o).all()) for o in ref), "the default forward left pixels unwritten"
    assert float(ref[1].max()) > 0.01, "nothing rendered"
    for variant in (FWD_PAIRS, FWD_ONE_FRAME):
        out = fwd(stack, homos, H, W, kw, variant, window, quad_keep)
        for name, a, b in zip(("rgb", "alpha", "asum"), ref, out):
            assert torch.equal(a, b), f"{name}: the default forward differs from variant {variant:#x} in {int((a != b).sum())} values"


@pytest.mark.parametrize("kind", STACKS)
@pytest.mark.parametrize("W,H", SIZES)
def test_row_pairs_equal_frame_pairs_and_one_frame_kernel_bitwise(dev, W, H, kind):
    """A case = frame size x stack, rendered under both coordinate conventions.  (33 x 47 at 1.0x: the benchmark camera's row pitch of 1.005
    texels skips no row in 47, so under the planar convention every pair shares; the utils_mpi convention's pitch of (Hs - 1) / Hs repeats one.)"""
    scenes = [scene(conv, kind, W, H) for conv in CONVENTIONS]
    assert_both_paths(scenes, H, W)
    for kw, homos, Hs, Ws in scenes:
        for T in (1, 2, 5):
            stack = synth.make_plane_stack(D, T, Hs, Ws, seed=31 + T, device=dev)
            assert_three_kernels_equal(stack, homos, H, W, kw)


@pytest.mark.parametrize("conv", list(CONVENTIONS))
def test_row_pairs_in_a_window_of_the_frame(dev, conv):
    """row0, col0 != 0 (odd: the pairs start on an odd frame row), a window that is no multiple of the tile."""
    Wf, Hf, W, H, window = 150, 60, 70, 33, (7, 13)
    for kind in ("1.1x", "1.6x"):
        kw, homos, Hs, Ws = scene(conv, kind, Wf, Hf)
        assert_both_paths([(kw, homos, Hs, Ws)], H, W, window)
        stack = synth.make_plane_stack(D, 3, Hs, Ws, seed=37, device=dev)
        assert_three_kernels_equal(stack, homos, H, W, kw, window)
        full = fwd(stack, homos, Hf, Wf, kw, FWD_DEFAULT)
        part = fwd(stack, homos, H, W, kw, FWD_DEFAULT, window)
        for a, b in zip(full, part):
            assert torch.equal(a[:, window[0]:window[0] + H, window[1]:window[1] + W], b)


@pytest.mark.parametrize("nframes", [2, 3])
def test_row_pairs_on_a_run_of_frames_inside_a_longer_clip(dev, nframes):
    """vl3d_render_fwd_frames: the planes of the run are a clip's length apart, not the run's."""
    from videoloop3d_amd.render import RenderSpec, render_frame_run
    W, H, frame0 = 70, 17, 2
    for conv in CONVENTIONS:
        kw, homos, Hs, Ws = scene(conv, "1.1x", W, H)
        assert_both_paths([(kw, homos, Hs, Ws)], H, W)
        clip = synth.make_plane_stack(D, 7, Hs, Ws, seed=43, device=dev)
        outs = [render_frame_run(clip, frame0, nframes, homos.to(dev), H, W, RenderSpec(variant=v, **kw)) for v in (FWD_DEFAULT, FWD_PAIRS, FWD_ONE_FRAME)]
        gathered = fwd(clip[:, frame0:frame0 + nframes].contiguous(), homos, H, W, kw, FWD_DEFAULT)
        for out in outs[1:] + [gathered[:2]]:
            assert torch.equal(outs[0][0], out[0]) and torch.equal(outs[0][1], out[1])


def test_row_pairs_fuzz_32_small_scenes(dev):
    """fixed seed: random plane counts, clip lengths, frame sizes, stack scales, views (shift, zoom, rotation, perspective), windows."""
    gen = torch.Generator().manual_seed(20250)
    rnd = lambda lo, hi: lo + (hi - lo) * float(torch.rand((), generator=gen))
    rint = lambda lo, hi: int(torch.randint(lo, hi + 1, (), generator=gen))
    ran_own = ran_shared = 0
    for i in range(32):
        conv = ("mpv", "utils_mpi")[i & 1]
        Dn, T, W, H = rint(1, 6), rint(2, 5), rint(1, 140), rint(1, 40)
        kw, homos, Hs, Ws = scene(conv, f"{rnd(0.8, 1.7):.2f}x", W + rint(0, 9), H + rint(0, 9), Dn)
        th, z = math.radians(rnd(-8.0, 8.0)), rnd(0.9, 1.1)
        view = torch.tensor([[z * math.cos(th), -math.sin(th), rnd(-3, 3)], [math.sin(th), z * math.cos(th), rnd(-3, 3)], [rnd(-2e-4, 2e-4), rnd(-2e-4, 2e-4), 1.0]])
        homos = homos @ view
        window = (rint(0, 5), rint(0, 5)) if i % 3 == 0 else (0, 0)
        own, pairs = own_lanes(kw, homos, H, W, Hs, Ws, window)
        ran_own, ran_shared = ran_own + own, ran_shared + pairs - own
        stack = synth.make_plane_stack(Dn, T, Hs, Ws, seed=100 + i, device=dev)
        ref = fwd(stack, homos, H, W, kw, FWD_DEFAULT, window)
        assert all(bool(torch.isfinite(o).all()) for o in ref), f"scene {i}"
        for variant in (FWD_PAIRS, FWD_ONE_FRAME):
            for a, b in zip(ref, fwd(stack, homos, H, W, kw, variant, window)):
                assert torch.equal(a, b), f"scene {i} ({conv}, D={Dn}, T={T}, {W}x{H} of stack {Ws}x{Hs}, window {window}): differs from variant {variant:#x}"
    assert ran_own > 1000 and ran_shared > 1000, (ran_own, ran_shared)


@pytest.mark.parametrize("T", [2, 5])
def test_fp16_and_tile_culled_forwards_keep_their_kernels_bits(dev, T):
    """fp16 stacks and tile-culled models stay on the frame pairs: the default call, variant 7 and the one-frame kernel give the same bits."""
    W, H = 70, 17
    kw, homos, Hs, Ws = scene("mpv", "1.1x", W, H)
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=53, device=dev)
    assert_three_kernels_equal(stack.to(torch.float16), homos, H, W, kw)
    keep = torch.rand(D, 3, 4, generator=torch.Generator().manual_seed(5)) < 0.6
    assert_three_kernels_equal(stack, homos, H, W, kw, quad_keep=keep)
    culled, dense = fwd(stack, homos, H, W, kw, FWD_DEFAULT, quad_keep=keep), fwd(stack, homos, H, W, kw, FWD_DEFAULT)
    assert not torch.equal(culled[1], dense[1]), "the quad map culled nothing: the culled forward was not exercised"
