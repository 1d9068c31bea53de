"""The playback model on the MI355X (videoloop3d_amd/baked.py, csrc/vl3d_render_baked.hip): the bake rule u8 = uint8(trunc(clip(act(s) * 255,
0, 255))), the forward render from baked RGBA8 texels (bilinear blend of the decoded taps, no activation behind it) against the pinned float
kernels and against a plain fp64 statement, its guards, and bake() / render_frames(baked=...) on a tiny sparsified tile-exact MPMeshVid.

Shapes: D = 4 planes, a clip of 5 frames of which frames 1..3 are rendered (an odd run: one frame pair and its tail), planes of 40 x 72 texels
= 5 x 9 quads of 8 x 8, output 37 x 70 (no multiple of the 64 x 8 workgroup tile, an odd row count: 2 x 5 workgroups), the benchmark camera
of synth.make_cameras (translation (0.03, 0.01, 0), 0.5 degrees about y) on planes scaled and shifted so that they leave the frame on its sides."""
import dataclasses
import types

import numpy as np
import pytest
import torch

import baked_models as BM
from baked_models import D, H, HS, QH, QW, T_ALLOC, W, WS
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu

F0, NF = 1, 3
# the activation pairs the product's dispatch table lists (csrc/vl3d_render_packed.hip, conv_affine_hardcut_post_*)
ACT_PAIRS = [("sigmoid", "sigmoid"), ("none", "none"), ("none", "sigmoid"), ("clamp", "sigmoid"), ("relu", "sigmoid"), ("abs", "sigmoid"),
             ("clamp", "clamp"), ("sigmoid", "clamp"), ("none", "clamp")]


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _homographies():
    """[D,3,3] target pixel -> plane pixel of the benchmark camera (near 1, far 100), as __graft_entry__.smoke() forms them."""
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    depths = make_depths(D, 1.0, 100.0).flip(0)
    return compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3), depths[None])[0].float()


@pytest.fixture(scope="module")
def scene(dev):
    """the baked clip (hash-random texels through the bake kernel), the homographies, a quad map with about half of the quads and no quad of
    plane 2, and the float kernels' render of the decoded texels per layout -- computed once, never modified."""
    from videoloop3d_amd.baked import bake_texels
    from videoloop3d_amd.render import render_frame_run
    stack = synth.make_plane_stack(D, T_ALLOC, HS, WS, seed=7, device=dev, alpha_bias=-0.5)
    baked = bake_texels(stack, "sigmoid", "sigmoid")
    keep = synth.hash_uniform((D, QH, QW), seed=11) < 0.5
    keep[2] = False
    assert 0.3 < float(keep.float().mean()) < 0.6
    keep = keep.to(torch.uint8).to(dev)
    homos = _homographies().to(dev)
    decoded = baked.float() / 255
    ref = {}
    for layout, spec in BM.specs().items():
        qk = None if layout == "dense" else keep
        rgb, alpha = render_frame_run(decoded, F0, NF, homos, H, W, spec, quad_keep=qk)
        ref[layout] = (rgb.clone(), alpha.clone())
    return types.SimpleNamespace(baked=baked, keep=keep, homos=homos, ref=ref)


# ---- 1. the bake rule --------------------------------------------------------------------------------------------------------------------
def _torch_rule(t, rgb_act, alpha_act):
    from videoloop3d_amd.plane_model import ACTIVATES
    s = t.float()
    a = torch.cat([ACTIVATES[rgb_act](s[..., :3]), ACTIVATES[alpha_act](s[..., 3:])], -1)
    return (a * 255).clamp(0, 255).to(torch.uint8)      # (.to(uint8) truncates)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_bake_rule_exact_levels(dev, dtype):
    """logit((k + 0.5) / 255) is half a level away from either boundary: every one of the 255 levels bakes to exactly k, in every channel; the
    ends saturate.  (fp16: the logits are rounded to 11 bits first -- at most 2e-3 of a logit, a few hundredths of a level; still exact.)"""
    from videoloop3d_amd.baked import bake_texels
    k = torch.arange(255, dtype=torch.float64)
    p = (k + 0.5) / 255
    t = torch.log(p / (1 - p)).to(dtype)[:, None].expand(255, 4).contiguous().to(dev)
    out = bake_texels(t, "sigmoid", "sigmoid")
    assert out.dtype == torch.uint8 and out.shape == (255, 4) and out.device == t.device
    assert torch.equal(out.cpu(), k.to(torch.uint8)[:, None].expand(255, 4))
    ends = torch.tensor([[-30.0] * 4, [30.0] * 4], dtype=dtype, device=dev)
    assert bake_texels(ends, "sigmoid", "sigmoid").tolist() == [[0] * 4, [255] * 4]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("acts", ACT_PAIRS, ids=["-".join(a) for a in ACT_PAIRS])
def test_bake_random_texels_within_one_level(dev, dtype, acts):
    """hash-random texels, an odd texel count (the fp16 kernel's two-texel loads and their tail): every byte within 1 of the torch expression,
    on the device and on the host (the same function: the export runs on the host)."""
    from videoloop3d_amd.baked import bake_texels
    t = (synth.hash_uniform((3, 37, 23, 4), seed=13, device=dev) * 6 - 3).to(dtype)
    out = bake_texels(t, *acts)
    want = _torch_rule(t, *acts)
    diff = (out.int() - want.int()).abs()
    print(f"bake {acts} {dtype}: max |level diff| {int(diff.max())}, differing bytes {int((diff > 0).sum())} of {diff.numel()}")
    assert int(diff.max()) <= 1
    assert int((bake_texels(t.cpu(), *acts).int() - want.cpu().int()).abs().max()) <= 1


_ACT64 = {"sigmoid": lambda v: 1 / (1 + torch.exp(-v)), "none": lambda v: v, "clamp": lambda v: v.clamp(0, 1), "relu": torch.relu, "abs": torch.abs}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("acts", ACT_PAIRS, ids=["-".join(a) for a in ACT_PAIRS])
def test_bake_rule_fp64_interval(dev, dtype, acts):
    """the bake rule against fp64, where the test above accepts any byte within one level (a kernel that rounds instead of truncating passes
    it).  a64 = act(s widened) in float64; every byte b satisfies floor(255 a64 (1 - r)) <= b <= floor(255 a64 (1 + r)) after the clip to
    [0, 255].  r = 8 * 2^-24 for sigmoid: __expf(-v) is an exp2 of a rounded product -- |v| <= 3 ulp in the result --, one ulp each for the
    exp2, the reciprocal, `1 +` and `* 255` (vl3d_common.h: "4 instrs, ~1 ulp").  r = 2^-24 for clamp / relu / abs / none, exact in fp32: the only
    rounding is `* 255`.  The same inputs as above (|s| <= 3, the odd texel count); the host path of bake_texels meets the same interval."""
    from videoloop3d_amd.baked import bake_texels
    t = (synth.hash_uniform((3, 37, 23, 4), seed=13, device=dev) * 6 - 3).to(dtype)
    s = t.cpu().double()
    a64 = torch.cat([_ACT64[acts[0]](s[..., :3]), _ACT64[acts[1]](s[..., 3:])], -1)
    r = torch.tensor([8 * 2.0 ** -24 if a == "sigmoid" else 2.0 ** -24 for a in (acts[0],) * 3 + (acts[1],)], dtype=torch.float64)
    lo = (255 * a64 * (1 - r)).clamp(0, 255).floor().long()
    hi = (255 * a64 * (1 + r)).clamp(0, 255).floor().long()
    two = int((hi > lo).sum())
    for where, out in (("device", bake_texels(t, *acts)), ("host", bake_texels(t.cpu(), *acts))):
        b = out.cpu().long()
        outside = int(((b < lo) | (b > hi)).sum())
        print(f"bake {acts} {dtype} [{where}]: {outside} bytes outside the fp64 interval, {two} two-valued intervals of {b.numel()}")
        assert out.dtype == torch.uint8 and outside == 0, (where, outside)


# ---- 2. parity with the pinned float kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "shared", "exact"])
def test_baked_render_matches_the_float_kernels(dev, scene, layout):
    """render_frame_run_baked(baked) against render_frame_run(baked / 255) under identity activations -- the order of activation and
    interpolation is then immaterial, and the float kernels are pinned to goldens G2 / G17 / G19.  1e-5 max abs on EVERY pixel, rgb and alpha
    (the forward tolerance of tests/test_gpu_render.py): coverage comes from the same device functions in both renders."""
    from videoloop3d_amd.render import render_frame_run_baked
    spec = BM.specs()[layout]
    qk = None if layout == "dense" else scene.keep
    rgb, alpha = render_frame_run_baked(scene.baked, F0, NF, scene.homos, H, W, spec, quad_keep=qk)
    rgb_f, alpha_f = scene.ref[layout]
    e_rgb, e_a = float((rgb - rgb_f).abs().max()), float((alpha - alpha_f).abs().max())
    covered = float((alpha_f > 0).float().mean())
    print(f"baked vs float [{layout}]: max |d rgb| {e_rgb:.3e}, max |d alpha| {e_a:.3e}, covered pixels {covered:.3f}")
    assert rgb.shape == (NF, H, W, 3) and alpha.shape == (NF, H, W)
    assert e_rgb <= 1e-5 and e_a <= 1e-5
    # the case is not trivial: hard-cut edges on two sides (uncovered pixels in the first AND the last columns), and frames that differ
    assert 0.3 < covered < 1.0
    if layout == "dense":
        assert bool((alpha_f[:, :, 0] < alpha_f[:, :, 8]).any()) and bool((alpha_f[:, :, -1] < alpha_f[:, :, -9]).any())
    assert float((rgb_f[0] - rgb_f[2]).abs().max()) > 0.05
    # a single frame (the one-frame kernel) and an even run equal the frames of the odd run bit for bit
    r1, a1 = render_frame_run_baked(scene.baked, F0 + 2, 1, scene.homos, H, W, spec, quad_keep=qk)
    assert torch.equal(r1[0], rgb[2]) and torch.equal(a1[0], alpha[2])
    r2, a2 = render_frame_run_baked(scene.baked, F0, 2, scene.homos, H, W, spec, quad_keep=qk)
    assert torch.equal(r2, rgb[:2]) and torch.equal(a2, alpha[:2])


# ---- 3. parity with a statement written here -----------------------------------------------------------------------------------------------
def _fp64_render(baked, homos, spec, frames):
    """decode, four taps, hard cut, front-to-back composite, plane by plane in fp64 -> (rgb [n,H,W,3], alpha [n,H,W], inside [H,W]: the pixels
    whose sample lies at least 2 texels inside every plane)."""
    tex = baked.double() / 255
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=baked.device) + spec.pixel_center,
                            torch.arange(W, dtype=torch.float64, device=baked.device) + spec.pixel_center, indexing="ij")
    n = len(frames)
    Tr = torch.ones((n, H, W), dtype=torch.float64, device=baked.device)
    rgb = torch.zeros((n, H, W, 3), dtype=torch.float64, device=baked.device)
    acc = torch.zeros((n, H, W), dtype=torch.float64, device=baked.device)
    inside = torch.ones((H, W), dtype=torch.bool, device=baked.device)
    for d in range(baked.shape[0]):
        h = homos[d].double()
        Z = h[2, 0] * xs + h[2, 1] * ys + h[2, 2]
        u = (h[0, 0] * xs + h[0, 1] * ys + h[0, 2]) / Z * spec.scale[0] + spec.offset[0]
        v = (h[1, 0] * xs + h[1, 1] * ys + h[1, 2]) / Z * spec.scale[1] + spec.offset[1]
        cov = (u >= 0) & (u <= WS - 1) & (v >= 0) & (v <= HS - 1)                     # the hard cut at the outermost texel centres
        inside &= (u >= 2) & (u <= WS - 3) & (v >= 2) & (v <= HS - 3)
        x0, y0 = u.floor().clamp(0, WS - 2).long(), v.floor().clamp(0, HS - 2).long()
        fx, fy = (u - x0).clamp(0, 1), (v - y0).clamp(0, 1)
        pl = tex[d, frames]                                                              # n,HS,WS,4
        val = (pl[:, y0, x0] * ((1 - fx) * (1 - fy))[None, ..., None] + pl[:, y0, x0 + 1] * (fx * (1 - fy))[None, ..., None]
               + pl[:, y0 + 1, x0] * ((1 - fx) * fy)[None, ..., None] + pl[:, y0 + 1, x0 + 1] * (fx * fy)[None, ..., None])
        a = val[..., 3] * cov[None]
        w = a * Tr
        rgb += w[..., None] * val[..., :3]
        acc += w
        Tr = Tr * (1 - a)
    return rgb, acc, inside


def test_baked_render_matches_a_plain_fp64_statement(dev, scene):
    from videoloop3d_amd.render import render_frame_run_baked
    spec = BM.specs()["dense"]
    rgb, alpha = render_frame_run_baked(scene.baked, F0, NF, scene.homos, H, W, spec)
    rgb64, a64, inside = _fp64_render(scene.baked, scene.homos, spec, list(range(F0, F0 + NF)))
    assert int(inside.sum()) > H * W // 2
    sel = inside[None].expand(NF, H, W)
    e_rgb, e_a = float((rgb.double() - rgb64)[sel].abs().max()), float((alpha.double() - a64)[sel].abs().max())
    print(f"baked vs fp64 statement: max |d rgb| {e_rgb:.3e}, max |d alpha| {e_a:.3e} on {int(inside.sum())} interior pixels")
    assert e_rgb <= 1e-5 and e_a <= 1e-5
    assert float(a64[sel].min()) > 0.3      # (the interior is covered by all four planes)


# ---- 4. determinism and guards ---------------------------------------------------------------------------------------------------------
def test_determinism_and_guards(dev, scene):
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd.render import RenderSpec, _desc, render_frame_run_baked
    specs = BM.specs()
    for layout in ("dense", "exact"):
        qk = None if layout == "dense" else scene.keep
        a = render_frame_run_baked(scene.baked, F0, NF, scene.homos, H, W, specs[layout], quad_keep=qk)
        b = render_frame_run_baked(scene.baked, F0, NF, scene.homos, H, W, specs[layout], quad_keep=qk)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    lib = L.lib()
    rgb = torch.empty((NF, H, W, 3), device=dev)
    alpha = torch.empty((NF, H, W), device=dev)
    stream = L.stream_ptr(dev)

    def desc(spec, dtype):
        d = _desc(scene.baked, H, W, spec, 0, 0)
        d.T, d.stack_dtype = NF, L.STACK_DTYPE[dtype]
        return d

    def baked_rc(d):
        return lib.vl3d_render_fwd_baked(d, L.ptr(scene.baked), T_ALLOC, L.ptr(scene.homos), BM.run_sel(F0), None, 0, 0, None, BM.float_out(rgb, alpha),
                                         stream)
    EINVAL = 1
    assert baked_rc(desc(specs["dense"], "u8")) == 0
    # the float entry points refuse baked texels (error returns, before any launch)
    d = desc(specs["dense"], "u8")
    d.T = T_ALLOC
    assert lib.vl3d_render_fwd(d, L.ptr(scene.baked), L.ptr(scene.homos), None, 0, 0, None, L.ptr(rgb), L.ptr(alpha), None, stream) == EINVAL
    assert b"stack_dtype" in lib.vl3d_last_error()
    d.T = NF
    assert lib.vl3d_render_fwd_frames(d, L.ptr(scene.baked), F0, T_ALLOC, L.ptr(scene.homos), None, 0, 0, None, L.ptr(rgb), L.ptr(alpha), stream) == EINVAL
    # the baked entry refuses everything but the planar convention on VL3D_U8 texels
    assert baked_rc(desc(RenderSpec(), "u8")) == EINVAL                                              # utils_mpi coordinates
    assert b"planar" in lib.vl3d_last_error()
    assert baked_rc(desc(dataclasses.replace(specs["dense"], uv_noise_seed=5), "u8")) == EINVAL
    assert b"uv_noise" in lib.vl3d_last_error()
    assert baked_rc(desc(specs["dense"], "f32")) == EINVAL
    d = desc(specs["dense"], "u8")
    d.T = T_ALLOC      # frames 1 .. 5 of a clip of 5
    assert baked_rc(d) == EINVAL
    with pytest.raises(RuntimeError, match="planar"):
        render_frame_run_baked(scene.baked, F0, NF, scene.homos, H, W, RenderSpec())
    with pytest.raises(RuntimeError, match="uint8"):
        render_frame_run_baked(scene.baked.float(), F0, NF, scene.homos, H, W, specs["dense"])
    with pytest.raises(RuntimeError, match="no backward"):
        with torch.enable_grad():
            render_frame_run_baked(scene.baked, F0, NF, scene.homos.clone().requires_grad_(True), H, W, specs["dense"])
    torch.cuda.synchronize()


# ---- 5. module level -------------------------------------------------------------------------------------------------------------------
def test_module_bake_and_render_frames(dev):
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd.baked import BakedMPV, bake
    from videoloop3d_amd.render import render_frame_run
    model, Hm, Wm, K = BM.tile_exact_model(dev, "0.2#0.4#0.6")
    baked = bake(model)
    assert isinstance(baked, BakedMPV) and baked.texels.dtype == torch.uint8 and baked.texels.shape == model.stack.shape
    assert baked.nbytes * 4 == model.stack.numel() * model.stack.element_size()
    assert baked.quad_keep is not None and baked.spec == model.spec
    # three cameras (world-to-camera), frames: a run of three on the first camera, then single frames
    ext = np.tile(np.eye(4, dtype=np.float32)[None], (5, 1, 1))
    ext[3:, :3, 3] = [0.03, 0.01, 0.0]
    ext[4, :3, 3] = [-0.05, 0.02, 0.01]
    intr = np.tile(K.astype(np.float32)[None], (5, 1, 1))
    rt = np.array([1, 2, 3, 5, 0])
    frames = RV.render_frames(model, Hm, Wm, ext, intr, rt, baked=baked)
    assert frames.shape == (5, Hm, Wm, 3) and frames.dtype == torch.uint8 and frames.device.type == "cuda"
    # the float kernels on the decoded texels, through the same homographies, quad map and background
    spec = dataclasses.replace(model.spec, rgb_act="none", alpha_act="none")
    decoded = baked.texels.float() / 255
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    worst = 0
    for i in range(5):
        e = torch.tensor(ext[i:i + 1]) @ model.ref_extrin.cpu()[None].inverse().float()
        homos = model.plane_homographies(e, torch.tensor(intr[i:i + 1])).to(dev)
        rgb, alpha = render_frame_run(decoded, int(rt[i]), 1, homos, Hm, Wm, spec, quad_keep=model.quad_keep)
        want = RV.to8b(rgb * alpha[..., None] + bg[None, None, None] * (-alpha[..., None] + 1))[0]
        worst = max(worst, int((frames[i].int() - want.int()).abs().max()))
        # BakedMPV.render: the module's eval forward on the baked texels
        r, a = baked.render(Hm, Wm, torch.tensor(ext[i:i + 1]), torch.tensor(intr[i:i + 1]), torch.tensor(rt[i:i + 1]))
        assert r.shape == (1, 3, Hm, Wm) and a.shape == (1, Hm, Wm)
        assert int((RV.to8b(r.permute(0, 2, 3, 1))[0].int() - frames[i].int()).abs().max()) <= 1
    print(f"render_frames(baked=...) vs to8b(float render of the decoded texels): max |level diff| {worst}")
    assert worst <= 1
    assert float(frames.float().std()) > 1.0
    # the playback picture is close to the float model's, not equal to it (8-bit texels, activation before the filter)
    plain = RV.render_frames(model, Hm, Wm, ext, intr, rt)
    mse = float(((plain.float() - frames.float()) / 255).pow(2).mean())
    assert 0 < mse < 1e-2
    # a packed model, an atlas_exact model and a model on the host are refused
    model.pack_()
    with pytest.raises(RuntimeError, match="packed"):
        bake(model)
    cpu_model, _, _, _ = BM.tile_exact_model(torch.device("cpu"), "")
    with pytest.raises(RuntimeError, match="host"):
        bake(cpu_model)
    cpu_model.atlas_exact = True
    with pytest.raises(RuntimeError, match="atlas_exact"):
        bake(cpu_model)
