"""The baked playback model along a camera path on the MI355X (render.render_path_baked / render_path_baked_pool; the path selection
of vl3d_render_fwd_baked / _pool): N output frames, each with its own camera and its own frame of the clip, in one plan launch plus one render launch.  The
one-camera one-frame kernels (pinned by tests/test_gpu_baked.py and tests/test_gpu_baked_pool.py) are the oracle and the comparison is EXACT:
a frame has the same bits alone, in an even run and in an odd run (the composite is spelt out with contraction off), so every path frame must
be torch.equal to render_frame_run_baked(baked, t_i, 1, homos[cam_i], ...) -- no tolerance.

Shapes of tests/test_gpu_baked.py: D = 4, a clip of 5 frames, planes of 40 x 72 texels = 5 x 9 quads of 8 x 8, output 37 x 70 (2 x 5 workgroups of
64 x 8, a ragged edge, hard cuts inside the view), the layouts dense / shared / exact.  Three cameras: the benchmark camera, one with the
opposite translation, one whose principal point is shifted by 24 px (three quads).  The path: N = 7 output frames, (cam, t) = (0,1), (1,1),
(2,4), (0,0), (1,3), (1,4), (2,2) -- a repeated camera, non-monotone t, the first and the last frame of the clip, an odd N."""
import types

import numpy as np
import pytest
import torch

import baked_models as BM
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu

D, T, H, W = BM.D, BM.T_ALLOC, BM.H, BM.W
PATH = [(0, 1), (1, 1), (2, 4), (0, 0), (1, 3), (1, 4), (2, 2)]
CAM = [c for c, _ in PATH]
TS = [t for _, t in PATH]
N = len(PATH)
TILES = ((H + 7) // 8) * ((W + 63) // 64)


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _homographies():
    """[3,D,3,3] target pixel -> plane pixel of the three cameras (near 1, far 100)."""
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    opposite = tar_e.clone()
    opposite[:3, 3] = -tar_e[:3, 3]
    shifted = Kt.clone()
    shifted[0, 2] += 24.0
    depths = make_depths(D, 1.0, 100.0).flip(0)
    normal = torch.tensor([0., 0., 1.]).expand(1, D, 3)
    return torch.stack([compute_homography(ref_e[None], Kr[None], e[None], k[None], normal, depths[None])[0].float()
                        for e, k in ((tar_e, Kt), (opposite, Kt), (tar_e, shifted))])


def _assert_bit_equal(path_out, single):
    """every path frame against its one-frame render: `single(i)` -> (rgb [1,H,W,3], alpha [1,H,W])"""
    rgb, alpha = path_out
    assert rgb.shape == (N, H, W, 3) and alpha.shape == (N, H, W) and rgb.dtype == alpha.dtype == torch.float32
    for i in range(N):
        r1, a1 = single(i)
        print(f"  frame {i} (cam {CAM[i]}, t {TS[i]}): max |d rgb| {float((rgb[i] - r1[0]).abs().max()):.3e}, "
              f"max |d alpha| {float((alpha[i] - a1[0]).abs().max()):.3e}")
        assert torch.equal(rgb[i], r1[0]) and torch.equal(alpha[i], a1[0]), i


@pytest.fixture(scope="module")
def scene(dev):
    """the baked clip and quad map of tests/test_gpu_baked.py, the three cameras' homographies, and per layout the seven one-frame renders --
    the reference, computed once and never modified."""
    from videoloop3d_amd.baked import bake_texels
    from videoloop3d_amd.render import render_frame_run_baked
    baked = bake_texels(synth.make_plane_stack(D, T, BM.HS, BM.WS, seed=7, device=dev, alpha_bias=-0.5), "sigmoid", "sigmoid")
    keep = synth.hash_uniform((D, BM.QH, BM.QW), seed=11) < 0.5
    keep[2] = False
    keep = keep.to(torch.uint8).to(dev)
    sparse = torch.zeros((D, BM.QH, BM.QW), dtype=torch.uint8)      # plane d keeps only quad column 2 d + 1, plane 2 nothing
    for d in range(D):
        if d != 2:
            sparse[d, :, 2 * d + 1] = 1
    sparse = sparse.to(dev)
    homos = _homographies().to(dev)
    specs = BM.specs()

    def singles(layout, qk):
        return [tuple(x.clone() for x in render_frame_run_baked(baked, TS[i], 1, homos[CAM[i]], H, W, specs[layout], quad_keep=qk)) for i in range(N)]
    ref = {layout: singles(layout, None if layout == "dense" else keep) for layout in specs}
    ref_sparse = {layout: singles(layout, sparse) for layout in ("shared", "exact")}
    return types.SimpleNamespace(baked=baked, keep=keep, sparse=sparse, homos=homos, specs=specs, ref=ref, ref_sparse=ref_sparse)


# ---- 1. the dense clip ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "shared", "exact"])
def test_path_frames_equal_their_single_frame_renders(dev, scene, layout):
    from videoloop3d_amd.render import render_path_baked
    qk = None if layout == "dense" else scene.keep
    out = render_path_baked(scene.baked, CAM, TS, scene.homos, H, W, scene.specs[layout], quad_keep=qk)
    ref = scene.ref[layout]
    _assert_bit_equal(out, lambda i: ref[i])
    # numpy indices and caller-owned buffers: the same bits
    buf = (torch.full((N, H, W, 3), 123.0, device=dev), torch.full((N, H, W), 123.0, device=dev))
    got = render_path_baked(scene.baked, np.array(CAM, dtype=np.int64), np.array(TS, dtype=np.int32), scene.homos, H, W, scene.specs[layout], out=buf,
                            quad_keep=qk)
    assert got[0] is buf[0] and got[1] is buf[1] and torch.equal(buf[0], out[0]) and torch.equal(buf[1], out[1])
    # the case is not trivial: frames of different cameras at the same t differ (path frames 0 and 1: cameras 0 and 1 at t = 1; 4 and ... cameras
    # 1 and 2 at t = 4 are frames 5 and 2), hard-cut edges inside the view
    d01 = float((out[0][0] - out[0][1]).abs().max())
    d12 = float((out[0][5] - out[0][2]).abs().max())
    covered = float((out[1] > 0).float().mean())
    print(f"[{layout}] cameras 0 / 1 at t = 1 differ by {d01:.3f}, cameras 1 / 2 at t = 4 by {d12:.3f}; covered pixels {covered:.3f}")
    assert d01 > 0.05 and d12 > 0.05
    assert 0.3 < covered < 1.0


# ---- 2. the pool ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(BM.GEOMS))
def test_pool_path_frames_equal_their_single_frame_renders(dev, scene, geom):
    """the pool of tests/test_gpu_baked_pool.py (hash-random texels behind the block table, static / dynamic / unstored blocks), both tile layouts"""
    from videoloop3d_amd.baked import BakedMPV, BakedPool, bake_texels
    from videoloop3d_amd.packed import PackedLayout
    from videoloop3d_amd.render import render_frame_run_baked_pool, render_path_baked_pool
    g = BM.GEOMS[geom]
    keep = synth.hash_uniform((D, g["QH"], g["QW"]), seed=11) < 0.5
    keep[2] = False
    dyn = keep & (synth.hash_uniform((D, g["QH"], g["QW"]), seed=12) < 1.0 / 3.0)
    lay = PackedLayout(keep.to(dev), dyn.to(dev), BM.T_MODEL, g["Hs"], g["Ws"], g["tile"])
    e = lay.blocks
    assert int((e < 0).sum()) > 0 and int(((e >= 0) & ((e & 1) == 0)).sum()) > 0 and int(((e >= 0) & ((e & 1) == 1)).sum()) > 0
    clip = bake_texels(synth.make_plane_stack(D, BM.T_MODEL, g["Hs"], g["Ws"], seed=7, device=dev, alpha_bias=-0.5), "sigmoid", "sigmoid")
    pool = BM.scatter_pool(lay, clip, torch.zeros((1, 4), dtype=torch.uint8, device=dev))
    spec, qk, culled = BM.pool_spec(g), keep.to(torch.uint8).to(dev), 7 | 11 << 8 | 13 << 16 | 0 << 24
    out = render_path_baked_pool(lay, pool, CAM, TS, scene.homos, H, W, spec, quad_keep=qk, culled_rgba8=culled)
    _assert_bit_equal(out, lambda i: render_frame_run_baked_pool(lay, pool, TS[i], 1, scene.homos[CAM[i]], H, W, spec, quad_keep=qk, culled_rgba8=culled))
    covered = float((out[1] > 0).float().mean())
    print(f"[{geom}] covered pixels {covered:.3f}, cameras 0 / 1 at t = 1 differ by {float((out[0][0] - out[0][1]).abs().max()):.3f}")
    assert 0.3 < covered < 1.0 and float((out[0][0] - out[0][1]).abs().max()) > 0.05
    # BakedPool.render_path equals BakedMPV.render_path on the unpacked texels (a camera whose plane_homographies are this file's)
    cam = types.SimpleNamespace(ref_extrin=torch.eye(4), plane_homographies=lambda e, k: scene.homos[int(k[0, 0, 0])].cpu(),
                                _on=lambda device, name: torch.eye(4))
    ext = torch.eye(4)[None].repeat(N, 1, 1)
    intr = torch.eye(3)[None].repeat(N, 1, 1)
    intr[:, 0, 0] = torch.tensor(CAM, dtype=torch.float32)      # (the stand-in camera reads its index here)
    bp = BakedPool(pool, lay, qk, spec, "0.2#0.4#0.6", cam, culled)
    bm = BakedMPV(bp.unpack_frames(range(BM.T_MODEL)), qk, spec, "0.2#0.4#0.6", cam)
    rp, ap = bp.render_path(H, W, ext, intr, TS)
    rm, am = bm.render_path(H, W, ext, intr, TS)
    assert rp.shape == (N, 3, H, W) and ap.shape == (N, H, W)
    assert torch.equal(rp, rm) and torch.equal(ap, am)
    assert torch.equal(ap, out[1])
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    assert torch.equal(rp.permute(0, 2, 3, 1), out[0] * out[1][..., None] + bg[None, None, None] * (-out[1][..., None] + 1))


# ---- 3. the plan is per camera -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["shared", "exact"])
def test_the_plan_is_per_camera(dev, scene, layout):
    """a sparse quad map -- plane d keeps only quad column 2 d + 1, plane 2 nothing -- so that what a 64 x 8 workgroup lists depends on where the
    camera puts the columns; the masks are read back from a caller-held cull_scratch.  A kernel that read another camera's plan would skip
    planes this camera sees (or walk planes it does not): the bit comparison catches the first."""
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd.render import _desc_dims, render_path_baked
    spec = scene.specs[layout]
    need = int(L.lib().vl3d_render_path_cull_scratch_bytes(_desc_dims(D, N, BM.HS, BM.WS, H, W, spec, L.STACK_DTYPE["u8"]), 3))
    assert need == 3 * TILES * 16
    scratch = torch.full((need // 8 + 3,), -1, dtype=torch.int64, device=dev)
    out = render_path_baked(scene.baked, CAM, TS, scene.homos, H, W, spec, quad_keep=scene.sparse, cull_scratch=scratch)
    masks = scratch[:need // 8].view(3, TILES, 2).cpu()
    assert bool((scratch[need // 8:] == -1).all())                      # nothing written past [C][tiles][2]
    assert bool((masks[..., 1] == 0).all())                             # D = 4: the second word is empty
    assert bool(((masks[..., 0] >> 2) & 1 == 0).all())                  # plane 2 keeps nothing: bit 2 is clear in every mask
    assert bool(((masks[..., 0] & ~0xF) == 0).all()) and int((masks[..., 0] != 0).sum()) > 0
    differ = [(a, b) for a in range(3) for b in range(a + 1, 3) if not torch.equal(masks[a], masks[b])]
    print(f"[{layout}] plane masks per camera and tile: {masks[..., 0].tolist()}; cameras with different plans: {differ}")
    assert len(differ) >= 1
    ref = scene.ref_sparse[layout]
    _assert_bit_equal(out, lambda i: ref[i])
    assert float((out[1] > 0).float().mean()) > 0.02


# ---- 4. refusals, nothing launched ---------------------------------------------------------------------------------------------------------
def test_refusals(dev, scene):
    from videoloop3d_amd.render import render_path_baked, render_path_baked_pool
    spec, qk = scene.specs["shared"], scene.keep
    SENT = 123.0
    buf = (torch.full((N, H, W, 3), SENT, device=dev), torch.full((N, H, W), SENT, device=dev))

    def call(cam=CAM, ts=TS, homos=scene.homos, baked=scene.baked, out=buf, **kw):
        return render_path_baked(baked, cam, ts, homos, H, W, spec, out=out, quad_keep=qk, **kw)
    with pytest.raises(IndexError, match="frame index"):
        call(ts=TS[:-1] + [T])
    with pytest.raises(IndexError, match="frame index"):
        call(ts=[-1] + TS[1:])
    with pytest.raises(IndexError, match="camera index"):
        call(cam=CAM[:-1] + [3])
    with pytest.raises(IndexError, match="camera index"):
        call(cam=[-1] + CAM[1:])
    with pytest.raises(RuntimeError, match="same output frames"):
        call(cam=CAM[:-1])
    with pytest.raises(RuntimeError, match="empty path"):
        call(cam=[], ts=[])
    with pytest.raises(RuntimeError, match=r"\[C,D,3,3\]"):
        call(homos=scene.homos[0])
    with pytest.raises(RuntimeError, match=r"\[C,D,3,3\]"):
        call(homos=scene.homos[:, :3])
    with pytest.raises(RuntimeError, match="`out`"):
        call(out=(buf[0][:N - 1], buf[1][:N - 1]))
    with pytest.raises(RuntimeError, match="cull_scratch"):
        call(cull_scratch=torch.zeros(3 * TILES * 2 - 1, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="cull_scratch"):
        call(cull_scratch=torch.zeros(3 * TILES * 4, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="cull_scratch"):
        call(cull_scratch=torch.zeros(3 * TILES * 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no backward"):
        with torch.enable_grad():
            call(homos=scene.homos.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(baked=scene.baked.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(homos=scene.homos.cpu())
    with pytest.raises(RuntimeError, match="uint8"):
        call(baked=scene.baked.float())
    # the pool wrapper shares the index and scratch checks
    g = BM.GEOMS["shared"]
    from videoloop3d_amd.packed import PackedLayout
    keep = synth.hash_uniform((D, g["QH"], g["QW"]), seed=11) < 0.5
    lay = PackedLayout(keep.to(dev), torch.zeros_like(keep).to(dev), BM.T_MODEL, g["Hs"], g["Ws"], g["tile"])
    pool = torch.zeros((lay.n_slots * 64, 4), dtype=torch.uint8, device=dev)
    kw = dict(out=buf, quad_keep=keep.to(torch.uint8).to(dev), culled_rgba8=0)
    with pytest.raises(IndexError, match="frame index"):
        render_path_baked_pool(lay, pool, CAM, TS[:-1] + [BM.T_MODEL], scene.homos, H, W, BM.pool_spec(g), **kw)
    with pytest.raises(IndexError, match="camera index"):
        render_path_baked_pool(lay, pool, CAM[:-1] + [3], TS, scene.homos, H, W, BM.pool_spec(g), **kw)
    with pytest.raises(RuntimeError, match="cull_scratch"):
        render_path_baked_pool(lay, pool, CAM, TS, scene.homos, H, W, BM.pool_spec(g), cull_scratch=torch.zeros(1, dtype=torch.int64, device=dev), **kw)
    with pytest.raises(RuntimeError, match="quad map"):
        render_path_baked_pool(lay, pool, CAM, TS, scene.homos, H, W, BM.pool_spec(g), out=buf, quad_keep=None, culled_rgba8=0)
    torch.cuda.synchronize()
    assert bool((buf[0] == SENT).all()) and bool((buf[1] == SENT).all())      # nothing was launched


# ---- 5. render_frames(baked=) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mpv", "pool"])
def test_render_frames_takes_the_path_render(dev, kind, monkeypatch):
    """the tiny sparsified tile-exact MPMeshVid of tests/test_gpu_baked.py along a 7-pose path with t = i % T: the uint8 frames equal to8b of
    baked.render called frame by frame (0 levels), through ONE path call per chunk; a fixed view makes no path call."""
    from videoloop3d_amd import render as R
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd.baked import bake, bake_pool
    if kind == "mpv":
        model, Hm, Wm, K = BM.tile_exact_model(dev, "0.2#0.4#0.6")
        baked, name = bake(model), "render_path_baked"
    else:
        model, Hm, Wm, K = BM.pool_model(dev, "0.2#0.4#0.6", True)
        baked, name = bake_pool(model), "render_path_baked_pool"
    Tm = baked.frm_num
    n = 7
    ext = np.tile(np.eye(4, dtype=np.float32)[None], (n, 1, 1))
    for i in range(n):
        ext[i, :3, 3] = [0.03 * np.cos(i), 0.02 * np.sin(i), 0.004 * i]
    intr = np.tile(K.astype(np.float32)[None], (n, 1, 1))
    rt = np.arange(n) % Tm
    assert rt.tolist() == [0, 1, 2, 3, 4, 5, 0]
    calls = []
    real = getattr(R, name)

    def spy(*a, **kw):
        calls.append(len(a[2] if kind == "mpv" else a[3]))      # frame_t
        return real(*a, **kw)
    monkeypatch.setattr(R, name, spy)
    want = torch.cat([RV.to8b(baked.render(Hm, Wm, torch.tensor(ext[i:i + 1]), torch.tensor(intr[i:i + 1]), torch.tensor(rt[i:i + 1]))[0].permute(0, 2, 3, 1))
                      for i in range(n)])
    assert calls == []
    frames = RV.render_frames(model, Hm, Wm, ext, intr, rt, baked=baked)
    assert frames.shape == (n, Hm, Wm, 3) and frames.dtype == torch.uint8
    worst = int((frames.int() - want.int()).abs().max())
    print(f"[{kind}] render_frames(baked=) along the path vs to8b(baked.render) frame by frame: max |level diff| {worst}; path calls {calls}")
    assert worst == 0 and float(frames.float().std()) > 1.0
    assert calls == [n]                                                  # one chunk, one path call
    del calls[:]
    chunked = RV.render_frames(model, Hm, Wm, ext, intr, rt, max_batch=3, baked=baked)
    assert torch.equal(chunked, frames) and calls == [3, 3]              # chunks of 3, 3 and 1 frames: the last one is a run of one frame
    # baked.render_path: the same frames before the 8-bit conversion
    del calls[:]
    r, a = baked.render_path(Hm, Wm, ext, intr, rt)
    assert r.shape == (n, 3, Hm, Wm) and a.shape == (n, Hm, Wm) and calls == [n]
    assert torch.equal(RV.to8b(r.permute(0, 2, 3, 1)), frames)
    # a fixed view (v = 'r1'): one run, the frame-pair call, no path call
    del calls[:]
    vp, vi, vt = RV.select_views_times(ext, intr, ext, intr, Tm, v="r1")
    fixed = RV.render_frames(model, Hm, Wm, vp, vi, vt, baked=baked)
    assert fixed.shape == (Tm, Hm, Wm, 3) and calls == []
    assert torch.equal(fixed[0], frames[0]) is False and torch.equal(fixed[1], frames[1])      # pose 1 shows frame 1 in both
