"""Fractional loop time of the baked playback model on the MI355X (render.render_times_baked / render_times_baked_pool; vl3d_baked_times of
vl3d_render_fwd_baked_times / _pool_times): a camera path whose output frames carry a real-valued time tau in [0, T).  The model at tau is the
linear interpolation of its TEXELS between frame t0 = floor(tau) and frame t1 = t0 + 1, which wraps to frame 0 at the loop seam, by f = tau - t0.

Two statements are exact and compared with torch.equal: a frame at an integer time has the bits of the path frame (cam, t0), and storage that
holds the same taps in both frames ignores f.  The blend itself is compared with the FLOAT kernels on the interpolated texels: interpolating
the decoded texels first and filtering them bilinearly afterwards (the oracle) and filtering both frames and interpolating the results (the
kernel) are the same real number; in fp32 the two orders differ by rounding only -- 3.0e-7 at most in an emulation of both orders (D = 4,
4e5 random samples) --, far inside the 1e-5 bound tests/test_gpu_baked.py uses for the same kernel pair.  Every test prints its measured maximum
(docs/kernels/K9_baked_playback.md, "Fractional loop time", records it).

Shapes of tests/baked_models.py: D = 4, a clip of 5 frames, planes of 40 x 72 texels, output 37 x 70 (2 x 5 workgroups of 64 x 8, a ragged edge,
hard cuts inside the view), the layouts dense / shared / exact, the two pool geometries, the three cameras of tests/test_gpu_baked_path.py.
The mixed path: N = 7, (cam, tau) = (0, 1.0), (1, 1.5), (2, 4.25), (0, 0.0), (1, 3.75), (1, 4.0), (2, 2.125) -- integer times, the seam
(4 -> 0), the first and the last frame, fractions exact in fp32."""
import types

import numpy as np
import pytest
import torch

import baked_models as BM
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu

D, T, H, W = BM.D, BM.T_ALLOC, BM.H, BM.W
INT_PATH = [(0, 1), (1, 1), (2, 4), (0, 0), (1, 3), (1, 4), (2, 2)]      # the path of tests/test_gpu_baked_path.py
ICAM, ITS = [c for c, _ in INT_PATH], [t for _, t in INT_PATH]
MIX = [(0, 1.0), (1, 1.5), (2, 4.25), (0, 0.0), (1, 3.75), (1, 4.0), (2, 2.125)]
CAM, TAU = [c for c, _ in MIX], [t for _, t in MIX]
N = len(MIX)
BOUND = 1e-5
BG = (0.2, 0.4, 0.6)
CULLED = 7 | 11 << 8 | 13 << 16 | 0 << 24


def _t0_t1_f(tau, n_t=T):
    t0 = int(np.floor(tau))
    return t0, (t0 + 1 if t0 + 1 < n_t else 0), float(np.float32(tau) - np.float32(t0))


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _homographies():
    """[3,D,3,3] target pixel -> plane pixel of the three cameras of tests/test_gpu_baked_path.py (near 1, far 100)."""
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


def _pool_scene(dev, geom, dynamic=True, T_layout=BM.T_MODEL):
    """the pool of tests/test_gpu_baked_path.py: hash-random texels behind the block table, static / dynamic / unstored blocks"""
    from videoloop3d_amd.baked import bake_texels
    from videoloop3d_amd.packed import PackedLayout
    g = BM.GEOMS[geom]
    keep = synth.hash_uniform((D, g["QH"], g["QW"]), seed=11) < 0.5
    keep[2] = False
    dyn = keep & (synth.hash_uniform((D, g["QH"], g["QW"]), seed=12) < 1.0 / 3.0) if dynamic else torch.zeros_like(keep)
    lay = PackedLayout(keep.to(dev), dyn.to(dev), T_layout, g["Hs"], g["Ws"], g["tile"])
    clip = bake_texels(synth.make_plane_stack(D, T_layout, g["Hs"], g["Ws"], seed=7, device=dev, alpha_bias=-0.5), "sigmoid", "sigmoid")
    pool = BM.scatter_pool(lay, clip, torch.zeros((1, 4), dtype=torch.uint8, device=dev))
    return types.SimpleNamespace(g=g, lay=lay, pool=pool, spec=BM.pool_spec(g), qk=keep.to(torch.uint8).to(dev),
                                 kw=dict(quad_keep=keep.to(torch.uint8).to(dev), culled_rgba8=CULLED))


@pytest.fixture(scope="module")
def scene(dev):
    """the baked clip and quad map of tests/test_gpu_baked_path.py, the three cameras' homographies, the two pools, and per layout the mixed
    path's float render -- computed once and never modified"""
    from videoloop3d_amd.baked import bake_texels
    from videoloop3d_amd.render import render_times_baked
    baked = bake_texels(synth.make_plane_stack(D, T, BM.HS, BM.WS, seed=7, device=dev, alpha_bias=-0.5), "sigmoid", "sigmoid")
    keep = synth.hash_uniform((D, BM.QH, BM.QW), seed=11) < 0.5
    keep[2] = False
    keep = keep.to(torch.uint8).to(dev)
    homos = _homographies().to(dev)
    specs = BM.specs()
    qk = {"dense": None, "shared": keep, "exact": keep}
    mix = {layout: tuple(x.clone() for x in render_times_baked(baked, CAM, TAU, homos, H, W, specs[layout], quad_keep=qk[layout])) for layout in specs}
    pools = {geom: _pool_scene(dev, geom) for geom in BM.GEOMS}
    for p in pools.values():
        e = p.lay.blocks
        assert int((e < 0).sum()) > 0 and int(((e >= 0) & ((e & 1) == 0)).sum()) > 0 and int(((e >= 0) & ((e & 1) == 1)).sum()) > 0
    return types.SimpleNamespace(baked=baked, qk=qk, homos=homos, specs=specs, mix=mix, pools=pools)


def _oracle(clip, cam, t0, t1, f, homos, spec, qk):
    """the float kernels on the interpolated texels: decoded = u8 / 255, s = decoded[t0] + f (decoded[t1] - decoded[t0]) as a one-frame stack"""
    from videoloop3d_amd.render import render_frame_run
    decoded = clip.float() / 255
    s = (decoded[:, t0] + f * (decoded[:, t1] - decoded[:, t0]))[:, None].contiguous()
    rgb, alpha = render_frame_run(s, 0, 1, homos[cam], H, W, spec, quad_keep=qk)
    return rgb[0], alpha[0]


def _against_oracle(tag, out, clip, homos, spec, qk, n_t=T):
    """every pixel of every frame of the mixed path against the oracle, none excluded -> the worst (d rgb, d alpha)"""
    worst = [0.0, 0.0]
    for i, (cam, tau) in enumerate(MIX):
        r, a = _oracle(clip, cam, *_t0_t1_f(tau, n_t), homos, spec, qk)
        dr, da = float((out[0][i] - r).abs().max()), float((out[1][i] - a).abs().max())
        print(f"  [{tag}] frame {i} (cam {cam}, tau {tau}): max |d rgb| {dr:.3e}, max |d alpha| {da:.3e}")
        worst = [max(worst[0], dr), max(worst[1], da)]
        assert dr <= BOUND and da <= BOUND, (tag, i, dr, da)
    print(f"[{tag}] the times render against the float kernels on interpolated texels: max |d rgb| {worst[0]:.3e}, max |d alpha| {worst[1]:.3e} "
          f"(bound {BOUND:.0e})")
    return worst


# ---- 1. integer times are today's frames ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "shared", "exact"])
def test_integer_times_are_the_path_frames(dev, scene, layout):
    from videoloop3d_amd.render import render_frame_run_baked, render_path_baked, render_times_baked
    spec, qk = scene.specs[layout], scene.qk[layout]
    want = render_path_baked(scene.baked, ICAM, ITS, scene.homos, H, W, spec, quad_keep=qk)
    got = render_times_baked(scene.baked, ICAM, [float(t) for t in ITS], scene.homos, H, W, spec, quad_keep=qk)
    assert got[0].shape == (N, H, W, 3) and got[1].shape == (N, H, W) and got[0].dtype == got[1].dtype == torch.float32
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert 0.3 < float((got[1] > 0).float().mean()) < 1.0
    # numpy times (float64) and caller-owned buffers: the same bits
    buf = (torch.full((N, H, W, 3), 123.0, device=dev), torch.full((N, H, W), 123.0, device=dev))
    again = render_times_baked(scene.baked, np.array(ICAM), np.array(ITS, dtype=np.float64), scene.homos, H, W, spec, out=buf, quad_keep=qk)
    assert again[0] is buf[0] and torch.equal(buf[0], want[0]) and torch.equal(buf[1], want[1])
    for C in (3, 4):
        for bg in (None, BG):
            w8 = render_path_baked(scene.baked, ICAM, ITS, scene.homos, H, W, spec, quad_keep=qk, frames8=torch.zeros((N, H, W, C), dtype=torch.uint8, device=dev), bg=bg)
            g8 = render_times_baked(scene.baked, ICAM, [float(t) for t in ITS], scene.homos, H, W, spec, quad_keep=qk,
                                    frames8=torch.full((N, H, W, C), 0xAB, dtype=torch.uint8, device=dev), bg=bg)
            assert torch.equal(g8, w8), (layout, C, bg)
    # the mixed path: its frames at integer times (0: t = 1, 3: t = 0, 5: t = 4) equal their one-frame renders
    mix = scene.mix[layout]
    for i in (0, 3, 5):
        assert float(TAU[i]) == int(TAU[i])
        r1, a1 = render_frame_run_baked(scene.baked, int(TAU[i]), 1, scene.homos[CAM[i]], H, W, spec, quad_keep=qk)
        assert torch.equal(mix[0][i], r1[0]) and torch.equal(mix[1][i], a1[0]), (layout, i)


@pytest.mark.parametrize("geom", list(BM.GEOMS))
def test_integer_times_are_the_pool_path_frames(dev, scene, geom):
    from videoloop3d_amd.render import render_path_baked_pool, render_times_baked_pool
    p = scene.pools[geom]
    want = render_path_baked_pool(p.lay, p.pool, ICAM, ITS, scene.homos, H, W, p.spec, **p.kw)
    got = render_times_baked_pool(p.lay, p.pool, ICAM, [float(t) for t in ITS], scene.homos, H, W, p.spec, **p.kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert 0.3 < float((got[1] > 0).float().mean()) < 1.0
    for C in (3, 4):
        for bg in (None, BG):
            w8 = render_path_baked_pool(p.lay, p.pool, ICAM, ITS, scene.homos, H, W, p.spec, frames8=torch.zeros((N, H, W, C), dtype=torch.uint8, device=dev), bg=bg, **p.kw)
            g8 = render_times_baked_pool(p.lay, p.pool, ICAM, [float(t) for t in ITS], scene.homos, H, W, p.spec,
                                         frames8=torch.full((N, H, W, C), 0xAB, dtype=torch.uint8, device=dev), bg=bg, **p.kw)
            assert torch.equal(g8, w8), (geom, C, bg)


# ---- 2. the blend, against the float kernels; 3. the seam ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["dense", "shared", "exact"])
def test_the_blend_equals_the_float_render_of_interpolated_texels(dev, scene, layout):
    from videoloop3d_amd.render import render_frame_run_baked
    spec, qk, out = scene.specs[layout], scene.qk[layout], scene.mix[layout]
    _against_oracle(layout, out, scene.baked, scene.homos, spec, qk)
    covered = float((out[1] > 0).float().mean())
    assert 0.3 < covered < 1.0, covered
    # not trivial: frame 1 (cam 1, tau 1.5) is not the whole frame 1 of its camera
    r1, a1 = render_frame_run_baked(scene.baked, 1, 1, scene.homos[1], H, W, spec, quad_keep=qk)
    d_whole = float((out[0][1] - r1[0]).abs().max())
    # the seam: frame 2 (cam 2, tau 4.25) blends frame 4 with frame 0 -- it passed the comparison above with t1 = 0 --, not with frame 3, and
    # is not the whole frame 4
    assert _t0_t1_f(4.25) == (4, 0, 0.25)
    r3, a3 = _oracle(scene.baked, 2, 4, 3, 0.25, scene.homos, spec, qk)
    r4, a4 = render_frame_run_baked(scene.baked, 4, 1, scene.homos[2], H, W, spec, quad_keep=qk)
    d_mirror, d_last = float((out[0][2] - r3).abs().max()), float((out[0][2] - r4[0]).abs().max())
    print(f"[{layout}] covered {covered:.3f}; tau 1.5 vs whole frame 1: {d_whole:.3e}; tau 4.25 vs the blend with t1 = 3: {d_mirror:.3e}, vs whole frame 4: {d_last:.3e}")
    assert d_whole > 1e-3 and d_mirror > 1e-3 and d_last > 1e-3


# ---- 4. the pool equals the clip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(BM.GEOMS))
def test_the_pool_equals_the_clip_of_its_unpacked_frames(dev, scene, geom):
    from videoloop3d_amd.baked import BakedPool
    from videoloop3d_amd.render import render_times_baked, render_times_baked_pool
    p = scene.pools[geom]
    got = render_times_baked_pool(p.lay, p.pool, CAM, TAU, scene.homos, H, W, p.spec, **p.kw)
    clip = BakedPool(p.pool, p.lay, p.qk, p.spec, "", None, CULLED).unpack_frames(range(BM.T_MODEL))
    want = render_times_baked(clip, CAM, TAU, scene.homos, H, W, p.spec, quad_keep=p.qk)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert 0.3 < float((got[1] > 0).float().mean()) < 1.0
    assert float((got[0][1] - got[0][4]).abs().max()) > 0.05              # camera 1 at 1.5 and at 3.75: the dynamic blocks move
    _against_oracle("pool " + geom, got, clip, scene.homos, p.spec, p.qk, BM.T_MODEL)


# ---- 5. static storage ignores the fraction ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(BM.GEOMS))
def test_static_storage_ignores_the_fraction(dev, scene, geom):
    from videoloop3d_amd.render import render_path_baked_pool, render_times_baked_pool
    p = _pool_scene(dev, geom, dynamic=False)
    e = p.lay.blocks
    assert int(((e >= 0) & ((e & 1) == 1)).sum()) == 0 and int((e >= 0).sum()) > 0
    got = render_times_baked_pool(p.lay, p.pool, CAM, TAU, scene.homos, H, W, p.spec, **p.kw)
    want = render_path_baked_pool(p.lay, p.pool, CAM, [int(t) for t in TAU], scene.homos, H, W, p.spec, **p.kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert 0.3 < float((got[1] > 0).float().mean()) < 1.0


# ---- 6. the display sink ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["clip", "pool"])
def test_the_display_sink_stores_the_display_bytes(dev, scene, source, monkeypatch):
    from videoloop3d_amd.baked import display_frames
    from videoloop3d_amd.render import render_times_baked, render_times_baked_pool
    if source == "clip":
        def call(**o):
            return render_times_baked(scene.baked, CAM, TAU, scene.homos, H, W, scene.specs["shared"], quad_keep=scene.qk["shared"], **o)
    else:
        p = scene.pools["exact"]

        def call(**o):
            return render_times_baked_pool(p.lay, p.pool, CAM, TAU, scene.homos, H, W, p.spec, **p.kw, **o)
    rgb, alpha = call()
    assert float(display_frames(rgb, alpha, None, 3).float().std()) > 1.0
    for C in (3, 4):
        for bg in (None, BG):
            want = display_frames(rgb, alpha, bg, C)
            for store in (("packed", "bytes") if C == 3 else ("packed",)):
                monkeypatch.setenv("VL3D_DISPLAY_STORE3", store)
                buf = torch.full((N, H, W, C), 0xAB, dtype=torch.uint8, device=dev)
                got = call(frames8=buf, bg=bg)
                assert got is buf and torch.equal(got, want), (source, C, bg, store, int((got != want).sum()))


# ---- 7. the kernel's own guard ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["clip", "pool"])
def test_times_outside_the_loop_are_left_unwritten(dev, scene, source):
    """the C entries with a time array of our own, behind the wrapper's check: [1.5, nan, -0.5, 5.0, 2.0] with T = 5.  The storage is larger
    than the entry is told -- T + 2 frames per plane behind the clip's texels, a pool laid out for 7 frames -- so that a kernel without the
    guard would still read only allocated memory for each of these values.  Frames 1, 2, 3 keep the sentinel in every element; frames 0 and 4
    hold what a call with valid times gives."""
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd import render as R
    lib, stream, SENT, n = L.lib(), L.stream_ptr(dev), 123.0, 5
    times_bad = [1.5, float("nan"), -0.5, 5.0, 2.0]
    times_ok = [1.5, 0.0, 0.0, 0.0, 2.0]
    if source == "clip":
        spec, qk, g = scene.specs["shared"], scene.qk["shared"], dict(Hs=BM.HS, Ws=BM.WS)
        store = torch.zeros((D * (T + 2), BM.HS, BM.WS, 4), dtype=torch.uint8, device=dev)      # the clip's D * T frames, then 2 D frames of slack
        store[:D * T] = scene.baked.view(D * T, BM.HS, BM.WS, 4)
    else:
        p = _pool_scene(dev, "shared", T_layout=T + 2)
        spec, qk, g = p.spec, p.qk, p.g
    d = R._desc_dims(D, n, g["Hs"], g["Ws"], H, W, spec, L.STACK_DTYPE["u8"])
    cull = torch.zeros(int(lib.vl3d_render_path_cull_scratch_bytes(d, 3)) // 8, dtype=torch.int64, device=dev)
    grid = R._qgrid(qk, spec)

    def call(times):
        cams = torch.zeros(n, dtype=torch.int32, device=dev)
        tt = torch.tensor(times, dtype=torch.float32, device=dev)
        rgb, alpha = torch.full((n, H, W, 3), SENT, device=dev), torch.full((n, H, W), SENT, device=dev)
        sel, sink = L.BakedTimes(n_cams=3, frame_cam=cams.data_ptr(), frame_time=tt.data_ptr()), BM.float_out(rgb, alpha)
        if source == "clip":
            rc = lib.vl3d_render_fwd_baked_times(d, L.ptr(store), T, L.ptr(scene.homos), sel, L.ptr(qk), *grid, L.ptr(cull), sink, stream)
        else:
            rc = lib.vl3d_render_fwd_baked_pool_times(d, L.ptr(p.lay.blocks), L.ptr(p.pool), T, L.ptr(scene.homos), sel, L.ptr(qk), *grid, CULLED,
                                                      L.ptr(cull), sink, stream)
        assert rc == 0, lib.vl3d_last_error()
        torch.cuda.synchronize()
        return rgb, alpha
    want, got = call(times_ok), call(times_bad)
    assert not bool((want[0] == SENT).any()) and not bool((want[1] == SENT).any())
    for i in (1, 2, 3):
        assert bool((got[0][i] == SENT).all()) and bool((got[1][i] == SENT).all()), i
    for i in (0, 4):
        assert torch.equal(got[0][i], want[0][i]) and torch.equal(got[1][i], want[1][i]), i
    if source == "clip":      # (the clip the entry saw is the scene's: frame 0 of the call is the wrapper's render of (cam 0, 1.5))
        ref = R.render_times_baked(scene.baked, [0], [1.5], scene.homos, H, W, spec, quad_keep=qk)
        assert torch.equal(want[0][0], ref[0][0]) and torch.equal(want[1][0], ref[1][0])


# ---- 8. host refusals, nothing launched ------------------------------------------------------------------------------------------------------
def test_refusals(dev, scene):
    from videoloop3d_amd.render import render_times_baked, render_times_baked_pool
    spec, qk = scene.specs["shared"], scene.qk["shared"]
    SENT = 123.0
    buf = (torch.full((N, H, W, 3), SENT, device=dev), torch.full((N, H, W), SENT, device=dev))
    buf8 = torch.full((N, H, W, 3), 0xAB, dtype=torch.uint8, device=dev)

    def call(cam=CAM, tau=TAU, homos=scene.homos, baked=scene.baked, out=buf, **kw):
        return render_times_baked(baked, cam, tau, homos, H, W, spec, out=out, quad_keep=qk, **kw)
    with pytest.raises(ValueError, match="loop time"):
        call(tau=TAU[:-1] + [float(T)])
    with pytest.raises(ValueError, match="loop time"):
        call(tau=[-0.25] + TAU[1:])
    with pytest.raises(ValueError, match="finite"):
        call(tau=TAU[:3] + [float("nan")] + TAU[4:])
    with pytest.raises(ValueError, match="finite"):
        call(tau=TAU[:3] + [float("inf")] + TAU[4:])
    with pytest.raises(ValueError, match="loop time"):
        call(tau=TAU[:-1] + [np.nextafter(np.float64(T), 0)])      # below T in float64, T as float32
    with pytest.raises(RuntimeError, match="same output frames"):
        call(cam=CAM[:-1])
    with pytest.raises(RuntimeError, match="empty path"):
        call(cam=[], tau=[])
    with pytest.raises(RuntimeError, match=r"\[C,D,3,3\]"):
        call(homos=scene.homos[0])
    with pytest.raises(RuntimeError, match=r"\[C,D,3,3\]"):
        call(homos=scene.homos[:, :3])
    with pytest.raises(IndexError, match="camera index"):
        call(cam=CAM[:-1] + [3])
    with pytest.raises(IndexError, match="camera index"):
        call(cam=[-1] + CAM[1:])
    with pytest.raises(RuntimeError, match="`out`"):
        call(out=(buf[0][:N - 1], buf[1][:N - 1]))
    with pytest.raises(RuntimeError, match="frames8"):
        call(out=None, frames8=buf8[:N - 1])
    with pytest.raises(ValueError, match="two different outputs"):
        call(frames8=buf8)
    with pytest.raises(ValueError, match="`bg`"):
        call(bg=BG)
    with pytest.raises(RuntimeError, match="cull_scratch"):
        call(cull_scratch=torch.zeros(1, dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(baked=scene.baked.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(homos=scene.homos.cpu())
    # the pool wrapper shares the checks
    p = scene.pools["shared"]
    with pytest.raises(ValueError, match="loop time"):
        render_times_baked_pool(p.lay, p.pool, CAM, TAU[:-1] + [float(BM.T_MODEL)], scene.homos, H, W, p.spec, out=buf, **p.kw)
    with pytest.raises(ValueError, match="finite"):
        render_times_baked_pool(p.lay, p.pool, CAM, [float("nan")] + TAU[1:], scene.homos, H, W, p.spec, out=buf, **p.kw)
    with pytest.raises(IndexError, match="camera index"):
        render_times_baked_pool(p.lay, p.pool, CAM[:-1] + [3], TAU, scene.homos, H, W, p.spec, out=buf, **p.kw)
    with pytest.raises(RuntimeError, match="same output frames"):
        render_times_baked_pool(p.lay, p.pool, CAM, TAU[:-1], scene.homos, H, W, p.spec, out=buf, **p.kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        render_times_baked_pool(p.lay, p.pool.cpu(), CAM, TAU, scene.homos, H, W, p.spec, out=buf, **p.kw)
    with pytest.raises(RuntimeError, match="quad map"):
        render_times_baked_pool(p.lay, p.pool, CAM, TAU, scene.homos, H, W, p.spec, out=buf, quad_keep=None, culled_rgba8=0)
    torch.cuda.synchronize()
    assert bool((buf[0] == SENT).all()) and bool((buf[1] == SENT).all()) and bool((buf8 == 0xAB).all())      # nothing was launched


# ---- 9. the modules end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mpv", "pool"])
def test_modules_play_loop_times(dev, kind):
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd.baked import bake, bake_pool, display_frames
    if kind == "mpv":
        model, Hm, Wm, K = BM.tile_exact_model(dev, "0.2#0.4#0.6")
        baked = bake(model)
    else:
        model, Hm, Wm, K = BM.pool_model(dev, "0.2#0.4#0.6", True)
        baked = bake_pool(model)
    Tm, n = baked.frm_num, 9
    ext = np.tile(np.eye(4, dtype=np.float32)[None], (n, 1, 1))
    for i in range(n):
        ext[i, :3, 3] = [0.03 * np.cos(i), 0.02 * np.sin(i), 0.004 * i]
    intr = np.tile(K.astype(np.float32)[None], (n, 1, 1))
    ts = RV.retime(n, 60, 25)
    assert float(ts.max()) < Tm and not np.array_equal(ts, np.floor(ts))
    frames = baked.render_display(Hm, Wm, ext, intr, ts, fractional=True)
    assert frames.shape == (n, Hm, Wm, 3) and frames.dtype == torch.uint8 and float(frames.float().std()) > 1.0
    r, a = baked.render_path(Hm, Wm, ext, intr, ts, fractional=True)
    assert r.shape == (n, 3, Hm, Wm) and a.shape == (n, Hm, Wm)
    assert torch.equal(frames, display_frames(r.permute(0, 2, 3, 1), a, None, 3))      # (render_path composites over the background itself)
    rgba = baked.render_display(Hm, Wm, ext, intr, ts, channels=4, fractional=True)
    assert torch.equal(rgba[..., :3], frames) and torch.equal(rgba[..., 3], display_frames(r.permute(0, 2, 3, 1), a, None, 4)[..., 3])
    # the loop has no first frame: -0.25 is T - 0.25, and a time is its own reduction a whole number of loops later
    one = lambda t: baked.render_display(Hm, Wm, ext[:1], intr[:1], t, fractional=True)      # noqa: E731
    assert torch.equal(one([-0.25]), one([Tm - 0.25]))
    assert torch.equal(one([Tm - 0.25]), one([3 * Tm - 0.25])) and not torch.equal(one([Tm - 0.25]), one([Tm - 1.0]))
    assert torch.equal(one([float(Tm)]), baked.render_display(Hm, Wm, ext[:1], intr[:1], [0]))          # t = T is frame 0, not an IndexError
    # chunks of 4, 4 and 1 frames: the bytes of one chunk
    assert torch.equal(baked.render_display(Hm, Wm, ext, intr, ts, max_batch=4, fractional=True), frames)
    # without `fractional` the same times are truncated, as before
    trunc = baked.render_display(Hm, Wm, ext, intr, ts)
    assert torch.equal(trunc, baked.render_display(Hm, Wm, ext, intr, [int(t) for t in ts]))
    assert not torch.equal(trunc, frames)
    with pytest.raises(IndexError):
        baked.render_display(Hm, Wm, ext[:1], intr[:1], [float(Tm)])
    # render_frames passes it on
    assert torch.equal(RV.render_frames(model, Hm, Wm, ext, intr, ts, baked=baked, fractional=True), frames)
    assert torch.equal(RV.render_frames(model, Hm, Wm, ext, intr, ts, max_batch=2, baked=baked, fractional=True), frames)
