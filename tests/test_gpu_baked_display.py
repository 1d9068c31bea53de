"""The display output of the baked playback model on the MI355X (the display sink of vl3d_render_fwd_baked / _pool: vl3d_baked_out.frames; `frames8=` of
render.render_frame_run_baked / _pool, render_path_baked / _pool; BakedMPV / BakedPool.render_display; render_frames(baked=)): the render
launches store the uint8 frame a viewer shows.  The yardstick in every case is the existing FLOAT entry followed by baked.display_frames -- the
torch statement the kernels' store replaces -- and the comparison is torch.equal on every byte, no pixel excluded.

Shapes: D = 5 planes, a clip of 6 frames; the dense clip on planes of 40 x 72 texels (5 x 9 quads of 8 x 8: dense, shared-border culled,
tile-exact culled), the pool on 5 x 7 tiles of 6 x 10 texels (30 x 70 texels, tiles straddling the 8 x 8 blocks).  Culled texels hold
(0, 0, 0, CULLED_ALPHA) and static quads the same texels in every frame.  Two output sizes: 11 x 70 -- two x-tiles with a 6-pixel second
tile, a partial y-tile, a row pitch of 210 bytes, so RGB8 rows start misaligned -- and 8 x 128 -- full tiles, aligned rows: the lane-packed
RGB8 store's dword branch runs.  Both RGB8 stores (VL3D_DISPLAY_STORE3) are compared."""
import dataclasses
import types

import numpy as np
import pytest
import torch

import baked_models as BM
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu

D, T_CLIP, F0 = 5, 6, 1
SIZES = {"11x70": (11, 70), "8x128": (8, 128)}
LAYOUTS = ["dense", "shared", "exact", "pool"]
GEOM = {"dense": dict(Hs=40, Ws=72, QH=5, QW=9, tile=None), "shared": dict(Hs=40, Ws=72, QH=5, QW=9, tile=None),
        "exact": dict(Hs=40, Ws=72, QH=5, QW=9, tile=(8, 8)), "pool": dict(Hs=30, Ws=70, QH=5, QW=7, tile=(6, 10))}
BGS = [None, (1.0, 1.0, 1.0), (2.0, -1.0, 0.5)]      # the last one makes both clamps bite
PATH = [(0, 1), (1, 1), (2, 4), (0, 0), (1, 3), (1, 4), (2, 2)]      # (camera, frame): a repeated camera, non-monotone frames
CAM, TS = [c for c, _ in PATH], [t for _, t in PATH]
N = len(PATH)
SENT = 0xAB


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _spec(g, W):
    """plane pixel -> texel (lattice point) of geometry g for a view W pixels wide: the 40 x 72-texel extent of tests/test_gpu_baked.py, the
    x scale shrunk for the wider view so that most of it stays covered; hard-cut edges remain inside the view"""
    from videoloop3d_amd.render import RenderSpec
    sc, off = (1.06 * 70.0 / W, 1.1), (-1.0, -0.5)
    if g["tile"] is None:
        return RenderSpec.mpv(rgb_act="none", alpha_act="none", scale=sc, offset=off)
    th, tw = g["tile"]
    lat = ((g["QW"] * (tw - 1)) / 71.0, (g["QH"] * (th - 1)) / 39.0)
    return dataclasses.replace(RenderSpec.mpv(rgb_act="none", alpha_act="none", scale=(sc[0] * lat[0], sc[1] * lat[1]),
                                              offset=(off[0] * lat[0], off[1] * lat[1])), tile=(th, tw))


def _homographies(H, W):
    """[3,D,3,3] of three cameras (tests/test_gpu_baked_path.py): the benchmark camera, the opposite translation, a shifted principal point"""
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


@pytest.fixture(scope="module")
def models(dev):
    """per layout: the baked clip (or pool) with its quad map, as run / path closures of the FLOAT entry and of the display entry"""
    from videoloop3d_amd import tiles
    from videoloop3d_amd.baked import bake_texels
    from videoloop3d_amd.packed import PackedLayout
    from videoloop3d_amd import render as R
    out = {}
    for name, g in GEOM.items():
        keep = synth.hash_uniform((D, g["QH"], g["QW"]), seed=11) < 0.5
        keep[2] = False
        dyn = keep & (synth.hash_uniform((D, g["QH"], g["QW"]), seed=12) < 1.0 / 3.0)
        stack = synth.make_plane_stack(D, T_CLIP, g["Hs"], g["Ws"], seed=7, alpha_bias=-0.5)
        if name != "dense":      # static quads: frame 0 in every frame; culled texels: (0, 0, 0, CULLED_ALPHA)
            stack = torch.where(tiles.quad_to_texel_mask(dyn, g["Hs"], g["Ws"], g["tile"])[:, None, :, :, None], stack, stack[:, :1])
            stack = torch.where(tiles.quad_to_texel_mask(keep, g["Hs"], g["Ws"], g["tile"])[:, None, :, :, None], stack,
                                torch.tensor([0.0, 0.0, 0.0, tiles.CULLED_ALPHA]))
        clip = bake_texels(stack.to(dev), "sigmoid", "sigmoid")
        qk = None if name == "dense" else keep.to(torch.uint8).to(dev)
        m = types.SimpleNamespace(g=g, qk=qk, clip=clip)
        if name == "pool":
            lay = PackedLayout(keep.to(dev), dyn.to(dev), T_CLIP, g["Hs"], g["Ws"], g["tile"])
            e = lay.blocks
            assert int((e < 0).sum()) > 0 and int(((e >= 0) & ((e & 1) == 0)).sum()) > 0 and int(((e >= 0) & ((e & 1) == 1)).sum()) > 0
            pool = BM.scatter_pool(lay, clip, torch.zeros((1, 4), dtype=torch.uint8, device=dev))
            kw = dict(quad_keep=qk, culled_rgba8=0)      # sigmoid(CULLED_ALPHA) bakes to alpha 0
            m.lay, m.pool = lay, pool
            m.run = lambda t0, n, homos, H, W, spec, kw=kw, lay=lay, pool=pool, **o: R.render_frame_run_baked_pool(lay, pool, t0, n, homos, H, W, spec, **kw, **o)
            m.path = lambda cam, ts, homos, H, W, spec, kw=kw, lay=lay, pool=pool, **o: R.render_path_baked_pool(lay, pool, cam, ts, homos, H, W, spec, **kw, **o)
        else:
            m.run = lambda t0, n, homos, H, W, spec, clip=clip, qk=qk, **o: R.render_frame_run_baked(clip, t0, n, homos, H, W, spec, quad_keep=qk, **o)
            m.path = lambda cam, ts, homos, H, W, spec, clip=clip, qk=qk, **o: R.render_path_baked(clip, cam, ts, homos, H, W, spec, quad_keep=qk, **o)
        out[name] = m
    return out


def _frames8(n, H, W, C, dev):
    return torch.full((n, H, W, C), SENT, dtype=torch.uint8, device=dev)


# ---- 1. runs -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("layout", LAYOUTS)
def test_runs_store_the_display_bytes(dev, models, layout, size, monkeypatch):
    from videoloop3d_amd.baked import display_frames
    m, (H, W) = models[layout], SIZES[size]
    spec, homos = _spec(m.g, W), _homographies(H, W)[0].to(dev)
    worst = 0
    for T in (1, 4, 5):      # a single frame, an even run, an odd tail
        rgb, alpha = m.run(F0, T, homos, H, W, spec)
        covered = float((alpha > 0).float().mean())
        assert covered > 0.2 and float(alpha.min()) < 0.999, covered      # the view is covered, and the background shows through
        for bg in BGS:
            for C in (3, 4):
                want = display_frames(rgb, alpha, bg, C)
                for store in (("packed", "bytes") if C == 3 else ("packed",)):
                    monkeypatch.setenv("VL3D_DISPLAY_STORE3", store)
                    buf = _frames8(T, H, W, C, dev)
                    got = m.run(F0, T, homos, H, W, spec, frames8=buf, bg=bg)
                    assert got is buf
                    diff = int((got.int() - want.int()).abs().max())
                    worst = max(worst, diff)
                    assert torch.equal(got, want), (layout, size, T, bg, C, store, diff, int((got != want).sum()))
        if T == 5:      # the case is not trivial: both clamps bite under the last background, and the frames differ
            x = rgb * alpha[..., None] + torch.tensor(BGS[2], device=dev) * (-alpha[..., None] + 1)
            assert bool((x > 1).any()) and bool((x < 0).any())
            assert float(display_frames(rgb, alpha, None, 3).float().std()) > 1.0
    print(f"[{layout} {size}] runs of 1 / 4 / 5 frames, 3 backgrounds, RGB8 (both stores) and RGBA8: max |level diff| {worst}")


# ---- 2. a camera path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("layout", ["dense", "shared", "pool"])
def test_path_stores_the_display_bytes(dev, models, layout, size, monkeypatch):
    from videoloop3d_amd.baked import display_frames
    m, (H, W) = models[layout], SIZES[size]
    spec, homos = _spec(m.g, W), _homographies(H, W).to(dev)
    rgb, alpha = m.path(CAM, TS, homos, H, W, spec)
    assert float((rgb[0] - rgb[1]).abs().max()) > 0.05                    # cameras 0 and 1 at the same frame differ
    for bg in (None, BGS[2]):
        for C in (3, 4):
            want = display_frames(rgb, alpha, bg, C)
            for store in (("packed", "bytes") if C == 3 else ("packed",)):
                monkeypatch.setenv("VL3D_DISPLAY_STORE3", store)
                got = m.path(CAM, TS, homos, H, W, spec, frames8=_frames8(N, H, W, C, dev), bg=bg)
                assert torch.equal(got, want), (layout, size, bg, C, store, int((got != want).sum()))
            # ... and equal to the display RUN call of each frame alone
            for i in range(N):
                one = m.run(TS[i], 1, homos[CAM[i]], H, W, spec, frames8=_frames8(1, H, W, C, dev), bg=bg)
                assert torch.equal(one[0], got[i]), (layout, size, bg, C, i)


# ---- 3. an index out of range behind the wrapper's check -----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["shared", "pool"])
def test_out_of_range_path_frames_are_left_unwritten(dev, models, layout):
    """the C entry with index arrays of our own: frame 2 names camera 3 of 3, frame 5 frame -1 of the clip.  Their workgroups return before
    any load or store -- the bytes keep the sentinel --, every other frame holds the bytes of the checked call."""
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd import render as R
    m, (H, W) = models[layout], SIZES["11x70"]
    g, spec, homos = m.g, _spec(m.g, W), _homographies(H, W).to(dev)
    bg = (0.2, 0.4, 0.6)
    want = m.path(CAM, TS, homos, H, W, spec, frames8=_frames8(N, H, W, 3, dev), bg=bg)
    cam, ts = list(CAM), list(TS)
    cam[2], ts[5] = 3, -1
    idx = torch.tensor([cam, ts], dtype=torch.int32).to(dev)
    d = R._desc_dims(D, N, g["Hs"], g["Ws"], H, W, spec, L.STACK_DTYPE["u8"])
    lib, stream = L.lib(), L.stream_ptr(dev)
    cull = torch.zeros(int(lib.vl3d_render_path_cull_scratch_bytes(d, 3)) // 8, dtype=torch.int64, device=dev)
    buf = _frames8(N, H, W, 3, dev)
    bgc = (L.C.c_float * 3)(*bg)
    grid = R._qgrid(m.qk, spec)
    sel, sink = BM.path_sel(3, idx), BM.display_out(buf, 3, bgc)
    if layout == "pool":
        rc = lib.vl3d_render_fwd_baked_pool(d, L.ptr(m.lay.blocks), L.ptr(m.pool), T_CLIP, L.ptr(homos), sel, L.ptr(m.qk), *grid, 0, L.ptr(cull), sink,
                                            stream)
    else:
        rc = lib.vl3d_render_fwd_baked(d, L.ptr(m.clip), T_CLIP, L.ptr(homos), sel, L.ptr(m.qk), *grid, L.ptr(cull), sink, stream)
    assert rc == 0, lib.vl3d_last_error()
    torch.cuda.synchronize()
    for i in range(N):
        if i in (2, 5):
            assert bool((buf[i] == SENT).all()), i
        else:
            assert torch.equal(buf[i], want[i]), i


# ---- 4. render_frames(baked=) --------------------------------------------------------------------------------------------------------------
class _CountingLib:
    """the loaded library with every call's symbol recorded -- and, for the two baked render entries, the sink the call names: (symbol,
    out.frames set, out.rgb or out.alpha set)"""

    def __init__(self, lib, calls):
        self._lib, self._calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            if name in ("vl3d_render_fwd_baked", "vl3d_render_fwd_baked_pool"):
                sink = a[-2]      # (..., const vl3d_baked_out *out, stream)
                self._calls.append((name, bool(sink.frames), bool(sink.rgb) or bool(sink.alpha)))
            else:
                self._calls.append((name,))
            return fn(*a)
        return counted


@pytest.mark.parametrize("kind", ["mpv", "pool"])
def test_render_frames_writes_display_frames_directly(dev, kind, monkeypatch):
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd.baked import bake, bake_pool, display_frames
    if kind == "mpv":
        model, Hm, Wm, K = BM.tile_exact_model(dev, "0.2#0.4#0.6")
        baked = bake(model)
    else:
        model, Hm, Wm, K = BM.pool_model(dev, "0.2#0.4#0.6", True)
        baked = bake_pool(model)
    Tm, n = baked.frm_num, 7
    ext = np.tile(np.eye(4, dtype=np.float32)[None], (n, 1, 1))
    for i in range(n):
        ext[i, :3, 3] = [0.03 * np.cos(i), 0.02 * np.sin(i), 0.004 * i]
    intr = np.tile(K.astype(np.float32)[None], (n, 1, 1))
    rt = np.arange(n) % Tm

    def per_frame(e, k, t):      # display_frames of the frames from baked.render (already over the background), pose by pose
        return torch.cat([display_frames(baked.render(Hm, Wm, torch.tensor(e[i:i + 1]), torch.tensor(k[i:i + 1]), torch.tensor(t[i:i + 1]))[0]
                                         .permute(0, 2, 3, 1), None, None, 3) for i in range(len(t))])
    want = per_frame(ext, intr, rt)
    vp, vi, vt = RV.select_views_times(ext, intr, ext, intr, Tm, v="r1")
    want_fixed = per_frame(vp, vi, vt)
    calls = []
    monkeypatch.setattr(L, "_lib", _CountingLib(L.lib(), calls))
    for name, (e, k, t, ref) in {"spiral": (ext, intr, rt, want), "fixed view": (vp, vi, vt, want_fixed)}.items():
        for max_batch in (64, 3):
            del calls[:]
            frames = RV.render_frames(model, Hm, Wm, e, k, t, max_batch=max_batch, baked=baked)
            assert frames.dtype == torch.uint8 and frames.shape == (len(t), Hm, Wm, 3)
            assert torch.equal(frames, ref), (name, max_batch, int((frames != ref).sum()))
            renders = [c for c in calls if c[0].startswith("vl3d_render_fwd")]
            print(f"[{kind}] {name}, chunks of {max_batch}: {renders}")
            # no float render on this route: every render call is a baked entry whose sink is out.frames, out.rgb and out.alpha NULL
            assert len(renders) >= 1 and all(len(c) == 3 and c[1] and not c[2] for c in renders)
    assert float(want.float().std()) > 1.0
    # render_display: RGBA8 and a caller's buffer
    rgba = baked.render_display(Hm, Wm, ext, intr, rt, channels=4)
    assert rgba.shape == (n, Hm, Wm, 4) and torch.equal(rgba[..., :3], want)
    a = torch.cat([baked.render(Hm, Wm, torch.tensor(ext[i:i + 1]), torch.tensor(intr[i:i + 1]), torch.tensor(rt[i:i + 1]))[1] for i in range(n)])
    assert torch.equal(rgba[..., 3], display_frames(a[..., None].expand(-1, -1, -1, 3), a, None, 4)[..., 3])


# ---- 5. refusals, nothing launched ---------------------------------------------------------------------------------------------------------
def test_refusals(dev, models):
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd import render as R
    from videoloop3d_amd.baked import BakedMPV
    H, W = SIZES["11x70"]
    lib, stream, EINVAL = L.lib(), L.stream_ptr(dev), 1
    homos = _homographies(H, W).to(dev)
    n = 3
    for layout in ("shared", "pool"):
        m = models[layout]
        spec = _spec(m.g, W)
        buf3, buf4 = _frames8(n, H, W, 3, dev), _frames8(n, H, W, 4, dev)
        with pytest.raises(RuntimeError, match="frames8"):                                   # channels = 2
            m.run(F0, n, homos[0], H, W, spec, frames8=_frames8(n, H, W, 2, dev))
        raw = torch.full((n * H * W * 4 + 4,), SENT, dtype=torch.uint8, device=dev)
        odd = raw[1:1 + n * H * W * 4].view(n, H, W, 4)
        assert odd.is_contiguous() and odd.data_ptr() % 4 == 1
        with pytest.raises(RuntimeError, match="4-byte aligned"):
            m.run(F0, n, homos[0], H, W, spec, frames8=odd)
        with pytest.raises(RuntimeError, match="4-byte aligned"):
            m.path(CAM[:n], TS[:n], homos, H, W, spec, frames8=odd)
        m.run(F0, n, homos[0], H, W, spec, frames8=raw[1:1 + n * H * W * 3].view(n, H, W, 3))      # RGB8 needs no alignment
        raw[1:1 + n * H * W * 3] = SENT
        with pytest.raises(ValueError, match="frames8"):                                     # out= with frames8=
            m.run(F0, n, homos[0], H, W, spec, out=(torch.empty((n, H, W, 3), device=dev), torch.empty((n, H, W), device=dev)), frames8=buf3)
        with pytest.raises(ValueError, match="frames8"):
            m.path(CAM[:n], TS[:n], homos, H, W, spec, out=(torch.empty((n, H, W, 3), device=dev), torch.empty((n, H, W), device=dev)), frames8=buf3)
        with pytest.raises(ValueError, match="frames8"):                                     # a background without display frames
            m.run(F0, n, homos[0], H, W, spec, bg=(1, 1, 1))
        with pytest.raises(RuntimeError, match="finite"):
            m.run(F0, n, homos[0], H, W, spec, frames8=buf3, bg=(0.5, float("nan"), 0.5))
        with pytest.raises(RuntimeError, match="finite"):
            m.path(CAM[:n], TS[:n], homos, H, W, spec, frames8=buf4, bg=(float("inf"), 0.0, 0.0))
        with pytest.raises(RuntimeError, match="3 floats"):
            m.run(F0, n, homos[0], H, W, spec, frames8=buf3, bg=(0.5, 0.5))
        with pytest.raises(RuntimeError, match="frames8"):
            m.run(F0, n, homos[0], H, W, spec, frames8=buf3.cpu())
        with pytest.raises(RuntimeError, match="frames8"):
            m.run(F0, n, homos[0], H, W, spec, frames8=buf3.float())
        with pytest.raises(RuntimeError, match="frames8"):
            m.run(F0, n - 1, homos[0], H, W, spec, frames8=buf3)
        # the C entries: channels, a null frames pointer, and the quad grids the float sink refuses, with the float sink's own messages
        g = m.g
        d = R._desc_dims(D, n, g["Hs"], g["Ws"], H, W, spec, L.STACK_DTYPE["u8"])
        QH, QW = R._qgrid(m.qk, spec)
        cull = torch.zeros(int(lib.vl3d_render_path_cull_scratch_bytes(d, 3)) // 8, dtype=torch.int64, device=dev)
        idx = torch.tensor([CAM[:n], TS[:n]], dtype=torch.int32).to(dev)
        rgb, alpha = torch.full((n, H, W, 3), 123.0, device=dev), torch.full((n, H, W), 123.0, device=dev)
        hom, qk, sc = L.ptr(homos), L.ptr(m.qk), L.ptr(cull)
        sels = {"run": BM.run_sel(F0), "path": BM.path_sel(3, idx)}
        sinks = {"float": BM.float_out(rgb, alpha), "display": BM.display_out(buf3, 3)}
        if layout == "pool":
            bl, po = L.ptr(m.lay.blocks), L.ptr(m.pool)

            def call(sel, qh, qw, sink):
                return lib.vl3d_render_fwd_baked_pool(d, bl, po, T_CLIP, hom, sel, qk, qh, qw, 0, sc, sink, stream)
        else:
            cl = L.ptr(m.clip)

            def call(sel, qh, qw, sink):
                return lib.vl3d_render_fwd_baked(d, cl, T_CLIP, hom, sel, qk, qh, qw, sc, sink, stream)
        # (source: this layout's entry) x (selection) x (sink): all eight combinations over the two layouts
        bad = [(abs(QH), -abs(QW)), (0, abs(QW)), (-4, -7), (-g["Hs"], -g["Ws"])]
        for sname, sel in sels.items():
            for qh, qw in bad:      # the display-sink call refuses with the float-sink call's exact message
                assert call(sel, qh, qw, sinks["float"]) == EINVAL, (layout, sname, qh, qw)
                theirs = lib.vl3d_last_error()
                assert call(sel, qh, qw, sinks["display"]) == EINVAL, (layout, sname, qh, qw)
                assert lib.vl3d_last_error() == theirs and b"bad quad grid" in theirs, (layout, sname, theirs)
            for C in (0, 2, 5):
                assert call(sel, QH, QW, BM.display_out(buf3, C)) == EINVAL and b"channels" in lib.vl3d_last_error()
            assert call(sel, QH, QW, BM.display_out(None, 3)) == EINVAL and b"null pointer" in lib.vl3d_last_error()
        torch.cuda.synchronize()
        assert bool((buf3 == SENT).all()) and bool((buf4 == SENT).all()) and bool((raw == SENT).all())      # nothing was launched
        assert bool((rgb == 123.0).all()) and bool((alpha == 123.0).all())
        for sname, sel in sels.items():
            for kname, sink in sinks.items():
                assert call(sel, QH, QW, sink) == 0, (layout, sname, kname, lib.vl3d_last_error())
        torch.cuda.synchronize()
    # a random background is a draw per call: the display frames refuse it and point at render
    mpv = BakedMPV(models["shared"].clip, models["shared"].qk, _spec(GEOM["shared"], W), "random", None)
    with pytest.raises(RuntimeError, match="render"):
        mpv.render_display(H, W, torch.eye(4)[None], torch.eye(3)[None], [0])
