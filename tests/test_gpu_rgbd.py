"""RGB-D frames on the MI355X (include/vl3d.h "RGB-D"; csrc/vl3d_render_rgbd.hip): colour and depth of the baked playback model from one
launch, on the five storages of tests/disparity_models.baked_scenes() -- the dense clip, the shared-border and the tile-exact culled clip, the
pool in both layouts -- as runs (BS.RUNS), a camera path (BS.PATH) and a path in loop time (BS.TIMES).

Exact, bit for bit: (1) the float sink's rgb and alpha are the colour entry's on the same call; (2) its disp of a run or a path is the disparity
entry's; (3) the display frames are the colour entry's display sink, RGB8 and RGBA8, with and without a background, BS.BG_CLAMPS included;
(4) depth16 is trunc(65535 clip(disp, 0, 1)) taken in fp32 torch on the float sink's disp of the same call, under rows normalised over
(1, 100) (the lower clamp bites) and over (2, 50) (both bite: asserted on the host); (5) a loop time with f == 0 has the bits of path frame
(cam, t0), disp included, and static texels -- a clip in the static convention, a pool of static blocks, a model of one frame -- give the
same bits at any f; (6) the pool has the bits of the clip entry on the unpacked texels; (7) two calls give the same bits and a frame does
not depend on the run or path it is rendered in.

Against the fp64 statement of tests/rgbd_statement.py: the depth at a loop time, the one output no existing entry vouches for, within
B = 4 max |statement in fp32 - fp64| over the safe pixels (no floor; unsafe pixels at most 1 %), and depth16 within 65535 B + 1 levels.

Shapes (tests/disparity_models.py): D = 5, T = 5, planes 21 x 75, a view of 13 x 70 -- a full 64-pixel row segment (the lane-packed colour
stores) plus a ragged one (byte stores), and a ragged tile row; D = 70 once for the plane-mask word boundary."""
import copy
import dataclasses
import types

import numpy as np
import pytest
import torch

import baked_models as BM
import baked_statement as BS
import disparity_models as DM
import package_models as PM
import rgbd_statement as RS
import test_rgbd_refusals_cpu as RR

pytestmark = pytest.mark.gpu

STORAGES = ["dense", "shared", "exact", "pool_shared", "pool_exact"]
SENTINEL = 12345.0
PATH_CAMS, PATH_TS = [c for c, _ in BS.PATH], [t for _, t in BS.PATH]
TIME_CAMS, TIME_TS = [c for c, _ in BS.TIMES], [t for _, t in BS.TIMES]


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_CACHE = {}


def _cached(key, make):
    """a reference computed once, shared among the tests that need it, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _scene(name):
    return _cached("baked scenes", DM.baked_scenes)[name]


def _qk(keep, dev):
    return None if keep is None else keep.to(torch.uint8).to(dev)


def _calls(s, dev, rows=None):
    """a storage of disparity_models.baked_scenes on the device -> its RGB-D call rgbd(run= | path= | times=, sink...) under one camera (run:
    cam=) or all of them, the colour twins col(...) and the disparity twins dis(...)"""
    from videoloop3d_amd import render as R
    S = s.scene
    homos, rows, qk = S.homos.to(dev), (s.rows if rows is None else rows).to(dev), _qk(s.keep, dev)
    if s.kind == "pool":
        lay, pool, kw = copy.copy(s.lay).to(dev), s.pool.to(dev), dict(quad_keep=qk, culled_rgba8=s.culled)
        rgbd = lambda h, r, **k: R.render_rgbd_baked_pool(lay, pool, h, r, S.H, S.W, S.spec, **kw, **k)      # noqa: E731
        col = dict(run=lambda cam, f0, n, **o: R.render_frame_run_baked_pool(lay, pool, f0, n, homos[cam], S.H, S.W, S.spec, **kw, **o),
                   path=lambda c, t, **o: R.render_path_baked_pool(lay, pool, c, t, homos, S.H, S.W, S.spec, **kw, **o),
                   times=lambda c, t, **o: R.render_times_baked_pool(lay, pool, c, t, homos, S.H, S.W, S.spec, **kw, **o))
        dis = dict(run=lambda cam, f0, n: R.render_frame_run_disparity_baked_pool(lay, pool, f0, n, homos[cam], rows[cam], S.H, S.W, S.spec, **kw),
                   path=lambda c, t: R.render_path_disparity_baked_pool(lay, pool, c, t, homos, rows, S.H, S.W, S.spec, **kw))
        src = lambda: R._baked_pool("test", lay, pool, homos, S.spec, qk, s.culled)[1]      # noqa: E731
    else:
        clip = s.clip.to(dev)
        rgbd = lambda h, r, **k: R.render_rgbd_baked(clip, h, r, S.H, S.W, S.spec, quad_keep=qk, **k)      # noqa: E731
        col = dict(run=lambda cam, f0, n, **o: R.render_frame_run_baked(clip, f0, n, homos[cam], S.H, S.W, S.spec, quad_keep=qk, **o),
                   path=lambda c, t, **o: R.render_path_baked(clip, c, t, homos, S.H, S.W, S.spec, quad_keep=qk, **o),
                   times=lambda c, t, **o: R.render_times_baked(clip, c, t, homos, S.H, S.W, S.spec, quad_keep=qk, **o))
        dis = dict(run=lambda cam, f0, n: R.render_frame_run_disparity_baked(clip, f0, n, homos[cam], rows[cam], S.H, S.W, S.spec, quad_keep=qk),
                   path=lambda c, t: R.render_path_disparity_baked(clip, c, t, homos, rows, S.H, S.W, S.spec, quad_keep=qk))
        src = lambda: R._baked_dense("test", clip, homos, S.spec, qk)[1]      # noqa: E731

    def call(run=None, path=None, times=None, cam=0, **sink):
        if run is not None:
            return rgbd(homos[cam], rows[cam], run=run, path=path, times=times, **sink)
        return rgbd(homos, rows, path=path, times=times, **sink)
    return types.SimpleNamespace(rgbd=call, col=col, dis=dis, src=src, homos=homos, rows=rows, H=S.H, W=S.W, spec=S.spec)


def _selections():
    """name -> (the keyword of the RGB-D call, the arguments of the twin, the number of frames)"""
    out = {tag: ("run", (0, f0, n), n) for tag, (f0, n) in BS.RUNS.items()}
    out["path"] = ("path", (PATH_CAMS, PATH_TS), len(BS.PATH))
    out["times"] = ("times", (TIME_CAMS, TIME_TS), len(BS.TIMES))
    return out


def _rgbd_of(k, kind, args, **sink):
    return k.rgbd(run=args[1:], cam=args[0], **sink) if kind == "run" else k.rgbd(**{kind: args}, **sink)


# ---- contracts 1, 2, 7: the float sink -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STORAGES)
def test_float_sink_has_the_bits_of_the_colour_and_the_disparity_entries(dev, name):
    k = _calls(_scene(name), dev)
    frames = {}
    for tag, (kind, args, n) in _selections().items():
        rgb, alpha, disp = _rgbd_of(k, kind, args)
        assert rgb.shape == (n, k.H, k.W, 3) and alpha.shape == (n, k.H, k.W) and disp.shape == (n, k.H, k.W) and disp.dtype == torch.float32
        rgb_c, alpha_c = k.col[kind](*args)
        assert torch.equal(rgb, rgb_c) and torch.equal(alpha, alpha_c), (name, tag)
        if kind != "times":      # (a loop time has no disparity twin: the statement below)
            disp_d, alpha_d = k.dis[kind](*args)
            assert torch.equal(disp, disp_d) and torch.equal(alpha, alpha_d), (name, tag)
        again = _rgbd_of(k, kind, args)
        assert all(torch.equal(a, b) for a, b in zip((rgb, alpha, disp), again)), (name, tag)      # two calls: the same bits
        if kind == "run":
            for i in range(n):
                frames.setdefault((args[0], args[1] + i), []).append((rgb[i], alpha[i], disp[i]))
        elif kind == "path":
            for i, ct in enumerate(BS.PATH):
                frames.setdefault(ct, []).append((rgb[i], alpha[i], disp[i]))
    for (c, t) in BS.PATH:      # every frame of the path once more as the run of that frame alone
        frames[(c, t)].append(tuple(x[0] for x in k.rgbd(run=(t, 1), cam=c)))
    shared = [ct for ct, fr in frames.items() if len(fr) > 1]
    assert (0, 1) in shared and len(frames[(0, 1)]) >= 4      # frame 1 of camera 0: in two runs (frame pairs), on the path, alone; frame 3: a pair's odd tail
    for ct, fr in frames.items():      # a frame's bits do not depend on the run or path it is rendered in
        for other in fr[1:]:
            assert all(torch.equal(a, b) for a, b in zip(fr[0], other)), (name, ct)
    assert 0.3 < float((alpha > 0).double().mean()) < 1.0 and float(disp.max()) > 0.05


# ---- contracts 3, 4: the display sink --------------------------------------------------------------------------------------------------------------
def _levels(disp):
    """contract 4's right-hand side: fp32 torch on the float sink's disp"""
    assert disp.dtype == torch.float32
    return (65535 * disp.clamp(0, 1)).to(torch.int32)


@pytest.mark.parametrize("name", STORAGES)
def test_display_sink_has_the_colour_entrys_bytes_and_the_levels_of_its_own_disp(dev, name):
    s = _scene(name)
    k = _calls(s, dev, _cached("rows 1 100", lambda: DM.camera_rows(DM.D, DM.H, DM.W, normalise=(1.0, 100.0))))
    for tag, (kind, args, n) in _selections().items():
        _, _, disp = _rgbd_of(k, kind, args)
        want16 = _levels(disp)
        if tag in ("path", "times"):
            assert float(disp.min()) < 0.0 and float(disp.max()) < 1.0 and int((want16 == 0).sum()) > 0      # the lower clamp bites
        for channels in (3, 4):
            for bg in BS.BGS:
                frames8 = torch.full((n, k.H, k.W, channels), 77, dtype=torch.uint8, device=dev)
                depth16 = torch.full((n, k.H, k.W), 4242, dtype=torch.int32, device=dev).to(torch.uint16)
                got = _rgbd_of(k, kind, args, frames8=frames8, depth16=depth16, bg=bg)
                assert got[0] is frames8 and got[1] is depth16
                want8 = k.col[kind](*args, frames8=torch.empty_like(frames8), bg=bg)
                assert torch.equal(frames8, want8), (name, tag, channels, bg)
                assert torch.equal(depth16.to(torch.int32), want16), (name, tag, channels, bg)


@pytest.mark.parametrize("name", STORAGES)
def test_both_clamps_of_depth16_bite_under_rows_over_2_50(dev, name):
    s = _scene(name)
    k = _calls(s, dev, _cached("rows 2 50", lambda: DM.camera_rows(DM.D, DM.H, DM.W, normalise=(2.0, 50.0))))
    for kind, args, n in (_selections()["path"], _selections()["times"], _selections()["run of 3"]):
        _, _, disp = _rgbd_of(k, kind, args)
        depth16 = torch.zeros((n, k.H, k.W), dtype=torch.int32, device=dev).to(torch.uint16)
        _rgbd_of(k, kind, args, frames8=torch.empty((n, k.H, k.W, 3), dtype=torch.uint8, device=dev), depth16=depth16)
        host, lv = disp.cpu(), depth16.cpu().to(torch.int32)
        below, above = host < 0, host > 1
        assert int(below.sum()) > 0 and int(above.sum()) > 0, (name, kind)      # both clamps bite, decided on the host
        assert bool((lv[below] == 0).all()) and bool((lv[above] == 65535).all()) and int(((lv > 0) & (lv < 65535)).sum()) > 0
        assert torch.equal(lv, _levels(disp).cpu()), (name, kind)


# ---- contract 5: loop time -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STORAGES)
def test_a_loop_time_with_f_0_is_the_path_frame_and_static_texels_do_not_move(dev, name):
    from videoloop3d_amd import tiles
    s = _scene(name)
    k = _calls(s, dev)
    whole = [(c, t) for c, t in BS.TIMES if float(t) == int(t)]
    assert len(whole) >= 2
    at_time = k.rgbd(times=([c for c, _ in whole], [t for _, t in whole]))
    at_frame = k.rgbd(path=([c for c, _ in whole], [int(t) for _, t in whole]))
    assert all(torch.equal(a, b) for a, b in zip(at_time, at_frame)), name
    # static texels in both frames: the same bits at any f
    if s.kind == "pool":      # a pool of static blocks alone
        st = BM._pool_storage(name + " static", s.keep, s.keep & False, DM.T, DM.HS, DM.WS, s.tile, s.source, s.scene.homos, DM.H, DM.W, s.scene.spec)
        st.culled, st.rows = BS.CULLED, s.rows
        assert int(((st.lay.blocks >= 0) & ((st.lay.blocks & 1) == 1)).sum()) == 0
    else:                     # the static convention with no dynamic texel: every frame holds frame 0
        clip = BS.static_convention(s.clip, torch.zeros(s.clip.shape[0], DM.HS, DM.WS, dtype=torch.bool))
        st = types.SimpleNamespace(kind="clip", scene=BS.Scene(name, clip, s.scene.homos, DM.H, DM.W, s.scene.spec, s.keep), clip=clip, keep=s.keep, rows=s.rows)
    ks = _calls(st, dev)
    moving = ks.rgbd(times=(TIME_CAMS, TIME_TS))
    still = ks.rgbd(path=(TIME_CAMS, [int(t) for t in TIME_TS]))
    assert all(torch.equal(a, b) for a, b in zip(moving, still)), name
    assert not torch.equal(k.rgbd(times=(TIME_CAMS, TIME_TS))[2], k.rgbd(path=(TIME_CAMS, [int(t) for t in TIME_TS]))[2])      # (the moving scene moves)


@pytest.mark.parametrize("name", STORAGES)
def test_loop_time_depth_against_the_fp64_statement(dev, name):
    s = _scene(name)
    k = _calls(s, dev)
    st = _cached(("statement", name), lambda: RS.statement(s.scene, s.rows, BS.TIMES))
    assert st.unsafe_share <= 0.01
    _, alpha, disp = k.rgbd(times=(TIME_CAMS, TIME_TS))
    st.check("times", disp, alpha)
    # the 16-bit depth under rows normalised over (1, 100): within 65535 B + 1 levels of the statement
    rows = _cached("rows 1 100", lambda: DM.camera_rows(DM.D, DM.H, DM.W, normalise=(1.0, 100.0)))
    stn = _cached(("statement 1 100", name), lambda: RS.statement(s.scene, rows, BS.TIMES))
    n = len(BS.TIMES)
    depth16 = torch.zeros((n, k.H, k.W), dtype=torch.int32, device=dev).to(torch.uint16)
    _calls(s, dev, rows).rgbd(times=(TIME_CAMS, TIME_TS), frames8=torch.empty((n, k.H, k.W, 3), dtype=torch.uint8, device=dev), depth16=depth16)
    bad, worst, tol = RS.levels_outside(stn, depth16)
    print(f"[{name}] depth16 against the statement: worst distance {worst:.2f} levels of tolerance {tol:.2f}")
    assert bad == 0


# ---- contract 6: the pool against the clip on the unpacked texels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pool_shared", "pool_exact"])
def test_the_pool_has_the_bits_of_the_clip_entry_on_the_unpacked_texels(dev, name):
    s = _scene(name)
    k = _calls(s, dev)
    un = types.SimpleNamespace(kind="clip", scene=s.scene, clip=s.scene.clip, keep=s.keep, rows=s.rows)      # (BS.pool_as_clip of the table)
    ku = _calls(un, dev)
    for tag, (kind, args, n) in _selections().items():
        assert all(torch.equal(a, b) for a, b in zip(_rgbd_of(k, kind, args), _rgbd_of(ku, kind, args))), (name, tag)
        sinks = [dict(frames8=torch.empty((n, k.H, k.W, 4), dtype=torch.uint8, device=dev),
                      depth16=torch.zeros((n, k.H, k.W), dtype=torch.int32, device=dev).to(torch.uint16), bg=BS.BG_QUARTER) for _ in range(2)]
        _rgbd_of(k, kind, args, **sinks[0])
        _rgbd_of(ku, kind, args, **sinks[1])
        assert torch.equal(sinks[0]["frames8"], sinks[1]["frames8"]) and torch.equal(sinks[0]["depth16"].to(torch.int32), sinks[1]["depth16"].to(torch.int32))


# ---- the plane-mask word boundary; a model of one frame ------------------------------------------------------------------------------------------------
def test_plane_mask_word_boundary_and_a_clip_of_one_frame(dev):
    from videoloop3d_amd import render as R
    s = _cached("d70", DM.scene_d70)
    clip = (torch.sigmoid(s.stack.double()) * 255).floor().clamp(0, 255).to(torch.uint8).to(dev)      # BS.random_clip's bake rule
    homos, rows, qk = s.homos.to(dev), s.rows.to(dev), _qk(s.keep, dev)
    c = DM.CAM70
    rgb, alpha, disp = R.render_rgbd_baked(clip, homos[c], rows[c], s.H, s.W, s.spec, run=(0, 1), quad_keep=qk)
    rgb_c, alpha_c = R.render_frame_run_baked(clip, 0, 1, homos[c], s.H, s.W, s.spec, quad_keep=qk)
    disp_d, _ = R.render_frame_run_disparity_baked(clip, 0, 1, homos[c], rows[c], s.H, s.W, s.spec, quad_keep=qk)
    assert torch.equal(rgb, rgb_c) and torch.equal(alpha, alpha_c) and torch.equal(disp, disp_d)
    keep64 = s.keep.clone()
    keep64[64:] = False      # planes behind the word boundary contribute: without them another map
    d64 = R.render_rgbd_baked(clip, homos[c], rows[c], s.H, s.W, s.spec, run=(0, 1), quad_keep=_qk(keep64, dev))[2]
    assert float((d64 - disp).abs().max()) > 1e-4
    # T = 1: t1 = t0, the same bits at any f
    at = R.render_rgbd_baked(clip, homos, rows, s.H, s.W, s.spec, times=([c, c, c], [0.0, 0.5, 0.999]), quad_keep=qk)
    for i in range(3):
        assert torch.equal(at[0][i], rgb[0]) and torch.equal(at[1][i], alpha[0]) and torch.equal(at[2][i], disp[0]), i


# ---- out of range: nothing loaded, nothing stored ----------------------------------------------------------------------------------------------------
def _raw_call(k, dev, n, sel=None, times=None, n_cams=3, sink=None):
    """the C entry past the wrapper's range checks: idx rows uploaded as they are"""
    from videoloop3d_amd import _lib as L, render as R
    src = k.src()
    desc = R._desc_dims(src.dims[0], n, src.dims[1], src.dims[2], k.H, k.W, k.spec, L.STACK_DTYPE["u8"])
    fsel = tsel = None
    if sel is not None:
        fsel = L.BakedFrames(frame0=0, n_cams=n_cams, frame_cam=sel[0].data_ptr(), frame_t=sel[1].data_ptr())
    else:
        tsel = L.BakedTimes(n_cams=n_cams, frame_cam=times[0].data_ptr(), frame_time=times[1].data_ptr())
    with torch.cuda.device(dev):
        cull = None if src.qk is None else R._path_cull_scratch(desc, n_cams, dev, None, "test")
        grid = (0, 0) if src.qk is None else R._qgrid(src.qk, k.spec)
        entry = src.entry.replace("vl3d_render_fwd_", "vl3d_render_rgbd_")
        L.check(getattr(L.lib(), entry)(desc, *src.head, L.ptr(k.homos), L.ptr(k.rows), fsel, tsel, L.ptr(src.qk), *grid, *src.culled, L.ptr(cull), sink,
                                        L.stream_ptr(dev)), entry)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", STORAGES)
def test_an_out_of_range_camera_frame_or_time_leaves_prefilled_outputs_untouched(dev, name):
    from videoloop3d_amd import _lib as L
    k = _calls(_scene(name), dev)
    with pytest.raises(IndexError):
        k.rgbd(path=([0, 3], [1, 1]))
    with pytest.raises(IndexError):
        k.rgbd(path=([0, 1], [1, DM.T]))
    with pytest.raises(ValueError):
        k.rgbd(times=([0, 1], [1.0, float(DM.T)]))
    with pytest.raises(ValueError):
        k.rgbd(run=(0, 1), path=([0], [0]))
    cams = [0, 3, 1, -1, 2, 0]      # frames 1 .. 4 are out of range, each in its own way
    ts = [1, 1, DM.T, 2, -1, 4]
    tt = [1.5, 1.5, float(DM.T), 2.0, float("nan"), 4.25]
    n = len(cams)
    cam_d = torch.tensor(cams, dtype=torch.int32, device=dev)
    for second, kw in ((torch.tensor(ts, dtype=torch.int32, device=dev), "sel"), (torch.tensor(tt, dtype=torch.float32, device=dev), "times")):
        rgb = torch.full((n, k.H, k.W, 3), SENTINEL, device=dev)
        alpha, disp = torch.full((n, k.H, k.W), SENTINEL, device=dev), torch.full((n, k.H, k.W), SENTINEL, device=dev)
        _raw_call(k, dev, n, sink=L.RgbdOut(rgb=rgb.data_ptr(), alpha=alpha.data_ptr(), disp=disp.data_ptr()), **{kw: (cam_d, second)})
        frames8 = torch.full((n, k.H, k.W, 3), 77, dtype=torch.uint8, device=dev)
        depth16 = torch.full((n, k.H, k.W), 4242, dtype=torch.int32, device=dev).to(torch.uint16)
        _raw_call(k, dev, n, sink=L.RgbdOut(frames=frames8.data_ptr(), channels=3, depth16=depth16.data_ptr()), **{kw: (cam_d, second)})
        for i in (1, 2, 3, 4):
            assert bool((rgb[i] == SENTINEL).all()) and bool((alpha[i] == SENTINEL).all()) and bool((disp[i] == SENTINEL).all()), (name, kw, i)
            assert bool((frames8[i] == 77).all()) and bool((depth16[i].to(torch.int32) == 4242).all()), (name, kw, i)
        for i in (0, 5):
            one = k.rgbd(path=([cams[i]], [ts[i]])) if kw == "sel" else k.rgbd(times=([cams[i]], [tt[i]]))
            assert torch.equal(rgb[i], one[0][0]) and torch.equal(alpha[i], one[1][0]) and torch.equal(disp[i], one[2][0]), (name, kw, i)
            assert not bool((depth16[i].to(torch.int32) == 4242).all())


# ---- the refusals on real buffers ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def buffers(dev):
    """real buffers of the refusal rows' shapes (test_rgbd_refusals_cpu.refusal_desc): nothing is launched on them"""
    return dict(baked=torch.zeros((2, 5, 8, 8, 4), dtype=torch.uint8, device=dev), blocks=torch.zeros((2, 1, 1), dtype=torch.int32, device=dev),
                pool=torch.zeros((6 * 64, 4), dtype=torch.uint8, device=dev), homos=torch.eye(3, device=dev).repeat(2, 1, 1).contiguous(),
                rows=torch.zeros((2, 3), device=dev) + 0.5, qk=torch.ones((2, 2, 2), dtype=torch.uint8, device=dev),
                cull=torch.zeros(64, dtype=torch.int64, device=dev), rgb=torch.full((3, 4, 6, 3), SENTINEL, device=dev),
                alpha=torch.full((3, 4, 6), SENTINEL, device=dev), disp=torch.full((3, 4, 6), SENTINEL, device=dev),
                frames=torch.full((3, 4, 6, 4), 77, dtype=torch.uint8, device=dev),
                depth16=torch.full((3, 4, 6), 4242, dtype=torch.int32, device=dev).to(torch.uint16), idx=torch.zeros((2, 3), dtype=torch.int32, device=dev))


@pytest.mark.parametrize("entry, fields, over, fragment", RR.ROWS)
def test_refusals_leave_the_outputs_untouched(dev, buffers, entry, fields, over, fragment):
    over = {key: (buffers["disp"].data_ptr() if key == "disp" and v == RR.P else v) for key, v in over.items()}
    rc, msg = RR.call_refusal(entry, RR.refusal_desc(**fields), {key: v.data_ptr() for key, v in buffers.items()}, over)
    torch.cuda.synchronize()
    assert rc == RR.EINVAL, (rc, msg)
    assert msg.startswith(entry.encode() + b": ") and fragment in msg, msg
    for key in ("rgb", "alpha", "disp"):
        assert bool((buffers[key] == SENTINEL).all()), key
    assert bool((buffers["frames"] == 77).all()) and bool((buffers["depth16"].to(torch.int32) == 4242).all())


# ---- the models ------------------------------------------------------------------------------------------------------------------------------------------
def _poses(K, n=7):
    return np.stack([PM.tilted_pose(i) for i in range(n)]), np.stack([K.astype(np.float32)] * n)


def _model_case(dev, baked, Hm, Wm, K, tag):
    """_Baked.render_rgbd against render_path, render_disparity and render_display, bit for bit; fractional times against the statement"""
    from videoloop3d_amd.baked import path_cameras
    ext, intr = _poses(K)
    T = baked.frm_num
    ts = [i % T for i in range(7)]
    rgb, alpha, disp = baked.render_rgbd(Hm, Wm, ext, intr, ts, normalise=False)
    rgb_p, alpha_p = baked.render_path(Hm, Wm, ext, intr, ts)
    disp_d, alpha_d = baked.render_disparity(Hm, Wm, ext, intr, ts)
    assert torch.equal(rgb.permute(0, 3, 1, 2), rgb_p) and torch.equal(alpha, alpha_p), tag
    assert torch.equal(disp, disp_d) and torch.equal(alpha, alpha_d), tag
    assert float(disp.max()) > 0.05 and 0.2 < float((alpha > 0).double().mean()) < 1.0
    # chunks that are runs and chunks that are paths: the same bits
    same = np.stack([ext[1]] * 7)
    run_ts = [0, 1, 2, 3, 4, 5 % T, 0]
    a = baked.render_rgbd(Hm, Wm, same, intr, run_ts, normalise=False, max_batch=3)
    b = baked.render_rgbd(Hm, Wm, same, intr, run_ts, normalise=False, max_batch=64)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), tag
    # the display sink: render_display's bytes, and the levels of the normalised disp of the float sink
    frames8, depth16 = baked.render_rgbd(Hm, Wm, ext, intr, ts, display=True, channels=4)
    assert torch.equal(frames8, baked.render_display(Hm, Wm, ext, intr, ts, channels=4)), tag
    dn = baked.render_rgbd(Hm, Wm, ext, intr, ts)[2]
    assert depth16.dtype == torch.uint16 and torch.equal(depth16.to(torch.int32), _levels(dn)), tag
    assert float(dn.max()) > 0.05 and int(depth16.to(torch.int32).max()) > 1000
    # fractional loop times: colour is render_path's, depth within the statement's bound
    tf = [0.0, 1.5, 2.25, T - 0.5, T + 1.75, -0.25, 3.0]
    rgb_f, alpha_f, disp_f = baked.render_rgbd(Hm, Wm, ext, intr, tf, fractional=True, normalise=False)
    rgb_q, alpha_q = baked.render_path(Hm, Wm, ext, intr, tf, fractional=True)
    assert torch.equal(rgb_f.permute(0, 3, 1, 2), rgb_q) and torch.equal(alpha_f, alpha_q), tag
    from videoloop3d_amd.baked import loop_times
    cam_of, homos = path_cameras(baked.camera, torch.tensor(ext), torch.tensor(intr))
    first = [cam_of.index(c) for c in range(len(homos))]      # a pose of every distinct camera
    rows = baked.camera.depth_rows(baked.extrins_to_ref(torch.tensor(ext[first])), torch.tensor(intr[first]))
    texels = baked.unpack_frames(range(T)).cpu() if hasattr(baked, "unpack_frames") else baked.texels.cpu()
    keep = None if baked.quad_keep is None else baked.quad_keep.cpu().bool()
    spec = dataclasses.replace(baked.spec, rgb_act="none", alpha_act="none")      # the texels are activated already: the statement decodes them
    scene = BS.Scene(tag, texels, homos.float(), Hm, Wm, spec, keep, pool=hasattr(baked, "pool"))
    st = RS.statement(scene, rows, [(c, float(t)) for c, t in zip(cam_of, loop_times(tf, T))])
    st.check("fractional", disp_f, alpha_f)
    return frames8, depth16


def test_render_rgbd_of_the_baked_models(dev, tmp_path):
    from videoloop3d_amd.baked import bake, bake_pool
    from videoloop3d_amd.render_video import read_pgm16, render_rgbd_frames, write_pgm16
    model, Hm, Wm, K = BM.tile_exact_model(dev, "")
    _model_case(dev, bake(model), Hm, Wm, K, "baked tile-exact clip")
    packed, Hp, Wp, Kp = BM.pool_model(dev, "", exact=False)
    pool = bake_pool(packed)
    frames8, depth16 = _model_case(dev, pool, Hp, Wp, Kp, "baked pool")
    lean = pool.trimmed()      # a trimmed pool: the same bits
    ext, intr = _poses(Kp)
    ts = [i % pool.frm_num for i in range(7)]
    f_t, d_t = lean.render_rgbd(Hp, Wp, ext, intr, ts, display=True, channels=4)
    assert torch.equal(f_t, frames8) and torch.equal(d_t.to(torch.int32), depth16.to(torch.int32))
    f_v, d_v = render_rgbd_frames(pool, Hp, Wp, ext, intr, ts, channels=4, max_batch=3)
    assert torch.equal(f_v, frames8) and torch.equal(d_v.to(torch.int32), depth16.to(torch.int32))
    # one frame through the PGM file: big-endian samples, maxval 65535
    path = str(tmp_path / "0000.pgm")
    write_pgm16(path, depth16[2])
    raw = open(path, "rb").read()
    head = b"P5\n%d %d\n65535\n" % (Wp, Hp)
    assert raw.startswith(head) and len(raw) == len(head) + 2 * Hp * Wp
    host = depth16[2].cpu().numpy()
    y, x = np.unravel_index(int(host.argmax()), host.shape)
    o = len(head) + 2 * (y * Wp + x)
    assert host[y, x] > 255 and raw[o] == host[y, x] >> 8 and raw[o + 1] == host[y, x] & 255      # most significant byte first
    assert np.array_equal(read_pgm16(path), host)


def test_render_rgbd_of_an_opened_viewer_package(dev, tmp_path):
    import test_gpu_open_package as OP
    from videoloop3d_amd.baked import bake_pool, culled_texel_rgba8, open_viewer_package
    from videoloop3d_amd.export import save_viewer_package
    model, Hm, Wm, K = OP.straddling_model(dev, "")
    poses = np.tile(np.eye(4, dtype=np.float32)[None, :3], (2, 1, 1))
    save_viewer_package(model, str(tmp_path), poses, np.tile(K.astype(np.float32)[None], (2, 1, 1)), np.array([1.0, 100.0]))
    opened = open_viewer_package(str(tmp_path), dev, bg_color="", culled_rgba8=culled_texel_rgba8("sigmoid", "sigmoid"))
    _model_case(dev, opened, Hm, Wm, K, "opened package")
