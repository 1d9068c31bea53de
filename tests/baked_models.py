"""The tiny baked playback models the four GPU test files of the baked render share (tests/test_gpu_baked.py, _pool, _path, _display), and
the two structs of the C entries (include/vl3d.h: vl3d_baked_frames, vl3d_baked_out) as the direct calls of those tests fill them; at the
end, the same scenes in five storages, and drawn ones, for the fp64 statement (tests/baked_statement.py: fp64_scenes, fp64_random_scene).

The dense scene: D = 4 planes, a clip of 5 frames, planes of 40 x 72 texels = 5 x 9 quads of 8 x 8, output 37 x 70.  The pool scenes: the
shared-border lattice on the same planes, and 5 x 7 tiles of 6 x 10 texels = 30 x 70 texels (tiles straddling the 8 x 8 blocks)."""
import dataclasses
import types

import numpy as np
import torch

from videoloop3d_amd import synth

D, T_ALLOC, T_MODEL = 4, 5, 5
HS, WS, QH, QW = 40, 72, 5, 9
H, W = 37, 70
SC, OFF = (1.06, 1.1), (-1.0, -0.5)      # plane pixel -> texel of a 40 x 72 plane
GEOMS = {"shared": dict(Hs=40, Ws=72, QH=5, QW=9, tile=None),
         "exact": dict(Hs=30, Ws=70, QH=5, QW=7, tile=(6, 10))}


def run_sel(frame0):
    """vl3d_baked_frames of a run"""
    from videoloop3d_amd import _lib as L
    return L.BakedFrames(frame0=int(frame0))


def path_sel(n_cams, idx):
    """vl3d_baked_frames of a camera path: idx int32 [2,N] on the device, row 0 the cameras, row 1 the frames"""
    from videoloop3d_amd import _lib as L
    return L.BakedFrames(n_cams=int(n_cams), frame_cam=idx[0].data_ptr(), frame_t=idx[1].data_ptr())


def float_out(rgb, alpha):
    """vl3d_baked_out of the float sink (a tensor, or None for a NULL pointer)"""
    from videoloop3d_amd import _lib as L
    return L.BakedOut(rgb=None if rgb is None else rgb.data_ptr(), alpha=None if alpha is None else alpha.data_ptr())


def display_out(frames, channels, bg=None):
    """vl3d_baked_out of the display sink: frames a tensor or None, bg a ctypes float[3] (kept alive by the caller) or None"""
    import ctypes
    from videoloop3d_amd import _lib as L
    return L.BakedOut(frames=None if frames is None else frames.data_ptr(), channels=int(channels), bg=None if bg is None else ctypes.addressof(bg))


def specs():
    """layout -> RenderSpec with identity activations.  The plane pixels of the 37 x 70 view are scaled by (1.06, 1.1) and moved by (-1.0, -0.5)
    onto the 40 x 72-texel planes: every plane leaves the frame on the left and at the top (the near ones, with ~2 px of parallax, furthest),
    the far ones on the right and at the bottom as well -- hard-cut edges inside the view on all four sides, at other pixels for every plane."""
    from videoloop3d_amd.render import RenderSpec
    sc, off = (1.06, 1.1), (-1.0, -0.5)
    dense = RenderSpec.mpv(rgb_act="none", alpha_act="none", scale=sc, offset=off)
    # tile-exact: 5 x 9 tiles of 8 x 8 texels; the lattice a quad spans 7 units of is 36 x 64 points over the same plane extent
    lat = (63.0 / 71.0, 35.0 / 39.0)
    exact = dataclasses.replace(RenderSpec.mpv(rgb_act="none", alpha_act="none", scale=(sc[0] * lat[0], sc[1] * lat[1]),
                                               offset=(off[0] * lat[0], off[1] * lat[1])), tile=(8, 8))
    return {"dense": dense, "shared": dense, "exact": exact}


def pool_spec(g):
    """the RenderSpec of a geometry: (a) texel coordinates of the 40 x 72 plane; (b) LATTICE coordinates -- a tile of th x tw texels spans
    (th - 1) x (tw - 1) lattice units, so the 5 x 7 tiles of 6 x 10 are 26 x 64 lattice points over the same plane extent."""
    from videoloop3d_amd.render import RenderSpec
    if g["tile"] is None:
        return RenderSpec.mpv(rgb_act="none", alpha_act="none", scale=SC, offset=OFF)
    th, tw = g["tile"]
    lat = ((g["QW"] * (tw - 1)) / 71.0, (g["QH"] * (th - 1)) / 39.0)
    return dataclasses.replace(RenderSpec.mpv(rgb_act="none", alpha_act="none", scale=(SC[0] * lat[0], SC[1] * lat[1]),
                                              offset=(OFF[0] * lat[0], OFF[1] * lat[1])), tile=(th, tw))


def scatter_pool(lay, clip, fill):
    """dense uint8 clip [D,T,Hs,Ws,4] -> pool [n_slots * 64, 4] through the block table (static blocks take frame 0), plain torch."""
    pool = fill.repeat(lay.n_slots * 64, 1)
    for d in range(lay.D):
        lay.pack_plane_(pool, d, clip[d])
    return pool


def tile_exact_model(dev, bg_color):
    """a tiny sparsified MPMeshVid in the tile-exact layout: 6 planes, 6 frames, 4 x 6 tiles of 8 x 8 texels per plane, about half of the quads
    kept (plane 3 none), a third of the kept ones dynamic -- loaded through init_from_mpi like a checkpoint of this package."""
    from videoloop3d_amd.MPV import MPMeshVid
    Hm, Wm, Dm, Tm, qh, qw, th, tw = 36, 64, 6, 6, 4, 6, 8, 8
    K = np.array([[0.9 * Wm, 0, Wm / 2], [0, 0.9 * Wm, Hm / 2], [0, 0, 1]])
    args = types.SimpleNamespace(mpv_frm_num=Tm, mpv_isloop=True, mpi_h_scale=1.1, mpi_w_scale=1.1, mpi_d=Dm, atlas_grid_h=2, init_std=0.5,
                                 rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color=bg_color, scale_invariant=True,
                                 fp16=False, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1, sparsity_loss_weight=0.0,
                                 rgb_smooth_loss_weight=0.0, a_smooth_loss_weight=0.0, density_loss_weight=0.0, d_smooth_loss_weight=0.0,
                                 optimizer="adam", lrate=0.1, lrate_decay=30, mpi_h_verts=qh + 1, mpi_w_verts=qw + 1)
    model = MPMeshVid(args, Hm, Wm, np.eye(4), K, 1.0, 100.0)
    keep = synth.hash_uniform((Dm, qh, qw), seed=21) < 0.55
    keep[3] = False
    dyn = keep & (synth.hash_uniform((Dm, qh, qw), seed=22) < 0.35)
    stack = synth.make_plane_stack(Dm, Tm, qh * th, qw * tw, seed=5, alpha_bias=0.0) * 0.8
    model.init_from_mpi({"ref_extrin": model.ref_extrin, "ref_intrin": model.ref_intrin, "planedepth": model.planedepth, "stack": stack,
                         "quad_keep": keep, "quad_dyn": dyn, "self.is_sparse": True, "self.has_dyn": True, "self.tile_own": (th, tw),
                         "self.tile_full": (th, tw)})
    model = model.to(dev).eval()
    assert model.is_sparse and model.tile_own == (th, tw) and model.spec.tile == (th, tw) and model.stack.shape == (Dm, Tm, qh * th, qw * tw, 4)
    return model, Hm, Wm, K


def pool_model(dev, bg_color, exact=True):
    """a tiny sparsified MPMeshVid, loaded through init_from_mpi like a checkpoint of this package: 6 planes, 6 frames, about half of the quads
    kept (plane 3 none), a third of the kept ones dynamic.  exact: the tile-exact layout, 4 x 6 tiles of 8 x 8 texels (tile_exact_model's
    geometry); else the shared-border lattice on planes of 38 x 67 texels (ragged last blocks).  Texels no dynamic quad reads
    hold frame 0 in every frame -- the dense model's convention for static texels -- and texels no kept quad reads hold (0, 0, 0,
    tiles.CULLED_ALPHA), what PackedLayout.unpack_plane gives for them and BakedPool.culled_rgba8 bakes (the condition under which the pool and
    bake() of the dense model hold the same texels everywhere a sample can tap: docs/kernels/K9_baked_playback.md, "Culled texels")."""
    from videoloop3d_amd import tiles
    from videoloop3d_amd.MPV import MPMeshVid
    Hm, Wm, Dm, Tm, qh, qw, th, tw = 36, 64, 6, 6, 4, 6, 8, 8
    hs, ws = (qh * th, qw * tw) if exact else (38, 67)
    K = np.array([[0.9 * Wm, 0, Wm / 2], [0, 0.9 * Wm, Hm / 2], [0, 0, 1]])
    args = types.SimpleNamespace(mpv_frm_num=Tm, mpv_isloop=True, mpi_h_scale=1.1, mpi_w_scale=1.1, mpi_d=Dm, atlas_grid_h=2, init_std=0.5,
                                 rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color=bg_color, scale_invariant=True,
                                 fp16=False, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1, sparsity_loss_weight=0.0,
                                 rgb_smooth_loss_weight=0.0, a_smooth_loss_weight=0.0, density_loss_weight=0.0, d_smooth_loss_weight=0.0,
                                 optimizer="adam", lrate=0.1, lrate_decay=30, mpi_h_verts=qh + 1, mpi_w_verts=qw + 1)
    model = MPMeshVid(args, Hm, Wm, np.eye(4), K, 1.0, 100.0)
    keep = synth.hash_uniform((Dm, qh, qw), seed=21) < 0.55
    keep[3] = False
    dyn = keep & (synth.hash_uniform((Dm, qh, qw), seed=22) < 0.35)
    stack = synth.make_plane_stack(Dm, Tm, hs, ws, seed=5, alpha_bias=0.0) * 0.8
    dyn_t = tiles.quad_to_texel_mask(dyn, hs, ws, (th, tw) if exact else None)
    stack = torch.where(dyn_t[:, None, :, :, None], stack, stack[:, :1])
    keep_t = tiles.quad_to_texel_mask(keep, hs, ws, (th, tw) if exact else None)
    stack = torch.where(keep_t[:, None, :, :, None], stack, torch.tensor([0.0, 0.0, 0.0, tiles.CULLED_ALPHA]))
    sd = {"ref_extrin": model.ref_extrin, "ref_intrin": model.ref_intrin, "planedepth": model.planedepth, "stack": stack,
          "quad_keep": keep, "quad_dyn": dyn, "self.is_sparse": True, "self.has_dyn": True}
    if exact:
        sd.update({"self.tile_own": (th, tw), "self.tile_full": (th, tw)})
    model.init_from_mpi(sd)
    model = model.to(dev).eval()
    assert model.is_sparse and model.stack.shape == (Dm, Tm, hs, ws, 4) and (model.tile_own == (th, tw)) == exact
    return model, Hm, Wm, K


# ---- the scenes of the fp64 statement (tests/baked_statement.py): tests/test_baked_statement_cpu.py and tests/test_gpu_baked_fp64.py ---------
def _keep_dyn(Dn, QHn, QWn):
    keep = synth.hash_uniform((Dn, QHn, QWn), seed=11) < 0.5
    keep[2] = False
    return keep, keep & (synth.hash_uniform((Dn, QHn, QWn), seed=12) < 1.0 / 3.0)


def _widen_x(spec, Wv):
    """the x scale shrunk for a view Wv pixels wide (tests/test_gpu_baked_display.py: _spec), so that most of it stays covered"""
    return dataclasses.replace(spec, scale=(spec.scale[0] * 70.0 / Wv, spec.scale[1]))


def _pool_storage(name, keep, dyn, T, Hs, Ws, tile, source, homos, Hv, Wv, spec):
    """a pool through the product's own table (PackedLayout) and scatter, and its Scene: the table restated by baked_statement.pool_as_clip.
    `source`: the dense clip in the static convention, random where nothing is stored."""
    import baked_statement as BS
    from videoloop3d_amd import tiles
    from videoloop3d_amd.packed import PackedLayout
    lay = PackedLayout(keep, dyn, T, Hs, Ws, tile)
    source = BS.static_convention(source, tiles.quad_to_texel_mask(keep & dyn, Hs, Ws, tile))
    pool = scatter_pool(lay, source, torch.zeros((1, 4), dtype=torch.uint8))
    scene = BS.Scene(name, BS.pool_as_clip(lay.blocks, pool, T, Hs, Ws, BS.CULLED), homos, Hv, Wv, spec, keep, pool=True)
    return types.SimpleNamespace(kind="pool", scene=scene, keep=keep, dyn=dyn, lay=lay, pool=pool, source=source, tile=tile)


def fp64_scenes(Hv=H, Wv=W):
    """storage -> the five fixed storages of this file's scenes under the three cameras of tests/test_gpu_baked_path.py, on the host: the dense
    clip (dense, shared-border culled, tile-exact culled: every texel of every frame random) and the two pools of GEOMS (static, dynamic and
    unstored blocks; unstored blocks read baked_statement.CULLED), each with its baked_statement.Scene.  (Hv, Wv): the view."""
    import baked_statement as BS
    homos = BS.cameras(D, Hv, Wv)
    clip = BS.random_clip(D, T_ALLOC, HS, WS, seed=7)
    keep, _ = _keep_dyn(D, QH, QW)
    out = {}
    for layout, spec in specs().items():
        spec, qk = _widen_x(spec, Wv), (None if layout == "dense" else keep)
        out[layout] = types.SimpleNamespace(kind="clip", scene=BS.Scene(layout, clip, homos, Hv, Wv, spec, qk), clip=clip, keep=qk)
    for geom, g in GEOMS.items():
        k, dyn = _keep_dyn(D, g["QH"], g["QW"])
        out["pool_" + geom] = _pool_storage("pool_" + geom, k, dyn, T_MODEL, g["Hs"], g["Ws"], g["tile"], BS.random_clip(D, T_MODEL, g["Hs"], g["Ws"], seed=7),
                                            homos, Hv, Wv, _widen_x(pool_spec(g), Wv))
        e = out["pool_" + geom].lay.blocks
        assert int((e < 0).sum()) > 0 and int(((e >= 0) & ((e & 1) == 0)).sum()) > 0 and int(((e >= 0) & ((e & 1) == 1)).sum()) > 0
    return out


RANDOM_SEEDS = list(range(12))


def fp64_random_scene(seed):
    """a drawn model and view in the five storages -> (storages as fp64_scenes gives them, run [(cam, t)], times [(cam, tau)]).
    Ranges: D 1..6, T 1..5, quad grid 1..6 x 1..9 with a keep density from [0, 1] (every third seed: one plane all culled), shared-border planes
    of 2..75 texels per axis (every fourth seed below 8, then with quads of a texel or more under a frame of 4..8 x 8..16), tile-exact tiles of 2..10 texels per axis, frames of 1..40 x 1..140 (every fourth seed
    exactly 128 wide, every fourth wider than 64).  The homography as tests/test_gpu_fuzz.py: _case draws it -- scale 0.8 .. 1.3, rotation
    within 4 degrees, perspective terms within 2e-4 -- with per-plane parallax, two cameras.  Every shape lies inside the entries' rules
    (planes and tiles of at least 2 x 2 texels, D <= 128), so none is refused.  Offsets and zoom are drawn again until no pixel of a frame of fewer
    than 1000 pixels is unsafe and at most 1 % of a larger one (baked_statement.unsafe_mask), and the planes cover 30 % of the frame or more -- decided on the host, before anything renders."""
    import math
    import baked_statement as BS
    from videoloop3d_amd.render import RenderSpec
    g = torch.Generator().manual_seed(7000 + seed)
    r = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))      # noqa: E731
    u = lambda lo, hi: float(torch.rand(1, generator=g)) * (hi - lo) + lo      # noqa: E731
    tiny = seed % 4 == 1      # planes of a few texels: a quad spans a texel or more, and the frame is small enough to have no unsafe pixel
    Hs, Ws = (r(2, 7), r(2, 7)) if tiny else (r(2, 75), r(2, 75))
    Dn, Tn, QHn, QWn = r(1, 6), r(1, 5), r(1, min(6, Hs - 1)), r(1, min(9, Ws - 1))
    keep = torch.rand((Dn, QHn, QWn), generator=g) < u(0.0, 1.0)
    if seed % 3 == 0 and Dn > 1:
        keep[r(0, Dn - 1)] = False
    if not bool(keep.any()):
        keep[0, 0, 0] = True      # (a pool without a slot is no storage)
    dyn = keep & (torch.rand((Dn, QHn, QWn), generator=g) < 1.0 / 3.0)
    th, tw = r(2, 10), r(2, 10)
    Hv = r(4, 8) if tiny else r(1, 40)          # (not below 4 x 8 there: B is a maximum over the scene's pixels, and a handful samples the oracle's rounding too thinly)
    Wv = r(8, 16) if tiny else 128 if seed % 4 == 2 else r(65, 140) if seed % 4 == 3 else r(1, 140)
    scale, rot = u(0.8, 1.3), math.radians(u(-4, 4))
    kx, ky = min(1.0, Wv / 30.0), min(1.0, Hv / 30.0)      # translation and parallax in pixels, shrunk with a frame of a few pixels
    base = torch.tensor([[math.cos(rot) * scale, -math.sin(rot) * scale, u(-3, 3) * kx], [math.sin(rot) * scale, math.cos(rot) * scale, u(-3, 3) * ky],
                         [u(-2e-4, 2e-4), u(-2e-4, 2e-4), 1.0]])
    par = lambda px, py: torch.stack([base + torch.tensor([[0, 0, px * kx * d], [0, 0, py * ky * d], [0, 0, 0.0]]) for d in range(Dn)])      # noqa: E731
    homos = torch.stack([par(0.7, -0.4), par(-0.5, 0.6)]).float()
    ext = {"shared": (Ws - 1, Hs - 1), "exact": (QWn * (tw - 1), QHn * (th - 1))}
    for _ in range(200):
        # zoom: the plane smaller than the view (hard cuts inside it) or larger; the 0.15 below keeps a rotated frame of one row on the plane
        ox, oy, zoom = u(-0.15, 0.1), u(-0.15, 0.1), u(0.7, 1.2)
        spec = {k: dataclasses.replace(RenderSpec.mpv(rgb_act="none", alpha_act="none", scale=(e[0] / max(Wv * scale * zoom, 0.15 * Hv, 1.0), e[1] / max(Hv * scale * zoom, 0.15 * Wv, 1.0)),
                                                      offset=(ox * e[0], oy * e[1])), tile=((th, tw) if k == "exact" else (0, 0))) for k, e in ext.items()}
        views = (("shared", (Hs, Ws), None), ("shared", (Hs, Ws), keep), ("exact", (QHn * th, QWn * tw), keep))      # dense, shared, exact
        shares = [float(BS.unsafe_mask(homos[c], Hv, Wv, spec[k], hw[0], hw[1], qk).double().mean()) for c in range(2) for k, hw, qk in views]
        seen = min(float(BS.coverage(homos[c], Hv, Wv, spec["shared"], Hs, Ws).any(0).double().mean()) for c in range(2))
        if max(shares) <= (0.0 if Hv * Wv < 1000 else 0.01) and seen >= 0.3:
            break
    else:
        raise AssertionError(f"seed {seed}: no safe offsets in 200 draws")
    clip_s, clip_e = BS.random_clip(Dn, Tn, Hs, Ws, seed=100 + seed), BS.random_clip(Dn, Tn, QHn * th, QWn * tw, seed=200 + seed)
    out = {"dense": types.SimpleNamespace(kind="clip", scene=BS.Scene(f"seed {seed} dense", clip_s, homos, Hv, Wv, spec["shared"], None), clip=clip_s, keep=None),
           "shared": types.SimpleNamespace(kind="clip", scene=BS.Scene(f"seed {seed} shared", clip_s, homos, Hv, Wv, spec["shared"], keep), clip=clip_s, keep=keep),
           "exact": types.SimpleNamespace(kind="clip", scene=BS.Scene(f"seed {seed} exact", clip_e, homos, Hv, Wv, spec["exact"], keep), clip=clip_e, keep=keep),
           "pool_shared": _pool_storage(f"seed {seed} pool_shared", keep, dyn, Tn, Hs, Ws, None, clip_s, homos, Hv, Wv, spec["shared"]),
           "pool_exact": _pool_storage(f"seed {seed} pool_exact", keep, dyn, Tn, QHn * th, QWn * tw, (th, tw), clip_e, homos, Hv, Wv, spec["exact"])}
    f0 = r(0, Tn - 1)
    run = BS.run_sel(r(0, 1), f0, r(1, Tn - f0))
    last = float(np.nextafter(np.float32(Tn), np.float32(0)))
    times = [(0, Tn - 1 + 0.25), (1, 0.0), (1, u(0.0, float(Tn)) if Tn > 1 else 0.5), (0, last), (1, Tn - 1 + 0.625)]      # the seam three times
    return out, run, times
