"""The tiny baked playback models the four GPU test files of the baked render share (tests/test_gpu_baked.py, _pool, _path, _display), and
the two structs of the C entries (include/vl3d.h: vl3d_baked_frames, vl3d_baked_out) as the direct calls of those tests fill them.

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
