"""The scenes tests/test_disparity_cpu.py (conditions on the statement) and tests/test_gpu_disparity.py (the kernels) share: the smallest
shapes at which the disparity kernels can still go wrong.  D = 5 planes, clips of 5 frames, planes of 21 x 75 texels (no multiple of 8: ragged
8 x 8 blocks in the pool) = 3 x 5 quads, in the tile-exact layout 3 x 5 tiles of 7 x 15 texels; an output of 13 x 70 pixels -- a full 64-pixel
row segment plus a ragged one, and a ragged tile row -- under the three cameras of tests/baked_statement.py.  Every plane's hard-cut edges lie
inside the view: texel = 1.1 x - 1.0 reaches [-1, 76] over the 75 columns, 1.7 y - 0.6 reaches [-0.6, 21.5] over the 21 rows.
One more scene for the plane-mask word boundary: D = 70 on planes of 16 x 24 texels, 2 x 3 quads."""
import dataclasses
import types

import torch

import baked_models as BM
import baked_statement as BS
from videoloop3d_amd import synth
from videoloop3d_amd.render import RenderSpec, depth_rows

D, T = 5, 5
HS, WS, QH, QW, TILE = 21, 75, 3, 5, (7, 15)
H, W = 13, 70
SC, OFF = (1.1, 1.7), (-1.0, -0.6)
KEEPS = {"keep 0": 0.0, "keep 0.3": 0.3, "keep 1": 1.0}
RUNS = {"run of 3": (1, 3), "run of 1": (3, 1), "run of 2": (1, 2)}      # (frame0, n)


def camera_rows(Dn, Hv, Wv, normalise=None):
    """[3,Dn,3]: render.depth_rows of the three cameras of baked_statement.cameras (the benchmark camera, the opposite translation, a principal
    point shifted by 24 px; near 1, far 100), restated from the same synth.make_cameras"""
    from oracle import mpi_oracle as MO
    ref_e, _, tar_e, Kt = synth.make_cameras(Hv, Wv)
    opposite = tar_e.clone()
    opposite[:3, 3] = -tar_e[:3, 3]
    shifted = Kt.clone()
    shifted[0, 2] += 24.0
    to_ref = torch.linalg.inv(ref_e.double())
    E = torch.stack([tar_e.double() @ to_ref, opposite.double() @ to_ref, tar_e.double() @ to_ref])
    return depth_rows(E, torch.stack([Kt, Kt, shifted]), MO.make_depths(Dn, 1.0, 100.0).flip(0), normalise)


def spec_of(layout, rgb_act="none", alpha_act="none", dims=(HS, WS), grid=(QH, QW), tile=TILE, sc=SC, off=OFF):
    """RenderSpec of "dense" / "shared" (texel coordinates of the plane) or "exact" (LATTICE coordinates: a tile of th x tw texels spans
    (th - 1) x (tw - 1) of them over the same plane extent)"""
    if layout != "exact":
        return RenderSpec.mpv(rgb_act=rgb_act, alpha_act=alpha_act, scale=sc, offset=off)
    lat = (grid[1] * (tile[1] - 1) / (dims[1] - 1.0), grid[0] * (tile[0] - 1) / (dims[0] - 1.0))
    return dataclasses.replace(RenderSpec.mpv(rgb_act=rgb_act, alpha_act=alpha_act, scale=(sc[0] * lat[0], sc[1] * lat[1]),
                                              offset=(off[0] * lat[0], off[1] * lat[1])), tile=tuple(tile))


def keep_map(p, Dn=D, grid=(QH, QW), seed=31):
    return synth.hash_uniform((Dn,) + tuple(grid), seed=seed) < p


def float_scenes(dtype=torch.float32, alpha_act="sigmoid"):
    """name -> the float clip in one storage: dense, shared-border culled at three keep densities, tile-exact (keep 0.6).  The logits are
    synth.make_plane_stack's (alpha biased by -0.5: no plane hides the ones behind it), in `dtype`."""
    homos, rows = BS.cameras(D, H, W), camera_rows(D, H, W)
    stack = synth.make_plane_stack(D, T, HS, WS, seed=9, alpha_bias=-0.5).to(dtype)
    out = {"dense": types.SimpleNamespace(name="dense", stack=stack, keep=None, spec=spec_of("dense", "sigmoid", alpha_act))}
    for tag, p in KEEPS.items():
        out["shared " + tag] = types.SimpleNamespace(name="shared " + tag, stack=stack, keep=keep_map(p), spec=spec_of("shared", "sigmoid", alpha_act))
    out["exact"] = types.SimpleNamespace(name="exact", stack=stack, keep=keep_map(0.6), spec=spec_of("exact", "sigmoid", alpha_act))
    for s in out.values():
        s.homos, s.rows, s.H, s.W = homos, rows, H, W
    return out


def baked_scenes(culled=BS.CULLED):
    """the five storages of tests/test_gpu_baked_fp64.py: STORAGES on this file's shapes, as baked_models.fp64_scenes builds them (the dense
    clip: every texel of every frame random; the pools through PackedLayout, unstored blocks reading `culled`), each with its
    baked_statement.Scene and the cameras' rows"""
    homos, rows = BS.cameras(D, H, W), camera_rows(D, H, W)
    clip = BS.random_clip(D, T, HS, WS, seed=7)
    keep, dyn = BM._keep_dyn(D, QH, QW)
    out = {}
    for layout in ("dense", "shared", "exact"):
        qk = None if layout == "dense" else keep
        out[layout] = types.SimpleNamespace(kind="clip", scene=BS.Scene(layout, clip, homos, H, W, spec_of(layout), qk), clip=clip, keep=qk)
    for geom, tile in (("shared", None), ("exact", TILE)):
        source = BS.random_clip(D, T, HS, WS, seed=8)
        s = BM._pool_storage("pool_" + geom, keep, dyn, T, HS, WS, tile, source, homos, H, W, spec_of(geom))
        if culled != BS.CULLED:      # (another texel behind the blocks without storage: the table restated with it)
            s.scene = BS.Scene(s.scene.name, BS.pool_as_clip(s.lay.blocks, s.pool, T, HS, WS, culled), homos, H, W, s.scene.spec, keep, pool=True)
        s.culled = culled
        e = s.lay.blocks
        assert int((e < 0).sum()) > 0 and int(((e >= 0) & ((e & 1) == 0)).sum()) > 0 and int(((e >= 0) & ((e & 1) == 1)).sum()) > 0
        out["pool_" + geom] = s
    for s in out.values():
        s.rows = rows
    return out


CULLED_VISIBLE = 7 | 11 << 8 | 13 << 16 | 96 << 24       # blocks without storage with a visible alpha byte


D70, HS70, WS70, GRID70, CAM70 = 70, 16, 24, (2, 3), 1


def scene_d70():
    """the plane-mask word boundary: 70 planes of 16 x 24 texels under 2 x 3 quads at keep 0.5 (kept quads on both sides of plane 64), alpha
    biased by -3 so that the far planes still show; one frame, the 13 x 70 view of camera CAM70.  At one texel per pixel the planes cover a
    third of the view; 70 planes lay 70 parallel copies of every edge and quad boundary 0.03 px apart, so offset, scale and camera are chosen
    such that none of them passes within 1e-3 texel of a pixel centre (tests/test_disparity_cpu.py holds the unsafe share to 1 %)"""
    sc, off = (1.07, 1.23), (-20.3, -0.3)
    stack = synth.make_plane_stack(D70, 1, HS70, WS70, seed=13, alpha_bias=-3.0)
    keep = keep_map(0.5, D70, GRID70, seed=33)
    assert bool(keep[:64].any()) and bool(keep[64:].any())
    return types.SimpleNamespace(name="D = 70", stack=stack, keep=keep, spec=spec_of("shared", "sigmoid", "sigmoid", sc=sc, off=off),
                                 homos=BS.cameras(D70, H, W), rows=camera_rows(D70, H, W), H=H, W=W)


# ---- the model scenes ---------------------------------------------------------------------------------------------------------------------------
def model_view(Hm, Wm, K):
    """a ref -> target pose (the models' reference extrinsic is the identity) and the intrinsics of the call"""
    import package_models as PM
    return torch.tensor(PM.tilted_pose(2))[None], torch.tensor(K, dtype=torch.float32)[None]


def model_statement(name, model, stack, ext, Kc, Hv, Wv, ts, normalise=None):
    """the statement on a model's own weights (`stack`: its dense clip on the host), homographies and rows"""
    import disparity_statement as DS
    homos = model.plane_homographies(ext, Kc).cpu()
    rows = depth_rows(ext[0], Kc[0], model.planedepth, normalise)
    keep = model.quad_keep.cpu() if model.is_sparse else None
    return DS.clip_statement(name, stack, homos[None], rows[None], [(0, t) for t in ts], Hv, Wv, model.spec, keep)


def stage1_args(**kw):
    a = dict(mpi_h_scale=1.0, mpi_w_scale=1.0, mpi_d=4, atlas_grid_h=2, rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid",
             bg_color="", learn_loop_mask=False, upsample_stage="", scale_invariant=True, sparsity_loss_weight=0.004, rgb_smooth_loss_weight=0.2,
             a_smooth_loss_weight=0.5, density_loss_weight=0.02, d_smooth_loss_weight=0.0, l_smooth_loss_weight=0.0, optimizer="adam", lrate=0.05,
             lrate_decay=100, N_iters=3, sparsify_epoch=-1, density_loss_epoch=0, patch_h_size=16, patch_w_size=20, patch_h_stride=8,
             patch_w_stride=12, vid2img_mode="average", add_intrin_noise=False, i_weights=1, mpi_h_verts=4, mpi_w_verts=5, add_uv_noise=False)
    a.update(kw)
    return types.SimpleNamespace(**a)


def stage1_model(dev, head):
    """a stage-1 model of 4 planes of 24 x 32 texels with the colour head `head` ("direct" | "rgb_sh") and a rotated, cropped view of it
    -> (model, args, MH, MW, MK, near, far, ref -> target extrinsic [1,4,4] float64, crop intrinsics [1,3,3] float64, h, w)"""
    import numpy as np
    import package_models as PM
    from videoloop3d_amd.MPI import MPMesh
    MH, MW, near, far = 24, 32, 1.0, 100.0
    MK = np.array([[0.9 * MW, 0, MW / 2 + 1.5], [0, 0.85 * MW, MH / 2 - 1.0], [0, 0, 1]], np.float64)
    args = stage1_args(rgb_mlp_type=head)
    m = MPMesh(args, MH, MW, np.eye(4), MK, near, far).to(dev).eval()
    with torch.no_grad():
        m.stack.copy_((synth.make_plane_stack(4, 1, MH, MW, seed=17, alpha_bias=-0.5) * 0.7).to(dev))
        if head == "rgb_sh":
            m.stack_sh.copy_((synth.hash_uniform(tuple(m.stack_sh.shape), seed=18) - 0.5).to(dev))
    ext = torch.tensor(PM.tilted_pose(3), dtype=torch.float64)[None]
    Kc = torch.tensor(MK)[None].clone()
    Kc[0, 0, 2] -= 5
    Kc[0, 1, 2] -= 3
    return m, args, MH, MW, MK, near, far, ext, Kc, 20, 26


# ---- the refusals of the three C entries (include/vl3d.h "Disparity"): tests/test_disparity_cpu.py calls them on placeholder addresses where
# no device exists, tests/test_gpu_disparity.py on real buffers -- nothing is launched either way ----------------------------------------------
ENTRIES = ["vl3d_render_disp_fwd", "vl3d_render_disp_baked", "vl3d_render_disp_baked_pool"]
SOURCE = {"vl3d_render_disp_fwd": "stack", "vl3d_render_disp_baked": "baked", "vl3d_render_disp_baked_pool": "pool"}
EINVAL, EUNSUPPORTED = 1, 3


def refusal_desc(entry, **fields):
    """D 2, 3 output frames, 8 x 8 texels, 4 x 6 pixels, the planar convention, sigmoid / sigmoid; fp32 for the float entry, u8 for the baked ones"""
    from videoloop3d_amd import _lib as L
    d = L.RenderDesc()
    d.D, d.T, d.Hs, d.Ws, d.H, d.W = 2, 3, 8, 8, 4, 6
    d.coord_mode, d.border_mode, d.act_order = L.COORD["affine"], L.BORDER["hardcut"], L.ACT_ORDER["post"]
    d.rgb_act = d.alpha_act = L.ACT["sigmoid"]
    d.stack_dtype = L.STACK_DTYPE["f32"] if entry == ENTRIES[0] else L.STACK_DTYPE["u8"]
    d.pixel_center, d.sx, d.sy = 0.5, 1.0, 1.0
    for k, v in fields.items():
        setattr(d, k, v)
    return d


def refusal_rows():
    """[(id, entry, descriptor fields, argument overrides, status, a fragment of the message)].  Overrides: a pointer name -> None (NULL) or
    ("+", bytes) (misaligned by so many bytes); frame0 / QH / QW / a selection "sel" -> ("null" | "half" | "no_cams")."""
    rows = []
    for e in ENTRIES:
        pool, src = e == ENTRIES[2], SOURCE[e]
        with_map = {} if pool else dict(qk="map")      # (the pool always carries its map)
        rows += [("utils-mpi-coordinates", e, dict(coord_mode=0), {}, EUNSUPPORTED, b"the planar MPV convention only"),
                 ("zeros-border", e, dict(border_mode=0), {}, EUNSUPPORTED, b"the planar MPV convention only"),
                 ("uv-noise", e, dict(uv_noise_seed=5), {}, EUNSUPPORTED, b"add_uv_noise is a training switch"),
                 ("a-variant", e, dict(variant=1), {}, EINVAL, b"no kernel variants"),
                 ("129-planes", e, dict(D=129), {}, EINVAL, b"at most 128 planes"),
                 ("null-disp", e, {}, dict(disp=None), EINVAL, b"null pointer"),
                 ("null-rows", e, {}, dict(rows=None), EINVAL, b"null pointer"),
                 ("null-homos", e, {}, dict(homos=None), EINVAL, b"null pointer"),
                 ("null-" + src, e, {}, {src: None}, EINVAL, b"null pointer"),
                 ("misaligned-rows", e, {}, dict(rows=("+", 2)), EINVAL, b"4-byte aligned"),
                 ("misaligned-" + src, e, {}, {src: ("+", 2)}, EINVAL, b"aligned"),
                 ("run-past-the-clip", e, {}, dict(frame0=3), EINVAL, b"the run of frames leaves"),
                 ("run-before-the-clip", e, {}, dict(frame0=-1), EINVAL, b"the run of frames leaves"),
                 ("grid-of-mixed-signs", e, {}, dict(with_map, QW=-2), EINVAL, b"bad quad grid"),
                 ("tile-exact-grid-of-ragged-tiles", e, {}, dict(with_map, QH=-3, QW=-2), EINVAL, b"whole tiles"),
                 ("map-without-cull-scratch", e, {}, dict(with_map, cull=None), EINVAL, b"vl3d_render_cull_scratch_bytes")]
        if e == ENTRIES[0]:
            rows += [("bake-rule-order", e, dict(act_order=2), {}, EUNSUPPORTED, b"VL3D_ACT_BAKED"),
                     ("u8-texels", e, dict(stack_dtype=2), {}, EINVAL, b"stack_dtype must be VL3D_F32 or VL3D_F16")]
        else:
            rows += [("float-texels", e, dict(stack_dtype=0), {}, EINVAL, b"stack_dtype must be VL3D_U8"),
                     ("null-sel", e, {}, dict(sel="null"), EINVAL, b"null pointer (sel)"),
                     ("half-a-path", e, {}, dict(sel="half"), EINVAL, b"neither a run"),
                     ("a-path-of-no-cameras", e, {}, dict(sel="no_cams"), EINVAL, b"n_cams must be in [1, 65535]")]
        if pool:
            rows += [("null-blocks", e, {}, dict(blocks=None), EINVAL, b"null pointer"),
                     ("null-map", e, {}, dict(qk=None), EINVAL, b"the quad map and vl3d_render_cull_scratch_bytes"),
                     ("a-cull-window", e, dict(cull_Hs=16, cull_Ws=16), {}, EINVAL, b"the pool holds whole planes")]
    return rows


def call_refusal(entry, desc, ptr, over):
    """the entry on the addresses `ptr` (name -> int: stack, baked, blocks, pool, homos, rows, qk, cull, disp, alpha, idx) with a row's
    overrides: a clip of 5 frames, the run of desc.T = 3 from frame 1, a 2 x 2 quad map where the row (or the pool) carries one
    -> (status, message)"""
    from videoloop3d_amd import _lib as L
    a = dict(ptr, frame0=1, QH=2, QW=2, sel="run")
    if entry != ENTRIES[2] and over.get("qk") != "map":
        a["qk"], a["cull"], a["QH"], a["QW"] = None, None, 0, 0
    for k, v in over.items():
        if v == "map":
            continue
        a[k] = (ptr[k] + v[1]) if isinstance(v, tuple) else v
    sel = L.BakedFrames(frame0=int(a["frame0"]))
    if a["sel"] == "half":
        sel.n_cams, sel.frame_cam = 1, a["idx"]
    elif a["sel"] == "no_cams":
        sel.n_cams, sel.frame_cam, sel.frame_t = 0, a["idx"], a["idx"]
    sel = None if a["sel"] == "null" else sel
    lib = L.lib()
    if entry == ENTRIES[0]:
        rc = lib.vl3d_render_disp_fwd(desc, a["stack"], int(a["frame0"]), 5, a["homos"], a["rows"], a["qk"], a["QH"], a["QW"], a["cull"], a["disp"],
                                      a["alpha"], None)
    elif entry == ENTRIES[1]:
        rc = lib.vl3d_render_disp_baked(desc, a["baked"], 5, a["homos"], a["rows"], sel, a["qk"], a["QH"], a["QW"], a["cull"], a["disp"], a["alpha"], None)
    else:
        rc = lib.vl3d_render_disp_baked_pool(desc, a["blocks"], a["pool"], 5, a["homos"], a["rows"], sel, a["qk"], a["QH"], a["QW"], 0, a["cull"],
                                             a["disp"], a["alpha"], None)
    return rc, lib.vl3d_last_error()
