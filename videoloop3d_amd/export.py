"""Export to the REFERENCE's checkpoint / asset layout: what `MPMeshVid.state_dict()`, `save_mesh` and `save_texture`
of the reference produce (MPV.py:290-341), from the dense plane stack + quad maps of this build.

  reference_state_dict(model)   -> the state_dict the reference's MPMeshVid.init_from_mpi / load_state_dict reads (MPV.py:235-304):
                                   `_verts` (vertex grid, utils_mpi.py:80-89), `faces` / `faces_dyn` (two triangles per quad, vertex
                                   order of MPV.py:66-71), `uvs*` / `uvfaces*` (4 corners per tile, MPI.py:403-418), `atlas` [1,4,..]
                                   (static tiles, stored ONCE) and `atlas_dyn` [T,4,..] (dynamic tiles), camera buffers and the
                                   python scalars under "self.*" keys.  Tiles are packed like MPI.py:364-400 (get_hw grid, row major,
                                   the last tile repeated into the residual slots).
  save_mesh(model, prefix)      -> prefix.obj / prefix_dyn.obj with the reference's OBJ writer conventions (utils.py:403-435:
                                   unused vertices culled, UVs flipped and moved to texel centres by normalize_uv).
  save_texture(model, prefix)   -> prefix_static.png (activated rgba) and prefix_dyn_%04d.png (activated rgb * alpha per frame).
                                   The reference writes the dynamic frames as one .mov through imageio/ffmpeg (MPV.py:341), which this
                                   image does not have: the same frames go out as PNG files instead.
  save_viewer_package(model, outdir, poses, intrins, bds)
                                -> the package a web player loads (scripts/script_export_mesh.py:76-191): geometry.obj (static + dynamic mesh,
                                   vertex colours, faces far to near), static.png / dynamic/%04d.png (straight RGBA, baked by baked.bake_texels
                                   -- the one bake rule, shared with the on-device playback model) and meta.json (camera and clip facts).
The reader of this layout is videoloop3d_amd.tiles.stack_from_reference_state (used by MPMeshVid.init_from_mpi): export -> read
round-trips (tests/test_export_cpu.py).  Unpinned like every statement about the reference's packed format: no checkpoint ships
with the reference and its MPI.py / MPV.py cannot be imported here (oracle/ckpt_oracle.py restates the packing for the tests).
"""
import os
import struct
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from .utils_mpi import gen_mpi_vertices


def atlas_grid(n, max_ratio=4):
    """MPI.py:366-377 get_hw: tile grid (rows, cols, residual slots) for n tiles."""
    if n == 0:
        return 0, 0, 0
    n_min, n_max = int(np.sqrt(n / max_ratio)), int(np.sqrt(n))
    n_try = np.arange(n_min, n_max)
    if len(n_try) == 0 or n_try[0] == 0:          # the reference's arange is empty / starts at 0 for tiny n: one row
        return 1, n + 1, 1
    h = int(n_try[np.argmin(n_try - n % n_try)])
    w = n // h + 1
    return h, w, h * w - n


def quad_faces(D, hv, wv):
    """MPV.py:66-71: [D*(hv-1)*(wv-1), 2, 3] vertex ids, quad order (d, vy, vx), triangles (v0,v1,v3), (v3,v2,v0)."""
    vid = torch.arange(D * hv * wv).reshape(D, hv, wv)
    f013 = torch.stack([vid[:, :-1, :-1], vid[:, :-1, 1:], vid[:, 1:, 1:]], -1)
    f320 = torch.stack([vid[:, 1:, 1:], vid[:, 1:, :-1], vid[:, :-1, :-1]], -1)
    return torch.cat([f013.reshape(-1, 1, 3), f320.reshape(-1, 1, 3)], dim=1)


def _pack_tiles(stack, mask, frames, tile_hw, own=False):
    """tiles of the quads in `mask` [D,QH,QW], sampled from stack (D,T,H,W,4) like MPI.py:306-340 (grid_sample, align_corners=True,
    from the quad's first to its last corner), packed row-major into an atlas [frames,4,Ah,Aw] + per-tile corner UVs / uv faces.
    own: the stack is in the TILE-EXACT layout (tile (vy, vx) = rows [vy ih, (vy+1) ih), columns [vx iw, (vx+1) iw)): its tiles are copied
    texel for texel -- the checkpoint the model was read from comes back bit for bit."""
    D, T, H, W, _ = stack.shape
    QH, QW = mask.shape[1:]
    ch, cw = (H - 1) / QH, (W - 1) / QW
    ih, iw = tile_hw
    idx = mask.reshape(-1).nonzero()[:, 0]
    n = len(idx)
    if n == 0:
        return idx, torch.zeros((frames, 4, 1, 1), device=stack.device), torch.zeros((0, 2), device=stack.device), torch.zeros((0, 3), dtype=torch.long), (0, 0)
    d, rem = idx // (QH * QW), idx % (QH * QW)
    vy, vx = rem // QW, rem % QW
    ys = vy[:, None].double() * ch + torch.linspace(0, ch, ih, dtype=torch.float64)[None]
    xs = vx[:, None].double() * cw + torch.linspace(0, cw, iw, dtype=torch.float64)[None]
    gy, gx = (ys / (H - 1) * 2 - 1).float(), (xs / (W - 1) * 2 - 1).float()
    grid = torch.stack([gx[:, None, :].expand(n, ih, iw), gy[:, :, None].expand(n, ih, iw)], -1).to(stack.device)
    # plane by plane, all frames and all of the plane's tiles in one call (the tiles' grids stacked along the rows): indexing
    # stack[d, t] with one plane index per TILE materialised a whole (H,W,4) plane per tile -- 174 GB at the shipped size
    tiles = torch.empty((frames, n, 4, ih, iw), dtype=torch.float32, device=stack.device)
    dd = d.to(stack.device)
    for plane in torch.unique(d).tolist():
        sel = (dd == plane).nonzero()[:, 0]
        if own:
            img = stack.plane(plane, frames, raw=True).float()                                  # frames,H,W,4 = frames,QH,ih,QW,iw,4
            tl = img.reshape(frames, QH, ih, QW, iw, 4)[:, vy[sel.cpu()].to(img.device), :, vx[sel.cpu()].to(img.device)]    # n_sel,frames,ih,iw,4
            tiles[:, sel] = tl.permute(1, 0, 4, 2, 3)
            continue
        g = grid[sel].reshape(1, len(sel) * ih, iw, 2).expand(frames, -1, -1, -1)
        img = stack.plane(plane, frames).permute(0, 3, 1, 2).float()                            # frames,4,H,W
        out = F.grid_sample(img, g, mode="bilinear", align_corners=True)                        # frames,4,len(sel)*ih,iw
        tiles[:, sel] = out.reshape(frames, 4, len(sel), ih, iw).permute(0, 2, 1, 3, 4)
    gh, gw, pad = atlas_grid(n)
    tiles = torch.cat([tiles, tiles[:, -1:].expand(-1, pad, -1, -1, -1)], 1)                    # MPI.py:392
    atlas = tiles.reshape(frames, gh, gw, 4, ih, iw).permute(0, 3, 1, 4, 2, 5).reshape(frames, 4, gh * ih, gw * iw)
    Ah, Aw = atlas.shape[-2:]
    k = torch.arange(n)
    u0 = (k % gw).double() * iw / (Aw - 1) * 2 - 1                                              # gen_quad_uvs, MPI.py:403-418
    v0 = (k // gw).double() * ih / (Ah - 1) * 2 - 1
    du, dv = 2 / (Aw - 1) * (iw - 1), 2 / (Ah - 1) * (ih - 1)
    uvs = torch.stack([torch.stack([u0, v0], -1), torch.stack([u0 + du, v0], -1), torch.stack([u0, v0 + dv], -1),
                       torch.stack([u0 + du, v0 + dv], -1)], 1).reshape(-1, 2).float()
    uvfaces = ((k * 4)[:, None, None] + torch.tensor([[0, 1, 3], [3, 2, 0]])[None]).reshape(-1, 3)
    return idx, atlas, uvs, uvfaces, (gh, gw)


def check_quad_maps(quad_maps, keep, dyn, own):
    """quad_maps = (keep', dyn') [D,QH,QW] of an export against the model's maps (bool, host) -> (keep', dyn') bool on the host.  The quads written
    are the given ones, so they must be subsets: keep' within quad_keep, dyn' within keep' & quad_dyn (a quad of dyn outside dyn' is written from
    frame 0 into the static atlas) -- else ValueError.  A model of the shared-border lattice (own false) may only drop quads, dyn' == keep' &
    quad_dyn: its export resamples logits, under which "alpha byte 0" survives (a convex combination of logits below the threshold stays below
    it) and "equal bytes in every frame" does not."""
    k, d = (torch.as_tensor(m).detach().cpu().bool() for m in quad_maps)
    if k.shape != keep.shape or d.shape != keep.shape:
        raise ValueError(f"quad_maps: two maps of the model's quad grid {tuple(keep.shape)}, got {tuple(k.shape)} and {tuple(d.shape)}")
    if bool((k & ~keep).any()):
        raise ValueError("quad_maps: keep holds a quad outside the model's quad_keep (an export writes the model's quads, or fewer)")
    if bool((d & ~(k & dyn)).any()):
        raise ValueError("quad_maps: dyn holds a quad outside keep & the model's quad_dyn")
    if not own and not torch.equal(d, k & dyn):
        raise ValueError("quad_maps: a model of the shared-border lattice exports resampled logits and may only drop quads (dyn == keep & quad_dyn); "
                         "writing a dynamic quad from frame 0 needs the tile-exact layout, whose texels are copied")
    return k, d


def reference_state_dict(model, tile_texels=None, quad_maps=None, atlas_to_host=True):
    """model: videoloop3d_amd MPMeshVid / MPMesh (dense or sparsified).  tile_texels=(ih, iw) overrides the tile size (default:
    one sample per texel of the quad, round(quad extent) + 1, the choice oracle/ckpt_oracle.py pins the reader with).
    quad_maps=(keep, dyn): write these quads in place of the model's (check_quad_maps: subsets of them; BakedPool.trimmed gives such maps).
    atlas_to_host=False leaves `atlas` / `atlas_dyn` on the model's device (save_viewer_package bakes them there)."""
    class _Planes:
        """plane accessor: stack[d, :frames] of the dense model without ever holding more than one plane of a packed one."""
        def __init__(self, m):
            self.m = m
            self.shape = tuple(m.stack_dims()) + (4,) if hasattr(m, "stack_dims") else tuple(m.stack.shape)
            self.device = (m._param() if hasattr(m, "_param") else m.stack).device

        def plane(self, d, frames, raw=False):
            pl = self.m.stack_plane(d, range(frames)) if hasattr(self.m, "stack_plane") else self.m.stack.detach()[d, :frames]
            pl = pl.detach()
            if bool(getattr(self.m, "is_sparse", False)) and not raw:
                # texels no kept quad can read hold the alpha logit CULLED_ALPHA (-1e4, tiles.py); a tile's border samples sit exactly on
                # texel centres, but their fp32 coordinates carry ~1e-6 texels of rounding, which would pull 1e-6 * (-1e4) of a culled
                # neighbour into an exported kept texel.  -30 is as transparent (sigmoid = 1e-13) and bleeds nothing.
                pl = torch.cat([pl[..., :3], pl[..., 3:].clamp_min(-30.0)], dim=-1)
            return pl
    stack = _Planes(model)
    D, T, H, W, _ = stack.shape
    hv, wv = int(model.args.mpi_h_verts), int(model.args.mpi_w_verts)
    QH, QW = hv - 1, wv - 1
    own = getattr(model, "tile_own", None) is not None
    if own:                                         # tile-exact layout: the model's tiles ARE the reference's (texel for texel)
        if tile_texels is not None and tuple(tile_texels) != tuple(model.tile_own):
            raise RuntimeError(f"a tile-exact model exports its own tiles of {model.tile_own} texels")
        tile_texels = tuple(model.tile_own)
    if tile_texels is None:
        tile_texels = (int(round((H - 1) / QH)) + 1, int(round((W - 1) / QW)) + 1)
    sparse = bool(getattr(model, "is_sparse", False)) and getattr(model, "quad_keep", None) is not None
    if sparse:
        keep, dyn = model.quad_keep.cpu().bool(), model.quad_dyn.cpu().bool()
    else:                                           # a dense model: every quad exists and is dynamic ("load static as dynamic", MPV.py:266)
        keep = torch.ones((D, QH, QW), dtype=torch.bool)
        dyn = keep.clone()
        if not hasattr(model, "frm_num"):           # ... a dense stage-1 MPI is one static atlas (MPI.py:95-117)
            dyn = torch.zeros_like(keep)
    if quad_maps is not None:
        keep, dyn = check_quad_maps(quad_maps, keep, keep & dyn, own)
    faces = quad_faces(D, hv, wv)
    idx_s, atlas_s, uvs_s, uvf_s, (gh_s, gw_s) = _pack_tiles(stack, keep & ~dyn, 1, tile_texels, own)
    idx_d, atlas_d, uvs_d, uvf_d, (gh_d, gw_d) = _pack_tiles(stack, dyn, T, tile_texels, own)
    # atlas_full_*: the atlas size at FULL resolution -- what MPV.lod scales its tiles from (MPV.py:149-151); a model exported at a pyramid
    # level keeps the full tile size there (tile-exact models know it: tile_full), everything else is exported at the size it has
    full_hw = tuple(model.tile_full) if (own and getattr(model, "tile_full", None) is not None) else tuple(tile_texels)
    intrin_mpi = model.ref_intrin_mpi.detach().cpu().float()
    mh, mw = model.mpi_h, model.mpi_w
    verts = gen_mpi_vertices(mh, mw, intrin_mpi, hv, wv, model.planedepth.detach().cpu().float())
    if bool(getattr(model.args, "normalize_verts", False)):
        # the reference stores `_verts` divided by the plane depth under this flag and multiplies it back in its `verts` property (MPV.py:62-64)
        verts = (verts.reshape(D, -1, 3) / model.planedepth.detach().cpu().float().reshape(D, 1, 1)).reshape(verts.shape)
    if not hasattr(model, "frm_num") and not sparse:
        # a dense stage-1 MPI: the reference's MPMesh.state_dict() before sparsify_faces has no dynamic lists (MPI.py:207-221)
        return {"_verts": verts, "planedepth": model.planedepth.detach().cpu().clone(), "ref_extrin": model.ref_extrin.detach().cpu().clone(),
                "ref_intrin": model.ref_intrin.detach().cpu().clone(), "faces": faces[idx_s].reshape(-1, 3), "uvfaces": uvf_s, "uvs": uvs_s.cpu(),
                "atlas": atlas_s.cpu(), "self.is_sparse": False, "self.atlas_grid_h": gh_s, "self.atlas_grid_w": gw_s,
                "self.atlas_full_h": int(atlas_s.shape[-2]), "self.atlas_full_w": int(atlas_s.shape[-1])}
    return {
        "_verts": verts, "planedepth": model.planedepth.detach().cpu().clone(), "ref_extrin": model.ref_extrin.detach().cpu().clone(),
        "ref_intrin": model.ref_intrin.detach().cpu().clone(),
        "faces": faces[idx_s].reshape(-1, 3), "uvfaces": uvf_s, "uvs": uvs_s.cpu(), "atlas": atlas_s.cpu() if atlas_to_host else atlas_s,
        "faces_dyn": faces[idx_d].reshape(-1, 3), "uvfaces_dyn": uvf_d, "uvs_dyn": uvs_d.cpu(), "atlas_dyn": atlas_d.cpu() if atlas_to_host else atlas_d,
        "self.is_sparse": sparse, "self.has_dyn": True,
        "self.atlas_grid_h": gh_s, "self.atlas_grid_w": gw_s, "self.atlas_full_h": gh_s * full_hw[0] if gh_s else int(atlas_s.shape[-2]), "self.atlas_full_w": gw_s * full_hw[1] if gw_s else int(atlas_s.shape[-1]),
        "self.atlas_grid_dyn_h": gh_d, "self.atlas_grid_dyn_w": gw_d, "self.atlas_full_dyn_h": gh_d * full_hw[0] if gh_d else int(atlas_d.shape[-2]),
        "self.atlas_full_dyn_w": gw_d * full_hw[1] if gw_d else int(atlas_d.shape[-1]),
    }


# ---- assets -----------------------------------------------------------------------------------------------------------------
def normalize_uv(uv, h, w):
    """utils.py:403-407: flip v, [-1,1] -> [0,1], then to texel centres of an h x w texture."""
    uv = np.array(uv, dtype=np.float64, copy=True)
    uv[:, 1] = -uv[:, 1]
    uv = uv * 0.5 + 0.5
    return uv * np.array([w - 1, h - 1]) / np.array([w, h]) + 0.5 / np.array([w, h])


def _cull_unused(v, f):
    """utils.py:410-416."""
    ids = np.unique(f)
    old2new = -np.ones(len(v), dtype=np.int64)
    old2new[ids] = np.arange(len(ids))
    return v[ids], old2new[f]


def save_obj(path, verts, faces, uvs, uvfaces, rm_unused=True):
    """utils.py:419-435."""
    if rm_unused:
        verts, faces = _cull_unused(verts, faces)
        uvs, uvfaces = _cull_unused(uvs, uvfaces)
    with open(path, "w") as f:
        for p in verts:
            f.write(f"v {p[0]} {p[1]} {p[2]}\n")
        for uv in uvs:
            f.write(f"vt {uv[0]} {uv[1]}\n")
        for face, uvface in zip(faces + 1, uvfaces + 1):
            f.write(f"f {face[0]}/{uvface[0]} {face[1]}/{uvface[1]} {face[2]}/{uvface[2]}\n")
        f.write("\n")


def save_mesh(model, prefix, state=None):
    """MPV.py:306-323: the static and the dynamic mesh as OBJ files (returns the paths written)."""
    sd = reference_state_dict(model) if state is None else state
    out = []
    for faces_k, uvs_k, uvf_k, atlas_k, suffix in (("faces", "uvs", "uvfaces", "atlas", ".obj"), ("faces_dyn", "uvs_dyn", "uvfaces_dyn", "atlas_dyn", "_dyn.obj")):
        faces = sd[faces_k].numpy()
        if len(faces) == 0:
            continue
        uvs = normalize_uv(sd[uvs_k].numpy(), sd[atlas_k].shape[2], sd[atlas_k].shape[3])
        print(f"Saving to {prefix + suffix}: # v = {len(sd['_verts'])}, # f = {len(faces)}")
        save_obj(prefix + suffix, sd["_verts"].numpy(), faces, uvs, sd[uvf_k].numpy())
        out.append(prefix + suffix)
    return out


def write_png(path, img):
    """uint8 [H,W,3|4] -> PNG (zlib + CRC from the standard library; imageio is not in this image)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w, c = img.shape
    assert c in (3, 4)
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * c)], axis=1).tobytes()      # filter type 0 in front of every row

    def chunk(tag, data):
        body = tag + data
        return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6 if c == 4 else 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


@torch.no_grad()
def save_texture(model, prefix, state=None):
    """MPV.py:325-341: activated textures, static as one RGBA image, dynamic as rgb * alpha frames."""
    sd = reference_state_dict(model) if state is None else state
    out = []
    if len(sd["faces"]) > 0:
        t = sd["atlas"][0].permute(1, 2, 0)
        rgba = torch.cat([model.rgb_activate(t[..., :-1]), model.alpha_activate(t[..., -1:])], dim=-1)
        write_png(prefix + "_static.png", (rgba * 255).type(torch.uint8).numpy())
        out.append(prefix + "_static.png")
    if len(sd["faces_dyn"]) > 0:
        t = sd["atlas_dyn"].permute(0, 2, 3, 1)
        rgb = model.rgb_activate(t[..., :-1]) * model.alpha_activate(t[..., -1:])
        frames = (rgb * 255).type(torch.uint8).numpy()
        names = [f"{prefix}_dyn_{i:04d}.png" for i in range(len(frames))]
        # (zlib releases the interpreter lock: the T frames of a 2K x 4K dynamic atlas compress side by side -- 25 s -> a few for T = 50)
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1, len(frames)))) as ex:
            list(ex.map(write_png, names, frames))
        out.extend(names)
    return out


def _viewer_meta(poses, intrins, bds, frame_count, fps):
    """script_export_mesh.py:88-111: what the player needs to know about the cameras -- vertical field of view of the mean pinhole, depth range,
    the views' mean up axis (y flipped: the player's y points up), the point the spiral looks at (3 : 1 in inverse depth between 0.9 x near
    and 5 x far, as render_video.load_llff_poses) and how far the viewer may move per axis (0.8 x the largest camera offset)."""
    poses, intrins, bds = np.asarray(poses, dtype=np.float64), np.asarray(intrins, dtype=np.float64), np.asarray(bds, dtype=np.float64)
    up = poses[:, :3, 1].sum(0)
    up = up / np.linalg.norm(up)
    look_near, look_far = bds.min() * .9, bds.max() * 5.
    return {"fps": fps,
            "fov": float(np.degrees(2 * np.arctan(intrins[:, 1, 2].mean() / intrins[:, 0, 0].mean()))),
            "frame_count": int(frame_count),
            "near": float(bds.min()), "far": float(bds.max()),
            "up": [float(up[0]), float(-up[1]), float(up[2])],
            "lookat": [0, 0, float(1. / (.25 / look_near + .75 / look_far))],
            "limit": (np.abs(poses[:, :3, 3]).max(0) * 0.8).tolist()}


def _write_viewer_obj(path, sd):
    """geometry.obj of the package (script_export_mesh.py:155-184): the static mesh (vertex colour 1,0,0) and the dynamic mesh (0,1,0) in one
    file -- unused vertices dropped per mesh, UVs at texel centres of their own atlas, the dynamic indices shifted behind the static ones --
    with the faces sorted far to near by the depth of their first vertex (the player blends them in file order)."""
    verts = sd["_verts"].numpy().reshape(-1, 3)
    v_all, uv_all, f_all, uvf_all = [], [], [], []
    nv = nuv = 0
    for faces_k, uvs_k, uvf_k, atlas_k, colour in (("faces", "uvs", "uvfaces", "atlas", (1.0, 0.0, 0.0)),
                                                   ("faces_dyn", "uvs_dyn", "uvfaces_dyn", "atlas_dyn", (0.0, 1.0, 0.0))):
        faces = sd[faces_k].numpy().reshape(-1, 3)
        if len(faces) == 0:
            continue
        v, f = _cull_unused(verts, faces)
        uv, uvf = _cull_unused(normalize_uv(sd[uvs_k].numpy(), sd[atlas_k].shape[2], sd[atlas_k].shape[3]), sd[uvf_k].numpy().reshape(-1, 3))
        v_all.append(np.concatenate([v, np.broadcast_to(np.array(colour), v.shape)], axis=1))
        uv_all.append(uv)
        f_all.append(f + nv)
        uvf_all.append(uvf + nuv)
        nv, nuv = nv + len(v), nuv + len(uv)
    v_all, uv_all = np.concatenate(v_all), np.concatenate(uv_all)
    f_all, uvf_all = np.concatenate(f_all), np.concatenate(uvf_all)
    order = np.argsort(-v_all[f_all[:, 0], 2], kind="stable")
    with open(path, "w") as f:
        for p in v_all:
            f.write(f"v {p[0]} {p[1]} {p[2]} {p[3]} {p[4]} {p[5]}\n")
        for uv in uv_all:
            f.write(f"vt {uv[0]} {uv[1]}\n")
        for face, uvface in zip(f_all[order] + 1, uvf_all[order] + 1):
            f.write(f"f {face[0]}/{uvface[0]} {face[1]}/{uvface[1]} {face[2]}/{uvface[2]}\n")


@torch.no_grad()
def save_viewer_package(model, outdir, poses, intrins, bds, fps=25, quad_maps=None):
    """scripts/script_export_mesh.py:76-191: the viewer package of `model` (MPMeshVid, dense or sparsified) in `outdir` -- geometry.obj,
    static.png, dynamic/%04d.png, meta.json; poses [V,3,4] camera-to-world, intrins [V,3,3], bds (near, far) as render_video.load_llff_poses
    returns them.  The PNGs are the atlases of reference_state_dict(model) through baked.bake_texels: activated, times 255, clipped, truncated,
    straight RGBA -- the texels a player filters and baked.BakedMPV renders from.  Returns the paths written.
    quad_maps=(keep, dyn): the quads written are these (reference_state_dict; the maps of BakedPool.trimmed drop what never shows and write
    frozen dynamic quads once).  With them, a tile-exact model on the device has its atlases baked THERE (vl3d_bake_rgba8): its tiles are
    copied texel for texel, so the package holds the bytes of bake_pool(model) -- the bytes the maps were decided on.  Without the keyword
    nothing changes: the host bake, the model's own maps."""
    import json
    from concurrent.futures import ThreadPoolExecutor
    from .baked import bake_texels
    if hasattr(model, "_flush_deferred_updates"):
        model._flush_deferred_updates()
    param = model._param() if hasattr(model, "_param") else getattr(model, "stack", None)
    on_device = quad_maps is not None and getattr(model, "tile_own", None) is not None and param is not None and param.is_cuda
    sd = reference_state_dict(model) if quad_maps is None else reference_state_dict(model, quad_maps=quad_maps, atlas_to_host=not on_device)
    if "atlas_dyn" not in sd:
        raise RuntimeError("save_viewer_package: a video model (MPMeshVid) with its dynamic atlas")
    os.makedirs(os.path.join(outdir, "dynamic"), exist_ok=True)
    acts = (model.args.rgb_activate, model.args.alpha_activate)
    place = (lambda t: t.contiguous()) if on_device else (lambda t: t.cpu())      # the device rule where the texels lie, else the host rule
    static = bake_texels(place(sd["atlas"][0].permute(1, 2, 0).float()), *acts).cpu().numpy()
    frames = bake_texels(place(sd["atlas_dyn"].permute(0, 2, 3, 1).float()), *acts).cpu().numpy()
    if on_device:
        sd["atlas"], sd["atlas_dyn"] = sd["atlas"].cpu(), sd["atlas_dyn"].cpu()
    meta = _viewer_meta(poses, intrins, bds, len(frames), fps)
    out = [os.path.join(outdir, "meta.json"), os.path.join(outdir, "geometry.obj"), os.path.join(outdir, "static.png")]
    with open(out[0], "w") as f:
        f.write(json.dumps(meta, indent=4))
    _write_viewer_obj(out[1], sd)
    names = [os.path.join(outdir, "dynamic", f"{i:04d}.png") for i in range(len(frames))]
    with ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1, len(frames) + 1))) as ex:      # (zlib releases the interpreter lock)
        list(ex.map(write_png, [out[2]] + names, [static] + list(frames)))
    return out + names


# ---- reading a viewer package back ----------------------------------------------------------------------------------------------
def _png_chunks(path):
    """(IHDR fields (w, h, depth, colour, compression, filter, interlace), concatenated IDAT bytes) of a PNG file, every chunk's CRC checked."""
    b = open(path, "rb").read()
    if b[:8] != b"\x89PNG\r\n\x1a\n":
        raise RuntimeError(f"read_png: {path}: not a PNG file (signature)")
    pos, idat, hdr, ended = 8, [], None, False
    while pos + 12 <= len(b) and not ended:
        n, tag = struct.unpack(">I", b[pos:pos + 4])[0], b[pos + 4:pos + 8]
        if pos + 12 + n > len(b):
            raise RuntimeError(f"read_png: {path}: chunk {tag!r} runs past the end of the file")
        body = b[pos + 8:pos + 8 + n]
        if struct.unpack(">I", b[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + body) & 0xFFFFFFFF:
            raise RuntimeError(f"read_png: {path}: CRC mismatch in chunk {tag!r}")
        if tag == b"IHDR":
            if n != 13:
                raise RuntimeError(f"read_png: {path}: IHDR of {n} bytes")
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        ended = tag == b"IEND"
        pos += 12 + n
    if hdr is None or not ended:
        raise RuntimeError(f"read_png: {path}: no IHDR or no IEND chunk")
    return hdr, b"".join(idat)


def _png_check_header(path, hdr):
    w, h, depth, colour, comp, filt, interlace = hdr
    if depth != 8:
        raise RuntimeError(f"read_png: {path}: bit depth {depth}; 8-bit RGB / RGBA only")
    if colour not in (2, 6):
        raise RuntimeError(f"read_png: {path}: colour type {colour} (palette / grey); 8-bit RGB / RGBA only")
    if interlace != 0 or comp != 0 or filt != 0:
        raise RuntimeError(f"read_png: {path}: interlaced (or an unknown compression / filter method); non-interlaced only")
    if w == 0 or h == 0:
        raise RuntimeError(f"read_png: {path}: empty image")
    return w, h, 4 if colour == 6 else 3


def png_size(path):
    """(H, W, channels) of an 8-bit RGB / RGBA PNG from its header, without inflating it."""
    with open(path, "rb") as f:
        b = f.read(33)
    if len(b) < 33 or b[:8] != b"\x89PNG\r\n\x1a\n" or b[12:16] != b"IHDR":
        raise RuntimeError(f"read_png: {path}: not a PNG file (signature / IHDR)")
    if struct.unpack(">I", b[29:33])[0] != zlib.crc32(b[12:29]) & 0xFFFFFFFF:
        raise RuntimeError(f"read_png: {path}: CRC mismatch in chunk b'IHDR'")
    w, h, c = _png_check_header(path, struct.unpack(">IIBBBBB", b[16:29]))
    return h, w, c


def read_png(path):
    """8-bit RGB / RGBA PNG, non-interlaced, any number of IDAT chunks, all five filter types -> uint8 [H,W,3|4] (zlib + numpy: the inverse of
    write_png, and of any encoder's output in those formats).  Rows of filter type 0, 1 and 2 are undone with array operations (Sub is a
    running sum per channel, Up an add of the row above); Average and Paeth rows -- which write_png never emits -- take a plain loop per byte.
    A CRC mismatch, another bit depth, a palette and interlace are refused."""
    hdr, idat = _png_chunks(path)
    w, h, c = _png_check_header(path, hdr)
    try:
        raw = zlib.decompress(idat)
    except zlib.error as e:
        raise RuntimeError(f"read_png: {path}: {e}")
    if len(raw) != h * (1 + w * c):
        raise RuntimeError(f"read_png: {path}: {len(raw)} bytes of image data for {h} rows of {1 + w * c}")
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + w * c)
    ftype, data = rows[:, 0], rows[:, 1:]
    if not ftype.any():                                                                  # what write_png writes: nothing to undo
        return data.reshape(h, w, c).copy()
    if int(ftype.max()) > 4:
        raise RuntimeError(f"read_png: {path}: filter type {int(ftype.max())}")
    out = data.copy()
    sub = ftype == 1                                                                     # Sub: independent of the row above, all such rows at once
    if sub.any():
        out[sub] = np.cumsum(data[sub].reshape(-1, w, c), axis=1, dtype=np.uint8).reshape(-1, w * c)
    zero = np.zeros(w * c, dtype=np.uint8)
    for y in np.nonzero(ftype >= 2)[0].tolist():
        up = out[y - 1] if y > 0 else zero
        if ftype[y] == 2:
            out[y] = data[y] + up                                                        # (uint8 arithmetic wraps modulo 256)
            continue
        cur, upl, fl = bytearray(w * c), up.tolist(), data[y].tolist()
        for i in range(w * c):
            a = cur[i - c] if i >= c else 0
            if ftype[y] == 3:
                pred = (a + upl[i]) >> 1
            else:
                bb, cc = upl[i], (upl[i - c] if i >= c else 0)
                p = a + bb - cc
                pa, pb, pc = abs(p - a), abs(p - bb), abs(p - cc)
                pred = a if (pa <= pb and pa <= pc) else (bb if pb <= pc else cc)
            cur[i] = (fl[i] + pred) & 0xFF
        out[y] = np.frombuffer(bytes(cur), dtype=np.uint8)
    return out.reshape(h, w, c)


def _progression(q, what, where):
    """the values q (x / z or y / z of every vertex) on ONE arithmetic progression -> (step, origin, index of every value).  The step is the
    smallest positive difference between distinct values (values closer than 1e-4 of a first estimate are one grid line with float32 rounding),
    refitted over the whole span; the origin is the smallest value."""
    s = np.sort(q)
    diffs = np.diff(s)
    span = s[-1] - s[0]
    big = diffs[diffs > 1e-6 * max(span, np.abs(s).max(), 1e-30)]
    if len(big) == 0:
        raise RuntimeError(f"read_viewer_package: {where}: the {what} of all vertices are one value: no vertex grid (rule: x / z and y / z lie on an arithmetic progression)")
    step = float(big.min())
    origin = float(s[0])
    n = int(round(span / step))
    step = span / n                                      # refit: the whole span over its number of steps
    idx = np.rint((q - origin) / step)
    off = np.abs(q - (origin + idx * step)).max() / step
    if off > 1e-3:
        raise RuntimeError(f"read_viewer_package: {where}: a vertex lies {off:.3g} steps off the arithmetic progression of the {what} "
                           "(rule: x / z and y / z of all vertices lie on one arithmetic progression per axis)")
    return step, origin, idx.astype(np.int64)


def read_viewer_package(dir):
    """The viewer package save_viewer_package writes, read back from its four artefacts alone -- no checkpoint, no training arguments:
    meta.json, geometry.obj (`v x y z r g b`, `vt u v`, `f a/b c/d e/f`; vertex colour (1,0,0) = static mesh, (0,1,0) = dynamic mesh; two
    consecutive faces over the same four uv corners = one quad) and the sizes of static.png / dynamic/%04d.png.  The PNGs' texels are NOT read
    here (baked.open_viewer_package decodes them on a thread pool).  -> dict:
      planedepth [D] float32 (the distinct vertex depths, ascending);  step, origin: (x, y) of the progression x / z, y / z of the vertex grid
      (gen_mpi_vertices: a linspace grid through a pinhole);  quad_keep, quad_dyn [D,QH,QW] bool over the bounding box of the quads present;
      tile_src [D,QH,QW] int32 = -1 (culled) | k << 1 | dynamic, k the tile's row-major index in its atlas;  tile (th, tw);
      grid_w (static, dynamic atlas grid widths; 0 for an empty mesh), atlas_hw ((As_h, As_w), (Ad_h, Ad_w); (0, 0) for an empty mesh),
      static_path, dynamic_paths, frame_count, fps, meta.
    Whatever does not fit the layout is refused with the rule it breaks."""
    import json
    who = f"read_viewer_package: {dir}"
    for name in ("meta.json", "geometry.obj", "static.png"):
        if not os.path.isfile(os.path.join(dir, name)):
            raise RuntimeError(f"{who}: {name} is missing (rule: a package is meta.json, geometry.obj, static.png and dynamic/%04d.png)")
    meta = json.load(open(os.path.join(dir, "meta.json")))
    want = ("fps", "fov", "frame_count", "near", "far", "up", "lookat", "limit")
    if sorted(meta) != sorted(want):
        raise RuntimeError(f"{who}: meta.json holds {sorted(meta)} (rule: the keys of the package's meta.json are {sorted(want)})")
    T = int(meta["frame_count"])
    # ---- the PNGs: names, count, sizes
    ddir = os.path.join(dir, "dynamic")
    have = sorted(f for f in os.listdir(ddir) if f.endswith(".png")) if os.path.isdir(ddir) else []
    if T < 1 or have != [f"{i:04d}.png" for i in range(T)]:
        raise RuntimeError(f"{who}: dynamic/ holds {len(have)} PNG files, meta.json says frame_count = {T} "
                           "(rule: dynamic/0000.png .. one file per frame, their count equal to frame_count)")
    dyn_paths = [os.path.join(ddir, f) for f in have]
    sizes = {png_size(p) for p in dyn_paths}
    if len(sizes) != 1:
        raise RuntimeError(f"{who}: the dynamic frames have the sizes {sorted(sizes)} (rule: every PNG in dynamic/ has one size)")
    static_path = os.path.join(dir, "static.png")
    hw = {0: png_size(static_path), 1: sizes.pop()}
    if hw[0][2] != 4 or hw[1][2] != 4:
        raise RuntimeError(f"{who}: the atlases must be RGBA (rule: straight RGBA8 tiles)")
    # ---- geometry.obj
    v, vt, f = [], [], []
    for line in open(os.path.join(dir, "geometry.obj")):
        p = line.split()
        if not p:
            continue
        if p[0] == "v" and len(p) == 7:
            v.append([float(x) for x in p[1:]])
        elif p[0] == "vt" and len(p) == 3:
            vt.append([float(x) for x in p[1:]])
        elif p[0] == "f" and len(p) == 4:
            f.append([[int(i) for i in c.split("/")] for c in p[1:]])
        else:
            raise RuntimeError(f"{who}: geometry.obj line {line.strip()!r} (rule: `v x y z r g b`, `vt u v`, `f a/b c/d e/f`)")
    if not f or len(f) % 2:
        raise RuntimeError(f"{who}: {len(f)} faces (rule: two consecutive faces form one quad)")
    v, vt, f = np.array(v, dtype=np.float64), np.array(vt, dtype=np.float64), np.array(f, dtype=np.int64) - 1
    if f.min() < 0 or f[..., 0].max() >= len(v) or f[..., 1].max() >= len(vt):
        raise RuntimeError(f"{who}: a face index outside the vertex / uv lists")
    red, green = (v[:, 3:] == [1, 0, 0]).all(1), (v[:, 3:] == [0, 1, 0]).all(1)
    if not (red | green).all():
        raise RuntimeError(f"{who}: a vertex colour that is neither (1,0,0) nor (0,1,0) (rule: vertex colour marks the static / the dynamic mesh)")
    z = v[:, 2]
    if (z == 1).all():
        raise RuntimeError(f"{who}: every vertex has z == 1: geometry written with normalize_verts carries no plane depths "
                           "(rule: the plane of a vertex is its z)")
    if not (z > 0).all():
        raise RuntimeError(f"{who}: a vertex with z <= 0 (rule: the plane of a vertex is its z)")
    planedepth = np.unique(z.astype(np.float32))
    d_of_v = np.searchsorted(planedepth, z.astype(np.float32))
    sx, ox, ix = _progression(v[:, 0] / z, "x / z", dir)
    sy, oy, iy = _progression(v[:, 1] / z, "y / z", dir)
    # ---- quads: faces (2i, 2i + 1) = triangles (c0, c1, c3), (c3, c2, c0) of the corners c0 .. c3
    f1, f2 = f[0::2], f[1::2]
    if not ((f2[:, 0] == f1[:, 2]).all() and (f2[:, 2] == f1[:, 0]).all()):
        raise RuntimeError(f"{who}: faces 2i and 2i + 1 do not share their diagonal (rule: two consecutive faces with the same four uv corners form one quad)")
    qv = np.concatenate([f1[..., 0], f2[:, 1:2, 0]], axis=1)            # n,4 vertex ids: c0, c1, c3, c2
    quv = vt[np.concatenate([f1[..., 1], f2[:, 1:2, 1]], axis=1)]       # n,4,2
    is_dyn = green[qv[:, 0]]
    if not ((green[qv] == is_dyn[:, None]).all() and (d_of_v[qv] == d_of_v[qv[:, :1]]).all()):
        raise RuntimeError(f"{who}: a quad whose vertices differ in colour or depth (rule: a quad lies in one plane of one mesh)")
    qx, qy, qd = ix[qv].min(1), iy[qv].min(1), d_of_v[qv[:, 0]]
    if not ((ix[qv].max(1) - qx == 1).all() and (iy[qv].max(1) - qy == 1).all()):
        raise RuntimeError(f"{who}: a quad that does not span one step of the vertex grid per axis (rule: the grid index of a vertex is round((q - origin) / step))")
    D, QH, QW = len(planedepth), int(qy.max()) + 1, int(qx.max()) + 1
    flat = (qd * QH + qy) * QW + qx
    if len(np.unique(flat)) != len(flat):
        raise RuntimeError(f"{who}: two quads at one (plane, row, column) (rule: a quad is static or dynamic, once)")
    # ---- tiles: invert normalize_uv on the first uv corner (texel centres of an Ah x Aw atlas, v flipped)
    tile, grid_w, k_of = None, [0, 0], np.zeros(len(flat), dtype=np.int64)
    for mesh, name in ((0, "static.png"), (1, "dynamic/%04d.png")):
        sel = is_dyn == bool(mesh)
        if not sel.any():
            hw[mesh] = (0, 0, 4)                                        # an empty mesh: its atlas file is 1 x 1 and ignored
            continue
        Ah, Aw = hw[mesh][:2]
        uv = quv[sel]
        du, dv = uv[..., 0].max(1) - uv[..., 0].min(1), uv[..., 1].max(1) - uv[..., 1].min(1)
        tw, th = int(round(float(np.median(du)) * Aw)) + 1, int(round(float(np.median(dv)) * Ah)) + 1      # uv extent of a quad = (tw - 1) / Aw
        if tile is not None and tile != (th, tw):
            raise RuntimeError(f"{who}: static tiles of {tile}, dynamic tiles of {(th, tw)} texels (rule: both atlases agree on the tile size)")
        tile = (th, tw)
        if th < 2 or tw < 2 or Ah % th or Aw % tw:
            raise RuntimeError(f"{who}: {name} is {Ah} x {Aw}, the tiles are {th} x {tw} (rule: the atlas size is a multiple of the tile size)")
        col, row = uv[:, 0, 0] * Aw - 0.5, Ah - 0.5 - uv[:, 0, 1] * Ah
        ci, ri = np.rint(col).astype(np.int64), np.rint(row).astype(np.int64)
        ok = (np.abs(du * Aw + 1 - tw) < 1e-2) & (np.abs(dv * Ah + 1 - th) < 1e-2) & (np.abs(col - ci) < 1e-2) & (np.abs(row - ri) < 1e-2) \
            & (ci % tw == 0) & (ri % th == 0) & (ci >= 0) & (ri >= 0) & (ci < Aw) & (ri < Ah) \
            & (np.abs(uv[:, 0, 0] - uv[..., 0].min(1)) < 1e-9) & (np.abs(uv[:, 0, 1] - uv[..., 1].max(1)) < 1e-9)
        if not ok.all():
            raise RuntimeError(f"{who}: the uv corners of a quad do not name a tile of {name} (rule: the first uv corner, through the inverse of "
                               "normalize_uv, is the first texel of tile k; a quad spans (tw - 1) / Aw)")
        grid_w[mesh] = Aw // tw
        k_of[sel] = (ri // th) * grid_w[mesh] + ci // tw
    keep = np.zeros(D * QH * QW, dtype=bool)
    dyn = np.zeros(D * QH * QW, dtype=bool)
    src = np.full(D * QH * QW, -1, dtype=np.int32)
    keep[flat], dyn[flat], src[flat] = True, is_dyn, (k_of << 1 | is_dyn).astype(np.int32)
    return {"planedepth": planedepth, "step": (sx, sy), "origin": (ox, oy),
            "quad_keep": torch.from_numpy(keep.reshape(D, QH, QW)), "quad_dyn": torch.from_numpy(dyn.reshape(D, QH, QW)),
            "tile_src": torch.from_numpy(src.reshape(D, QH, QW)), "tile": tile, "grid_w": tuple(grid_w),
            "atlas_hw": (tuple(hw[0][:2]), tuple(hw[1][:2])), "static_path": static_path, "dynamic_paths": dyn_paths,
            "frame_count": T, "fps": meta["fps"], "meta": meta}
