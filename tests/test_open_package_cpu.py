"""Reading a viewer package back (videoloop3d_amd/export.read_png, read_viewer_package; baked.package_camera): the files
save_viewer_package wrote give back the quad maps, the plane depths, the tile of every quad and a camera that samples where the model's
does.  CPU only; the model is the one of tests/test_baked_package_cpu.py, rebuilt here."""
import json
import os
import shutil
import struct
import types
import zlib

import numpy as np
import pytest
import torch

from package_models import lattice_coords

T = 3
K = np.array([[50., 0, 30], [0, 50., 20], [0, 0, 1]])


def _args(**kw):
    a = dict(mpi_h_scale=1.0, mpi_w_scale=1.0, mpi_d=3, rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid",
             bg_color="", learn_loop_mask=True, mpi_h_verts=5, mpi_w_verts=7, sparsify_rmfirstlayer=0, atlas_grid_h=1,
             mpv_frm_num=T, mpv_isloop=True, init_std=0.5, scale_invariant=True, fp16=False,
             swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1)
    a.update(kw)
    return types.SimpleNamespace(**a)


def _model(H=41, W=61, **kw):
    """a sparsified MPMeshVid on the host: 3 planes of 4 x 6 quads of 10 x 10 texels, about 60 % kept, plane 1 culled, half of the kept dynamic."""
    from videoloop3d_amd import tiles
    from videoloop3d_amd.MPV import MPMeshVid
    torch.manual_seed(4)
    m = MPMeshVid(_args(**kw), H, W, np.eye(4), K, 1.0, 100.0)
    keep = torch.rand(3, 4, 6) < 0.6
    keep[1] = False
    dyn = keep & (torch.rand(3, 4, 6) < 0.5)
    with torch.no_grad():
        m.stack.uniform_(-3.0, 3.0)
        tiles.cull_stack_(m.stack.data, keep)
    m.register_buffer("quad_keep", keep)
    m.register_buffer("quad_dyn", dyn)
    m.is_sparse = m.has_dyn = True
    return m


def _cameras():
    """three camera-to-world poses around the origin, their pinhole intrinsics, depth bounds."""
    poses = np.tile(np.eye(4, dtype=np.float32)[None, :3], (3, 1, 1))
    poses[:, :, 3] = np.array([[-0.2, 0.05, 0.0], [0.0, -0.1, 0.02], [0.3, 0.0, -0.05]], dtype=np.float32)
    return poses, np.tile(K.astype(np.float32)[None], (3, 1, 1)), np.array([1.0, 100.0], dtype=np.float32)


@pytest.fixture(scope="module")
def package(tmp_path_factory):
    from videoloop3d_amd.export import read_viewer_package, save_viewer_package
    m = _model()
    # the condition on the input: the kept quads reach all four sides of the quad grid (the bounding box of the quads present is the grid),
    # and the package has static and dynamic quads
    keep, dyn = m.quad_keep, m.quad_dyn
    rows, cols = keep.any(0).any(1), keep.any(0).any(0)
    assert rows[0] and rows[-1] and cols[0] and cols[-1]
    assert bool((keep & ~dyn).any()) and bool(dyn.any())
    out = str(tmp_path_factory.mktemp("viewer"))
    save_viewer_package(m, out, *_cameras())
    return m, out, read_viewer_package(out)


def _chunk(tag, data):
    body = tag + data
    return struct.pack(">I", len(data)) + body + struct.pack(">I", zlib.crc32(body) & 0xFFFFFFFF)


# ---- read_png ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 7, 4), (4, 3, 3)])
def test_read_png_round_trip(tmp_path, shape):
    from videoloop3d_amd.export import png_size, read_png, write_png
    img = np.random.default_rng(3).integers(0, 256, shape, dtype=np.uint8)
    p = str(tmp_path / "a.png")
    write_png(p, img)
    got = read_png(p)
    assert got.dtype == np.uint8 and np.array_equal(got, img)
    assert png_size(p) == shape


def _filtered_png(img):
    """6 rows of RGBA, row y written with PNG filter type min(y, 4) (rows 0-4: None, Sub, Up, Average, Paeth; row 5 Paeth again), by the
    definitions of the PNG specification, byte by byte; the stream split over two IDAT chunks."""
    h, w, c = img.shape
    raw = bytearray()
    for y in range(h):
        ft = min(y, 4)
        cur = img[y].reshape(-1).astype(int).tolist()
        up = img[y - 1].reshape(-1).astype(int).tolist() if y else [0] * (w * c)
        raw.append(ft)
        for i in range(w * c):
            a = cur[i - c] if i >= c else 0
            b, cc = up[i], (up[i - c] if i >= c else 0)
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            else:
                p = a + b - cc
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
            raw.append((cur[i] - pred) & 0xFF)
    z = zlib.compress(bytes(raw), 6)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + _chunk(b"IDAT", z[:len(z) // 2])
            + _chunk(b"IDAT", z[len(z) // 2:]) + _chunk(b"IEND", b""))


def test_read_png_all_filter_types_two_idat_chunks(tmp_path):
    from videoloop3d_amd.export import read_png
    img = np.random.default_rng(5).integers(0, 256, (6, 5, 4), dtype=np.uint8)
    p = tmp_path / "f.png"
    p.write_bytes(_filtered_png(img))
    assert np.array_equal(read_png(str(p)), img)


def test_read_png_refusals(tmp_path):
    from videoloop3d_amd.export import read_png, write_png
    img = np.random.default_rng(6).integers(0, 256, (4, 4, 4), dtype=np.uint8)
    p = str(tmp_path / "a.png")
    write_png(p, img)
    b = bytearray(open(p, "rb").read())
    b[-13] ^= 0x01                                             # the last byte of the IDAT chunk's CRC (IEND is the final 12 bytes)
    bad = tmp_path / "crc.png"
    bad.write_bytes(bytes(b))
    with pytest.raises(RuntimeError, match=r"crc\.png.*CRC"):
        read_png(str(bad))
    for name, hdr in (("depth16", (4, 4, 16, 6, 0, 0, 0)), ("palette", (4, 4, 8, 3, 0, 0, 0)), ("interlaced", (4, 4, 8, 6, 0, 0, 1))):
        q = tmp_path / f"{name}.png"
        q.write_bytes(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", *hdr)) + _chunk(b"IDAT", zlib.compress(b"\0" * 68)) + _chunk(b"IEND", b""))
        with pytest.raises(RuntimeError, match=name):
            read_png(str(q))


# ---- read_viewer_package -----------------------------------------------------------------------------------------------------------
def test_package_maps_depths_and_tile(package):
    from videoloop3d_amd.export import reference_state_dict
    m, out, pk = package
    planes = m.quad_keep.flatten(1).any(1).nonzero()[:, 0]
    assert planes.tolist() == [0, 2]
    assert pk["quad_keep"].dtype == torch.bool and torch.equal(pk["quad_keep"], m.quad_keep[planes])
    assert pk["quad_dyn"].dtype == torch.bool and torch.equal(pk["quad_dyn"], m.quad_dyn[planes])
    assert np.array_equal(pk["planedepth"], m.planedepth[planes].numpy())
    sd = reference_state_dict(m)
    tile = (sd["atlas"].shape[2] // sd["self.atlas_grid_h"], sd["atlas"].shape[3] // sd["self.atlas_grid_w"])
    assert tile == (11, 11) and pk["tile"] == tile
    assert pk["grid_w"] == (sd["self.atlas_grid_w"], sd["self.atlas_grid_dyn_w"])
    assert pk["atlas_hw"] == (tuple(sd["atlas"].shape[2:]), tuple(sd["atlas_dyn"].shape[2:]))
    meta = json.load(open(os.path.join(out, "meta.json")))
    assert pk["meta"] == meta and pk["frame_count"] == T and pk["fps"] == 25 and len(pk["dynamic_paths"]) == T
    ts = pk["tile_src"]
    assert ts.dtype == torch.int32 and torch.equal(ts >= 0, pk["quad_keep"]) and torch.equal((ts >= 0) & ((ts & 1) == 1), pk["quad_dyn"])


@pytest.mark.parametrize("dynamic", ["none", "all"])
def test_package_with_one_mesh_only(tmp_path, dynamic):
    """no dynamic quads, or no static quads: the empty mesh's atlas file is 1 x 1, the reader reports it as (0, 0) with a grid of 0 tiles, and
    baked.atlas_tile_map accepts the map (every k is checked against the other grid only; the empty atlas travels as NULL)."""
    from videoloop3d_amd.baked import atlas_tile_map
    from videoloop3d_amd.export import png_size, read_viewer_package, save_viewer_package
    from videoloop3d_amd.packed import PackedLayout
    m = _model()
    m.quad_dyn.copy_(m.quad_keep if dynamic == "all" else torch.zeros_like(m.quad_keep))
    save_viewer_package(m, str(tmp_path), *_cameras())
    pk = read_viewer_package(str(tmp_path))
    e = 0 if dynamic == "all" else 1                          # the empty mesh
    assert png_size(pk["static_path"] if e == 0 else pk["dynamic_paths"][0])[:2] == (1, 1)
    assert pk["atlas_hw"][e] == (0, 0) and pk["grid_w"][e] == 0 and pk["atlas_hw"][1 - e][0] > 0
    planes = m.quad_keep.flatten(1).any(1).nonzero()[:, 0]
    assert torch.equal(pk["quad_keep"], m.quad_keep[planes]) and torch.equal(pk["quad_dyn"], m.quad_dyn[planes])
    ts = pk["tile_src"]
    assert torch.equal(ts >= 0, pk["quad_keep"]) and bool(((ts[ts >= 0] & 1) == 1 - e).all())
    assert sorted((ts[ts >= 0] >> 1).tolist()) == list(range(int(pk["quad_keep"].sum())))
    (th, tw), (D, QH, QW) = pk["tile"], ts.shape
    lay = PackedLayout(pk["quad_keep"], pk["quad_dyn"], pk["frame_count"], QH * th, QW * tw, (th, tw))
    tm = atlas_tile_map(ts, lay, *pk["atlas_hw"])
    assert (tm.static_hw, tm.dyn_hw)[e] == (0, 0) and (lay.n_static, lay.n_dynamic)[e] == 0 and (lay.n_static, lay.n_dynamic)[1 - e] > 0
    with pytest.raises(RuntimeError, match="outside the .* atlas grid"):      # a tile that names the empty atlas is refused on the host
        bad = ts.clone()
        bad[ts >= 0] ^= 1
        atlas_tile_map(bad, lay, *pk["atlas_hw"])


def test_tile_src_points_at_the_quads_texels(package):
    """every tile_src entry names the tile whose PNG texels are bake_texels of the state dict's tile of that quad."""
    from videoloop3d_amd.baked import bake_texels
    from videoloop3d_amd.export import read_png, reference_state_dict
    m, out, pk = package
    sd = reference_state_dict(m)
    th, tw = pk["tile"]
    planes = m.quad_keep.flatten(1).any(1).nonzero()[:, 0].tolist()
    pngs = {0: read_png(pk["static_path"]), 1: read_png(pk["dynamic_paths"][T - 1])}
    n = 0
    for mesh, mask, atlas in ((0, m.quad_keep & ~m.quad_dyn, sd["atlas"][0]), (1, m.quad_dyn, sd["atlas_dyn"][T - 1])):
        baked = bake_texels(atlas.permute(1, 2, 0).float(), "sigmoid", "sigmoid").numpy()          # Ah,Aw,4
        gw_model = atlas.shape[2] // tw
        order = mask.reshape(-1).nonzero()[:, 0].tolist()                                          # the state dict's tile order: quads (d, qy, qx) ascending
        for k_model, flat in enumerate(order):
            d, rem = divmod(flat, 4 * 6)
            qy, qx = divmod(rem, 6)
            src = int(pk["tile_src"][planes.index(d), qy, qx])
            assert src >= 0 and (src & 1) == mesh
            k = src >> 1
            gw = pk["grid_w"][mesh]
            got = pngs[mesh][(k // gw) * th:(k // gw + 1) * th, (k % gw) * tw:(k % gw + 1) * tw]
            want = baked[(k_model // gw_model) * th:(k_model // gw_model + 1) * th, (k_model % gw_model) * tw:(k_model % gw_model + 1) * tw]
            assert np.array_equal(got, want), (mesh, d, qy, qx)
            n += 1
    assert n == int(m.quad_keep.sum())


def test_opened_camera_samples_where_the_models_does(package):
    """fp64: a 9 x 13 grid of target pixels of three poses through (a) the model's plane_homographies and spec and (b) the opened camera's
    land on the same lattice coordinate to 1e-3 (fp32 eps 6e-8 x coordinates below 2e3 x a few operations on the OBJ's float32 vertices).
    The model's texel pitch is one lattice unit: a quad spans 10 texels, its exported tile of 11 texels 10 lattice units."""
    from videoloop3d_amd.baked import _Camera, package_camera
    m, _, pk = package
    cam, spec = package_camera(pk)
    assert spec.tile == (11, 11) and spec.scale == (1.0, 1.0) and spec.offset == (0.0, 0.0) and spec.pixel_center == 0.5
    assert spec.coord_mode == "affine" and spec.border == "hardcut" and (spec.rgb_act, spec.alpha_act) == ("none", "none")
    assert cam.plane_homographies.__func__ is _Camera.plane_homographies and torch.equal(cam.ref_extrin, torch.eye(4, dtype=torch.float64))
    poses, intrins, _ = _cameras()
    c2w = np.tile(np.eye(4, dtype=np.float32)[None], (3, 1, 1))
    c2w[:, :3] = poses
    ext = np.linalg.inv(c2w)
    # the 9 x 13 grid: a view of 9 x 13 pixels whose pinhole covers the model's 41 x 61 view
    Kv = intrins.copy()
    Kv[:, 0] *= 13 / 61
    Kv[:, 1] *= 9 / 41
    planes = m.quad_keep.flatten(1).any(1).nonzero()[:, 0].tolist()
    a = lattice_coords(_Camera(m), m.spec, ext, Kv, 9, 13, planes)
    b = lattice_coords(cam, spec, ext, Kv, 9, 13)
    assert a.shape == b.shape == (3, 2, 9, 13, 2)
    err = float(np.abs(a - b).max())
    print(f"max |model - opened| = {err:.3g} lattice units (coordinates up to {float(np.abs(a).max()):.3g})")
    assert float(np.abs(a).max()) > 30 and err <= 1e-3


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _copy(package, tmp_path):
    dst = str(tmp_path / "pkg")
    shutil.copytree(package[1], dst)
    return dst


def test_refuses_a_missing_dynamic_frame(package, tmp_path):
    from videoloop3d_amd.export import read_viewer_package
    d = _copy(package, tmp_path)
    os.remove(os.path.join(d, "dynamic", "0001.png"))
    with pytest.raises(RuntimeError, match="count equal to frame_count"):
        read_viewer_package(d)


def test_refuses_two_dynamic_sizes(package, tmp_path):
    from videoloop3d_amd.export import read_png, read_viewer_package, write_png
    d = _copy(package, tmp_path)
    p = os.path.join(d, "dynamic", "0002.png")
    write_png(p, read_png(p)[:, :-11])
    with pytest.raises(RuntimeError, match="every PNG in dynamic/ has one size"):
        read_viewer_package(d)


def test_refuses_an_atlas_that_is_no_multiple_of_the_tile(package, tmp_path):
    from videoloop3d_amd.export import read_png, read_viewer_package, write_png
    d = _copy(package, tmp_path)
    p = os.path.join(d, "static.png")
    write_png(p, read_png(p)[:, :-1])
    with pytest.raises(RuntimeError, match="multiple of the tile size"):
        read_viewer_package(d)


def test_refuses_a_vertex_off_the_progression(package, tmp_path):
    from videoloop3d_amd.export import read_viewer_package
    d = _copy(package, tmp_path)
    p = os.path.join(d, "geometry.obj")
    lines = open(p).read().split("\n")
    i = next(j for j, l in enumerate(lines) if l.startswith("v ") and float(l.split()[1]) != 0.0)
    f = lines[i].split()
    f[1] = repr(float(f[1]) * 1.013)
    lines[i] = " ".join(f)
    open(p, "w").write("\n".join(lines))
    with pytest.raises(RuntimeError, match="arithmetic progression"):
        read_viewer_package(d)


def test_refuses_normalize_verts_geometry(tmp_path):
    from videoloop3d_amd.export import read_viewer_package, save_viewer_package
    m = _model(normalize_verts=True)
    d = str(tmp_path / "nv")
    save_viewer_package(m, d, *_cameras())
    with pytest.raises(RuntimeError, match="normalize_verts"):
        read_viewer_package(d)
