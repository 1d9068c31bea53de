"""Opening a viewer package on the MI355X (baked.open_viewer_package, vl3d_pool_from_atlas_rgba8): the files save_viewer_package wrote come
back as a BakedPool with the bytes of bake_pool(model) -- storage, block table, and the display frames along a camera path -- and the
package's own camera renders the in-process pool's frames to within one level.

Two tile-exact models, 6 frames each: tests/baked_models.pool_model (6 planes, plane 3 empty, 4 x 6 tiles of 8 x 8: tiles = blocks) and one of
5 x 7 tiles of 6 x 10 texels (30 x 70 texels: tiles straddle the 8 x 8 blocks, the last block row is ragged, blocks are shared by static,
dynamic and culled tiles).  A package does not hold planes without quads: the in-process side is compared on the planes that have some."""
import types

import numpy as np
import pytest
import torch

import baked_models as BM
import package_models as PM
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu

BG = "0.2#0.4#0.6"


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def straddling_model(dev, bg_color, dynamic="some"):
    """pool_model's recipe on 5 planes of 5 x 7 tiles of 6 x 10 texels (30 x 70): every plane has quads, the kept quads reach all four sides.
    dynamic: "some" of the kept quads, "none" (the package's dynamic mesh is empty) or "all" (its static mesh is)."""
    from videoloop3d_amd import tiles
    from videoloop3d_amd.MPV import MPMeshVid
    Hm, Wm, Dm, Tm, qh, qw, th, tw = 36, 64, 5, 6, 5, 7, 6, 10
    K = np.array([[0.9 * Wm, 0, Wm / 2], [0, 0.9 * Wm, Hm / 2], [0, 0, 1]])
    args = types.SimpleNamespace(mpv_frm_num=Tm, mpv_isloop=True, mpi_h_scale=1.1, mpi_w_scale=1.1, mpi_d=Dm, atlas_grid_h=2, init_std=0.5,
                                 rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color=bg_color, scale_invariant=True,
                                 fp16=False, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1, sparsity_loss_weight=0.0,
                                 rgb_smooth_loss_weight=0.0, a_smooth_loss_weight=0.0, density_loss_weight=0.0, d_smooth_loss_weight=0.0,
                                 optimizer="adam", lrate=0.1, lrate_decay=30, mpi_h_verts=qh + 1, mpi_w_verts=qw + 1)
    model = MPMeshVid(args, Hm, Wm, np.eye(4), K, 1.0, 100.0)
    keep = synth.hash_uniform((Dm, qh, qw), seed=41) < 0.5
    dyn = keep & (synth.hash_uniform((Dm, qh, qw), seed=42) < {"some": 0.4, "none": -1.0, "all": 2.0}[dynamic])
    stack = synth.make_plane_stack(Dm, Tm, qh * th, qw * tw, seed=9, alpha_bias=0.0) * 0.8
    stack = torch.where(tiles.quad_to_texel_mask(dyn, qh * th, qw * tw, (th, tw))[:, None, :, :, None], stack, stack[:, :1])
    stack = torch.where(tiles.quad_to_texel_mask(keep, qh * th, qw * tw, (th, tw))[:, None, :, :, None], stack,
                        torch.tensor([0.0, 0.0, 0.0, tiles.CULLED_ALPHA]))
    model.init_from_mpi({"ref_extrin": model.ref_extrin, "ref_intrin": model.ref_intrin, "planedepth": model.planedepth, "stack": stack,
                         "quad_keep": keep, "quad_dyn": dyn, "self.is_sparse": True, "self.has_dyn": True, "self.tile_own": (th, tw),
                         "self.tile_full": (th, tw)})
    model = model.to(dev).eval()
    assert model.tile_own == (th, tw) and model.stack.shape == (Dm, Tm, qh * th, qw * tw, 4)
    return model, Hm, Wm, K


@pytest.fixture(scope="module", params=["tiles8x8", "tiles6x10"])
def case(request, dev, tmp_path_factory):
    """the model, its in-process pool, its package on disk and the package opened again"""
    from videoloop3d_amd.baked import bake_pool, culled_texel_rgba8, open_viewer_package
    from videoloop3d_amd.export import save_viewer_package
    model, Hm, Wm, K = BM.pool_model(dev, BG, exact=True) if request.param == "tiles8x8" else straddling_model(dev, BG)
    keep = model.quad_keep.cpu()
    # the condition on the input: the kept quads reach all four sides of the quad grid, static and dynamic quads exist
    rows, cols = keep.any(0).any(1), keep.any(0).any(0)
    assert rows[0] and rows[-1] and cols[0] and cols[-1]
    assert bool((keep & ~model.quad_dyn.cpu()).any()) and bool(model.quad_dyn.any())
    planes = keep.flatten(1).any(1).nonzero()[:, 0].tolist()
    out = str(tmp_path_factory.mktemp("pkg_" + request.param))
    poses = np.tile(np.eye(4, dtype=np.float32)[None, :3], (2, 1, 1))
    save_viewer_package(model, out, poses, np.tile(K.astype(np.float32)[None], (2, 1, 1)), np.array([1.0, 100.0]))
    culled = culled_texel_rgba8("sigmoid", "sigmoid")
    opened = open_viewer_package(out, dev, bg_color=BG, culled_rgba8=culled)
    return types.SimpleNamespace(model=model, H=Hm, W=Wm, K=K.astype(np.float32), dir=out, planes=planes, culled=culled, opened=opened,
                                 inproc=bake_pool(model), T=int(model.frm_num))


def test_storage_bit_for_bit(case):
    o, p = case.opened, case.inproc
    assert o.frm_num == case.T and o.layout.tile == tuple(case.model.tile_own) and o.layout.D == len(case.planes)
    assert torch.equal(o.quad_keep, p.quad_keep[case.planes])
    assert torch.equal(o.layout.blocks, p.layout.blocks[case.planes])
    assert o.layout.n_slots == p.layout.n_slots and o.pool.shape == p.pool.shape
    assert torch.equal(o.unpack_frames(range(case.T)), p.unpack_frames(range(case.T))[case.planes])
    # (the pools themselves differ where a ragged block reaches past the plane: 0 here, the bake of an unset float texel in bake_pool's; no
    # render and no unpack reads those texels.  test_kernel_against_plain_torch compares whole pools.)


@pytest.mark.parametrize("dynamic", ["none", "all"])
def test_package_with_one_mesh_only(dev, tmp_path, dynamic):
    """a package without dynamic quads (one scatter call, the dynamic atlas NULL) and one without static quads (the static atlas NULL): the
    atlas file of the empty mesh is 1 x 1 and ignored, and the opened storage is bake_pool(model)'s."""
    from videoloop3d_amd.baked import bake_pool, culled_texel_rgba8, open_viewer_package
    from videoloop3d_amd.export import png_size, read_viewer_package, save_viewer_package
    model, _, _, K = straddling_model(dev, BG, dynamic)
    assert int(model.quad_dyn.sum()) == (0 if dynamic == "none" else int(model.quad_keep.sum())) and bool(model.quad_keep.any(0).any())
    poses = np.tile(np.eye(4, dtype=np.float32)[None, :3], (2, 1, 1))
    save_viewer_package(model, str(tmp_path), poses, np.tile(K.astype(np.float32)[None], (2, 1, 1)), np.array([1.0, 100.0]))
    pk = read_viewer_package(str(tmp_path))
    empty = pk["dynamic_paths"][0] if dynamic == "none" else pk["static_path"]
    assert png_size(empty)[:2] == (1, 1) and pk["atlas_hw"][dynamic == "none"] == (0, 0)
    o, p = open_viewer_package(str(tmp_path), dev, bg_color=BG, culled_rgba8=culled_texel_rgba8("sigmoid", "sigmoid")), bake_pool(model)
    T = int(model.frm_num)
    assert (o.layout.n_dynamic == 0) if dynamic == "none" else (o.layout.n_static == 0)
    assert torch.equal(o.layout.blocks, p.layout.blocks) and torch.equal(o.quad_keep, p.quad_keep)
    assert torch.equal(o.unpack_frames(range(T)), p.unpack_frames(range(T)))


def test_kernel_against_plain_torch(case, dev):
    """vl3d_pool_from_atlas_rgba8 over a pool of sentinel bytes against the same scatter in torch: the atlases unpacked tile by tile into each
    plane's (T,Hs,Ws,4) texels, then PackedLayout.pack_plane_ into a pool of zeros.  Whole pools compared: every texel of every stored slot is
    written, the ones past the plane's edge with 0."""
    from videoloop3d_amd.baked import atlas_tile_map, pool_from_atlas_
    from videoloop3d_amd.export import read_png, read_viewer_package
    pk = read_viewer_package(case.dir)
    lay, (th, tw), T = case.opened.layout, pk["tile"], case.T
    static = torch.from_numpy(read_png(pk["static_path"]))
    dyn = torch.stack([torch.from_numpy(read_png(p)) for p in pk["dynamic_paths"]])      # T,Ah,Aw,4
    culled = torch.tensor([(case.culled >> (8 * k)) & 0xff for k in range(4)], dtype=torch.uint8)
    ref = torch.zeros_like(case.opened.pool)
    D, QH, QW = pk["tile_src"].shape
    for d in range(D):
        plane = culled.expand(T, QH * th, QW * tw, 4).clone()
        for qy in range(QH):
            for qx in range(QW):
                src = int(pk["tile_src"][d, qy, qx])
                if src < 0:
                    continue
                k, gw = src >> 1, pk["grid_w"][src & 1]
                ys, xs = slice((k // gw) * th, (k // gw + 1) * th), slice((k % gw) * tw, (k % gw + 1) * tw)
                plane[:, qy * th:(qy + 1) * th, qx * tw:(qx + 1) * tw] = dyn[:, ys, xs] if src & 1 else static[ys, xs][None]
        lay.pack_plane_(ref, d, plane)
    got = torch.full_like(case.opened.pool, 0xAB)
    tm = atlas_tile_map(pk["tile_src"], lay, *pk["atlas_hw"])
    static_d, dyn_d = static.to(dev), dyn.to(dev)
    for t in range(T):
        pool_from_atlas_(lay, got, tm, static_d, dyn_d[t].contiguous(), t, case.culled)
    assert lay.n_static > 0 and lay.n_dynamic > 0
    assert torch.equal(got.cpu(), ref.cpu())
    assert torch.equal(got, case.opened.pool)
    past = torch.zeros((lay.D, lay.blocks.shape[1] * 8, lay.blocks.shape[2] * 8), dtype=torch.bool)
    past[:, lay.Hs:], past[:, :, lay.Ws:] = True, True
    if past.any():      # a ragged layout: the texels of stored blocks past the plane's edge are 0, not the sentinel
        b = lay.blocks.cpu().long()
        stored = (b >= 0).repeat_interleave(8, 1).repeat_interleave(8, 2) & past
        slot0 = (b >> 1).repeat_interleave(8, 1).repeat_interleave(8, 2)
        yy, xx = torch.meshgrid(torch.arange(past.shape[1]), torch.arange(past.shape[2]), indexing="ij")
        idx = (slot0 * 64 + (yy % 8) * 8 + xx % 8)[stored]
        assert len(idx) > 0 and int(got.cpu()[idx].max()) == 0


def _path(T, n=7):
    return [i % T for i in range(n)]


def test_render_path_bit_for_bit(case):
    """the opened storage behind the MODEL's spec, camera and background renders the in-process pool's display frames, byte for byte"""
    from videoloop3d_amd.baked import BakedPool, _Camera
    o = case.opened
    cam = _Camera(case.model)
    cam.planedepth, cam.mpi_d = cam.planedepth[case.planes].clone(), len(case.planes)      # the package holds the planes that have quads
    mixed = BakedPool(o.pool, o.layout, o.quad_keep, case.model.spec, BG, cam, case.culled)
    ext = np.stack([PM.tilted_pose(i) for i in range(7)])
    intr = np.stack([case.K] * 7)
    for channels in (3, 4):
        a = mixed.render_display(case.H, case.W, ext, intr, _path(case.T), channels=channels)
        b = case.inproc.render_display(case.H, case.W, ext, intr, _path(case.T), channels=channels)
        assert a.shape == (7, case.H, case.W, channels) and torch.equal(a, b)
        assert int(b[..., :3].max()) > 100 and len(torch.unique(b)) > 50


def test_render_with_the_packages_own_camera(case):
    """7 tilted poses of an 18 x 32 view, moved (on the host, fp64) until no sample lies within 1e-3 lattice units of a tile border or a plane
    edge -- the bound of the geometry test, under which both cameras put every sample into the same tile --: every byte of the opened model's
    display frames is within 1 level of the in-process pool's.

    These are NOT the 7 poses of test_render_path_bit_for_bit at its 36 x 64 view: the view is halved and every pose is tilted_pose(i, attempt)
    of the first attempt that is clear.  At 36 x 64 about 23 000 sample coordinates per pose make a clear pose a one-in-700 draw, at 18 x 32 one
    in five; the same planes, tiles, frames and camera code are exercised.  The model's own camera is held to the same margin less the measured
    disagreement of the two cameras, so no sample of either lies on the other side of a border."""
    from videoloop3d_amd.baked import _Camera
    o = case.opened
    H, W = case.H // 2, case.W // 2
    K = case.K.copy()
    K[:2] *= 0.5
    ext = PM.clear_poses(o.camera, o.spec, K, H, W, 7)
    intr = np.stack([K] * 7)
    mine = PM.lattice_coords(o.camera, o.spec, ext, intr, H, W)
    theirs = PM.lattice_coords(_Camera(case.model), case.model.spec, ext, intr, H, W, case.planes)
    geo = float(np.abs(mine - theirs).max())
    print(f"cameras agree to {geo:.3g} lattice units; nearest tile border {PM.border_distance(mine, o.spec.tile):.3g}")
    assert geo <= 1e-3 and PM.border_distance(mine, o.spec.tile) > 1e-3 and PM.border_distance(theirs, o.spec.tile) > 1e-3 - geo
    for channels in (3, 4):
        a = o.render_display(H, W, ext, intr, _path(case.T), channels=channels).cpu().int()
        b = case.inproc.render_display(H, W, ext, intr, _path(case.T), channels=channels).cpu().int()
        diff = (a - b).abs()
        print(f"channels {channels}: {int((diff > 0).sum())} of {diff.numel()} bytes differ, max {int(diff.max())} level(s)")
        assert int(diff.max()) <= 1
        assert int(b[..., :3].max()) > 100 and len(torch.unique(b)) > 50
