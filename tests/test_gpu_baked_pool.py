"""The baked tile pool on the MI355X (videoloop3d_amd/baked.py: bake_pool / BakedPool; csrc/vl3d_render_baked_pool.hip): RGBA8 blocks of 8 x 8
texels behind the block table of packed.PackedLayout, rendered without a dense clip.  The render must equal the dense baked render
(vl3d_render_fwd_baked, pinned by tests/test_gpu_baked.py) of the unpacked texels BIT FOR BIT on every pixel; the pool must hold the bytes the
dense bake holds; bake_pool / render_frames(baked=) / BakedPool.render on a tiny MPMeshVid, packed and not; determinism and guards.

Shapes: D = 4 planes, a model of 5 frames of which frames 1..3 (an odd run: one frame pair and its tail), frame 3 alone (the one-frame kernel)
and frames 1..2 (an even run) are rendered; output 37 x 70 (2 x 5 workgroups of 64 x 8, none of them full) with the camera, scale and offset of
tests/test_gpu_baked.py (hard-cut edges of every plane inside the view).  Two plane geometries: (a) the shared-border lattice, 40 x 72 texels =
5 x 9 quads; (b) tile-exact, 5 x 7 tiles of 6 x 10 texels = 30 x 70 texels: tiles straddle the 8 x 8 blocks and the last block row and column
are ragged (4 x 9 blocks).  About half of the quads kept, plane 2 none, a third of the kept ones dynamic."""
import dataclasses
import types

import numpy as np
import pytest
import torch

import baked_models as BM
from baked_models import GEOMS, D, H, T_MODEL, W
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu

RUNS = [(1, 3), (3, 1), (1, 2)]      # (frame0, n): the odd run, a single frame, the even run


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _homographies():
    """[D,3,3] target pixel -> plane pixel of the benchmark camera (near 1, far 100), as tests/test_gpu_baked.py forms them."""
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    depths = make_depths(D, 1.0, 100.0).flip(0)
    return compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3), depths[None])[0].float()


def _base_taps(g, spec, homos, keep):
    """fp64 statement of the sample positions: (covered [D,H,W] bool, x0 [D,H,W] base tap column) -- enough to see which tap pairs cross a
    block seam.  (Tile-exact: the texel coordinate is the lattice coordinate plus the quad index.)"""
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64) + spec.pixel_center, torch.arange(W, dtype=torch.float64) + spec.pixel_center,
                            indexing="ij")
    cov, x0s = [], []
    for d in range(D):
        h = homos[d].double().cpu()
        Z = h[2, 0] * xs + h[2, 1] * ys + h[2, 2]
        u = (h[0, 0] * xs + h[0, 1] * ys + h[0, 2]) / Z * spec.scale[0] + spec.offset[0]
        v = (h[1, 0] * xs + h[1, 1] * ys + h[1, 2]) / Z * spec.scale[1] + spec.offset[1]
        if g["tile"] is None:
            qx = (u * g["QW"] / (g["Ws"] - 1)).floor().clamp(0, g["QW"] - 1).long()
            qy = (v * g["QH"] / (g["Hs"] - 1)).floor().clamp(0, g["QH"] - 1).long()
        else:
            qx = (u / (g["tile"][1] - 1)).floor().clamp(0, g["QW"] - 1).long()
            qy = (v / (g["tile"][0] - 1)).floor().clamp(0, g["QH"] - 1).long()
            u, v = u + qx, v + qy
        inside = (u >= 0) & (u <= g["Ws"] - 1) & (v >= 0) & (v <= g["Hs"] - 1)
        cov.append(inside & keep[d].cpu().bool()[qy, qx])
        x0s.append(u.floor().clamp(0, g["Ws"] - 2).long())
    return torch.stack(cov), torch.stack(x0s)


@pytest.fixture(scope="module")
def scenes(dev):
    """per geometry: the BakedPool of hash-random texels, its dense unpacking, and the DENSE baked kernel's render of that clip for the three
    runs -- the reference, computed once and never modified."""
    from videoloop3d_amd.baked import BakedPool, bake_texels
    from videoloop3d_amd.packed import PackedLayout
    from videoloop3d_amd.render import render_frame_run_baked
    homos = _homographies().to(dev)
    out = {}
    for name, g in GEOMS.items():
        keep = synth.hash_uniform((D, g["QH"], g["QW"]), seed=11) < 0.5
        keep[2] = False
        dyn = keep & (synth.hash_uniform((D, g["QH"], g["QW"]), seed=12) < 1.0 / 3.0)
        assert 0.3 < float(keep.float().mean()) < 0.6 and 0.15 < float(dyn.sum()) / float(keep.sum()) < 0.55
        lay = PackedLayout(keep.to(dev), dyn.to(dev), T_MODEL, g["Hs"], g["Ws"], g["tile"])
        e = lay.blocks
        # the case cannot become trivial silently: static, dynamic and unstored blocks are all there
        assert int((e < 0).sum()) > 0 and int(((e >= 0) & ((e & 1) == 0)).sum()) > 0 and int(((e >= 0) & ((e & 1) == 1)).sum()) > 0
        clip = bake_texels(synth.make_plane_stack(D, T_MODEL, g["Hs"], g["Ws"], seed=7, device=dev, alpha_bias=-0.5), "sigmoid", "sigmoid")
        pool = BM.scatter_pool(lay, clip, torch.zeros((1, 4), dtype=torch.uint8, device=dev))
        spec = BM.pool_spec(g)
        qk = keep.to(torch.uint8).to(dev)
        bp = BakedPool(pool, lay, qk, spec, "", None, 7 | 11 << 8 | 13 << 16 | 0 << 24)      # (a culled texel with colour: it must never show)
        dense = bp.unpack_frames(range(T_MODEL))
        assert dense.shape == (D, T_MODEL, g["Hs"], g["Ws"], 4) and dense.dtype == torch.uint8
        ref = {run: tuple(t.clone() for t in render_frame_run_baked(dense, run[0], run[1], homos, H, W, spec, quad_keep=qk)) for run in RUNS}
        cov, x0 = _base_taps(g, spec, homos, keep)
        out[name] = types.SimpleNamespace(g=g, bp=bp, dense=dense, qk=qk, spec=spec, ref=ref, cov=cov, x0=x0, keep=keep)
    return types.SimpleNamespace(homos=homos, geo=out)


# ---- 1. bit equality with the dense baked kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
def test_pool_render_equals_the_dense_baked_render(dev, scenes, geom):
    from videoloop3d_amd.render import render_frame_run_baked_pool
    s = scenes.geo[geom]
    seam = s.cov & (s.x0 % 8 == 7)
    print(f"[{geom}] covered samples {int(s.cov.sum())}, of them across a block seam {int(seam.sum())}; blocks {tuple(s.bp.layout.blocks.shape)}, "
          f"static {s.bp.layout.n_static}, dynamic {s.bp.layout.n_dynamic}, slots {s.bp.layout.n_slots}")
    assert int(seam.sum()) > 0 and int((s.cov & (s.x0 % 8 != 7)).sum()) > 0
    got = {}
    for run in RUNS:
        rgb, alpha = render_frame_run_baked_pool(s.bp.layout, s.bp.pool, run[0], run[1], scenes.homos, H, W, s.spec, quad_keep=s.qk,
                                                 culled_rgba8=s.bp.culled_rgba8)
        rgb_d, alpha_d = s.ref[run]
        assert rgb.shape == (run[1], H, W, 3) and alpha.shape == (run[1], H, W)
        print(f"[{geom}] frames {run[0]}..{run[0] + run[1] - 1}: max |d rgb| {float((rgb - rgb_d).abs().max()):.3e}, "
              f"max |d alpha| {float((alpha - alpha_d).abs().max()):.3e}")
        assert torch.equal(rgb, rgb_d) and torch.equal(alpha, alpha_d)
        got[run] = (rgb, alpha)
    odd, one, even = (got[r] for r in RUNS)
    assert torch.equal(one[0][0], odd[0][2]) and torch.equal(one[1][0], odd[1][2])
    assert torch.equal(even[0], odd[0][:2]) and torch.equal(even[1], odd[1][:2])
    rgb_d, alpha_d = s.ref[RUNS[0]]
    covered = float((alpha_d > 0).float().mean())
    print(f"[{geom}] covered pixels {covered:.3f}, max |frame 1 - frame 3| {float((rgb_d[0] - rgb_d[2]).abs().max()):.3f}")
    assert 0.3 < covered < 1.0
    assert float((rgb_d[0] - rgb_d[2]).abs().max()) > 0.05      # the dynamic blocks show


# ---- 2. pool contents, 3. module level ---------------------------------------------------------------------------------------------------
def _cameras(K):
    """three cameras (world-to-camera) over five output frames: a run of three on the first, then single frames (tests/test_gpu_baked.py)."""
    ext = np.tile(np.eye(4, dtype=np.float32)[None], (5, 1, 1))
    ext[3:, :3, 3] = [0.03, 0.01, 0.0]
    ext[4, :3, 3] = [-0.05, 0.02, 0.01]
    return ext, np.tile(K.astype(np.float32)[None], (5, 1, 1)), np.array([1, 2, 3, 5, 0])


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "lattice"])
def test_pool_contents(dev, exact):
    from videoloop3d_amd.baked import BakedPool, bake, bake_pool, bake_texels
    model, _, _, _ = BM.pool_model(dev, "", exact)
    dense_bake = bake(model)
    from_dense = bake_pool(model)                       # the unpacked sparsified model: plane by plane through the table
    assert isinstance(from_dense, BakedPool) and from_dense.pool.dtype == torch.uint8 and from_dense.pool.is_cuda
    assert from_dense.layout.tile == (model.tile_own if exact else None)
    model.pack_()
    packed = bake_pool(model)                           # the packed model: one bake over its float pool
    lay = packed.layout
    assert packed.pool.shape == (lay.n_slots * 64, 4) and torch.equal(lay.blocks, model.packed.blocks) and lay.blocks is not model.packed.blocks
    assert lay.n_static > 0 and lay.n_dynamic > 0 and int((lay.blocks < 0).sum()) > 0
    assert torch.equal(packed.pool, bake_texels(model.stack_pool.data.view(-1, 4), "sigmoid", "sigmoid"))
    assert torch.equal(from_dense.pool, packed.pool) and torch.equal(from_dense.layout.blocks, lay.blocks)
    assert from_dense.culled_rgba8 == packed.culled_rgba8 == (127 | 127 << 8 | 127 << 16)      # sigmoid(0) * 255 = 127.5; sigmoid(-1e4) = 0
    up = packed.unpack_frames(range(packed.frm_num))
    assert up.shape == dense_bake.texels.shape and up.dtype == torch.uint8
    stored = torch.stack([lay._plane_index(d)[2] for d in range(lay.D)])      # D,Hs,Ws
    assert 0.0 < float(stored.float().mean()) < 1.0
    sel = stored[:, None].expand(up.shape[:4])
    assert torch.equal(up[sel], dense_bake.texels[sel])
    fill = torch.tensor([127, 127, 127, 0], dtype=torch.uint8, device=dev)
    assert bool((up[~sel] == fill).all())
    # 256 bytes per slot + the table, less than the dense baked clip
    assert packed.nbytes == 256 * lay.n_slots + 4 * lay.blocks.numel()
    assert packed.nbytes < dense_bake.nbytes


def test_module_bake_pool_and_render_frames(dev):
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd.baked import bake, bake_pool
    for exact in (True, False):
        model, Hm, Wm, K = BM.pool_model(dev, "0.2#0.4#0.6", exact)
        dense_bake, pool_bake = bake(model), bake_pool(model)
        assert pool_bake.frm_num == dense_bake.frm_num == 6 and pool_bake.spec == model.spec and pool_bake.bg_color == "0.2#0.4#0.6"
        ext, intr, rt = _cameras(K)
        want = RV.render_frames(model, Hm, Wm, ext, intr, rt, baked=dense_bake)
        got = RV.render_frames(model, Hm, Wm, ext, intr, rt, baked=pool_bake)
        assert got.shape == (5, Hm, Wm, 3) and got.dtype == torch.uint8 and torch.equal(got, want)
        assert float(want.float().std()) > 1.0
        for i in (0, 3, 4):      # BakedPool.render against BakedMPV.render: a run of three frames, single frames, the whole clip
            ts = torch.tensor(rt[:3] if i == 0 else rt[i:i + 1])
            r, a = pool_bake.render(Hm, Wm, torch.tensor(ext[i:i + 1]), torch.tensor(intr[i:i + 1]), ts)
            r_d, a_d = dense_bake.render(Hm, Wm, torch.tensor(ext[i:i + 1]), torch.tensor(intr[i:i + 1]), ts)
            assert r.shape == (len(ts), 3, Hm, Wm) and torch.equal(r, r_d) and torch.equal(a, a_d)
        r, a = pool_bake.render(Hm, Wm, torch.tensor(ext[4:5]), torch.tensor(intr[4:5]))
        r_d, a_d = dense_bake.render(Hm, Wm, torch.tensor(ext[4:5]), torch.tensor(intr[4:5]))
        assert r.shape == (6, 3, Hm, Wm) and torch.equal(r, r_d) and torch.equal(a, a_d)
        with pytest.raises(IndexError):
            pool_bake.render(Hm, Wm, torch.tensor(ext[:1]), torch.tensor(intr[:1]), torch.tensor([5, 6]))
        # after pack_(): bake_pool works and gives the same frames; bake still refuses
        model.pack_()
        packed_bake = bake_pool(model)
        assert torch.equal(RV.render_frames(model, Hm, Wm, ext, intr, rt, baked=packed_bake), want)
        with pytest.raises(RuntimeError, match="packed"):
            bake(model)
        assert packed_bake.nbytes == 256 * packed_bake.layout.n_slots + 4 * packed_bake.layout.blocks.numel() < dense_bake.nbytes


def test_bake_pool_refusals(dev):
    from videoloop3d_amd.baked import bake_pool
    model, _, _, _ = BM.pool_model(dev, "")
    model.is_sparse = False
    with pytest.raises(RuntimeError, match="not sparse"):
        bake_pool(model)
    cpu_model, _, _, _ = BM.pool_model(torch.device("cpu"), "")
    with pytest.raises(RuntimeError, match="host"):
        bake_pool(cpu_model)
    cpu_model.atlas_exact = True
    with pytest.raises(RuntimeError, match="atlas_exact"):
        bake_pool(cpu_model)


# ---- 4. determinism and guards -----------------------------------------------------------------------------------------------------------
def test_determinism_and_guards(dev, scenes):
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd.render import RenderSpec, render_frame_run_baked_pool
    for s in scenes.geo.values():
        a = render_frame_run_baked_pool(s.bp.layout, s.bp.pool, 1, 3, scenes.homos, H, W, s.spec, quad_keep=s.qk, culled_rgba8=s.bp.culled_rgba8)
        b = render_frame_run_baked_pool(s.bp.layout, s.bp.pool, 1, 3, scenes.homos, H, W, s.spec, quad_keep=s.qk, culled_rgba8=s.bp.culled_rgba8)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    s = scenes.geo["shared"]
    g, lay, pool = s.g, s.bp.layout, s.bp.pool
    lib = L.lib()
    SENT = 123.0
    rgb = torch.full((3, H, W, 3), SENT, device=dev)
    alpha = torch.full((3, H, W), SENT, device=dev)
    stream = L.stream_ptr(dev)

    def desc(spec=s.spec, dtype="u8", n=3, **over):
        d = L.RenderDesc()
        d.D, d.T, d.Hs, d.Ws, d.H, d.W = D, n, g["Hs"], g["Ws"], H, W
        d.coord_mode, d.border_mode, d.act_order = L.COORD[spec.coord_mode], L.BORDER[spec.border], L.ACT_ORDER[spec.act_order]
        d.stack_dtype = L.STACK_DTYPE[dtype]
        d.pixel_center = float(spec.pixel_center)
        d.sx, d.sy, d.ox, d.oy = float(spec.scale[0]), float(spec.scale[1]), float(spec.offset[0]), float(spec.offset[1])
        d.uv_noise_seed = int(spec.uv_noise_seed)
        for k, v in over.items():
            setattr(d, k, v)
        return d
    cull = torch.empty((int(lib.vl3d_render_cull_scratch_bytes(desc())) + 3) // 4, dtype=torch.float32, device=dev)
    ARGS = dict(blocks=L.ptr(lay.blocks), pool=L.ptr(pool), frame0=1, T_model=T_MODEL, homos=L.ptr(scenes.homos), quad_keep=L.ptr(s.qk), QH=g["QH"],
                QW=g["QW"], culled=s.bp.culled_rgba8, cull=L.ptr(cull), rgb=rgb, alpha=alpha)

    def rc(d, **over):
        a = dict(ARGS, **over)
        return lib.vl3d_render_fwd_baked_pool(d, a["blocks"], a["pool"], a["T_model"], a["homos"], BM.run_sel(a["frame0"]), a["quad_keep"], a["QH"],
                                              a["QW"], a["culled"], a["cull"], BM.float_out(a["rgb"], a["alpha"]), stream)
    EINVAL = 1

    def refused(fragment, d=None, **over):
        assert rc(desc() if d is None else d, **over) == EINVAL
        assert fragment in lib.vl3d_last_error(), lib.vl3d_last_error()
    for name in ("blocks", "pool", "homos", "quad_keep", "cull", "rgb", "alpha"):
        refused(b"null pointer", **{name: None})
    assert rc(None) == EINVAL
    refused(b"VL3D_U8", desc(dtype="f32"))
    refused(b"planar", desc(RenderSpec()))
    refused(b"uv_noise", desc(dataclasses.replace(s.spec, uv_noise_seed=5)))
    refused(b"variant", desc(variant=1))
    refused(b"leaves the model", frame0=3)                       # frames 3 .. 5 of a model of 5
    refused(b"leaves the model", frame0=-1)
    refused(b"leaves the model", T_model=3)
    refused(b"4-byte aligned", pool=L.C.c_void_p(pool.data_ptr() + 1))
    refused(b"bad quad grid", QH=0)
    refused(b"bad quad grid", QH=-g["QH"])                       # mixed signs
    refused(b"bad quad grid", QH=-7, QW=-9)                      # tile-exact: 40 texels are not 7 whole tiles
    refused(b"128 planes", desc(D=129))
    refused(b"2 x 2", desc(Hs=1))
    refused(b"2 x 2", desc(Ws=1))
    refused(b"cull_", desc(cull_Hs=g["Hs"], cull_Ws=g["Ws"]))
    torch.cuda.synchronize()
    assert bool((rgb == SENT).all()) and bool((alpha == SENT).all())      # error returns: nothing was launched
    assert rc(desc()) == 0
    torch.cuda.synchronize()
    assert torch.equal(rgb, s.ref[(1, 3)][0]) and torch.equal(alpha, s.ref[(1, 3)][1])
    # the Python entry
    kw = dict(quad_keep=s.qk, culled_rgba8=s.bp.culled_rgba8)
    with pytest.raises(RuntimeError, match="planar"):
        render_frame_run_baked_pool(lay, pool, 1, 3, scenes.homos, H, W, RenderSpec(), **kw)
    with pytest.raises(RuntimeError, match="uint8"):
        render_frame_run_baked_pool(lay, pool.float(), 1, 3, scenes.homos, H, W, s.spec, **kw)
    with pytest.raises(RuntimeError, match="no backward"):
        with torch.enable_grad():
            render_frame_run_baked_pool(lay, pool, 1, 3, scenes.homos.clone().requires_grad_(True), H, W, s.spec, **kw)
    with pytest.raises(RuntimeError, match="leave the model"):
        render_frame_run_baked_pool(lay, pool, 3, 3, scenes.homos, H, W, s.spec, **kw)
    with pytest.raises(RuntimeError, match="quad map"):
        render_frame_run_baked_pool(lay, pool, 1, 3, scenes.homos, H, W, s.spec, quad_keep=None, culled_rgba8=0)
    with pytest.raises(TypeError):      # the quad map and the culled texel are required arguments
        render_frame_run_baked_pool(lay, pool, 1, 3, scenes.homos, H, W, s.spec, quad_keep=s.qk)
    with pytest.raises(RuntimeError, match="built from"):      # a quad map of another grid than the table's
        render_frame_run_baked_pool(lay, pool, 1, 3, scenes.homos, H, W, s.spec, quad_keep=s.qk[:, :4].contiguous(), culled_rgba8=0)
    import copy
    bad = copy.copy(lay)
    bad.blocks = lay.blocks[:, :, :8].contiguous()      # a table that is not ceil(Hs/8) x ceil(Ws/8)
    with pytest.raises(RuntimeError, match="block table"):
        render_frame_run_baked_pool(bad, pool, 1, 3, scenes.homos, H, W, s.spec, **kw)
    with pytest.raises(RuntimeError, match="tile"):
        render_frame_run_baked_pool(lay, pool, 1, 3, scenes.homos, H, W, scenes.geo["exact"].spec, **kw)
    torch.cuda.synchronize()


# ---- 7. the four culled forward entries share one quad-grid rule ---------------------------------------------------------------------------
def test_culled_forward_entries_share_the_grid_rule(dev, scenes):
    """vl3d_render_fwd_frames (with a quad map), _fwd_packed, _fwd_baked and _fwd_baked_pool at the C ABI, on the `exact` (30 x 70 texels, 5 x 7 tiles) and
    `shared` (40 x 72 texels, 5 x 9 quads) scenes: every entry refuses the same bad quad grids with VL3D_EINVAL -- mixed signs, a zero, a
    tile-exact grid that does not divide the plane, a tile-exact grid of 1-texel tiles -- before anything is launched (the sentinel-filled
    outputs stay untouched), and accepts the scene's own grid."""
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd.render import _desc_dims, _qgrid
    lib, stream, n, EINVAL, SENT = L.lib(), L.stream_ptr(dev), 3, 1, 123.0
    frames = torch.arange(1, 1 + n, dtype=torch.int32, device=dev)
    for name in ("exact", "shared"):
        s = scenes.geo[name]
        g, lay = s.g, s.bp.layout
        QH, QW = _qgrid(s.qk, s.spec)
        assert (QH < 0) == (name == "exact")
        stack = synth.make_plane_stack(D, T_MODEL, g["Hs"], g["Ws"], seed=7, device=dev)
        fpool = lay.new_pool(dev)
        rgb = torch.full((n, H, W, 3), SENT, device=dev)
        alpha = torch.full((n, H, W), SENT, device=dev)
        d_f32 = _desc_dims(D, n, g["Hs"], g["Ws"], H, W, s.spec, L.STACK_DTYPE["f32"])
        d_pk = _desc_dims(D, T_MODEL, g["Hs"], g["Ws"], H, W, s.spec, L.STACK_DTYPE["f32"])
        d_u8 = _desc_dims(D, n, g["Hs"], g["Ws"], H, W, s.spec, L.STACK_DTYPE["u8"])
        cull = torch.empty((int(lib.vl3d_render_cull_scratch_bytes(d_f32)) + 3) // 4, dtype=torch.float32, device=dev)
        hom, qk, out = L.ptr(scenes.homos), L.ptr(s.qk), (L.ptr(rgb), L.ptr(alpha))
        sel, sink = BM.run_sel(1), BM.float_out(rgb, alpha)
        entries = {
            "vl3d_render_fwd_frames": lambda qh, qw: lib.vl3d_render_fwd_frames(d_f32, L.ptr(stack), 1, T_MODEL, hom, qk, qh, qw, L.ptr(cull), *out, stream),
            "vl3d_render_fwd_packed": lambda qh, qw: lib.vl3d_render_fwd_packed(d_pk, L.ptr(lay.blocks), L.ptr(fpool), L.ptr(frames), n, hom, qk, qh, qw,
                                                                                0.0, *out, stream),
            "vl3d_render_fwd_baked": lambda qh, qw: lib.vl3d_render_fwd_baked(d_u8, L.ptr(s.dense), T_MODEL, hom, sel, qk, qh, qw, L.ptr(cull), sink, stream),
            "vl3d_render_fwd_baked_pool": lambda qh, qw: lib.vl3d_render_fwd_baked_pool(d_u8, L.ptr(lay.blocks), L.ptr(s.bp.pool), T_MODEL, hom, sel, qk,
                                                                                        qh, qw, s.bp.culled_rgba8, L.ptr(cull), sink, stream),
        }
        bad = [(abs(QH), -abs(QW)), (0, abs(QW)), (-4, -7), (-30, -70)]
        for entry, call in entries.items():
            for qh, qw in bad:
                assert call(qh, qw) == EINVAL, (name, entry, qh, qw)
        torch.cuda.synchronize()
        assert bool((rgb == SENT).all()) and bool((alpha == SENT).all())      # error returns: nothing was launched
        for entry, call in entries.items():
            assert call(QH, QW) == 0, (name, entry, lib.vl3d_last_error())
        torch.cuda.synchronize()
