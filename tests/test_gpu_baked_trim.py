"""Trimming a baked pool on the MI355X (baked.BakedPool.trimmed; vl3d_baked_trim_classify / _move, csrc/vl3d_baked_trim.hip) against the rule
stated in plain torch (tests/baked_trim_statement.py), and the trimmed pool's frames against its source's -- every comparison torch.equal or an
integer equality, no pixel excluded.

Shapes (the tiny ones of tests/baked_models.py): the two pools of fp64_scenes() -- D = 4, T = 5, 40 x 72 texels block aligned on the shared-border
lattice, and 30 x 70 in tiles of 6 x 10 straddling the 8 x 8 blocks with ragged last blocks -- edited so that every third kept quad has alpha byte 0
and every second dynamic quad repeats frame 0; pool_model(exact=False): D = 6, T = 6, 38 x 67 ragged, sigmoid activations, where the invisible
alpha logits are exactly -12 and the frozen quads copy frame 0 in float; pool_model(exact=True) (4 x 6 tiles of 8 x 8) for the package.  The traps
run on 2 planes of 20 x 27 texels (3 x 4 blocks, ragged on both axes), T = 3."""
import copy
import os
import types

import numpy as np
import pytest
import torch

import baked_models as BM
import baked_statement as BS
import baked_trim_statement as TS

pytestmark = pytest.mark.gpu

H, W = BM.H, BM.W
BG = "0.2#0.4#0.6"


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bg_string(bg):
    return "" if bg is None else "#".join(repr(float(v)) for v in bg)


def _edit_model(model, inner_only=False):
    """every third kept quad invisible (alpha logit exactly -12 on the texels it can read: the byte 0 under the host and the device rule), every
    second dynamic quad frozen (frame 0 copied in float).  inner_only: invisible quads are taken off the rim of the quad grid (the package test)."""
    from videoloop3d_amd import tiles
    keep, dyn = model.quad_keep.cpu().bool(), (model.quad_keep & model.quad_dyn).cpu().bool()
    pick = keep.clone()
    if inner_only:
        pick[:, 0], pick[:, -1], pick[:, :, 0], pick[:, :, -1] = False, False, False, False
    invisible = torch.zeros(keep.numel(), dtype=torch.bool)
    invisible[pick.flatten().nonzero()[:, 0][::3]] = True
    frozen = torch.zeros(keep.numel(), dtype=torch.bool)
    frozen[dyn.flatten().nonzero()[:, 0][::2]] = True
    st = model.stack.data
    D, T, Hs, Ws, _ = st.shape
    fr = tiles.quad_to_texel_mask(frozen.reshape(keep.shape), Hs, Ws, model.tile_own).to(st.device)
    st.copy_(torch.where(fr[:, None, :, :, None], st[:, :1], st))
    inv = tiles.quad_to_texel_mask(invisible.reshape(keep.shape), Hs, Ws, model.tile_own).to(st.device)
    st[..., 3] = torch.where(inv[:, None], torch.full_like(st[..., 3], -12.0), st[..., 3])
    return invisible.reshape(keep.shape), frozen.reshape(keep.shape)


def _stand_in_camera(homos):
    """a camera whose plane_homographies are this file's (tests/test_gpu_baked_path.py): the intrinsics' [0, 0] entry carries the camera index"""
    return types.SimpleNamespace(ref_extrin=torch.eye(4), plane_homographies=lambda e, k: homos[int(k[0, 0, 0])].cpu(), _on=lambda device, name: torch.eye(4))


def _stand_in_poses(cams):
    ext, intr = torch.eye(4)[None].repeat(len(cams), 1, 1), torch.eye(3)[None].repeat(len(cams), 1, 1)
    intr[:, 0, 0] = torch.tensor(cams, dtype=torch.float32)
    return ext, intr


def _model_poses(K, cams):
    base = np.tile(np.eye(4, dtype=np.float32)[None], (3, 1, 1))
    base[1, :3, 3] = [0.03, 0.01, 0.0]
    base[2, :3, 3] = [-0.05, 0.02, 0.01]
    return torch.tensor(base[cams]), torch.tensor(np.tile(K.astype(np.float32)[None], (len(cams), 1, 1)))


@pytest.fixture(scope="module")
def cases(dev):
    """name -> the source pool, the rule's result on its bytes (host, computed once), the kernels' classification, trimmed(), and how to pose it"""
    from videoloop3d_amd.baked import BakedPool, bake_pool, trim_classify
    from videoloop3d_amd.packed import PackedLayout
    out = {}
    for geom in BM.GEOMS:
        st = BM.fp64_scenes()["pool_" + geom]
        pool, _ = TS.edit_scene(st)
        D, T, Hs, Ws = st.scene.dims
        lay = PackedLayout(st.keep.to(dev), st.dyn.to(dev), T, Hs, Ws, st.tile)
        assert torch.equal(lay.blocks.cpu(), st.lay.blocks)
        bp = BakedPool(pool.to(dev), lay, st.keep.to(torch.uint8).to(dev), st.scene.spec, BG, _stand_in_camera(st.scene.homos), BS.CULLED,
                       quad_dyn=(st.keep & st.dyn).to(torch.uint8).to(dev))
        out[geom] = types.SimpleNamespace(bp=bp, tile=st.tile, H=H, W=W, poses=_stand_in_poses, times=BS.TIMES)
    model, Hm, Wm, K = BM.pool_model(dev, BG, exact=False)
    _edit_model(model)
    last = float(np.nextafter(np.float32(6), np.float32(0)))
    out["lattice"] = types.SimpleNamespace(bp=bake_pool(model), tile=None, H=Hm, W=Wm, poses=lambda cams: _model_poses(K, cams),
                                           times=[(0, 1.0), (1, 0.0), (2, 1.5), (0, 2.125), (1, 2.7), (2, 5.25), (0, last)])
    for name, c in out.items():
        bp, lay = c.bp, c.bp.layout
        c.before = [t.clone() for t in (bp.pool, lay.blocks, bp.quad_keep, bp.quad_dyn)]
        c.tr = TS.trim(lay.blocks, bp.pool, lay.T, lay.Hs, lay.Ws, bp.culled_rgba8, bp.quad_keep, c.tile)
        c.kernels = trim_classify(lay, bp.pool, bp.culled_rgba8)
        c.t = bp.trimmed()
        # the case cannot become trivial silently
        assert int(c.tr.dropped.sum()) > 0 and int(c.tr.demoted.sum()) > 0 and int((bp.quad_keep.cpu().bool() & ~c.tr.keep).sum()) > 0, name
        assert int(((c.tr.blocks >= 0) & ((c.tr.blocks & 1) == 1)).sum()) > 0, name
    return out


NAMES = ["shared", "exact", "lattice"]


# ---- 1. the kernels against the rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_kernels_equal_the_statement(cases, name):
    c = cases[name]
    tr, t, lay = c.tr, c.t, c.bp.layout
    flags, slots, tclass = (x.cpu() for x in c.kernels)
    assert flags.shape == tclass.shape == (lay.D, lay.Hs, lay.Ws) and slots.shape == lay.blocks.shape and slots.dtype == torch.int32
    assert torch.equal(flags, tr.vis.to(torch.uint8) | tr.dif.to(torch.uint8) << 1)
    assert torch.equal(tclass, tr.show.to(torch.uint8) | tr.moves.to(torch.uint8) << 1)
    assert torch.equal(slots.long(), tr.size)
    assert torch.equal(t.layout.blocks.cpu(), tr.blocks) and t.layout.n_slots == tr.n_slots and t.layout.blocks.dtype == torch.int32
    assert t.layout.n_static == int((tr.size == 1).sum()) and t.layout.n_dynamic == int((tr.size > 1).sum()) and t.layout._index_cache == {}
    assert t.pool.shape == (tr.n_slots * 64, 4) and torch.equal(t.pool.cpu(), tr.pool)
    assert t.quad_keep.dtype == t.quad_dyn.dtype == torch.uint8 and t.quad_keep.shape == t.quad_dyn.shape == c.bp.quad_keep.shape
    assert torch.equal(t.quad_keep.cpu().bool(), tr.keep) and torch.equal(t.quad_dyn.cpu().bool(), tr.dyn)
    e = lay.blocks.cpu()
    r = t.trim_report
    print(f"[{name}] {r}")
    assert r["blocks_stored"] == int((e >= 0).sum()) and r["blocks_dropped"] == int(tr.dropped.sum()) and r["blocks_demoted"] == int(tr.demoted.sum())
    assert (r["slots_before"], r["slots_after"], r["bytes_before"], r["bytes_after"]) == (lay.n_slots, tr.n_slots, 256 * lay.n_slots, 256 * tr.n_slots)
    keep0, dyn0 = c.bp.quad_keep.cpu().bool(), c.bp.quad_dyn.cpu().bool()
    assert (r["quads_kept"], r["quads_dropped"], r["quads_demoted"]) == (int(tr.keep.sum()), int((keep0 & ~tr.keep).sum()), int((dyn0 & tr.keep & ~tr.dyn).sum()))
    if name in BM.GEOMS:      # the figures of the rule's first check on the oracle (docs/kernels/K9_baked_playback.md "Trimming the pool")
        want = {"shared": (135, 25, 42, 559, 282, 25), "exact": (97, 1, 18, 269, 196, 19)}[name]
        assert (r["blocks_stored"], r["blocks_dropped"], r["blocks_demoted"], r["slots_before"], r["slots_after"], r["quads_dropped"]) == want


def test_one_frame_makes_every_dynamic_block_static(dev):
    from videoloop3d_amd.baked import BakedPool
    from videoloop3d_amd.packed import PackedLayout
    st = BM.fp64_scenes()["pool_exact"]
    D, _, Hs, Ws = st.scene.dims
    lay = PackedLayout(st.keep.to(dev), st.dyn.to(dev), 1, Hs, Ws, st.tile)
    pool = BM.scatter_pool(lay, st.source[:, :1].to(dev), torch.zeros((1, 4), dtype=torch.uint8, device=dev))
    t = BakedPool(pool, lay, st.keep.to(torch.uint8).to(dev), st.scene.spec, "", None, BS.CULLED).trimmed()
    tr = TS.trim(lay.blocks, pool, 1, Hs, Ws, BS.CULLED, st.keep, st.tile)
    assert lay.n_dynamic > 0 and t.layout.n_dynamic == 0 and torch.equal(t.layout.blocks.cpu(), tr.blocks) and torch.equal(t.pool.cpu(), tr.pool)
    assert not bool(t.quad_dyn.any()) and t.trim_report["quads_demoted"] is None


# ---- 2. traps, each decided by one texel --------------------------------------------------------------------------------------------------------------
TD, TT, THS, TWS = 2, 3, 20, 27


def _trap_layout(dev):
    from videoloop3d_amd.packed import PackedLayout
    ones = torch.ones((TD, 2, 3), dtype=torch.bool, device=dev)
    lay = PackedLayout(ones, ones, TT, THS, TWS, None)
    assert lay.n_dynamic == lay.blocks.numel() == TD * 3 * 4      # every block stored, dynamic
    return lay


def _trap(dev, edits=(), pool_edits=()):
    """the trap pool: alpha byte 0 everywhere, hash-random colours equal in all frames -- every block drops.  edits: (d, t or None, y, x, channel, value)
    on the clip; pool_edits: (d, by, bx, t, ly, lx, channel, value) on a block's stored texel, in the plane or past its edge.
    -> (block slot counts of the kernels [D,3,4], the statement's result); the two are compared here."""
    from videoloop3d_amd.baked import trim_classify
    lay = _trap_layout(dev)
    clip = BS.random_clip(TD, 1, THS, TWS, seed=3).repeat(1, TT, 1, 1, 1)
    clip[..., :3] = clip[..., :3].clamp(min=20)
    clip[..., 3] = 0
    for d, t, y, x, ch, v in edits:
        clip[d, slice(None) if t is None else t, y, x, ch] = v
    pool = BM.scatter_pool(lay, clip.to(dev), torch.zeros((1, 4), dtype=torch.uint8, device=dev))
    for d, by, bx, t, ly, lx, ch, v in pool_edits:
        pool[((int(lay.blocks[d, by, bx]) >> 1) + t) * 64 + ly * 8 + lx, ch] = v
    flags, slots, tclass = trim_classify(lay, pool, BS.CULLED)
    tr = TS.trim(lay.blocks, pool, TT, THS, TWS, BS.CULLED, torch.ones((TD, 2, 3), dtype=torch.bool), None)
    assert torch.equal(slots.cpu().long(), tr.size) and torch.equal(flags.cpu(), tr.vis.to(torch.uint8) | tr.dif.to(torch.uint8) << 1)
    assert torch.equal(tclass.cpu(), tr.show.to(torch.uint8) | tr.moves.to(torch.uint8) << 1)
    return slots.cpu(), tr


def test_trap_a_neighbours_facing_edge_or_corner_keeps_a_zero_alpha_block(dev):
    base, _ = _trap(dev)
    assert int(base.sum()) == 0      # nothing shows: every block drops
    edge, _ = _trap(dev, [(0, None, 10, 16, 3, 5)])      # the first column of block (1, 2): block (1, 1) has alpha 0 and its column 15 shows
    want = torch.zeros_like(base)
    want[0, 1, 1] = want[0, 1, 2] = 1
    assert torch.equal(edge, want)
    inner, _ = _trap(dev, [(0, None, 10, 17, 3, 5)])     # one texel further in: block (1, 1) drops
    want[0, 1, 1] = 0
    assert torch.equal(inner, want)
    corner, _ = _trap(dev, [(1, None, 16, 16, 3, 5)])    # the corner texel of block (2, 2): the three blocks around the corner stay
    want = torch.zeros_like(base)
    want[1, 1, 1] = want[1, 1, 2] = want[1, 2, 1] = want[1, 2, 2] = 1
    assert torch.equal(corner, want)


def test_trap_b_c_one_byte_of_a_showing_texel_keeps_a_block_dynamic(dev):
    vis = (0, None, 3, 3, 3, 9)                                        # block (0, 0) of plane 0: one visible texel
    still, _ = _trap(dev, [vis])
    assert int(still[0, 0, 0]) == 1 and int(still.sum()) == 1
    moving, tr = _trap(dev, [vis, (0, TT - 1, 3, 4, 1, 7)])           # the last frame's green byte of the texel beside it: it shows
    assert int(moving[0, 0, 0]) == TT and int(moving.sum()) == TT and int(tr.moves.sum()) == 1
    hidden, tr = _trap(dev, [vis, (0, TT - 1, 6, 6, 1, 7)])           # the same byte three texels away: it cannot show
    assert int(hidden[0, 0, 0]) == 1 and int(hidden.sum()) == 1 and bool(tr.demoted[0, 0, 0]) and int(tr.dif.sum()) == 1 and int(tr.moves.sum()) == 0


def test_trap_d_alpha_in_one_frame_only_keeps_the_block(dev):
    one, tr = _trap(dev, [(1, 1, 12, 12, 3, 1)])                      # alpha byte 1 in frame 1 alone, block (1, 1) of plane 1
    assert int(one[1, 1, 1]) == TT and int(one.sum()) == TT and not bool(tr.dropped[1, 1, 1])


def test_trap_e_bytes_past_the_planes_edge_never_count(dev):
    vis = (0, None, 5, 26, 3, 9)                                       # the plane's last column (x = 26) in the ragged block (0, 3): lx = 2
    base, _ = _trap(dev, [vis])
    assert int(base[0, 0, 3]) == 1 and int(base.sum()) == 1
    # stored texels at x = 27 (lx = 3, beside the visible one) and below the plane in block (2, 0) (y = 20: ly = 4): other bytes in the last frame, alpha > 0
    past, tr = _trap(dev, [vis], [(0, 0, 3, TT - 1, 5, 3, 1, 99), (0, 0, 3, TT - 1, 5, 3, 3, 200), (0, 2, 0, 1, 4, 2, 3, 200)])
    assert torch.equal(past, base) and bool(tr.demoted[0, 0, 3]) and bool(tr.dropped[0, 2, 0])


# ---- 3. frames --------------------------------------------------------------------------------------------------------------------------------------
def _pair(c, bg_color):
    a, b = copy.copy(c.bp), copy.copy(c.t)
    a.bg_color = b.bg_color = bg_color
    return a, b


@pytest.mark.parametrize("name", NAMES)
def test_frames_of_the_trimmed_pool_are_the_sources(cases, name):
    c = cases[name]
    for bg_color in ("", BG):
        src, trm = _pair(c, bg_color)
        for label, (f0, n) in BS.RUNS.items():
            for cam in range(3):
                ext, intr = c.poses([cam])
                want, got = (p.render(c.H, c.W, ext, intr, list(range(f0, f0 + n))) for p in (src, trm))
                assert got[0].shape == (n, 3, c.H, c.W) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (name, label, cam)
        ext, intr = c.poses([cam for cam, _ in BS.PATH])
        want, got = (p.render_path(c.H, c.W, ext, intr, [t for _, t in BS.PATH]) for p in (src, trm))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and 0.2 < float((want[1] > 0).float().mean())
        ext, intr = c.poses([cam for cam, _ in c.times])
        want, got = (p.render_path(c.H, c.W, ext, intr, [t for _, t in c.times], fractional=True) for p in (src, trm))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("name", NAMES)
def test_display_frames_of_the_trimmed_pool_are_the_sources(cases, name):
    c = cases[name]
    for bg in BS.BGS:
        src, trm = _pair(c, _bg_string(bg))
        for channels in (3, 4):
            ext, intr = c.poses([cam for cam, _ in BS.PATH])
            want, got = (p.render_display(c.H, c.W, ext, intr, [t for _, t in BS.PATH], channels=channels) for p in (src, trm))
            assert got.dtype == torch.uint8 and got.shape == (len(BS.PATH), c.H, c.W, channels) and torch.equal(got, want) and float(want.float().std()) > 1.0
            ext, intr = c.poses([cam for cam, _ in c.times])
            want, got = (p.render_display(c.H, c.W, ext, intr, [t for _, t in c.times], channels=channels, fractional=True) for p in (src, trm))
            assert torch.equal(got, want)
            ext, intr = c.poses([1, 1, 1])      # a run on one camera: the run entry
            want, got = (p.render_display(c.H, c.W, ext, intr, [1, 2, 3], channels=channels) for p in (src, trm))
            assert torch.equal(got, want)


# ---- 4. the texels --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_unpacked_texels_outside_dropped_blocks(cases, name):
    c = cases[name]
    lay = c.bp.layout
    want, got = c.bp.unpack_frames(range(lay.T)).cpu(), c.t.unpack_frames(range(lay.T)).cpu()
    dropped = c.tr.dropped.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :lay.Hs, :lay.Ws]
    demoted = c.tr.demoted.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :lay.Hs, :lay.Ws]
    culled = torch.tensor(BS.rgba8_bytes(c.bp.culled_rgba8), dtype=torch.uint8)
    assert bool((got.permute(0, 2, 3, 1, 4)[dropped] == culled).all()) and int(dropped.sum()) > 0
    rest = ~dropped & ~demoted
    assert torch.equal(got.permute(0, 2, 3, 1, 4)[rest], want.permute(0, 2, 3, 1, 4)[rest])
    assert torch.equal(got.permute(0, 2, 3, 1, 4)[demoted], want[:, :1].expand_as(want).permute(0, 2, 3, 1, 4)[demoted])      # frame 0 in every frame
    assert torch.equal(got.permute(0, 2, 3, 1, 4)[c.tr.show], want.permute(0, 2, 3, 1, 4)[c.tr.show])                          # whatever shows is untouched
    assert torch.equal(got, c.tr.clip)


# ---- 5. a visible culled texel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shared", "exact"])
def test_a_visible_culled_texel_drops_no_block(cases, name):
    from videoloop3d_amd.baked import BakedPool
    c = cases[name]
    culled = 7 | 11 << 8 | 13 << 16 | 9 << 24
    src = BakedPool(c.bp.pool, c.bp.layout, c.bp.quad_keep, c.bp.spec, BG, c.bp.camera, culled, quad_dyn=c.bp.quad_dyn)
    t = src.trimmed()
    lay = src.layout
    tr = TS.trim(lay.blocks, src.pool, lay.T, lay.Hs, lay.Ws, culled, src.quad_keep, c.tile)
    assert t.trim_report["blocks_dropped"] == 0 == int(tr.dropped.sum()) and t.trim_report["quads_dropped"] > 0 and t.trim_report["blocks_demoted"] > 0
    assert torch.equal(t.layout.blocks.cpu(), tr.blocks) and torch.equal(t.pool.cpu(), tr.pool)
    assert torch.equal(t.quad_keep.cpu().bool(), tr.keep) and torch.equal(t.quad_dyn.cpu().bool(), tr.dyn)
    ext, intr = c.poses([cam for cam, _ in BS.PATH])
    want, got = (p.render_path(c.H, c.W, ext, intr, [t_ for _, t_ in BS.PATH]) for p in (src, t))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    ext, intr = c.poses([cam for cam, _ in c.times])
    for channels in (3, 4):
        want, got = (p.render_display(c.H, c.W, ext, intr, [t_ for _, t_ in c.times], channels=channels, fractional=True) for p in (src, t))
        assert torch.equal(got, want)


# ---- 6. idempotence, the source untouched ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_idempotent_and_the_source_is_untouched(cases, name):
    c = cases[name]
    again = c.t.trimmed()
    assert torch.equal(again.pool, c.t.pool) and torch.equal(again.layout.blocks, c.t.layout.blocks) and again.layout.n_slots == c.t.layout.n_slots
    assert torch.equal(again.quad_keep, c.t.quad_keep) and torch.equal(again.quad_dyn, c.t.quad_dyn)
    r = again.trim_report
    assert r["blocks_dropped"] == r["blocks_demoted"] == r["quads_dropped"] == r["quads_demoted"] == 0 and r["slots_after"] == r["slots_before"]
    bp = c.bp
    for now, then in zip((bp.pool, bp.layout.blocks, bp.quad_keep, bp.quad_dyn), c.before):
        assert torch.equal(now, then)
    assert c.t.pool.data_ptr() != bp.pool.data_ptr() and c.t.layout is not bp.layout and c.t.layout.blocks.data_ptr() != bp.layout.blocks.data_ptr()
    assert bp.trim_report is None and bp.layout.n_slots * 64 == bp.pool.shape[0]


# ---- 7. the package ------------------------------------------------------------------------------------------------------------------------------------
def test_the_trimmed_package_plays_the_same_frames(dev, tmp_path):
    from videoloop3d_amd import tiles
    from videoloop3d_amd.baked import bake_pool, culled_texel_rgba8, open_viewer_package
    from videoloop3d_amd.export import read_viewer_package, save_viewer_package
    model, Hm, Wm, K = BM.pool_model(dev, BG, exact=True)
    _edit_model(model, inner_only=True)
    inproc = bake_pool(model)
    t = inproc.trimmed()
    keep, dyn = t.quad_keep.cpu().bool(), t.quad_dyn.cpu().bool()
    keep0, dyn0 = model.quad_keep.cpu().bool(), (model.quad_keep & model.quad_dyn).cpu().bool()
    assert int((keep0 & ~keep).sum()) > 0 and int((dyn0 & keep & ~dyn).sum()) > 0
    # the scene empties no plane, no rim row or column of the quad grid, and neither mesh: both packages derive the same planes, origin and step
    assert torch.equal(keep.flatten(1).any(1), keep0.flatten(1).any(1)) and keep.any(0).any(1)[[0, -1]].all() and keep.any(0).any(0)[[0, -1]].all()
    assert bool(dyn.any()) and bool((keep & ~dyn).any())
    poses = np.tile(np.eye(4, dtype=np.float32)[None, :3], (2, 1, 1))
    views = (poses, np.tile(K.astype(np.float32)[None], (2, 1, 1)), np.array([1.0, 100.0]))
    full, lean = str(tmp_path / "full"), str(tmp_path / "lean")
    save_viewer_package(model, full, *views)
    save_viewer_package(model, lean, *views, quad_maps=(t.quad_keep, t.quad_dyn))
    pf, pl = read_viewer_package(full), read_viewer_package(lean)
    assert np.array_equal(pf["planedepth"], pl["planedepth"]) and pf["origin"] == pl["origin"] and pf["step"] == pl["step"] and pf["tile"] == pl["tile"]
    planes = keep.flatten(1).any(1)
    assert torch.equal(pl["quad_keep"], keep[planes]) and torch.equal(pl["quad_dyn"], dyn[planes])
    culled = culled_texel_rgba8("sigmoid", "sigmoid")
    a, b = (open_viewer_package(d, dev, bg_color=BG, culled_rgba8=culled) for d in (full, lean))
    ext, intr = _model_poses(K, [cam for cam, _ in BS.PATH])
    for channels in (3, 4):
        want, got = (p.render_display(Hm, Wm, ext, intr, [t_ for _, t_ in BS.PATH], channels=channels) for p in (a, b))
        assert torch.equal(got, want) and float(want.float().std()) > 1.0
    times = [(0, 1.0), (1, 0.0), (2, 1.5), (0, 2.125), (1, 2.7), (2, 5.25)]
    ext, intr = _model_poses(K, [cam for cam, _ in times])
    want, got = (p.render_path(Hm, Wm, ext, intr, [t_ for _, t_ in times], fractional=True) for p in (a, b))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # the opened pool's kept-quad texels are the in-process trimmed pool's
    T = int(model.frm_num)
    texels = tiles.quad_to_texel_mask(keep, t.layout.Hs, t.layout.Ws, t.layout.tile)[planes]
    assert torch.equal(b.unpack_frames(range(T)).cpu().permute(0, 2, 3, 1, 4)[texels], t.unpack_frames(range(T)).cpu()[planes].permute(0, 2, 3, 1, 4)[texels])
    # an opened package trims like the pool it was written from
    ta = a.trimmed()
    assert torch.equal(ta.quad_keep.cpu().bool(), keep[planes]) and torch.equal(ta.quad_dyn.cpu().bool(), dyn[planes])
    assert torch.equal(ta.layout.blocks.cpu(), t.layout.blocks.cpu()[planes]) and ta.layout.n_slots == t.layout.n_slots      # (a plane without quads has no slots)

    def faces(d):
        return sum(1 for line in open(os.path.join(d, "geometry.obj")) if line.startswith("f "))

    def png_bytes(d):
        return os.path.getsize(os.path.join(d, "static.png")) + sum(os.path.getsize(os.path.join(d, "dynamic", f)) for f in os.listdir(os.path.join(d, "dynamic")))
    print(f"faces {faces(full)} -> {faces(lean)}, PNG bytes {png_bytes(full)} -> {png_bytes(lean)}; {t.trim_report}")
    assert faces(lean) == 2 * int(keep.sum()) < faces(full) == 2 * int(keep0.sum()) and png_bytes(lean) < png_bytes(full)


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, cases):
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd.baked import BakedPool
    lib = L.lib()
    bp = cases["exact"].bp
    lay = bp.layout
    D, T, Hs, Ws = lay.D, lay.T, lay.Hs, lay.Ws
    need = int(lib.vl3d_baked_trim_scratch_bytes(D, Hs, Ws))
    assert need >= D * Hs * Ws and need % 256 == 0 and int(lib.vl3d_baked_trim_scratch_bytes(0, Hs, Ws)) == 0
    scratch = torch.zeros(need, dtype=torch.uint8, device=dev)
    slots = torch.full(lay.blocks.shape, -7, dtype=torch.int32, device=dev)
    tclass = torch.full((D, Hs, Ws), 77, dtype=torch.uint8, device=dev)
    st = L.stream_ptr(dev)

    def classify(D=D, T=T, Hs=Hs, Ws=Ws, blocks=L.ptr(lay.blocks), pool=L.ptr(bp.pool), scr=L.ptr(scratch), nbytes=need, sl=L.ptr(slots), tc=L.ptr(tclass)):
        return lib.vl3d_baked_trim_classify(D, T, Hs, Ws, blocks, pool, lay.n_slots, bp.culled_rgba8, scr, nbytes, sl, tc, st)
    for kw in (dict(D=0), dict(T=0), dict(Hs=0), dict(Ws=0), dict(D=65536), dict(blocks=None), dict(pool=None), dict(scr=None), dict(sl=None),
               dict(tc=None), dict(nbytes=need - 1), dict(nbytes=0), dict(tc=L.ptr(scratch))):
        assert classify(**kw) == 1, kw      # VL3D_EINVAL
        assert len(lib.vl3d_last_error()) > 0
    new_pool = torch.full_like(cases["exact"].t.pool, 55)
    nb, nn = cases["exact"].t.layout.blocks, cases["exact"].t.layout.n_slots

    def move(D=D, T=T, Hs=Hs, Ws=Ws, blocks=L.ptr(lay.blocks), pool=L.ptr(bp.pool), new_blocks=L.ptr(nb), out=L.ptr(new_pool)):
        return lib.vl3d_baked_trim_move(D, T, Hs, Ws, blocks, pool, lay.n_slots, new_blocks, out, nn, st)
    for kw in (dict(D=0), dict(T=0), dict(Hs=0), dict(Ws=0), dict(D=65536), dict(blocks=None), dict(pool=None), dict(new_blocks=None), dict(out=None),
               dict(out=L.ptr(bp.pool))):
        assert move(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((slots == -7).all()) and bool((tclass == 77).all()) and bool((new_pool == 55).all()) and not bool(scratch.any())      # nothing launched
    assert classify() == 0 and move() == 0
    torch.cuda.synchronize()
    assert torch.equal(new_pool, cases["exact"].t.pool) and torch.equal(slots.cpu().long(), cases["exact"].tr.size)
    host = BakedPool(bp.pool.cpu(), copy.copy(lay), bp.quad_keep.cpu(), bp.spec, "", None, bp.culled_rgba8)
    with pytest.raises(RuntimeError, match="on the host"):
        host.trimmed()
