"""Where the plane walk ends (walk_planes / walk_planes_cond, csrc/vl3d_render_core.h): the forward families that walk their planes through
the helper -- the baked clip, the two baked pool kernels, the float disparity and the baked disparity kernels -- at the plane counts at which
the walk stops in another place.

Dense: D = 1, 2, 3 and 5 end after the first fetch, in slot B, in slot A and in slot A on a second trip.
Listed: models of D = 3 whose quad maps keep whole planes {}, {1}, {0, 2} and {0, 1, 2} leave the workgroups 0, 1, 2 and 3 listed planes
(asserted on the plan's own masks: at least four of the six list them all, none more; read back from the float forward's scratch at the same geometry), and one drawn map mixes the counts; a
pool stores something, so its "0 planes" map keeps plane 1's last quad row alone: some workgroups list nothing, the others that plane.  A model of
D = 66 keeps planes 63, 64 and 65 alone, so the walk crosses from the first mask word into the second.

Frames of 23 x 70 pixels: two tile columns (the second ragged), three tile rows; T = 3 for the odd frame pair.  Every case is held to the
fp64 statements of tests/baked_statement.py and disparity_statement.py with their own bounds; the frame pairs are compared bit for bit with
the one-frame kernel (a run of one), a pool with the clip entries on its unpacked texels."""
import copy
import dataclasses
import types

import pytest
import torch

import baked_models as BM
import baked_statement as BS
import disparity_models as DM
import disparity_statement as DS

pytestmark = pytest.mark.gpu

H, W, T = 23, 70, 3
DENSE_D = [1, 2, 3, 5]
WHOLE_PLANES = {"0 planes": (), "1 plane": (1,), "2 planes": (0, 2), "3 planes": (0, 1, 2)}
GRID = (3, 5)      # quads of the baked and disparity models
SC = (1.1, 0.9)      # plane pixel -> texel: 0.9 y - 0.6 keeps the 21 texel rows under all 23 pixel rows (disparity_models.SC: 13 rows)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _qk(keep, dev):
    return None if keep is None else keep.to(torch.uint8).to(dev)


def _whole(Dn, planes, grid):
    keep = torch.zeros((Dn,) + tuple(grid), dtype=torch.bool)
    for d in planes:
        keep[d] = True
    return keep


def _listed_counts(dev, Dn, keep):
    """the planes the plan lists for each 64 x 8 workgroup at this file's geometry: the float forward's scratch (the baked and disparity
    entries launch the same plan kernel over the same tiles) -> (counts, the four 32-bit mask words per workgroup)"""
    from videoloop3d_amd import _lib as L, render as R
    spec = dataclasses.replace(DM.spec_of("shared", "sigmoid", "sigmoid", sc=SC), variant=0x600)
    s = DM.synth.make_plane_stack(Dn, 1, DM.HS, DM.WS, seed=9).to(dev)
    desc = R._desc(s, H, W, spec, 0, 0)
    rgb, alpha = torch.empty((1, H, W, 3), device=dev), torch.empty((1, H, W), device=dev)
    homos = BS.cameras(Dn, H, W)[0].to(dev).float().contiguous()
    with torch.cuda.device(dev):
        qk = R._quad_map(keep.to(dev), Dn)
        cull = R._cull_scratch(desc, dev)
        L.check(L.lib().vl3d_render_fwd(desc, L.ptr(s), L.ptr(homos), *R._qmap(qk, spec), L.ptr(cull), L.ptr(rgb), L.ptr(alpha), None,
                                        L.stream_ptr(dev)), "vl3d_render_fwd")
    tiles = ((W + 63) // 64) * ((H + 7) // 8)
    words = cull.view(torch.int32)[:tiles * 4].cpu().reshape(tiles, 4)
    return [sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in row) for row in words], words


# ---- the baked clip, the pools and the disparity entries ------------------------------------------------------------------------------------------
def _baked_scene(Dn, keep, pool):
    """DM's shapes at another plane count: the clip (or the pool of it through PackedLayout), the three cameras and their rows"""
    homos, rows = BS.cameras(Dn, H, W), DM.camera_rows(Dn, H, W)
    clip = BS.random_clip(Dn, T, DM.HS, DM.WS, seed=7)
    spec = DM.spec_of("shared", sc=SC)
    if pool:
        dyn = keep & (DM.synth.hash_uniform(tuple(keep.shape), seed=12) < 0.5)
        s = BM._pool_storage("pool", keep, dyn, T, DM.HS, DM.WS, None, clip, homos, H, W, spec)
    else:
        s = types.SimpleNamespace(kind="clip", scene=BS.Scene("clip", clip, homos, H, W, spec, keep), clip=clip, keep=keep)
    s.rows = rows
    return s


def _baked_case(dev, s, tag, expect_empty=False):
    """colour (frame pairs and the lone frame of T = 3) and disparity of one storage against their statements; a pool: the clip entries' bits"""
    from videoloop3d_amd import render as R
    S = s.scene
    homos, rows, qk, sel = S.homos.to(dev), s.rows.to(dev), _qk(s.keep, dev), BS.run_sel(0, 0, T)
    if s.kind == "pool":
        lay, pool, kw = copy.copy(s.lay).to(dev), s.pool.to(dev), dict(quad_keep=qk, culled_rgba8=BS.CULLED)
        rgb, alpha = R.render_frame_run_baked_pool(lay, pool, 0, T, homos[0], H, W, S.spec, **kw)
        disp, dalpha = R.render_frame_run_disparity_baked_pool(lay, pool, 0, T, homos[0], rows[0], H, W, S.spec, **kw)
        unpacked = S.clip.to(dev)
        rgb2, alpha2 = R.render_frame_run_baked(unpacked, 0, T, homos[0], H, W, S.spec, quad_keep=qk)
        disp2, _ = R.render_frame_run_disparity_baked(unpacked, 0, T, homos[0], rows[0], H, W, S.spec, quad_keep=qk)
        assert torch.equal(rgb, rgb2) and torch.equal(alpha, alpha2) and torch.equal(disp, disp2), tag
    else:
        clip = s.clip.to(dev)
        rgb, alpha = R.render_frame_run_baked(clip, 0, T, homos[0], H, W, S.spec, quad_keep=qk)
        disp, dalpha = R.render_frame_run_disparity_baked(clip, 0, T, homos[0], rows[0], H, W, S.spec, quad_keep=qk)
    S.statement(sel).check_float(tag, rgb, alpha)
    DS.scene_statement(S, s.rows, sel).check(tag, disp, dalpha)
    assert torch.equal(alpha, dalpha), tag      # the colour entry's alpha bits
    for t in range(T):      # the one-frame kernel (a run of one) gives the frame pairs' bits
        r1, a1 = (R.render_frame_run_baked_pool(lay, pool, t, 1, homos[0], H, W, S.spec, **kw) if s.kind == "pool"
                  else R.render_frame_run_baked(clip, t, 1, homos[0], H, W, S.spec, quad_keep=qk))
        assert torch.equal(r1[0], rgb[t]) and torch.equal(a1[0], alpha[t]), (tag, t)
    assert (float(alpha.abs().max()) == 0.0) == expect_empty, tag


def _float_disparity_case(dev, Dn, keep, tag):
    from videoloop3d_amd import render as R
    homos, rows = BS.cameras(Dn, H, W), DM.camera_rows(Dn, H, W)
    stack = DM.synth.make_plane_stack(Dn, T, DM.HS, DM.WS, seed=9, alpha_bias=-0.5)
    spec = DM.spec_of("dense" if keep is None else "shared", "sigmoid", "sigmoid", sc=SC)
    disp, alpha = R.render_frame_run_disparity(stack.to(dev), 0, T, homos[0].to(dev), rows[0], H, W, spec, quad_keep=_qk(keep, dev))
    DS.clip_statement(tag, stack, homos, rows, BS.run_sel(0, 0, T), H, W, spec, keep).check(tag, disp, alpha)
    _, a_col = R.render_frame_run(stack.to(dev), 0, T, homos[0].to(dev), H, W, spec, quad_keep=_qk(keep, dev))
    assert torch.equal(alpha == 0, a_col == 0), tag


@pytest.mark.parametrize("Dn", DENSE_D)
def test_dense_baked_and_disparity(dev, Dn):
    _baked_case(dev, _baked_scene(Dn, None, False), f"baked dense D {Dn}")
    _float_disparity_case(dev, Dn, None, f"float disparity dense D {Dn}")


@pytest.mark.parametrize("tag", list(WHOLE_PLANES) + ["drawn map"])
def test_listed_baked_pool_and_disparity(dev, tag):
    keep = DM.keep_map(0.4, 3, GRID) if tag == "drawn map" else _whole(3, WHOLE_PLANES[tag], GRID)
    empty = not bool(keep.any())
    counts, _ = _listed_counts(dev, 3, keep)
    if tag == "drawn map":
        assert len(set(counts)) > 1, counts
    else:      # (every plane lies under most of the view: at least four of the six workgroups list all kept planes, none lists more)
        assert max(counts) == len(WHOLE_PLANES[tag]) and counts.count(max(counts)) >= 4, (tag, counts)
    _baked_case(dev, _baked_scene(3, keep, False), f"baked clip, {tag}", empty)
    pool_keep = keep.clone()
    if empty:      # a pool stores something: plane 1's last quad row alone (texel rows from 13.3 on), far from the first tile row's pixels
        pool_keep[1, 2] = True
        counts, _ = _listed_counts(dev, 3, pool_keep)
        assert 0 in counts and max(counts) == 1, counts      # some workgroups list no plane, the others this one
    _baked_case(dev, _baked_scene(3, pool_keep, True), f"baked pool, {tag}")
    _float_disparity_case(dev, 3, keep, f"float disparity, {tag}")


def test_listed_baked_pool_and_disparity_cross_the_mask_word(dev):
    keep = _whole(66, (63, 64, 65), GRID)
    counts, words = _listed_counts(dev, 66, keep)
    full = [r for r, c in zip(words, counts) if c == 3]
    assert len(full) >= 4 and max(counts) == 3, counts
    assert all(int(r[0]) == 0 and int(r[1]) & 0xFFFFFFFF == 0x80000000 and int(r[2]) == 3 and int(r[3]) == 0 for r in full), words
    _baked_case(dev, _baked_scene(66, keep, False), "baked clip, D 66 planes 63 .. 65")
    _baked_case(dev, _baked_scene(66, keep, True), "baked pool, D 66 planes 63 .. 65")
    _float_disparity_case(dev, 66, keep, "float disparity, D 66 planes 63 .. 65")
