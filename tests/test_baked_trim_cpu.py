"""The trim rule of a baked pool on the host (tests/baked_trim_statement.py) against the project's fp64 oracle (tests/baked_statement.py), and the
`quad_maps=` of the export -- no device.

The rule is exact, not a quality trade: the trimmed pool, read as a clip, renders the frames of the untrimmed one BIT FOR BIT, in the oracle's fp32
and fp64 evaluation, at every (camera, frame) of baked_statement.PATH and every (camera, loop time) of TIMES (integer times, fractions, the loop
seam, the last float32 below T), with the old quad map and with the new one.  The scenes are the two pools of baked_models.fp64_scenes() (D = 4,
T = 5; 40 x 72 texels block aligned, and 30 x 70 in tiles of 6 x 10 straddling the 8 x 8 blocks with ragged last blocks), edited so that every
third kept quad has alpha byte 0 and every second dynamic quad repeats frame 0 (baked_trim_statement.edit_scene).  Every comparison is
torch.equal or an integer equality."""
import os
import types

import numpy as np
import pytest
import torch

import baked_models as BM
import baked_statement as BS
import baked_trim_statement as TS

SEL = [(c, int(t)) for c, t in BS.PATH] + [(c, float(t)) for c, t in BS.TIMES]


@pytest.fixture(scope="module")
def scenes():
    """name -> the storage of fp64_scenes(), its edited pool, the rule's result on it"""
    out = {}
    for name, st in BM.fp64_scenes().items():
        if st.kind != "pool":
            continue
        pool, _ = TS.edit_scene(st)
        D, T, Hs, Ws = st.scene.dims
        tr = TS.trim(st.lay.blocks, pool, T, Hs, Ws, BS.CULLED, st.keep, st.tile)
        out[name] = types.SimpleNamespace(st=st, pool=pool, tr=tr, clip=BS.pool_as_clip(st.lay.blocks, pool, T, Hs, Ws, BS.CULLED), dims=(D, T, Hs, Ws))
    return out


def _frames(s, clip, keep, dtype):
    sc = s.st.scene
    return [BS.render(clip, sc.homos, c, t, sc.H, sc.W, sc.spec, keep, dtype) for c, t in SEL]


def _same(a, b):
    return all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["pool_shared", "pool_exact"])
def test_the_trimmed_clip_renders_the_oracles_frames(scenes, name):
    s = scenes[name]
    tr, e = s.tr, s.st.lay.blocks
    stored = int((e >= 0).sum())
    print(f"[{name}] stored blocks {stored}, dropped {int(tr.dropped.sum())}, demoted {int(tr.demoted.sum())}, slots {s.st.lay.n_slots} -> {tr.n_slots}, "
          f"quads off the map {int((s.st.keep & ~tr.keep).sum())} of {int(s.st.keep.sum())}, dynamic quads {int((s.st.keep & s.st.dyn).sum())} -> {int(tr.dyn.sum())}")
    # the scene cannot become trivial silently: blocks are dropped and demoted, quads leave the map, and static, dynamic and unstored blocks remain
    assert int(tr.dropped.sum()) > 0 and int(tr.demoted.sum()) > 0 and tr.n_slots < s.st.lay.n_slots and int((s.st.keep & ~tr.keep).sum()) > 0
    nb = tr.blocks
    assert int(((nb >= 0) & ((nb & 1) == 1)).sum()) > 0 and int(((nb >= 0) & ((nb & 1) == 0)).sum()) > 0
    assert not bool((tr.keep & ~s.st.keep).any())
    # the figures of the rule's first check on the oracle (docs/kernels/K9_baked_playback.md "Trimming the pool"): stored, dropped, demoted, slots, quads off
    want = {"pool_shared": (135, 25, 42, 559, 282, 25, 75), "pool_exact": (97, 1, 18, 269, 196, 19, 57)}[name]
    assert (stored, int(tr.dropped.sum()), int(tr.demoted.sum()), s.st.lay.n_slots, tr.n_slots, int((s.st.keep & ~tr.keep).sum()), int(s.st.keep.sum())) == want
    for dtype in (torch.float32, torch.float64):
        want = _frames(s, s.clip, s.st.keep, dtype)
        assert float(torch.stack([a for _, a in want]).mean()) > 0.1      # (something is seen)
        assert _same(want, _frames(s, tr.clip, s.st.keep, dtype)), (name, dtype, "old quad map")
        assert _same(want, _frames(s, tr.clip, tr.keep, dtype)), (name, dtype, "new quad map")
        assert _same(want, _frames(s, s.clip, tr.keep, dtype)), (name, dtype, "new quad map on the untrimmed clip")


def test_the_rule_is_idempotent(scenes):
    for name, s in scenes.items():
        D, T, Hs, Ws = s.dims
        again = TS.trim(s.tr.blocks, s.tr.pool, T, Hs, Ws, BS.CULLED, s.tr.keep, s.st.tile)
        assert torch.equal(again.blocks, s.tr.blocks) and torch.equal(again.pool, s.tr.pool)
        assert torch.equal(again.keep, s.tr.keep) and torch.equal(again.dyn, s.tr.dyn)


def test_dropping_on_own_alpha_alone_changes_a_frame(scenes):
    """straight RGBA: a footprint that straddles a zero-alpha block and a visible neighbour blends the block's stored COLOUR, and a dropped block
    reads culled_rgba8's.  Every visible stored block of an even block column whose right neighbour is one too gets alpha byte 0 on its own 64 texels
    only: the rule keeps them all (their edge columns show), the variant that looks at a block's own alpha drops them -- and renders other frames."""
    s = scenes["pool_shared"]
    D, T, Hs, Ws = s.dims
    e = s.st.lay.blocks
    vis_block = torch.nn.functional.max_pool2d(s.tr.vis[:, None].float(), 8, 8)[:, 0] > 0      # (40 x 72: block aligned)
    ok = (e >= 0) & vis_block
    left = torch.zeros_like(ok)
    left[:, :, 0:-1:2] = ok[:, :, 0:-1:2] & ok[:, :, 1::2]      # visible stored blocks of an even column whose right neighbour (odd, left as it is) is one too
    assert int(left.sum()) >= 10
    pool = s.pool.clone()
    for d, by, bx in left.nonzero().tolist():
        slot, n = int(e[d, by, bx]) >> 1, (T if int(e[d, by, bx]) & 1 else 1)
        pool[slot * 64:(slot + n) * 64, 3] = 0
        assert int(pool[slot * 64:(slot + n) * 64, :3].max()) > 13      # its colour is not the culled texel's
    good = TS.trim(e, pool, T, Hs, Ws, BS.CULLED, s.st.keep, s.st.tile)
    bad = TS.trim(e, pool, T, Hs, Ws, BS.CULLED, s.st.keep, s.st.tile, own_alpha_only=True)
    assert not bool(good.dropped[left].any()) and bool(bad.dropped[left].all())
    clip = BS.pool_as_clip(e, pool, T, Hs, Ws, BS.CULLED)
    sc = s.st.scene
    same = {}
    for tag, tr in (("rule", good), ("own alpha", bad)):
        same[tag] = all(torch.equal(BS.render(clip, sc.homos, c, 0, sc.H, sc.W, sc.spec, s.st.keep, torch.float64)[0],
                                    BS.render(tr.clip, sc.homos, c, 0, sc.H, sc.W, sc.spec, s.st.keep, torch.float64)[0]) for c in range(3))
    assert same["rule"] and not same["own alpha"], same


def test_a_scene_where_nothing_trims_returns_the_same_table():
    """every stored texel visible, every dynamic block moving: the table, the pool and quad_keep come back as they went in"""
    st = BM.fp64_scenes()["pool_exact"]
    D, T, Hs, Ws = st.scene.dims
    src = st.source.clone()
    src[..., 3] = src[..., 3].clamp(min=1)
    src[:, 1:, :, :, 0] = src[:, :1, :, :, 0] ^ 1      # every texel of a dynamic block differs from frame 0 (static blocks keep frame 0 alone)
    pool = BM.scatter_pool(st.lay, src, torch.ones((1, 4), dtype=torch.uint8))
    tr = TS.trim(st.lay.blocks, pool, T, Hs, Ws, BS.CULLED, st.keep, st.tile)
    assert int(tr.dropped.sum()) == 0 and int(tr.demoted.sum()) == 0 and tr.n_slots == st.lay.n_slots
    assert torch.equal(tr.blocks, st.lay.blocks.cpu()) and torch.equal(tr.pool, pool) and torch.equal(tr.keep, st.keep)
    assert not bool((st.keep & st.dyn & ~tr.dyn).any())      # (more quads move here than are dynamic: the edit touches static tiles inside dynamic blocks)


def test_one_frame_makes_every_dynamic_block_static(scenes):
    from videoloop3d_amd.packed import PackedLayout
    s = scenes["pool_exact"]
    st = s.st
    D, _, Hs, Ws = s.dims
    lay = PackedLayout(st.keep, st.dyn, 1, Hs, Ws, st.tile)
    assert lay.n_dynamic > 0
    pool = BM.scatter_pool(lay, st.source[:, :1], torch.zeros((1, 4), dtype=torch.uint8))
    tr = TS.trim(lay.blocks, pool, 1, Hs, Ws, BS.CULLED, st.keep, st.tile)
    was_dyn = (lay.blocks >= 0) & ((lay.blocks & 1) == 1)
    assert int(((tr.blocks >= 0) & ((tr.blocks & 1) == 1)).sum()) == 0 and torch.equal(tr.demoted, was_dyn & ~tr.dropped) and int(tr.demoted.sum()) > 0
    assert not bool(tr.dyn.any()) and not bool(tr.moves.any()) and tr.n_slots == int((tr.blocks >= 0).sum())


def test_the_products_quad_reduction_is_the_statements():
    """baked.quad_any (two matrix products, what trimmed() reduces its texel maps with) against one quad_to_texel_mask per quad, on both layouts,
    on ragged planes, and on quads smaller than two texels"""
    from videoloop3d_amd.baked import quad_any
    g = torch.Generator().manual_seed(5)
    for Hs, Ws, QH, QW, tile in ((40, 72, 5, 9, None), (38, 67, 4, 6, None), (30, 70, 5, 7, (6, 10)), (7, 5, 6, 4, None), (9, 11, 2, 3, None), (4, 6, 2, 3, (2, 2))):
        for density in (0.002, 0.05, 0.5):
            m = torch.rand((3, Hs, Ws), generator=g) < density
            assert torch.equal(quad_any(m, QH, QW, tile), TS.quad_any(m, (3, QH, QW), tile)), (Hs, Ws, QH, QW, tile, density)


# ---- the export: save_viewer_package(quad_maps=) ------------------------------------------------------------------------------------------------------
def _views(K):
    poses = np.tile(np.eye(4, dtype=np.float32)[None, :3], (2, 1, 1))
    return poses, np.tile(K.astype(np.float32)[None], (2, 1, 1)), np.array([1.0, 100.0])


def _faces(dir):
    return sum(1 for line in open(os.path.join(dir, "geometry.obj")) if line.startswith("f "))


def _drop_and_demote(model):
    """(keep', dyn') of a host model: an inner kept static quad dropped, a dynamic quad demoted -- chosen so that every plane, the first and last row
    and column of the quad grid, and both meshes keep a quad (the package then derives the same planes, origin and step)"""
    keep, dyn = model.quad_keep.cpu().bool(), (model.quad_keep & model.quad_dyn).cpu().bool()
    k2, d2 = keep.clone(), dyn.clone()
    inner = (keep & ~dyn)[:, 1:-1, 1:-1].nonzero()[0]
    k2[int(inner[0]), int(inner[1]) + 1, int(inner[2]) + 1] = False
    q = dyn.nonzero()[0]
    d2[tuple(int(v) for v in q)] = False
    for m in (k2,):
        assert torch.equal(m.flatten(1).any(1), keep.flatten(1).any(1)) and m.any(0).any(1)[[0, -1]].all() and m.any(0).any(0)[[0, -1]].all()
    assert bool(d2.any()) and bool((k2 & ~d2).any())
    return k2, d2


def test_package_holds_exactly_the_given_maps(tmp_path):
    from videoloop3d_amd.export import read_viewer_package, save_viewer_package
    model, _, _, K = BM.tile_exact_model(torch.device("cpu"), "")
    k2, d2 = _drop_and_demote(model)
    planes = k2.flatten(1).any(1)
    save_viewer_package(model, str(tmp_path / "a"), *_views(K), quad_maps=(k2, d2))
    pk = read_viewer_package(str(tmp_path / "a"))
    assert torch.equal(pk["quad_keep"], k2[planes]) and torch.equal(pk["quad_dyn"], d2[planes])
    assert _faces(str(tmp_path / "a")) == 2 * int(k2.sum())
    save_viewer_package(model, str(tmp_path / "b"), *_views(K))
    assert _faces(str(tmp_path / "b")) == 2 * int(model.quad_keep.sum()) > _faces(str(tmp_path / "a"))
    # a lattice model may drop quads
    lattice, _, _, K = BM.pool_model(torch.device("cpu"), "", exact=False)
    keep, dyn = lattice.quad_keep.cpu().bool(), (lattice.quad_keep & lattice.quad_dyn).cpu().bool()
    k3 = keep.clone()
    inner = keep[:, 1:-1, 1:-1].nonzero()[0]
    k3[int(inner[0]), int(inner[1]) + 1, int(inner[2]) + 1] = False
    assert k3.any(0).any(1)[[0, -1]].all() and k3.any(0).any(0)[[0, -1]].all() and torch.equal(k3.flatten(1).any(1), keep.flatten(1).any(1))
    save_viewer_package(lattice, str(tmp_path / "c"), *_views(K), quad_maps=(k3, k3 & dyn))
    pk = read_viewer_package(str(tmp_path / "c"))
    planes = k3.flatten(1).any(1)
    assert torch.equal(pk["quad_keep"], k3[planes]) and torch.equal(pk["quad_dyn"], (k3 & dyn)[planes]) and _faces(str(tmp_path / "c")) == 2 * int(k3.sum())


def test_maps_that_are_no_subsets_and_a_lattice_demotion_are_refused(tmp_path):
    from videoloop3d_amd.export import reference_state_dict, save_viewer_package
    model, _, _, K = BM.tile_exact_model(torch.device("cpu"), "")
    keep, dyn = model.quad_keep.cpu().bool(), (model.quad_keep & model.quad_dyn).cpu().bool()
    more = keep.clone()
    more[tuple(int(v) for v in (~keep).nonzero()[0])] = True
    with pytest.raises(ValueError, match="quad_keep"):
        save_viewer_package(model, str(tmp_path), *_views(K), quad_maps=(more, dyn))
    promoted = dyn.clone()
    promoted[tuple(int(v) for v in (keep & ~dyn).nonzero()[0])] = True
    with pytest.raises(ValueError, match="quad_dyn"):
        reference_state_dict(model, quad_maps=(keep, promoted))
    dropped = keep.clone()
    dropped[tuple(int(v) for v in dyn.nonzero()[0])] = False
    with pytest.raises(ValueError, match="quad_dyn"):      # dynamic, but not kept
        reference_state_dict(model, quad_maps=(dropped, dyn))
    with pytest.raises(ValueError, match="quad grid"):
        reference_state_dict(model, quad_maps=(keep[:, :-1], dyn[:, :-1]))
    lattice, _, _, K = BM.pool_model(torch.device("cpu"), "", exact=False)
    keep, dyn = lattice.quad_keep.cpu().bool(), (lattice.quad_keep & lattice.quad_dyn).cpu().bool()
    demoted = dyn.clone()
    demoted[tuple(int(v) for v in dyn.nonzero()[0])] = False
    with pytest.raises(ValueError, match="may only drop"):
        save_viewer_package(lattice, str(tmp_path), *_views(K), quad_maps=(keep, demoted))


def test_without_the_keyword_the_files_are_todays(tmp_path):
    from videoloop3d_amd.export import save_viewer_package
    model, _, _, K = BM.tile_exact_model(torch.device("cpu"), "")
    a = save_viewer_package(model, str(tmp_path / "a"), *_views(K))
    b = save_viewer_package(model, str(tmp_path / "b"), *_views(K), quad_maps=None)
    c = save_viewer_package(model, str(tmp_path / "c"), *_views(K), quad_maps=(model.quad_keep, model.quad_keep & model.quad_dyn))
    assert [os.path.relpath(p, tmp_path / "a") for p in a] == [os.path.relpath(p, tmp_path / "b") for p in b] and len(a) == 3 + int(model.frm_num)
    for pa, pb, pc in zip(a, b, c):
        assert open(pa, "rb").read() == open(pb, "rb").read(), pa
        assert open(pa, "rb").read() == open(pc, "rb").read(), pa      # (the model's own maps on a host model: the host bake, the same files)
