"""The disparity kernels on the MI355X (include/vl3d.h "Disparity"; csrc/vl3d_render_disp.hip) against the fp64 statement of
tests/disparity_statement.py -- the CPU oracle's layers and composite times the affine rows of render.depth_rows, sharing no code with the
kernels -- on the float clip (fp32 / fp16; dense, shared-border culled at three keep densities, tile-exact), the baked clip and the baked pool
(the five storages of tests/test_gpu_baked_fp64.py), as runs and as a camera path, then through the models.

Shapes (tests/disparity_models.py): D = 5, clips of 5 frames, planes of 21 x 75 texels, an output of 13 x 70 -- a full 64-pixel row segment
plus a ragged one, and a ragged tile row; one case with D = 70 on planes of 16 x 24 texels for the plane-mask word boundary.

Bound: per scene and output, B = 4 max |statement in fp32 - statement in fp64| over the safe pixels, no floor; unsafe pixels (within 1e-3
texel of a plane edge or a quad boundary) are not compared -- tests/test_disparity_cpu.py holds their share to 1 % and shows that the comparison
fails under planted faults.  Every check prints B and the measured maximum.  Beside the statement: alpha is 0 exactly where the colour entry's
is; a baked source's alpha has the bits of the colour entry's float sink; a frame has the same bits alone, in a longer run and on a path; the
pool has the bits of the clip entry on the unpacked texels; an out-of-range path index leaves its frame unwritten; every refusal returns its
status and message and leaves disp untouched."""
import copy
import types

import numpy as np
import pytest
import torch

import baked_models as BM
import baked_statement as BS
import disparity_models as DM
import disparity_statement as DS
import package_models as PM
from oracle import mpv_oracle

pytestmark = pytest.mark.gpu

STORAGES = ["dense", "shared", "exact", "pool_shared", "pool_exact"]      # (tests/test_gpu_baked_fp64.py: STORAGES)
FLOAT_STORAGES = ["dense", "shared keep 0", "shared keep 0.3", "shared keep 1", "exact"]
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_CACHE = {}


def _cached(key, make):
    """a reference computed once, shared among the tests that need it, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _qk(keep, dev):
    return None if keep is None else keep.to(torch.uint8).to(dev)


# ---- 1. the float entry -----------------------------------------------------------------------------------------------------------------------
def _float_case(dev, s, cam, runs, tag, colour=True):
    """the runs of one float scene under one camera: statement within B, alpha == 0 where the colour entry's is, frame bits independent of the run"""
    from videoloop3d_amd import render as R
    stack, homos, qk = s.stack.to(dev), s.homos[cam].to(dev), _qk(s.keep, dev)
    got = {}
    for name, (f0, n) in runs.items():
        disp, alpha = R.render_frame_run_disparity(stack, f0, n, homos, s.rows[cam], s.H, s.W, s.spec, quad_keep=qk)
        assert disp.shape == (n, s.H, s.W) and disp.dtype == torch.float32 and alpha.shape == disp.shape
        st = _cached((tag, cam, f0, n), lambda: DS.clip_statement(f"{tag} | {s.name}", s.stack, s.homos, s.rows, BS.run_sel(cam, f0, n), s.H, s.W, s.spec, s.keep))
        st.check(name, disp, alpha)
        if colour:
            _, a_col = R.render_frame_run(stack, f0, n, homos, s.H, s.W, s.spec, quad_keep=qk)
            assert torch.equal(alpha == 0, a_col == 0), (tag, name, int(((alpha == 0) != (a_col == 0)).sum()))
        for i in range(n):
            got.setdefault(f0 + i, []).append((disp[i].clone(), alpha[i].clone()))
    for t, frames in got.items():      # a frame rendered in several runs: the same bits
        for d, a in frames[1:]:
            assert torch.equal(d, frames[0][0]) and torch.equal(a, frames[0][1]), (tag, t)
    return got


@pytest.mark.parametrize("storage", FLOAT_STORAGES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_float_entry_against_the_statement(dev, dtype, storage):
    s = _cached(("float scenes", dtype, "sigmoid"), lambda: DM.float_scenes(dtype))[storage]
    got = _float_case(dev, s, 0, DM.RUNS, f"float {dtype} sigmoid {storage}")
    assert sorted(got) == [1, 2, 3] and len(got[1]) == 2 and len(got[3]) == 2      # frames 1 .. 3, frame 3 alone and inside the run of 3
    a = got[2][0][1]
    if storage == "shared keep 0":
        assert float(a.abs().max()) == 0.0 and float(got[2][0][0].abs().max()) == 0.0      # nothing kept: nothing composited
    else:
        assert 0.3 < float((a > 0).double().mean()) < 1.0      # hard-cut edges (and culled quads) inside the view


@pytest.mark.parametrize("storage", FLOAT_STORAGES)
def test_float_entry_with_another_activation(dev, storage):
    """clamp (with a sigmoid colour: a pair the colour entry takes): alpha is 0 over whole regions of a covered plane, so the zero pattern is
    the blend's as well as the coverage's"""
    s = _cached(("float scenes", torch.float32, "clamp"), lambda: DM.float_scenes(torch.float32, alpha_act="clamp"))[storage]
    _float_case(dev, s, 1, {"run of 3": DM.RUNS["run of 3"]}, f"float clamp {storage}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("act", ["relu", "abs", "none"])
def test_float_entry_takes_every_alpha_activation(dev, act, dtype):
    """the activations the colour entry does not take as alpha_act, fp16 included: the statement alone"""
    s = _cached(("float scenes", dtype, act), lambda: DM.float_scenes(dtype, alpha_act=act))["shared keep 0.3"]
    _float_case(dev, s, 2, {"run of 2": DM.RUNS["run of 2"]}, f"float {dtype} {act}", colour=False)


def test_float_entry_plane_mask_word_boundary(dev):
    """D = 70: the plane list walks both 64-bit words"""
    s = _cached("d70", DM.scene_d70)
    got = _float_case(dev, s, DM.CAM70, {"one frame": (0, 1)}, "float D = 70")
    # planes behind the word boundary contribute: the same clip without them renders another map
    from videoloop3d_amd import render as R
    keep64 = s.keep.clone()
    keep64[64:] = False
    d64, _ = R.render_frame_run_disparity(s.stack.to(dev), 0, 1, s.homos[DM.CAM70].to(dev), s.rows[DM.CAM70], s.H, s.W, s.spec, quad_keep=_qk(keep64, dev))
    assert float((d64[0] - got[0][0][0]).abs().max()) > 1e-4


# ---- 2. the baked clip and the baked pool --------------------------------------------------------------------------------------------------------
def _baked_calls(s, dev):
    """a storage of disparity_models.baked_scenes on the device -> its disparity and colour calls: run(cam, f0, n), path(cams, ts) and the
    float sink's col_run / col_path"""
    from videoloop3d_amd import render as R
    S = s.scene
    homos, rows, qk = S.homos.to(dev), s.rows.to(dev), _qk(s.keep, dev)
    if s.kind == "pool":
        lay, pool, kw = copy.copy(s.lay).to(dev), s.pool.to(dev), dict(quad_keep=qk, culled_rgba8=s.culled)
        return types.SimpleNamespace(
            run=lambda cam, f0, n, **o: R.render_frame_run_disparity_baked_pool(lay, pool, f0, n, homos[cam], rows[cam], S.H, S.W, S.spec, **kw, **o),
            path=lambda cams, ts, **o: R.render_path_disparity_baked_pool(lay, pool, cams, ts, homos, rows, S.H, S.W, S.spec, **kw, **o),
            col_run=lambda cam, f0, n: R.render_frame_run_baked_pool(lay, pool, f0, n, homos[cam], S.H, S.W, S.spec, **kw),
            col_path=lambda cams, ts: R.render_path_baked_pool(lay, pool, cams, ts, homos, S.H, S.W, S.spec, **kw),
            src=lambda: R._baked_pool("test", lay, pool, homos, S.spec, qk, s.culled)[1], homos=homos, rows=rows)
    clip = s.clip.to(dev)
    return types.SimpleNamespace(
        run=lambda cam, f0, n, **o: R.render_frame_run_disparity_baked(clip, f0, n, homos[cam], rows[cam], S.H, S.W, S.spec, quad_keep=qk, **o),
        path=lambda cams, ts, **o: R.render_path_disparity_baked(clip, cams, ts, homos, rows, S.H, S.W, S.spec, quad_keep=qk, **o),
        col_run=lambda cam, f0, n: R.render_frame_run_baked(clip, f0, n, homos[cam], S.H, S.W, S.spec, quad_keep=qk),
        col_path=lambda cams, ts: R.render_path_baked(clip, cams, ts, homos, S.H, S.W, S.spec, quad_keep=qk),
        src=lambda: R._baked_dense("test", clip, homos, S.spec, qk)[1], homos=homos, rows=rows)


BAKED_CASES = [(n, "alpha 0") for n in STORAGES] + [(n, "visible") for n in STORAGES if n.startswith("pool")]


@pytest.mark.parametrize("name, culled", BAKED_CASES, ids=[f"{n}-culled {c}" for n, c in BAKED_CASES])
def test_baked_entries_against_the_statement(dev, name, culled):
    word = BS.CULLED if culled == "alpha 0" else DM.CULLED_VISIBLE
    s = _cached(("baked scenes", word), lambda: DM.baked_scenes(word))[name]
    S, k = s.scene, _baked_calls(s, dev)
    frames = {}
    for tag, (f0, n) in DM.RUNS.items():
        disp, alpha = k.run(0, f0, n)
        _cached(("baked", word, name, tag), lambda: DS.scene_statement(S, s.rows, BS.run_sel(0, f0, n))).check(tag, disp, alpha)
        assert torch.equal(alpha, k.col_run(0, f0, n)[1]), (name, tag)      # the bits of the colour entry's float sink (frame pairs there)
        for i in range(n):
            frames.setdefault(f0 + i, []).append((disp[i].clone(), alpha[i].clone()))
    for t, fr in frames.items():
        for d, a in fr[1:]:
            assert torch.equal(d, fr[0][0]) and torch.equal(a, fr[0][1]), (name, t)
    cams, ts = [c for c, _ in BS.PATH], [t for _, t in BS.PATH]
    disp, alpha = k.path(cams, ts)
    st = _cached(("baked", word, name, "path"), lambda: DS.scene_statement(S, s.rows, BS.PATH))
    st.check("path", disp, alpha)
    assert 0.3 < float((st.alpha > 0).double().mean()) < 1.0
    assert torch.equal(alpha, k.col_path(cams, ts)[1]), name
    for i, (c, t) in enumerate(BS.PATH):      # frame i of a path: the bits of the run of that frame alone
        d1, a1 = k.run(c, t, 1)
        assert torch.equal(disp[i], d1[0]) and torch.equal(alpha[i], a1[0]), (name, i)
    if s.kind == "pool":      # the bits of the clip entry on the unpacked texels
        from videoloop3d_amd import render as R
        unpacked = S.clip.to(dev)
        d2, a2 = R.render_path_disparity_baked(unpacked, cams, ts, k.homos, k.rows, S.H, S.W, S.spec, quad_keep=_qk(s.keep, dev))
        assert torch.equal(disp, d2) and torch.equal(alpha, a2), name


@pytest.mark.parametrize("name", STORAGES)
def test_an_out_of_range_path_index_leaves_its_frame_unwritten(dev, name):
    """the wrapper range-checks the indices (IndexError); behind it the kernels check them again: a camera or a frame out of range -- here
    uploaded past the wrapper -- returns before any load or store"""
    from videoloop3d_amd import render as R
    s = _cached(("baked scenes", BS.CULLED), lambda: DM.baked_scenes(BS.CULLED))[name]
    S, k = s.scene, _baked_calls(s, dev)
    with pytest.raises(IndexError):
        k.path([0, 3], [1, 1])
    with pytest.raises(IndexError):
        k.path([0, 1], [1, DM.T])
    cams, ts = [0, 3, 1, -1, 2, 0], [1, 1, DM.T, 2, -1, 4]      # frames 1 .. 4 are out of range, each in its own way
    idx = torch.tensor([cams, ts], dtype=torch.int32, device=dev)
    disp = torch.full((len(cams), S.H, S.W), SENTINEL, device=dev)
    alpha = torch.full((len(cams), S.H, S.W), SENTINEL, device=dev)
    R._baked_disparity("test", k.src(), len(cams), 0, (3, idx), k.homos, k.rows, S.H, S.W, S.spec, (disp, alpha))
    for i in (1, 2, 3, 4):
        assert bool((disp[i] == SENTINEL).all()) and bool((alpha[i] == SENTINEL).all()), (name, i)
    for i in (0, 5):
        d1, a1 = k.run(cams[i], ts[i], 1)
        assert torch.equal(disp[i], d1[0]) and torch.equal(alpha[i], a1[0]), (name, i)


# ---- 3. the models ------------------------------------------------------------------------------------------------------------------------------------
_view, _model_statement = DM.model_view, DM.model_statement


def test_mpmeshvid_tile_exact_and_packed_against_the_statement(dev):
    """the two layouts the materialised-layer path never served: a tile-exact model (runs of consecutive frames read in place, other lists
    split into runs) and a packed one (the requested frames unpacked)"""
    model, Hm, Wm, K = BM.tile_exact_model(dev, "")
    ext, Kc = _view(Hm, Wm, K)
    ts = [1, 2, 4]
    disp, alpha = model.render_disparity(Hm, Wm, ext, Kc, ts=ts)
    assert disp.shape == (3, Hm, Wm)
    _model_statement("tile-exact model", model, model.stack.detach().cpu(), ext, Kc, Hm, Wm, ts).check("ts 1, 2, 4", disp, alpha)
    for i, t in enumerate(ts):      # split into runs: the bits of every frame alone
        d1, a1 = model.render_disparity(Hm, Wm, ext, Kc, ts=[t])
        assert torch.equal(d1[0], disp[i]) and torch.equal(a1[0], alpha[i])
    with torch.no_grad():
        _, var = model.render(Hm, Wm, ext, Kc, torch.tensor(ts))
    assert var["disp_norm"] is None and torch.equal(var["alpha"] == 0, alpha == 0)      # render keeps today's values
    with pytest.raises(RuntimeError):      # (the layout the materialised path refuses)
        model.render(Hm, Wm, ext, Kc, torch.tensor(ts), need_layers=True)
    packed, Hp, Wp, Kp = BM.pool_model(dev, "", exact=False)
    dense = packed.stack.detach().cpu().clone()
    packed.pack_()
    assert packed.packed is not None
    ext, Kc = _view(Hp, Wp, Kp)
    disp, alpha = packed.render_disparity(Hp, Wp, ext, Kc, ts=[0, 3])
    _model_statement("packed model", packed, dense, ext, Kc, Hp, Wp, [0, 3]).check("ts 0, 3", disp, alpha)


def test_mpmeshvid_lattice_against_the_materialised_path(dev):
    """a shared-border (lattice) model: against the statement, and against variables['disp_norm'] of the existing materialised-layer path
    within the sum of both paths' bounds -- each an fp32 evaluation of the statement, held to B"""
    model, Hm, Wm, K = BM.pool_model(dev, "", exact=False)
    ext, Kc = _view(Hm, Wm, K)
    ts = [2, 3]
    disp, alpha = model.render_disparity(Hm, Wm, ext, Kc, ts=ts)
    st = _model_statement("lattice model", model, model.stack.detach().cpu(), ext, Kc, Hm, Wm, ts)
    st.check("ts 2, 3", disp, alpha)
    with torch.no_grad():
        _, var = model.render(Hm, Wm, ext, Kc, torch.tensor(ts), need_layers=True)
    old = var["disp_norm"].detach().cpu().double()
    e_old = float((old - st.disp)[st.safe].abs().max())
    e = float((old - disp.cpu().double())[st.safe].abs().max())
    print(f"materialised disp_norm: max |d| to the statement {e_old:.3e}, to the kernel {e:.3e}; B disp {st.bound[0]:.3e}")
    assert e <= 2 * st.bound[0]


@pytest.mark.parametrize("head", ["direct", "rgb_sh"])
def test_mpmesh_against_the_stage1_oracles_disparity(dev, head):
    """MPMesh.render_disparity -- plain, normalise (MPI.py:494), normalise + by_alpha (MPI.py:564-565) -- against the disparity the stage-1
    oracle forms (oracle.mpv_oracle.mpi_forward's own statements: _layers, overcompose, _inv_depth, evaluated in float64 on the model's
    weights).  Bound: B of the statement plus the oracle's own rounding -- _inv_depth returns float32: 6e-8 relative, on a normalised
    disparity of at most 1 / (1 - near / far) -- ; with by_alpha the quotient q = disp / alpha carries (B_disp + q B_alpha) / alpha."""
    from oracle import mpi_oracle as MO
    m, args, MH, MW, MK, near, far, ext, Kc, h, w = DM.stage1_model(dev, head)
    # the oracle, in float64 where its statements keep the dtype
    stack64 = m.stack.detach().cpu().double()
    mpi_h, mpi_w, planedepth, ref_intrin_mpi, extrins = mpv_oracle._geometry(args, 4, MH, MW, np.eye(4), MK, near, far, ext, stack64.shape[2:4])
    homos = m.plane_homographies(ext, Kc).cpu()      # the model's own float32 homographies: the oracle's differ from them in the last bit
    assert float((homos - mpv_oracle._homos(ref_intrin_mpi, extrins[0:1], Kc[0:1], planedepth)).abs().max()) <= 1e-5
    layers, _ = mpv_oracle._layers(stack64, homos.double(), h, w, args, mpi_h, mpi_w, 0.5, None, None)
    bw = MO.overcompose(layers[..., 3], layers[..., :3])[1]
    a_o = bw.sum(-1)
    inv_z = mpv_oracle._inv_depth(homos, h, w, ref_intrin_mpi, planedepth, extrins[0], 0.5).double()
    norm = (inv_z - 1 / far) / (1 / near - 1 / far)
    want = {"plain": (bw * inv_z[None]).sum(-1), "normalise": (bw * norm[None]).sum(-1),
            "by_alpha": ((bw / a_o.clamp_min(1e-10)[..., None]) * norm[None]).sum(-1)}
    rounding = 2e-7 / (1 - near / far)
    for tag, kw in (("plain", {}), ("normalise", dict(normalise=True)), ("by_alpha", dict(normalise=True, by_alpha=True))):
        disp, alpha = m.render_disparity(h, w, ext, Kc, **kw)
        st = _model_statement(f"MPMesh {head} {tag}", m, m.stack.detach().cpu(), ext, Kc, h, w, [0], (near, far) if kw else None)
        b_d, b_a = st.bound
        err = (disp.cpu().double() - want[tag]).abs()
        if tag == "by_alpha":
            tol = (b_d + want[tag] * b_a) / a_o.clamp_min(1e-10) * 1.01 + rounding
            ok = st.safe & (a_o > 0.05)
        else:
            st.check(tag, disp, alpha)
            tol, ok = torch.full_like(err, b_d + rounding), st.safe
        print(f"[MPMesh {head} | {tag}] oracle's disparity: max |d| {float(err[ok].max()):.3e}, bound {float(tol[ok].max()):.3e}, {int(ok.sum())} pixels")
        assert bool((err <= tol)[ok].all()) and int(ok.sum()) > 100
        assert float((alpha.cpu().double() - a_o)[st.safe].abs().max()) <= b_a


def test_atlas_exact_is_refused_with_a_sentence(dev):
    from videoloop3d_amd.MPI import MPMesh
    m = MPMesh(DM.stage1_args(), 24, 32, np.eye(4), np.array([[28.8, 0, 16], [0, 28.8, 12], [0, 0, 1.0]]), 1.0, 100.0, atlas_exact=True).to(dev).eval()
    with pytest.raises(RuntimeError, match="atlas_exact"):
        m.render_disparity(24, 32, torch.eye(4)[None], m.ref_intrin.cpu()[None])


def _straddling_case(dev, tmp):
    """tests/test_gpu_open_package.py's model of 5 x 7 tiles of 6 x 10 texels (every plane has quads), its in-process pool, its package on
    disk and the package opened again"""
    import test_gpu_open_package as OP
    from videoloop3d_amd.baked import bake_pool, culled_texel_rgba8, open_viewer_package
    from videoloop3d_amd.export import save_viewer_package
    model, Hm, Wm, K = OP.straddling_model(dev, "")
    poses = np.tile(np.eye(4, dtype=np.float32)[None, :3], (2, 1, 1))
    save_viewer_package(model, tmp, poses, np.tile(K.astype(np.float32)[None], (2, 1, 1)), np.array([1.0, 100.0]))
    culled = culled_texel_rgba8("sigmoid", "sigmoid")
    return types.SimpleNamespace(model=model, H=Hm, W=Wm, K=K.astype(np.float32), culled=culled, inproc=bake_pool(model),
                                 opened=open_viewer_package(tmp, dev, bg_color="", culled_rgba8=culled), T=int(model.frm_num))


def test_baked_pool_of_an_opened_package(dev, tmp_path):
    """a pool from open_viewer_package, built from a package export.save_viewer_package wrote: its disparity is the disparity of the pool it
    was exported from, bit for bit -- the opened storage behind the model's spec and camera, as tests/test_gpu_open_package.py compares the
    display frames --; a trimmed pool gives the same bits; with the package's own camera (its own homographies and depth rows) the alpha has
    the bits of its own render_path and the map stays within the fp64 statement's bound of the opened texels."""
    from videoloop3d_amd.baked import BakedPool, _Camera
    c = _straddling_case(dev, str(tmp_path))
    o, p = c.opened, c.inproc
    assert o.layout.D == p.layout.D and torch.equal(o.layout.blocks, p.layout.blocks)
    mixed = BakedPool(o.pool, o.layout, o.quad_keep, c.model.spec, "", _Camera(c.model), c.culled)
    ext = np.stack([PM.tilted_pose(i) for i in range(7)])
    intr = np.stack([c.K] * 7)
    ts = [i % c.T for i in range(7)]
    d_o, a_o = mixed.render_disparity(c.H, c.W, ext, intr, ts)
    d_p, a_p = p.render_disparity(c.H, c.W, ext, intr, ts)
    assert d_o.shape == (7, c.H, c.W) and torch.equal(d_o, d_p) and torch.equal(a_o, a_p)
    assert float(d_p.max()) > 0.05 and 0.2 < float((a_p > 0).double().mean()) < 1.0
    assert torch.equal(a_p, p.render_path(c.H, c.W, ext, intr, ts)[1])
    d_t, a_t = p.trimmed().render_disparity(c.H, c.W, ext, intr, ts)
    assert torch.equal(d_t, d_p) and torch.equal(a_t, a_p)
    # chunks that are runs and chunks that are paths: the same bits
    same = np.stack([ext[1]] * 7)
    d_r, _ = p.render_disparity(c.H, c.W, same, intr, [0, 1, 2, 3, 4, 5, 0], max_batch=3)
    d_q, _ = p.render_disparity(c.H, c.W, same, intr, [0, 1, 2, 3, 4, 5, 0], max_batch=64)
    assert torch.equal(d_r, d_q)
    # the package's own camera
    d_own, a_own = o.render_disparity(c.H, c.W, ext, intr, ts)
    assert torch.equal(a_own, o.render_path(c.H, c.W, ext, intr, ts)[1])
    rows_own = o.camera.depth_rows(o.extrins_to_ref(torch.tensor(ext)), torch.tensor(intr))
    rows_mod = _Camera(c.model).depth_rows(p.extrins_to_ref(torch.tensor(ext)), torch.tensor(intr))
    assert float((rows_own - rows_mod).abs().max()) <= 2e-7 * float(rows_mod.abs().max())      # (the plane depths come back from the package's float32)
    from videoloop3d_amd.baked import path_cameras
    _, homos = path_cameras(o.camera, torch.tensor(ext), torch.tensor(intr))
    scene = BS.Scene("opened package", o.unpack_frames(range(c.T)).cpu(), homos.float(), c.H, c.W, o.spec, o.quad_keep.cpu().bool(), pool=True)
    DS.scene_statement(scene, rows_own, list(zip(range(7), ts))).check("own camera", d_own, a_own)


def test_render_disparity_frames_equals_the_per_frame_calls(dev):
    from videoloop3d_amd.baked import bake_pool
    from videoloop3d_amd.render_video import render_disparity_frames
    model, Hm, Wm, K = BM.tile_exact_model(dev, "")
    ext = np.stack([PM.tilted_pose(0)] * 3 + [PM.tilted_pose(1), PM.tilted_pose(2)])
    intr = np.stack([K.astype(np.float32)] * 5)
    ts = [2, 3, 4, 0, 5]
    got = render_disparity_frames(model, Hm, Wm, ext, intr, ts, max_batch=2)
    assert got.shape == (5, Hm, Wm) and got.dtype == torch.float32
    for i, t in enumerate(ts):
        one, _ = model.render_disparity(Hm, Wm, torch.tensor(ext[i:i + 1]), torch.tensor(intr[i:i + 1]), ts=[t])
        assert torch.equal(got[i], one[0]), i
    baked = bake_pool(model)
    got_b = render_disparity_frames(model, Hm, Wm, ext, intr, ts, max_batch=4, baked=baked)
    for i, t in enumerate(ts):
        one, _ = baked.render_disparity(Hm, Wm, ext[i:i + 1], intr[i:i + 1], [t])
        assert torch.equal(got_b[i], one[0]), i
    assert float(got.max()) > 0.05 and float(got_b.max()) > 0.05


# ---- 4. the refusals -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def buffers(dev):
    """real buffers of the refusal rows' shapes (disparity_models.refusal_desc): nothing is launched on them"""
    t = dict(stack=torch.zeros((2, 5, 8, 8, 4), device=dev), baked=torch.zeros((2, 5, 8, 8, 4), dtype=torch.uint8, device=dev),
             blocks=torch.zeros((2, 1, 1), dtype=torch.int32, device=dev), pool=torch.zeros((6 * 64, 4), dtype=torch.uint8, device=dev),
             homos=torch.eye(3, device=dev).repeat(2, 1, 1).contiguous(), rows=torch.zeros((2, 3), device=dev) + 0.5,
             qk=torch.ones((2, 2, 2), dtype=torch.uint8, device=dev), cull=torch.zeros(64, dtype=torch.int64, device=dev),
             disp=torch.full((3, 4, 6), SENTINEL, device=dev), alpha=torch.full((3, 4, 6), SENTINEL, device=dev),
             idx=torch.zeros((2, 3), dtype=torch.int32, device=dev))
    return t


@pytest.mark.parametrize("entry, fields, over, status, fragment", [pytest.param(*r[1:], id=f"{r[1][12:]}-{r[0]}") for r in DM.refusal_rows()])
def test_refusals_leave_disp_untouched(dev, buffers, entry, fields, over, status, fragment):
    rc, msg = DM.call_refusal(entry, DM.refusal_desc(entry, **fields), {k: v.data_ptr() for k, v in buffers.items()}, over)
    torch.cuda.synchronize()
    assert rc == status, (rc, msg)
    assert msg.startswith(entry.encode() + b": ") and fragment in msg, msg
    assert bool((buffers["disp"] == SENTINEL).all()) and bool((buffers["alpha"] == SENTINEL).all())
