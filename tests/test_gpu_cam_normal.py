"""The camera normal equations on the device -- vl3d_render_cam_normal through render.render_normal_equations,
PlaneModel.camera_normal_equations and poses.refine_cameras_gn -- against tests/normal_statement.py: the forward-mode Jacobian of the CPU oracle
in fp64 and its sums, bound B = m max |oracle in fp32 - oracle in fp64| over the normalised entries, no floor (m = 16 on exact-coordinate
scenes, 4 elsewhere).  Every figure is printed before it is asserted.  The shapes are the smallest at which the kernel can go wrong: a
33 x 131 frame is a ragged last tile in x and in y and 27 workgroups for the finish."""
import dataclasses

import pytest
import torch

import camera_statement as CS
import normal_statement as NS
import render_statement as RS
from test_gpu_camera_grad import _model

pytestmark = pytest.mark.gpu

SCENES = CS.scenes()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _solve(dev, scene, stack, dh, tgt, w, window=(0, 0), **kw):
    import videoloop3d_amd.render as R
    keep = None if scene.keep is None else scene.keep.to(dev)
    A, b, cost = R.render_normal_equations(stack.to(dev), scene.homos.to(dev), dh.to(dev), tgt.to(dev), scene.H, scene.W, scene.spec, window=window,
                                           quad_keep=keep, weight=None if w is None else w.to(dev), **kw)
    P = len(dh)
    assert A.dtype == b.dtype == cost.dtype == torch.float64 and A.device == dev and tuple(A.shape) == (P, P) and tuple(b.shape) == (P,) and cost.dim() == 0
    return A.cpu(), b.cpu(), cost.cpu()


def _check(dev, scene, tag, Tn=RS.T, P=7, kind="random", window=(0, 0), stack=None, Dn=RS.D, key=None):
    stack = RS.make_stack(scene, Tn, Dn=Dn) if stack is None else stack
    dh, tgt, w = NS.tangents(scene, P), NS.target(scene, Tn), NS.weights(scene, Tn, window, kind)
    st = NS.statement(scene, stack, dh, tgt, w, window=window, key=key)
    assert st.unsafe <= CS.UNSAFE_CAP
    got = _solve(dev, scene, stack, dh, tgt, w, window)
    assert torch.equal(got[0], got[0].T)      # both triangles written, from one sum
    st.check(f"{tag}, P = {P}, weight {kind}", got)
    return got


@pytest.mark.parametrize("name", sorted(SCENES))
def test_seven_scenes(dev, name):
    """D = 4, T = 3, P = 7 (the eight-column build, one column idle), a weight map: partial waves, partial tile rows, an odd frame count"""
    _check(dev, SCENES[name], "T = 3", key=("gpu", name))


@pytest.mark.parametrize("P", [1, 6, 7, 8])
@pytest.mark.parametrize("name", ["lattice", "perspective", "utils_mpi"])
def test_parameter_counts(dev, name, P):
    """P = 1 and 6: the six-column build (five columns idle, none idle); 7 and 8: the eight-column build"""
    _check(dev, SCENES[name], "T = 2", Tn=2, P=P)


@pytest.mark.parametrize("Tn", [1, 2, 3])
@pytest.mark.parametrize("name", ["minify", "perspective", "utils_mpi"])
def test_frame_counts(dev, name, Tn):
    _check(dev, SCENES[name], f"T = {Tn}", Tn=Tn, P=6)


def test_five_planes(dev):
    for name, scene in RS.views(CS.HS, CS.WS, Dn=5).items():
        if name in ("minify", "perspective"):
            assert scene.homos.shape[0] == 5
            _check(dev, scene, "D = 5", P=6, Dn=5)


@pytest.mark.parametrize("name", ["lattice", "perspective", "utils_mpi"])
def test_window_offset(dev, name):
    """window = (row0, col0): the 28 x 124 window at (5, 7) of the 33 x 131 frame"""
    window, (h, w) = (5, 7), (28, 124)
    sc = dataclasses.replace(SCENES[name], H=h, W=w)
    _check(dev, sc, f"window {window}", P=6, window=window)


@pytest.mark.parametrize("name", ["shared/lattice", "shared/perspective"])
def test_shared_border_quad_map(dev, name):
    _check(dev, RS.quad_scenes()[name], "quad map")


def test_identity_activations_on_opaque_planes(dev):
    """none / none: the look-ahead behind (nearly) opaque samples, once per colour channel, instead of the quotient (S - P) / (1 - a)"""
    act = ("none", "none")
    scenes = dict(RS.views(CS.HS, CS.WS, act=act), utils_mpi=RS.utils_mpi_scene(CS.HS, CS.WS, act=act))
    for name in ("lattice", "lattice-", "perspective", "utils_mpi"):
        sc = scenes[name]
        for P in (6, 7):
            _check(dev, sc, "opaque, none / none", Tn=2, P=P, stack=RS.opaque_stack(sc, 2))


@pytest.mark.parametrize("name", ["lattice+", "magnify"])
def test_without_weight(dev, name):
    """weight = NULL is weight 1 (scenes without unsafe pixels); the 0 / 1 map on a scene with some"""
    none = _check(dev, SCENES[name], "T = 2", Tn=2, P=6, kind="none")
    ones = _check(dev, SCENES[name], "T = 2", Tn=2, P=6, kind="mask")
    assert all(torch.equal(x, y) for x, y in zip(none, ones))
    _check(dev, SCENES["perspective"], "T = 2", Tn=2, P=6, kind="mask")


@pytest.mark.parametrize("name", ["perspective", "utils_mpi"])
def test_two_calls_give_equal_bits(dev, name):
    import videoloop3d_amd.render as R
    sc = SCENES[name]
    stack, dh, tgt, w = RS.make_stack(sc), NS.tangents(sc, 7), NS.target(sc), NS.weights(sc)
    a = _solve(dev, sc, stack, dh, tgt, w)
    b = _solve(dev, sc, stack, dh, tgt, w)
    rgb = R.render_planes(stack.to(dev), sc.homos.to(dev), sc.H, sc.W, sc.spec)[0]
    c = _solve(dev, sc, stack, dh, tgt, w, rgb=rgb)      # the caller's forward picture instead of a forward of its own
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


def test_python_refusals(dev):
    import videoloop3d_amd.render as R
    sc = SCENES["perspective"]
    stack, homos, dh, tgt = RS.make_stack(sc).to(dev), sc.homos.to(dev), NS.tangents(sc, 7).to(dev), NS.target(sc).to(dev)
    call = lambda **kw: R.render_normal_equations(**{**dict(stack=stack, homos=homos, dhomos=dh, target=tgt, H=sc.H, W=sc.W, spec=sc.spec), **kw})      # noqa: E731
    with pytest.raises(RuntimeError, match="float32 stacks only"):
        call(stack=stack.half())
    with pytest.raises(RuntimeError, match="built for the planar convention"):
        call(spec=dataclasses.replace(sc.spec, border="zeros"))
    with pytest.raises(RuntimeError, match="add_uv_noise"):
        call(spec=dataclasses.replace(sc.spec, uv_noise_seed=3))
    with pytest.raises(RuntimeError, match="no kernel variants"):
        call(spec=dataclasses.replace(sc.spec, variant=1))
    tile = RS.quad_scenes()["tile/lattice"]
    with pytest.raises(RuntimeError, match="tile-exact layout"):
        R.render_normal_equations(RS.make_stack(tile).to(dev), tile.homos.to(dev), NS.tangents(tile, 6).to(dev), NS.target(tile).to(dev), tile.H, tile.W,
                                  tile.spec, quad_keep=tile.keep.to(dev))
    with pytest.raises(RuntimeError, match=r"dhomos must be \[P,D,3,3\]"):
        call(dhomos=torch.cat([dh, dh[:2]]))      # P = 9
    with pytest.raises(RuntimeError, match=r"dhomos must be \[P,D,3,3\]"):
        call(dhomos=dh[:0])
    with pytest.raises(RuntimeError, match="target must be"):
        call(target=tgt[:, :-1])
    with pytest.raises(RuntimeError, match="weight must be"):
        call(weight=torch.ones((1, sc.H, sc.W), device=dev))
    with pytest.raises(RuntimeError, match="rgb must be"):
        call(rgb=tgt[:1])
    with pytest.raises(RuntimeError, match="MI355X only"):
        call(target=tgt.cpu())
    A, b, cost = call()
    assert not A.requires_grad and bool(torch.isfinite(A).all())


def test_abi_refusals(dev):
    """the codes, a sentence in vl3d_last_error, and `out` untouched (nothing launched)"""
    import videoloop3d_amd._lib as L
    import videoloop3d_amd.render as R
    scene = SCENES["perspective"]
    D, Tn, P = 4, 2, 6
    stack = RS.make_stack(scene, Tn).to(dev)
    homos, dh, tgt = scene.homos.to(dev), NS.tangents(scene, P).to(dev), NS.target(scene, Tn).to(dev)
    rgb, _ = R.render_planes(stack, homos, scene.H, scene.W, scene.spec)
    keep = torch.ones((D, 4, 8), dtype=torch.uint8, device=dev)
    out = torch.full((P * P + P + 1,), 7.0, dtype=torch.float64, device=dev)
    NULL = L.C.c_void_p(0)

    def call(qk=None, QH=0, QW=0, short=0, P=P, ptrs=None, **fields):
        desc = R._desc(stack, scene.H, scene.W, scene.spec, 0, 0)
        for k, v in fields.items():
            setattr(desc, k, v)
        ok = R._desc(stack, scene.H, scene.W, scene.spec, 0, 0)
        nb = int(L.lib().vl3d_render_cam_normal_scratch_bytes(ok, 6))
        assert nb == 27 * (21 + 6 + 1) * 8      # 3 x 9 tiles of 64 x 4 pixels, the sums of the six-column build, fp64
        assert int(L.lib().vl3d_render_cam_normal_scratch_bytes(ok, 7)) == int(L.lib().vl3d_render_cam_normal_scratch_bytes(ok, 8)) == 27 * 45 * 8
        assert int(L.lib().vl3d_render_cam_normal_scratch_bytes(ok, 0)) == int(L.lib().vl3d_render_cam_normal_scratch_bytes(ok, 9)) == 0
        scratch = torch.empty(27 * 45, dtype=torch.float64, device=dev)
        p = dict(stack=L.ptr(stack), homos=L.ptr(homos), dhomos=L.ptr(dh), rgb=L.ptr(rgb), target=L.ptr(tgt), out=L.ptr(out))
        p.update(ptrs or {})
        rc = L.lib().vl3d_render_cam_normal(desc, p["stack"], p["homos"], p["dhomos"], P, None if qk is None else L.ptr(qk), QH, QW, p["rgb"], p["target"],
                                            None, p["out"], L.ptr(scratch), nb - short, L.stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, (L.lib().vl3d_last_error() or b"").decode()

    UNSUPPORTED, EINVAL = 3, 1
    cases = [("fp16", dict(stack_dtype=1), UNSUPPORTED), ("affine_planes", dict(coord_mode=L.COORD["affine_planes"]), UNSUPPORTED),
             ("(affine, zeros, post)", dict(border_mode=L.BORDER["zeros"]), UNSUPPORTED), ("baked", dict(act_order=L.ACT_ORDER["baked"]), UNSUPPORTED),
             ("tile-exact grid", dict(qk=keep, QH=-4, QW=-8), UNSUPPORTED), ("cull window", dict(qk=keep, QH=4, QW=8, cull_Hs=80, cull_Ws=280), UNSUPPORTED),
             ("uv noise", dict(uv_noise_seed=3), UNSUPPORTED), ("variant", dict(variant=1), EINVAL), ("null stack", dict(ptrs=dict(stack=NULL)), EINVAL),
             ("misaligned stack", dict(ptrs=dict(stack=L.C.c_void_p(stack.data_ptr() + 4))), EINVAL), ("short scratch", dict(short=8), EINVAL),
             ("D = 0", dict(D=0), EINVAL), ("D = 129", dict(D=129), EINVAL),
             ("P = 0", dict(P=0), EINVAL), ("P = 9", dict(P=9), EINVAL), ("null dhomos", dict(ptrs=dict(dhomos=NULL)), EINVAL),
             ("null rgb", dict(ptrs=dict(rgb=NULL)), EINVAL), ("null target", dict(ptrs=dict(target=NULL)), EINVAL),
             ("null out", dict(ptrs=dict(out=NULL)), EINVAL), ("out not 8-byte aligned", dict(ptrs=dict(out=L.C.c_void_p(out.data_ptr() + 4))), EINVAL)]
    for tag, kw, want in cases:
        rc, msg = call(**kw)
        print(f"{tag}: code {rc}: {msg}")
        assert rc == want and msg.startswith("vl3d_render_cam_normal: "), (tag, rc, msg)
        assert bool((out == 7.0).all()), tag
    rc, _ = call(qk=keep, QH=4, QW=8)
    assert rc == 0 and not bool((out == 7.0).any())


# ---- poses ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learn_focal", [False, True])
@pytest.mark.parametrize("video", [False, True])
def test_model_normal_equations_against_the_oracle_chain(dev, video, learn_focal):
    """PlaneModel.camera_normal_equations on MPMesh, and on MPMeshVid with ts = [0, 2]: the tangents of the float64 chain on the host, the
    kernel's sums -- against the same chain and the forward-mode statement on the oracle"""
    from videoloop3d_amd import poses
    model, K, E_true = _model(dev, video)
    ts, Tn = ([0, 2], 2) if video else (None, 1)
    E = poses.se3_exp(torch.tensor([3e-3, -2e-3, 8e-3, 1e-3, -7e-4, 5e-4], dtype=torch.float64)) @ E_true
    Kp, depths = model.ref_intrin_mpi.detach().cpu().double(), model.planedepth.detach().cpu().double()
    homos, dh = NS.oracle_tangents(Kp, depths, E, K, learn_focal)
    mh, mdh = poses.camera_tangents(model, E, K, learn_focal)
    scale = dh.abs().amax((1, 2, 3), keepdim=True)
    print(f"tangents: product against oracle chain, max difference {float(((mdh - dh).abs() / scale).max()):.1e} of each parameter's largest entry")
    assert float((mh - homos).abs().max()) <= 2.0 ** -22 * float(homos.abs().max()) and float(((mdh - dh).abs() / scale).max()) <= 2.0 ** -22
    sc = RS.Scene("MPMeshVid ts = [0, 2]" if video else "MPMesh", homos, model.H, model.W, CS.HS, CS.WS, model.spec)
    stack = model.stack.detach().cpu()
    stack = stack if ts is None else stack[:, ts]
    tgt, w = NS.target(sc, Tn), NS.weights(sc, Tn)
    st = NS.statement(sc, stack, dh, tgt, w)
    assert st.unsafe <= CS.UNSAFE_CAP
    before = model.stack.detach().clone()
    A, b, cost = model.camera_normal_equations(model.H, model.W, E, K, tgt, ts=ts, learn_focal=learn_focal, weight=w)
    assert A.device == dev and A.dtype == torch.float64 and torch.equal(model.stack.detach(), before)
    st.check(f"P = {len(dh)}", (A.cpu(), b.cpu(), cost.cpu()))


def test_model_refusals(dev):
    model, K, E = _model(dev, False)
    tgt = torch.zeros((1, model.H, model.W, 3))
    model.tile_own = (9, 17)
    with pytest.raises(RuntimeError, match="camera_normal_equations: .*tile-exact layout"):
        model.camera_normal_equations(model.H, model.W, E, K, tgt)
    model.tile_own = None
    model.atlas_exact = True
    with pytest.raises(RuntimeError, match="camera_normal_equations: atlas_exact"):
        model.camera_normal_equations(model.H, model.W, E, K, tgt)
    model.atlas_exact = False
    model.rgb_mlp_type = "rgb_sh"
    with pytest.raises(RuntimeError, match="camera_normal_equations: .*view-dependent colour head"):
        model.camera_normal_equations(model.H, model.W, E, K, tgt)


def test_gauss_newton_refinement(dev):
    """the setting of test_gpu_camera_grad.test_refinement (camera_statement.REFINE): three Levenberg-Marquardt steps at damping 1e-3 bring rotation
    and translation error below 1e-2 of their start (60 Adam steps: below 1e-1); the stack keeps its bits"""
    from videoloop3d_amd import poses
    g = CS.REFINE
    model, K, E_true = _model(dev, False)
    with torch.no_grad():
        target = model.render_cameras(g["H"], g["W"], E_true[None], K[None])[0][None].clone()      # [V = 1, T = 1, H, W, 3]
    start = poses.se3_exp(torch.tensor(g["xi"], dtype=torch.float64)) @ E_true
    r0, t0 = (float(v) for v in poses.pose_error(start, E_true))
    before = model.stack.detach().clone()
    E, Kr, hist, cov = poses.refine_cameras_gn(model, target, start[None], K[None], steps=3, damping=1e-3)
    r1, t1 = (float(v) for v in poses.pose_error(E[0], E_true))
    sd = torch.sqrt(torch.diagonal(cov[0]))
    print(f"rotation {r0:.2e} -> {r1:.2e} ({r1 / r0:.2e}), translation {t0:.2e} -> {t1:.2e} ({t1 / t0:.2e}), cost {hist[0]}; standard deviations {sd.tolist()}")
    assert torch.equal(model.stack.detach(), before) and model.stack.requires_grad and torch.equal(Kr[0], K)
    assert len(hist) == 1 and len(hist[0]) == 4 and min(hist[0]) < hist[0][0]
    assert tuple(cov.shape) == (1, 6, 6) and cov.dtype == torch.float64 and bool((torch.linalg.eigvalsh(cov[0]) > 0).all())
    assert r1 < 1e-2 * r0 and t1 < 1e-2 * t0


def test_gauss_newton_refinement_with_focal_length(dev):
    """the same start and a focal length 5e-4 off: within three steps the focal length is back to 1e-5 relative (the oracle in fp64: 5e-8 after 2)"""
    from videoloop3d_amd import poses
    g = CS.REFINE
    model, K, E_true = _model(dev, False)
    with torch.no_grad():
        target = model.render_cameras(g["H"], g["W"], E_true[None], K[None])[0][None].clone()
    start = poses.se3_exp(torch.tensor(g["xi"], dtype=torch.float64)) @ E_true
    K0 = poses._focal_scaled(K, torch.log(torch.tensor(1 + 5e-4, dtype=torch.float64)))
    before = model.stack.detach().clone()
    E, Kr, hist, cov = poses.refine_cameras_gn(model, target, start[None], K0[None], steps=3, damping=1e-3, learn_focal=True)
    fx, fy = abs(float(Kr[0, 0, 0] / K[0, 0]) - 1), abs(float(Kr[0, 1, 1] / K[1, 1]) - 1)
    r0, t0 = (float(v) for v in poses.pose_error(start, E_true))
    r1, t1 = (float(v) for v in poses.pose_error(E[0], E_true))
    print(f"focal error 5e-4 -> {fx:.2e} / {fy:.2e}, rotation {r1 / r0:.2e}, translation {t1 / t0:.2e} of the start, cost {hist[0]}")
    assert torch.equal(model.stack.detach(), before) and tuple(cov.shape) == (1, 7, 7)
    assert torch.equal(Kr[0, :, 2], K[:, 2])      # the principal point is not an unknown
    assert fx <= 1e-5 and fy <= 1e-5
