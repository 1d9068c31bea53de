"""Camera registration on the device -- vl3d_render_cam_register through render.render_register_equations,
PlaneModel.camera_register_equations and poses.register_cameras -- against tests/register_statement.py: the forward-mode Jacobian of the CPU
oracle in fp64, the per-frame or long-exposure residual with or without the brightness unknowns, and their sums; bound
B = m max |oracle in fp32 - oracle in fp64| over the normalised entries, no floor (m = 16 on exact-coordinate scenes, 4 elsewhere).  Every
figure is printed before it is asserted.  The shapes are camera_statement's: a 33 x 131 frame is two full 64-wide tiles and a 3-pixel tail in
x, a 1-row tail tile in y, 27 workgroups for the finish.  The (J, C) of a (scene, T, P) is computed once on the CPU and shared by the four
combinations of mode and brightness."""
import dataclasses
import math

import pytest
import torch

import camera_statement as CS
import normal_statement as NS
import register_statement as REG
import render_statement as RS
from test_gpu_camera_grad import _model

pytestmark = pytest.mark.gpu

SCENES = CS.scenes()
MODES = [(False, False), (False, True), (True, False), (True, True)]      # (long exposure, brightness unknowns)
POINTS = [(0.0, 0.0), REG.POINT]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _solve(dev, scene, stack, dh, tgt, w, long_exposure, photo, point=(0.0, 0.0), window=(0, 0), **kw):
    """render.render_register_equations; without the brightness unknowns the Python entry evaluates at (0, 0)"""
    import videoloop3d_amd.render as R
    assert photo or point == (0.0, 0.0)
    keep = None if scene.keep is None else scene.keep.to(dev)
    A, b, cost = R.render_register_equations(stack.to(dev), scene.homos.to(dev), dh.to(dev), tgt.to(dev), scene.H, scene.W, scene.spec, window=window,
                                             quad_keep=keep, weight=None if w is None else w.to(dev), long_exposure=long_exposure,
                                             brightness=point if photo else None, **kw)
    Q = len(dh) + 2 * photo
    assert A.dtype == b.dtype == cost.dtype == torch.float64 and A.device == dev and tuple(A.shape) == (Q, Q) and tuple(b.shape) == (Q,) and cost.dim() == 0
    return A.cpu(), b.cpu(), cost.cpu()


def _raw(dev, scene, stack, dh, tgt, w, long_exposure, photo, point):
    """the C entry itself on a dense scene: any (log_gain, bias) with or without the unknowns"""
    import videoloop3d_amd._lib as L
    import videoloop3d_amd.render as R
    assert scene.keep is None
    stack, homos, dh, tgt = stack.to(dev), scene.homos.to(dev).contiguous(), dh.to(dev).contiguous(), tgt.to(dev).contiguous()
    w = None if w is None else w.to(dev).contiguous()
    rgb = R.render_planes(stack, homos, scene.H, scene.W, scene.spec)[0].contiguous()
    desc = R._desc(stack, scene.H, scene.W, scene.spec, 0, 0)
    P = len(dh)
    Q = P + 2 * photo
    nb = int(L.lib().vl3d_render_cam_register_scratch_bytes(desc, P, int(photo)))
    scratch = torch.empty(nb // 8, dtype=torch.float64, device=dev)
    out = torch.empty(Q * Q + Q + 1, dtype=torch.float64, device=dev)
    L.check(L.lib().vl3d_render_cam_register(desc, L.ptr(stack), L.ptr(homos), L.ptr(dh), P, None, 0, 0, L.ptr(rgb), L.ptr(tgt), L.ptr(w),
                                             int(long_exposure), int(photo), point[0], point[1], L.ptr(out), L.ptr(scratch), nb, L.stream_ptr(dev)),
            "vl3d_render_cam_register")
    out = out.cpu()
    return out[:Q * Q].view(Q, Q), out[Q * Q:Q * Q + Q], out[Q * Q + Q]


def _key(scene, Tn, P, window, tag):
    """what the CPU's (J, C) depends on: the scene, the stack (the tag names another than make_stack's), the tangents, the window"""
    return (scene.name, scene.spec.rgb_act, scene.spec.alpha_act, Tn, P, window, tag)


def _check(dev, scene, tag, Tn=RS.T, P=7, kind="random", window=(0, 0), stack=None, modes=MODES, points=(REG.POINT,), raw=False):
    """the modes at `points`; without the brightness unknowns the Python entry evaluates at (0, 0) only -- `raw`: the other points too, through
    the C entry itself (a dense scene, no window)"""
    stack = RS.make_stack(scene, Tn) if stack is None else stack
    dh = NS.tangents(scene, P)
    key = _key(scene, Tn, P, window, tag)
    got = {}
    for long_exposure, photo in modes:
        tgt, w = REG.target(scene, Tn, long_exposure), REG.weights(scene, Tn, long_exposure, window, kind)
        for point in (points if (photo or raw) else [(0.0, 0.0)]):
            st = REG.statement(scene, stack, dh, tgt, w, long_exposure, photo, point, window=window, key=key)
            assert st.unsafe <= CS.UNSAFE_CAP
            if photo or point == (0.0, 0.0):
                res = _solve(dev, scene, stack, dh, tgt, w, long_exposure, photo, point, window)
            else:
                res = _raw(dev, scene, stack, dh, tgt, w, long_exposure, photo, point)
            assert torch.equal(res[0], res[0].T)      # both triangles written, from one sum
            st.check(f"{tag}, P = {P}, weight {kind}, {'long exposure' if long_exposure else 'per frame'}, {'brightness' if photo else 'camera only'} "
                     f"at {point}", res)
            got[long_exposure, photo, point] = res
    return got


@pytest.mark.parametrize("name", sorted(SCENES))
def test_seven_scenes(dev, name):
    """D = 4, T = 3, P = 7 (the eight-column build: 66 sums with the brightness unknowns), a weight map, at (0.2, -0.05): both conventions"""
    _check(dev, SCENES[name], "T = 3")


@pytest.mark.parametrize("P", [6, 7])
@pytest.mark.parametrize("Tn", [1, 2, 3])
@pytest.mark.parametrize("name", ["perspective", "utils_mpi"])
def test_frame_and_parameter_counts(dev, name, Tn, P):
    """T in {1, 2, 3} x P in {6, 7} x mode x brightness at (0, 0) and (0.2, -0.05); without the unknowns the second point goes through the C
    entry itself"""
    _check(dev, SCENES[name], f"T = {Tn}", Tn=Tn, P=P, points=POINTS, raw=True)


@pytest.mark.parametrize("name", ["lattice+", "magnify"])
def test_weights(dev, name):
    """weight = NULL is weight 1 (scenes without unsafe pixels), the 0 / 1 map, the random map"""
    none = _check(dev, SCENES[name], "T = 2", Tn=2, P=6, kind="none")
    ones = _check(dev, SCENES[name], "T = 2", Tn=2, P=6, kind="mask")
    assert all(torch.equal(x, y) for k in none for x, y in zip(none[k], ones[k]))
    _check(dev, SCENES[name], "T = 2", Tn=2, P=6, kind="random")
    _check(dev, SCENES["perspective"], "T = 2", Tn=2, P=6, kind="mask")


@pytest.mark.parametrize("name", ["lattice", "perspective", "utils_mpi"])
def test_window_offset(dev, name):
    """window = (row0, col0): the 28 x 124 window at (5, 7) of the 33 x 131 frame"""
    window, (h, w) = (5, 7), (28, 124)
    sc = dataclasses.replace(SCENES[name], H=h, W=w)
    _check(dev, sc, f"window {window}", P=6, window=window)


@pytest.mark.parametrize("name", ["shared/lattice", "shared/perspective"])
def test_shared_border_quad_map(dev, name):
    _check(dev, RS.quad_scenes()[name], "quad map")


def _clamped_opaque_stack(sc, Tn):
    """render_statement.opaque_stack for a clamp alpha: the opaque blocks hold 1.5, which the clamp makes exactly 1 with slope 0 on both sides
    (at exactly 1 torch's clamp has slope 1 and the kernels' 0: a convention, not what this test is about)"""
    s = RS.opaque_stack(sc, Tn)
    s[..., 3] = torch.where(s[..., 3] == 1.0, torch.full_like(s[..., 3], 1.5), s[..., 3])
    return s


@pytest.mark.parametrize("name", ["lattice", "lattice-", "perspective"])
def test_clamp_alpha_on_opaque_planes(dev, name):
    """none / clamp (the planar convention: the forward of the utils_mpi one is not built for a clamp): the look-ahead behind opaque samples,
    once per colour channel, in a kernel that does not clear J between frames"""
    sc = RS.views(CS.HS, CS.WS, act=("none", "clamp"))[name]
    for P in (6, 7):
        _check(dev, sc, "opaque, none / clamp", Tn=2, P=P, stack=_clamped_opaque_stack(sc, 2))


def test_identity_activations_on_opaque_planes_utils_mpi(dev):
    """none / none under activate-then-sample: the look-ahead of the other convention"""
    sc = RS.utils_mpi_scene(CS.HS, CS.WS, act=("none", "none"))
    for P in (6, 7):
        _check(dev, sc, "opaque, none / none", Tn=2, P=P, stack=RS.opaque_stack(sc, 2))


# ---- anchors ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["perspective", "utils_mpi"])
def test_per_frame_camera_only_is_the_normal_equations(dev, name):
    """photo = 0, per frame, (0, 0): within 2 B of vl3d_render_cam_normal on the same inputs (each is within B of the statement)"""
    import videoloop3d_amd.render as R
    sc = SCENES[name]
    for P in (6, 7):
        stack, dh, tgt, w = RS.make_stack(sc), NS.tangents(sc, P), NS.target(sc), NS.weights(sc)
        st = REG.statement(sc, stack, dh, tgt, w, False, False, key=_key(sc, RS.T, P, (0, 0), "T = 3"))
        a = _solve(dev, sc, stack, dh, tgt, w, False, False)
        n = R.render_normal_equations(stack.to(dev), sc.homos.to(dev), dh.to(dev), tgt.to(dev), sc.H, sc.W, sc.spec, weight=w.to(dev))
        n = tuple(t.cpu() for t in n)
        d = float((st.norm(a) - st.norm(n)).abs().max()) / st.bound
        print(f"[{name}] P = {P}: registration against vl3d_render_cam_normal {d:.3f} B; equal bits: {all(torch.equal(x, y) for x, y in zip(a, n))}")
        assert d <= 2.0


@pytest.mark.parametrize("photo", [False, True])
@pytest.mark.parametrize("name", ["perspective", "utils_mpi"])
def test_one_frame_gives_both_modes_the_same_bits(dev, name, photo):
    sc = SCENES[name]
    stack, dh, tgt, w = RS.make_stack(sc, 1), NS.tangents(sc, 7), NS.target(sc, 1), NS.weights(sc, 1)
    point = REG.POINT if photo else (0.0, 0.0)
    a = _solve(dev, sc, stack, dh, tgt, w, False, photo, point)
    b = _solve(dev, sc, stack, dh, tgt[0].contiguous(), w[0].contiguous(), True, photo, point)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("long_exposure,photo", MODES)
@pytest.mark.parametrize("name", ["perspective", "utils_mpi"])
def test_two_calls_give_equal_bits(dev, name, long_exposure, photo):
    import videoloop3d_amd.render as R
    sc = SCENES[name]
    stack, dh = RS.make_stack(sc), NS.tangents(sc, 7)
    tgt, w = REG.target(sc, RS.T, long_exposure), REG.weights(sc, RS.T, long_exposure)
    point = REG.POINT if photo else (0.0, 0.0)
    a = _solve(dev, sc, stack, dh, tgt, w, long_exposure, photo, point)
    b = _solve(dev, sc, stack, dh, tgt, w, long_exposure, photo, point)
    rgb = R.render_planes(stack.to(dev), sc.homos.to(dev), sc.H, sc.W, sc.spec)[0]
    c = _solve(dev, sc, stack, dh, tgt, w, long_exposure, photo, point, rgb=rgb)      # the caller's forward picture instead of a forward of its own
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))


def test_camera_block_of_the_larger_system(dev):
    """the P x P block, b[:P] and the cost of the system with the brightness unknowns are the sums of the system without them at the same point"""
    sc = SCENES["perspective"]
    stack, dh = RS.make_stack(sc, 2), NS.tangents(sc, 6)
    for long_exposure in (False, True):
        tgt, w = REG.target(sc, 2, long_exposure), REG.weights(sc, 2, long_exposure)
        A, b, cost = _raw(dev, sc, stack, dh, tgt, w, long_exposure, True, REG.POINT)
        A0, b0, cost0 = _raw(dev, sc, stack, dh, tgt, w, long_exposure, False, REG.POINT)
        assert torch.equal(A[:6, :6], A0) and torch.equal(b[:6], b0) and torch.equal(cost, cost0)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_python_refusals(dev):
    import videoloop3d_amd.render as R
    sc = SCENES["perspective"]
    stack, homos, dh, tgt = RS.make_stack(sc).to(dev), sc.homos.to(dev), NS.tangents(sc, 7).to(dev), NS.target(sc).to(dev)
    call = lambda **kw: R.render_register_equations(**{**dict(stack=stack, homos=homos, dhomos=dh, target=tgt, H=sc.H, W=sc.W, spec=sc.spec), **kw})      # noqa: E731
    with pytest.raises(RuntimeError, match="float32 stacks only"):
        call(stack=stack.half())
    with pytest.raises(RuntimeError, match="built for the planar convention"):
        call(spec=dataclasses.replace(sc.spec, border="zeros"))
    with pytest.raises(RuntimeError, match="add_uv_noise"):
        call(spec=dataclasses.replace(sc.spec, uv_noise_seed=3))
    with pytest.raises(RuntimeError, match="no kernel variants"):
        call(spec=dataclasses.replace(sc.spec, variant=1))
    with pytest.raises(RuntimeError, match=r"dhomos must be \[P,D,3,3\]"):
        call(dhomos=torch.cat([dh, dh[:2]]))      # P = 9
    with pytest.raises(RuntimeError, match=r"target must be \[T,H,W,3\]"):
        call(target=tgt[0])
    with pytest.raises(RuntimeError, match=r"target must be \[H,W,3\]"):
        call(long_exposure=True)
    with pytest.raises(RuntimeError, match=r"weight must be \[H,W\]"):
        call(long_exposure=True, target=tgt[0], weight=torch.ones((3, sc.H, sc.W), device=dev))
    with pytest.raises(RuntimeError, match="rgb must be"):
        call(rgb=tgt[:1])
    with pytest.raises(RuntimeError, match="must be finite"):
        call(brightness=(float("nan"), 0.0))
    with pytest.raises(RuntimeError, match="MI355X only"):
        call(target=tgt.cpu())
    A, b, cost = call(long_exposure=True, target=tgt[0], brightness=(0.0, 0.0))
    assert tuple(A.shape) == (9, 9) and not A.requires_grad and bool(torch.isfinite(A).all())


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
    out = torch.full(((P + 2) * (P + 2) + P + 2 + 1,), 7.0, dtype=torch.float64, device=dev)
    NULL = L.C.c_void_p(0)
    ok = R._desc(stack, scene.H, scene.W, scene.spec, 0, 0)
    nbytes = L.lib().vl3d_render_cam_register_scratch_bytes
    assert int(nbytes(ok, 6, 0)) == 27 * 28 * 8 and int(nbytes(ok, 6, 1)) == 27 * (28 + 17) * 8      # 3 x 9 tiles, the sums of the six-column build, fp64
    assert int(nbytes(ok, 7, 0)) == int(nbytes(ok, 8, 0)) == 27 * 45 * 8 and int(nbytes(ok, 7, 1)) == int(nbytes(ok, 8, 1)) == 27 * 66 * 8
    assert int(nbytes(ok, 0, 0)) == int(nbytes(ok, 9, 1)) == int(nbytes(ok, 6, 2)) == int(nbytes(ok, 6, -1)) == 0

    def call(qk=None, QH=0, QW=0, short=0, P=P, ptrs=None, mode=0, photo=1, point=(0.2, -0.05), **fields):
        desc = R._desc(stack, scene.H, scene.W, scene.spec, 0, 0)
        for k, v in fields.items():
            setattr(desc, k, v)
        nb = 27 * 66 * 8
        scratch = torch.empty(27 * 66, dtype=torch.float64, device=dev)
        need = int(nbytes(ok, 6, 1))
        p = dict(stack=L.ptr(stack), homos=L.ptr(homos), dhomos=L.ptr(dh), rgb=L.ptr(rgb), target=L.ptr(tgt), out=L.ptr(out), scratch=L.ptr(scratch),
                 weight=None)
        p.update(ptrs or {})
        rc = L.lib().vl3d_render_cam_register(desc, p["stack"], p["homos"], p["dhomos"], P, None if qk is None else L.ptr(qk), QH, QW, p["rgb"], p["target"],
                                              p["weight"], mode, photo, point[0], point[1], p["out"], p["scratch"], need - short if short else nb,
                                              L.stream_ptr(dev))
        torch.cuda.synchronize()
        return rc, (L.lib().vl3d_last_error() or b"").decode()

    off = lambda t, n: L.C.c_void_p(t.data_ptr() + n)      # noqa: E731
    UNSUPPORTED, EINVAL = 3, 1
    cases = [("fp16", dict(stack_dtype=1), UNSUPPORTED), ("affine_planes", dict(coord_mode=L.COORD["affine_planes"]), UNSUPPORTED),
             ("(affine, zeros, post)", dict(border_mode=L.BORDER["zeros"]), UNSUPPORTED), ("baked", dict(act_order=L.ACT_ORDER["baked"]), UNSUPPORTED),
             ("tile-exact grid", dict(qk=keep, QH=-4, QW=-8), UNSUPPORTED), ("cull window", dict(qk=keep, QH=4, QW=8, cull_Hs=80, cull_Ws=280), UNSUPPORTED),
             ("uv noise", dict(uv_noise_seed=3), UNSUPPORTED), ("variant", dict(variant=1), EINVAL), ("D = 0", dict(D=0), EINVAL), ("D = 129", dict(D=129), EINVAL),
             ("mode = 2", dict(mode=2), EINVAL), ("mode = -1", dict(mode=-1), EINVAL), ("photo = 2", dict(photo=2), EINVAL), ("photo = -1", dict(photo=-1), EINVAL),
             ("log_gain nan", dict(point=(float("nan"), 0.0)), EINVAL), ("log_gain inf", dict(point=(float("inf"), 0.0)), EINVAL),
             ("bias nan", dict(point=(0.0, float("nan"))), EINVAL), ("bias -inf", dict(point=(0.0, float("-inf"))), EINVAL),
             ("log_gain 100 (exp overflows)", dict(point=(100.0, 0.0)), EINVAL),
             ("P = 0", dict(P=0), EINVAL), ("P = 9", dict(P=9), EINVAL),
             ("null stack", dict(ptrs=dict(stack=NULL)), EINVAL), ("null homos", dict(ptrs=dict(homos=NULL)), EINVAL),
             ("null dhomos", dict(ptrs=dict(dhomos=NULL)), EINVAL), ("null rgb", dict(ptrs=dict(rgb=NULL)), EINVAL),
             ("null target", dict(ptrs=dict(target=NULL)), EINVAL), ("null out", dict(ptrs=dict(out=NULL)), EINVAL),
             ("null scratch", dict(ptrs=dict(scratch=NULL)), EINVAL),
             ("misaligned stack", dict(ptrs=dict(stack=off(stack, 4))), EINVAL), ("misaligned dhomos", dict(ptrs=dict(dhomos=off(dh, 2))), EINVAL),
             ("misaligned target", dict(ptrs=dict(target=off(tgt, 1))), EINVAL), ("misaligned weight", dict(ptrs=dict(weight=off(tgt, 2))), EINVAL),
             ("out not 8-byte aligned", dict(ptrs=dict(out=off(out, 4))), EINVAL), ("short scratch", dict(short=8), EINVAL)]
    for tag, kw, want in cases:
        rc, msg = call(**kw)
        print(f"{tag}: code {rc}: {msg}")
        assert rc == want and msg.startswith("vl3d_render_cam_register: "), (tag, rc, msg)
        assert bool((out == 7.0).all()), tag
    rc, _ = call(qk=keep, QH=4, QW=8)
    assert rc == 0 and not bool((out == 7.0).any())


# ---- the model and the poses -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_exposure", [False, True])
def test_model_register_equations_against_the_oracle_chain(dev, long_exposure):
    """PlaneModel.camera_register_equations on MPMeshVid with ts = [0, 2] and the focal length: the tangents of the float64 chain, the
    kernel's sums -- against the same chain and the statement on the oracle"""
    model, K, E_true = _model(dev, True)
    from videoloop3d_amd import poses
    E = poses.se3_exp(torch.tensor([3e-3, -2e-3, 8e-3, 1e-3, -7e-4, 5e-4], dtype=torch.float64)) @ E_true
    Kp, depths = model.ref_intrin_mpi.detach().cpu().double(), model.planedepth.detach().cpu().double()
    homos, dh = NS.oracle_tangents(Kp, depths, E, K, True)
    sc = RS.Scene("MPMeshVid ts = [0, 2]", homos, model.H, model.W, CS.HS, CS.WS, model.spec)
    stack = model.stack.detach().cpu()[:, [0, 2]]
    tgt, w = REG.target(sc, 2, long_exposure), REG.weights(sc, 2, long_exposure)
    st = REG.statement(sc, stack, dh, tgt, w, long_exposure, True, REG.POINT)
    assert st.unsafe <= CS.UNSAFE_CAP
    before = model.stack.detach().clone()
    A, b, cost = model.camera_register_equations(model.H, model.W, E, K, tgt, ts=[0, 2], learn_focal=True, weight=w, long_exposure=long_exposure,
                                                 brightness=REG.POINT)
    assert A.device == dev and A.dtype == torch.float64 and tuple(A.shape) == (9, 9) and torch.equal(model.stack.detach(), before)
    st.check(f"P = 7 + 2, long exposure {long_exposure}", (A.cpu(), b.cpu(), cost.cpu()))


def test_model_refusals(dev):
    model, K, E = _model(dev, False)
    tgt = torch.zeros((1, model.H, model.W, 3))
    model.tile_own = (9, 17)
    with pytest.raises(RuntimeError, match="camera_register_equations: .*tile-exact layout"):
        model.camera_register_equations(model.H, model.W, E, K, tgt)
    model.tile_own = None
    model.atlas_exact = True
    with pytest.raises(RuntimeError, match="camera_register_equations: atlas_exact"):
        model.camera_register_equations(model.H, model.W, E, K, tgt)
    model.atlas_exact = False
    model.rgb_mlp_type = "rgb_sh"
    with pytest.raises(RuntimeError, match="camera_register_equations: .*view-dependent colour head"):
        model.camera_register_equations(model.H, model.W, E, K, tgt)


def _captured(dev, roll, gain, bias, video=True):
    """(model, K, E_true, start, clip [F,H,W,3]): the view's clip rendered at the true camera, started `roll` frames later, exposed by gain, bias"""
    from videoloop3d_amd import poses
    g = CS.REFINE
    model, K, E_true = _model(dev, video)
    with torch.no_grad():
        frames = model.render_cameras(g["H"], g["W"], E_true[None], K[None])[0].clone()
    start = poses.se3_exp(torch.tensor(g["xi"], dtype=torch.float64)) @ E_true
    return model, K, E_true, start, REG.captured_clip(frames, roll, gain, bias)


def _ratios(E, start, E_true):
    from videoloop3d_amd import poses
    r0, t0 = (float(v) for v in poses.pose_error(start, E_true))
    r1, t1 = (float(v) for v in poses.pose_error(E, E_true))
    return r1 / r0, t1 / t0


def test_register_cameras_end_to_end(dev):
    """camera_statement.REFINE at T = 3, the clip started one frame later and exposed by 1.25 x + 0.05: within 8 steps rotation and translation
    error are below 1e-2 of the start, and (log gain, bias) within max(1e-3, 10 x the fp32 oracle's own deviation) of (ln 1.25, 0.05).  The
    oracle in fp32 on the CPU (register_statement.oracle_system under poses.register_loop, 8 steps) ends 2.4e-6 / 6.4e-7 from (ln 1.25, 0.05)
    (in fp64: 2.9e-7 / 9.2e-8), so the tolerance is 1e-3.
    refine_cameras_gn on the same clip's frames does not find the camera: on the oracle its rotation error is 0.62, 0.91, 1.58 of the start
    after 3, 5, 8 steps and its translation error 0.65, 0.46, 0.84 -- it wanders.  At the 8 steps the registration gets, the rotation error
    must end above its start and no component anywhere near the 1e-2 the registration reaches (the two failure modes one at a time, where
    both components end above the start, are test_refine_cameras_gn_loses_the_camera)."""
    from videoloop3d_amd import poses
    model, K, E_true, start, clip = _captured(dev, 1, REG.GAIN, REG.BIAS)
    before = model.stack.detach().clone()
    res = poses.register_cameras(model, clip[None], start[None], K[None], steps=8)
    r, t = _ratios(res.extrinsics[0], start, E_true)
    da, db = abs(float(res.log_gain[0]) - math.log(REG.GAIN)), abs(float(res.bias[0]) - REG.BIAS)
    sd = torch.sqrt(torch.diagonal(res.covariance[0]))
    print(f"register_cameras: rotation {r:.2e}, translation {t:.2e} of the start; log gain off by {da:.1e}, bias by {db:.1e}; cost {res.costs[0]}; "
          f"standard deviations {sd.tolist()}")
    E, _, hist, _ = poses.refine_cameras_gn(model, clip[None], start[None], K[None], steps=8)
    r_gn, t_gn = _ratios(E[0], start, E_true)
    print(f"refine_cameras_gn on the same frames: rotation {r_gn:.2e}, translation {t_gn:.2e} of the start; cost {hist[0]}")
    assert torch.equal(model.stack.detach(), before) and torch.equal(res.intrinsics[0], K)
    assert len(res.costs) == 1 and len(res.costs[0]) == 9 and tuple(res.log_gain.shape) == tuple(res.bias.shape) == (1,)
    assert tuple(res.covariance.shape) == (1, 8, 8) and res.covariance.dtype == torch.float64 and bool((torch.linalg.eigvalsh(res.covariance[0]) > 0).all())
    assert r < 1e-2 and t < 1e-2
    tol = max(1e-3, 10 * 2.4e-6)
    assert da <= tol and db <= tol
    assert r_gn > 1.0 and min(r_gn, t_gn) > 0.1


@pytest.mark.parametrize("what", ["brightness", "loop time"])
def test_refine_cameras_gn_loses_the_camera(dev, what):
    """the two failure modes one at a time, as the oracle in fp64 shows them (tests/test_register_statement_cpu.py): a clip exposed by
    1.25 x + 0.05 (T = 1), and a T = 3 clip started one frame later.  refine_cameras_gn ends above its start in rotation AND translation;
    register_cameras ends below 1e-2 of it"""
    from videoloop3d_amd import poses
    if what == "brightness":
        model, K, E_true, start, clip = _captured(dev, 0, REG.GAIN, REG.BIAS, video=False)
        kw = dict(steps=6, long_exposure=False, fit_brightness=True)
    else:
        model, K, E_true, start, clip = _captured(dev, 1, 1.0, 0.0)
        kw = dict(steps=5, long_exposure=True, fit_brightness=False)
    E, _, hist, _ = poses.refine_cameras_gn(model, clip[None], start[None], K[None], steps=kw["steps"])
    r_gn, t_gn = _ratios(E[0], start, E_true)
    res = poses.register_cameras(model, [clip], start[None], K[None], **kw)
    r, t = _ratios(res.extrinsics[0], start, E_true)
    print(f"[{what}] refine_cameras_gn: rotation {r_gn:.2e}, translation {t_gn:.2e} of the start; register_cameras: {r:.2e} / {t:.2e}, "
          f"log gain {float(res.log_gain[0]):.6f}, bias {float(res.bias[0]):.6f}")
    assert r_gn > 1.0 and t_gn > 1.0
    assert r < 1e-2 and t < 1e-2
    Q = 6 + 2 * kw["fit_brightness"]
    assert tuple(res.covariance.shape) == (1, Q, Q)
    if what == "brightness":
        assert abs(float(res.log_gain[0]) - math.log(REG.GAIN)) <= 1e-3 and abs(float(res.bias[0]) - REG.BIAS) <= 1e-3


def test_register_cameras_refusals(dev):
    from videoloop3d_amd import poses
    model, K, E_true, start, clip = _captured(dev, 0, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="needs the 3 rendered frames"):
        poses.register_cameras(model, clip[None, :2], start[None], K[None], long_exposure=False)
    with pytest.raises(RuntimeError, match="1 clips, 2 extrinsics"):
        poses.register_cameras(model, clip[None], torch.stack([start, start]), K[None])
    res = poses.register_cameras(model, [torch.cat([clip, clip])], start[None], K[None], steps=1)      # F = 6: two whole loop periods
    assert len(res.costs[0]) == 2
