"""Conditions on the reference alone for tests/register_statement.py (no GPU): the unsafe share, the planted faults, b the reverse-mode
gradient in all Q unknowns, the long exposure of one frame against the per-frame mode, its invariance under a roll of the model's frames, and
the Levenberg-Marquardt runs on the oracle in fp64 -- a brightness offset and a clip started at another loop time, each of which today's system
(normal_statement.oracle_system under poses.gn_loop) turns into a WORSE camera and poses.register_loop on the registration system recovers."""
import math

import pytest
import torch

import camera_statement as CS
import normal_statement as NS
import register_statement as REG
import render_statement as RS
from videoloop3d_amd import poses

SCENES = CS.scenes()
TN, P = 3, 6
MODES = [(False, False), (False, True), (True, False), (True, True)]      # (long exposure, brightness unknowns)


def _case(name, Tn=TN):
    sc = SCENES[name]
    return sc, RS.make_stack(sc, Tn), NS.tangents(sc, P)


@pytest.mark.parametrize("name", ["lattice", "perspective", "utils_mpi"])
def test_statement_rejects_the_planted_faults(name):
    sc, stack, dh = _case(name)
    for long_exposure, photo in MODES:
        tgt, w = REG.target(sc, TN, long_exposure), REG.weights(sc, TN, long_exposure)
        st = REG.statement(sc, stack, dh, tgt, w, long_exposure, photo, REG.POINT, key=("cpu", name))
        Q = P + 2 * photo
        assert st.unsafe <= CS.UNSAFE_CAP and tuple(st.s64[0].shape) == (Q, Q) and tuple(st.s64[1].shape) == (Q,)
        assert st.ratio(st.s64) == 0.0 and 0 < st.ratio(st.s32) <= 1.0
        for fault in REG.FAULTS:
            if not REG.fault_applies(TN, long_exposure, photo, REG.POINT, fault):
                continue
            f = st.ratio(REG.evaluate(sc, stack, dh, tgt, w, long_exposure, photo, REG.POINT, fault=fault, jc=REG._JC[("cpu", name)][torch.float64]))
            print(f"[{name} | long exposure {long_exposure}, brightness {photo}] B {st.bound:.3e}, planted {fault}: {f:.1f} B")
            assert f > 1.0, (name, long_exposure, photo, fault, f)


@pytest.mark.parametrize("long_exposure", [False, True])
@pytest.mark.parametrize("name", ["perspective", "utils_mpi"])
def test_b_is_the_gradient_in_all_unknowns(name, long_exposure):
    sc, stack, dh = _case(name)
    tgt, w = REG.target(sc, TN, long_exposure), REG.weights(sc, TN, long_exposure)
    A, b, cost = REG.statement(sc, stack, dh, tgt, w, long_exposure, True, REG.POINT, key=("cpu", name)).s64
    g = REG.gradient(sc, stack, dh, tgt, w, long_exposure, REG.POINT)
    err = float((b - g).abs().max() / g.abs().max())
    ev = torch.linalg.eigvalsh(0.5 * (A + A.T))
    print(f"[{name} | long exposure {long_exposure}] |b - reverse mode| {err:.1e} relative, eigenvalues of A {float(ev.min()):.3e} .. {float(ev.max()):.3e}")
    assert len(g) == P + 2 and err <= 1e-12 and float(ev.min()) > 0 and float(cost) > 0
    assert float((A - A.T).abs().max()) <= 1e-12 * float(A.abs().max())


@pytest.mark.parametrize("photo", [False, True])
def test_long_exposure_of_one_frame_is_the_per_frame_mode(photo):
    sc, stack, dh = _case("perspective", 1)
    tgt, w = REG.target(sc, 1, False), REG.weights(sc, 1, False)
    jc = NS.jacobian(sc, stack, dh)
    a = REG.evaluate(sc, stack, dh, tgt, w, False, photo, REG.POINT, jc=jc)
    b = REG.evaluate(sc, stack, dh, tgt[0], w[0], True, photo, REG.POINT, jc=jc)
    assert all(torch.allclose(x, y, rtol=1e-14, atol=0) for x, y in zip(a, b))


def test_long_exposure_does_not_see_the_loop_time():
    """torch.roll of the model's frames: the long-exposure system is the same up to fp64 rounding; the per-frame system is not"""
    sc, stack, dh = _case("perspective")
    tgt, w = REG.target(sc, TN, True), REG.weights(sc, TN, True)
    a = REG.evaluate(sc, stack, dh, tgt, w, True, True, REG.POINT)
    b = REG.evaluate(sc, torch.roll(stack, 1, 1), dh, tgt, w, True, True, REG.POINT)
    err = max(float((x - y).abs().max() / x.abs().max()) for x, y in zip(a, b))
    tf, wf = REG.target(sc, TN, False), REG.weights(sc, TN, False)
    c = REG.evaluate(sc, stack, dh, tf, wf, False, True, REG.POINT)
    d = REG.evaluate(sc, torch.roll(stack, 1, 1), dh, tf, wf, False, True, REG.POINT)
    per_frame = float((c[1] - d[1]).abs().max() / c[1].abs().max())
    print(f"rolled frames: long exposure differs by {err:.1e} relative, per frame b by {per_frame:.1e}")
    assert err <= 1e-12 and per_frame > 1e-3


# ---- the Levenberg-Marquardt runs, float64 ----------------------------------------------------------------------------------------------
def _runs(Tn, roll, gain, bias, long_exposure, photo, steps):
    """-> (today's errors / start, the registration's errors / start, fitted (a, beta))"""
    g = CS.REFINE
    stack, K_plane, depths, E_true, K, spec = REG.refine_video_setting(Tn)
    with torch.no_grad():
        frames = CS.oracle_render_cameras(stack, K_plane, depths, spec, g["H"], g["W"], torch.float64)(E_true[None], K[None])
    clip = REG.captured_clip(frames, roll, gain, bias)
    start = poses.se3_exp(torch.tensor(g["xi"], dtype=torch.float64)) @ E_true
    r0, t0 = (float(v) for v in poses.pose_error(start, E_true))
    today = NS.oracle_system(stack, K_plane, depths, spec, g["H"], g["W"], clip, torch.float64)
    E, _, costs, _, _ = poses.gn_loop(today, start, K, steps=steps, damping=1e-3)
    r1, t1 = (float(v) for v in poses.pose_error(E, E_true))
    system = REG.oracle_system(stack, K_plane, depths, spec, g["H"], g["W"], clip.mean(0) if long_exposure else clip, torch.float64, long_exposure, photo)
    E, Kr, a, beta, costs, A, cost = poses.register_loop(system, start, K, steps=steps, damping=1e-3, fit_brightness=photo)
    r2, t2 = (float(v) for v in poses.pose_error(E, E_true))
    print(f"T = {Tn}, roll {roll}, x {gain} + {bias}: today's system rotation {r1 / r0:.2e} translation {t1 / t0:.2e} of the start; "
          f"registration (long exposure {long_exposure}, brightness {photo}, {steps} steps) {r2 / r0:.2e} / {t2 / t0:.2e}, a {a:.7f} beta {beta:.7f}")
    assert torch.equal(Kr, K) and cost < costs[0] and len(costs) == steps + 1
    return (r1 / r0, t1 / t0), (r2 / r0, t2 / t0), (a, beta)


def test_brightness_fit_recovers_the_camera_where_todays_system_loses_it():
    today, reg, (a, beta) = _runs(1, 0, REG.GAIN, REG.BIAS, False, True, 6)
    assert today[0] > 1 and today[1] > 1
    assert reg[0] < 1e-2 and reg[1] < 1e-2
    assert abs(a - math.log(REG.GAIN)) <= 1e-6 and abs(beta - REG.BIAS) <= 1e-6


def test_long_exposure_recovers_the_camera_of_a_clip_started_at_another_time():
    today, reg, _ = _runs(3, 1, 1.0, 0.0, True, False, 5)
    assert today[0] > 1 and today[1] > 1
    assert reg[0] < 1e-2 and reg[1] < 1e-2


def test_long_exposure_with_brightness_fit():
    """both at once (today's system on this clip: rotation above the start, translation half of it -- printed, not a condition)"""
    today, reg, (a, beta) = _runs(3, 1, REG.GAIN, REG.BIAS, True, True, 6)
    assert reg[0] < 1e-2 and reg[1] < 1e-2
    assert abs(a - math.log(REG.GAIN)) <= 1e-6 and abs(beta - REG.BIAS) <= 1e-6
