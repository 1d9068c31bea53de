"""Conditions on the reference alone for tests/normal_statement.py (no GPU): the unsafe share, the closed form of include/vl3d.h ("Camera
normal equations") against the forward-mode statement, the planted faults, A symmetric positive definite, b the reverse-mode gradient, the
tangents of poses.camera_tangents' chain against a central difference, and the three-step Gauss-Newton run on the oracle in fp32."""
import types

import pytest
import torch

import camera_statement as CS
import normal_statement as NS
import render_statement as RS
from videoloop3d_amd import poses

SCENES = CS.scenes()
TN, P = 2, 7


def _case(name):
    sc = SCENES[name]
    return sc, RS.make_stack(sc, TN), NS.tangents(sc, P), NS.target(sc, TN), NS.weights(sc, TN)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_statement_closed_form_and_faults(name):
    sc, stack, dh, tgt, w = _case(name)
    st = NS.statement(sc, stack, dh, tgt, w, key=("cpu", name))
    assert st.unsafe <= CS.UNSAFE_CAP and float((w == 0).double().mean()) == pytest.approx(st.unsafe)
    r = st.ratio(NS.closed_form(sc, stack, dh, tgt, w))
    print(f"[{name}] B {st.bound:.3e} ({st.m:g} x the oracle in fp32), closed form {r:.2e} B, unsafe {100 * st.unsafe:.3f} %")
    assert r <= 1e-3
    for fault in NS.FAULTS:
        assert NS.fault_applies(sc, w, P, fault), fault
        f = st.ratio(NS.closed_form(sc, stack, dh, tgt, w, fault=fault))
        print(f"[{name}] planted {fault}: {f:.1f} B")
        assert f > 1.0, (name, fault, f)


@pytest.mark.parametrize("name", ["lattice", "perspective", "utils_mpi"])
def test_system_is_spd_and_b_is_the_gradient(name):
    sc, stack, dh, tgt, w = _case(name)
    A, b, cost = NS.statement(sc, stack, dh, tgt, w, key=("cpu", name)).s64
    assert torch.equal(A, A.T) or float((A - A.T).abs().max()) <= 1e-12 * float(A.abs().max())
    ev = torch.linalg.eigvalsh(0.5 * (A + A.T))
    g = NS.gradient(sc, stack, dh, tgt, w)
    err = float((b - g).abs().max() / g.abs().max())
    print(f"[{name}] eigenvalues of A {float(ev.min()):.3e} .. {float(ev.max()):.3e}, cost {float(cost):.3e}, |b - reverse mode| {err:.1e} relative")
    assert float(ev.min()) > 0 and float(cost) > 0 and err <= 1e-12


def test_weight_none_is_weight_one():
    sc, stack, dh, tgt, _ = _case("magnify")
    a = NS.evaluate(sc, stack, dh, tgt, NS.weights(sc, TN, kind="none"))
    b = NS.evaluate(sc, stack, dh, tgt, NS.weights(sc, TN, kind="mask"))
    assert all(torch.allclose(x, y, rtol=1e-14, atol=0) for x, y in zip(a, b))


@pytest.mark.parametrize("learn_focal", [False, True])
def test_camera_tangents_against_a_central_difference(learn_focal):
    """poses.camera_tangents on a stand-in for a PlaneModel (homography_chain = camera_statement.oracle_homographies, the chain the models
    spell) against (H(+h) - H(-h)) / 2h of the float64 chain, h = 1e-6: the truncation is h^2, the rounding 1e-16 / h"""
    stack, K_plane, depths, E, K, spec = CS.refine_setting()
    model = types.SimpleNamespace(homography_chain=lambda e, k: CS.oracle_homographies(K_plane, depths, e[0], k[0]))
    E0 = poses.se3_exp(torch.tensor(CS.REFINE["xi"], dtype=torch.float64)) @ E
    homos, dh = poses.camera_tangents(model, E0, K, learn_focal)
    Pn = 7 if learn_focal else 6
    assert homos.dtype == dh.dtype == torch.float32 and tuple(dh.shape) == (Pn, CS.REFINE["D"], 3, 3)
    assert torch.equal(homos, CS.oracle_homographies(K_plane, depths, E0, K).float())
    h = 1e-6
    for k in range(Pn):
        def at(s):
            th = torch.zeros(Pn, dtype=torch.float64)
            th[k] = s
            Kt = poses._focal_scaled(K, th[6]) if learn_focal else K
            return CS.oracle_homographies(K_plane, depths, poses.se3_exp(th[:6]) @ E0, Kt)
        fd = (at(h) - at(-h)) / (2 * h)
        err = float((dh[k].double() - fd).abs().max() / fd.abs().max())
        print(f"parameter {k}: max |tangent| {float(fd.abs().max()):.3e}, relative difference {err:.1e}")
        assert err <= 2.0 ** -23      # float32 rounding of the tangent; the difference quotient itself is good to 1e-9
    oh, odh = NS.oracle_tangents(K_plane, depths, E0, K, learn_focal)
    assert torch.equal(oh, homos) and torch.equal(odh, dh)


def test_three_gauss_newton_steps_on_the_oracle_in_fp32():
    """the setting of camera_statement.REFINE: after 3 steps at damping 1e-3 rotation and translation error are both below 1e-2 of the start"""
    g = CS.REFINE
    stack, K_plane, depths, E_true, K, spec = CS.refine_setting()
    with torch.no_grad():
        tgt = CS.oracle_render_cameras(stack, K_plane, depths, spec, g["H"], g["W"], torch.float64)(E_true[None], K[None]).float()
    start = poses.se3_exp(torch.tensor(g["xi"], dtype=torch.float64)) @ E_true
    r0, t0 = (float(v) for v in poses.pose_error(start, E_true))
    system = NS.oracle_system(stack, K_plane, depths, spec, g["H"], g["W"], tgt, torch.float32)
    E, Kr, costs, A, cost = poses.gn_loop(system, start, K, steps=3, damping=1e-3)
    r1, t1 = (float(v) for v in poses.pose_error(E, E_true))
    print(f"rotation {r0:.2e} -> {r1:.2e} ({r1 / r0:.2e}), translation {t0:.2e} -> {t1:.2e} ({t1 / t0:.2e}), cost {costs[0]:.3e} -> {cost:.3e} over {costs}")
    assert len(costs) == 4 and cost < costs[0] and torch.equal(Kr, K)
    assert r1 < 1e-2 * r0 and t1 < 1e-2 * t0
