"""The camera-gradient statement (tests/camera_statement.py) on the reference alone; no GPU.

* the closed form the kernels implement equals the autograd statement in fp64 on all seven scenes;
* the oracle in fp32 stays inside B (it sits at 1 / m of it by construction), and so does the closed form in fp32;
* the unsafe share stays below the cap;
* every planted fault that applies to a scene lands at 4 B or more: B cannot hide a lost pixel, a lost wave, clamped edge taps or a
  missing division by Z;
* poses.se3_exp against torch.matrix_exp, value and gradient, at 0 and away from it;
* the refinement loop (poses.refine_loop) on the oracle meets the condition the GPU test holds the kernels to."""
import pytest
import torch

import camera_statement as CS
import render_statement as RS
from videoloop3d_amd import poses

SCENES = CS.scenes()


def _case(name):
    scene = SCENES[name]
    stack = RS.make_stack(scene)
    obj = CS.objective(scene)
    return scene, stack, obj, CS.statement(scene, stack, obj, key=("cpu", name))


def test_seven_scenes():
    assert sorted(SCENES) == sorted(RS.EXACT_VIEWS + ("perspective", "utils_mpi"))
    assert all((s.H, s.W, s.Hs, s.Ws) == (33, 131, 40, 140) and s.homos.shape[0] == 4 for s in SCENES.values())


@pytest.mark.parametrize("name", sorted(SCENES))
def test_closed_form_equals_autograd_in_fp64(name):
    scene, stack, obj, st = _case(name)
    r = st.ratio(CS.closed_form(scene, stack, obj))
    print(f"[{name}] closed form in fp64 vs autograd: {r:.3e} B (B {st.bound:.3e})")
    assert r <= 1e-6


@pytest.mark.parametrize("name", sorted(SCENES))
def test_fp32_inside_the_bound_and_unsafe_cap(name):
    scene, stack, obj, st = _case(name)
    r32, rc32 = st.ratio(st.g32), st.ratio(CS.closed_form(scene, stack, obj, torch.float32))
    print(f"[{name}] B {st.bound:.3e}: oracle in fp32 {r32:.3f} B, closed form in fp32 {rc32:.3f} B, unsafe {100 * st.unsafe:.2f} %")
    assert st.bound > 0 and r32 <= 1.0 and rc32 <= 1.0
    assert st.unsafe <= CS.UNSAFE_CAP
    assert (st.unsafe == 0) == scene.exact_coverage


@pytest.mark.parametrize("name", sorted(SCENES))
def test_planted_faults_are_seen(name):
    scene, stack, obj, st = _case(name)
    for fault in CS.FAULTS:
        if not CS.fault_applies(scene, fault):
            continue
        r = st.ratio(CS.closed_form(scene, stack, obj, fault=fault))
        print(f"[{name}] {fault}: {r:.1f} B")
        assert r >= 4.0, (name, fault, r)


def test_window_and_no_alpha_statements_are_consistent():
    """the closed form follows the statement under a (row0, col0) window and without g_alpha"""
    scene = SCENES["perspective"]
    stack = RS.make_stack(scene)
    for window, alpha in (((5, 7), True), ((0, 0), False)):
        obj = CS.objective(scene, window=window, alpha=alpha)
        st = CS.statement(scene, stack, obj, window=window)
        assert st.ratio(CS.closed_form(scene, stack, obj, window=window)) <= 1e-6


def test_warp_statement():
    st = CS.warp_statement()
    print(f"[warp] B {st.bound:.3e}, unsafe {100 * st.unsafe:.2f} %")
    assert st.bound > 0 and st.unsafe <= CS.UNSAFE_CAP and float(st.g64.abs().max()) > 0


def _twist_matrix(xi):
    w, v = xi[:3], xi[3:]
    m = torch.zeros((4, 4), dtype=torch.float64)
    m[0, 1], m[0, 2], m[1, 0], m[1, 2], m[2, 0], m[2, 1] = -w[2], w[1], w[2], -w[0], -w[1], w[0]
    m[:3, 3] = v
    return m


@pytest.mark.parametrize("scale", [0.0, 1e-9, 1e-4, 9.9e-3, 1.01e-2, 0.3, 2.5])
def test_se3_exp_against_matrix_exp(scale):
    base = torch.tensor([0.3, -0.5, 0.8, 0.2, -0.7, 0.4], dtype=torch.float64)
    xi = base * torch.tensor([scale] * 3 + [1.0] * 3, dtype=torch.float64) / base[:3].norm()
    got = poses.se3_exp(xi)
    want = torch.matrix_exp(_twist_matrix(xi))
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-14
    probe = torch.arange(16, dtype=torch.float64).reshape(4, 4) / 7 - 1
    f = lambda fn: torch.autograd.functional.jacobian(lambda x: (fn(x) * probe).sum(), xi)      # noqa: E731
    assert float((f(poses.se3_exp) - f(lambda x: torch.matrix_exp(_twist_matrix_diff(x)))).abs().max()) <= 1e-12
    assert poses.se3_exp(torch.zeros(2, 5, 6)).shape == (2, 5, 4, 4)


def _twist_matrix_diff(xi):
    z = torch.zeros((), dtype=xi.dtype)
    rows = [torch.stack([z, -xi[2], xi[1], xi[3]]), torch.stack([xi[2], z, -xi[0], xi[4]]), torch.stack([-xi[1], xi[0], z, xi[5]]),
            torch.zeros(4, dtype=xi.dtype)]
    return torch.stack(rows)


def test_camera_deltas():
    cd = poses.CameraDeltas(3, learn_focal=True)
    base_e = torch.eye(4, dtype=torch.float64).expand(3, 4, 4).clone()
    base_k = torch.tensor([[100.0, 0, 50], [0, 100, 30], [0, 0, 1]], dtype=torch.float64).expand(3, 3, 3).clone()
    assert cd.xi.dtype == torch.float64 and cd.xi.device.type == "cpu" and float(cd.xi.detach().abs().max()) == 0
    assert torch.equal(cd.extrins(base_e, [0, 2]), base_e[[0, 2]]) and torch.equal(cd.intrins(base_k), base_k)
    with torch.no_grad():
        cd.log_focal[1] = 0.1
    k = cd.intrins(base_k, [1])[0].detach()
    assert abs(float(k[0, 0]) - 100 * torch.exp(torch.tensor(0.1, dtype=torch.float64)).item()) < 1e-12 and float(k[0, 2]) == 50 and float(k[2, 2]) == 1


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_refinement_on_the_oracle(dtype):
    """the true camera perturbed by xi = (4, -3, 5, 6, -4, 3) 1e-4 (at most 0.14 px), Adam lr 5e-5, 60 steps, stack frozen: rotation and
    translation error both end below one tenth of their start"""
    g = CS.REFINE
    stack, K_plane, depths, E_true, K, spec = CS.refine_setting()
    render = CS.oracle_render_cameras(stack, K_plane, depths, spec, g["H"], g["W"], dtype)
    with torch.no_grad():
        target = render(E_true[None], K[None])
    start = poses.se3_exp(torch.tensor(g["xi"], dtype=torch.float64)) @ E_true
    r0, t0 = (float(v) for v in poses.pose_error(start, E_true))
    E, _, hist = poses.refine_loop(render, target, start[None], K[None], steps=g["steps"], lr=g["lr"])
    r1, t1 = (float(v) for v in poses.pose_error(E[0], E_true))
    print(f"[{dtype}] rotation {r0:.2e} -> {r1:.2e} ({r1 / r0:.3f}), translation {t0:.2e} -> {t1:.2e} ({t1 / t0:.3f}), loss {hist[0]:.3e} -> {hist[-1]:.3e}")
    assert r1 < 0.1 * r0 and t1 < 0.1 * t0
