"""Conditions on the loop-time depth statement of tests/rgbd_statement.py, on the reference alone; no GPU.  What makes it a test for
tests/test_gpu_rgbd.py: at f == 0 it is disparity_statement's frame t0; few unsafe pixels; a covered share strictly between none and all;
normalised rows under which the clamps of the 16-bit depth bite; a seam time in the selection; and the comparison fails, by a wide margin,
under each planted fault."""
import pytest
import torch

import baked_statement as BS
import disparity_models as DM
import disparity_statement as DS
import rgbd_statement as RS

STORAGES = ["dense", "shared", "exact", "pool_shared", "pool_exact"]
UNSAFE_CAP = 0.01
_CACHE = {}


def _scenes():
    if "scenes" not in _CACHE:
        _CACHE["scenes"] = DM.baked_scenes()
    return _CACHE["scenes"]


def _statement(name):
    if name not in _CACHE:
        s = _scenes()[name]
        _CACHE[name] = RS.statement(s.scene, s.rows, BS.TIMES)
    return _CACHE[name]


def test_the_selection_holds_integer_times_fractions_and_the_seam():
    parts = [BS.loop_time(t, DM.T) for _, t in BS.TIMES]
    assert any(f == 0.0 for _, _, f in parts) and any(0.0 < f < 1.0 for _, _, f in parts)
    assert any(t1 == 0 and t0 == DM.T - 1 and f > 0.0 for t0, t1, f in parts)      # a seam time: t1 wraps to frame 0


@pytest.mark.parametrize("name", STORAGES)
def test_an_integer_time_is_the_disparity_statement_of_that_frame(name):
    s = _scenes()[name]
    whole = [(c, t) for c, t in BS.TIMES if BS.loop_time(t, DM.T)[2] == 0.0]
    assert len(whole) >= 2
    got = RS.statement(s.scene, s.rows, whole)
    want = DS.scene_statement(s.scene, s.rows, [(c, BS.loop_time(t, DM.T)[0]) for c, t in whole])
    assert torch.equal(got.disp, want.disp) and torch.equal(got.alpha, want.alpha)


@pytest.mark.parametrize("name", STORAGES)
def test_conditions_on_the_scene(name):
    st = _statement(name)
    b_d, b_a = st.bound
    covered = float((st.alpha > 0).double().mean())
    print(f"[{name}] unsafe {100 * st.unsafe_share:.3f} %, covered {100 * covered:.1f} %, B disp {b_d:.3e} alpha {b_a:.3e}, "
          f"max disp {float(st.disp.max()):.3f}")
    assert st.unsafe_share <= UNSAFE_CAP
    assert 0.3 < covered < 1.0
    assert 0.0 < b_d < 1e-3 and float(st.disp.max()) > 0.05      # a bound far below the signal


@pytest.mark.parametrize("name", STORAGES)
def test_both_clamps_of_the_depth_levels_bite_under_rows_over_2_50(name):
    s = _scenes()[name]
    rows = DM.camera_rows(DM.D, DM.H, DM.W, normalise=(2.0, 50.0))
    st = RS.statement(s.scene, rows, BS.TIMES)
    below, above = int(((st.disp < 0) & st.safe).sum()), int(((st.disp > 1) & st.safe).sum())
    print(f"[{name}] rows over (2, 50): disp {float(st.disp.min()):.3f} .. {float(st.disp.max()):.3f}; {below} pixels below 0, {above} above 1")
    assert below > 0 and above > 0
    lv = RS.depth_levels(st.disp32)
    assert int((lv == 0).sum()) >= below and int((lv == 65535).sum()) >= above and 0 < int(((lv > 0) & (lv < 65535)).sum())
    # (1, 100): the lower clamp alone
    st1 = RS.statement(s.scene, DM.camera_rows(DM.D, DM.H, DM.W, normalise=(1.0, 100.0)), BS.TIMES)
    assert float(st1.disp.min()) < 0.0 and float(st1.disp.max()) < 1.0


@pytest.mark.parametrize("fault", RS.FAULTS)
@pytest.mark.parametrize("name", STORAGES)
def test_a_planted_fault_exceeds_the_bound(name, fault):
    s, st = _scenes()[name], _statement(name)
    bad = RS.statement(s.scene, s.rows, BS.TIMES, fault=fault)
    e_d, _ = st.errors(bad.disp, bad.alpha)
    print(f"[{name} | {fault}] max |d disp| {e_d:.3e} against B {st.bound[0]:.3e}: {e_d / st.bound[0]:.0f} x")
    assert e_d >= 4 * st.bound[0]
    if fault == "seam_to_t0":      # only the seam frames move
        seam = [i for i, (_, t) in enumerate(BS.TIMES) if BS.loop_time(t, DM.T)[1] == 0]
        rest = [i for i in range(len(BS.TIMES)) if i not in seam]
        assert torch.equal(bad.disp[rest], st.disp[rest]) and not torch.equal(bad.disp[seam], st.disp[seam])


def test_the_level_tolerance_takes_the_fp32_statement_and_refuses_a_shift():
    s, st = _scenes()["shared"], None
    rows = DM.camera_rows(DM.D, DM.H, DM.W, normalise=(1.0, 100.0))
    st = RS.statement(s.scene, rows, BS.TIMES)
    lv = RS.depth_levels(st.disp32)
    bad, worst, tol = RS.levels_outside(st, lv)
    print(f"levels of the fp32 statement: worst distance {worst:.2f} of tolerance {tol:.2f}")
    assert bad == 0
    moved = torch.where(lv > 0, lv + int(tol) + 2, lv)
    assert RS.levels_outside(st, moved)[0] > 0
