"""The baked playback kernels on the MI355X against the fp64 statement of tests/baked_statement.py -- the CPU oracle (oracle/mpi_oracle.py:
render_planes) on decoded texels, sharing no code with the kernels -- on every storage (the dense clip: dense, shared-border culled, tile-exact
culled; the pool in both geometries, with static, dynamic and unstored blocks), every selection (frame run, camera path, loop time) and both
sinks (float; display RGB8 / RGBA8, with and without a background).  The other baked test files compare kernels with kernels; a fault in what
the families share (the tap arithmetic, plane_cull, the plane lists, the blend's tap order, the composite) passes all of them and fails here.

Bound: per scene and output, B = 4 max |oracle in fp32 - oracle in fp64| over the safe pixels -- no floor, no 1e-5 (below the oracle's own fp32
noise on these scenes).  Unsafe pixels (within 1e-3 texel of a plane edge or a quad boundary in fp64: coverage is a step function there) are
compared in neither sink; tests/test_baked_statement_cpu.py holds their share to 1 % and shows that the comparison fails under planted faults.
Display bytes must lie in the interval the statement and the propagated bound give (baked_statement.Statement.byte_interval).  Every test prints B
and the measured maximum (docs/kernels/K9_baked_playback.md, "Parity with the fp64 oracle", records them).

Fixed scenes: those of tests/baked_models.py (D = 4, a clip of 5 frames, planes of 40 x 72 texels, output 37 x 70, three cameras), and for the
display sink also 8 x 128, where the lane-packed RGB8 store's dword branch runs.  Randomized scenes: 12 seeds, all five storages per seed
(baked_models.fp64_random_scene)."""
import copy
import types

import pytest
import torch

import baked_models as BM
import baked_statement as BS

pytestmark = pytest.mark.gpu

SIZES = {"37x70": (BM.H, BM.W), "8x128": (8, 128)}
STORAGES = ["dense", "shared", "exact", "pool_shared", "pool_exact"]


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _on_device(s, dev):
    """a storage of baked_models.fp64_scenes on the device -> the three render calls: run(cam, frame0, n, **sink), path(cams, frames, **sink),
    times(cams, taus, **sink)"""
    from videoloop3d_amd import render as R
    S = s.scene
    homos, qk = S.homos.to(dev), (None if s.keep is None else s.keep.to(torch.uint8).to(dev))
    if s.kind == "pool":
        lay, pool, kw = copy.copy(s.lay).to(dev), s.pool.to(dev), dict(quad_keep=qk, culled_rgba8=BS.CULLED)
        return types.SimpleNamespace(
            run=lambda cam, f0, n, **o: R.render_frame_run_baked_pool(lay, pool, f0, n, homos[cam], S.H, S.W, S.spec, **kw, **o),
            path=lambda cams, ts, **o: R.render_path_baked_pool(lay, pool, cams, ts, homos, S.H, S.W, S.spec, **kw, **o),
            times=lambda cams, taus, **o: R.render_times_baked_pool(lay, pool, cams, taus, homos, S.H, S.W, S.spec, **kw, **o))
    clip = s.clip.to(dev)
    return types.SimpleNamespace(
        run=lambda cam, f0, n, **o: R.render_frame_run_baked(clip, f0, n, homos[cam], S.H, S.W, S.spec, quad_keep=qk, **o),
        path=lambda cams, ts, **o: R.render_path_baked(clip, cams, ts, homos, S.H, S.W, S.spec, quad_keep=qk, **o),
        times=lambda cams, taus, **o: R.render_times_baked(clip, cams, taus, homos, S.H, S.W, S.spec, quad_keep=qk, **o))


@pytest.fixture(scope="module")
def fixed():
    """the fixed scenes on the host, per view size; built once, never modified"""
    return {size: BM.fp64_scenes(*hw) for size, hw in SIZES.items()}


def _frames8(n, S, C, dev):
    return torch.full((n, S.H, S.W, C), 0xAB, dtype=torch.uint8, device=dev)


def _cams_times(sel):
    return [c for c, _ in sel], [t for _, t in sel]


# ---- 1. the float sink: runs, path, times ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STORAGES)
def test_float_sink_against_the_fp64_statement(dev, fixed, name):
    s = fixed["37x70"][name]
    S, k = s.scene, _on_device(s, dev)
    for tag, (f0, n) in BS.RUNS.items():
        rgb, alpha = k.run(0, f0, n)
        S.statement(BS.run_sel(0, f0, n)).check_float(tag, rgb, alpha)
    rgb, alpha = k.path(*_cams_times(BS.PATH))
    st = S.statement(BS.PATH)
    st.check_float("path", rgb, alpha)
    assert 0.3 < float((st.alpha > 0).double().mean()) < 0.97
    rgb, alpha = k.times(*_cams_times(BS.TIMES))
    st = S.statement(BS.TIMES)
    st.check_float("times", rgb, alpha)
    # the times path holds the seam twice (4.25, and the last float32 below T: f just below 1) and a fraction that is inexact in fp32
    assert [BS.loop_time(t, BS.T_FIXED)[:2] for _, t in BS.TIMES[-2:]] == [(4, 0), (4, 0)] and BS.loop_time(BS.TIMES[-1][1], BS.T_FIXED)[2] > 0.9999
    assert BS.f32(2.7) != 2.7


# ---- 2. the display sink ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("name", STORAGES)
def test_display_sink_bytes_lie_in_the_fp64_interval(dev, fixed, name, size):
    """one run of 3 frames and the times path, RGB8 and RGBA8, no background / the quarter-level background / the clamping one: every byte of
    every safe pixel inside the interval"""
    s = fixed[size][name]
    S, k = s.scene, _on_device(s, dev)
    f0, n = BS.RUNS["run of 3"]
    run, times = S.statement(BS.run_sel(0, f0, n)), S.statement(BS.TIMES)
    for C in (3, 4):
        for bg in BS.BGS:
            run.check_bytes(f"{size} run of 3, C = {C}, bg {bg}", k.run(0, f0, n, frames8=_frames8(n, S, C, dev), bg=bg), bg)
            times.check_bytes(f"{size} times, C = {C}, bg {bg}", k.times(*_cams_times(BS.TIMES), frames8=_frames8(len(BS.TIMES), S, C, dev), bg=bg), bg)


# ---- 3. randomized scenes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", BM.RANDOM_SEEDS)
def test_randomized_scenes(dev, seed):
    """a drawn model and view in all five storages: one run and one times path of 5 frames that holds the seam; the float sink within B (per
    scene: the run's and the path's frames together), the RGBA8 bytes over the quarter-level background within the interval.  Every drawn
    shape lies inside the entries' rules, so no call is refused; nothing is caught."""
    storages, run, times = BM.fp64_random_scene(seed)
    for name in STORAGES:
        s = storages[name]
        S, k = s.scene, _on_device(s, dev)
        st = S.statement(run + times)
        (cam, f0), n = run[0], len(run)
        r_run, a_run = k.run(cam, f0, n)
        r_t, a_t = k.times(*_cams_times(times))
        print(f"  D T Hs Ws {S.dims}, {S.H} x {S.W}, quads {tuple(s.keep.shape[1:]) if s.keep is not None else None}, tile {S.spec.tile}, "
              f"covered {float((st.alpha > 0).double().mean()):.3f}")
        st.check_float(f"run of {n} from {f0} + times", torch.cat([r_run, r_t]), torch.cat([a_run, a_t]))
        got = torch.cat([k.run(cam, f0, n, frames8=_frames8(n, S, 4, dev), bg=BS.BG_QUARTER),
                         k.times(*_cams_times(times), frames8=_frames8(len(times), S, 4, dev), bg=BS.BG_QUARTER)])
        st.check_bytes("RGBA8 over the quarter-level background", got, BS.BG_QUARTER)
