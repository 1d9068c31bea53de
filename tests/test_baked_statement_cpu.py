"""Conditions on the fp64 statement of the baked playback model ALONE (tests/baked_statement.py, the scenes of tests/baked_models.py), so that no
GPU test of tests/test_gpu_baked_fp64.py can hide behind its own exclusions: the statement equals a second, independently written one; the
pool's restatement holds the source clip's texels; unsafe pixels are rare; the scenes reach the edges, borders and seams they are meant to
test; the byte interval admits the oracle's own fp32 output; and the comparison the GPU tests make fails under five planted faults, with the
oracle's fp32 evaluation standing in for the kernel.  Everything is printed: the unsafe shares and the fp32-vs-fp64 noise per scene."""
import dataclasses

import pytest
import torch

import baked_models as BM
import baked_statement as BS

SIZES = {"37x70": (BM.H, BM.W), "8x128": (8, 128)}
STORAGES = ["dense", "shared", "exact", "pool_shared", "pool_exact"]


@pytest.fixture(scope="module")
def fixed():
    return {size: BM.fp64_scenes(*hw) for size, hw in SIZES.items()}


@pytest.fixture(scope="module")
def drawn():
    return {seed: BM.fp64_random_scene(seed) for seed in BM.RANDOM_SEEDS}


def _selections():
    return dict({k: BS.run_sel(0, *v) for k, v in BS.RUNS.items()}, path=BS.PATH, times=BS.TIMES)


# ---- 1. a second statement ---------------------------------------------------------------------------------------------------------------------
def test_the_oracle_equals_the_plain_fp64_statement_of_the_baked_tests(fixed):
    """tests/test_gpu_baked.py: _fp64_render is written without the oracle (its own coordinates, taps, hard cut and composite); on the dense
    scene the two agree to 1e-12 on that statement's interior pixels, for all three cameras (the descriptor's floats widened from fp32 in both)"""
    from test_gpu_baked import F0, NF, _fp64_render
    S = fixed["37x70"]["dense"].scene
    spec = dataclasses.replace(S.spec, scale=tuple(BS.f32(v) for v in S.spec.scale), offset=tuple(BS.f32(v) for v in S.spec.offset))
    for cam in range(3):
        rgb, alpha, inside = _fp64_render(S.clip, S.homos[cam], spec, list(range(F0, F0 + NF)))
        st = S.statement(BS.run_sel(cam, F0, NF))
        sel = inside[None].expand(NF, BM.H, BM.W)
        e_rgb, e_a = float((st.rgb - rgb)[sel].abs().max()), float((st.alpha - alpha)[sel].abs().max())
        print(f"camera {cam}: oracle in fp64 against _fp64_render on {int(inside.sum())} interior pixels: max |d rgb| {e_rgb:.3e}, |d alpha| {e_a:.3e}")
        assert int(inside.sum()) > BM.H * BM.W // 4 and e_rgb <= 1e-12 and e_a <= 1e-12


# ---- 2. the pool's restatement -------------------------------------------------------------------------------------------------------------------
def _check_restatement(s):
    from videoloop3d_amd import tiles
    S = s.scene
    D, T, Hs, Ws = S.dims
    reach = tiles.quad_to_texel_mask(s.keep, Hs, Ws, s.tile)                   # every texel a kept quad can tap
    stored = BS.stored_texels(s.lay.blocks, Hs, Ws)
    assert bool((stored | ~reach).all())                                       # ... has storage
    sel = reach[:, None, :, :, None].expand_as(S.clip)
    assert torch.equal(S.clip[sel], s.source[sel])
    fill = torch.tensor(BS.rgba8_bytes(BS.CULLED), dtype=torch.uint8)
    assert bool((S.clip[~stored[:, None].expand(D, T, Hs, Ws)] == fill).all())
    return int(reach.sum()), int((~stored).sum())


@pytest.mark.parametrize("geom", list(BM.GEOMS))
def test_the_pool_restatement_holds_the_source_clip(fixed, drawn, geom):
    s = fixed["37x70"]["pool_" + geom]
    n_reach, n_unstored = _check_restatement(s)
    assert n_reach > 0 and n_unstored > 0 and float((s.source[:, 1:] != s.source[:, :1]).float().mean()) > 0.05      # unstored and moving texels exist
    # random filler where nothing is stored: the source clip is not the culled colour there
    stored = BS.stored_texels(s.lay.blocks, *s.scene.dims[2:])
    assert not torch.equal(s.source[~stored[:, None].expand(*s.scene.dims)], s.scene.clip[~stored[:, None].expand(*s.scene.dims)])
    for seed, (storages, _, _) in drawn.items():
        _check_restatement(storages["pool_" + geom])


# ---- 3. unsafe pixels are rare -------------------------------------------------------------------------------------------------------------------
def test_unsafe_share(fixed, drawn):
    for size, storages in fixed.items():
        for name in STORAGES:
            shares = [float(storages[name].scene.unsafe(cam).double().mean()) for cam in range(3)]
            print(f"[{size} {name}] unsafe pixels per camera: " + ", ".join(f"{100 * v:.3f} %" for v in shares))
            assert max(shares) <= 0.01
    for seed, (storages, _, _) in drawn.items():
        for name in STORAGES:
            S = storages[name].scene
            shares = [float(S.unsafe(cam).double().mean()) for cam in range(2)]
            print(f"[seed {seed} {name}] {S.H} x {S.W}: unsafe pixels per camera: " + ", ".join(f"{100 * v:.3f} %" for v in shares))
            assert max(shares) <= (0.0 if S.H * S.W < 1000 else 0.01)
    sizes = [(st["dense"].scene.H, st["dense"].scene.W) for st, _, _ in drawn.values()]
    assert any(h * w < 1000 for h, w in sizes) and any(w == 128 for _, w in sizes) and any(w > 64 and w != 128 for _, w in sizes)


# ---- 4. the scenes are not trivial -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STORAGES)
def test_fixed_scenes_reach_what_they_test(fixed, name):
    """a fixed scene is a storage under its three cameras.  37 x 70: 30-97 % of its pixels covered, a covered pixel within one texel of the hard
    cut on each of the four sides, safe samples at a kept / culled quad border, at a tile seam (tile-exact) and at a block seam in x and in y
    (pool).  8 x 128, the view of the display store's dword branch, shows 8.8 texel rows of the planes' 40: no bottom edge and too few rows
    for a seam in y; coverage, the other three edges, the quad border and the block seam in x hold there too."""
    for size in SIZES:
        S = fixed[size][name].scene
        c = [S.conditions(cam) for cam in range(3)]
        any_ = lambda k: any(ci[k] for ci in c)      # noqa: E731
        covered = sum(ci["covered"] for ci in c) / 3
        print(f"[{size} {name}] covered {covered:.3f} (" + ", ".join(f"{ci['covered']:.3f}" for ci in c) + "); " +
              ", ".join(f"{k} {any_(k)}" for k in c[0] if k not in ("covered", "unsafe")))
        assert 0.30 <= covered <= 0.97
        assert any_("edge_left") and any_("edge_right") and any_("edge_top")
        if name != "dense":
            assert any_("quad_border")
        if S.pool:
            assert any_("block_seam_x")
        if size == "37x70":
            assert any_("edge_bottom")
            assert not S.spec.tile[0] or any_("tile_seam")
            assert not S.pool or any_("block_seam_y")
    # ragged last blocks: the tile-exact pool's planes are 30 x 70 texels
    assert name != "pool_exact" or (fixed["37x70"][name].scene.dims[2] % 8 and fixed["37x70"][name].scene.dims[3] % 8)


# ---- 5. the noise floor, and the byte interval admits the oracle's own fp32 output ------------------------------------------------------------------
@pytest.mark.parametrize("name", STORAGES)
def test_noise_and_byte_interval_self_check(fixed, name):
    for size in SIZES:
        S = fixed[size][name].scene
        for tag, sel in _selections().items():
            st = S.statement(sel)
            n = st.noise
            print(f"[{size} {name} | {tag}] oracle in fp32 against fp64: rgb {n[0]:.3e} alpha {n[1]:.3e} -> B rgb {st.bound[0]:.3e} alpha {st.bound[1]:.3e}; "
                  f"unsafe {100 * st.unsafe_share:.3f} %")
            assert 0 < n[0] < 1e-4 and 0 < n[1] < 1e-4
            assert st.errors(st.rgb32, st.alpha32) == n                       # the stand-in passes the float comparison by construction ...
            if tag in ("run of 3", "times"):
                for C in (3, 4):
                    for bg in BS.BGS:
                        bad, two = st.bytes_outside(BS.display_bytes(st.rgb32, st.alpha32, C, bg), bg)
                        assert bad == 0, (size, name, tag, C, bg, bad)      # ... and the byte comparison
    # the backgrounds: uncovered pixels are decided, and both clamps bite under the last one
    assert all(min(255 * v % 1, 1 - 255 * v % 1) >= 0.25 for v in BS.BG_QUARTER)
    st = fixed["37x70"][name].scene.statement(BS.run_sel(0, 1, 3))
    x = st.rgb * st.alpha[..., None] + torch.tensor(BS.BG_CLAMPS, dtype=torch.float64) * (1 - st.alpha[..., None])
    assert bool((x > 1).any()) and bool((x < 0).any())


def test_noise_of_the_drawn_scenes(drawn):
    for seed, (storages, run, times) in drawn.items():
        for name in STORAGES:
            S = storages[name].scene
            for tag, sel in (("run", run), ("times", times)):
                st = S.statement(sel)
                print(f"[seed {seed} {name} | {tag}] D T Hs Ws {S.dims}, {S.H} x {S.W}: noise rgb {st.noise[0]:.3e} alpha {st.noise[1]:.3e}, "
                      f"covered {float((st.alpha > 0).double().mean()):.3f}, unsafe {100 * st.unsafe_share:.3f} %")
                assert st.noise[0] < 1e-4 and st.noise[1] < 1e-4
        assert any(t0 + 1 == S.dims[1] for t0, _, _ in (BS.loop_time(tau, S.dims[1]) for _, tau in times))      # the times path holds the seam


# ---- 6. the tests bite -------------------------------------------------------------------------------------------------------------------------------
def _fails(st, rgb, alpha):
    e, b = st.errors(rgb, alpha), st.bound
    return e[0] > b[0] or e[1] > b[1], e


@pytest.mark.parametrize("name", STORAGES)
def test_planted_faults_fail_the_comparison(fixed, name):
    """the oracle's fp32 evaluation stands in for the kernel; each fault is planted in it alone and the comparison of the GPU tests
    (Statement.errors against Statement.bound; Statement.bytes_outside) must fail on the fixed scene"""
    s = fixed["37x70"][name]
    S = s.scene
    D, T, Hs, Ws = S.dims
    run, times = S.statement(BS.run_sel(0, 1, 3)), S.statement(BS.TIMES)
    # (a) decode with / 256
    bad, e = _fails(run, *S.fp32(BS.run_sel(0, 1, 3), decode=256.0))
    print(f"[{name}] decode / 256: {e[0]:.3e} {e[1]:.3e} against B {run.bound[0]:.3e} {run.bound[1]:.3e}")
    assert bad
    # (b) one plane's taps shifted by one texel
    plane = 1 if name != "dense" else 2
    moved = S.clip.clone()
    moved[plane] = torch.roll(S.clip[plane], 1, dims=2)
    bad, e = _fails(run, *dataclasses.replace(S, clip=moved).fp32(BS.run_sel(0, 1, 3)))
    print(f"[{name}] plane {plane} shifted by one texel: {e[0]:.3e} {e[1]:.3e}")
    assert bad
    # (c) t1 = T - 1 at the seam in place of 0
    bad, e = _fails(times, *S.fp32(BS.TIMES, seam=T - 1))
    print(f"[{name}] t1 = T - 1 at the seam: {e[0]:.3e} {e[1]:.3e} against B {times.bound[0]:.3e} {times.bound[1]:.3e}")
    assert bad
    # (d) display bytes rounded in place of truncated
    for bg in BS.BGS:
        bad_bytes, _ = run.bytes_outside(BS.display_bytes(run.rgb32, run.alpha32, 4, bg, rounding=True), bg)
        print(f"[{name}] rounded display bytes, bg {bg}: {bad_bytes} outside the interval")
        assert bad_bytes > 0
    if not S.pool:
        return
    # (e) the block table.  An UNSTORED block treated as stored cannot show, and neither can culled_rgba8: a block is unstored exactly when no
    # kept quad can tap a texel of it, and a sample in a culled quad is not covered -- stated here as a fact about the model (every unstored
    # entry in turn pointed at slot 0, and the culled colour set to white: no safe pixel moves).  What the fetch CAN get wrong and a picture
    # shows: a stored block read as unstored, a dynamic block read without + t, a static block read with + t.
    path = S.statement(BS.PATH)
    table = s.lay.blocks.cpu().long()
    restate = lambda tab, culled=BS.CULLED, pool=s.pool: dataclasses.replace(S, clip=BS.pool_as_clip(tab, pool, T, Hs, Ws, culled)).fp32(BS.PATH)      # noqa: E731
    for idx in (table < 0).nonzero().tolist():
        tab = table.clone()
        tab[tuple(idx)] = 0
        assert path.errors(*restate(tab)) == path.noise, idx
    assert path.errors(*restate(table, 0xFFFFFFFF)) == path.noise
    faults = {"every stored block of a plane read as unstored": table.clone(), "dynamic blocks read without + t": table.clone(),
              "static blocks read with + t": table.clone()}
    d_kept = int((table >= 0).flatten(1).any(1).nonzero()[0])
    faults["every stored block of a plane read as unstored"][d_kept] = -1
    t = faults["dynamic blocks read without + t"]
    t[(t >= 0) & (t & 1 == 1)] &= ~1
    t = faults["static blocks read with + t"]
    t[(t >= 0) & (t & 1 == 0)] |= 1
    grown = torch.cat([s.pool, s.pool[:T * 64]])      # (a static block's slot + t may pass the pool's end)
    for what, tab in faults.items():
        bad, e = _fails(path, *restate(tab, pool=grown))
        print(f"[{name}] {what}: {e[0]:.3e} {e[1]:.3e} against B {path.bound[0]:.3e} {path.bound[1]:.3e}")
        assert bad, what
    # one single stored block read as unstored: every block a safe covered sample taps
    hit = 0
    for idx in (table >= 0).nonzero().tolist()[::7]:
        tab = table.clone()
        tab[tuple(idx)] = -1
        hit += _fails(path, *restate(tab))[0]
    print(f"[{name}] single stored blocks read as unstored (every 7th): {hit} of {len((table >= 0).nonzero().tolist()[::7])} fail the comparison")
    assert hit > 0
