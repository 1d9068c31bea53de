"""Conditions on the fp64 statement of the float training render ALONE (tests/render_statement.py), so that no GPU test of
tests/test_gpu_render_fp64.py can hide behind its own exclusions: the exact-coordinate scenes are exact, unsafe pixels are rare (none on
the exact scenes), every scene reaches all four plane edges and is covered, the pristine fp32 oracle passes the comparison the GPU tests
make, and five faults planted in a copy of the fp32 oracle fail it -- the smallest by 4 bounds or more, which caps the margin m.
Everything is printed: shares, noise per scene and output, and what each fault costs on each scene."""
import pytest
import torch

import render_statement as RS
from oracle import mpi_oracle as MO

STACKS = {"1.0x": (RS.H, RS.W), "1.1x": (37, 145)}


def _all_scenes():
    out = {}
    for size, (Hs, Ws) in STACKS.items():
        for name, sc in RS.views(Hs, Ws).items():
            out[f"{size}/{name}"] = sc
    out.update(RS.quad_scenes())
    out["1.0x/utils_mpi"] = RS.utils_mpi_scene(RS.H, RS.W)
    return out


@pytest.fixture(scope="module")
def scenes():
    return _all_scenes()


@pytest.fixture(scope="module")
def statements(scenes):
    """scene -> (stack, objective, Statement) with the sparsity sums in the objective (the loop-mask label on the dense planar scenes)"""
    out = {}
    for name, sc in scenes.items():
        stack = RS.make_stack(sc)
        dense_planar = sc.keep is None and sc.spec.coord_mode == "affine"
        mask = RS.synth.hash_uniform((RS.D, RS.T, sc.Hs, sc.Ws), seed=6) * 3 - 2 if dense_planar else None
        obj = RS.objective(sc, asum=True, label=dense_planar)
        out[name] = (stack, obj, mask, RS.statement(sc, stack, obj, mask))
    return out


def test_sizes_reach_every_region_shape_and_both_sides_of_fits():
    """33 x 131: three regions across and two down for every owned interior of the backward's region shapes (62 x 14, 62 x 6, 30 x 14, 62 x 10),
    an odd T and an odd H; the 1.0x stack inside rule 4's `fits`, the 1.1x stack outside it"""
    for iw, ih in ((62, 14), (62, 6), (30, 14), (62, 10)):
        assert -(-RS.W // iw) >= 3 and -(-RS.H // ih) >= 2
    assert RS.T % 2 == 1 and RS.H % 2 == 1
    fits = lambda Hs, Ws: Hs * 100 <= RS.H * 107 or Ws * 100 <= RS.W * 107      # noqa: E731
    assert fits(*STACKS["1.0x"]) and not fits(*STACKS["1.1x"])


def test_exact_scenes_are_exact_and_have_no_unsafe_pixel(scenes):
    """the oracle's fp32 coordinates equal its fp64 ones bit for bit on every exact-coordinate view (and on the shared-border quad scene; on
    the tile-exact one the LATTICE coordinate, which decides coverage and the quad); lattice views put samples exactly on texel centres, on
    tx == 0 and tx == Ws - 1, lattice+- taps of weight exactly 2^-10"""
    n_exact = 0
    for name, sc in scenes.items():
        exact = RS.coords_exact(sc)
        print(f"[{name}] fp32 coordinates exact: {exact}; exact_coverage {sc.exact_coverage}, m {sc.m:g}")
        assert exact == sc.exact_coverage, name
        if sc.exact_coverage:
            n_exact += 1
            assert not bool(RS.unsafe_mask(sc).any())
            assert sc.m == (RS.M_COORD if sc.spec.tile[0] else RS.M_EXACT)
            assert torch.equal(sc.homos[:, 2], torch.tensor([0.0, 0.0, 1.0]).expand(RS.D, 3))
        else:
            assert sc.m == RS.M_COORD
        tx, ty = RS.plane_coords(sc.homos, sc.H, sc.W, sc.spec, sc.Hs, sc.Ws)
        view = name.split("/")[-1]
        ex = sc.keep.shape[2] * (sc.spec.tile[1] - 1) if sc.spec.tile[0] else sc.Ws - 1
        if view == "lattice":
            assert bool((tx == tx.round()).all()) and bool((ty == ty.round()).all())
            assert bool((tx == 0).any()) and bool((tx == ex).any()) and bool((ty == 0).any())
        if view in ("lattice+", "lattice-"):
            f = tx - tx.floor()
            assert bool(((f == RS.EPS) | (f == 1 - RS.EPS)).all())
    assert n_exact == 2 * len(RS.EXACT_VIEWS) + 2
    # different integer shifts per plane
    lat = scenes["1.0x/lattice"].homos
    assert len({(float(h[0, 2]), float(h[1, 2])) for h in lat}) == RS.D


def test_unsafe_share_and_conditions(scenes):
    for name, sc in scenes.items():
        c = RS.conditions(sc)
        print(f"[{name}] " + ", ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in c.items()))
        assert c["unsafe"] <= 0.01 and (c["unsafe"] == 0.0 or not sc.exact_coverage), name
        assert c["covered"] >= 0.30, name
        assert c["edge_left"] and c["edge_right"] and c["edge_top"] and c["edge_bottom"], name
        if sc.keep is not None:
            assert c["quad_border"], name
            assert not sc.spec.tile[0] or c["tile_seam"], name
    assert RS.conditions(scenes["1.0x/perspective"])["unsafe"] > 0      # the mask is not vacuous


def test_the_objective_is_zero_at_unsafe_pixels(scenes):
    sc = scenes["1.0x/perspective"]
    obj, bad = RS.objective(sc, asum=True, label=True), RS.unsafe_mask(sc)
    for g in (obj.g_rgb, obj.g_alpha, obj.g_asum, obj.g_label):
        assert float(g[:, bad].abs().max()) == 0.0 and float(g[:, ~bad].abs().max()) > 0.1


def test_the_pristine_fp32_oracle_passes(statements):
    for name, (stack, obj, mask, st) in statements.items():
        noise = {n: st.noise(n) for n in RS.OUTPUTS if getattr(st.r64, n) is not None}
        print(f"[{name}] oracle in fp32 against fp64: " + ", ".join(f"{n} {v:.3e}" for n, v in noise.items()) +
              f"; max |gradient| {float(st.r64.grad.abs().max()):.3f}")
        assert all(0 < v < 1e-4 for v in noise.values()), name
        if st.scene.m == RS.M_EXACT:      # value arithmetic alone: about 1000 times below the suite's flat 1e-4
            assert max(noise.values()) < 5e-7, name
        st.check("oracle fp32", st.r32)
        r = st.ratios(st.r32)
        assert max(r.values()) == pytest.approx(1 / st.scene.m)


def test_the_copy_that_takes_the_faults_is_the_oracle(scenes):
    """render_statement._copy_render without a fault gives MO.render_planes' bits in fp32 and in fp64, forward and gradient"""
    for name in ("1.0x/lattice", "1.0x/lattice-", "1.1x/minify", "1.0x/perspective"):
        sc = scenes[name]
        stack, o = RS.make_stack(sc), RS.BS.oracle_spec(sc.spec)
        for dtype in (torch.float32, torch.float64):
            outs = []
            for fn in (lambda s: MO.render_planes(s, sc.homos.to(dtype), sc.H, sc.W, o, return_layers=True, layer_order="plane"),      # noqa: E731
                       lambda s: RS._copy_render(s, sc.homos.to(dtype), sc.H, sc.W, o)):      # noqa: E731
                s = stack.to(dtype).requires_grad_(True)
                rgb, alpha, bw, layers = fn(s)
                (g,) = torch.autograd.grad((rgb * rgb).sum() + alpha.sum(), s)
                outs.append((rgb, alpha, bw, layers, g))
            assert all(torch.equal(a, b) for a, b in zip(*outs)), (name, dtype)


def _fault_case(sc, fault):
    if fault == "opaque_behind":
        sc = sc.with_spec(rgb_act="none", alpha_act="none")
        return sc, RS.opaque_stack(sc)
    return sc, RS.make_stack(sc)


def test_planted_faults_fail_the_comparison(scenes):
    """the oracle's fp32 evaluation stands in for the kernel; each fault is planted in it alone.  Per fault the largest excess over the
    exact-coordinate views (measured / allowance, 1.0 = the bound) -- the comparison must fail, and the SMALLEST of these maxima is at least 4:
    raising m = 16 by that factor would let a fault through, so 4 x 16 caps m."""
    worst = {}
    for fault in RS.FAULTS:
        per_scene = {}
        for view in RS.EXACT_VIEWS + ("perspective",):
            sc, stack = _fault_case(scenes[f"1.0x/{view}"], fault)
            obj = RS.objective(sc, asum=True)
            st = RS.statement(sc, stack, obj)
            if fault == "opaque_behind":      # the scene has what the fault needs: blended alphas of exactly 1 with planes behind them
                assert float(st.r64.alpha.max()) >= 1.0 - 1e-12 and float(st.r64.asum[..., 0].max()) > 1.0
            per_scene[view] = max(st.ratios(RS.evaluate(sc, stack, obj, torch.float32, fault=fault)).values())
        print(f"[{fault}] measured / allowance per view: " + ", ".join(f"{k} {v:.2f}" for k, v in per_scene.items()))
        worst[fault] = max(v for k, v in per_scene.items() if k != "perspective")
        assert worst[fault] > 1.0, fault
    print("smallest planted fault: " + min(worst, key=worst.get) + f" at {min(worst.values()):.2f} bounds (m = {RS.M_EXACT:g}); it would pass at m = "
          f"{RS.M_EXACT * min(worst.values()):.0f}")
    assert min(worst.values()) >= 4.0, worst
    # what the flat tolerance of the fp32 comparisons (1e-4, gradient 1e-4 max(1, max |g|)) lets through even on this scene: the sigmoid
    sc = scenes["1.0x/lattice+"]
    stack, obj = RS.make_stack(sc), RS.objective(sc)
    st = RS.statement(sc, stack, obj)
    for fault in ("sigmoid_1e-5",):
        got = RS.evaluate(sc, stack, obj, torch.float32, fault=fault)
        flat = max(float((got.rgb.double() - st.r64.rgb).abs().max()), float((got.alpha.double() - st.r64.alpha).abs().max()),
                   float((got.grad.double() - st.r64.grad).abs().max()))
        print(f"[{fault}] on lattice+: max deviation {flat:.3e} -- inside the flat 1e-4")
        assert flat < 1e-4


def test_opaque_plane_gradient_of_the_statement():
    """the finding the GPU value-edge test rests on, on four stacked alphas (0.3, 1.0, 0.4, 0.6) with q = (1, 2, 3, 4): d/da_1 of
    sum_k w_k q_k is T_1 (q_1 - composite behind) = 0.7 (2 - (0.4 * 3 + 0.6 * 0.6 * 4)) -- torch's cumprod backward is exact at the zero"""
    a = torch.tensor([0.3, 1.0, 0.4, 0.6], dtype=torch.float64, requires_grad=True)
    q = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)
    _, bw = MO.overcompose(a[None, None, None], q[None, None, None, :, None])
    (g,) = torch.autograd.grad((bw[0, 0, 0] * q).sum(), a)
    assert float(g[1]) == pytest.approx(0.7 * (2.0 - (0.4 * 3.0 + 0.6 * 0.6 * 4.0)), abs=1e-12)
    assert 0.7 * 2.0 == pytest.approx(1.4)      # what the shortcut `behind = 0` leaves
