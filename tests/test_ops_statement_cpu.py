"""The statement of the unfused drop-ins (tests/ops_statement.py) on the reference alone; no GPU.

* the closed division-free form equals autograd on the reference's cumprod chain in fp64, for overcompose and for overcomposeNto0 (flipped),
  to 1e-12 of each bound's scale on every ray: the statement does not lean on cumprod's own handling of zeros;
* the division-free form in float32 passes every bound on every ray -- the bounds can be met;
* each planted spelling ("divide the total transmittance back out", "difference of the running sums, zero at the singularity") fails on the
  rays named for it and passes the uniform [0, 0.9) ray of 8 planes; the worst error / bound per ray and spelling is printed;
* the warp cases meet their tap-count conditions and the 2 % cap; the oracle in fp32 sits at 1 / m of the warp bound;
* a planted "clamp to the edge texel instead of 0" exceeds the warp bound on the shifted view."""
import pytest
import torch

import ops_statement as OS

RAY_NAMES = sorted(OS.RAYS)
GRADS = ("g_alpha", "g_content")


def _case(name, C=3, with_bw=True):
    return OS.comp_statement(name, OS.P_OVER, C, with_bw)


def test_the_rays():
    assert len(OS.RAYS) == 12
    for name in RAY_NAMES:
        a = OS.ray_rows(name, 258)
        assert a.dtype == torch.float32 and a.shape[0] == 258 and float(a.min()) >= 0 and float(a.max()) <= 1
    assert OS.ray_rows("near_opaque", 1)[0, 2].item() == 1 - 2.0 ** -23 and OS.ray_rows("single_plane", 10).shape == (10, 1)
    assert float(OS.ray_rows("uniform0.9_x8", 258).max()) < 0.9 and float(OS.ray_rows("uniform1_x32", 258).max()) > 0.99
    assert set(OS.ray_rows("single_plane", 258).flatten().tolist()) >= {0.0, 1.0}


@pytest.mark.parametrize("with_bw", [True, False])
@pytest.mark.parametrize("name", RAY_NAMES)
def test_closed_form_equals_autograd_in_fp64(name, with_bw):
    for C in (1, 3, 8):
        case, ref, bnd = _case(name, C, with_bw)
        got = OS.closed_form(case, torch.float64)
        # 1e-12 relative: in units of the bound, which is 2^-23 n times each output's scale
        n = sum(case.dims[1:]) + 4
        worst = {k: OS.ratio(got[k], ref[k], bnd[k]) * OS.EPS * n for k in OS.COMP_OUTPUTS}
        print(f"[{name} C {C} g_bw {with_bw}] closed form vs autograd, relative to each bound's scale: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        assert max(worst.values()) <= 1e-12, (name, C, worst)


@pytest.mark.parametrize("name", RAY_NAMES)
def test_closed_form_equals_autograd_nto0(name):
    """the same through the reference's overcomposeNto0 (cumprod on the flipped stack), with and without blend_content"""
    for C, blend in ((3, False), (1, True), (4, True), (8, True)):
        case = OS.comp_case(name, OS.P_NTO0, C, with_bw=False)
        mpi, bc, g_rgb = OS.nto0_inputs(case, blend=blend)
        ref = OS.reference_nto0(mpi, bc, g_rgb)
        got, bnd = OS.closed_form(case, torch.float64), OS.bounds(case)
        n = sum(case.dims[1:]) + 4
        g_content = ref["g_blend"] if blend else ref["g_mpi"][:, :, :3]
        pairs = dict(rgb=(OS.rgb_to_nto0(got["rgb"]), ref["rgb"], OS.rgb_to_nto0(bnd["rgb"])),
                     trans=(OS.to_nto0(got["trans"]), ref["trans"], OS.to_nto0(bnd["trans"])),
                     g_alpha=(OS.to_nto0(got["g_alpha"]), ref["g_mpi"][:, :, 3], OS.to_nto0(bnd["g_alpha"])),
                     g_content=(OS.to_nto0(got["g_content"]), g_content, OS.to_nto0(bnd["g_content"])))
        worst = {k: OS.ratio(*v) * OS.EPS * n for k, v in pairs.items()}
        print(f"[{name} C {C} blend {blend}] closed form vs autograd on overcomposeNto0: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        assert max(worst.values()) <= 1e-12, (name, C, worst)
        if blend:      # the colour channels of mpi are filler: they take no gradient
            assert float(ref["g_mpi"][:, :, :3].abs().max()) == 0.0


@pytest.mark.parametrize("name", RAY_NAMES)
def test_division_free_fp32_passes_every_bound(name):
    for C in (1, 3, 8):
        for with_bw in (True, False):
            case, ref, bnd = _case(name, C, with_bw)
            got = OS.closed_form(case, torch.float32)
            worst = {k: OS.ratio(got[k], ref[k], bnd[k]) for k in OS.COMP_OUTPUTS}
            worst["trans"] = OS.ratio(got["trans"], OS.closed_form(case, torch.float64)["trans"], bnd["trans"])
            print(f"[{name} C {C} g_bw {with_bw}] division-free in float32, worst |d| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
            assert max(worst.values()) <= 1.0, (name, C, with_bw, worst)


def test_planted_spellings():
    """the two spellings the kernels had: outside the bound on the rays named for each, inside on the easy ray; the forward outputs are shared"""
    table = {}
    for name in RAY_NAMES:
        case, ref, bnd = _case(name, 3, True)
        for sp in OS.SPELLINGS:
            got = OS.closed_form(case, torch.float32, sp)
            table[name, sp] = max(OS.ratio(got[k], ref[k], bnd[k]) for k in GRADS)
            e = float((got["g_alpha"].double() - ref["g_alpha"]).abs().max())
            print(f"[{name}] {sp}: worst |d| / bound {table[name, sp]:.3g}, max abs error of d / d alpha {e:.3g}")
    for name in RAY_NAMES:
        assert table[name, "division_free"] <= 1.0, name
    # the easy ray: 258 draws of uniform [0, 0.9) alphas.  divide_back passes every one.  running_sums passes the typical draw (the first one, and
    # the median) but not all: where the planes in front leave T_k ~ 1e-4, S - P_k keeps the absolute error of S (worst 57 x the bound here)
    case, ref, bnd = _case(OS.EASY_RAY, 3, True)
    per_ray = {sp: ((OS.closed_form(case, torch.float32, sp)["g_alpha"].double() - ref["g_alpha"]).abs() / bnd["g_alpha"]).amax(1) for sp in OS.SPELLINGS}
    for sp, r in per_ray.items():
        print(f"[{OS.EASY_RAY}] {sp}: first ray {float(r[0]):.3f}, median {float(r.median()):.3f}, inside the bound on {100 * float((r <= 1).double().mean()):.1f} % of 258 rays")
    assert table[OS.EASY_RAY, "divide_back"] <= 1.0
    assert float(per_ray["running_sums"][0]) <= 1.0 and float(per_ray["running_sums"].median()) <= 1.0
    for sp, rays in OS.FAULT_RAYS.items():
        for name in rays:
            assert table[name, sp] > 1.0, (sp, name, table[name, sp])


# ---- warp ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OS.WARP_ALL)
def test_warp_conditions(name):
    st = OS.warp_statement(name)
    c, g = OS.warp_conditions(st.case), st.case.dims
    print(f"[{name}] " + ", ".join(f"{k} {v}" for k, v in c.items() if k != "span"))
    assert c["excluded"] <= OS.EXCLUDED_CAP and c["live"] > 0
    assert bool(torch.isfinite(st.out64).all() and torch.isfinite(st.g64).all() and torch.isfinite(st.out32).all() and torch.isfinite(st.g32).all())
    assert float(st.case.gout[st.case.excluded.expand_as(st.case.gout)].abs().sum()) == 0.0
    if name == "cover":
        assert c["all_four"]
    if name == "shifted":
        assert c["two_left"] and c["two_right"] and c["two_top"] and c["two_bottom"] and c["corner_one"]
        assert c["rows_outside"] >= g["B"] * g["D"] and c["cols_outside"] >= g["B"] * g["D"]
        lines = OS.outside_lines(st.case)
        assert float(st.out64[lines.expand_as(st.out64)].abs().max()) == 0.0
        _, gi = OS.warp_evaluate(st.case, gout=lines.expand_as(st.case.gout).float())
        assert float(gi.abs().max()) == 0.0
    if name == "minify":
        assert 2.4 <= c["step"] <= 2.6 and c["busiest_texel"] == 1
        # texels between the footprints: inside the span the frame covers, some texel columns take no gradient at all
        lo, hi = c["span"]
        col = st.g64.abs().sum((2, 3))      # [B,D,Ws]
        assert all(bool((col[n // g["D"], n % g["D"], int(lo[n]):int(hi[n]) + 1] == 0).any()) for n in range(g["B"] * g["D"]))
    if name == "magnify":
        assert 0.3 <= c["step"] <= 0.36 and c["busiest_texel"] >= 9
    if name == "zflip":
        assert c["z_both_signs"] and c["z_min"] > 1e-5 and c["excluded"] > 0
    if name == "1x1":      # exact arithmetic on both sides: the bound is 0 and asks for the exact sum
        assert st.bound("picture") == 0.0 and st.bound("image gradient") == 0.0
        assert torch.equal(st.g64.flatten(), st.case.gout.double().sum().reshape(1))


@pytest.mark.parametrize("name", OS.WARP_ALL)
def test_warp_fp32_inside_the_bound(name):
    st = OS.warp_statement(name)
    for out, got in (("picture", st.out32), ("image gradient", st.g32)):
        r = st.ratio(out, got)
        print(f"[{name}] {out}: B {st.bound(out):.3e}, oracle in fp32 {r:.3f} B")
        assert r <= 1.0


def test_warp_clamp_edge_is_seen():
    st = OS.warp_statement("shifted")
    out, gi = OS.warp_evaluate(st.case, torch.float32, fn=OS.warp_clamp_edge)
    r = st.ratio("picture", out), st.ratio("image gradient", gi)
    print(f"[shifted] clamp to the edge texel: picture {r[0]:.1f} B, image gradient {r[1]:.1f} B")
    assert r[0] > 1.0 and r[1] > 1.0
    # where no tap leaves the texture the copy is the oracle, bit for bit
    cover = OS.warp_statement("cover")
    assert torch.equal(OS.warp_evaluate(cover.case, torch.float64, fn=OS.warp_clamp_edge)[0], cover.out64)
