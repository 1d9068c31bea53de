"""tests/loss_statement.py without a device: the statement is the reference's (the oracle's own fold bit for bit, goldens G7 and G9, MPV.py:484-507
re-executed literally), the conditions every case table of tests/test_gpu_loss_fp64.py rests on (checked on the reference and the chooser alone), and
planted faults: each is applied to the fp32 oracle's output and has to land at 4 bounds or more -- the cap on the bound's factor."""
import numpy as np
import pytest
import torch

import loss_statement as LS
from oracle import vid_oracle as VO
from videoloop3d_amd import synth

T_ = lambda a: torch.from_numpy(np.asarray(a))      # noqa: E731
ALL_CASES = [c for name in LS.CONFIGS for c in LS.cases(name)]


@pytest.fixture(scope="module")
def UV():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import utils_vid
    return utils_vid


# ---- the statement is the reference's ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ps,pt,s,st,alpha", [((12, 20, 31, 39), 11, 3, 4, 1, 0.5), ((9, 14, 21, 25), 3, 3, 2, 1, 1e10), ((8, 5, 16, 20), 4, 2, 4, 2, 0.01)])
def test_fold_is_the_oracles_fold_bit_for_bit(shape, ps, pt, s, st, alpha):
    Tx, Ty, H, W = shape
    x, y = synth.make_video(Tx, H, W, seed=3), synth.make_video(Ty, H, W, seed=4)
    so, wo, nn = VO.find_nn_and_merge(x, y, ps, pt, s, st, alpha, return_nn=True)
    sm, w, y2x = LS.fold(y[0], nn, ps, pt, s, st, Tx, torch.float32)
    assert sm.dtype == torch.float32 and torch.equal(sm, so[0]) and torch.equal(w, wo[0, 0]) and torch.equal(y2x, (so / wo)[0])
    assert len(nn.unique()) > 1


@pytest.mark.parametrize("ps,pt,s,st,al", [(5, 3, 2, 1, 1e10), (3, 3, 2, 1, 1e10), (5, 3, 2, 1, 0.5), (3, 2, 1, 2, 0.05)])
def test_fold_reproduces_g7(golden, ps, pt, s, st, al):
    g = golden("g7_merge.npz")
    key = f"ps{ps}_pt{pt}_s{s}_st{st}_a{al:g}"
    x, y = T_(g["x"]), T_(g["y"])
    nn = VO.find_nn_and_merge(x, y, ps, pt, s, st, al, return_nn=True)[2]
    sm, w, _ = LS.fold(y[0], nn, ps, pt, s, st, x.shape[2], torch.float32)
    assert float((w.double() - T_(g[key + "_weight"])[0, 0].double()).abs().max()) == 0
    assert float((sm.double() - T_(g[key + "_sum"])[0].double()).abs().max()) <= 1e-6


def test_loss_reproduces_g9(golden):
    g = golden("g9_robust.npz")
    x = T_(g["x"])
    for rou, sc in LS.RHOS:
        for dtype in (torch.float32, torch.float64):
            rho, mean, grad, e = LS.loss(x, torch.zeros_like(x), rou, sc, dtype)
            ref, refg = T_(g[f"rou{rou}_s{sc}"]).double(), T_(g[f"rou{rou}_s{sc}_grad"]).double()
            assert float((rho.double() - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max()))
            assert float((grad.double() * x.numel() - refg).abs().max()) <= 1e-5 * max(1.0, float(refg.abs().max()))
            assert abs(float(mean) - float(ref.mean())) <= 1e-6 * max(1.0, float(ref.abs().max()))
        if rou in ("-2", "1"):      # the closed form the exponent fault is planted in is the derivative
            e64 = x.double()
            g64 = LS.loss(x, torch.zeros_like(x), rou, sc, torch.float64)[2] * x.numel()
            assert float((LS.rho_grad_general(e64, rou, float(np.float32(sc))) - g64).abs().max()) <= 1e-12 * float(g64.abs().max())


@pytest.mark.parametrize("T,pad,h,w", [(5, 2, 3, 64), (1, 1, 5, 67), (17, 0, 5, 67)])
def test_prologue_is_the_reference_lines(T, pad, h, w):
    """MPV.py:484-507 re-executed literally (rgb NHWC from the render, res [1,F,3,h,w], swd_patcht_size - 1 pad frames, scale_invariant) against
    LS.prologue in fp32: bit for bit, forward and gradient"""
    rgb0, res0, g_x = LS.prologue_inputs(T, pad, h, w, crop=True)
    leaf = rgb0.clone().requires_grad_(True)
    res = res0[None]
    rgb = leaf.permute(0, 3, 1, 2)
    rgb_pad = rgb
    if pad > 0:
        pad_frame = pad
        rgb_pad = torch.cat([rgb, rgb[:pad_frame]], 0)
    res_avg = res[0].mean(dim=0)
    rgb_avg = rgb.detach().mean(dim=0)
    scale = torch.exp(torch.log((res_avg + 0.01) / (rgb_avg + 0.01)).mean())
    scale = (scale + 3) / 4  # prevent scaling ambiguouity
    rgb_pad = rgb_pad * scale
    x = rgb_pad.permute(1, 0, 2, 3)[None]
    (g,) = torch.autograd.grad((x[0] * g_x).sum(), leaf)
    p = LS.prologue(rgb0, res0, pad, torch.float32, g_x)
    assert torch.equal(p["x"], x[0].detach()) and torch.equal(p["gain"], scale.detach()) and torch.equal(p["g_rgb"], g)
    assert float(p["log_sum"]) == pytest.approx(float(LS.log_terms(rgb0, res0, torch.float32).sum()), rel=1e-6)
    off = LS.prologue(rgb0, None, pad, torch.float32, g_x)
    assert torch.equal(off["x"], torch.cat([rgb, rgb[:pad]], 0).permute(1, 0, 2, 3).detach()) and off["gain"] is None


# ---- conditions on the case tables ----------------------------------------------------------------------------------------------------------------------
def test_frames_are_on_the_patch_grid_and_wider_than_64():
    for name, (ps, s, pt, st, H, W, nat) in LS.CONFIGS.items():
        assert (H - ps) % s == 0 and (W - ps) % s == 0 and H >= ps, name
        # two 64-wide tiles, the second ragged; three 32-wide ones; rows no multiple of 4 (a grid of fours has no other row count)
        assert 64 < W < 96 and (H % 4 != 0 or (ps % 4 == 0 and s % 4 == 0)) and H < 20, name
        cover = -(-ps // s)
        assert nat == ((3 if cover == 3 else 2 if cover <= 2 else 0) if (pt, st) == (3, 1) else 0), name
        for c in LS.cases(name):
            assert (c.Tx - pt) % st == 0 and c.Tx >= pt and (c.Ty - pt) % st == 0 and c.Ty >= pt, c
        txs, tys = sorted({c.Tx for c in LS.cases(name)}), sorted({c.Ty for c in LS.cases(name)})
        assert len(txs) == 4 and all(abs(a - b) < st for a, b in zip(txs, LS.TX)) and tys == sorted({LS.on_grid(t, pt, st) for t in LS.TY}), name
        assert {(c.Tx, c.Ty) for c in LS.cases(name)} == {(a, b) for a in txs for b in tys}, name      # every Tx meets every Ty
        if (pt, st) == (3, 1):
            # Tx 3: n1 == 1, groups past the third empty | 6: trailing empty groups at G = 8 | 13: last group short | 53: past the x queue
            assert txs == [3, 6, 13, 53] and -(-53 // 4) == 14 > 12 and -(-53 // 8) == 7 > 4 and -(-13 // 4) * 3 < 13 < -(-13 // 4) * 4
            assert min(c.grid[2] for c in LS.cases(name)) == 1 and min(c.grid[3] for c in LS.cases(name)) == 1
    assert {(r, sc) for c in ALL_CASES for r, sc in [(c.rou, c.scaling)]} == set(LS.RHOS)
    assert max(3 * c.Tx * c.cfg[4] * c.cfg[5] for c in ALL_CASES) == 3 * 53 * 19 * 75


def test_index_patterns_are_valid_and_differ_between_neighbours():
    for c in ALL_CASES:
        nn = LS.indices(c)
        h_o, w_o, n1, n2 = c.grid
        assert nn.shape == (h_o, w_o, n1) and nn.dtype == torch.int64 and int(nn.min()) >= 0 and int(nn.max()) <= n2 - 1, c
        horiz, vert = (nn[:, 1:] != nn[:, :-1]).double().mean(), (nn[1:] != nn[:-1]).double().mean()
        if c.pattern in ("first", "last") or n2 == 1:
            assert horiz == 0 and vert == 0 and int(nn.max()) == (0 if c.pattern == "first" else n2 - 1)
        elif c.pattern == "checker":
            assert horiz == 1 and vert == 1 and set(nn.unique().tolist()) == {0, n2 - 1}
        elif c.pattern == "ramp":
            assert vert == 1 and (horiz == 1 or n2 == 2), c
        else:
            assert horiz >= 0.4 and vert >= 0.4 and len(nn.unique()) == min(n2, len(nn.unique())) and int(nn.max()) == n2 - 1, (c, horiz, vert)
    # ... and no table is all n2 == 1
    assert sum(c.grid[3] > 2 for c in ALL_CASES) > len(ALL_CASES) // 2


def test_abs_kink_share_and_planted_zeros():
    """|x - y2x| <= ABS_GAP away from the planted zeros: at most 1 % of any case (measured: up to 0.23 %, nearly all of it the planted +-1 ulp and 2^-20 residuals); every case has planted exact
    zeros, +-1 ulp residuals and residuals over the clips' whole range"""
    worst = 0.0
    for c in ALL_CASES:
        st = LS.statement(c)
        e = st.l64[3]
        left_out = ((e.abs() <= LS.ABS_GAP) & ~st.planted).double().mean()
        worst = max(worst, float(left_out))
        assert left_out <= LS.ABS_SHARE, c
        assert int(st.planted.sum()) >= 3 and bool((e[st.planted] == 0).all())
        small = e[(e != 0) & (e.abs() < 1e-7)]
        assert small.numel() >= 3 and float(e.abs().max()) > 0.8, c
        if c.rou == "abs":
            assert bool((st.l64[2][st.planted] == 0).all()) and bool((st.l32[2][st.planted] == 0).all())
        if c.rou in ("-2", "1"):      # residuals so small that u = (e / scale)^2 / b + 1 rounds to 1 in fp32
            z = small.float() / np.float32(c.scaling)
            assert bool((z * z / 4 + 1 == 1).any())
    print(f"largest share of voxels left out of the 'abs' gradient comparison: {100 * worst:.4f} %")


def test_zero_noise_cases_are_the_single_vote_ones():
    """one vote per voxel (ps == stride, and pt == stridet or a single patch in time): the oracle's fp32 sum and y2x are exact, B == 0 -- the kernels get nothing there"""
    for c in ALL_CASES:
        st = LS.statement(c)
        ps, s, pt, stt = c.cfg[:4]
        single = ps == s and (pt == stt or c.grid[2] == 1)
        assert (float(st.f64[1].max()) == 1.0) == single
        assert torch.equal(st.f32[1].double(), st.f64[1])
        if single:
            assert LS.noise(st.f32[0], st.f64[0]) == 0 and LS.noise(st.f32[2], st.f64[2]) == 0
        else:      # (zero also where every voxel's votes are one value k times, k in {1, 2, 4}: no order of the adds rounds)
            n = LS.noise(st.f32[0], st.f64[0])
            assert 0 < n < 1e-4 or (n == 0 and (c.grid[3] == 1 or c.pattern in ("first", "last")) and set(st.f64[1].unique().tolist()) <= {1.0, 2.0, 4.0}), c


def test_fold_choice_gives_each_row_of_the_gpu_table(UV):
    """asked of the library without a device: every (shape, nb) row of every case launches exactly that instantiation; together 5 shapes x nb
    {0, 2, 3}, and variant 1 of the plain entry the unstaged kernel"""
    seen = set()
    for c in ALL_CASES:
        for shape, nb, variant in LS.rows(c.config):
            for fused in (False, True):
                rc, ch = UV.fold_choice(LS.desc_of(c, variant), fused)
                assert rc == 0 and (ch.staged, ch.shape, ch.nb, (ch.fw, ch.fh, ch.threads)) == (1, shape, nb, LS.FOLD_SHAPES[shape]), (c, shape, nb, fused)
            seen.add((shape, nb))
        rc, ch = UV.fold_choice(LS.desc_of(c, 1), False)
        assert rc == 0 and (ch.staged, ch.shape, ch.threads) == (0, -1, 256)
        assert UV.fold_choice(LS.desc_of(c, 1), True)[1].staged == 1          # the fused entry has the staged kernel only
    assert seen == {(i, nb) for i in range(5) for nb in (0, 2, 3)}
    for name in LS.CONFIGS:
        assert {(s_, n_) for s_, n_, _ in LS.rows(name)} >= {(i, LS.CONFIGS[name][6]) for i in range(5)}


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------------------------
def _fold_ratio(st, sm, w):
    """the excess of a faulty (sum, weight) over the allowances of sum and y2x (1.0 = the bound)"""
    y2x = sm / w
    r1 = LS.excess(sm, st.f64[0], LS.M_EXACT * LS.noise(st.f32[0], st.f64[0]))[1]
    r2 = LS.excess(y2x, st.f64[2], LS.M_EXACT * LS.noise(st.f32[2], st.f64[2]), LS.Y2X_ULPS)[1]
    return max(r1, r2)


def _fold_faults(st):
    """fault name -> excess, each planted in the oracle's fp32 fold of this case"""
    c = st.case
    ps, s, pt, stt, H, W, _ = c.cfg
    h_o, w_o, n1, n2 = c.grid
    f32 = lambda nn=st.nn, src=None: LS.fold(st.y, nn, ps, pt, s, stt, c.Tx, torch.float32, src)[:2]      # noqa: E731
    out = {}
    # one vote dropped at a tile-border pixel: the first pixel of the second 64-wide tile, frame 0 -- its first covering location's vote
    sm, w = (t.clone() for t in st.f32[:2])
    eta, xi = 1, 64
    by, bx = max(0, (eta - ps + s) // s), max(0, (xi - ps + s) // s)
    sm[:, 0, eta, xi] -= st.y[:, int(st.nn[by, bx, 0]) * stt, eta, xi]
    w[0, eta, xi] = (w[0, eta, xi] - 1).clamp_min(1e-10)
    out["vote dropped at a tile border"] = _fold_ratio(st, sm, w)
    # one location's index row swapped with its right neighbour's
    differ = (st.nn[:, 1:] != st.nn[:, :-1]).any(-1).nonzero()
    by, bx = differ[len(differ) // 2].tolist()
    nn = st.nn.clone()
    nn[by, bx], nn[by, bx + 1] = st.nn[by, bx + 1], st.nn[by, bx]
    out["index row swapped with the right neighbour's"] = _fold_ratio(st, *f32(nn))
    # one patch's index off by one frame
    nn = st.nn.clone()
    i = n1 // 2
    nn[h_o // 2, w_o // 2, i] += 1 if int(nn[h_o // 2, w_o // 2, i]) < n2 - 1 else -1
    out["one index off by one frame"] = _fold_ratio(st, *f32(nn))
    # the count at the last frame off by one
    w = st.f32[1].clone()
    w[c.Tx - 1] += 1
    out["count at the last frame off by one"] = _fold_ratio(st, st.f32[0], w)
    # frame j + 2 read as j + 1 for one temporal group (the patch-major form's third running sum): the second of four groups
    if (pt, stt) == (3, 1):
        chunk = -(-c.Tx // 4)
        grp = (torch.arange(n1) >= chunk) & (torch.arange(n1) < 2 * chunk)
        assert bool(grp.any())
        out["frame j+2 read as j+1 for one group"] = _fold_ratio(st, *f32(src=lambda kt: st.nn * stt + (torch.where(grp, 1, 2) if kt == 2 else kt)))
    # gscale from the untrimmed size (one more row and column than the patch grid keeps)
    n_trim, n_full = 3 * c.Tx * H * W, 3 * c.Tx * (H + 1) * (W + 1)
    g = st.l32[2] * np.float32(n_trim / n_full)
    out["gscale from the untrimmed size"] = LS.excess(g, st.l64[2], LS.M_EXACT * LS.noise(st.l32[2], st.l64[2], st.grad_sel), LS.GRAD_ULPS + LS.RHO_ULPS, st.grad_sel)[1]
    # rho' of the general case with exponent d / 2 instead of d / 2 - 1
    if c.rou in ("-2", "1"):
        g = (LS.rho_grad_general(st.l32[3], c.rou, np.float32(c.scaling), 0.0) / np.float32(n_trim)).float()
        ok = (LS.rho_grad_general(st.l32[3], c.rou, np.float32(c.scaling)) / np.float32(n_trim)).float()
        B = LS.M_EXACT * LS.noise(st.l32[2], st.l64[2])
        assert LS.excess(ok, st.l64[2], B, LS.GRAD_ULPS + LS.RHO_ULPS)[1] <= 1.0          # the closed form itself passes
        out["rho' with exponent d/2"] = LS.excess(g, st.l64[2], B, LS.GRAD_ULPS + LS.RHO_ULPS)[1]
    return out


def test_planted_faults_land_at_four_bounds_or_more():
    """the oracle's fp32 evaluation stands in for the kernel; each fault is planted in it alone, at the Tx = 13 and Tx = 53 cases of every
    configuration whose indices differ between neighbours, and at the prologue cases with 0 < pad < T.  Per fault the SMALLEST excess over its cases
    (measured / allowance, 1.0 = the bound): all at 4 or more, so the factor M_EXACT = 16 could grow fourfold at most before a fault passes."""
    worst = {}
    for c in ALL_CASES:
        if c.pattern not in ("random", "ramp") or c.Tx < 12 or c.grid[3] < 3:
            continue
        for k, v in _fold_faults(LS.statement(c)).items():
            worst[k] = min(worst.get(k, np.inf), v)
    for T, pad, h, w in [p for p in LS.prologue_cases() if 0 < p[1] < p[0]]:
        rgb, res, g_x, p64, p32, _, _ = LS.prologue_statement(T, pad, h, w, True, True)
        Bg, Bx = LS.M_EXACT * LS.noise(p32["g_rgb"], p64["g_rgb"]), LS.M_EXACT * LS.noise(p32["x"], p64["x"])
        g = (g_x[:, :T] * p32["gain"]).permute(1, 2, 3, 0)
        worst["pad frames' gradient not added"] = min(worst.get("pad frames' gradient not added", np.inf), LS.excess(g, p64["g_rgb"], Bg)[1])
        bad = LS.prologue(rgb, res, pad, torch.float32, g_x, gain_frames=T + pad)
        r = max(LS.excess(bad["x"], p64["x"], Bx)[1], LS.excess(bad["g_rgb"], p64["g_rgb"], Bg)[1])
        worst["gain's rgb mean over T + pad"] = min(worst.get("gain's rgb mean over T + pad", np.inf), r)
    for k, v in sorted(worst.items(), key=lambda kv: kv[1]):
        print(f"[{k}] smallest measured / allowance over its cases: {v:.1f}")
    assert len(worst) == 9
    print(f"smallest planted fault: {min(worst, key=worst.get)} at {min(worst.values()):.1f} bounds (factor {LS.M_EXACT:g}); it would pass at a factor of "
          f"{LS.M_EXACT * min(worst.values()):.0f}")
    assert min(worst.values()) >= 4.0, worst


def test_the_pristine_fp32_oracle_passes():
    """... and the comparison passes what it should: the oracle in fp32 sits at 1 / M_EXACT of every bound, the scalar loss inside B_loss"""
    for c in ALL_CASES[::7]:
        st = LS.statement(c)
        rep = LS.Report(f"{c.config} Tx {c.Tx} Ty {c.Ty} {c.pattern} rou {c.rou} s {c.scaling}")
        rep.check("sum", st.f32[0], st.f64[0], st.f32[0])
        rep.exact("weight", st.f32[1], st.f64[1])
        rep.check("y2x", st.f32[2], st.f64[2], st.f32[2], LS.Y2X_ULPS)
        rep.check("rho", st.l32[0], st.l64[0], st.l32[0])
        rep.check("grad", st.l32[2], st.l64[2], st.l32[2], LS.GRAD_ULPS, st.grad_sel)
        B = st.loss_bound(LS.frames_per_thread(c, 0), 8)
        print(f"[{rep.tag}] loss: B_loss {B:.3e}, fp32 mean off by {abs(float(st.l32[1]) - float(st.l64[1])):.3e} of {float(st.l64[1]):.3e}")
        assert abs(float(st.l32[1]) - float(st.l64[1])) <= B
        rep.done()
