"""tests/terms_statement.py without a device: the statement in fp32 is the reference's lines bit for bit (train_3d.py:200-220 written out as
test_stage1_loss_equals_the_torch_chain writes them), its sparsity and density are oracle/mpv_oracle.py's on per-plane alphas, the case tables of
tests/test_gpu_terms_fp64.py are what they claim, and planted faults: each is applied to the fp32 oracle's output and has to land at 4 bounds or
more -- the cap on the bound's factor."""
import dataclasses
import math
import types

import numpy as np
import pytest
import torch

import terms_statement as TS
from videoloop3d_amd import synth

ALL_CASES = [c for shape in TS.SHAPES for c in TS.cases(shape)]


# ---- the statement is the reference's ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gain", [((2, 37, 53), True), ((1, 5, 7), True), ((3, 24, 32), False)])
def test_statement_in_fp32_is_the_reference_lines(shape, gain):
    """train_3d.py:200-220 written out, as test_stage1_loss_equals_the_torch_chain writes it, on the module's output rgbl (MPI.py:600: an NHWC
    render viewed as NCHW, the label its last channel) against TS.objective in fp32: img_loss, loop_loss, the gain and the gradient of w_img img + w_loop loop, bit for bit"""
    c = TS.Case(shape, "crop", "all", gain, TS.WEIGHTS[1], TS.EPS[0], TS.MPI_D[0])
    st = TS.statement(c)
    x = st.x
    leaf = torch.cat([x.rgb, x.label[..., None]], -1).clone().requires_grad_(True)
    target, tm = x.target, x.tmask
    r = leaf.permute(0, 3, 1, 2)
    lm = torch.clamp(r[:, -1], 0.001, 1 - 0.001)
    loop_t = -(tm * torch.log(lm) + (1 - tm) * torch.log(1 - lm)).mean()
    rgb = r[:, :3]
    sc = torch.ones(())
    if gain:
        sc = (torch.exp(torch.log((target + 0.01) / (rgb.detach() + 0.01)).mean()) + 3) / 4
        rgb = rgb * sc
    img_t = ((rgb - target) ** 2).mean()
    W = [np.float32(v) for v in c.weights]
    (g,) = torch.autograd.grad(float(W[0]) * img_t + float(W[1]) * loop_t, leaf)
    o = st.r32
    assert o.out.dtype == torch.float32
    assert float(o.out[1]) == float(img_t.detach()) and float(o.out[2]) == float(loop_t.detach()) and float(o.out[7]) == float(sc.detach())
    assert torch.equal(o.g["rgb"], g[..., :3]) and torch.equal(o.g["label"], g[..., 3])
    assert float((g[..., 3] == 0).float().mean()) > 0.05 and float(g[..., 3].abs().max()) > 0


def test_sparsity_and_density_are_the_oracles_on_per_plane_alphas():
    """oracle/mpv_oracle.mpi_forward (MPI.py:603-607, 647-650 on the composited layers) on a tiny scene whose view leaves part of the crop uncovered:
    the statement from (sum a, sum a^2) and alpha gives the oracle's sparsity and density; for a >= 0 the spelling from the sums IS the reference's
    norm(p=1) / norm(p=2).clamp_min(eps), and d / d sum a^2 is 0 at an all-zero pixel in fp32 and fp64"""
    from oracle import mpv_oracle as MPO
    MO = MPO.MO
    H, W, D, h, w = 20, 28, 6, 12, 16
    args = types.SimpleNamespace(mpi_h_scale=1.0, mpi_w_scale=1.0, mpi_d=D, rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color="",
                                 sparsity_loss_weight=0.004, rgb_smooth_loss_weight=0.0, a_smooth_loss_weight=0.0, density_loss_weight=0.02)
    K = torch.tensor([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]], dtype=torch.float32)
    K_crop = K.clone()
    K_crop[0, 2] += 4.0          # the crop looks past the planes' left edge
    ext = torch.eye(4)[None]
    stack = synth.make_plane_stack(D, 1, H, W, seed=5, alpha_bias=0.0)
    _, extra = MPO.mpi_forward(stack, None, args, H, W, np.eye(4, dtype=np.float32), K, 1.0, 100.0, h, w, ext, K_crop[None])
    mpi_h, mpi_w, planedepth, ref_intrin_mpi, extrins = MPO._geometry(args, D, H, W, np.eye(4, dtype=np.float32), K, 1.0, 100.0, ext, (H, W))
    homos = MPO._homos(ref_intrin_mpi, extrins[:1], K_crop[None], planedepth)
    layers, cov = MPO._layers(stack, homos, h, w, args, mpi_h, mpi_w, 0.5, None, None)
    a = MO.layers_to_slots(layers, cov)[..., -1]
    alpha = MO.overcompose(layers[..., 3], layers[..., :3])[1].sum(-1)
    asum = torch.stack([a.sum(-1), (a * a).sum(-1)], -1)
    assert float((asum[..., 1] == 0).float().mean()) > 0.05 and float((asum[..., 1] > 0.1).float().mean()) > 0.3
    eps = TS.f32(1e-6)
    sp = TS.sparsity_terms(asum, eps).mean() * TS.f32(1.0 / np.sqrt(D))
    assert float(sp) == pytest.approx(float(extra["sparsity"]), rel=1e-6) and float(extra["sparsity"]) > 0.1
    assert float(TS.density_terms(alpha).mean()) == pytest.approx(float(extra["density"]), rel=1e-6)
    # the two spellings in fp64 on hash planes with uncovered pixels and pixels of faint planes, and their gradients where a > 0
    for eps_ in TS.EPS:
        e = TS.f32(eps_)
        a = synth.hash_uniform((3, 7, 9, TS.PLANES), seed=9).double()
        a[0, :2] = 0
        a[1, :2] *= 1e-7
        a = a.requires_grad_(True)
        ref = a.norm(dim=-1, p=1) / a.norm(dim=-1, p=2).clamp_min(e)
        got = TS.sparsity_terms(torch.stack([a.sum(-1), (a * a).sum(-1)], -1), e)
        assert float((got - ref).detach().abs().max()) <= 1e-12 * float(ref.detach().abs().max())
        g_ref, g_got = torch.autograd.grad(ref.sum(), a)[0], torch.autograd.grad(got.sum(), a)[0]
        pos = (a > 0).all(-1)
        assert float((g_got - g_ref)[pos].abs().max()) <= 1e-9 * float(g_ref[pos].abs().max())
    for dtype in (torch.float32, torch.float64):
        z = torch.zeros((4, 2), dtype=dtype, requires_grad=True)
        (g,) = torch.autograd.grad(TS.sparsity_terms(z, eps).sum(), z)
        assert bool((g[:, 1] == 0).all()) and bool((g[:, 0] == 1 / torch.tensor(eps, dtype=dtype)).all())


def test_head_statement_is_the_reference_total():
    """train_3dvid.py:230-240 literally: loss = swd; loss = loss + weight_k * term_k in order"""
    for n in TS.HEAD_N:
        v, coef, groups = TS.head_inputs(n, 3)
        loss = v[0] * coef[0]
        for k in range(1, n):
            loss = loss + v[k] * coef[k]
        total, share = TS.head(v, coef, groups, 3, torch.float32)
        assert float(total) == float(loss)
        assert float(share.double().sum()) == pytest.approx(float(total), rel=1e-5, abs=1e-6)


# ---- conditions on the case tables ----------------------------------------------------------------------------------------------------------------------
def test_shapes_and_tables_are_what_they_claim():
    ns = [b * h * w for b, h, w in TS.SHAPES]
    assert ns == [1, 35, 258, 3922, 2304] and ns[1] < 64 and -(-ns[2] // 256) == 2
    n_big = TS.BIG[0] * TS.BIG[1] * TS.BIG[2]
    assert n_big == 1051650 and -(-n_big // 256) > TS.GRID_CAP and n_big - TS.GRID_CAP * 256 == 3074 and TS.trips(n_big) == 2 and TS.trips(ns[3]) == 1
    assert 3 * n_big < 2 ** 24                                                        # (float)(3 n) is exact in every case
    assert TS.SCALE_N[2] // 4 - TS.SCALE_CAP * 256 == 257 and TS.trips(TS.SCALE_N[2] // 4, cap=TS.SCALE_CAP) == 2 and TS.SCALE_N[1] // 4 == 257
    assert {(c.subset, c.gain) for c in ALL_CASES} == {(s, g) for s in TS.SUBSETS for g in (True, False)}
    assert {(c.subset, c.layout) for c in ALL_CASES} == {(s, l) for s in TS.SUBSETS for l in TS.LAYOUTS}
    assert {c.weights for c in ALL_CASES} == set(TS.WEIGHTS) and {c.eps for c in ALL_CASES} == set(TS.EPS) and {c.mpi_d for c in ALL_CASES} == set(TS.MPI_D)
    for s in TS.SHAPES:
        assert len(TS.cases(s)) == 12 and {c.eps for c in TS.cases(s)} == set(TS.EPS)
    flat = [w for ws in TS.WEIGHTS for w in ws]
    assert 0.0 in flat and any(math.frexp(w)[0] != 0.5 for w in flat if w)            # a zero weight, weights that are no power of two
    assert any(ws[1] not in (0.0, 1.0) for ws in TS.WEIGHTS)
    for n in TS.HEAD_N:
        for ng in TS.HEAD_NGROUPS:
            v, coef, groups = TS.head_inputs(n, ng)
            assert len(groups) == n and max(groups) == ng - 1 and min(groups) >= 0
    _, _, groups = TS.head_inputs(16, 16)
    assert groups[15] == 15 and TS.groups_word(groups) >> 60 == 15 and TS.groups_word(groups) < 2 ** 64


@pytest.mark.parametrize("shape", TS.SHAPES + (TS.BIG,))
def test_planted_inputs_are_what_they_claim(shape):
    B, h, w = shape
    n = B * h * w
    up, dn = torch.tensor(2.0), torch.tensor(-1.0)
    lo, hi = torch.tensor(TS.LO, dtype=torch.float32), torch.tensor(TS.HI, dtype=torch.float32)
    for eps in TS.EPS:
        for layout in TS.LAYOUTS:
            x = TS.inputs(shape, layout, eps)
            t, m = x.target, x.tmask
            assert t.shape == (B, 3, h, w) and m.shape == (B, h, w) and t.stride(3) == 1 and m.stride(2) == 1
            if layout == "crop":      # the strides really are a crop's, the parents hold sentinels around it
                assert t.stride(2) > w and t.stride(0) != 3 * t.stride(1) and t.stride(0) > 3 * h * t.stride(2) and m.stride(1) > w
                assert m.stride(1) != t.stride(2) and t.storage_offset() > 0 and m.storage_offset() > 0 and not t.is_contiguous()
                assert int((t._base == TS.SENTINEL).sum()) == t._base.numel() - t.numel() and int((m._base == TS.SENTINEL).sum()) == m._base.numel() - m.numel()
            else:
                assert t.is_contiguous() and m.is_contiguous()
            assert float(t.min()) >= 0 and float(t.max()) < 1 and float(x.rgb.min()) >= 0 and float(x.rgb.max()) < 1
            # the floor decides identically in fp32, fp64 and the kernel
            y = x.asum[..., 1].double()
            n2 = torch.sqrt(y.clamp_min(TS.TINY))
            assert float(((n2 - TS.f32(eps)).abs() / TS.f32(eps)).min()) >= TS.FLOOR_GAP
            n2f = torch.sqrt(x.asum[..., 1].clamp_min(TS.TINY))
            assert torch.equal(n2f < np.float32(eps), n2 < TS.f32(eps)) and torch.equal(x.asum[..., 1] < np.float32(1e-30), y < TS.TINY)
        if n == 1:      # the single pixel is an ordinary one
            assert int(x.cls.max()) == 0
            continue
        cls, lab, al, ys = x.cls.flatten(), x.label.flatten(), x.alpha.flatten(), x.asum.reshape(n, 2)
        count = lambda k: int((cls == k).sum())      # noqa: E731
        want = max(1, n // TS.PERIOD)
        assert all(count(k) in (want, want + 1) for k in range(1, min(n, 35)))            # every planted class has its 1 / 67 share
        pl = TS.planted_labels()
        assert torch.equal(pl[:2], torch.stack([lo, hi])) and pl[2] < lo < pl[3] and pl[4] < hi < pl[5] and pl[6] < 0 and pl[7] > 1
        assert torch.equal(pl[2:6], torch.stack([torch.nextafter(lo, dn), torch.nextafter(lo, up), torch.nextafter(hi, dn), torch.nextafter(hi, up)]))
        for k in range(8):
            assert bool((lab[cls == TS.LABEL_CLASS + k] == pl[k]).all())
        outside = ((lab < lo) | (lab > hi)).float().mean()
        assert 0.05 < float(outside) < 0.3 and float(lab.min()) < 0 and float(lab.max()) > 1
        pa = TS.planted_alphas()
        assert pa.tolist() == [1.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 0.0, float(np.float32(1.2))]
        for k in range(5):
            assert bool((al[cls == TS.ALPHA_CLASS + k] == pa[k]).all())
        ps = TS.planted_asums(eps)
        e2 = TS.f32(eps) ** 2
        assert ps.shape == (18, 2) and [float(v) for v in ps[::3, 1]] == [float(np.float32(v)) for v in (0.0, 1e-38, 1e-31, 1e-29, e2 / 4, 4 * e2)]
        assert float(ps[0, 0]) == 0 and bool((ps[1:, 0] > 0).all()) and float(ps[9, 1]) > TS.TINY > float(ps[6, 1]) and float(ps[12, 1]) < e2 < float(ps[15, 1])
        if n > TS.ASUM_CLASS + 18:
            for k in range(18):
                assert bool((ys[cls == TS.ASUM_CLASS + k] == ps[k]).all())
        st = TS.Statement(TS.Case(shape, layout, "all", True, TS.WEIGHTS[0], eps, 32), x, None, None)
        sel = st.sel
        assert int(sel["uncovered"].sum()) == sum(count(TS.ASUM_CLASS + k) for k in range(9))
        assert int(sel["floor"].sum()) == sum(count(TS.ASUM_CLASS + k) for k in range(9, 15)) and int(sel["ordinary"].sum()) == n - sum(count(TS.ASUM_CLASS + k) for k in range(18))
        assert int(sel["above"].sum()) == sum(count(TS.ASUM_CLASS + k) for k in range(15, 18))          # the 4 eps^2 class alone: no hash pixel is near the floor
        mk = x.tmask.flatten()
        soft = int(((mk != 0) & (mk != 1)).sum())
        assert soft == sum(count(k) for k in TS.SOFT_QUARTER + TS.SOFT_HALF) and set(mk.unique().tolist()) == {0.0, 0.25, 0.5, 1.0}
        if n > TS.ZERO_CLASS + 1:
            z = (cls == TS.ZERO_CLASS) | (cls == TS.ZERO_CLASS + 1)
            assert bool((x.rgb.reshape(n, 3)[z] == 0).all()) and bool((x.target.permute(0, 2, 3, 1).reshape(n, 3)[z] == 0).all())
            lg = torch.log((x.target + np.float32(0.01)) / (x.rgb.permute(0, 3, 1, 2) + np.float32(0.01)))
            assert bool((lg.permute(0, 2, 3, 1).reshape(n, 3)[z] == 0).all())


# ---- planted faults ---------------------------------------------------------------------------------------------------------------------------------------
def _ratio(st, **over):
    o = TS.oracle_outputs(st)
    o.update(over)
    rep = TS.Report("fault", quiet=True)
    TS.check_objective(rep, st, **o)
    return rep.worst


def _all_of(r):
    return TS.oracle_outputs(None, r)


def _restrided(view, strides, mod=False):
    """`view` read again from its parent through other strides (the same offset); mod: indices wrap inside the parent"""
    base = view._base
    if not mod:
        return torch.as_strided(base, view.shape, strides, view.storage_offset())
    idx = torch.zeros(view.shape, dtype=torch.int64) + view.storage_offset()
    for d, s in enumerate(strides):
        shape = [1] * view.dim()
        shape[d] = view.shape[d]
        idx = idx + (torch.arange(view.shape[d]) * s).reshape(shape)
    return base.flatten()[idx % base.numel()]


def _missing(st, pixels):
    """the smallest excess, over the sums a case has, of that sum formed without `pixels` (a bool [B,h,w])"""
    c, r32 = st.case, st.r32
    W = [TS.f32(v) for v in c.weights]
    sps = TS.f32(1.0 / np.sqrt(c.mpi_d))
    worst = math.inf
    for i, k, wt in ((1, "img", W[0]), (2, "loop", W[1]), (3, "sp", W[2] * sps), (4, "dn", W[3])):
        t = r32.t[k]
        if t is None or (wt == 0 and i > 2):
            continue
        part = float((t.permute(0, 2, 3, 1)[pixels] if t.dim() == 4 else t[pixels]).double().sum()) / t.numel()
        out = r32.out.clone()
        out[i] -= part * (wt if i > 2 else 1.0)
        out[0] -= part * wt
        worst = min(worst, _ratio(st, out=out))
    return worst


def _faults(st):
    """fault name -> excess (measured / allowance, the largest over the outputs), each planted in the oracle's fp32 outputs of this case"""
    c, x, r32 = st.case, st.x, st.r32
    has_label, has_alpha, has_asum, has_smooth = c.has
    B, h, w = c.shape
    n = c.n
    W = [np.float32(v) for v in c.weights]
    sps = np.float32(1.0 / np.sqrt(c.mpi_d))
    sel = st.sel
    out = {}
    if c.gain and W[0] != 0:
        out["gain not detached"] = _ratio(st, g_rgb=TS.objective(x, c, torch.float32, gain_detached=False).g["rgb"])
    if W[0] != 0:
        out["count n where 3 n belongs"] = _ratio(st, g_rgb=r32.g["rgb"] * 3)
    if has_label and W[1] != 0:
        out["count 3 n where n belongs"] = _ratio(st, g_label=r32.g["label"] / 3)
        if W[1] != 1:
            out["w_loop applied to g_label twice"] = _ratio(st, g_label=r32.g["label"] * W[1])
        if bool(sel["outside"].any()):
            m, l = x.tmask, torch.clamp(x.label, TS.LO, TS.HI)
            g = -(m / l - (1 - m) / (1 - l)) * (W[1] / np.float32(n))
            out["clamp gradient not cut"] = _ratio(st, g_label=torch.where(sel["outside"], g, r32.g["label"]))
    if has_asum and W[2] != 0:
        out["sparsity_scale dropped"] = _ratio(st, g_asum=r32.g["asum"] / sps)
        low = sel["uncovered"] | sel["floor"]
        if bool((low & (x.asum[..., 0] > 0)).any()):
            n2 = torch.sqrt(x.asum[..., 1].clamp_min(TS.TINY))
            gy = -x.asum[..., 0] / (2 * n2 * n2 * n2) * (W[2] * sps / np.float32(n))
            g = r32.g["asum"].clone()
            g[..., 1] = torch.where(low, gy, g[..., 1])
            out["floor-side d / d sum a^2 not zeroed"] = _ratio(st, g_asum=g)
    if c.layout == "crop":
        t, m = x.target, x.tmask
        if h > 1:
            bad = dataclasses.replace(x, target=_restrided(t, (t.stride(0), t.stride(1), w, 1)))
            out["t_sr taken as w"] = _ratio(st, **_all_of(TS.objective(bad, c, torch.float32)))
        if B > 1:
            bad = dataclasses.replace(x, target=_restrided(t, (3 * h * w, t.stride(1), t.stride(2), 1)))
            out["batch stride taken as 3 h w"] = _ratio(st, **_all_of(TS.objective(bad, c, torch.float32)))
        if has_label and h > 1 and W[1] != 0:
            bad = dataclasses.replace(x, tmask=_restrided(m, (t.stride(0), t.stride(2), 1), mod=True))
            out["mask read at the target's strides"] = _ratio(st, **_all_of(TS.objective(bad, c, torch.float32)))
    if n > 256:
        block = (torch.arange(n) < 256).reshape(B, h, w)
        out["one workgroup's 256 pixels missing from a sum"] = _missing(st, block)
    if TS.trips(n) > 1:
        out["the second grid trip skipped"] = _missing(st, (torch.arange(n) >= TS.GRID_CAP * 256).reshape(B, h, w))
    return out


def test_planted_faults_land_at_four_bounds_or_more():
    """the oracle's fp32 evaluation stands in for the kernel; each fault is planted in it alone, at every case of every shape it can show at (and the
    big shape for the sums).  Per fault the SMALLEST excess over its cases (measured / allowance, 1.0 = the bound): all at 4 or more, so the factor
    M_EXACT = 16 could grow fourfold at most before a fault passes."""
    worst = {}
    for c in ALL_CASES + [TS.BIG_CASE]:
        st = TS.statement(c)
        assert _ratio(st) <= 1.0, c          # the pristine oracle passes
        for k, v in _faults(st).items():
            worst[k] = min(worst.get(k, math.inf), v)
    # a head term summed into the neighbouring group
    for n in TS.HEAD_N[1:]:
        for ng in TS.HEAD_NGROUPS[1:]:
            v, coef, groups = TS.head_inputs(n, ng)
            total, share = TS.head(v, coef, groups, ng, torch.float64)
            i = n // 2
            bad = list(groups)
            bad[i] = (groups[i] + 1) % ng
            _, share_bad = TS.head(v, coef, bad, ng, torch.float32)
            r = max(abs(float(share_bad[g]) - float(share[g])) / TS.head_bound(v, coef, torch.tensor(groups) == g) if any(q == g for q in groups)
                    else math.inf for g in (groups[i], bad[i]))
            worst["a head term summed into the neighbouring group"] = min(worst.get("a head term summed into the neighbouring group", math.inf), r)
    for k, v in sorted(worst.items(), key=lambda kv: kv[1]):
        print(f"[{k}] smallest measured / allowance over its cases: {v:.1f}")
    assert len(worst) == 13, sorted(worst)
    print(f"smallest planted fault: {min(worst, key=worst.get)} at {min(worst.values()):.1f} bounds (factor {TS.M_EXACT:g})")
    assert min(worst.values()) >= 4.0, worst


def test_the_pristine_fp32_oracle_passes_every_check():
    """... and the comparison passes what it should: the oracle in fp32 sits at 1 / M_EXACT of every per-element bound, its scalars inside theirs;
    the unit-sum statements and the head likewise"""
    for c in ALL_CASES[::5]:
        st = TS.statement(c)
        rep = TS.Report(f"{c}")
        TS.check_objective(rep, st, **TS.oracle_outputs(st))
        rep.done()
        assert max((r for name, B, _, _, r in rep.rows if name.startswith("g_") and B > 0), default=0.0) <= 1.0 / TS.M_EXACT      # (B == 0: g_alpha, under its ulp alone)
    for shape in TS.SHAPES[1:4]:
        for C, gain in ((4, True), (3, False)):
            st = TS.statement(TS.loss_case(shape, C, gain), unit=True)
            r = st.r32
            grad = torch.cat([r.g["rgb"]] + ([r.g["label"][..., None]] if C == 4 else []), -1)
            sums = [float(r.t["img"].sum()), float(r.t["loop"].sum()) if C == 4 else 0.0]
            rep = TS.Report(f"stage1_loss {shape} C {C}")
            TS.check_stage1_loss(rep, st, C, sums, grad, float(r.t["log"].sum()) if gain else None)
            rep.done()
        for which in ("both", "sparsity", "density"):
            st = TS.statement(TS.terms_case(shape, which, TS.EPS[1]), unit=True)
            r = st.r32
            sums = [0.0 if r.t["sp"] is None else float(r.t["sp"].sum()), 0.0 if r.t["dn"] is None else float(r.t["dn"].sum())]
            rep = TS.Report(f"pixel_terms {shape} {which}")
            TS.check_pixel_terms(rep, st, sums, r.g["asum"], r.g["alpha"])
            rep.done()
    for n in TS.HEAD_N:
        for ng in TS.HEAD_NGROUPS:
            v, coef, groups = TS.head_inputs(n, ng)
            t64, s64 = TS.head(v, coef, groups, ng, torch.float64)
            t32, s32 = TS.head(v, coef, groups, ng, torch.float32)
            assert abs(float(t32) - float(t64)) <= TS.head_bound(v, coef)
            for g in range(ng):
                assert abs(float(s32[g]) - float(s64[g])) <= TS.head_bound(v, coef, torch.tensor(groups) == g)
