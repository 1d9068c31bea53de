"""The looping loss after the search -- vote_fold_k, the 15 vote_fold_lds_k instantiations, the fused robust loss and its gradient, robust_fwd_k /
robust_bwd_k and the four loop_*_k prologue kernels -- against the fp64 statement of tests/loss_statement.py, through the C ABI with constructed
tensors.  The search does not run here: the fold gets indices of the test's choosing (all first, all last, checker, hash-random and a ramp per
location and patch; valid ones only).  Clips are hash-uniform, so a wrong frame or pixel is off by O(0.3) against bounds of 1e-6 to 1e-4.
Bounds: per case and output 16 max |oracle fp32 - oracle fp64| plus the named ulp allowances of loss_statement's docstring; the weight exactly.
tests/test_loss_statement_cpu.py shows what the comparison catches without a device, and that every row below launches the instantiation it names
(asserted again here before each call).  Every row and entry is compared with the statement directly, and every comparison prints its bound beside
the measured maximum."""
import numpy as np
import pytest
import torch

import loss_statement as LS

pytestmark = pytest.mark.gpu
SENTINEL = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _L():
    from videoloop3d_amd import _lib as L
    return L


def _rho(rou):
    L = _L()
    if rou in ("mse", "abs"):
        return L.RHO[rou], 0.0
    return L.RHO["barron"], float(rou)


def _general(rou):
    return rou in ("-2", "1")


def _ok(rc, what):
    _L().check(rc, what)


def _fold(dev, desc, y, nn, normalize):
    L = _L()
    s = torch.full((3, desc.Tx, desc.H, desc.W), SENTINEL, dtype=torch.float32, device=dev)
    w = torch.full((desc.Tx, desc.H, desc.W), SENTINEL, dtype=torch.float32, device=dev)
    _ok(L.lib().vl3d_vote_fold(desc, L.ptr(y), L.ptr(nn), L.ptr(s), L.ptr(w), normalize, L.stream_ptr(dev)), "vl3d_vote_fold")
    return s, w


def _fused(dev, desc, y, nn, x, rou, scaling, write):
    L = _L()
    kind, r = _rho(rou)
    shape = (3, desc.Tx, desc.H, desc.W)
    y2x = torch.full(shape, SENTINEL, dtype=torch.float32, device=dev) if write else None
    w = torch.full(shape[1:], SENTINEL, dtype=torch.float32, device=dev) if write else None
    gx = torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)
    acc = torch.full((1,), SENTINEL, dtype=torch.float64, device=dev)
    _ok(L.lib().vl3d_vote_fold_robust(desc, L.ptr(y), L.ptr(nn), L.ptr(x), kind, r, float(scaling), L.ptr(y2x), L.ptr(w), L.ptr(gx), L.ptr(acc),
                                      L.stream_ptr(dev)), "vl3d_vote_fold_robust")
    return y2x, w, gx, float(acc) / gx.numel()


def _box(dev, t, fill=True):
    """t [3,T,H,W] as a box inside a buffer one frame, 3 rows and 5 columns larger on each axis' far side and 1 / 2 / 3 on the near side, the rest
    SENTINEL -> (buffer, view)"""
    _, T, H, W = t.shape
    big = torch.full((3, T + 2, H + 5, W + 8), SENTINEL, dtype=torch.float32, device=dev)
    view = big[:, 1:1 + T, 2:2 + H, 3:3 + W]
    if fill:
        view.copy_(t)
    return big, view


def _strided(dev, c, variant, y, nn, x, rou, scaling):
    """the strided entry: x, y and grad_x are boxes inside larger buffers (row pitch > W, frame stride > H x pitch)"""
    L = _L()
    kind, r = _rho(rou)
    (_, xb), (_, yb), (gbig, gb) = _box(dev, x), _box(dev, y), _box(dev, x, fill=False)
    d = LS.desc_of(c, variant)
    d.x_sc, d.x_st, d.x_sr = xb.stride(0), xb.stride(1), xb.stride(2)
    d.y_sc, d.y_st, d.y_sr = yb.stride(0), yb.stride(1), yb.stride(2)
    assert d.x_sr > d.W and d.x_st > d.H * d.x_sr and gb.stride(2) > d.W and gb.stride(1) > d.H * gb.stride(2)
    acc = torch.full((1,), SENTINEL, dtype=torch.float64, device=dev)
    _ok(L.lib().vl3d_vote_fold_robust_strided(d, L.ptr(yb), L.ptr(nn), L.ptr(xb), kind, r, float(scaling), None, None, L.ptr(gb), gb.stride(0),
                                              gb.stride(1), gb.stride(2), L.ptr(acc), L.stream_ptr(dev)), "vl3d_vote_fold_robust_strided")
    outside = torch.ones_like(gbig, dtype=torch.bool)
    outside[:, 1:1 + d.Tx, 2:2 + d.H, 3:3 + d.W] = False
    assert bool((gbig[outside] == SENTINEL).all()), "the strided entry wrote outside its box"
    assert bool(torch.isfinite(gb).all()) and not bool((gb == SENTINEL).all())
    return gb.contiguous(), float(acc) / gb.numel()


def _check_loss(rep, name, got, st, shape):
    c = st.case
    fw, fh, nt = LS.FOLD_SHAPES[shape]
    B = st.loss_bound(LS.frames_per_thread(c, shape), nt // 64) + (LS.RHO_ULPS * LS.ULP * float(st.l64[0].abs().mean()) if _general(c.rou) else 0.0)
    ref = float(st.l64[1])
    print(f"[{rep.tag}] {name}: B_loss {B:.3e} measured {abs(got - ref):.3e} (x{abs(got - ref) / B if B else 0:.2f}), statement {ref:.6e}, "
          f"oracle fp32 off by {abs(float(st.l32[1]) - ref):.3e}")
    if not (np.isfinite(got) and abs(got - ref) <= B):
        rep.bad.append((name, got, ref, B))


def _run_case(dev, c, rows=None):
    """every row of the case's configuration at every entry"""
    from videoloop3d_amd import utils_vid as UV
    st = LS.statement(c)
    y, x, nn = st.y.to(dev), st.x.to(dev), st.nn.to(torch.int32).to(dev).contiguous()
    gulps = LS.GRAD_ULPS + (LS.RHO_ULPS if _general(c.rou) else 0)
    ran = set()
    for shape, nb, variant in (LS.rows(c.config) if rows is None else rows):
        desc = LS.desc_of(c, variant)
        for fused in (False, True):      # the intended instantiation is what runs
            rc, ch = UV.fold_choice(desc, fused)
            assert rc == 0 and (ch.staged, ch.shape, ch.nb, (ch.fw, ch.fh, ch.threads)) == (1, shape, nb, LS.FOLD_SHAPES[shape]), (c, shape, nb)
        rep = LS.Report(f"{c.config} Tx {c.Tx} Ty {c.Ty} {c.pattern} | shape {shape} nb {nb} | rou {c.rou} s {c.scaling}")
        s0, w0 = _fold(dev, desc, y, nn, 0)
        s1, w1 = _fold(dev, desc, y, nn, 1)
        rep.check("sum", s0, st.f64[0], st.f32[0])
        rep.check("y2x", s1, st.f64[2], st.f32[2], LS.Y2X_ULPS)
        rep.exact("weight", w0, st.f64[1])
        rep.exact("weight (normalized)", w1, st.f64[1])
        fy, fw_, g_a, loss_a = _fused(dev, desc, y, nn, x, c.rou, c.scaling, True)
        _, _, g_b, loss_b = _fused(dev, desc, y, nn, x, c.rou, c.scaling, False)
        g_c, loss_c = _strided(dev, c, variant, y, nn, x, c.rou, c.scaling)
        assert torch.equal(fy, s1) and torch.equal(fw_, w1), (rep.tag, "the fused y2x / weight are not the plain fold's bits")
        for name, g, ls in (("fused, y2x and weight written", g_a, loss_a), ("fused", g_b, loss_b), ("fused, strided boxes", g_c, loss_c)):
            rep.check(f"gradient ({name})", g, st.l64[2], st.l32[2], gulps, st.grad_sel)
            _check_loss(rep, f"loss ({name})", ls, st, shape)
        rep.done()
        ran.add((shape, nb))
    if rows is None:      # the unstaged kernel: the plain entry, variant 1
        desc = LS.desc_of(c, 1)
        rc, ch = UV.fold_choice(desc, False)
        assert rc == 0 and (ch.staged, ch.shape, ch.threads) == (0, -1, 256)
        rep = LS.Report(f"{c.config} Tx {c.Tx} Ty {c.Ty} {c.pattern} | unstaged")
        s0, w0 = _fold(dev, desc, y, nn, 0)
        s1, w1 = _fold(dev, desc, y, nn, 1)
        rep.check("sum", s0, st.f64[0], st.f32[0])
        rep.check("y2x", s1, st.f64[2], st.f32[2], 0)      # (vote_fold_k divides)
        rep.exact("weight", w0, st.f64[1])
        rep.exact("weight (normalized)", w1, st.f64[1])
        rep.done()
        ran.add("unstaged")
    return ran


# ---- the fold and the fused loss: every configuration x Tx x pattern, every row of the launch table ----------------------------------------------------
@pytest.mark.parametrize("config", list(LS.CONFIGS))
def test_fold_rows_on_chosen_indices(dev, config):
    """20 cases (every Tx with every index pattern, Ty and rho cycling) x every fold_shapes row at the natural covering form and at nb 0, and the
    unstaged kernel; entries: vl3d_vote_fold (normalize 0 / 1), vl3d_vote_fold_robust with y2x / weight written and with both NULL, and the
    strided entry on boxes inside sentinel-filled buffers"""
    want = {(s_, n_) for s_, n_, _ in LS.rows(config)} | {"unstaged"}
    for c in LS.cases(config):
        assert _run_case(dev, c) == want
    assert len(want) == (11 if LS.CONFIGS[config][6] else 6)


def test_every_staged_row_and_the_unstaged_kernel_ran(dev):
    """the 15 (shape, nb) instantiations between three configurations' rows, each asserted through fold_choice before its call"""
    ran = set()
    for config, k in (("nb3_ps7_s3", 13), ("nb2_ps4_s4", 8), ("fm_ps3_s2_pt3_st2", 18)):
        ran |= _run_case(dev, LS.cases(config)[k])
    assert ran == {(i, nb) for i in range(5) for nb in (0, 2, 3)} | {"unstaged"}


@pytest.mark.parametrize("rou,scaling", LS.RHOS)
def test_fused_robust_loss_every_rho(dev, rou, scaling):
    """rou x scaling on the fused kernel, on the patch-major NB 2 / NB 3 / dynamic forms and a frame-major one (Tx 13, random indices): planted exact
    zeros, +-1 ulp residuals (u rounds to 1), residuals over the clips' whole range"""
    for config in ("nb3_ps11_s4", "nb2_ps3_s2", "dyn_ps5_s1", "fm_ps4_s4_pt2_st2"):
        pt, stt = LS.CONFIGS[config][2:4]
        c = LS.Case(config, LS.on_grid(13, pt, stt), LS.on_grid(7, pt, stt), "random", rou, scaling)
        _run_case(dev, c, rows=LS.rows(config)[:2])


@pytest.mark.parametrize("rou,scaling", LS.RHOS)
def test_robust_kernels_alone(dev, rou, scaling):
    """vl3d_robust_fwd / _bwd at n = 4096 x 256 + 257 (the grid-stride loop, a ragged tail) and n = 1, upstream gradient 0.37.  The single element
    takes its bounds from the long run of the same rho (one element's own fp32 noise may be 0 by luck): B_rho as it is, the gradient's times n"""
    L = _L()
    kind, r = _rho(rou)
    g32 = np.float32(LS.GOUT)
    n_big = LS.ROBUST_N[0]
    _, _, planted_big, b64, b32 = LS.robust_statement(n_big, rou, scaling)
    sel_big = ((b64[3].abs() > LS.ABS_GAP) | planted_big) if rou == "abs" else None
    B_rho = LS.M_EXACT * LS.noise(b32[0], b64[0])
    B_grad_big = LS.M_EXACT * LS.noise(b32[2] * g32, b64[2] * float(g32), sel_big)      # (of gradients scaled by 1 / n_big)
    for n in LS.ROBUST_N:
        x, y2x, planted, l64, l32 = LS.robust_statement(n, rou, scaling)
        rep = LS.Report(f"robust n {n} rou {rou} s {scaling}")
        xd, yd = x.to(dev), y2x.to(dev)
        acc = torch.full((1,), SENTINEL, dtype=torch.float64, device=dev)
        _ok(L.lib().vl3d_robust_fwd(n, L.ptr(xd), L.ptr(yd), kind, r, float(scaling), L.ptr(acc), L.stream_ptr(dev)), "vl3d_robust_fwd")
        per_thread = -(-n // (min(-(-n // 256), 4096) * 256))
        B = B_rho + LS.ULP * float(l64[0].abs().mean()) * (per_thread + 6 + 4)
        got, ref = float(acc) / n, float(l64[1])
        print(f"[{rep.tag}] loss: B_loss {B:.3e} measured {abs(got - ref):.3e}, statement {ref:.6e}, oracle fp32 off by {abs(float(l32[1]) - ref):.3e}")
        assert np.isfinite(got) and abs(got - ref) <= B
        gout = torch.tensor([LS.GOUT], dtype=torch.float32, device=dev)
        gx = torch.full((n,), SENTINEL, dtype=torch.float32, device=dev)
        _ok(L.lib().vl3d_robust_bwd(n, L.ptr(xd), L.ptr(yd), kind, r, float(scaling), L.ptr(gout), 1.0 / n, L.ptr(gx), L.stream_ptr(dev)), "vl3d_robust_bwd")
        sel = ((l64[3].abs() > LS.ABS_GAP) | planted) if rou == "abs" else None
        # (n == 1: one element's noise may be 0 by luck -- the bound is the long run's, the same rho over the same range of residuals, times n_big / n)
        rep.check("gradient", gx, l64[2] * float(g32), l32[2] * g32, LS.BWD_ULPS, sel, B=B_grad_big * n_big / n)
        if rou == "abs":
            assert bool((gx.cpu()[planted] == 0).all())
        rep.done()


# ---- the prologue ------------------------------------------------------------------------------------------------------------------------------------------
def _prologue_case(dev, T, pad, h, w, gain, crop, gram_only=False):
    L = _L()
    rgb, res, g_x, p64, p32, t64, t32 = LS.prologue_statement(T, pad, h, w, gain, crop)
    rep = LS.Report(f"prologue T {T} pad {pad} {h}x{w} gain {'on' if gain else 'off'}" + (" res crop" if crop else ""))
    rgbd = rgb.to(dev)
    log_sum = None
    if gain:
        log_sum = torch.full((1,), SENTINEL, dtype=torch.float64, device=dev)
        if crop:
            resd = synth_like(dev, res)
            assert resd.stride(2) > w and resd.stride(1) > h * resd.stride(2) and not resd.is_contiguous()
            _ok(L.lib().vl3d_loop_gain_strided(T, res.shape[0], h, w, L.ptr(rgbd), L.ptr(resd), resd.stride(0), resd.stride(1), resd.stride(2),
                                               L.ptr(log_sum), L.stream_ptr(dev)), "vl3d_loop_gain_strided")
        else:
            resd = res.to(dev).contiguous()
            _ok(L.lib().vl3d_loop_gain(T, res.shape[0], h, w, L.ptr(rgbd), L.ptr(resd), L.ptr(log_sum), L.stream_ptr(dev)), "vl3d_loop_gain")
        B = LS.log_sum_bound(t64, t32)
        got, ref = float(log_sum), float(p64["log_sum"])
        off32 = abs(float(p32["log_sum"]) - ref)
        print(f"[{rep.tag}] log_sum: B {B:.3e} measured {abs(got - ref):.3e} (x{abs(got - ref) / B:.2f}), statement {ref:.6e}, oracle fp32 off by "
              f"{off32:.3e} (measured is {abs(got - ref) / (LS.M_EXACT * off32) if off32 else float('inf'):.2f} of 16 x that one scalar's noise)")
        if not (np.isfinite(got) and abs(got - ref) <= B):
            rep.bad.append(("log_sum", got, ref, B))
    F = T + pad
    x = torch.full((3, F, h, w), SENTINEL, dtype=torch.float32, device=dev)
    _ok(L.lib().vl3d_loop_pad_fwd(T, pad, h, w, L.ptr(rgbd), L.ptr(log_sum), L.ptr(x), L.stream_ptr(dev)), "vl3d_loop_pad_fwd")
    rep.check("x", x, p64["x"], p32["x"])
    xg = torch.full((int(L.lib().vl3d_gram_major_bytes(F, h, w)) // 4,), SENTINEL, dtype=torch.float32, device=dev)
    x2 = torch.full_like(x, SENTINEL)
    _ok(L.lib().vl3d_loop_pad_fwd_gram(T, pad, h, w, L.ptr(rgbd), L.ptr(log_sum), L.ptr(x2), L.ptr(xg), L.stream_ptr(dev)), "vl3d_loop_pad_fwd_gram")
    assert torch.equal(x, x2), (rep.tag, "vl3d_loop_pad_fwd_gram does not write vl3d_loop_pad_fwd's bits")
    if not gram_only:
        # g_x contiguous, and with the channel / frame strides of a larger buffer
        gxd = g_x.to(dev)
        big = torch.full((3, F + 2, h * w + 5), SENTINEL, dtype=torch.float32, device=dev)
        view = big[:, 1:1 + F, :h * w]
        view.copy_(gxd.reshape(3, F, h * w))
        outs = []
        for src, sc, st_ in ((gxd, F * h * w, h * w), (view, view.stride(0), view.stride(1))):
            g = torch.full((T, h, w, 3), SENTINEL, dtype=torch.float32, device=dev)
            _ok(L.lib().vl3d_loop_pad_bwd(T, pad, h, w, L.ptr(src), sc, st_, L.ptr(log_sum), L.ptr(g), L.stream_ptr(dev)), "vl3d_loop_pad_bwd")
            outs.append(g)
        rep.check("g_rgb", outs[0], p64["g_rgb"], p32["g_rgb"])
        assert torch.equal(outs[0], outs[1]), (rep.tag, "strided g_x gives other bits")
    rep.done()


def synth_like(dev, view):
    """a CPU view (a crop of a larger clip) rebuilt on the device with the same strides"""
    base = view._base if view._base is not None else view
    return torch.as_strided(base.to(dev), view.shape, view.stride(), view.storage_offset())


@pytest.mark.parametrize("T", LS.PRO_T)
def test_prologue_kernels(dev, T):
    """T in {1, 2, 5, 17} x pad in {0, 1, 2, T} x (3 x 64, 5 x 67) x gain on (res contiguous / a crop of a larger clip) and off: log_sum, x from both
    forward kernels (same bits), g_rgb for a hash g_x given contiguous and through channel / frame strides"""
    for t, pad, h, w in [p for p in LS.prologue_cases() if p[0] == T]:
        for gain, crop in ((True, False), (True, True), (False, False)):
            _prologue_case(dev, t, pad, h, w, gain, crop)


@pytest.mark.parametrize("T,pad", LS.GRAM_TP)
def test_prologue_gram_form_around_a_multiple_of_16_frames(dev, T, pad):
    """T + pad in {15, 16, 17}: the gram kernel's groups of 16 frames, last group short by one, full, and a group of one"""
    for h, w in LS.PRO_SIZES:
        _prologue_case(dev, T, pad, h, w, True, True, gram_only=True)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_a_status_and_launch_nothing(dev):
    L = _L()
    lib = L.lib()
    c = LS.Case("nb2_ps3_s2", 6, 7, "ramp", "-2", 0.1)
    st = LS.statement(c)
    desc = LS.desc_of(c)
    y, x, nn = st.y.to(dev), st.x.to(dev), st.nn.to(torch.int32).to(dev).contiguous()
    outs = [torch.full((3, c.Tx, desc.H, desc.W), SENTINEL, dtype=torch.float32, device=dev) for _ in range(3)]
    y2x, w, gx = outs
    acc = torch.full((1,), SENTINEL, dtype=torch.float64, device=dev)
    s, P = L.stream_ptr(dev), L.ptr

    def refused(rc, word):
        msg = lib.vl3d_last_error()
        assert rc != 0 and msg and word in msg.decode(), (rc, msg, word)

    fs = desc.H * desc.W
    refused(lib.vl3d_vote_fold_robust(desc, P(y), P(nn), P(x), 2, -2.0, 0.1, P(y2x), None, P(gx), P(acc), s), "together")
    refused(lib.vl3d_vote_fold_robust(desc, P(y), P(nn), P(x), 2, -2.0, 0.1, None, P(w), P(gx), P(acc), s), "together")
    refused(lib.vl3d_vote_fold_robust(desc, P(y), P(nn), P(x), 3, -2.0, 0.1, None, None, P(gx), P(acc), s), "rho kind")
    refused(lib.vl3d_vote_fold_robust(desc, P(y), P(nn), P(x), 2, -2.0, 0.0, None, None, P(gx), P(acc), s), "scale")
    refused(lib.vl3d_vote_fold_robust_strided(desc, P(y), P(nn), P(x), 2, -2.0, 0.1, None, None, P(gx), fs * c.Tx, fs, desc.W - 1, P(acc), s), "strides")
    for args in ((None, P(nn), P(x), P(gx), P(acc)), (P(y), None, P(x), P(gx), P(acc)), (P(y), P(nn), None, P(gx), P(acc)), (P(y), P(nn), P(x), None, P(acc)),
                 (P(y), P(nn), P(x), P(gx), None)):
        refused(lib.vl3d_vote_fold_robust(desc, args[0], args[1], args[2], 2, -2.0, 0.1, None, None, args[3], args[4], s), "null pointer")
    refused(lib.vl3d_vote_fold_robust(None, P(y), P(nn), P(x), 2, -2.0, 0.1, None, None, P(gx), P(acc), s), "null")
    for args in ((None, P(nn), P(y2x), P(w)), (P(y), None, P(y2x), P(w)), (P(y), P(nn), None, P(w)), (P(y), P(nn), P(y2x), None)):
        refused(lib.vl3d_vote_fold(desc, args[0], args[1], args[2], args[3], 1, s), "null pointer")
    n = x.numel()
    gout = torch.ones(1, dtype=torch.float32, device=dev)
    refused(lib.vl3d_robust_fwd(n, None, P(x), 2, -2.0, 0.1, P(acc), s), "bad arguments")
    refused(lib.vl3d_robust_fwd(0, P(x), P(x), 2, -2.0, 0.1, P(acc), s), "bad arguments")
    refused(lib.vl3d_robust_fwd(n, P(x), P(x), 3, -2.0, 0.1, P(acc), s), "rho kind")
    refused(lib.vl3d_robust_fwd(n, P(x), P(x), 2, -2.0, 0.0, P(acc), s), "scale")
    refused(lib.vl3d_robust_bwd(n, P(x), P(x), 2, -2.0, 0.1, None, 1.0 / n, P(gx), s), "bad arguments")
    refused(lib.vl3d_robust_bwd(n, P(x), P(x), 3, -2.0, 0.1, P(gout), 1.0 / n, P(gx), s), "rho kind")
    refused(lib.vl3d_robust_bwd(n, P(x), P(x), 2, -2.0, 0.0, P(gout), 1.0 / n, P(gx), s), "scale")
    # the prologue: pad > T, NULL pointers
    T, h, wd = 2, 3, 64
    rgb = torch.rand((T, h, wd, 3), device=dev)
    xo = torch.full((3, 2 * T + 1, h, wd), SENTINEL, dtype=torch.float32, device=dev)
    xg = torch.full((int(lib.vl3d_gram_major_bytes(2 * T + 1, h, wd)) // 4,), SENTINEL, dtype=torch.float32, device=dev)
    g_rgb = torch.full((T, h, wd, 3), SENTINEL, dtype=torch.float32, device=dev)
    refused(lib.vl3d_loop_pad_fwd(T, T + 1, h, wd, P(rgb), None, P(xo), s), "vl3d_loop_pad_fwd")
    refused(lib.vl3d_loop_pad_fwd_gram(T, T + 1, h, wd, P(rgb), None, P(xo), P(xg), s), "vl3d_loop_pad_fwd_gram")
    refused(lib.vl3d_loop_pad_bwd(T, T + 1, h, wd, P(xo), xo.stride(0), xo.stride(1), None, P(g_rgb), s), "vl3d_loop_pad_bwd")
    refused(lib.vl3d_loop_pad_fwd(T, -1, h, wd, P(rgb), None, P(xo), s), "vl3d_loop_pad_fwd")
    refused(lib.vl3d_loop_pad_fwd(T, 1, h, wd, None, None, P(xo), s), "vl3d_loop_pad_fwd")
    refused(lib.vl3d_loop_pad_fwd(T, 1, h, wd, P(rgb), None, None, s), "vl3d_loop_pad_fwd")
    refused(lib.vl3d_loop_pad_fwd_gram(T, 1, h, wd, P(rgb), None, P(xo), None, s), "vl3d_loop_pad_fwd_gram")
    refused(lib.vl3d_loop_pad_bwd(T, 1, h, wd, None, xo.stride(0), xo.stride(1), None, P(g_rgb), s), "vl3d_loop_pad_bwd")
    refused(lib.vl3d_loop_pad_bwd(T, 1, h, wd, P(xo), xo.stride(0), xo.stride(1), None, None, s), "vl3d_loop_pad_bwd")
    refused(lib.vl3d_loop_gain(T, 7, h, wd, None, P(rgb), P(acc), s), "vl3d_loop_gain")
    refused(lib.vl3d_loop_gain(T, 7, h, wd, P(rgb), None, P(acc), s), "vl3d_loop_gain")
    refused(lib.vl3d_loop_gain(T, 7, h, wd, P(rgb), P(rgb), None, s), "vl3d_loop_gain")
    refused(lib.vl3d_loop_gain(T, 0, h, wd, P(rgb), P(rgb), P(acc), s), "vl3d_loop_gain")
    torch.cuda.synchronize(dev)
    # nothing was launched: every output still holds the sentinel
    for t in outs + [acc, xo, xg, g_rgb]:
        assert bool((t == SENTINEL).all())
