"""The scalar head of a training iteration -- every kernel of csrc/vl3d_terms.hip (pixel_terms_k, stage1_gain_k, stage1_loss_k,
stage1_objective_gain_k, stage1_objective_k, linear_head_fwd_k / _bwd_k) and scale_inplace_k -- against the fp64 statement of
tests/terms_statement.py, through the C ABI with constructed tensors.  Bounds: per case and group of elements 16 max |oracle fp32 - oracle fp64|
plus the named ulp allowances of terms_statement's docstring; scalars under the derived chain bound; scale_inplace and the head's backward bit for
bit.  tests/test_terms_statement_cpu.py shows without a device that the statement is the reference's, that the case tables are what they claim and
what the comparison catches.  Every comparison prints its bound beside the measured maximum; the module prints one summary line per output at
the end (TABLE | ...)."""
import numpy as np
import pytest
import torch

import terms_statement as TS

pytestmark = pytest.mark.gpu
SENTINEL = TS.SENTINEL
PAD = 8          # sentinel floats on either side of every output


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    TS.Report.print_table()


def _L():
    from videoloop3d_amd import _lib as L
    return L


def _ok(rc, what):
    _L().check(rc, what)


def _on(dev, view):
    """a CPU tensor (possibly a crop of a larger one) rebuilt on the device with the same strides and the same sentinels around it"""
    base = view._base if view._base is not None else view
    return torch.as_strided(base.to(dev), view.shape, view.stride(), view.storage_offset())


class _Box:
    """an output of `n` elements inside a sentinel-filled buffer, PAD elements on either side"""

    def __init__(self, dev, n, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=dev)

    @property
    def view(self):
        return self.buf[PAD:PAD + self.n]

    @property
    def ptr(self):
        return _L().ptr(self.view)

    def refill(self):
        self.buf.fill_(SENTINEL)

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.n:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def _desc(st):
    L = _L()
    c = st.case
    B, h, w = c.shape
    return L.Stage1ObjectiveDesc(B, h, w, 1 if c.gain else 0, *[float(v) for v in c.weights], float(np.float32(1.0 / np.sqrt(c.mpi_d))), float(c.eps),
                                 (L.C.c_float * 4)(*st.x.coef))


class _ObjectiveCall:
    """the device side of one vl3d_stage1_objective case: inputs as the statement has them, every output in a sentinel box, absent ones NULL"""

    def __init__(self, dev, st):
        c, x = st.case, st.x
        self.st, self.dev, n = st, dev, c.n
        has_label, has_alpha, has_asum, has_smooth = c.has
        self.rgb = x.rgb.to(dev)
        self.label = x.label.to(dev) if has_label else None
        self.alpha = x.alpha.to(dev) if has_alpha else None
        self.asum = x.asum.to(dev) if has_asum else None
        self.smooth = x.smooth.to(dev) if has_smooth else None
        self.target = _on(dev, x.target)
        self.tmask = _on(dev, x.tmask) if has_label else None
        assert self.target.stride() == x.target.stride() and (self.tmask is None or self.tmask.stride() == x.tmask.stride())
        self.scratch = _Box(dev, 6, torch.float64)
        self.out = _Box(dev, 8)
        self.g_rgb = _Box(dev, 3 * n)
        self.g_label = _Box(dev, n) if has_label else None
        self.g_alpha = _Box(dev, n) if has_alpha else None
        self.g_asum = _Box(dev, 2 * n) if has_asum else None
        self.g_smooth = _Box(dev, 4) if has_smooth else None
        self.boxes = [b for b in (self.scratch, self.out, self.g_rgb, self.g_label, self.g_alpha, self.g_asum, self.g_smooth) if b is not None]

    def run(self):
        L = _L()
        P = L.ptr
        bp = lambda b: None if b is None else b.ptr      # noqa: E731
        t, m = self.target, self.tmask
        d = _desc(self.st)
        return L.lib().vl3d_stage1_objective(L.C.byref(d), P(self.rgb), P(self.label), P(self.alpha), P(self.asum), P(self.smooth), P(t), t.stride(0), t.stride(1),
                                             t.stride(2), P(m), 0 if m is None else m.stride(0), 0 if m is None else m.stride(1), self.scratch.ptr, self.out.ptr,
                                             self.g_rgb.ptr, bp(self.g_label), bp(self.g_alpha), bp(self.g_asum), bp(self.g_smooth), L.stream_ptr(self.dev))

    def check(self, rep):
        c = self.st.case
        B, h, w = c.shape
        assert all(b.intact() for b in self.boxes), (rep.tag, "an entry wrote outside an output")
        v = lambda b, shape: None if b is None else b.view.cpu().reshape(shape)      # noqa: E731
        TS.check_objective(rep, self.st, self.out.view.cpu(), v(self.g_rgb, (B, h, w, 3)), v(self.g_label, (B, h, w)), v(self.g_alpha, (B, h, w)),
                           v(self.g_asum, (B, h, w, 2)), v(self.g_smooth, (4,)), float(self.scratch.view[0]) if c.gain else None)


def _objective_case(dev, c):
    st = TS.statement(c)
    call = _ObjectiveCall(dev, st)
    rep = TS.Report(f"objective {c.shape} {c.layout} {c.subset} gain {'on' if c.gain else 'off'} w {c.weights} eps {c.eps:g} D {c.mpi_d}", entry="vl3d_stage1_objective")
    _ok(call.run(), "vl3d_stage1_objective")
    call.check(rep)
    first = call.out.view.clone()
    # the ticket (scratch[5]) does not carry over: a second call on the same scratch writes `out` again
    for b in call.boxes[1:]:
        b.refill()
    _ok(call.run(), "vl3d_stage1_objective")
    again = TS.Report(rep.tag + " | second call on one scratch", quiet=True)
    call.check(again)
    if c.n <= 256:          # one workgroup: one order of the adds
        assert torch.equal(first, call.out.view), (rep.tag, "a second call on the same scratch gives another out")
    rep.done()
    again.done()          # several workgroups: the order of the double atomics is free, so the second call is held to the same bounds


# ---- vl3d_stage1_objective ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TS.SHAPES)
def test_stage1_objective(dev, shape):
    """12 cases per shape: contiguous targets and crops of sentinel-filled stills x {all terms, no label, no alpha, no alpha_sums, no smoothness sums,
    rgb only}; gain, weights (a zero, no powers of two), eps 1e-6 / 1e-4 and mpi_d cycle.  Absent inputs' gradient buffers are NULL, present ones
    sit inside sentinels; each case is called twice on one scratch"""
    for c in TS.cases(shape):
        _objective_case(dev, c)


def test_stage1_objective_second_grid_trip(dev):
    """(2, 513, 1025): 1 051 650 pixels, 4096 workgroups and tickets, a ragged second trip of 3074 pixels; every term, gain, crops"""
    _objective_case(dev, TS.BIG_CASE)


# ---- vl3d_stage1_loss ------------------------------------------------------------------------------------------------------------------------------------------
def _loss_case(dev, shape, C, gain, layout):
    L = _L()
    st = TS.statement(TS.loss_case(shape, C, gain), unit=True)
    x = st.x
    B, h, w = shape
    base = (torch.cat([x.rgb, x.label[..., None]], -1) if C == 4 else x.rgb).contiguous().to(dev)
    r = base.permute(0, 3, 1, 2)
    if layout == "nchw":
        r = r.contiguous()
    assert r.stride(3) * w == r.stride(2)
    t, m = x.target.to(dev), (x.tmask.to(dev) if C == 4 else None)
    assert t.is_contiguous()
    sums, log_sum, grad = _Box(dev, 2, torch.float64), _Box(dev, 1, torch.float64), _Box(dev, B * h * w * C)
    rep = TS.Report(f"stage1_loss {shape} C {C} gain {'on' if gain else 'off'} {layout}", entry="vl3d_stage1_loss")
    _ok(L.lib().vl3d_stage1_loss(B, C, h, w, L.ptr(r), r.stride(0), r.stride(1), r.stride(3), L.ptr(t), L.ptr(m), 1 if gain else 0, log_sum.ptr if gain else None,
                                 sums.ptr, grad.ptr, L.stream_ptr(dev)), "vl3d_stage1_loss")
    assert sums.intact() and grad.intact() and (log_sum.intact() if gain else log_sum.untouched())
    TS.check_stage1_loss(rep, st, C, [float(v) for v in sums.view], grad.view.cpu().reshape(B, h, w, C), float(log_sum.view[0]) if gain else None)
    rep.done()


@pytest.mark.parametrize("shape", TS.SHAPES)
def test_stage1_loss(dev, shape):
    """C = 3 | 4 x gain on / off x the NHWC-backed NCHW view MPMesh.forward returns and a plain NCHW tensor: both double sums, the log-ratio sum,
    the gradient (unit upstream, counts not folded in) with the label's inside and outside the clamp held apart"""
    for C in (3, 4):
        for gain in (True, False):
            for layout in ("nhwc", "nchw"):
                _loss_case(dev, shape, C, gain, layout)


def test_stage1_loss_second_grid_trip(dev):
    _loss_case(dev, TS.BIG, 4, True, "nhwc")


# ---- vl3d_pixel_terms ------------------------------------------------------------------------------------------------------------------------------------------
def _terms_case(dev, shape, which, eps):
    L = _L()
    st = TS.statement(TS.terms_case(shape, which, eps), unit=True)
    x, n = st.x, st.case.n
    _, has_alpha, has_asum, _ = st.case.has
    a, s = (x.alpha.to(dev) if has_alpha else None), (x.asum.to(dev) if has_asum else None)
    sums, ga, gs = _Box(dev, 2, torch.float64), (_Box(dev, n) if has_alpha else None), (_Box(dev, 2 * n) if has_asum else None)
    bp = lambda b: None if b is None else b.ptr      # noqa: E731
    rep = TS.Report(f"pixel_terms {shape} {which} eps {eps:g}", entry="vl3d_pixel_terms")
    _ok(L.lib().vl3d_pixel_terms(n, L.ptr(a), L.ptr(s), float(eps), sums.ptr, bp(gs), bp(ga), L.stream_ptr(dev)), "vl3d_pixel_terms")
    assert sums.intact() and all(b.intact() for b in (ga, gs) if b is not None)
    TS.check_pixel_terms(rep, st, [float(v) for v in sums.view], None if gs is None else gs.view.cpu().reshape(x.asum.shape),
                         None if ga is None else ga.view.cpu().reshape(x.alpha.shape))
    if n <= 256:          # without gradient buffers: the same sums (one workgroup: the same bits)
        first = sums.view.clone()
        _ok(L.lib().vl3d_pixel_terms(n, L.ptr(a), L.ptr(s), float(eps), sums.ptr, None, None, L.stream_ptr(dev)), "vl3d_pixel_terms")
        assert torch.equal(first, sums.view)
    rep.done()


@pytest.mark.parametrize("shape", TS.SHAPES)
def test_pixel_terms(dev, shape):
    """both inputs, alpha_sums alone, alpha alone x eps 1e-6 / 1e-4: the double sums and the unit gradients, uncovered / floor-side / just above the floor /
    ordinary pixels held apart"""
    for which in ("both", "sparsity", "density"):
        for eps in TS.EPS:
            _terms_case(dev, shape, which, eps)


def test_pixel_terms_second_grid_trip(dev):
    _terms_case(dev, TS.BIG, "both", TS.EPS[0])


# ---- vl3d_scale_inplace ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TS.SCALE_N)
def test_scale_inplace_is_the_fp32_product(dev, n):
    """n = 4, 4 x 257 and 4 x (8192 x 256 + 257) (a second trip of the grid-stride loop): scale 1.0 leaves every bit, planted NaN payloads
    included; 2.5 and -0.37 give the fp32 product bit for bit; the sentinels behind the end stay"""
    L = _L()
    x = TS.synth.hash_uniform((n,), seed=77) * 4 - 2
    for scale in TS.SCALES:
        xi = x.clone()
        if scale == 1.0:      # NaNs with payloads, infinities, denormals, -0
            words = np.array([0x7FC12345, 0xFFC12345, 0x7F800000, 0x00000001, 0x80000000][:min(5, n)], dtype=np.uint32)
            bits = torch.from_numpy(words.view(np.int32).copy())
            xi.view(torch.int32)[torch.arange(bits.numel()) * (n // bits.numel())] = bits
        box = _Box(dev, n)
        box.view.copy_(xi)
        s = torch.tensor([scale], dtype=torch.float32, device=dev)
        _ok(L.lib().vl3d_scale_inplace(n, box.ptr, L.ptr(s), L.stream_ptr(dev)), "vl3d_scale_inplace")
        want = xi if scale == 1.0 else xi * np.float32(scale)
        assert torch.equal(box.view.cpu().view(torch.int32), want.view(torch.int32)), (n, scale)
        assert box.intact()


# ---- vl3d_linear_head_fwd / _bwd -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", TS.HEAD_N)
def test_linear_head(dev, n):
    """n in {1, 2, 7, 16} x ngroups in {1, 3, 16}: out[0] and the groups' shares against the fp64 chain under 2^-24 sum |coef v| (1 + n); group id
    15 in term 15's nibble (the top one of the 64-bit word); grad_terms bit for bit coef * g"""
    L = _L()
    for ng in TS.HEAD_NGROUPS:
        v, coef, groups = TS.head_inputs(n, ng)
        vd, cd = v.to(dev), coef.to(dev)
        out = _Box(dev, 1 + ng)
        _ok(L.lib().vl3d_linear_head_fwd(n, TS.groups_word(groups), ng, L.ptr(vd), L.ptr(vd[1:]) if n > 1 else None, L.ptr(cd), out.ptr, L.stream_ptr(dev)),
            "vl3d_linear_head_fwd")
        assert out.intact()
        total, share = TS.head(v, coef, groups, ng, torch.float64)
        rep = TS.Report(f"linear_head n {n} ngroups {ng}", entry="vl3d_linear_head_fwd")
        got = out.view.cpu()
        rep.scalar("out[0] total", got[0], total, TS.head_bound(v, coef))
        for g in range(ng):
            members = torch.tensor(groups) == g
            rep.scalar("out[1 + g] group shares", got[1 + g], share[g], TS.head_bound(v, coef, members))
        gt = _Box(dev, n)
        gout = torch.tensor([0.37], dtype=torch.float32, device=dev)
        _ok(L.lib().vl3d_linear_head_bwd(n, L.ptr(cd), L.ptr(gout), gt.ptr, L.stream_ptr(dev)), "vl3d_linear_head_bwd")
        assert gt.intact() and torch.equal(gt.view.cpu(), coef * np.float32(0.37)), (n, ng)
        rep.done()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_a_status_and_launch_nothing(dev):
    L = _L()
    lib, P, s = L.lib(), L.ptr, L.stream_ptr(dev)

    def refused(rc, word):
        msg = lib.vl3d_last_error()
        assert rc != 0 and msg and word in msg.decode(), (rc, msg, word)

    shape = TS.SHAPES[3]
    B, h, w = shape
    n = B * h * w
    st = TS.statement(TS.cases(shape)[0])
    assert st.case.subset == "all"
    call = _ObjectiveCall(dev, st)
    x = st.x
    a, asum = x.alpha.to(dev), x.asum.to(dev)
    sums, ga, gs = _Box(dev, 2, torch.float64), _Box(dev, n), _Box(dev, 2 * n)
    # vl3d_pixel_terms
    refused(lib.vl3d_pixel_terms(0, P(a), P(asum), 1e-6, sums.ptr, gs.ptr, ga.ptr, s), "bad arguments")
    refused(lib.vl3d_pixel_terms(-n, P(a), P(asum), 1e-6, sums.ptr, gs.ptr, ga.ptr, s), "bad arguments")
    refused(lib.vl3d_pixel_terms(n, P(a), P(asum), 1e-6, None, gs.ptr, ga.ptr, s), "bad arguments")
    refused(lib.vl3d_pixel_terms(n, None, None, 1e-6, sums.ptr, None, None, s), "bad arguments")
    refused(lib.vl3d_pixel_terms(n, None, P(asum), 1e-6, sums.ptr, gs.ptr, ga.ptr, s), "without its input")
    refused(lib.vl3d_pixel_terms(n, P(a), None, 1e-6, sums.ptr, gs.ptr, ga.ptr, s), "without its input")
    # vl3d_stage1_loss
    r4 = torch.cat([x.rgb, x.label[..., None]], -1).to(dev).permute(0, 3, 1, 2)
    t, m = x.target.contiguous().to(dev), x.tmask.contiguous().to(dev)
    log_sum, grad = _Box(dev, 1, torch.float64), _Box(dev, n * 5)
    args = lambda B_=B, C=4, h_=h, r=r4, t_=t, m_=m, si=1, ls=log_sum.ptr, su=sums.ptr, g=grad.ptr: lib.vl3d_stage1_loss(      # noqa: E731
        B_, C, h_, w, P(r), r4.stride(0), r4.stride(1), r4.stride(3), P(t_), P(m_), si, ls, su, g, s)
    refused(args(B_=0), "bad arguments")
    refused(args(h_=0), "bad arguments")
    refused(args(C=2), "bad arguments")
    refused(args(C=5), "bad arguments")
    refused(args(su=None), "bad arguments")
    refused(args(g=None), "bad arguments")
    refused(args(r=None), "bad arguments")
    refused(args(t_=None), "bad arguments")
    refused(args(m_=None), "needs its target")
    refused(args(ls=None), "log_sum")
    # vl3d_stage1_objective
    d = _desc(st)
    tg, tm = call.target, call.tmask

    def objective(desc=d, rgb=call.rgb, label=call.label, alpha=call.alpha, asum_=call.asum, smooth=call.smooth, target=tg, mask=tm, scratch=call.scratch.ptr,
                  out=call.out.ptr, g_rgb=call.g_rgb.ptr, g_label=call.g_label.ptr, g_alpha=call.g_alpha.ptr, g_asum=call.g_asum.ptr, g_smooth=call.g_smooth.ptr):
        return lib.vl3d_stage1_objective(None if desc is None else L.C.byref(desc), P(rgb), P(label), P(alpha), P(asum_), P(smooth), P(target), tg.stride(0), tg.stride(1),
                                         tg.stride(2), P(mask), tm.stride(0), tm.stride(1), scratch, out, g_rgb, g_label, g_alpha, g_asum, g_smooth, s)

    d0 = _desc(st)
    d0.B = 0
    refused(objective(desc=d0), "bad arguments")
    d0 = _desc(st)
    d0.w = -3
    refused(objective(desc=d0), "bad arguments")
    for kw in (dict(desc=None), dict(rgb=None), dict(target=None), dict(scratch=None), dict(out=None), dict(g_rgb=None)):
        refused(objective(**kw), "bad arguments")
    for kw in (dict(mask=None), dict(label=None), dict(g_label=None), dict(label=None, mask=None)):
        refused(objective(**kw), "comes with its target and its gradient buffer")
    for kw in (dict(alpha=None), dict(g_alpha=None), dict(asum_=None), dict(g_asum=None), dict(smooth=None), dict(g_smooth=None)):
        refused(objective(**kw), "every optional input comes with its gradient buffer")
    # vl3d_linear_head_fwd / _bwd
    v, coef, groups = TS.head_inputs(7, 3)
    vd, cd = v.to(dev), coef.to(dev)
    out, gt = _Box(dev, 17), _Box(dev, 16)
    word = TS.groups_word(groups)
    for n_, ng in ((0, 3), (17, 3), (7, 0), (7, 17), (-1, 3)):
        refused(lib.vl3d_linear_head_fwd(n_, word, ng, P(vd), P(vd[1:]), P(cd), out.ptr, s), "vl3d_linear_head_fwd")
    refused(lib.vl3d_linear_head_fwd(7, word, 3, P(vd), None, P(cd), out.ptr, s), "vl3d_linear_head_fwd")
    refused(lib.vl3d_linear_head_fwd(7, word, 3, None, P(vd[1:]), P(cd), out.ptr, s), "vl3d_linear_head_fwd")
    refused(lib.vl3d_linear_head_fwd(7, word, 3, P(vd), P(vd[1:]), None, out.ptr, s), "vl3d_linear_head_fwd")
    refused(lib.vl3d_linear_head_fwd(7, word, 3, P(vd), P(vd[1:]), P(cd), None, s), "vl3d_linear_head_fwd")
    for n_ in (0, 17):
        refused(lib.vl3d_linear_head_bwd(n_, P(cd), P(vd), gt.ptr, s), "vl3d_linear_head_bwd")
    refused(lib.vl3d_linear_head_bwd(7, P(cd), None, gt.ptr, s), "vl3d_linear_head_bwd")
    refused(lib.vl3d_linear_head_bwd(7, P(cd), P(vd), None, s), "vl3d_linear_head_bwd")
    # vl3d_scale_inplace
    xs = _Box(dev, 16)
    one = torch.tensor([2.5], dtype=torch.float32, device=dev)
    for n_ in (0, -4, 5, 6, 7):
        refused(lib.vl3d_scale_inplace(n_, xs.ptr, P(one), s), "vl3d_scale_inplace")
    refused(lib.vl3d_scale_inplace(16, None, P(one), s), "vl3d_scale_inplace")
    refused(lib.vl3d_scale_inplace(16, xs.ptr, None, s), "vl3d_scale_inplace")
    torch.cuda.synchronize(dev)
    # nothing was launched: every output still holds the sentinel
    for b in [sums, ga, gs, log_sum, grad, out, gt, xs] + call.boxes:
        assert b.untouched()
