"""The looping loss AFTER the search, stated against the CPU oracle in fp64 (oracle/vid_oracle.py; reference utils_vid.py:206-229, :10-26, :348 and
MPV.py:484-507), for tests/test_loss_statement_cpu.py (the statement is the reference's, conditions on the case tables, planted faults) and
tests/test_gpu_loss_fp64.py (vote_fold_k, every vote_fold_lds_k instantiation, the fused robust loss, robust_fwd_k / robust_bwd_k and the four
loop_*_k prologue kernels against it).  Plain torch on the CPU; of the product only synth and the descriptor helper (patchnn_rows.loss_desc) are
imported.  The search does not appear: the fold takes its indices as an INPUT, and here they are chosen, not searched.

The statement.
  fold(y, nn, ...)        gather + FoldNd of utils_vid.py:217-228 for GIVEN indices nn [h_o, w_o, n1]: the vote sum [3,Tx,H,W], the vote count clamped
                          at 1e-10, and y2x = sum / weight.  The adds run in the oracle's own order (kt, kh, kw ascending), so in fp32 and with the
                          oracle's own indices it IS VO.find_nn_and_merge bit for bit.
  loss(x, y2x, ...)       VO.robust_lossfun(x - y2x, rou, scaling) per element, its mean, d mean / d x by autograd.
  prologue(rgb, res, pad) MPV.py:484-507: gain (exp(mean log((mean_f res + .01) / (mean_t rgb + .01))) + 3) / 4, detached; x [3,T+pad,h,w]; for a given
                          g_x the gradient g_rgb [T,h,w,3] with the pad frames' share folded back (autograd through cat and the product).
Each in float64 on the widened fp32 inputs (the statement) and in float32 ("the oracle in fp32": the reference's own rounding noise).  `scaling`
is the fp32 value the ABI takes, widened; b, d and b / d of the Barron case are formed as the reference forms them.

The bound.  Per case and per output B = M_EXACT max |oracle fp32 - oracle fp64| over what is compared (M_EXACT = 16 is render_statement's: value
arithmetic alone, no coordinate rounds).  No floor.  The weight is compared EXACTLY.  tests/test_loss_statement_cpu.py shows every planted fault
at 4 B or more: that is the cap on the factor.

Roundings the kernels have and the oracle has not.  Where the oracle's fp32 noise is exactly 0 (one vote per voxel: sum, and sum / 1) B is 0 and the
kernels have to be exact there too -- they are: rcp(1) == 1, s * 1 == s.  Elsewhere each rounding below adds 2^-24 |v64| (v64: the statement's value
of that element) to the allowance of the output it enters; nothing is added that is not named here:
  y2x      Y2X_ULPS  = 2: v_rcp_f32(count), and the product s * rcp (the oracle has ONE quotient).  vote_fold_k divides: 0 there.
  rho      RHO_ULPS  = 2 (fused kernel, general Barron case only): host reciprocals inv_scale and inv_b in place of the two quotients.
  gradient GRAD_ULPS = 3 (fused kernel): gscale = 1 / (3 Tx H W) is a product of floats (one rounding of the product, one of the reciprocal) and
           multiplies rho' (one more), where autograd divides by the count once; + RHO_ULPS in the general case (inv_scale, inv_b again).
           robust_bwd_k: BWD_ULPS = 2 (inv_n = 1 / n arrives rounded to a float, and gout * inv_n is rounded before it multiplies rho').
  x, g_rgb, log_sum (prologue): none named -- the gain is held by B alone.
The scalar loss does not take its bound from one scalar's lucky noise (the fp32 mean lands anywhere between 1e-9 and 2e-7 relative):
  B_loss = mean(B_rho per element) + 2^-24 mean |rho64| (frames per thread + 6 shuffle steps + waves per workgroup),
the fp32 chain a kernel has before its double atomic; log_sum (a sum of 3 h w logs) likewise: 3 h w B_term + 2^-24 sum |term64| (2 + 6 + 3).
This log_sum bound is LOOSER than the per-output rule 16 |fp32 - fp64| of that one scalar, and deliberately not it: torch's pairwise fp32 sum of
~1000 logs lands 2e-7 to 5e-6 from the fp64 sum by luck of cancellation, while loop_gain_k adds terms of the hardware log (v_log_f32 x ln 2, an
absolute error near 1e-7 per term) in lane order -- measured up to 6e-5 off, several times 16 x the scalar's own noise (the GPU test prints that
ratio per case).  What log_sum is FOR is held at the per-output rule: it enters x and g_rgb as the gain, an error d of log_sum moves x by about
d / (4 x 3 h w), and x and g_rgb are compared at B = 16 x their own noise (about 1e-6) with nothing added.

rou = 'abs' has a sign kink at e = 0: its gradient is compared where |e64| > ABS_GAP = 1e-5 and at voxels planted with e == 0 exactly (gradient 0
on both sides); the share left out is a condition of the inputs (at most ABS_SHARE = 1 %, tests/test_loss_statement_cpu.py).

Planted residuals.  A voxel with exactly one vote has y2x == that y value on every side, whatever the order of the adds.  At those voxels x is set
to y2x + e for e cycling through PLANT: exact zeros, +-1 ulp (|e| down to 1e-9: (e / scale)^2 / b + 1 rounds to 1), and powers of two up to 2^-6;
everywhere else x - y2x runs over the clips' full range (-1, 1)."""
import dataclasses
import math

import numpy as np
import torch

import patchnn_rows as PR
from oracle import vid_oracle as VO
from render_statement import M_EXACT
from videoloop3d_amd import synth

ULP = 2.0 ** -24
ABS_GAP, ABS_SHARE = 1e-5, 0.01
Y2X_ULPS, RHO_ULPS, GRAD_ULPS, BWD_ULPS = 2, 2, 3, 2

# ---- the case tables of tests/test_gpu_loss_fp64.py -------------------------------------------------------------------------------------------------
# name -> (ps, stride, pt, stridet, H, W, natural nb): small frames on the patch grid wider than 64 (two 64-wide tiles, the second ragged; three
# 32-wide ones), rows no multiple of 4
CONFIGS = {
    "nb3_ps11_s4": (11, 4, 3, 1, 19, 75, 3),
    "nb3_ps7_s3": (7, 3, 3, 1, 13, 67, 3),
    "nb2_ps3_s2": (3, 2, 3, 1, 19, 75, 2),
    "nb2_ps4_s4": (4, 4, 3, 1, 12, 68, 2),          # one location per pixel
    "dyn_ps5_s1": (5, 1, 3, 1, 9, 69, 0),           # 5 x 5 covering locations: dynamic loops
    "fm_ps4_s4_pt2_st2": (4, 4, 2, 2, 12, 68, 0),   # frame-major forms
    "fm_ps3_s2_pt3_st2": (3, 2, 3, 2, 19, 75, 0),
    "fm_ps1": (1, 1, 1, 1, 9, 69, 0),
}
TX = (3, 6, 13, 53)          # n1 = 1 and empty groups | trailing empty groups at G = 8 | last group short | past the 12-deep x queue
TY = (3, 7, 20)              # n2 = 1 | .. | ..
PATTERNS = ("first", "last", "checker", "random", "ramp")
RHOS = [(rou, sc) for rou in ("mse", "abs", "0", "2", "-2", "1") for sc in (0.1, 0.2)]
FOLD_SHAPES = ((64, 2, 512), (32, 4, 512), (32, 2, 256), (64, 1, 256), (32, 1, 256))      # csrc/vl3d_patchnn_choice.h fold_shapes[], asserted via fold_choice
PLANT = (0.0, "+ulp", "-ulp", 2.0 ** -20, -2.0 ** -16, 0.0, 2.0 ** -12, -2.0 ** -6)


def on_grid(t, pt, st):
    """the size nearest to t that sits on the temporal patch grid"""
    return pt + max(0, int(math.floor((t - pt) / st + 0.5))) * st


@dataclasses.dataclass(frozen=True)
class Case:
    config: str
    Tx: int
    Ty: int
    pattern: str
    rou: str
    scaling: float

    @property
    def cfg(self):
        return CONFIGS[self.config]

    @property
    def grid(self):
        ps, s, pt, st, H, W, _ = self.cfg
        return (H - ps) // s + 1, (W - ps) // s + 1, (self.Tx - pt) // st + 1, (self.Ty - pt) // st + 1      # h_o, w_o, n1, n2


def cases(config):
    """20 cases per configuration: every Tx with every pattern; Ty and (rou, scaling) cycle so that each Tx meets each Ty and the 12 rho settings
    are spread over the table.  Tx and Ty of the strided-time configurations are the nearest sizes on their temporal grid"""
    ps, s, pt, st = CONFIGS[config][:4]
    k0 = 7 * list(CONFIGS).index(config)
    out = []
    for ti, tx in enumerate(TX):
        for pi, pat in enumerate(PATTERNS):
            rou, sc = RHOS[(k0 + 5 * ti + pi) % len(RHOS)]
            out.append(Case(config, on_grid(tx, pt, st), on_grid(TY[(ti + pi) % 3], pt, st), pat, rou, sc))
    return out


def rows(config):
    """the (shape, nb, variant) rows a configuration is run at: every fold_shapes row forced through bits 12-15, at the natural covering form and at
    nb 0 through bit 9"""
    nat = CONFIGS[config][6]
    out = []
    for i in range(len(FOLD_SHAPES)):
        out.append((i, nat, (i + 1) << 12))
        if nat:
            out.append((i, 0, (i + 1) << 12 | 0x200))
    return out


def desc_of(case, variant=0):
    ps, s, pt, st, H, W, _ = case.cfg
    return PR.loss_desc((case.Tx, case.Ty, H, W, ps, pt, s, st, None, variant))


def frames_per_thread(case, shape):
    fw, fh, nt = FOLD_SHAPES[shape]
    return -(-case.Tx // (nt // (fw * fh)))


def indices(case):
    """nn [h_o, w_o, n1] int64, every entry in [0, n2 - 1]"""
    h_o, w_o, n1, n2 = case.grid
    by, bx, i = torch.meshgrid(torch.arange(h_o), torch.arange(w_o), torch.arange(n1), indexing="ij")
    p = case.pattern
    if p == "first":
        return torch.zeros_like(by)
    if p == "last":
        return torch.full_like(by, n2 - 1)
    if p == "checker":
        return ((by + bx + i) % 2) * (n2 - 1)
    if p == "ramp":
        return (i + by + 2 * bx) % n2
    assert p == "random"
    u = synth.hash_uniform((h_o, w_o, n1), seed=1000 + 31 * case.Tx + case.Ty)
    return (u.double() * n2).long().clamp(max=n2 - 1)


# ---- the statement -----------------------------------------------------------------------------------------------------------------------------------
def fold(y, nn, ps, pt, s, st, Tx, dtype, src_frame=None):
    """y [3,Ty,H,W]; nn [h_o,w_o,n1] -> (sum [3,Tx,H,W], weight [Tx,H,W] clamped at 1e-10, y2x).  src_frame(kt) -> the y frame [h_o,w_o,n1] patch
    element kt is gathered from (default nn * st + kt; tests/test_loss_statement_cpu.py plants faults through it)"""
    y = y.detach().to(dtype)
    H, W = y.shape[-2:]
    nn = nn.long()
    h_o, w_o, n1 = nn.shape
    assert (h_o, w_o, n1) == ((H - ps) // s + 1, (W - ps) // s + 1, (Tx - pt) // st + 1)
    rows_, cols_ = torch.arange(h_o)[:, None, None] * s, torch.arange(w_o)[None, :, None] * s
    acc = torch.zeros((3, Tx, H, W), dtype=dtype)
    cnt = torch.zeros((Tx, H, W), dtype=dtype)
    for kt in range(pt):
        f = nn * st + kt if src_frame is None else src_frame(kt)
        for kh in range(ps):
            for kw in range(ps):
                v = y[:, f, rows_ + kh, cols_ + kw].permute(0, 3, 1, 2)                          # [3, n1, h_o, w_o]
                acc[:, kt:kt + st * n1:st, kh:kh + s * h_o:s, kw:kw + s * w_o:s] += v
                cnt[kt:kt + st * n1:st, kh:kh + s * h_o:s, kw:kw + s * w_o:s] += 1
    w = cnt.clamp_min(1e-10)
    return acc, w, acc / w


def rho_grad_general(e, rou, scale, exponent_shift=-1.0):
    """rho' of the general case in closed form, 10 (e / scale) (s / b + 1)^(d / 2 + shift): shift -1 is the derivative (checked against autograd in
    the CPU tests), shift 0 a planted fault"""
    rou = float(rou)
    b = abs(rou - 2) + 1e-6
    d = rou + 1e-6 if rou >= 0 else rou - 1e-6
    z = e / scale
    return 10.0 * z * torch.pow(z * z / b + 1.0, 0.5 * d + exponent_shift)


def loss(x, y2x, rou, scaling, dtype):
    """-> (rho per element, its mean, d mean / d x, e = x - y2x), detached"""
    sc = float(np.float32(scaling))
    xv = x.detach().to(dtype).requires_grad_(True)
    e = xv - y2x.detach().to(dtype)
    r = VO.robust_lossfun(e, rou, sc)
    m = r.mean()
    (g,) = torch.autograd.grad(m, xv)
    return r.detach(), m.detach(), g.detach(), e.detach()


def log_terms(rgb, res, dtype):
    """log((mean_f res + .01) / (mean_t rgb + .01)) [3,h,w] (MPV.py:500-502)"""
    r = rgb.detach().to(dtype).permute(0, 3, 1, 2)
    return torch.log((res.detach().to(dtype).mean(dim=0) + 0.01) / (r.mean(dim=0) + 0.01))


def prologue(rgb, res, pad, dtype, g_x=None, gain_frames=None):
    """rgb [T,h,w,3], res [F,3,h,w] or None -> dict(gain, log_sum, x [3,T+pad,h,w], g_rgb [T,h,w,3] for g_x [3,T+pad,h,w]).  MPV.py:484-507 line by
    line.  gain_frames: a planted fault (the gain's rgb mean over that many frames of the padded clip)"""
    leaf = rgb.detach().to(dtype).requires_grad_(True)
    r = leaf.permute(0, 3, 1, 2)
    rgb_pad = torch.cat([r, r[:pad]], 0)
    out = dict(gain=None, log_sum=None)
    if res is not None:
        res_avg = res.detach().to(dtype).mean(dim=0)
        rgb_avg = (r if gain_frames is None else rgb_pad[:gain_frames]).detach().mean(dim=0)
        lg = torch.log((res_avg + 0.01) / (rgb_avg + 0.01))
        scale = (torch.exp(lg.mean()) + 3) / 4
        rgb_pad = rgb_pad * scale
        out.update(gain=scale.detach(), log_sum=lg.sum().detach())
    x = rgb_pad.permute(1, 0, 2, 3)
    out["x"] = x.detach()
    if g_x is not None:
        (out["g_rgb"],) = torch.autograd.grad((x * g_x.detach().to(dtype)).sum(), leaf)
    return out


# ---- comparison --------------------------------------------------------------------------------------------------------------------------------------
def noise(r32, r64, sel=None):
    d = (r32.double() - r64).abs()
    d = d if sel is None else d[sel]
    return float(d.max()) if d.numel() else 0.0


def excess(got, r64, B, ulps=0, sel=None):
    """(max |got - statement|, max of that over the allowance B + ulps 2^-24 |v64|)"""
    got = got.detach().cpu().double().reshape(r64.shape)
    assert bool(torch.isfinite(got).all()), "not finite"
    d = (got - r64).abs()
    allow = B + ulps * ULP * r64.abs()
    if sel is not None:
        d, allow = d[sel], allow[sel]
    if not d.numel():
        return 0.0, 0.0
    ratio = torch.where(allow > 0, d / allow, torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
    return float(d.max()), float(ratio.max())


class Report:
    """prints each bound beside the measured maximum; `done()` holds every line to its allowance"""

    def __init__(self, tag):
        self.tag, self.bad = tag, []

    def check(self, name, got, r64, r32, ulps=0, sel=None, B=None):
        B = M_EXACT * noise(r32, r64, sel) if B is None else B
        e, r = excess(got, r64, B, ulps, sel)
        print(f"[{self.tag}] {name}: B {B:.3e} (+{ulps} ulp) measured max {e:.3e} (x{r:.2f} of the allowance), max |statement| {float(r64.abs().max()):.3e}")
        if not r <= 1.0:
            self.bad.append((name, e, B, r))
        return r

    def exact(self, name, got, ref):
        same = torch.equal(got.detach().cpu().double().reshape(ref.shape), ref.double())
        print(f"[{self.tag}] {name}: compared exactly: {'equal' if same else 'DIFFERENT'}")
        if not same:
            self.bad.append((name, "not equal"))

    def done(self):
        assert not self.bad, (self.tag, self.bad)


@dataclasses.dataclass
class FoldStatement:
    case: Case
    x: torch.Tensor              # [3,Tx,H,W] fp32, planted
    y: torch.Tensor              # [3,Ty,H,W] fp32
    nn: torch.Tensor             # [h_o,w_o,n1] int64
    f64: tuple                   # fold in fp64: (sum, weight, y2x)
    f32: tuple
    l64: tuple                   # loss in fp64: (rho, mean, grad, e)
    l32: tuple
    planted: torch.Tensor        # [3,Tx,H,W] bool: voxels planted with e == 0 exactly

    @property
    def grad_sel(self):
        """where the gradient is compared: everywhere; rou 'abs': away from the kink, and at the planted exact zeros"""
        if self.case.rou != "abs":
            return None
        return (self.l64[3].abs() > ABS_GAP) | self.planted

    def loss_bound(self, frames, waves):
        """B_loss of the module docstring for a kernel whose threads add `frames` values before 6 shuffle steps and `waves` partials"""
        return M_EXACT * noise(self.l32[0], self.l64[0]) + ULP * float(self.l64[0].abs().mean()) * (frames + 6 + waves)


_CACHE = {}


def clips(case):
    """(x, y) hash-uniform in [0, 1); a wrong frame or pixel is off by O(0.3)"""
    ps, s, pt, st, H, W, _ = case.cfg
    k = list(CONFIGS).index(case.config)
    return synth.hash_uniform((3, case.Tx, H, W), seed=50 + k), synth.hash_uniform((3, case.Ty, H, W), seed=70 + k)


def statement(case):
    """the FoldStatement of a case, computed once"""
    if case in _CACHE:
        return _CACHE[case]
    ps, s, pt, st, H, W, _ = case.cfg
    x, y = clips(case)
    nn = indices(case)
    f64 = fold(y, nn, ps, pt, s, st, case.Tx, torch.float64)
    f32 = fold(y, nn, ps, pt, s, st, case.Tx, torch.float32)
    # planted residuals at the voxels with exactly one vote: y2x is that y value, bit for bit, on every side
    one = (f64[1] == 1.0)[None].expand(3, -1, -1, -1)
    assert bool(one.any()) and torch.equal(f32[2][one].double(), f64[2][one])
    v = f32[2][one]
    # (at most one voxel in 200, spread evenly over the one-vote voxels: the residuals under ABS_GAP among them stay far below ABS_SHARE)
    keep = torch.zeros(v.numel(), dtype=torch.bool)
    keep[torch.linspace(0, v.numel() - 1, min(v.numel(), max(len(PLANT), x.numel() // 200))).long()] = True
    k = torch.where(keep, keep.long().cumsum(0) - 1, torch.full((v.numel(),), -1)) % len(PLANT)
    k = torch.where(keep, k, torch.full_like(k, -1))
    xv, zero = v.clone(), torch.zeros_like(v, dtype=torch.bool)
    for j, p in enumerate(PLANT):      # (x - y2x is exact in fp32 for every one of these: neighbours, or Sterbenz)
        if p == "+ulp":
            xv = torch.where(k == j, torch.nextafter(v, torch.full_like(v, 2.0)), xv)
        elif p == "-ulp":
            xv = torch.where(k == j, torch.nextafter(v, torch.full_like(v, -1.0)), xv)
        elif p == 0.0:
            zero |= k == j
        else:
            xv = torch.where(k == j, v + p, xv)
    x = x.clone()
    x[one] = torch.where(keep, xv, x[one])
    planted = torch.zeros_like(one)
    planted[one] = zero
    l64 = loss(x, f64[2], case.rou, case.scaling, torch.float64)
    l32 = loss(x, f32[2], case.rou, case.scaling, torch.float32)
    assert bool((l64[3][planted] == 0).all()) and bool((l32[3][planted] == 0).all())
    st_ = FoldStatement(case, x, y, nn, f64, f32, l64, l32, planted)
    _CACHE[case] = st_
    return st_


# ---- the robust kernels on their own (vl3d_robust_fwd / _bwd) ---------------------------------------------------------------------------------------------
ROBUST_N = (4096 * 256 + 257, 1)          # the grid-stride loop with a ragged tail | one element
GOUT = 0.37                               # the upstream gradient is not 1


def robust_inputs(n):
    """x, y2x [n] fp32: residuals over the full range; for n >= 4096 the first 4096 cycle through exact zeros, +-1 ulp and 2^-18"""
    y2x = synth.hash_uniform((n,), seed=91)
    x = synth.hash_uniform((n,), seed=92)
    m = 4096 if n >= 4096 else 0          # (a single element keeps its hash residual)
    k = torch.arange(m) % 4
    head = y2x[:m]
    up, dn = torch.nextafter(head, torch.full_like(head, 2.0)), torch.nextafter(head, torch.full_like(head, -1.0))
    x[:m] = torch.where(k == 0, head, torch.where(k == 1, up, torch.where(k == 2, dn, head + 2.0 ** -18)))
    i = torch.arange(n)
    return x, y2x, (i % 4 == 0) & (i < m)


def robust_statement(n, rou, scaling):
    """(x, y2x, planted exact zeros, loss in fp64, loss in fp32), computed once"""
    key = ("robust", n, rou, scaling)
    if key not in _CACHE:
        x, y2x, planted = robust_inputs(n)
        _CACHE[key] = (x, y2x, planted, loss(x, y2x, rou, scaling, torch.float64), loss(x, y2x, rou, scaling, torch.float32))
    return _CACHE[key]


# ---- the prologue's cases ---------------------------------------------------------------------------------------------------------------------------------
PRO_T, PRO_SIZES, PRO_F = (1, 2, 5, 17), ((3, 64), (5, 67)), 7
GRAM_TP = ((13, 2), (14, 2), (15, 2), (8, 8))          # T + pad = 15, 16, 17, 16: either side of a multiple of 16


def prologue_cases():
    """(T, pad, h, w): pad in {0, 1, 2, T}, at most T"""
    out = []
    for T in PRO_T:
        for pad in sorted({p for p in (0, 1, 2, T) if p <= T}):
            for h, w in PRO_SIZES:
                out.append((T, pad, h, w))
    return out


def prologue_inputs(T, pad, h, w, crop):
    """rgb [T,h,w,3]; res [F,3,h,w] -- contiguous, or a crop at (1, 2) of a clip 3 rows and 5 columns larger; g_x [3,T+pad,h,w]"""
    rgb = synth.hash_uniform((T, h, w, 3), seed=11 + T)
    if crop:
        res = synth.hash_uniform((PRO_F, 3, h + 3, w + 5), seed=12)[..., 1:1 + h, 2:2 + w]
    else:
        res = synth.hash_uniform((PRO_F, 3, h, w), seed=12)
    g_x = synth.hash_uniform((3, T + pad, h, w), seed=13) * 2 - 1
    return rgb, res, g_x


def prologue_statement(T, pad, h, w, gain, crop):
    key = ("prologue", T, pad, h, w, gain, crop)
    if key not in _CACHE:
        rgb, res, g_x = prologue_inputs(T, pad, h, w, crop)
        r = res if gain else None
        p64, p32 = prologue(rgb, r, pad, torch.float64, g_x), prologue(rgb, r, pad, torch.float32, g_x)
        t64 = t32 = None
        if gain:
            t64, t32 = log_terms(rgb, res, torch.float64), log_terms(rgb, res, torch.float32)
        _CACHE[key] = (rgb, res, g_x, p64, p32, t64, t32)
    return _CACHE[key]


def log_sum_bound(t64, t32):
    """3 h w B_term + 2^-24 sum |term64| (2 adds per thread + 6 shuffle steps + 3 adds of the wave partials)"""
    return t64.numel() * M_EXACT * noise(t32, t64) + ULP * float(t64.abs().sum()) * (2 + 6 + 3)
