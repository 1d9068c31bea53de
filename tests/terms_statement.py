"""The scalar head of a training iteration, stated in fp64 from the reference's lines, for tests/test_terms_statement_cpu.py (the statement is the
reference's, conditions on the case tables, planted faults) and tests/test_gpu_terms_fp64.py (every kernel of csrc/vl3d_terms.hip and
scale_inplace_k against it, through the C ABI).  Plain torch on the CPU; of the product only synth is imported.

The statement.
  train_3d.py:200-232   loop_loss = -mean(m log l + (1 - m) log(1 - l)), l = clamp(label, .001, 1 - .001); the scale-invariant gain
                        s = (exp(mean log((target + .01) / (rgb.detach() + .01))) + 3) / 4; img_loss = img2mse(rgb s, target) = mean((.)^2);
                        loss = img_loss + loop_loss + sum_k weight_k extra_k (the ABI also weighs the first two: w_img, w_loop).
  MPI.py:603-607        sparsity = mean_p(|a|_1 / |a|_2.clamp_min(eps)) / sqrt(mpi_d), stated from alpha_sums = (sum a, sum a^2) as the kernels take
                        it: x / sqrt(y.clamp_min(1e-30)).clamp_min(eps) (the inner clamp keeps the root's gradient finite at y = 0), times
                        `sparsity_scale`.  tests/test_terms_statement_cpu.py shows that this is the reference's spelling on per-plane a >= 0.
  MPI.py:647-650        density = mean_p |alpha - 1|.
  MPI.py:605-619        rgb_smooth = coef0 s0 + coef1 s1, a_smooth = coef2 s2 + coef3 s3 from the render's four sums (coef = denorm / count).
  train_3dvid.py:230-240  the stage-2 total: sum_i coef_i v_i, added in the order of the terms; group g's share of it.
Each in float64 on the widened fp32 inputs (the statement) and in float32 ("the oracle in fp32": the reference's own rounding noise).  Gradients of
the total w.r.t. rgb, label, alpha, alpha_sums and the smoothness sums come from autograd.  The constants the ABI fixes as floats enter as their
fp32 values, widened: 0.01f, 0.001f, 0.999f, 1e-30f, eps, the weights, sparsity_scale, smooth_coef.  So a label on a clamp bound, sum a^2 against
1e-30 and against eps^2 (the inputs keep |sqrt(max(y, 1e-30)) - eps| >= FLOOR_GAP eps, a condition of the tables), and alpha against 1 decide the
same way in fp32, in fp64 and in the kernel, and no element is left out of any comparison.

The bound.  Per case and per GROUP of elements B = M_EXACT max |oracle fp32 - oracle fp64| over the group (M_EXACT = 16 is render_statement's: value
arithmetic alone), no floor.  Groups, so that one class cannot shelter another: g_alpha_sums (each component) at uncovered pixels (y < 1e-30), at
floor-side pixels (sqrt(y) < eps), at pixels just above the floor (sqrt(y) < NEAR_FLOOR eps: the planted 4 eps^2 class, whose d / d sum a^2 is
~1e11 times an ordinary pixel's) and at ordinary pixels; g_label inside and outside the clamp (outside: an exact 0); g_rgb per case.  g_alpha is
+-k or 0 with an exactly known sign: it is compared with +-k64 under its ulp allowance alone (B = 0).

Roundings the kernels have and the oracle has not.  Each adds 2^-24 |v64| (v64: the statement's value of that element) to the allowance of the
output it enters; nothing is added that is not named here:
  g_rgb        RGB_ULPS = 2   (objective) k_img = w_img / (float)(3 n) is a float quotient, and (2 d s) k_img one more product; autograd divides once.
  g_label      LABEL_ULPS = 2 (objective) k_loop = w_loop / (float)n, and its product with the entropy's derivative.
  g_alpha_sums ASUM_ULPS = 3  (objective) k_sp = w_sp sparsity_scale / (float)n is a product and a quotient of floats, and multiplies the ratio's
                              derivative (x: k_sp / den).
  g_alpha      DEN_ULPS = 1   (objective) k_den = w_den / (float)n, one quotient.  Compared with +-k64, so this is its whole allowance.
  g_smooth     none: coef_i w, one product on both sides.
  vl3d_stage1_loss's grad and vl3d_pixel_terms's gradients (unit upstream gradient, counts not folded in): none.
Scalars -- out[1..6], the double `sums` of vl3d_pixel_terms and vl3d_stage1_loss, the log-ratio sum -- do not take their bound from one scalar's
lucky noise (the fp32 means land between 3e-9 and 7e-8 relative from fp64) but from the fp32 chain a kernel has before its double atomic:
  B_sum  = N M_EXACT max |term32 - term64| + 2^-24 sum |term64| (adds per thread + 6 shuffle steps + 3 adds of the wave partials)
  B_mean = B_sum / N + 2^-24 |mean64|                                  (the final (float))
with N the number of terms, adds per thread = trips of the grid-stride loop (x 3 for the image sum and the log-ratio sum: three channels).
  out[1] img, out[2] loop   B_mean.
  out[3] w sparsity         |w_sp sparsity_scale| B_mean + 2 x 2^-24 |v64|   (two products after the (float))
  out[4] w density          |w_den| B_mean + 2^-24 |v64|
  out[5], out[6]            4 x 2^-24 |w| (|c_a s_a| + |c_b s_b|)            (two products, one add, one product)
  out[0] total              |w_img| B_1 + |w_loop| B_2 + B_3 + .. + B_6 + 7 x 2^-24 sum |part64|      (two products, five adds)
  out[7] gain               e / 4 (B_sum(log) / (3 n) + 2 x 2^-24 |mean64|) + 2^-24 (e + (e + 3)) / 4, e = exp(mean64): the log-sum's bound through
                            exp(.) / 4; the (float) of the mean and the exponential's argument product; the exponential's and the sum's rounding.
No number is fixed for __logf / __expf (v_log_f32 / v_exp_f32): their accuracy is what these bounds measure.  The gain's accuracy where it matters
is held by g_rgb and img at their own B, with nothing added for it.
vl3d_linear_head_fwd: B = 2^-24 sum |coef_i v_i| (1 + n) over the terms that enter (one product each, n adds of a chain); grad_terms are compared
bit for bit with the fp32 product coef_i g.  vl3d_scale_inplace: bit for bit with the fp32 product.

Literals of tests/test_terms_statement_cpu.py (statement against oracle, never a kernel): 1e-6 relative between two fp32 means of O(1) terms added
in different orders (192 pixels: a few ulps of 6e-8); 1e-12 / 1e-9 relative between two fp64 spellings of one ratio and of its gradient (a few
hundred ulps of 1.1e-16; the gradient divides by |a|_2^3); 1e-5 relative + 1e-6 absolute between an fp32 chain of <= 16 terms and the sum of its
three groups' chains (16 adds of 6e-8 on terms up to 3).

Planted inputs.  Pixel i has class i % PERIOD (PERIOD = 67: the classes drift across lanes and rows); class 0 and the classes above the last planted
one are hash-uniform: labels in [-0.05, 1.05), alpha in [0, 1.2), alpha_sums from 8 hash planes, rgb and target in [0, 1), masks binary.  Planted:
labels on each clamp bound and one ulp either side, below 0 and above 1; soft masks 0.25 / 0.5; alpha 1, 1 +- ulp, 0, 1.2; sum a^2 in
{0, 1e-38, 1e-31, 1e-29, eps^2 / 4, 4 eps^2}, each with three sum a (0 or sqrt(y) max 1e-23, then 1.7 and 2.5 times that: a pixel of a few faint
planes); rgb == target == 0 (log ratio exactly 0)."""
import dataclasses
import math

import numpy as np
import torch

from render_statement import M_EXACT
from videoloop3d_amd import synth

ULP = 2.0 ** -24
RGB_ULPS, LABEL_ULPS, ASUM_ULPS, DEN_ULPS = 2, 2, 3, 1
FLOOR_GAP = 1e-3
NEAR_FLOOR = 100.0          # sqrt(sum a^2) below NEAR_FLOOR eps: d / d sum a^2 is ~1e11 times an ordinary pixel's there (the planted 4 eps^2 class)
ASUM_GROUPS = ("uncovered", "floor", "above", "ordinary")
SENTINEL = -7.0
PERIOD = 67


def f32(v):
    """the fp32 value of an ABI float, widened"""
    return float(np.float32(v))


C01, LO, HI, TINY = f32(0.01), f32(0.001), f32(0.999), f32(1e-30)

# ---- the case tables of tests/test_gpu_terms_fp64.py ----------------------------------------------------------------------------------------------------
SHAPES = ((1, 1, 1), (1, 5, 7), (1, 3, 86), (2, 37, 53), (3, 24, 32))      # n = 1 | less than a wave | 258 pixels, two workgroups | B = 2, odd | B = 3
BIG = (2, 513, 1025)                                                      # 1 051 650 pixels: 4096 workgroups, a ragged second trip of 3074
LAYOUTS = ("contiguous", "crop")
SUBSETS = ("all", "no_label", "no_alpha", "no_asum", "no_smooth", "rgb_only")
WEIGHTS = ((1.0, 1.0, 0.004, 0.002, 0.05, 0.03), (0.7, 1.3, 0.0, 0.37, 2.5, 0.0), (0.0, 3.0, 1.7, 0.0, 0.0, 0.11))      # img, loop, sparsity, density, rgb_smooth, a_smooth
EPS = (1e-6, 1e-4)                                                        # MPMesh | MPMeshVid
MPI_D = (32, 24)                                                          # sparsity_scale = 1 / sqrt(mpi_d)
PLANES = 8                                                                # planes behind the ordinary alpha_sums and the smoothness counts
LABEL_CLASS, ALPHA_CLASS, ASUM_CLASS, ZERO_CLASS = 1, 9, 14, 32
SOFT_QUARTER, SOFT_HALF = (3, 7, 34, 36), (5, 35)
GRID_CAP, SCALE_CAP = 4096, 8192


@dataclasses.dataclass(frozen=True)
class Case:
    shape: tuple
    layout: str
    subset: str
    gain: bool
    weights: tuple
    eps: float
    mpi_d: int

    @property
    def n(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def has(self):
        """(label, alpha, alpha_sums, smooth sums) given"""
        s = self.subset
        return (s not in ("no_label", "rgb_only"), s not in ("no_alpha", "rgb_only"), s not in ("no_asum", "rgb_only"), s not in ("no_smooth", "rgb_only"))


def cases(shape):
    """12 cases per shape: both layouts x every subset; gain, weights, eps and mpi_d cycle so that over the shapes every subset meets both gains"""
    si = (SHAPES + (BIG,)).index(shape)
    out = []
    for li, layout in enumerate(LAYOUTS):
        for ki, subset in enumerate(SUBSETS):
            k = si + li + ki
            out.append(Case(shape, layout, subset, k % 2 == 0, WEIGHTS[(si + 2 * li + ki) % 3], EPS[(k // 2) % 2], MPI_D[(si + ki) % 2]))
    return out


BIG_CASE = Case(BIG, "crop", "all", True, WEIGHTS[1][:2] + (0.004, 0.37, 2.5, 0.03), EPS[0], MPI_D[0])


def trips(n, per=256, cap=GRID_CAP):
    """trips of the grid-stride loop the busiest thread makes (grid_for: at most `cap` workgroups of `per`)"""
    grid = min(-(-n // per), cap)
    return -(-n // (grid * per))


class _Seeds:
    """seed + j: seeds that differ in their HIGH bits (hash_uniform mixes index ^ seed: seeds that differ in low bits only permute one field)"""

    def __init__(self, si):
        self.si = si

    def __add__(self, j):
        return ((16 * self.si + j) * 0x9E3779B1) & 0x7FFFFFFF


@dataclasses.dataclass
class Inputs:
    rgb: torch.Tensor            # [B,h,w,3]
    label: torch.Tensor          # [B,h,w]
    alpha: torch.Tensor          # [B,h,w]
    asum: torch.Tensor           # [B,h,w,2]
    smooth: torch.Tensor         # [4]
    target: torch.Tensor         # [B,3,h,w], contiguous or a crop of a sentinel-filled parent
    tmask: torch.Tensor          # [B,h,w], likewise
    coef: tuple                  # smooth_coef, fp32 values
    cls: torch.Tensor            # [B,h,w] the pixel's class


def planted_labels():
    lo, hi = torch.tensor(LO, dtype=torch.float32), torch.tensor(HI, dtype=torch.float32)
    dn, up = torch.tensor(-1.0), torch.tensor(2.0)
    return torch.stack([lo, hi, torch.nextafter(lo, dn), torch.nextafter(lo, up), torch.nextafter(hi, dn), torch.nextafter(hi, up),
                        torch.tensor(-0.03), torch.tensor(1.04)])


def planted_alphas():
    one = torch.tensor(1.0)
    return torch.stack([one, torch.nextafter(one, torch.tensor(2.0)), torch.nextafter(one, torch.tensor(0.0)), torch.tensor(0.0), torch.tensor(1.2)])


def planted_asums(eps):
    """[18, 2] fp32: (x, y) for y in {0, 1e-38, 1e-31, 1e-29, eps^2 / 4, 4 eps^2} x three x"""
    e = f32(eps)
    out = []
    for y in (0.0, 1e-38, 1e-31, 1e-29, e * e / 4, 4 * e * e):
        x0 = max(math.sqrt(y), 1e-23)
        out += [(0.0 if y == 0.0 else x0, y), (1.7 * x0, y), (2.5 * x0, y)]
    return torch.tensor(out, dtype=torch.float64).to(torch.float32)


def inputs(shape, layout, eps):
    B, h, w = shape
    n = B * h * w
    c = (torch.arange(n) % PERIOD).reshape(B, h, w)
    seed = _Seeds((SHAPES + (BIG,)).index(shape))
    rgb, tgt = synth.hash_uniform((B, h, w, 3), seed=seed + 1), synth.hash_uniform((B, 3, h, w), seed=seed + 2)
    zero = (c == ZERO_CLASS) | (c == ZERO_CLASS + 1)
    rgb[zero] = 0
    tgt.permute(0, 2, 3, 1)[zero] = 0
    label = synth.hash_uniform((B, h, w), seed=seed + 3) * 1.1 - 0.05
    for k, v in enumerate(planted_labels()):
        label[c == LABEL_CLASS + k] = v
    mask = (synth.hash_uniform((B, h, w), seed=seed + 4) > 0.5).float()
    for k in SOFT_QUARTER:
        mask[c == k] = 0.25
    for k in SOFT_HALF:
        mask[c == k] = 0.5
    alpha = synth.hash_uniform((B, h, w), seed=seed + 5) * 1.2
    for k, v in enumerate(planted_alphas()):
        alpha[c == ALPHA_CLASS + k] = v
    a = synth.hash_uniform((B, h, w, PLANES), seed=seed + 6)
    asum = torch.stack([a.sum(-1), (a * a).sum(-1)], -1)
    for k, v in enumerate(planted_asums(eps)):
        asum[c == ASUM_CLASS + k] = v
    smooth = synth.hash_uniform((4,), seed=seed + 7) * 1000 + 1
    nx, ny = max(1, B * h * (w - 1) * PLANES), max(1, B * (h - 1) * w * PLANES)
    coef = tuple(f32(v) for v in (1.0 / (3 * nx), 1.0 / (3 * ny), 1.0 / nx, 1.0 / ny))
    if layout == "crop":      # a crop of a larger still: row pitch > w, batch stride != 3 x channel stride, non-zero offsets, sentinels around
        tp = torch.full((B, 4, h + 3, w + 5), SENTINEL, dtype=torch.float32)
        tv = tp[:, 1:4, 1:1 + h, 2:2 + w]
        tv.copy_(tgt)
        mp = torch.full((B, h + 2, w + 7), SENTINEL, dtype=torch.float32)
        mv = mp[:, 1:1 + h, 3:3 + w]
        mv.copy_(mask)
        tgt, mask = tv, mv
    return Inputs(rgb, label, alpha, asum, smooth, tgt, mask, coef, c)


# ---- the statement -----------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Result:
    out: torch.Tensor            # [8] total, img, loop, w sparsity, w density, w rgb_smooth, w a_smooth, gain
    g: dict                      # rgb [B,h,w,3], label, alpha [B,h,w], asum [B,h,w,2], smooth [4] (None where the input is absent)
    t: dict                      # the terms behind the sums: img [B,3,h,w], loop, sp, dn [B,h,w], log [B,3,h,w] (None where absent)


def sparsity_terms(asum, eps):
    """MPI.py:603-605 per pixel from alpha_sums [..., 2] = (sum a, sum a^2): |a|_1 / |a|_2.clamp_min(eps); eps an fp32 value, widened"""
    norm2 = torch.sqrt(asum[..., 1].clamp_min(TINY))
    return asum[..., 0] / norm2.clamp_min(eps)


def density_terms(alpha):
    """MPI.py:648-649 per pixel"""
    return (alpha - 1).abs()


def objective(x, case, dtype, gain_detached=True, unit_sums=False):
    """train_3d.py:200-232 on MPI.py:596-652's outputs.  unit_sums: the total is the plain SUM of every term (vl3d_stage1_loss / vl3d_pixel_terms hand
    out d sums / d input for a unit upstream gradient).  gain_detached=False is a planted fault"""
    has_label, has_alpha, has_asum, has_smooth = case.has
    W = [f32(v) for v in case.weights]
    eps, sps = f32(case.eps), f32(1.0 / np.sqrt(case.mpi_d))
    leaf = lambda t, on=True: t.detach().to(dtype).requires_grad_(True) if on else None      # noqa: E731
    rgb_l, label, alpha, asum, smooth = leaf(x.rgb), leaf(x.label, has_label), leaf(x.alpha, has_alpha), leaf(x.asum, has_asum), leaf(x.smooth, has_smooth)
    target = x.target.detach().to(dtype)
    rgb = rgb_l.permute(0, 3, 1, 2)
    t = dict(img=None, loop=None, sp=None, dn=None, log=None)
    zero = torch.zeros((), dtype=dtype)
    loop = zero
    if has_label:
        tm = x.tmask.detach().to(dtype)
        lm = torch.clamp(label, LO, HI)
        ent = tm * torch.log(lm) + (1 - tm) * torch.log(1 - lm)
        t["loop"], loop = -ent, -ent.mean()
    gain = torch.ones((), dtype=dtype)
    if case.gain:
        t["log"] = torch.log((target + C01) / ((rgb.detach() if gain_detached else rgb) + C01))
        gain = (torch.exp(t["log"].mean()) + 3) / 4
        rgb = rgb * gain
    t["img"] = (rgb - target) ** 2
    img = t["img"].mean()
    sparsity = density = rgb_smooth = a_smooth = zero
    if has_asum:
        t["sp"] = sparsity_terms(asum, eps)
        sparsity = t["sp"].mean() * sps
    if has_alpha:
        t["dn"] = density_terms(alpha)
        density = t["dn"].mean()
    if has_smooth:
        rgb_smooth = x.coef[0] * smooth[0] + x.coef[1] * smooth[1]
        a_smooth = x.coef[2] * smooth[2] + x.coef[3] * smooth[3]
    parts = [W[0] * img, W[1] * loop, W[2] * sparsity, W[3] * density, W[4] * rgb_smooth, W[5] * a_smooth]
    loss = parts[0] + parts[1]
    for v in parts[2:]:
        loss = loss + v
    if unit_sums:
        loss = sum(v.sum() for v in (t["img"], t["loop"], t["sp"], t["dn"]) if v is not None)
    leaves = dict(rgb=rgb_l, label=label, alpha=alpha, asum=asum, smooth=smooth)
    on = [k for k, v in leaves.items() if v is not None and not (unit_sums and k == "smooth")]
    grads = dict.fromkeys(leaves)
    grads.update(zip(on, torch.autograd.grad(loss, [leaves[k] for k in on])))
    out = torch.stack([loss, img, loop] + parts[2:] + [gain]).detach()
    return Result(out, grads, {k: (None if v is None else v.detach()) for k, v in t.items()})


def head(v, coef, groups, ngroups, dtype):
    """train_3dvid.py:230-240: loss = swd + sum_k weight_k term_k, added in order -> (total, [ngroups] the groups' shares); term i is of group groups[i]"""
    tv = v.to(dtype) * coef.to(dtype)
    total = torch.zeros((), dtype=dtype)
    share = [torch.zeros((), dtype=dtype) for _ in range(ngroups)]
    for i in range(tv.numel()):
        total = total + tv[i]
        if groups[i] < ngroups:
            share[groups[i]] = share[groups[i]] + tv[i]
    return total, torch.stack(share)


def head_bound(v, coef, members=None):
    """2^-24 sum |coef_i v_i| (1 + n) over the terms that enter: one product each, a chain of n adds"""
    tv = (v.double() * coef.double()).abs()
    return ULP * float(tv.sum() if members is None else tv[members].sum()) * (1 + v.numel())


def groups_word(groups):
    """the 64-bit `groups` argument: term i's group in nibble i"""
    return sum(int(g) << (4 * i) for i, g in enumerate(groups))


# ---- statements per case, computed once ------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Statement:
    case: Case
    x: Inputs
    r64: Result
    r32: Result
    unit: bool = False

    @property
    def sel(self):
        """the groups of elements: label inside / outside the clamp; alpha_sums uncovered / floor-side / just above the floor / ordinary"""
        lab, y = self.x.label.double(), self.x.asum[..., 1].double()
        inside = (lab >= LO) & (lab <= HI)
        unc = y < TINY
        n2, eps = torch.sqrt(y), f32(self.case.eps)
        floor_ = ~unc & (n2 < eps)
        above = ~unc & ~floor_ & (n2 < NEAR_FLOOR * eps)
        return dict(inside=inside, outside=~inside, uncovered=unc, floor=floor_, above=above, ordinary=~unc & ~floor_ & ~above)


_CACHE = {}


def statement(case, unit=False):
    key = (case, unit)
    if key not in _CACHE:
        x = inputs(case.shape, case.layout, case.eps)
        _CACHE[key] = Statement(case, x, objective(x, case, torch.float64, unit_sums=unit), objective(x, case, torch.float32, unit_sums=unit), unit)
    return _CACHE[key]


# ---- comparison --------------------------------------------------------------------------------------------------------------------------------------
def noise(r32, r64, sel=None):
    d = (r32.double() - r64).abs()
    d = d if sel is None else d[sel]
    return float(d.max()) if d.numel() else 0.0


def excess(got, r64, B, ulps=0, sel=None):
    """(max |got - statement|, max of that over the allowance B + ulps 2^-24 |v64|); a deviation where the allowance is 0 is infinite"""
    got = got.detach().cpu().double().reshape(r64.shape)
    if not bool(torch.isfinite(got if sel is None else got[sel]).all()):
        return math.inf, math.inf
    d = (got - r64).abs()
    allow = B + ulps * ULP * r64.abs()
    if sel is not None:
        d, allow = d[sel], allow[sel]
    if not d.numel():
        return 0.0, 0.0
    ratio = torch.where(allow > 0, d / allow, torch.where(d > 0, torch.full_like(d, math.inf), torch.zeros_like(d)))
    return float(d.max()), float(ratio.max())


def sum_bound(t64, t32, adds_per_trip, n, cap=GRID_CAP):
    """B_sum of the module docstring"""
    return t64.numel() * M_EXACT * noise(t32, t64) + ULP * float(t64.abs().sum()) * (adds_per_trip * trips(n, cap=cap) + 6 + 3)


def mean_bound(t64, t32, adds_per_trip, n):
    """B_mean of the module docstring"""
    return sum_bound(t64, t32, adds_per_trip, n) / t64.numel() + ULP * abs(float(t64.mean()))


def out_bounds(st):
    """the allowance of each of out[0..7] (module docstring)"""
    c, r64, r32, n = st.case, st.r64, st.r32, st.case.n
    W = [f32(v) for v in c.weights]
    sps = f32(1.0 / np.sqrt(c.mpi_d))
    o = [abs(float(v)) for v in r64.out]
    mb = lambda k, adds: mean_bound(r64.t[k], r32.t[k], adds, n) if r64.t[k] is not None else 0.0      # noqa: E731
    B = [0.0] * 8
    B[1], B[2] = mb("img", 3), mb("loop", 1)
    B[3] = abs(W[2] * sps) * mb("sp", 1) + 2 * ULP * o[3]
    B[4] = abs(W[3]) * mb("dn", 1) + ULP * o[4]
    if c.has[3]:
        s, k = st.x.smooth.double().abs(), st.x.coef
        B[5] = 4 * ULP * abs(W[4]) * float(k[0] * s[0] + k[1] * s[1])
        B[6] = 4 * ULP * abs(W[5]) * float(k[2] * s[2] + k[3] * s[3])
    parts = abs(W[0]) * o[1] + abs(W[1]) * o[2] + o[3] + o[4] + o[5] + o[6]
    B[0] = abs(W[0]) * B[1] + abs(W[1]) * B[2] + B[3] + B[4] + B[5] + B[6] + 7 * ULP * parts
    if c.gain:
        lg = r64.t["log"]
        mean = float(lg.mean())
        e = math.exp(mean)
        B[7] = e / 4 * (sum_bound(lg, r32.t["log"], 3, n) / lg.numel() + 2 * ULP * abs(mean)) + ULP * (e + (e + 3)) / 4
    return B


class Report:
    """prints each bound beside the measured maximum; `done()` holds every line to its allowance.  `worst` is the largest measured / allowance"""

    TABLE = {}          # (entry, name) -> [smallest B, largest B, ulps, largest deviation, largest measured / allowance] over the reports of an entry

    def __init__(self, tag, quiet=False, entry=None):
        self.tag, self.bad, self.quiet, self.worst, self.rows, self.entry = tag, [], quiet, 0.0, [], entry

    def _row(self, name, B, ulps, e, r, empty=False):
        self.worst = max(self.worst, r)
        self.rows.append((name, B, ulps, e, r))
        if self.entry is not None and not empty:          # (a group no element of the case is in does not enter the table as B = 0)
            row = self.TABLE.setdefault((self.entry, name), [math.inf, 0.0, ulps, 0.0, 0.0])
            row[0], row[1], row[3], row[4] = min(row[0], B), max(row[1], B), max(row[3], e), max(row[4], r)
        if not self.quiet:
            print(f"[{self.tag}] {name}: B {B:.3e} (+{ulps} ulp) measured max {e:.3e} (x{r:.3f} of the allowance)")
        if not r <= 1.0:
            self.bad.append((name, e, B, r))

    def check(self, name, got, r64, r32, ulps=0, sel=None, B=None):
        B = M_EXACT * noise(r32, r64, sel) if B is None else B
        e, r = excess(got, r64, B, ulps, sel)
        self._row(name, B, ulps, e, r, empty=sel is not None and not bool(sel.any()))

    def scalar(self, name, got, ref, B):
        e = abs(float(got) - float(ref))
        r = (e / B if B > 0 else (0.0 if e == 0 else math.inf)) if math.isfinite(float(got)) else math.inf
        self._row(name, B, 0, e, r)

    def done(self):
        assert not self.bad, (self.tag, self.bad)

    @classmethod
    def print_table(cls):
        """one line per entry and output: B (smallest .. largest case), the ulp allowance beside it, the largest deviation, the largest ratio"""
        print()
        for (entry, name), (b0, b1, ulps, e, r) in cls.TABLE.items():
            print(f"TABLE | {entry} | {name} | {b0:.2e} .. {b1:.2e} | {ulps} ulp | {e:.2e} | {r:.3f}")


OUT_NAMES = ("out[0] total", "out[1] img", "out[2] loop", "out[3] w sparsity", "out[4] w density", "out[5] w rgb_smooth", "out[6] w a_smooth", "out[7] gain")


def check_objective(rep, st, out, g_rgb, g_label, g_alpha, g_asum, g_smooth, log_sum):
    """vl3d_stage1_objective's outputs (tensors, None where the input is absent; log_sum a float or None) against the statement of the case"""
    c, r64, r32, sel = st.case, st.r64, st.r32, st.sel
    has_label, has_alpha, has_asum, has_smooth = c.has
    for i, B in enumerate(out_bounds(st)):
        rep.scalar(OUT_NAMES[i], out[i], r64.out[i], B)
    if c.gain:
        rep.scalar("log-ratio sum", log_sum, r64.t["log"].sum(), sum_bound(r64.t["log"], r32.t["log"], 3, c.n))
    rep.check("g_rgb", g_rgb, r64.g["rgb"], r32.g["rgb"], RGB_ULPS)
    if has_label:
        rep.check("g_label inside the clamp", g_label, r64.g["label"], r32.g["label"], LABEL_ULPS, sel["inside"])
        rep.check("g_label outside the clamp", g_label, r64.g["label"], r32.g["label"], 0, sel["outside"], B=0.0)
    if has_alpha:
        rep.check("g_alpha against +-k64", g_alpha, r64.g["alpha"], r32.g["alpha"], DEN_ULPS, B=0.0)
    if has_asum:
        for k in ASUM_GROUPS:
            for j, comp in enumerate(("d/d sum a", "d/d sum a^2")):
                s = sel[k][..., None].expand(-1, -1, -1, 2) & (torch.arange(2) == j)
                rep.check(f"g_alpha_sums {comp}, {k} pixels", g_asum, r64.g["asum"], r32.g["asum"], ASUM_ULPS, s)
    if has_smooth:
        rep.check("g_smooth", g_smooth, r64.g["smooth"], r32.g["smooth"])


def oracle_outputs(st, r=None):
    """the fp32 oracle's outputs in check_objective's order (a dict, so that a fault can be planted in one of them)"""
    r = st.r32 if r is None else r
    return dict(out=r.out.clone(), g_rgb=r.g["rgb"], g_label=r.g["label"], g_alpha=r.g["alpha"], g_asum=r.g["asum"], g_smooth=r.g["smooth"],
                log_sum=None if r.t["log"] is None else float(r.t["log"].sum()))


# ---- vl3d_stage1_loss / vl3d_pixel_terms: unit sums --------------------------------------------------------------------------------------------------------
def loss_case(shape, C, gain):
    """the Case behind a vl3d_stage1_loss call: contiguous targets, label and mask with C == 4, nothing else"""
    return Case(shape, "contiguous", "no_smooth" if C == 4 else "rgb_only", gain, (1.0,) * 6, EPS[0], MPI_D[0])


def check_stage1_loss(rep, st, C, sums, grad, log_sum):
    """sums [2] doubles, grad [B,h,w,C], log_sum (a float or None) of vl3d_stage1_loss against the unit-sum statement"""
    c, r64, r32, sel = st.case, st.r64, st.r32, st.sel
    rep.scalar("sums[0] img", sums[0], r64.t["img"].sum(), sum_bound(r64.t["img"], r32.t["img"], 3, c.n))
    if c.gain:
        rep.scalar("log-ratio sum", log_sum, r64.t["log"].sum(), sum_bound(r64.t["log"], r32.t["log"], 3, c.n))
    rep.check("grad rgb", grad[..., :3], r64.g["rgb"], r32.g["rgb"])
    if C == 4:
        rep.scalar("sums[1] loop", sums[1], r64.t["loop"].sum(), sum_bound(r64.t["loop"], r32.t["loop"], 1, c.n))
        rep.check("grad label inside the clamp", grad[..., 3], r64.g["label"], r32.g["label"], 0, sel["inside"])
        rep.check("grad label outside the clamp", grad[..., 3], r64.g["label"], r32.g["label"], 0, sel["outside"], B=0.0)
    else:
        rep.scalar("sums[1] without a label", sums[1], 0.0, 0.0)


def terms_case(shape, which, eps):
    return Case(shape, "contiguous", {"both": "no_label", "sparsity": "no_alpha", "density": "no_asum"}[which], False, (1.0,) * 6, eps, MPI_D[0])


def check_pixel_terms(rep, st, sums, g_asum, g_alpha):
    """sums [2] doubles and the gradients of vl3d_pixel_terms against the unit-sum statement (an absent input's sum stays 0)"""
    c, r64, r32, sel = st.case, st.r64, st.r32, st.sel
    _, has_alpha, has_asum, _ = c.has
    if has_asum:
        rep.scalar("sums[0] sparsity", sums[0], r64.t["sp"].sum(), sum_bound(r64.t["sp"], r32.t["sp"], 1, c.n))
        for k in ASUM_GROUPS:
            for j, comp in enumerate(("d/d sum a", "d/d sum a^2")):
                s = sel[k][..., None].expand(-1, -1, -1, 2) & (torch.arange(2) == j)
                rep.check(f"g_alpha_sums {comp}, {k} pixels", g_asum, r64.g["asum"], r32.g["asum"], 0, s)
    else:
        rep.scalar("sums[0] without alpha_sums", sums[0], 0.0, 0.0)
    if has_alpha:
        rep.scalar("sums[1] density", sums[1], r64.t["dn"].sum(), sum_bound(r64.t["dn"], r32.t["dn"], 1, c.n))
        rep.check("g_alpha against +-1", g_alpha, r64.g["alpha"], r32.g["alpha"], 0, B=0.0)
    else:
        rep.scalar("sums[1] without alpha", sums[1], 0.0, 0.0)


# ---- vl3d_scale_inplace / vl3d_linear_head ---------------------------------------------------------------------------------------------------------------
SCALE_N = (4, 4 * 257, 4 * (SCALE_CAP * 256 + 257))          # one float4 | two workgroups | a second trip of the grid-stride loop (8192 x 256 float4 per trip)
SCALES = (1.0, 2.5, -0.37)
HEAD_N, HEAD_NGROUPS = (1, 2, 7, 16), (1, 3, 16)


def head_inputs(n, ngroups):
    """v, coef [n] fp32 and the groups of the n terms: the first and the last term are of the last group (id 15 in term 15's nibble, the word's top
    one, at n = ngroups = 16), term i between them of group i % ngroups"""
    v = synth.hash_uniform((n,), seed=200 + n) * 4 - 1
    coef = synth.hash_uniform((n,), seed=300 + n) * 2 - 0.5
    groups = [ngroups - 1 if i in (0, n - 1) else i % ngroups for i in range(n)]
    return v, coef, groups
