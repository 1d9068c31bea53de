"""Camera registration -- the normal equations of include/vl3d.h ("Camera registration"): a per-frame or a long-exposure residual, with or
without the two brightness unknowns -- stated against the CPU oracle in fp64, for tests/test_register_statement_cpu.py (conditions on the
reference alone, planted faults, the Levenberg-Marquardt runs) and tests/test_gpu_cam_register.py (the kernel against it).  Plain torch on the
CPU; of the product only synth (and, through normal_statement, poses: the pose chain).

The statement.  C [T,H,W,3] and J [T,H,W,3,P] are normal_statement.jacobian's (the forward-mode Jacobian of oracle/mpi_oracle.render_planes
in float64), g = exp(a):
    per frame:      r = g C + beta - I [T,H,W,3];  columns g J, then with the brightness unknowns g C and 1
    long exposure:  Cm = mean_t C, Jm = mean_t J;  r = g Cm + beta - I [H,W,3];  columns g Jm, g Cm, 1
and A = sum w col_k col_l, b = sum w col_k r, cost = sum w r^2 by torch.sum as normal_statement._sums forms them.  The same in float32, sums
included, is "the oracle in fp32".

Comparison: normal_statement.Statement -- its normalisation (A_kl / sqrt(A64_kk A64_ll), b_k / sqrt(A64_kk cost64), cost / cost64) and its
bound B = m max |fp32 - fp64| take Q = P + 2 entries as they take P; m and the unsafe pixels (weight 0 there, cap 5 %) are camera_statement's.

Faults to plant (`evaluate(fault=...)`): no_inv_t (the long exposure is the SUM of the frames), no_gain (the geometric columns without g),
bias_by_c (the bias column is the picture instead of 1), frame0 (the long-exposure residual against frame 0 of the render instead of the
mean)."""
import math

import torch

import camera_statement as CS
import normal_statement as NS
import render_statement as RS
from videoloop3d_amd import synth

FAULTS = ("no_inv_t", "no_gain", "bias_by_c", "frame0")
POINT = (0.2, -0.05)      # a (log gain, bias) away from (0, 0)


def target(scene, Tn, long_exposure, seed=73):
    """[T,H,W,3], or [H,W,3] for the long exposure: float32 in [0, 1), not the render's picture"""
    return NS.target(scene, 1, seed)[0].contiguous() if long_exposure else NS.target(scene, Tn, seed)


def weights(scene, Tn, long_exposure, window=(0, 0), kind="random", seed=79):
    """normal_statement.weights, [T,H,W] or (long exposure) [H,W]; None for "none\""""
    w = NS.weights(scene, 1 if long_exposure else Tn, window, kind, seed)
    return w if (w is None or not long_exposure) else w[0].contiguous()


def fault_applies(Tn, long_exposure, photo, point, fault):
    if fault in ("no_inv_t", "frame0"):
        return long_exposure and Tn > 1
    if fault == "no_gain":
        return point[0] != 0.0
    return bool(photo)      # bias_by_c


def sums(J, C, tgt, w, long_exposure, photo, point=(0.0, 0.0), fault=None):
    """J [T,H,W,3,P], C [T,H,W,3] in one dtype -> (A [Q,Q], b [Q], cost) in that dtype"""
    dtype = J.dtype
    g, beta = math.exp(point[0]), point[1]
    tgt = tgt.to(dtype)
    w = None if w is None else w.to(dtype)
    if long_exposure:
        over = (lambda t: t.sum(0, keepdim=True)) if fault == "no_inv_t" else (lambda t: t.mean(0, keepdim=True))      # noqa: E731
        Cr = C[:1] if fault == "frame0" else over(C)
        J, C = over(J), over(C)
        tgt, w = tgt[None], None if w is None else w[None]
    else:
        Cr = C
    return _assemble(J, C, Cr, tgt, w, g, beta, photo, fault)


def _assemble(J, C, Cr, tgt, w, g, beta, photo, fault):
    r = g * Cr + beta - tgt
    cols = [J if fault == "no_gain" else g * J]
    if photo:
        cols += [(g * C)[..., None], (g * C if fault == "bias_by_c" else torch.ones_like(C))[..., None]]
    return NS._sums(torch.cat(cols, -1), r, w)


def evaluate(scene, stack, dh, tgt, w=None, long_exposure=False, photo=False, point=(0.0, 0.0), dtype=torch.float64, window=(0, 0), fault=None, jc=None):
    """-> (A [Q,Q], b [Q], cost) in `dtype`; `jc`: a (J, C) of normal_statement.jacobian in `dtype`, if the caller holds it"""
    J, C = NS.jacobian(scene, stack, dh, dtype, window) if jc is None else jc
    return sums(J, C, tgt, w, long_exposure, photo, point, fault)


def gradient(scene, stack, dh, tgt, w, long_exposure, point, window=(0, 0)):
    """reverse mode: d (1/2 sum w r^2) / d (eps, a, beta) at (0, point) in float64 -- what b must equal with the brightness unknowns"""
    import baked_statement as BS
    from oracle import mpi_oracle as MO
    o = BS.oracle_spec(scene.spec)
    eps = torch.zeros(len(dh), dtype=torch.float64, requires_grad=True)
    a = torch.tensor(point[0], dtype=torch.float64, requires_grad=True)
    beta = torch.tensor(point[1], dtype=torch.float64, requires_grad=True)
    hom = scene.homos.double() + (eps[:, None, None, None] * dh.double()).sum(0)
    rgb = MO.render_planes(stack.double(), hom, scene.H + window[0], scene.W + window[1], o, quad_keep=scene.keep)[0][:, window[0]:, window[1]:]
    if long_exposure:
        rgb = rgb.mean(0)
    r = torch.exp(a) * rgb + beta - tgt.double()
    half = 0.5 * ((r * r) if w is None else (r * r * w.double()[..., None])).sum()
    return torch.cat([t.reshape(-1) for t in torch.autograd.grad(half, [eps, a, beta])]).detach()


_JC = {}


def statement(scene, stack, dh, tgt, w, long_exposure, photo, point=(0.0, 0.0), window=(0, 0), key=None):
    """the normal_statement.Statement of one case.  `key`: the (J, C) of (scene, stack, tangents, window) in both precisions is computed once
    and shared among the cases that differ in mode, brightness, point, target and weight only."""
    if key is None or key not in _JC:
        jc = {dt: NS.jacobian(scene, stack, dh, dt, window) for dt in (torch.float64, torch.float32)}
        if key is not None:
            _JC[key] = jc
    else:
        jc = _JC[key]
    s64, s32 = (evaluate(scene, stack, dh, tgt, w, long_exposure, photo, point, dt, window, jc=jc[dt]) for dt in (torch.float64, torch.float32))
    return NS.Statement(scene.name, s64, s32, scene.m, float(CS.unsafe_mask(scene, window).double().mean()))


# ---- poses: registration on the oracle chain ---------------------------------------------------------------------------------------------
GAIN, BIAS = 1.25, 0.05      # the exposure of the captured clip: clip = GAIN picture + BIAS


def refine_video_setting(Tn=3):
    """camera_statement.refine_setting with a T-frame stack (the stack of test_gpu_camera_grad._model(dev, True))"""
    _, K_plane, depths, E, K, spec = CS.refine_setting()
    g = CS.REFINE
    return synth.make_plane_stack(g["D"], Tn, g["Hs"], g["Ws"], seed=41), K_plane, depths, E, K, spec


def captured_clip(frames, roll=0, gain=1.0, bias=0.0):
    """the clip a camera would have captured of the loop `frames` [T,H,W,3]: started `roll` frames later, exposed by gain and bias"""
    return torch.roll(frames, -roll, 0) * gain + bias


def oracle_system(stack, K_plane, depths, spec, H, W, tgt, dtype, long_exposure, photo):
    """system(extrin, intrin, a, beta) -> (A, b, cost) as float64 host values, formed on the oracle in `dtype`: poses.register_loop's argument"""
    def system(E, K, a, beta):
        homos, dh = NS.oracle_tangents(K_plane, depths, E, K)
        sc = RS.Scene("register", homos, H, W, stack.shape[2], stack.shape[3], spec)
        A, b, cost = evaluate(sc, stack, dh, tgt, None, long_exposure, photo, (a, beta), dtype)
        return A.double(), b.double(), float(cost)
    return system
