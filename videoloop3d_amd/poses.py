"""Camera refinement on the camera-differentiable render (render.render_planes with `homos.requires_grad`, PlaneModel.render_cameras).

The inputs of this method are asynchronous hand-held captures whose poses come from COLMAP; both stages take them as given.  A photometric
refinement needs d loss / d homographies from the render kernels (vl3d_render_bwd_homos) and, on the host, the small differentiable chain
pose -> homographies (utils_mpi.compute_homography, plain torch as in the reference).  Everything here is host-side float64 torch: a pose is
six numbers.

Second order: the render kernels also form the normal equations of the photometric residual in the camera parameters (vl3d_render_cam_normal
from the tangents of the homographies, camera_tangents), and refine_cameras_gn takes Levenberg-Marquardt steps on them -- no learning rate,
and a pose covariance at the end.

Captured clips: a clip of a view is the same loop started at an unknown time and exposed differently, so a per-frame residual against it has no
meaning and a brightness offset would be absorbed into the pose.  register_cameras fits the temporal mean of the rendered frames to the temporal
mean of the clip (stage 1's statistic, train_3d.py:52-56) with a log gain and a bias per view (train_3d.py:217, MPV.py:499-504), on the normal
equations of vl3d_render_cam_register."""
import dataclasses

import torch
import torch.nn as nn


def _hat(w):
    """[..., 3] -> the cross-product matrices [..., 3, 3]"""
    z = torch.zeros_like(w[..., 0])
    return torch.stack([torch.stack([z, -w[..., 2], w[..., 1]], -1), torch.stack([w[..., 2], z, -w[..., 0]], -1),
                        torch.stack([-w[..., 1], w[..., 0], z], -1)], -2)


def se3_exp(xi):
    """the exponential of the twist xi [..., 6] = (rotation vector w, translation v) -> [..., 4, 4] in float64: exp [[w^, v], [0, 0]] =
    [[R, V v], [0, 1]] with R = I + A w^ + B w^2, V = I + B w^ + C w^2, A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3, t = |w|.
    Differentiable everywhere: below t^2 = 1e-4 the three coefficients are their series in t^2 (next term below 3e-16), so neither the value
    nor the gradient divides by t at 0."""
    xi = xi.to(torch.float64)
    w, v = xi[..., :3], xi[..., 3:]
    t2 = (w * w).sum(-1)
    small = t2 < 1e-4
    t2s = torch.where(small, torch.ones_like(t2), t2)      # (the closed forms are evaluated away from 0 only: no NaN in the unused branch's gradient)
    t = torch.sqrt(t2s)
    A = torch.where(small, 1 - t2 / 6 + t2 * t2 / 120 - t2 ** 3 / 5040, torch.sin(t) / t)
    B = torch.where(small, 0.5 - t2 / 24 + t2 * t2 / 720 - t2 ** 3 / 40320, (1 - torch.cos(t)) / t2s)
    C = torch.where(small, 1.0 / 6 - t2 / 120 + t2 * t2 / 5040 - t2 ** 3 / 362880, (t - torch.sin(t)) / (t2s * t))
    W = _hat(w)
    W2 = W @ W
    eye = torch.eye(3, dtype=torch.float64, device=xi.device).expand(W.shape)
    R = eye + A[..., None, None] * W + B[..., None, None] * W2
    V = eye + B[..., None, None] * W + C[..., None, None] * W2
    top = torch.cat([R, V @ v[..., None]], -1)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=xi.device).expand(top.shape[:-2] + (1, 4))
    return torch.cat([top, bottom], -2)


def pose_error(extrin, true_extrin):
    """(rotation angle in radians, translation norm) of extrin @ inverse(true_extrin), float64"""
    r = torch.as_tensor(extrin).to(torch.float64) @ torch.inverse(torch.as_tensor(true_extrin).to(torch.float64))
    cos = ((r[..., 0, 0] + r[..., 1, 1] + r[..., 2, 2]) - 1) / 2
    skew = torch.stack([r[..., 2, 1] - r[..., 1, 2], r[..., 0, 2] - r[..., 2, 0], r[..., 1, 0] - r[..., 0, 1]], -1).norm(dim=-1) / 2
    return torch.atan2(skew, cos), r[..., :3, 3].norm(dim=-1)


class CameraDeltas(nn.Module):
    """per-view corrections of given cameras: a twist xi [V,6] (float64, on the host, zero at the start) applied on the left of the extrinsics,
    and with `learn_focal` a log focal scale per view."""

    def __init__(self, n_views, learn_focal=False):
        super().__init__()
        self.xi = nn.Parameter(torch.zeros((int(n_views), 6), dtype=torch.float64))
        self.log_focal = nn.Parameter(torch.zeros(int(n_views), dtype=torch.float64)) if learn_focal else None

    def extrins(self, base, idx=None):
        """se3_exp(xi[idx]) @ base[idx]: base [V,4,4] -> [len(idx),4,4] float64"""
        idx = torch.arange(len(self.xi)) if idx is None else torch.as_tensor(idx, dtype=torch.long)
        return se3_exp(self.xi[idx]) @ torch.as_tensor(base).to(torch.float64)[idx]

    def intrins(self, base, idx=None):
        """base [V,3,3] with the focal entries (the upper-left 2 x 2 block) scaled by exp(log_focal[idx]) -> [len(idx),3,3] float64"""
        idx = torch.arange(len(self.xi)) if idx is None else torch.as_tensor(idx, dtype=torch.long)
        K = torch.as_tensor(base).to(torch.float64)[idx]
        if self.log_focal is None:
            return K
        s = torch.exp(self.log_focal[idx])[:, None, None]
        block = torch.zeros((3, 3), dtype=torch.float64)
        block[:2, :2] = 1
        return K * (1 + block * (s - 1))


def refine_loop(render, targets, extrins, intrins, steps=60, lr=5e-5, learn_focal=False, params=()):
    """Adam on a CameraDeltas over `render(extrins [V,4,4], intrins [V,3,3]) -> rgb`, a picture shaped like `targets`: the mean squared error
    against `targets`.  `params`: further tensors to train beside the cameras (the stack), at the same rate.
    -> (refined extrinsics [V,4,4], refined intrinsics [V,3,3], losses [steps]) -- float64 host tensors and a list of floats."""
    extrins, intrins = torch.as_tensor(extrins).detach().cpu().to(torch.float64), torch.as_tensor(intrins).detach().cpu().to(torch.float64)
    deltas = CameraDeltas(len(extrins), learn_focal)
    groups = [dict(params=list(deltas.parameters()), lr=lr)]
    if len(params):
        groups.append(dict(params=list(params), lr=lr))
    opt = torch.optim.Adam(groups)
    history = []
    for _ in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        rgb = render(deltas.extrins(extrins), deltas.intrins(intrins))
        loss = ((rgb - targets) ** 2).mean()
        loss.backward()
        opt.step()
        history.append(loss.detach().item())
    with torch.no_grad():
        return deltas.extrins(extrins).clone(), deltas.intrins(intrins).clone(), history


def refine_cameras(model, targets, extrins, intrins, ts=None, steps=60, lr=5e-5, train_stack=False, crop=None, learn_focal=False):
    """Photometric refinement of the cameras of a PlaneModel (MPMesh / MPMeshVid): Adam on a CameraDeltas, the mean squared error of
    model.render_cameras against `targets` [V,T',H,W,3] (T' = the frames `ts`; 1 for a static model).  extrins [V,4,4] (ref -> target) and
    intrins [V,3,3]: the cameras to start from.  The stack is frozen unless `train_stack` (then trained beside the cameras, at `lr`).  crop (row0, col0, h, w): compare that window of the frames only (a shifted principal point, utils.py:196-200).
    -> (refined extrinsics [V,4,4], refined intrinsics [V,3,3], loss history) -- float64 host tensors and a list of floats."""
    from .plane_model import get_new_intrin
    V, Tn, H, W = (int(v) for v in targets.shape[:4])
    dev = model.stack.device
    tgt = targets.to(dev, torch.float32)
    r0 = c0 = 0
    if crop is not None:
        r0, c0, H, W = (int(v) for v in crop)
        tgt = tgt[:, :, r0:r0 + H, c0:c0 + W]
    tgt = tgt.reshape(V * Tn, H, W, 3)

    def render(E, K):
        return model.render_cameras(H, W, E, get_new_intrin(K, r0, c0), ts=ts)[0]

    stack = model.stack
    was = stack.requires_grad
    stack.requires_grad_(bool(train_stack))
    try:
        return refine_loop(render, tgt, extrins, intrins, steps, lr, learn_focal, [stack] if train_stack else ())
    finally:
        stack.requires_grad_(was)


# ---- Gauss-Newton / Levenberg-Marquardt on the normal equations of the render (vl3d_render_cam_normal) ---------------------------------
def _focal_scaled(K, log_focal):
    """K [3,3] with the focal entries (the upper-left 2 x 2 block) scaled by exp(log_focal): CameraDeltas.intrins' rule for one view"""
    block = torch.zeros((3, 3), dtype=torch.float64)
    block[:2, :2] = 1
    return K * (1 + block * (torch.exp(log_focal) - 1))


def camera_tangents(model, extrin, intrin, learn_focal=False):
    """The homographies of one view of a PlaneModel and their tangents in the camera parameters theta = (left twist xi in R^6[, log focal
    scale]) at theta = 0: E(theta) = se3_exp(xi) E, the focal entries of K scaled by exp(log focal) as CameraDeltas.intrins scales them.
    extrin [4,4] (ref -> target), intrin [3,3].  The Jacobian of the model's float64 homography chain (PlaneModel.homography_chain) on the
    host, by forward-mode autograd, rounded to float32 once.
    -> (homos [D,3,3] float32, dhomos [P,D,3,3] float32), P = 6 or 7: what render.render_normal_equations takes."""
    E = torch.as_tensor(extrin).detach().cpu().to(torch.float64).reshape(4, 4)
    K = torch.as_tensor(intrin).detach().cpu().to(torch.float64).reshape(3, 3)
    P = 7 if learn_focal else 6

    def chain(theta):
        Kt = _focal_scaled(K, theta[6]) if learn_focal else K
        return model.homography_chain((se3_exp(theta[:6]) @ E)[None], Kt[None])

    theta0 = torch.zeros(P, dtype=torch.float64)
    with torch.enable_grad():
        jac = torch.autograd.functional.jacobian(chain, theta0, vectorize=True, strategy="forward-mode")      # [D,3,3,P]
    with torch.no_grad():
        homos = chain(theta0)
    return homos.float(), jac.permute(3, 0, 1, 2).contiguous().float()


def gn_loop(system, extrin, intrin, steps=5, damping=1e-3, learn_focal=False):
    """Levenberg-Marquardt on one camera over `system(extrin [4,4], intrin [3,3]) -> (A [P,P], b [P], cost)`, the normal equations of a
    residual in theta = (left twist[, log focal scale]) at that camera (float64 host tensors and a float).  Per step
    delta = -(A + lambda diag A)^-1 b, E <- se3_exp(delta_xi) E, the focal entries scaled by exp(delta_f).  lambda starts at `damping`; a step
    whose cost is not below the last accepted one is undone and lambda multiplied by 10, an accepted step divides it by 10, down to `damping`.
    -> (extrin, intrin, costs: the cost at every evaluated point, A and cost at the last accepted point)."""
    E, K = extrin, intrin
    A, b, cost = system(E, K)
    costs, lam = [cost], float(damping)
    for _ in range(int(steps)):
        delta = -torch.linalg.solve(A + lam * torch.diag(torch.diagonal(A)), b)
        E_try = se3_exp(delta[:6]) @ E
        K_try = _focal_scaled(K, delta[6]) if learn_focal else K
        A_try, b_try, cost_try = system(E_try, K_try)
        costs.append(cost_try)
        if cost_try < cost:
            E, K, A, b, cost = E_try, K_try, A_try, b_try, cost_try
            lam = max(lam / 10, float(damping))
        else:      # undone: the same point, more damping
            lam *= 10
    return E, K, costs, A, cost


def refine_cameras_gn(model, targets, extrins, intrins, ts=None, steps=5, damping=1e-3, learn_focal=False, crop=None, weight=None):
    """Photometric refinement of the cameras of a PlaneModel by Levenberg-Marquardt (gn_loop) on the normal equations the render kernels
    form (PlaneModel.camera_normal_equations): no learning rate.  targets [V,T',H,W,3], extrins [V,4,4], intrins [V,3,3], `ts`, `crop` as
    refine_cameras takes them; weight [V,T',H,W] or None: per-pixel weights of the residual (cropped like the targets).  The views are
    independent blocks and run one after the other, in float64 on the host.  The stack is frozen and untouched.
    -> (extrinsics [V,4,4], intrinsics [V,3,3], cost history per view (a list of lists: the cost at every evaluated point), covariance [V,P,P])
    -- float64 host tensors; covariance = sigma^2 A^-1 at the last accepted point, sigma^2 = cost / (N - P), N the count of weighted residuals
    (pixels of non-zero weight x 3 colour channels; without weights frames x pixels x 3)."""
    from .plane_model import get_new_intrin
    extrins = torch.as_tensor(extrins).detach().cpu().to(torch.float64).reshape(-1, 4, 4).clone()
    intrins = torch.as_tensor(intrins).detach().cpu().to(torch.float64).reshape(-1, 3, 3).clone()
    V, Tn, H, W = (int(v) for v in targets.shape[:4])
    if len(extrins) != V or len(intrins) != V:
        raise RuntimeError(f"refine_cameras_gn: {V} views of targets, {len(extrins)} extrinsics and {len(intrins)} intrinsics")
    dev = model.stack.device
    tgt = torch.as_tensor(targets).to(dev, torch.float32)
    wgt = None if weight is None else torch.as_tensor(weight).to(dev, torch.float32)
    r0 = c0 = 0
    if crop is not None:
        r0, c0, H, W = (int(v) for v in crop)
        tgt = tgt[:, :, r0:r0 + H, c0:c0 + W]
        wgt = None if wgt is None else wgt[:, :, r0:r0 + H, c0:c0 + W]
    P = 7 if learn_focal else 6
    history, covs = [], []
    for v in range(V):
        t_v, w_v = tgt[v].contiguous(), None if wgt is None else wgt[v].contiguous()
        n_res = 3.0 * (float(Tn * H * W) if w_v is None else float((w_v != 0).sum()))

        def system(E, K):
            A, b, cost = model.camera_normal_equations(H, W, E, get_new_intrin(K, r0, c0), t_v, ts=ts, learn_focal=learn_focal, weight=w_v)
            return A.cpu(), b.cpu(), float(cost)

        extrins[v], intrins[v], costs, A, cost = gn_loop(system, extrins[v], intrins[v], steps, damping, learn_focal)
        history.append(costs)
        covs.append(cost / max(n_res - P, 1.0) * torch.linalg.inv(A))
    return extrins, intrins, history, torch.stack(covs)


# ---- registration against a captured clip: long exposure and a brightness fit (vl3d_render_cam_register) ------------------------------------
@dataclasses.dataclass
class Registration:
    """what register_cameras returns, float64 host tensors: extrinsics [V,4,4], intrinsics [V,3,3], log_gain [V] and bias [V] (the clip is
    exp(log_gain) picture + bias; zeros without the brightness fit), costs (per view: the cost at every evaluated point), covariance [V,Q,Q] of
    theta = (twist[, log focal][, log gain, bias]) at the last accepted point."""
    extrinsics: torch.Tensor
    intrinsics: torch.Tensor
    log_gain: torch.Tensor
    bias: torch.Tensor
    costs: list
    covariance: torch.Tensor


def register_loop(system, extrin, intrin, steps=8, damping=1e-3, learn_focal=False, fit_brightness=True, log_gain=0.0, bias=0.0):
    """gn_loop with two more unknowns: Levenberg-Marquardt on one camera and, with `fit_brightness`, the log gain a and the bias beta of its
    clip, over `system(extrin [4,4], intrin [3,3], a, beta) -> (A [Q,Q], b [Q], cost)` in theta = (left twist[, log focal scale][, a, beta])
    at that point (float64 host tensors and a float).  Per step delta = -(A + lambda diag A)^-1 b, E <- se3_exp(delta_xi) E, the focal entries
    scaled by exp(delta_f), a <- a + delta_a, beta <- beta + delta_beta; the accept / reject rule and the damping schedule are gn_loop's.
    -> (extrin, intrin, a, beta, costs: the cost at every evaluated point, A and cost at the last accepted point)."""
    E, K, a, beta = extrin, intrin, float(log_gain), float(bias)
    A, b, cost = system(E, K, a, beta)
    costs, lam = [cost], float(damping)
    n_cam = 7 if learn_focal else 6
    for _ in range(int(steps)):
        delta = -torch.linalg.solve(A + lam * torch.diag(torch.diagonal(A)), b)
        E_try = se3_exp(delta[:6]) @ E
        K_try = _focal_scaled(K, delta[6]) if learn_focal else K
        a_try, beta_try = (a + float(delta[n_cam]), beta + float(delta[n_cam + 1])) if fit_brightness else (a, beta)
        A_try, b_try, cost_try = system(E_try, K_try, a_try, beta_try)
        costs.append(cost_try)
        if cost_try < cost:
            E, K, a, beta, A, b, cost = E_try, K_try, a_try, beta_try, A_try, b_try, cost_try
            lam = max(lam / 10, float(damping))
        else:      # undone: the same point, more damping
            lam *= 10
    return E, K, a, beta, costs, A, cost


def register_cameras(model, clips, extrins, intrins, ts=None, steps=8, damping=1e-3, learn_focal=False, crop=None, weight=None, long_exposure=True,
                     fit_brightness=True):
    """Register the cameras of captured clips against a PlaneModel: refine_cameras_gn for targets that are NOT the model's own frames.  A
    captured clip of a view is the same loop started at an unknown time, possibly with another frame count, and exposed differently, so
      * `long_exposure`: the residual is taken between the temporal mean of the rendered frames (`ts`; None: every frame) and the temporal mean
        of the clip -- clips [V,F,H,W,3] or a list of V clips [F_v,H,W,3], any F.  The two means describe the same picture only when the clip
        spans whole loop periods: a caveat of the method.  Without it the residual is per frame, and F must be the number of rendered frames;
      * `fit_brightness`: a log gain and a bias per view are fitted beside the camera (clip = exp(log_gain) picture + bias), instead of being
        absorbed into the pose.
    Levenberg-Marquardt (register_loop) on PlaneModel.camera_register_equations, the views one after the other, in float64 on the host; the
    stack is frozen and untouched.  weight: per-pixel weights, [V,H,W] with `long_exposure`, else [V,F,H,W]; `crop`, `learn_focal`, `steps`,
    `damping` as refine_cameras_gn takes them.
    -> Registration; covariance = sigma^2 A^-1, sigma^2 = cost / (N - Q), N the count of weighted residuals (pixels of non-zero weight x 3;
    with `long_exposure` the pixels of ONE picture)."""
    from .plane_model import get_new_intrin
    who = "register_cameras"
    extrins = torch.as_tensor(extrins).detach().cpu().to(torch.float64).reshape(-1, 4, 4).clone()
    intrins = torch.as_tensor(intrins).detach().cpu().to(torch.float64).reshape(-1, 3, 3).clone()
    clips = [torch.as_tensor(c) for c in clips] if isinstance(clips, (list, tuple)) else list(torch.as_tensor(clips))
    V = len(clips)
    if len(extrins) != V or len(intrins) != V:
        raise RuntimeError(f"{who}: {V} clips, {len(extrins)} extrinsics and {len(intrins)} intrinsics")
    if weight is not None and len(weight) != V:
        raise RuntimeError(f"{who}: {V} clips and {len(weight)} weight maps")
    dev = model.stack.device
    n_frames = int(model.stack.shape[1]) if ts is None else len(ts)
    P = 7 if learn_focal else 6
    Q = P + (2 if fit_brightness else 0)
    history, covs, gains, biases = [], [], [], []
    for v in range(V):
        clip = clips[v].to(dev, torch.float32)
        if clip.dim() != 4 or clip.shape[-1] != 3 or clip.shape[0] < 1:
            raise RuntimeError(f"{who}: clip {v} must be [F,H,W,3], got {tuple(clip.shape)}")
        if not long_exposure and clip.shape[0] != n_frames:
            raise RuntimeError(f"{who}: without long_exposure clip {v} needs the {n_frames} rendered frames, got {clip.shape[0]}")
        t_v = clip.double().mean(0).float() if long_exposure else clip      # the long exposure: the clip's temporal mean
        w_v = None if weight is None else torch.as_tensor(weight[v]).to(dev, torch.float32)
        H, W = (int(s) for s in clip.shape[1:3])
        r0 = c0 = 0
        if crop is not None:
            r0, c0, H, W = (int(s) for s in crop)
            t_v = t_v[..., r0:r0 + H, c0:c0 + W, :]
            w_v = None if w_v is None else w_v[..., r0:r0 + H, c0:c0 + W]
        t_v, w_v = t_v.contiguous(), None if w_v is None else w_v.contiguous()
        n_res = 3.0 * (float(t_v.numel() // 3) if w_v is None else float((w_v != 0).sum()))

        def system(E, K, a, beta):
            A, b, cost = model.camera_register_equations(H, W, E, get_new_intrin(K, r0, c0), t_v, ts=ts, learn_focal=learn_focal, weight=w_v,
                                                         long_exposure=long_exposure, brightness=(a, beta) if fit_brightness else None)
            return A.cpu(), b.cpu(), float(cost)

        extrins[v], intrins[v], a, beta, costs, A, cost = register_loop(system, extrins[v], intrins[v], steps, damping, learn_focal, fit_brightness)
        history.append(costs)
        gains.append(a)
        biases.append(beta)
        covs.append(cost / max(n_res - Q, 1.0) * torch.linalg.inv(A))
    return Registration(extrins, intrins, torch.tensor(gains, dtype=torch.float64), torch.tensor(biases, dtype=torch.float64), history, torch.stack(covs))
