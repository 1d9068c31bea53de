"""The statement of stage 1's view-dependent colour head (rgb_mlp_type = 'rgb_sh'; MPI.py:512-537, utils_mpi.py:50-61, 365-383), in plain torch
on the oracle's public pieces (oracle/mpi_oracle.py), float64 when its inputs are.  TEST INFRASTRUCTURE ONLY.

    d = normalize(M (x, y, 1)^T) for the INTEGER pixel indices of the image (utils.py:182-193),  M = inverse(E)[:3,:3] inverse(K)
    b = (C0, -C1 d_y, C1 d_z, -C1 d_x)
    per plane: pre_c = sum_k b_k sample(coef_{c,k}),  pre_a = sample(alpha);  rgba = (rgb_act(pre_rgb), alpha_act(pre_a)) x coverage
    front-to-back composite (MO.overcompose), or the hit-slot layers of the regularisers (MO.layers_to_slots)

Storage as the product holds it: stack (D,1,Hs,Ws,4) = (R0, G0, B0, alpha logit), stack_sh (D,1,Hs,Ws,3,4) with stack_sh[..., k - 1, c] coefficient
k = 1..3 of colour c."""
import dataclasses
import math

import torch

from oracle import mpi_oracle as MO

C0, C1 = 0.28209479177387814, 0.4886025119029199      # utils_mpi.py:321-322


def head(feat, dirs):
    """SphericalHarmoic_RGB(13, 3) restated: feat [N,13] in the REFERENCE's channel order (4 c + k; 12 = alpha), unit dirs [N,3] -> [N,4]"""
    b = torch.stack([torch.full_like(dirs[:, 0], C0), -C1 * dirs[:, 1], C1 * dirs[:, 2], -C1 * dirs[:, 0]], -1)      # N,4
    rgb = (feat[:, :12].reshape(-1, 3, 4) * b[:, None, :]).sum(-1)
    return torch.cat([rgb, feat[:, 12:]], -1)


def ray_matrix(extrin, intrin):
    """float64 M = inverse(E)[:3,:3] inverse(K)"""
    return torch.linalg.inv(extrin.double())[:3, :3] @ torch.linalg.inv(intrin.double())


def ray_dirs(ray_m, H, W, row0=0, col0=0):
    y, x = torch.meshgrid(torch.arange(H, dtype=ray_m.dtype) + row0, torch.arange(W, dtype=ray_m.dtype) + col0, indexing="ij")
    d = torch.stack([x, y, torch.ones_like(x)], -1) @ ray_m.T
    return d / d.norm(dim=-1, keepdim=True)


def basis(ray_m, H, W, row0=0, col0=0):
    d = ray_dirs(ray_m, H, W, row0, col0)
    return torch.stack([torch.full_like(d[..., 0], C0), -C1 * d[..., 1], C1 * d[..., 2], -C1 * d[..., 0]], -1)      # H,W,4


def layers(stack, stack_sh, homos, ray_m, H, W, spec, quad_keep=None):
    """-> (plane-indexed layers [1,H,W,D,4], covered [H,W,D] bool): four MO.sample_layers calls with identity activations, contracted with the
    basis, then the activations times the coverage."""
    assert spec.act_order == "post" and spec.border == "hardcut" and spec.coord_mode == "affine"
    ident = dataclasses.replace(spec, rgb_act="none", alpha_act="none")
    s0, cov = MO.sample_layers(stack, homos, H, W, ident, quad_keep)                      # 1,H,W,D,4 (already times the coverage)
    b = basis(ray_m.to(stack.dtype), H, W)[None, :, :, None, :]                          # 1,H,W,1,4
    pre_rgb = s0[..., :3] * b[..., 0:1]
    for k in range(3):
        sk, _ = MO.sample_layers(stack_sh[..., k, :], homos, H, W, ident, quad_keep)
        pre_rgb = pre_rgb + sk[..., :3] * b[..., k + 1:k + 2]
    c = cov[None, ..., None].to(stack.dtype)
    out = torch.cat([MO.ACTS[spec.rgb_act](pre_rgb), MO.ACTS[spec.alpha_act](s0[..., 3:])], -1) * c
    return out, cov


def render(stack, stack_sh, homos, ray_m, H, W, spec, quad_keep=None):
    """-> (rgb [1,H,W,3], alpha [1,H,W], alpha_sums [1,H,W,2], layers, covered)"""
    lay, cov = layers(stack, stack_sh, homos, ray_m, H, W, spec, quad_keep)
    rgb, bw = MO.overcompose(lay[..., 3], lay[..., :3])
    a = lay[..., 3]
    return rgb, bw.sum(-1), torch.stack([a.sum(-1), (a * a).sum(-1)], -1), lay, cov


def extras(lay, cov, alpha, mpi_d):
    """the reference's regulariser formulas (MPI.py:603-623, 647-650) on the statement's SLOT layers -> dict of scalars"""
    mpi = MO.layers_to_slots(lay, cov)
    a = mpi[..., -1]
    out = {"sparsity": (a.norm(dim=-1, p=1) / a.norm(dim=-1, p=2).clamp_min(1e-6)).mean() / math.sqrt(mpi_d)}
    c = mpi[..., :-1]
    denorm = mpi.shape[-2] / mpi_d
    out["rgb_smooth"] = ((c[:, :, :-1] - c[:, :, 1:]).abs().mean() + (c[:, :-1] - c[:, 1:]).abs().mean()) * denorm
    out["a_smooth"] = ((a[:, :, :-1] - a[:, :, 1:]).abs().mean() + (a[:, :-1] - a[:, 1:]).abs().mean()) * denorm
    out["density"] = (alpha - 1).abs().mean()
    return out
