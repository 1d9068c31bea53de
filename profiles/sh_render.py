#!/usr/bin/env python3
"""The view-dependent colour head (vl3d_render_sh_fwd / _bwd, render.render_planes_sh) against the direct render (render.render_planes) on the
SAME `stack`, at the stage-1 shapes: the 180 x 320 training crop of a 360 x 640 frame and a whole 720p frame, D = 32, planes 1.6x the frame.

One process; the four legs (direct forward, SH forward, direct forward + backward, SH forward + backward) alternate round by round; every leg is
warmed up at its shape first; a round times ITERS calls between two HIP events, so the figures are device time per call as the user's autograd
call spends it (the gradient buffers' allocation, the clears and the plan kernels of the direct backward included).  Backward = (forward +
backward) - forward of the same round.  Reported: the median over the rounds, the ratio SH / direct, the bytes each SH call must move (texels a
covered sample reads: 64 against 16 per tap) and the atomic bytes per second the SH backward reached (13 floats per tap with a non-zero weight).

    python profiles/sh_render.py [--out profiles/sh_render.json] [--rounds 7] [--iters 20]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scene(Hf, Wf, crop, D, dev):
    """planes 1.6x the Hf x Wf frame, a target camera a few degrees off the reference, `crop` = (h, w, h0, w0) or None for the whole frame ->
    (homos [D,3,3], ray_m [3,3], H, W, spec, Hs, Ws)"""
    from videoloop3d_amd.plane_model import get_new_intrin
    from videoloop3d_amd.render import RenderSpec, sh_ray_matrix
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    Hs, Ws = int(1.6 * Hf), int(1.6 * Wf)
    K = torch.tensor([[0.9 * Wf, 0, Wf / 2], [0, 0.9 * Wf, Hf / 2], [0, 0, 1.0]], dtype=torch.float64)
    K_mpi = get_new_intrin(K, -((Hs - Hf) // 2), -((Ws - Wf) // 2))
    a = np.radians(2.0)
    E = torch.eye(4, dtype=torch.float64)
    E[:3, :3] = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    E[:3, 3] = torch.tensor([0.05, -0.02, 0.01])
    H, W, Kt = Hf, Wf, K
    if crop is not None:
        H, W, h0, w0 = crop
        Kt = get_new_intrin(K, h0, w0)
    depths = make_depths(D, 1.0, 100.0).flip(0).double()
    homos = compute_homography(torch.eye(4, dtype=torch.float64)[None], K_mpi[None], E[None], Kt[None],
                               torch.tensor([0., 0., 1.], dtype=torch.float64).expand(1, D, 3), depths[None])[0].float()
    return homos.to(dev), sh_ray_matrix(E, Kt).to(dev), H, W, RenderSpec.mpv(), Hs, Ws


def covered_samples(homos, H, W, spec, Hs, Ws):
    """(pixel, plane) samples the hard cut keeps: elementwise in float64 on the device (layers.plane_texel_coords forms them with one batched 3 x 3
    product per sample, which at the frame's 29.5 M samples returned a wrong count on the device: observed here, not investigated)"""
    h = homos.double()[:, :, :, None, None]
    y, x = torch.meshgrid(torch.arange(H, device=homos.device, dtype=torch.float64) + spec.pixel_center,
                          torch.arange(W, device=homos.device, dtype=torch.float64) + spec.pixel_center, indexing="ij")
    z = h[:, 2, 0] * x + h[:, 2, 1] * y + h[:, 2, 2]
    tx = (h[:, 0, 0] * x + h[:, 0, 1] * y + h[:, 0, 2]) / z * spec.scale[0] + spec.offset[0]
    ty = (h[:, 1, 0] * x + h[:, 1, 1] * y + h[:, 1, 2]) / z * spec.scale[1] + spec.offset[1]
    return int(((tx >= 0) & (tx <= Ws - 1) & (ty >= 0) & (ty <= Hs - 1)).sum())


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def measure(name, Hf, Wf, crop, D, dev, rounds, iters):
    from videoloop3d_amd import synth
    from videoloop3d_amd.render import render_planes, render_planes_sh
    homos, ray_m, H, W, spec, Hs, Ws = scene(Hf, Wf, crop, D, dev)
    stack = synth.make_plane_stack(D, 1, Hs, Ws, seed=2, device=dev).requires_grad_(True)
    sh = ((synth.hash_uniform((D, 1, Hs, Ws, 3, 4), seed=3, device=dev) - 0.5) * 0.5)
    sh[..., 3] = 0
    sh.requires_grad_(True)
    g_rgb = synth.hash_uniform((1, H, W, 3), seed=5, device=dev) - 0.5

    def d_fwd():
        with torch.no_grad():
            render_planes(stack, homos, H, W, spec)

    def s_fwd():
        with torch.no_grad():
            render_planes_sh(stack, sh, homos, ray_m, H, W, spec)

    def d_both():
        rgb, _ = render_planes(stack, homos, H, W, spec)
        torch.autograd.grad(rgb, stack, g_rgb)

    def s_both():
        rgb, _ = render_planes_sh(stack, sh, homos, ray_m, H, W, spec)
        torch.autograd.grad(rgb, [stack, sh], g_rgb)

    legs = {"direct_fwd": d_fwd, "sh_fwd": s_fwd, "direct_fwd_bwd": d_both, "sh_fwd_bwd": s_both}
    for fn in legs.values():                      # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t[k].append(timed(fn, iters))
    med = {k: statistics.median(v) for k, v in t.items()}
    d_bwd = statistics.median(b - f for b, f in zip(t["direct_fwd_bwd"], t["direct_fwd"]))
    s_bwd = statistics.median(b - f for b, f in zip(t["sh_fwd_bwd"], t["sh_fwd"]))
    n_cov = covered_samples(homos, H, W, spec, Hs, Ws)
    atomic_bytes = n_cov * 4 * 13 * 4
    return {"case": name, "D": D, "planes": [Hs, Ws], "view": [H, W], "covered_samples": n_cov, "rounds": rounds, "iters_per_round": iters,
            "ms": {"direct_fwd": med["direct_fwd"], "sh_fwd": med["sh_fwd"], "direct_bwd": d_bwd, "sh_bwd": s_bwd},
            "ms_min_max": {k: [min(v), max(v)] for k, v in t.items()},
            "ratio_sh_over_direct": {"fwd": med["sh_fwd"] / med["direct_fwd"], "bwd": s_bwd / d_bwd},
            "tap_bytes_read": {"direct": n_cov * 4 * 16, "sh": n_cov * 4 * 64},
            "sh_bwd_atomic_bytes": atomic_bytes, "sh_bwd_atomic_GB_per_s": atomic_bytes / (s_bwd * 1e-3) / 1e9,
            "sh_bwd_cleared_bytes": D * Hs * Ws * 64}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sh_render.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profiles/sh_render.py measures on the MI355X: no GPU found")
    import __graft_entry__ as g
    g.build()
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0),
           "cases": [measure("crop 180x320 of 360x640", 360, 640, (180, 320, 90, 160), 32, dev, a.rounds, a.iters),
                     measure("frame 720x1280", 720, 1280, None, 32, dev, a.rounds, a.iters)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for c in out["cases"]:
        print(json.dumps({k: c[k] for k in ("case", "ms", "ratio_sh_over_direct", "sh_bwd_atomic_GB_per_s")}))


if __name__ == "__main__":
    main()
