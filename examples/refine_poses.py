#!/usr/bin/env python3
"""Photometric pose refinement on the camera-differentiable render (videoloop3d_amd/poses.py, PlaneModel.render_cameras).

A synthetic static model (MPMesh, D planes of a hash-noise texture), `views` true cameras around the benchmark camera; the targets are the
model's own pictures from the true cameras; the cameras handed to the refinement are the true ones perturbed by a known twist xi (rotation
vector, translation); Adam on one CameraDeltas, the stack frozen.  Prints the rotation and translation error of every view before and after,
and the refinement's steps per second.

    python examples/refine_poses.py [--views 3] [--steps 60] [--planes 4] [--frame 33 131] [--scale 1e-4] [--lr 5e-5] [--method adam|gn]

--method gn: Levenberg-Marquardt on the normal equations of the render kernels (poses.refine_cameras_gn, --gn-steps of them, no learning rate)
instead of Adam: the same scene and the same prints, then both methods timed in the same run -- the steps and the wall time each takes until
every view's rotation and translation error is at a tenth of its start.

The default perturbation moves a pixel by 0.14 px at the most: inside the basin of a noise texture, whose photometric error is convex over a
fraction of a texel only.  Real textures are smooth over many pixels and take larger perturbations; this example checks the machinery."""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def time_to_a_tenth(model, targets, start, Ks, true_E, steps, lr, gn_steps, damping=1e-3):
    """both methods on the same start: (steps, seconds) until every view's rotation and translation error is at most a tenth of its start, or
    (None, None).  Adam refines the views together (one poses.refine_loop: its render callback sees the cameras of every step); the
    Levenberg-Marquardt blocks are independent and run one after the other (poses.gn_loop per view: steps and seconds add up)."""
    from videoloop3d_amd import poses
    V, _, H, W = (int(v) for v in targets.shape[:4])
    r0, t0 = poses.pose_error(start, true_E)

    def reached(E, v=slice(None)):
        r, t = poses.pose_error(E, true_E[v])
        return bool((r <= 0.1 * r0[v]).all() and (t <= 0.1 * t0[v]).all())

    seen = []

    def render(E, K):
        torch.cuda.synchronize()
        seen.append((time.perf_counter(), E.detach().clone()))
        return model.render_cameras(H, W, E, K)[0]

    was = model.stack.requires_grad
    model.stack.requires_grad_(False)
    try:
        poses.refine_loop(render, targets.reshape(V, H, W, 3).to(model.stack.device), start, Ks, steps, lr)
    finally:
        model.stack.requires_grad_(was)
    adam = next(((i, t - seen[0][0]) for i, (t, E) in enumerate(seen) if reached(E)), (None, None))
    gn_n, gn_s = 0, 0.0
    for v in range(V):
        calls = []

        def system(E, K):
            torch.cuda.synchronize()
            calls.append((time.perf_counter(), E.clone()))
            A, b, cost = model.camera_normal_equations(H, W, E, K, targets[v], learn_focal=False)
            return A.cpu(), b.cpu(), float(cost)

        poses.gn_loop(system, start[v], Ks[v], gn_steps, damping)
        hit = next(((i, t - calls[0][0]) for i, (t, E) in enumerate(calls) if reached(E, v)), None)
        if hit is None:
            return adam, (None, None)
        gn_n, gn_s = gn_n + hit[0], gn_s + hit[1]
    return adam, (gn_n, gn_s)


def run(views=3, steps=60, planes=4, frame=(33, 131), scale=1e-4, lr=5e-5, dev="cuda:0", method="adam", gn_steps=5):
    from videoloop3d_amd import poses, synth
    from videoloop3d_amd.MPI import MPMesh
    dev = torch.device(dev)
    H, W = frame
    args = types.SimpleNamespace(mpi_h_scale=1.2, mpi_w_scale=1.08, mpi_d=planes, atlas_grid_h=1, rgb_mlp_type="direct", rgb_activate="sigmoid",
                                 alpha_activate="sigmoid", bg_color="", learn_loop_mask=False, upsample_stage="")
    _, K, E, _ = synth.make_cameras(H, W, dtype=torch.float64)
    model = MPMesh(args, H, W, np.eye(4), K.numpy(), 1.0, 100.0).to(dev)
    with torch.no_grad():
        model.stack.copy_(synth.make_plane_stack(*model.stack.shape[:4], seed=41))
    # the true cameras: the benchmark camera with its translation turned a little per view
    true_E = []
    for v in range(views):
        e = E.clone()
        a = 2 * np.pi * v / max(views, 1)
        e[:3, 3] = torch.tensor([0.03 * np.cos(a), 0.03 * np.sin(a), 0.0], dtype=torch.float64)
        true_E.append(e)
    true_E, Ks = torch.stack(true_E), K.expand(views, 3, 3).clone()
    with torch.no_grad():
        targets = model.render_cameras(H, W, true_E, Ks)[0].reshape(views, 1, H, W, 3).clone()
    xi = torch.tensor([4.0, -3.0, 5.0, 6.0, -4.0, 3.0], dtype=torch.float64) * scale
    signs = torch.tensor([[1.0 if (v >> k) & 1 == 0 else -1.0 for k in range(6)] for v in range(views)], dtype=torch.float64)
    start = poses.se3_exp(xi[None] * signs) @ true_E
    r0, t0 = poses.pose_error(start, true_E)
    if method == "gn":
        return run_gn(model, targets, start, Ks, true_E, steps, lr, gn_steps)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    refined, _, hist = poses.refine_cameras(model, targets, start, Ks, steps=steps, lr=lr)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    r1, t1 = poses.pose_error(refined, true_E)
    for v in range(views):
        print(f"view {v}: rotation error {float(r0[v]):.3e} -> {float(r1[v]):.3e} rad, translation error {float(t0[v]):.3e} -> {float(t1[v]):.3e}")
    print(f"loss {hist[0]:.3e} -> {hist[-1]:.3e}; {steps / dt:.1f} steps/s ({views} views of {H} x {W}, D = {planes}, planes {tuple(model.stack.shape[2:4])})")
    return {"rotation_before": r0.tolist(), "rotation_after": r1.tolist(), "translation_before": t0.tolist(), "translation_after": t1.tolist(),
            "loss_first": hist[0], "loss_last": hist[-1], "steps_per_s": steps / dt}


def run_gn(model, targets, start, Ks, true_E, steps, lr, gn_steps):
    from videoloop3d_amd import poses
    views, _, H, W = (int(v) for v in targets.shape[:4])
    r0, t0 = poses.pose_error(start, true_E)
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    refined, _, hist, cov = poses.refine_cameras_gn(model, targets, start, Ks, steps=gn_steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t_start
    r1, t1 = poses.pose_error(refined, true_E)
    for v in range(views):
        print(f"view {v}: rotation error {float(r0[v]):.3e} -> {float(r1[v]):.3e} rad, translation error {float(t0[v]):.3e} -> {float(t1[v]):.3e}")
    first, last = sum(h[0] for h in hist), sum(min(h) for h in hist)
    print(f"cost {first:.3e} -> {last:.3e}; {views * gn_steps / dt:.1f} steps/s ({views} views of {H} x {W}, D = {model.stack.shape[0]}, "
          f"planes {tuple(model.stack.shape[2:4])}); largest standard deviation of a pose parameter {float(torch.sqrt(torch.diagonal(cov, dim1=1, dim2=2)).max()):.2e}")
    (an, asec), (gn, gsec) = time_to_a_tenth(model, targets, start, Ks, true_E, steps, lr, gn_steps)
    fmt = lambda n, s: "not reached" if n is None else f"{n} steps, {1e3 * s:.1f} ms"      # noqa: E731
    print(f"to a tenth of the starting error: adam (lr {lr:g}, {steps} steps at the most) {fmt(an, asec)}; gn ({gn_steps} steps per view at the most) {fmt(gn, gsec)}")
    return {"rotation_before": r0.tolist(), "rotation_after": r1.tolist(), "translation_before": t0.tolist(), "translation_after": t1.tolist(),
            "cost_first": first, "cost_last": last, "steps_per_s": views * gn_steps / dt, "adam_to_a_tenth": {"steps": an, "seconds": asec},
            "gn_to_a_tenth": {"steps": gn, "seconds": gsec}}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--planes", type=int, default=4)
    ap.add_argument("--frame", type=int, nargs=2, default=(33, 131))
    ap.add_argument("--scale", type=float, default=1e-4)
    ap.add_argument("--lr", type=float, default=5e-5)
    ap.add_argument("--method", choices=("adam", "gn"), default="adam")
    ap.add_argument("--gn-steps", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.views, a.steps, a.planes, tuple(a.frame), a.scale, a.lr, method=a.method, gn_steps=a.gn_steps)))
