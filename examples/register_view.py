#!/usr/bin/env python3
"""Registering a captured view against a video model (videoloop3d_amd/poses.py: register_cameras).

A synthetic video model (MPMeshVid, D planes of a hash-noise texture, `frames` loop frames) and one view: its clip is rendered at the true
camera, then made into what a camera would have captured -- started `--start` frames into the loop, `--periods` whole loop periods long, and
exposed by `--gain` x + `--bias`.  The camera handed to the registration is the true one perturbed by a known twist.  Prints the rotation and
translation error and the steps per second of
  * poses.refine_cameras_gn on the first loop period of the clip, frame for frame: the per-frame residual has no meaning against a clip
    started at another time, and the exposure is absorbed into the pose;
  * poses.register_cameras: the long exposure of the render against the long exposure of the clip, with a log gain and a bias per view.

    python examples/register_view.py [--frames 3] [--start 1] [--periods 2] [--gain 1.25] [--bias 0.05] [--steps 8] [--planes 4]
                                     [--frame 33 131] [--scale 1e-4]

The long exposure of a clip equals the loop's only when the clip spans whole loop periods (`--periods`): a caveat of the method.  The default
perturbation stays inside the basin of a noise texture (examples/refine_poses.py)."""
import argparse
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def run(frames=3, start_frame=1, periods=2, gain=1.25, bias=0.05, steps=8, planes=4, frame=(33, 131), scale=1e-4, dev="cuda:0"):
    from videoloop3d_amd import poses, synth
    from videoloop3d_amd.MPV import MPMeshVid
    dev = torch.device(dev)
    H, W = frame
    args = types.SimpleNamespace(mpi_h_scale=1.2, mpi_w_scale=1.08, mpi_d=planes, atlas_grid_h=1, rgb_mlp_type="direct", rgb_activate="sigmoid",
                                 alpha_activate="sigmoid", bg_color="", learn_loop_mask=False, upsample_stage="", sparsity_loss_weight=0.0,
                                 rgb_smooth_loss_weight=0.0, a_smooth_loss_weight=0.0, density_loss_weight=0.0, d_smooth_loss_weight=0.0,
                                 l_smooth_loss_weight=0.0, mpv_frm_num=frames, mpv_isloop=True, init_std=0.5, scale_invariant=True, add_uv_noise=False,
                                 fp16=False, normalize_verts=False, atlas_cnl=4, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1)
    _, K, E, _ = synth.make_cameras(H, W, dtype=torch.float64)
    model = MPMeshVid(args, H, W, np.eye(4), K.numpy(), 1.0, 100.0).to(dev)
    with torch.no_grad():
        model.stack.copy_(synth.make_plane_stack(*model.stack.shape[:4], seed=41))
        loop = model.render_cameras(H, W, E[None], K[None])[0].clone()      # [frames,H,W,3] at the true camera
    clip = torch.roll(loop, -int(start_frame), 0).repeat(int(periods), 1, 1, 1) * gain + bias      # what the camera captured
    xi = torch.tensor([4.0, -3.0, 5.0, 6.0, -4.0, 3.0], dtype=torch.float64) * scale
    start = poses.se3_exp(xi) @ E
    r0, t0 = (float(v) for v in poses.pose_error(start, E))
    out = {"rotation_before": r0, "translation_before": t0}

    def timed(fn, n):
        torch.cuda.synchronize()
        t_start = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, n / (time.perf_counter() - t_start)

    # one system of each kind before the clock starts: the first call loads the kernels' code objects
    model.camera_normal_equations(H, W, start, K, clip[:frames])
    model.camera_register_equations(H, W, start, K, clip.mean(0), long_exposure=True, brightness=(0.0, 0.0))
    (E_gn, _, hist, _), sps = timed(lambda: poses.refine_cameras_gn(model, clip[None, :frames], start[None], K[None], steps=steps), steps)
    r1, t1 = (float(v) for v in poses.pose_error(E_gn[0], E))
    print(f"refine_cameras_gn (per frame, no brightness): rotation error {r0:.3e} -> {r1:.3e} rad, translation error {t0:.3e} -> {t1:.3e}; "
          f"cost {hist[0][0]:.3e} -> {min(hist[0]):.3e}; {sps:.1f} steps/s")
    out["refine_cameras_gn"] = {"rotation_after": r1, "translation_after": t1, "steps_per_s": sps}
    reg, sps = timed(lambda: poses.register_cameras(model, [clip], start[None], K[None], steps=steps), steps)
    r2, t2 = (float(v) for v in poses.pose_error(reg.extrinsics[0], E))
    print(f"register_cameras (long exposure, brightness fit): rotation error {r0:.3e} -> {r2:.3e} rad, translation error {t0:.3e} -> {t2:.3e}; "
          f"cost {reg.costs[0][0]:.3e} -> {min(reg.costs[0]):.3e}; gain {float(torch.exp(reg.log_gain[0])):.5f} (true {gain}), bias {float(reg.bias[0]):.5f} "
          f"(true {bias}); {sps:.1f} steps/s ({len(clip)} captured frames of {H} x {W} against {frames} loop frames, D = {planes})")
    out["register_cameras"] = {"rotation_after": r2, "translation_after": t2, "gain": float(torch.exp(reg.log_gain[0])), "bias": float(reg.bias[0]),
                               "steps_per_s": sps}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--start", type=int, default=1)
    ap.add_argument("--periods", type=int, default=2)
    ap.add_argument("--gain", type=float, default=1.25)
    ap.add_argument("--bias", type=float, default=0.05)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--planes", type=int, default=4)
    ap.add_argument("--frame", type=int, nargs=2, default=(33, 131))
    ap.add_argument("--scale", type=float, default=1e-4)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.frames, a.start, a.periods, a.gain, a.bias, a.steps, a.planes, tuple(a.frame), a.scale)))
