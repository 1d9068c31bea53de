#!/usr/bin/env python3
"""The evaluation script (scripts/script_evaluate_ours.py) on the device: `videoloop3d_amd.evaluations.evaluate` on a synthetic MPMeshVid at
the reference's factor-2 frames (360 x 640), D = 32, a 50-frame loop, 2 test views with 60-frame gt clips (the model's own loop, its first 10
frames again, plus noise of up to +-6 levels; the left half of every plane is static in time, so the loop mask has a static region).  Prints
one JSON line: the dataset row of metrics.txt and the wall time of each stage (render, loop mask, static + dyn statistics, NN metrics per
patch configuration), of a second run after a warm-up run.  `--gt-y4m A.y4m,B.y4m`: the ground-truth clips come from YUV4MPEG2 files, one per
test view (`y4m.videos_from_y4m`; frames of H x W), instead of the synthetic ones.  Synthetic poses and weights."""
import json
import os
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def run(H=360, W=640, planes=32, frames=50, gt_frames=60, views=2, dev="cuda:0", gt_y4m=None):
    from videoloop3d_amd import evaluations as E
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd import synth
    from videoloop3d_amd.MPV import MPMeshVid
    dev = torch.device(dev)
    gt_clips = None
    if gt_y4m:
        from videoloop3d_amd import y4m
        gt_clips = y4m.videos_from_y4m(gt_y4m, dev)
        views, gt_frames = len(gt_clips), len(gt_clips[0])
        if any(tuple(c.shape[1:3]) != (H, W) for c in gt_clips):
            raise ValueError(f"--gt-y4m: frames of {H} x {W} expected, got {[tuple(c.shape[1:3]) for c in gt_clips]}")
    rng = np.random.RandomState(3)
    rows = []
    for v in range(views):      # an LLFF poses_bounds array of full-resolution (2H x 2W) views: small rotations, positions on an arc
        a, b = np.radians(rng.uniform(-2, 2, 2))
        R = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]) @ np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
        t = np.array([0.3 * np.cos(2 * np.pi * v / views), 0.2 * np.sin(2 * np.pi * v / views), 0.0])
        rows.append(np.concatenate([np.concatenate([R, t[:, None], [[2 * H], [2 * W], [0.9 * 2 * W]]], 1).reshape(-1), [2.0, 50.0]]))
    pb = np.stack(rows)
    args = types.SimpleNamespace(mpv_frm_num=frames, mpv_isloop=True, mpi_h_scale=1.1, mpi_w_scale=1.1, mpi_d=planes, atlas_grid_h=4, init_std=0.5,
                                 rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color="", scale_invariant=True, fp16=False,
                                 swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1, sparsity_loss_weight=0.0, rgb_smooth_loss_weight=0.0,
                                 a_smooth_loss_weight=0.0, density_loss_weight=0.0, d_smooth_loss_weight=0.0, optimizer="adam", lrate=0.1, lrate_decay=30,
                                 factor=2, near_factor=1.0, far_factor=1.0, test_view_idx="")
    poses, intrins, bds, _, _ = RV.load_llff_poses(pb, factor=2)
    ext, K, near, far = RV.reference_camera(poses, intrins, bds)
    model = MPMeshVid(args, H, W, ext, K.astype(np.float64), near, far, device=dev).to(dev)
    with torch.no_grad():
        model.stack.copy_(synth.make_plane_stack(*model.stack.shape[:4], seed=5, device=dev) * 0.8)
        half = model.stack.shape[3] // 2
        model.stack[:, :, :, :half] = model.stack[:, :1, :, :half].clone()
    vext = RV.pose2extrin_np(poses)
    videos = []
    for v in range(0 if gt_clips is None else views, views):
        own = RV.render_frames(model, H, W, np.repeat(vext[v:v + 1], frames, 0), np.repeat(intrins[v:v + 1], frames, 0), np.arange(frames))
        clip = torch.cat([own, own[:gt_frames - frames]]).long()
        noise = (synth.hash_uniform(tuple(clip.shape), 70 + v, device=dev) * 13).long() - 6
        videos.append((clip + noise).clamp(0, 255).to(torch.uint8).cpu().numpy())
    if gt_clips is not None:
        videos = gt_clips
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for rep in range(2):      # the first run warms up (code objects, allocator); the second is reported
            tm = {}
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            res = E.evaluate(model, args, pb, videos, dataname="synthetic", out_dir=d, timings=tm)
            torch.cuda.synchronize(dev)
            total = time.perf_counter() - t0
        lines = open(os.path.join(d, "eval_metrics.txt")).read().splitlines()
    names = lines[0].split(", ")
    out["metrics"] = {k: float(x) for k, x in zip(names[1:], lines[-1].split(", ")[1:])}
    out["stage_ms"] = {k: round(1e3 * s, 3) for k, s in tm.items()}
    out["total_ms"] = round(1e3 * total, 3)
    out["shape"] = (f"{views} views, gt {gt_frames} x {H} x {W}, loop {frames} frames, D={planes}, planes {tuple(model.stack.shape[2:4])}, "
                    f"crop 40 -> {H - 80} x {W - 80}")
    assert len(res) == views
    return out


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--gt-y4m", default=None, metavar="A.y4m,B.y4m", help="ground-truth clips from YUV4MPEG2 files, one per test view")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(gt_y4m=a.gt_y4m)))
