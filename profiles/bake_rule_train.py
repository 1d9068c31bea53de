#!/usr/bin/env python3
"""In-process A/B of a training iteration's render under the bake rule (act_order="baked", include/vl3d.h VL3D_ACT_BAKED) against the
float rule (act_order="post") at cfg3 (D = 32, T = 50, 720p, fp32; docs/kernels/K9_baked_playback.md, "Training under the bake rule").
One resident stack, the same homographies and cotangents; the legs alternate round by round (and their order) under HIP events on the
launch stream, forward (render_planes) and backward (its autograd: vl3d_render_bwd) timed apart.  The "post" leg is the yardstick: the
kernels the parent commit ships, timed in this process.
  python profiles/bake_rule_train.py [--warm 20] [--iters 100] [--rounds 10] [--D 32 --T 50 --H 720 --W 1280] [--f16] [--out FILE]
Prints per leg and direction ms per call (median, min .. max over the rounds), the ratio baked / post, and the kernel family each backward ran."""
import argparse
import dataclasses
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--warm", type=int, default=20)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--rounds", type=int, default=10)
ap.add_argument("--D", type=int, default=32)
ap.add_argument("--T", type=int, default=50)
ap.add_argument("--H", type=int, default=720)
ap.add_argument("--W", type=int, default=1280)
ap.add_argument("--f16", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
assert a.warm >= 1 and a.iters >= a.rounds >= 1

import __graft_entry__ as ge  # noqa: E402
ge.build()
from videoloop3d_amd import render as R  # noqa: E402
from videoloop3d_amd import synth  # noqa: E402
from videoloop3d_amd.utils_mpi import compute_homography, make_depths  # noqa: E402

assert torch.cuda.is_available(), "profiles/bake_rule_train.py measures on the MI355X"
dev = torch.device("cuda:0")
D, T, H, W = a.D, a.T, a.H, a.W
ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
homos = compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3),
                           make_depths(D, 1.0, 100.0).flip(0)[None])[0].to(dev)
stack = synth.make_plane_stack(D, T, H, W, seed=2, device=dev, dtype=torch.float16 if a.f16 else torch.float32).requires_grad_(True)
g_rgb = synth.hash_uniform((T, H, W, 3), seed=5, device=dev) - 0.5
g_a = synth.hash_uniform((T, H, W), seed=6, device=dev) - 0.5
specs = {"post": R.RenderSpec.mpv(), "baked": dataclasses.replace(R.RenderSpec.mpv(), act_order="baked")}
families = {}


def call(leg, ev=None):
    """one forward and one backward of `leg`; ev: a list that receives the (start, mid, end) events of the call"""
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)] if ev is not None else None
    if e:
        e[0].record()
    rgb, alpha = R.render_planes(stack, homos, H, W, specs[leg])
    if e:
        e[1].record()
    torch.autograd.grad([rgb, alpha], stack, [g_rgb, g_a])
    if e:
        e[2].record()
        ev.append(e)


for leg in specs:
    for _ in range(a.warm):
        call(leg)
    families[leg] = list(R.last_bwd_choice())
torch.cuda.synchronize()
per = max(1, a.iters // a.rounds)
ms = {leg: {"fwd": [], "bwd": []} for leg in specs}
names = list(specs)
for r in range(a.rounds):
    for leg in (names if r % 2 == 0 else names[::-1]):
        ev = []
        for _ in range(per):
            call(leg, ev)
        ev[-1][2].synchronize()
        ms[leg]["fwd"].append(sum(e[0].elapsed_time(e[1]) for e in ev) / per)
        ms[leg]["bwd"].append(sum(e[1].elapsed_time(e[2]) for e in ev) / per)

res = {"config": {"D": D, "T": T, "H": H, "W": W, "dtype": "f16" if a.f16 else "f32", "warm": a.warm, "timed_calls_per_leg": per * a.rounds,
                  "rounds": a.rounds}, "backward_family": families}
for leg in specs:
    res[leg] = {}
    for k in ("fwd", "bwd"):
        v = ms[leg][k]
        res[leg][k] = {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)}
        print(f"{leg:6s} {k}: {statistics.median(v):7.3f} ms (min {min(v):.3f}, max {max(v):.3f} over {a.rounds} rounds of {per})   backward: {families[leg][:3]}")
for k in ("fwd", "bwd"):
    res[f"ratio_{k}"] = res["baked"][k]["ms_median"] / res["post"][k]["ms_median"]
res["ratio_iteration"] = ((res["baked"]["fwd"]["ms_median"] + res["baked"]["bwd"]["ms_median"])
                          / (res["post"]["fwd"]["ms_median"] + res["post"]["bwd"]["ms_median"]))
print(f"baked / post: forward {res['ratio_fwd']:.3f}, backward {res['ratio_bwd']:.3f}, forward + backward {res['ratio_iteration']:.3f}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
