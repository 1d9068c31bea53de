#!/usr/bin/env python3
"""In-process A/B of the float forward against the baked forward at cfg3 (D = 32, T = 50, 720p; docs/kernels/K9_baked_playback.md).
Both stacks are resident (fp32 23.6 GB + RGBA8 5.9 GB), both renders take the same homographies, the legs alternate round by round under
HIP events on the launch stream; the float leg is the yardstick (the same kernel the parent commit ships, timed in this process).
  python profiles/baked_fwd.py [--warm 20] [--iters 100] [--rounds 10] [--D 32 --T 50 --H 720 --W 1280] [--out FILE]
Prints per leg: ms per call (median / min over the rounds), Mpix/s, and the fraction of 8 TB/s its ALGORITHMIC bytes amount to -- per pixel
and frame one texel per plane and 16 bytes of output: 16 D + 16 (float), 4 D + 16 (baked)."""
import argparse
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
ap.add_argument("--out", default="")
a = ap.parse_args()
assert a.warm >= 1 and a.iters >= a.rounds >= 1

import __graft_entry__ as ge  # noqa: E402
ge.build()
from videoloop3d_amd import synth  # noqa: E402
from videoloop3d_amd.baked import bake_texels  # noqa: E402
from videoloop3d_amd.render import RenderSpec, render_frame_run, render_frame_run_baked  # noqa: E402
from videoloop3d_amd.utils_mpi import compute_homography, make_depths  # noqa: E402

assert torch.cuda.is_available(), "profiles/baked_fwd.py measures on the MI355X"
dev = torch.device("cuda:0")
D, T, H, W = a.D, a.T, a.H, a.W
ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
homos = compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3),
                           make_depths(D, 1.0, 100.0).flip(0)[None])[0].to(dev)
stack = synth.make_plane_stack(D, T, H, W, seed=2, device=dev)
baked = bake_texels(stack, "sigmoid", "sigmoid")
spec = RenderSpec.mpv()
out = (torch.empty((T, H, W, 3), device=dev), torch.empty((T, H, W), device=dev))
legs = {"float": lambda: render_frame_run(stack, 0, T, homos, H, W, spec, out=out),
        "baked": lambda: render_frame_run_baked(baked, 0, T, homos, H, W, spec, out=out)}
bytes_px = {"float": 16 * D + 16, "baked": 4 * D + 16}

for f in legs.values():
    for _ in range(a.warm):
        f()
torch.cuda.synchronize()
per = max(1, a.iters // a.rounds)
ms = {k: [] for k in legs}
for r in range(a.rounds):
    for k in (("float", "baked") if r % 2 == 0 else ("baked", "float")):      # alternate the order as well
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            legs[k]()
        e1.record()
        e1.synchronize()
        ms[k].append(e0.elapsed_time(e1) / per)
res = {"config": {"D": D, "T": T, "H": H, "W": W, "warm": a.warm, "timed_calls_per_leg": per * a.rounds, "rounds": a.rounds},
       "stack_GB": {"float": stack.numel() * 4 / 1e9, "baked": baked.numel() / 1e9}}
for k in legs:
    med, lo = statistics.median(ms[k]), min(ms[k])
    res[k] = {"ms_median": med, "ms_min": lo, "ms_max": max(ms[k]), "Mpix_s": T * H * W / med / 1e3, "algorithmic_bytes_per_pixel": bytes_px[k],
              "fraction_of_8TBs": T * H * W * bytes_px[k] / (med * 1e-3) / 8e12}
    print(f"{k:5s} forward: {med:7.3f} ms (min {lo:.3f}, max {max(ms[k]):.3f} over {a.rounds} rounds of {per})  {res[k]['Mpix_s']:8.0f} Mpix/s  "
          f"{bytes_px[k]} B/pixel -> {res[k]['fraction_of_8TBs']:.3f} of 8 TB/s")
res["speedup"] = res["float"]["ms_median"] / res["baked"]["ms_median"]
res["byte_ratio"] = bytes_px["float"] / bytes_px["baked"]
print(f"baked is {res['speedup']:.2f}x the float forward (algorithmic byte ratio {res['byte_ratio']:.2f}x)")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
