#!/usr/bin/env python3
"""The camera gradient against the stack backward at cfg3's shape (D = 32, T = 50, 720p, as bench.py builds it: the planar convention,
sigmoid / sigmoid, the benchmark camera, hash-drawn output gradients on rgb): vl3d_render_bwd_homos and vl3d_render_bwd with the same
arguments, alternated in one process, each call between two HIP events.

    python profiles/bwd_homos.py [--reps 12] [--warmup 3] [--D 32 --T 50 --H 720 --W 1280] [--out bwd_homos.json]

Prints one JSON line: per entry the median / min / max ms and GB/s on the stack's bytes (D T Hs Ws 16: what both read once), the ratio of the
medians, and the launches' count.  No GPU: it fails."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--H", type=int, default=720)
    ap.add_argument("--W", type=int, default=1280)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "profiles/bwd_homos.py measures on the MI355X: no GPU, no number"
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib as L, synth
    from videoloop3d_amd import render as R
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths

    dev = torch.device("cuda:0")
    D, T, H, W = a.D, a.T, a.H, a.W
    spec = R.RenderSpec.mpv()
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    homos = compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3),
                               make_depths(D, 1.0, 100.0).flip(0)[None])[0].to(dev).contiguous()
    stack = synth.make_plane_stack(D, T, H, W, seed=2, device=dev)
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5, device=dev) - 0.5
    with torch.no_grad():
        rgb, alpha = R.render_planes(stack, homos, H, W, spec)
    desc = R._desc(stack, H, W, spec, 0, 0)
    lib = L.lib()
    nb_s, nb_h = int(lib.vl3d_render_bwd_scratch_bytes(desc)), int(lib.vl3d_render_bwd_homos_scratch_bytes(desc))
    scratch_s = torch.empty((nb_s + 3) // 4, dtype=torch.float32, device=dev)
    scratch_h = torch.empty((nb_h + 3) // 4, dtype=torch.float32, device=dev)
    g_stack = torch.empty_like(stack)
    g_homos = torch.empty((D, 3, 3), dtype=torch.float32, device=dev)
    sp = L.stream_ptr(dev)

    def bwd_stack():
        L.check(lib.vl3d_render_bwd(desc, L.ptr(stack), L.ptr(homos), None, 0, 0, L.ptr(rgb), L.ptr(alpha), L.ptr(g_rgb), None, None, None, None,
                                    L.ptr(g_stack), L.ptr(scratch_s), nb_s, sp), "vl3d_render_bwd")

    def bwd_homos():
        L.check(lib.vl3d_render_bwd_homos(desc, L.ptr(stack), L.ptr(homos), None, 0, 0, L.ptr(rgb), L.ptr(alpha), L.ptr(g_rgb), None, L.ptr(g_homos),
                                          L.ptr(scratch_h), nb_h, sp), "vl3d_render_bwd_homos")

    times = {"vl3d_render_bwd": [], "vl3d_render_bwd_homos": []}
    for i in range(a.warmup + a.reps):
        for name, fn in (("vl3d_render_bwd", bwd_stack), ("vl3d_render_bwd_homos", bwd_homos)):      # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    first = g_homos.clone()
    bwd_homos()
    torch.cuda.synchronize()
    stack_bytes = D * T * H * W * 16
    res = {"shape": f"D={D} T={T} {H}x{W} planes {H}x{W} fp32, planar sigmoid/sigmoid", "reps": a.reps, "warmup": a.warmup,
           "stack_GB": stack_bytes / 1e9, "same_bits_on_two_calls": bool(torch.equal(first, g_homos)),
           "finite": bool(torch.isfinite(g_homos).all()), "stack_backward_choice": [getattr(R.bwd_choice(desc), k) for k in ("family", "width", "rows")]}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"median_ms": round(med, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "stack_GB_per_s": round(stack_bytes / med / 1e6, 1)}
    res["ratio_homos_over_stack_backward"] = round(res["vl3d_render_bwd_homos"]["median_ms"] / res["vl3d_render_bwd"]["median_ms"], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
