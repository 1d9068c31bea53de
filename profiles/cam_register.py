#!/usr/bin/env python3
"""Camera registration against the camera normal equations at cfg3's shape (D = 32, T = 50, 720p, as profiles/cam_normal.py builds it: the
planar convention, sigmoid / sigmoid, the benchmark camera, P = 6 tangents of a left twist): the four mode / brightness combinations of
vl3d_render_cam_register and vl3d_render_cam_normal with the same stack, homographies and forward picture, alternated in one process, each call
(render kernel + finish kernel) between two HIP events.

    python profiles/cam_register.py [--reps 12] [--warmup 3] [--P 6] [--D 32 --T 50 --H 720 --W 1280] [--out cam_register.json]

The expectation it confirms or refutes: the per-frame mode does render_cam_normal_k's work plus, with the brightness unknowns, 17 (P = 6) more
row sums per frame and pixel; the long exposure deposits once per pixel instead of once per frame, so it should not be slower than
vl3d_render_cam_normal.  Prints one JSON line: per entry the median / min / max ms and GB/s on the stack's bytes (D T Hs Ws 16), and the ratio
of each median to vl3d_render_cam_normal's.  No GPU: it fails."""
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
    ap.add_argument("--P", type=int, default=6)
    ap.add_argument("--D", type=int, default=32)
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--H", type=int, default=720)
    ap.add_argument("--W", type=int, default=1280)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "profiles/cam_register.py measures on the MI355X: no GPU, no number"
    assert 1 <= a.P <= 7, "P: 1 .. 6 components of a twist, 7 with the log focal scale"
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import _lib as L, poses, synth
    from videoloop3d_amd import render as R
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths

    dev = torch.device("cuda:0")
    D, T, H, W, P = a.D, a.T, a.H, a.W, a.P
    spec = R.RenderSpec.mpv()
    ref_e, Kr, tar_e, Kt = (t.double() for t in synth.make_cameras(H, W))
    normal, depths = torch.tensor([0., 0., 1.], dtype=torch.float64).expand(1, D, 3), make_depths(D, 1.0, 100.0).flip(0)[None].double()

    def chain(theta):      # the first min(P, 6) components of a left twist of the target camera; the seventh parameter is its log focal scale
        xi = torch.cat([theta[:min(P, 6)], theta.new_zeros(6 - min(P, 6))])
        K = poses._focal_scaled(Kt, theta[6]) if P == 7 else Kt
        return compute_homography(ref_e[None], Kr[None], (poses.se3_exp(xi) @ tar_e)[None], K[None], normal, depths)[0]

    theta0 = torch.zeros(P, dtype=torch.float64)
    dhomos = torch.autograd.functional.jacobian(chain, theta0, vectorize=True, strategy="forward-mode").permute(3, 0, 1, 2).float().contiguous().to(dev)
    homos = chain(theta0).float().contiguous().to(dev)
    stack = synth.make_plane_stack(D, T, H, W, seed=2, device=dev)
    noise = synth.hash_uniform((T, H, W, 3), seed=5, device=dev) - 0.5
    with torch.no_grad():
        rgb, _ = R.render_planes(stack, homos, H, W, spec)
    target = (1.25 * rgb + 0.05 + 0.1 * noise).contiguous()      # a clip exposed differently, per frame
    target_mean = target.mean(0).contiguous()                   # and its long exposure
    del noise
    desc = R._desc(stack, H, W, spec, 0, 0)
    lib = L.lib()
    sp = L.stream_ptr(dev)
    Qmax = P + 2
    out = torch.empty(Qmax * Qmax + Qmax + 1, dtype=torch.float64, device=dev)
    nb_n = int(lib.vl3d_render_cam_normal_scratch_bytes(desc, P))
    nb_r = int(lib.vl3d_render_cam_register_scratch_bytes(desc, P, 1))
    scratch = torch.empty((max(nb_n, nb_r) + 7) // 8, dtype=torch.float64, device=dev)

    def normal_eq():
        L.check(lib.vl3d_render_cam_normal(desc, L.ptr(stack), L.ptr(homos), L.ptr(dhomos), P, None, 0, 0, L.ptr(rgb), L.ptr(target), None, L.ptr(out),
                                           L.ptr(scratch), nb_n, sp), "vl3d_render_cam_normal")

    def register(mode, photo):
        def run():
            L.check(lib.vl3d_render_cam_register(desc, L.ptr(stack), L.ptr(homos), L.ptr(dhomos), P, None, 0, 0, L.ptr(rgb),
                                                 L.ptr(target_mean if mode else target), None, mode, photo, 0.2, 0.04, L.ptr(out), L.ptr(scratch), nb_r, sp),
                    "vl3d_render_cam_register")
        return run

    entries = [("vl3d_render_cam_normal", normal_eq)]
    for mode, mname in ((0, "per_frame"), (1, "long_exposure")):
        for photo, pname in ((0, "camera"), (1, "camera+brightness")):
            entries.append((f"vl3d_render_cam_register[{mname},{pname}]", register(mode, photo)))
    times = {name: [] for name, _ in entries}
    for i in range(a.warmup + a.reps):
        for name, fn in entries:      # alternated
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    first = out.clone()
    entries[-1][1]()
    torch.cuda.synchronize()
    stack_bytes = D * T * H * W * 16
    res = {"shape": f"D={D} T={T} {H}x{W} planes {H}x{W} fp32, planar sigmoid/sigmoid, P={P}", "reps": a.reps, "warmup": a.warmup,
           "stack_GB": stack_bytes / 1e9, "same_bits_on_two_calls": bool(torch.equal(first, out)), "finite": bool(torch.isfinite(out).all())}
    base = statistics.median(times["vl3d_render_cam_normal"])
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"median_ms": round(med, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "stack_GB_per_s": round(stack_bytes / med / 1e6, 1),
                     "ratio_to_cam_normal": round(med / base, 3)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
