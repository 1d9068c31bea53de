#!/usr/bin/env python3
"""Video I/O on the MI355X (csrc/vl3d_video.hip, videoloop3d_amd/y4m.py): what the conversion kernels and the file path cost.
  (a) 720p x 120 frames: encode 4:2:0, decode to uint8, decode to float -- ms per frame and achieved GB/s on the bytes the rule moves
      (encode: 3 read + 1.5 written per pixel; decode: 1.5 read + 3 or 12 written), with the rule in plain torch on the device beside each,
      for scale only;
  (b) both paths (wide / byte) of the same aligned shape;
  (c) render_video.write_video: frames per second into a file on a RAM-backed directory, against render_display alone, for the dense baked
      model and the baked pool.
Legs alternate inside one process; HIP events span each leg; the first pass of every leg is a warm-up and is not counted; medians with min
and max.  Writes profiles/video_io.json (or --out).  Usage: python profiles/video_io.py [--reps 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def alternate(legs, reps):
    """legs: {name: callable} -> {name: [ms]}: reps + 1 rounds over all legs in turn, each leg between two events; round 0 dropped."""
    ms = {k: [] for k in legs}
    for r in range(reps + 1):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r:
                ms[name].append(a.elapsed_time(b))
    return ms


def kernels(dev, reps, N=120, H=720, W=1280):
    from videoloop3d_amd import synth, y4m
    frames = (synth.hash_uniform((N, H, W, 3), seed=1, device=dev) * 256).clamp(0, 255).to(torch.uint8)
    fb = y4m.frame_bytes(H, W, "420")
    buf = torch.empty(N * fb, dtype=torch.uint8, device=dev)
    out8 = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    outf = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
    y4m.encode_frames(frames, buf, matrix="bt709")
    planes = y4m.planes_of(buf, N, H, W, "420")
    px = N * H * W
    legs = {
        "encode_420_wide": lambda: y4m.encode_frames(frames, buf, matrix="bt709"),
        "encode_420_byte": lambda: y4m.encode_frames(frames, buf, matrix="bt709", path=y4m.PATH_BYTE),
        "encode_420_torch_rule": lambda: y4m.rgb8_to_yuv8(frames, "420", "bt709"),
        "decode_u8_wide": lambda: y4m.decode_frames(buf, N, H, W, matrix="bt709", out=out8),
        "decode_u8_byte": lambda: y4m.decode_frames(buf, N, H, W, matrix="bt709", out=out8, path=y4m.PATH_BYTE),
        "decode_u8_torch_rule": lambda: y4m.yuv8_to_rgb8(*planes, "420", "center", "bt709"),
        "decode_f32_wide": lambda: y4m.decode_frames(buf, N, H, W, matrix="bt709", layout="float", out=outf),
        "decode_f32_byte": lambda: y4m.decode_frames(buf, N, H, W, matrix="bt709", layout="float", out=outf, path=y4m.PATH_BYTE),
        "decode_f32_torch_rule": lambda: y4m.yuv8_to_rgb8(*planes, "420", "center", "bt709", layout="float"),
    }
    bytes_px = {"encode": 4.5, "decode_u8": 4.5, "decode_f32": 13.5}
    res = {}
    for name, ms in alternate(legs, reps).items():
        bpp = bytes_px["encode" if name.startswith("encode") else "decode_f32" if "f32" in name else "decode_u8"]
        res[name] = {"ms_per_frame": stats([m / N for m in ms]), "GB_per_s_on_rule_bytes": stats([px * bpp / (m * 1e-3) / 1e9 for m in ms]),
                     "rule_bytes_per_pixel": bpp}
    same = bool(torch.equal(y4m.encode_frames(frames, matrix="bt709"), y4m.encode_frames(frames, matrix="bt709", path=y4m.PATH_BYTE)))
    return {"shape": f"{N} x {H} x {W}, 4:2:0, BT.709 limited", "legs": res, "wide_equals_byte": same}


def playback_model(dev, H=720, W=1280, D=32, T=50, hv=36, wv=64):
    """examples/playback.py --full: a sparsified 720p model, 40 % of the quads kept, 30 % of those dynamic"""
    from videoloop3d_amd import synth, tiles
    from videoloop3d_amd.MPV import MPMeshVid
    args = types.SimpleNamespace(mpv_frm_num=T, mpv_isloop=True, mpi_h_scale=1.1, mpi_w_scale=1.1, mpi_d=D, mpi_h_verts=hv, mpi_w_verts=wv, atlas_grid_h=4,
                                 init_std=0.02, rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color="", scale_invariant=True,
                                 fp16=False, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1, sparsity_loss_weight=0.0,
                                 rgb_smooth_loss_weight=0.0, a_smooth_loss_weight=0.0, density_loss_weight=0.0, d_smooth_loss_weight=0.0,
                                 optimizer="adam", lrate=0.1, lrate_decay=30)
    K = np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]])
    model = MPMeshVid(args, H, W, np.eye(4), K, 1.0, 100.0, device=dev).to(dev).eval()
    keep = synth.hash_uniform((D, hv - 1, wv - 1), seed=31) < 0.4
    dyn = keep & (synth.hash_uniform((D, hv - 1, wv - 1), seed=32) < 0.3)
    with torch.no_grad():
        model.stack.copy_(synth.make_plane_stack(*model.stack.shape[:4], seed=5, device=dev, alpha_bias=0.0))
        tiles.cull_stack_(model.stack.data, keep.to(dev))
        dyn_t = tiles.quad_to_texel_mask(dyn.to(dev), *model.stack.shape[2:4])
        model.stack.copy_(torch.where(dyn_t[:, None, :, :, None], model.stack.data, model.stack.data[:, :1]))
    model._set_quad_maps(keep, dyn, dev)
    model.is_sparse = model.has_dyn = True
    return model, K


def files(dev, reps, N=120, H=720, W=1280):
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd.baked import bake, bake_pool
    model, K = playback_model(dev, H, W)
    T = model.frm_num
    ext = np.stack([np.eye(4, dtype=np.float32)] * N)
    for i in range(N):
        a = 2 * np.pi * i / N
        ext[i, :3, 3] = [0.05 * np.cos(a), 0.03 * np.sin(a), 0.01 * np.sin(2 * a)]
    intr, rt = np.stack([K.astype(np.float32)] * N), np.arange(N) % T
    ram = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    res = {"directory": "RAM-backed (/dev/shm)" if ram else "the default temporary directory (no writable /dev/shm: NOT RAM-backed)"}
    with tempfile.TemporaryDirectory(dir=ram) as d:
        path = os.path.join(d, "spiral.y4m")
        for name, b in (("dense", bake(model)), ("pool", bake_pool(model))):
            def shown():
                b.render_display(H, W, ext, intr, rt)
                torch.cuda.synchronize()

            def written():
                RV.write_video(path, model, H, W, ext, intr, rt, baked=b)      # returns with the file closed
            fps = {"render_display": [], "write_video": []}
            for r in range(reps + 1):
                for leg, fn in (("render_display", shown), ("write_video", written)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    dt = time.perf_counter() - t0
                    if r:
                        fps[leg].append(N / dt)
            res[name] = {leg: {"frames_per_s": stats(v)} for leg, v in fps.items()}
            res[name]["file_MB"] = os.path.getsize(path) / 1e6
    res["shape"] = f"{N} poses of a spiral, {H} x {W}, D = 32, T = {T}, segments of 64 frames"
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "video_io.json"))
    ap.add_argument("--skip-files", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    if not torch.cuda.is_available():
        sys.exit("profiles/video_io.py measures on the MI355X: no device here, nothing measured")
    dev = torch.device("cuda:0")
    out = {"kernels": kernels(dev, a.reps)}
    if not a.skip_files:
        out["files"] = files(dev, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
