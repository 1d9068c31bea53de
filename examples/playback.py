#!/usr/bin/env python3
"""The playback model end to end: bake a small MPMeshVid (the `--small` shape of examples/pipeline.py: 180 x 320, D = 16, T = 12, 17 x 31 quads,
synthetic weights and a synthetic quad map), render the same spiral from the float model, from the baked one and from the baked POOL
(`baked.bake_pool`: static blocks once, dynamic blocks per frame, culled blocks not at all -- no dense clip) -- frames / s of
`render_video.render_frames` for each (the two baked models along the spiral through the path render: one plan launch and one render launch
per chunk of 64 poses, `calls` in the output, the launch storing the uint8 frames itself -- `route`: no float frames, no torch epilogue),
bytes of the three textures, PSNR between the float and the baked frames, and whether the pool's
frames equal the dense baked frames --, then write the viewer package (geometry.obj, static.png,
dynamic/%04d.png, meta.json), OPEN it again from the files alone (`baked.open_viewer_package`: no model, no arguments) and play the spiral
from it: load time (PNG decode apart), frames / s, and the byte difference of its frames against the in-process pool's (this model's tiles
share their borders, so the export resamples them: close, not equal).  `--full`: 720p, D = 32, T = 50.
`--fps-out R` (default off): also play the spiral RETIMED from the loop's 25 fps to a display of R frames per second, from the clip and from
the pool -- loop times `render_video.retime(N, R)`, texels interpolated between adjacent frames and across the loop seam
(`render_frames(..., fractional=True)`): frames / s of both, and whether the two frame sets are equal.
`--trim`: every fourth kept quad is made invisible first (alpha logit -12 on the texels it can read) and every second dynamic quad frozen (frame 0
in every frame) -- synthetic weights have nothing a player cannot show --, then `pool.trimmed()`: its report, whether the trimmed pool's spiral
equals the pool's, and the viewer package written with and without `quad_maps=` (this model's tiles share their borders, so the package may
only drop quads): MB, face count, and whether the two opened packages play equal frames."""
import argparse
import json
import os
import sys
import tempfile
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def run(full=False, outdir=None, dev="cuda:0", fps_out=None, trim=False, y4m=None):
    from videoloop3d_amd import render_video as RV
    from videoloop3d_amd import synth, tiles
    from videoloop3d_amd.baked import bake, bake_pool, culled_texel_rgba8, open_viewer_package
    from videoloop3d_amd.export import read_png, save_viewer_package
    from videoloop3d_amd.MPV import MPMeshVid
    dev = torch.device(dev)
    H, W, D, T, hv, wv, N = (720, 1280, 32, 50, 36, 64, 150) if full else (180, 320, 16, 12, 18, 32, 60)
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
        # a static quad is ONE texture shared by all frames (what training keeps true): frame 0 over every texel no dynamic quad reads
        dyn_t = tiles.quad_to_texel_mask(dyn.to(dev), *model.stack.shape[2:4])
        model.stack.copy_(torch.where(dyn_t[:, None, :, :, None], model.stack.data, model.stack.data[:, :1]))
        if trim:
            pick = lambda m, n: (torch.zeros(m.numel(), dtype=torch.bool).index_fill_(0, m.flatten().nonzero()[:, 0][::n], True)).reshape(m.shape)      # noqa: E731
            invisible, frozen = pick(keep, 4), pick(dyn, 2)
            fr = tiles.quad_to_texel_mask(frozen.to(dev), *model.stack.shape[2:4])
            model.stack.copy_(torch.where(fr[:, None, :, :, None], model.stack.data[:, :1], model.stack.data))
            model.stack.data[..., 3].masked_fill_(tiles.quad_to_texel_mask(invisible.to(dev), *model.stack.shape[2:4])[:, None], -12.0)
    model._set_quad_maps(keep, dyn, dev)
    model.is_sparse = model.has_dyn = True
    sync = torch.cuda.synchronize
    out = {}
    sync(); t0 = time.perf_counter()
    baked = bake(model)
    sync(); t1 = time.perf_counter()
    out["bake"] = {"seconds": t1 - t0, "float_MB": model.stack.numel() * 4 / 1e6, "baked_MB": baked.nbytes / 1e6}
    sync(); t0 = time.perf_counter()
    pool = bake_pool(model)
    sync(); t1 = time.perf_counter()
    out["bake_pool"] = {"seconds": t1 - t0, "pool_MB": pool.nbytes / 1e6, "slots": pool.layout.n_slots, "blocks_static": pool.layout.n_static,
                        "blocks_dynamic": pool.layout.n_dynamic, "dense_baked_over_pool": baked.nbytes / pool.nbytes}
    ext = np.stack([np.eye(4, dtype=np.float32)] * N)      # a spiral of cameras around the reference view
    for i in range(N):
        a = 2 * np.pi * i / N
        ext[i, :3, 3] = [0.05 * np.cos(a), 0.03 * np.sin(a), 0.01 * np.sin(2 * a)]
    intr, rt = np.stack([K.astype(np.float32)] * N), np.arange(N) % T
    frames = {}
    for name, kw in (("float", {}), ("baked", {"baked": baked}), ("baked_pool", {"baked": pool})):
        RV.render_frames(model, H, W, ext[:4], intr[:4], rt[:4], **kw)      # untimed: code objects, allocator
        sync(); t0 = time.perf_counter()
        frames[name] = RV.render_frames(model, H, W, ext, intr, rt, **kw)
        sync(); dt = time.perf_counter() - t0
        out[name] = {"frames": N, "frames_per_s": N / dt, "ms_per_frame": dt / N * 1e3}
        if kw:      # how render_frames launched the spiral: every pose its own camera -> one path call per chunk
            kinds = [k for k, _, _ in RV.path_segments(list(range(N)), rt, 64)]
            out[name]["calls"] = {k: kinds.count(k) for k in sorted(set(kinds))}
            out[name]["route"] = "render_display: uint8 frames stored by the render launches (frames8=)"
    if y4m:      # the baked spiral as a file any player opens (render_video.write_video: chunks of 64 frames through a y4m.Y4MWriter)
        sync(); t0 = time.perf_counter()
        n = RV.write_video(y4m, model, H, W, ext, intr, rt, fps=25, baked=baked)
        dt = time.perf_counter() - t0
        out["y4m"] = {"path": y4m, "frames": n, "bytes": os.path.getsize(y4m), "frames_per_s": n / dt}
    # the depth map beside the picture (render_video.render_disparity_frames): the float clip frame by frame, the baked models as path calls
    maps = {}
    for name, kw in (("float", {}), ("baked", {"baked": baked}), ("baked_pool", {"baked": pool})):
        RV.render_disparity_frames(model, H, W, ext[:4], intr[:4], rt[:4], **kw)      # untimed
        sync(); t0 = time.perf_counter()
        maps[name] = RV.render_disparity_frames(model, H, W, ext, intr, rt, **kw)
        sync(); dt = time.perf_counter() - t0
        out[name]["disparity"] = {"frames_per_s": N / dt, "ms_per_frame": dt / N * 1e3, "min": float(maps[name].min()), "max": float(maps[name].max())}
    out["pool_disparity_equals_baked_disparity"] = bool(torch.equal(maps["baked_pool"], maps["baked"]))
    out["max_abs_disparity_baked_vs_float"] = float((maps["baked"] - maps["float"]).abs().max())
    del maps
    # colour and 16-bit depth of every frame from one render launch per chunk (render_video.render_rgbd_frames)
    for name, model_b in (("baked", baked), ("baked_pool", pool)):
        RV.render_rgbd_frames(model_b, H, W, ext[:4], intr[:4], rt[:4])      # untimed
        sync(); t0 = time.perf_counter()
        RV.render_rgbd_frames(model_b, H, W, ext, intr, rt)
        sync(); dt = time.perf_counter() - t0
        out[name]["rgbd"] = {"frames_per_s": N / dt, "ms_per_frame": dt / N * 1e3}
    mse = float(((frames["float"].float() - frames["baked"].float()) / 255).pow(2).mean())
    out["psnr_baked_vs_float_dB"] = float("inf") if mse == 0 else -10 * np.log10(mse)
    out["pool_frames_equal_baked_frames"] = bool(torch.equal(frames["baked_pool"], frames["baked"]))
    if trim:
        sync(); t0 = time.perf_counter()
        lean = pool.trimmed()
        sync(); t1 = time.perf_counter()
        RV.render_frames(model, H, W, ext[:4], intr[:4], rt[:4], baked=lean)      # untimed
        sync(); t0f = time.perf_counter()
        lean_frames = RV.render_frames(model, H, W, ext, intr, rt, baked=lean)
        sync(); dt = time.perf_counter() - t0f
        out["trim"] = {"seconds": t1 - t0, "report": lean.trim_report, "pool_MB": lean.nbytes / 1e6, "frames_per_s": N / dt,
                       "frames_equal_the_pools": bool(torch.equal(lean_frames, frames["baked_pool"])),
                       "made_invisible_quads": int(invisible.sum()), "frozen_dynamic_quads": int(frozen.sum())}
    if fps_out:      # the same spiral shown at another rate: pose i at loop time i * 25 / fps_out
        ts = RV.retime(N, fps_out, 25.0)
        retimed = {}
        for name, b in (("baked", baked), ("baked_pool", pool)):
            RV.render_frames(model, H, W, ext[:4], intr[:4], ts[:4], baked=b, fractional=True)      # untimed
            sync(); t0 = time.perf_counter()
            retimed[name] = RV.render_frames(model, H, W, ext, intr, ts, baked=b, fractional=True)
            sync(); dt = time.perf_counter() - t0
            out["retimed_" + name] = {"frames": N, "fps_out": fps_out, "fps_loop": 25.0, "loops_played": float(ts[-1]) / T, "frames_per_s": N / dt,
                                      "ms_per_frame": dt / N * 1e3, "route": "render_display(fractional=True): one loop-time path call per chunk"}
        out["retimed_pool_frames_equal_baked_frames"] = bool(torch.equal(retimed["baked_pool"], retimed["baked"]))
        out["retimed_frames_at_integer_times_equal_the_spiral"] = bool(all(
            torch.equal(retimed["baked"][i], RV.render_frames(model, H, W, ext[i:i + 1], intr[i:i + 1], np.array([int(ts[i]) % T]), baked=baked)[0])
            for i in range(N) if float(ts[i]) == int(ts[i])))
    poses = np.linalg.inv(ext[:8])[:, :3, :4]              # eight of the cameras as the capture's views (camera-to-world)
    with tempfile.TemporaryDirectory() as tmp:
        where = outdir or tmp
        sync(); t0 = time.perf_counter()
        files = save_viewer_package(model, where, poses, intr[:8], np.array([1.0, 100.0]))
        out["package"] = {"seconds": time.perf_counter() - t0, "files": len(files), "MB": sum(os.path.getsize(f) for f in files) / 1e6,
                          "dir": outdir or "(temporary)"}
        # the package alone: open it, play the spiral from it
        sync(); t0 = time.perf_counter()
        opened = open_viewer_package(where, dev, bg_color="", culled_rgba8=culled_texel_rgba8("sigmoid", "sigmoid"))
        sync(); load_s = time.perf_counter() - t0
        t0 = time.perf_counter()      # the decoding alone, on one thread: every PNG of the package once more
        for f in files:
            if f.endswith(".png"):
                read_png(f)
        decode_s = time.perf_counter() - t0
        opened.render_display(H, W, ext[:4], intr[:4], rt[:4])      # untimed: allocator
        sync(); t0 = time.perf_counter()
        shown = opened.render_display(H, W, ext, intr, rt)
        sync(); dt = time.perf_counter() - t0
        diff = (shown.int() - frames["baked_pool"].to(shown.device).int()).abs()
        out["opened"] = {"load_seconds": load_s, "png_decode_one_thread_seconds": decode_s, "pool_MB": opened.nbytes / 1e6,
                         "tile": list(opened.layout.tile), "planes": opened.layout.D, "frames": N, "frames_per_s": N / dt, "ms_per_frame": dt / N * 1e3,
                         "bytes_differing_from_in_process_pool": int((diff > 0).sum()), "bytes": diff.numel(), "max_level_difference": int(diff.max()),
                         "mean_level_difference": float(diff.float().mean())}
        if trim:      # the package with the trimmed maps: a lattice model drops quads, its dynamic quads stay dynamic
            def facts(d, fs):
                return {"MB": sum(os.path.getsize(f) for f in fs) / 1e6, "faces": sum(1 for line in open(os.path.join(d, "geometry.obj")) if line.startswith("f "))}
            with tempfile.TemporaryDirectory() as tmp2:
                lk = lean.quad_keep.bool().cpu()
                lean_files = save_viewer_package(model, tmp2, poses, intr[:8], np.array([1.0, 100.0]), quad_maps=(lk, lk & dyn))
                lean_opened = open_viewer_package(tmp2, dev, bg_color="", culled_rgba8=culled_texel_rgba8("sigmoid", "sigmoid"))
                same_grid = lean_opened.layout.D == opened.layout.D and tuple(lean_opened.quad_keep.shape) == tuple(opened.quad_keep.shape)
                out["trim"]["package"] = {"without": facts(where, files), "with_quad_maps": facts(tmp2, lean_files),
                                          "opened_frames_equal": bool(same_grid and torch.equal(lean_opened.render_display(H, W, ext, intr, rt), shown))}
    out["shape"] = f"{H}x{W}, D={D}, T={T}, planes {tuple(model.stack.shape[2:4])}, {float(keep.float().mean()):.0%} of the quads kept, {N} spiral frames"
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--out", default=None, help="directory for the viewer package (default: a temporary one)")
    ap.add_argument("--fps-out", type=float, default=None, help="also play the spiral retimed from 25 fps to this display rate (default: off)")
    ap.add_argument("--y4m", default=None, metavar="PATH", help="also write the baked spiral to PATH as a YUV4MPEG2 (.y4m) file")
    ap.add_argument("--trim", action="store_true", help="also trim the pool (BakedPool.trimmed) and write the package with its quad maps")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.full, a.out, fps_out=a.fps_out, trim=a.trim, y4m=a.y4m)))
