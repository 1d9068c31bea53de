#!/usr/bin/env python3
"""Stage-2 training on the REFERENCE'S SCHEDULE (train_3dvid.py:22-66, 103-119, 262-290; configs/mpv_base.txt): V views with distinct
poses, the crops of `generate_patchinfo` (180 x 320, stride 90 x 160) at the last three pyramid levels of a 360 x 640 frame -- 4, 4 and
9 crops per view --, shuffled per epoch, adaptive learning rate, the crop-aware optimiser re-created at every level after `lod`.
`examples/stage2_step.py` cycles six overlapping crops under ONE pose, where a tile's deferred-update depth never exceeds a few steps;
here a crop's texel window comes back once per epoch, i.e. after len(dataset) = 32 ... 72 iterations, which is what the deferral of
`optim.WindowAdam` (replayed zero-gradient updates, O(depth) per texel, twice per iteration) has to live with in real training.

Reports iterations per second per level and overall (dataset construction and `lod` outside the timed loops: the reference does
them once per 50 epochs), and from a second, instrumented pass the histogram of catch-up depths (steps a window tile had missed when
its crop came back).  `profiles/kstats.sh` over this script gives the catch-up / step kernel times."""
import argparse
import json
import os
import sys
import time
import types
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def make_views(V, H, W, frames, dev):
    """V cameras on a small arc around the reference view (hand-held capture: translations of a few percent of the nearest plane's depth,
    rotations of about a degree), 3 x 4 camera-to-world poses like the dataloader's, and V synthetic clips [F,3,H,W]."""
    from videoloop3d_amd import synth
    poses, vids = [], []
    for v in range(V):
        a, b = np.radians(1.2 * np.cos(2 * np.pi * v / V)), np.radians(0.8 * np.sin(2 * np.pi * v / V))
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        t = np.array([0.06 * np.cos(2 * np.pi * v / V), 0.04 * np.sin(2 * np.pi * v / V), 0.01 * (v % 3 - 1)])
        if v == 0:
            Ry, Rx, t = np.eye(3), np.eye(3), np.zeros(3)           # view 0 is the reference view (loss_ref_idx = 0)
        poses.append(np.concatenate([Ry @ Rx, t[:, None]], 1))
        vids.append(synth.hash_uniform((frames, 3, H, W), seed=20 + v, device=dev))
    K = np.array([[0.9 * W, 0, W / 2], [0, 0.9 * W, H / 2], [0, 0, 1]], np.float64)
    return torch.tensor(np.stack(poses), dtype=torch.float32), torch.tensor(K, dtype=torch.float32)[None].repeat(V, 1, 1), vids


def run(views=8, epochs=2, planes=32, frames=50, clip=75, smooth=0.2, levels=3, dev="cuda:0", sparsify=False, fused=True, bwd_variant=0, generic_objective=False,
        tile_exact=False, gt_y4m=None):
    """tile_exact (with sparsify): the model in the TILE-EXACT layout a sparsified reference checkpoint is loaded into (every quad owns its tile,
    border texels included: 12 x 12 texels per quad of the 396 x 704 planes, MPI.py:296-313) instead of the shared-border pitch-1 stack."""
    from videoloop3d_amd.MPV import MPMeshVid
    from videoloop3d_amd.train_3dvid import MVVidPatchDataset, run_iter
    dev = torch.device(dev)
    # (a run inside a longer process -- the bench's last leg -- starts from a clean allocator: with segments of earlier legs cached, the 7 GB stack and its
    # moments occasionally landed so that the full-resolution level ran at 60-70 % of its usual rate: 426 / 337 it/s where every other run reads 570-600)
    import gc
    gc.collect()
    torch.cuda.empty_cache()
    H, W = 360, 640
    args = types.SimpleNamespace(
        mpv_frm_num=frames, mpv_isloop=True, mpi_h_scale=1.1, mpi_w_scale=1.1, mpi_d=planes, atlas_grid_h=4, init_std=0.02,
        rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color="", scale_invariant=True,
        add_uv_noise=False, fp16=False, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1,
        sparsity_loss_weight=0.0, rgb_smooth_loss_weight=smooth, a_smooth_loss_weight=smooth, density_loss_weight=0.0,
        d_smooth_loss_weight=0.0, swd_loss_weight=1.0, optimizer="adam", lrate=0.5, lrate_decay=100, lrate_adaptive=True,
        add_intrin_noise=True, mpi_h_verts=36, mpi_w_verts=64,
        generic_objective=bool(generic_objective),      # True: forward + weighted_total instead of MPMeshVid.objective (A/B)
        fused_adam_backward=bool(fused))      # dense models: the optimiser step inside the render backward (vl3d_render_bwd_adam)
    if gt_y4m:      # the views' clips from YUV4MPEG2 files, one per view, frames of 360 x 640 (y4m.videos_from_y4m); the poses stay synthetic
        from videoloop3d_amd import y4m
        files = [p for p in gt_y4m.split(",") if p]
        views = len(files)
    poses, intrins, vids = make_views(views, H, W, clip, dev)
    if gt_y4m:
        vids = y4m.videos_from_y4m(files, dev, layout="float")
        if any(tuple(v.shape[-2:]) != (H, W) for v in vids):
            raise ValueError(f"--gt-y4m: frames of {H} x {W} expected, got {[tuple(v.shape[-2:]) for v in vids]}")
    K = intrins[0].numpy()
    model = MPMeshVid(args, H, W, np.eye(4), K, 1.0, 100.0, device=dev).to(dev).train()
    if bwd_variant:      # A/B of the backward kernels (include/vl3d.h: desc->variant bits 0-3)
        import dataclasses
        model.spec = dataclasses.replace(model.spec, variant=int(bwd_variant))
    other = dict(loss_name="gpnn_lm", patch_size=3, patcht_size=3, stride=2, stridet=1, alpha=10000.0, rou="-2", scaling=0.1, dist_fn="mse",
                 macro_block=65)
    ref = dict(loss_name="gpnn_lm", loss_gain=3.5, patch_size=11, patcht_size=3, stride=4, stridet=1, alpha=0.0, rou="-2", scaling=0.1,
               dist_fn="mse", macro_block=65)
    cfgs = [ref] + [other] * (views - 1)
    if sparsify:      # what stage 2 starts from after sparsify_faces: ~16 % of the quads, half of them dynamic
        from videoloop3d_amd import tiles
        QH, QW = 35, 63
        qy, qx = torch.meshgrid(torch.arange(QH, device=dev), torch.arange(QW, device=dev), indexing="ij")
        keep = torch.zeros((planes, QH, QW), dtype=torch.bool, device=dev)
        for d in range(planes):
            cy, cx = (7 * d + 3) % QH, (11 * d + 5) % QW
            keep[d] = ((qy - cy).abs() <= QH // 5) & ((qx - cx).abs() <= QW // 4)
        model.register_buffer("quad_keep", keep)
        model.register_buffer("quad_dyn", keep & ((qy + qx) % 2 == 0)[None])
        model.is_sparse = model.has_dyn = True
        if tile_exact:
            # round(quad extent) + 1 texels per axis, as `sparsify_faces` sizes its tiles (MPI.py:296-313: 703 / 63 = 11.2 -> 12)
            th, tw = int(round((model.mpi_h - 1) / QH)) + 1, int(round((model.mpi_w - 1) / QW)) + 1
            model.tile_full = model.tile_own = (th, tw)
            with torch.no_grad():
                st = torch.randn((planes, frames, QH * th, QW * tw, 4), device=dev) * args.init_std
                st[..., -1] = -2
            model.register_parameter("stack", torch.nn.Parameter(st, requires_grad=True))
            model._set_texture_geometry(QH * th, QW * tw)
        with torch.no_grad():
            tiles.cull_stack_(model.stack.data, keep, model.tile_own)
        model._install_tie_hook()
    factors = [0.75 ** i for i in range(levels)][::-1]
    gen = torch.Generator().manual_seed(2)
    out = {"levels": []}
    total_it, total_s = 0, 0.0
    total_win = [0, 0]
    depth_hist = np.zeros(0, np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for li, f in enumerate(factors):
            hw = (int(H * f), int(W * f))
            model.lod(f)
            opt = model.get_optimizer(step=0)
            ds = MVVidPatchDataset(hw, vids, (180, 320), (90, 160), poses, intrins, loss_configs=cfgs)
            order = [i for _ in range(epochs + 1) for i in torch.randperm(len(ds), generator=gen).tolist()]
            from videoloop3d_amd.train_3dvid import pose2extrin_torch
            model.reserve_windows((it[4].shape[-2], it[4].shape[-1], pose2extrin_torch(it[2][None].cpu()), it[3][None].cpu())      # as train_3dvid.train() does
                                  for it in (ds[i] for i in range(len(ds))))

            win_texels = [0, 0]      # sum over the timed iterations of the crop window's texels per plane and frame | iterations counted

            def one(i, epoch):
                for (_, lr), g in zip(model.get_lrate(epoch), opt.param_groups):
                    g["lr"] = lr / len(ds)                                     # lrate_adaptive (train_3dvid.py:281-287)
                run_iter(model, opt, ds[i], args, dev)
            # warm-up: ONE WHOLE EPOCH (every crop of every view once), not eight iterations -- the optimiser's compact window / gradient / scratch
            # buffers grow to the largest window of the level and the caching allocator has seen every size before the clock starts.  With eight,
            # the timed loop contained one to three multi-GB hipMallocs per level (`reserved_changes_in_loop` below), normally 2 ms each -- and on some
            # boxes 1.2 s: the "stalled level" of rounds 5 and 6 (docs/measurement_log.md).  First-epoch allocations are real, once per pyramid
            # level; a rate over two epochs is not the place to charge them.
            nwarm = len(ds)
            for k in range(nwarm):
                one(order[k], 0)
            torch.cuda.synchronize()
            # the crop's texel window of every timed iteration (host integers: no synchronisation), for `roofline_iter`
            count_leaf = getattr(opt, "window_leaf", None) if getattr(model, "_window_opt", None) is opt else None
            if count_leaf is not None:
                def counting(window, plane_boxes=None, _orig=count_leaf):
                    win_texels[0] += int(window[2]) * int(window[3])
                    win_texels[1] += 1
                    return _orig(window, plane_boxes)
                opt.window_leaf = counting
            t0 = time.perf_counter()
            timed = order[nwarm:nwarm + epochs * len(ds)]
            # a device event, the host clock and the allocator's reserved bytes after every timed iteration: the median device time per iteration and the
            # longest interval (device and host, with their indices) go out beside the wall-clock rate, which stays THE rate.  What they found (round 6):
            # the rare "stalled level" -- one interval of 0.1 - 1.2 s -- is the HOST inside a multi-GB hipMalloc (a window buffer of the optimiser growing at
            # that iteration: `reserved_delta_at_host_max`), 2 ms on most boxes and a second on some.  The whole-epoch warm-up above takes the growth out of
            # the timed loop; the fields stay so that a recurrence reads as what it is.
            marks, host_t, reserved = [], [], []
            import gc
            gc_was = gc.isenabled()
            gc.disable()      # (no collector pause inside the timed loop: one suspect less for the rare stalled level; re-enabled right after it)
            for k, i in enumerate(timed):
                one(i, k // len(ds))
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                marks.append(ev)
                host_t.append(time.perf_counter())
                reserved.append(torch.cuda.memory_reserved(dev))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if gc_was:
                gc.enable()
            dgap = [marks[k - 1].elapsed_time(marks[k]) for k in range(1, len(marks))]
            hgap = [(host_t[k] - host_t[k - 1]) * 1e3 for k in range(1, len(marks))]
            gaps = sorted(dgap)
            kd, kh = int(np.argmax(dgap)), int(np.argmax(hgap))
            # (max / max_at: the longest device interval between two iterations' events and its index; host_max / host_max_at: the same on the host's clock
            # -- the enqueue side.  A device interval far above p50 WITH the same host interval at the same index is the host being away, not a kernel.)
            dev_ms = {"p50": gaps[len(gaps) // 2], "max": gaps[-1], "max_at": kd + 1, "host_max": hgap[kh], "host_max_at": kh + 1, "host_at_device_max": hgap[kd],
                      # the caching allocator's reserved bytes moved during the iteration of the longest host interval: a hipMalloc / hipFree inside it
                      "reserved_delta_at_host_max": int(reserved[kh + 1] - reserved[kh]), "reserved_changes_in_loop": int(sum(reserved[k] != reserved[k - 1] for k in range(1, len(reserved)))),
                      "stall_ms": dt * 1e3 - marks[0].elapsed_time(marks[-1]) * len(marks) / (len(marks) - 1),
                      "iters_per_s_without_intervals_over_20x_p50": (len(dgap) - sum(g > 20 * gaps[len(gaps) // 2] for g in dgap))
                      / max(1e-9, sum(g for g in dgap if g <= 20 * gaps[len(gaps) // 2]) * 1e-3)}
            if count_leaf is not None:
                opt.window_leaf = count_leaf
            if os.environ.get("VL3D_SCHED_DIAG"):      # measurement aid: the allocator's state after the level, the kernels of 12 more iterations
                from torch.profiler import profile, ProfilerActivity
                ms = torch.cuda.memory_stats()
                with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
                    for k in range(12):
                        one(order[k], 0)
                    torch.cuda.synchronize()
                top = [(e.key[:60], e.count, round(e.device_time_total / 12e3, 3), round(e.cpu_time_total / 12e3, 3))
                       for e in sorted(prof.key_averages(), key=lambda e: -max(e.device_time_total, e.cpu_time_total))[:14]]
                print("DIAG", hw, round(len(timed) / dt, 1), dev_ms, {k_: ms.get(k_) for k_ in ("num_device_alloc", "num_alloc_retries", "reserved_bytes.all.current",
                                                                                          "allocated_bytes.all.current")}, top, flush=True)
            total_it += len(timed)
            total_s += dt
            total_win[0] += win_texels[0]
            total_win[1] += win_texels[1]
            out["levels"].append({"frame": hw, "crops_per_view": len(ds) // views, "crops": len(ds), "iters": len(timed),
                                  "iters_per_s": len(timed) / dt, "stack": tuple(model.stack.shape[2:4]), "device_ms_per_iter": dev_ms})
            # instrumented pass (synchronising; not timed): how many steps had each tile of the crop's window missed?
            if hasattr(opt, "state") and getattr(model, "_window_opt", None) is opt:
                import videoloop3d_amd.optim as O
                ts = O.tile_side()
                orig = opt.window_leaf

                def spy(window, plane_boxes=None):
                    nonlocal depth_hist
                    st = opt.state.get(opt.p)
                    if st:
                        y0, x0, wh, ww = window
                        sub = st["last_step"][:, y0 // ts:-(-(y0 + wh) // ts), x0 // ts:-(-(x0 + ww) // ts)]
                        dep = np.bincount((opt.t - sub).clamp(min=0).flatten().cpu().numpy())
                        if len(dep) > len(depth_hist):
                            depth_hist = np.pad(depth_hist, (0, len(dep) - len(depth_hist)))
                        depth_hist[:len(dep)] += dep
                    return orig(window, plane_boxes)
                opt.window_leaf = spy
                for i in torch.randperm(len(ds), generator=gen).tolist():
                    one(i, epochs)
                opt.window_leaf = orig
    out["iters_per_s"] = total_it / total_s
    out["iters"] = total_it
    if total_win[1]:
        # the bytes a crop iteration MUST move: the window of the parameters read by the forward (1 stream), then read and written once
        # each with both Adam moments by the step (6 streams) -- 7 streams x D x T x 16 bytes per window texel (tile-culled: of the kept
        # texels) -- over the whole iteration's wall time (render, loss, regularisers, optimiser, host) against the 8 TB/s HBM peak
        kept = float(model.quad_keep.float().mean()) if sparsify else 1.0
        win = total_win[0] / total_win[1]
        nbytes = 7.0 * planes * frames * 16.0 * win * kept
        out["roofline_iter"] = {"bound": "hbm", "streams": 7, "mean_window_texels": win, "kept_fraction": kept, "compulsory_bytes": nbytes,
                                "ms_per_iter": total_s / total_it * 1e3, "achieved": nbytes / (total_s / total_it) / 1e9, "peak": 8000.0,
                                "unit": "GB/s", "frac": nbytes / (total_s / total_it) / 1e9 / 8000.0}
    if depth_hist.sum() > 0:
        c = np.cumsum(depth_hist) / depth_hist.sum()
        out["catchup_depth"] = {"mean": float((np.arange(len(depth_hist)) * depth_hist).sum() / depth_hist.sum()),
                                "p50": int(np.searchsorted(c, 0.5)), "p90": int(np.searchsorted(c, 0.9)), "max": int(len(depth_hist) - 1),
                                "histogram_by_8": [int(depth_hist[i:i + 8].sum()) for i in range(0, len(depth_hist), 8)]}
    out["shape"] = (f"V={views} views, D={planes}, T={frames}, clips of {clip} frames, 360x640 frames, crops 180x320 stride 90x160 at the last "
                    f"{levels} pyramid levels, {epochs} epochs per level, smooth {smooth}, {('tile-culled, tile-exact layout' if tile_exact else 'tile-culled') if sparsify else 'dense'} model{'' if sparsify else (', step inside the backward' if fused else ', backward + step kernel')}")
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--sparsify", action="store_true")
    ap.add_argument("--tile-exact", action="store_true", help="with --sparsify: every quad owns its tile, border texels included (the layout of a reference checkpoint)")
    ap.add_argument("--two-kernels", action="store_true", help="dense model: vl3d_render_bwd + the step kernel instead of the step inside the backward")
    ap.add_argument("--bwd-variant", type=int, default=0)
    ap.add_argument("--generic-objective", action="store_true", help="forward + weighted_total instead of MPMeshVid.objective")
    ap.add_argument("--gt-y4m", default=None, metavar="A.y4m,B.y4m", help="the views' clips from YUV4MPEG2 files (one per view, 360 x 640) instead of synthetic ones")
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    print(json.dumps(run(a.views, a.epochs, sparsify=a.sparsify, fused=not a.two_kernels, bwd_variant=a.bwd_variant, generic_objective=a.generic_objective,
                         tile_exact=a.tile_exact, gt_y4m=a.gt_y4m)))
