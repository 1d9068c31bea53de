#!/usr/bin/env python3
"""In-process A/B of the float forward against the baked forward at cfg3 (D = 32, T = 50, 720p; docs/kernels/K9_baked_playback.md).
Both stacks are resident (fp32 23.6 GB + RGBA8 5.9 GB), both renders take the same homographies, the legs alternate round by round under
HIP events on the launch stream; the float leg is the yardstick (the same kernel the parent commit ships, timed in this process).
  python profiles/baked_fwd.py [--warm 20] [--iters 100] [--rounds 10] [--D 32 --T 50 --H 720 --W 1280] [--legs all|dense|culled|path|display|times|open|trim|disparity|rgbd] [--out FILE]
Prints per leg: ms per call (median / min over the rounds), Mpix/s, and the fraction of 8 TB/s its ALGORITHMIC bytes amount to -- per pixel
and frame one texel per plane and 16 bytes of output: 16 D + 16 (float), 4 D + 16 (baked).

The CULLED pair (--legs culled, or all): the dense baked render WITH a quad map against the pool render (render_frame_run_baked_pool) of the
same texels, alternating in the same way.  The quad map: 35 x 63 quads per plane, one coherent blob per plane holding --keep (0.165) of the
plane's quads -- the nearest to the blob's centre -- of which the innermost --dyn (0.3) are dynamic; the pool is scattered from the baked clip
plane by plane, the dense leg's clip is the pool unpacked (texels without storage read culled_rgba8), the two outputs are compared bit for bit
before the timing.  Prints the two times, their ratio and the bytes of the pool against the dense baked clip.

The PATH leg (--legs path; not part of `all`): a spiral of --poses (120) cameras, pose i showing frame i % T, on three storages -- the dense baked
clip, the culled clip and the pool of the culled pair's map.  (a) the per-frame loop: one render_frame_run_baked / _pool call per pose (one
memset, one plan and one one-frame render launch each: what render_frames(baked=) issued along a spiral before the path render), the
yardstick; (b) ONE render_path_baked / _pool call.  The outputs are compared bit for bit first; then (a) and (b) alternate round by round
under HIP events that span the whole path.  Prints ms per frame of both (median, min .. max over the rounds) and their ratio; the condition is
path median <= loop median on every storage.

The DISPLAY leg (--legs display; not part of `all`): the same spiral and storages, the uint8 frames a viewer shows as the product, without a
background and over one.  (a) the yardstick, the route before the display output: ONE render_path_baked / _pool call into fp32 buffers, then
the torch epilogue (baked.display_frames and the copy into the uint8 result); (b) ONE path call with `frames8=`: RGB8 with the lane-packed
store, RGB8 with byte stores (VL3D_DISPLAY_STORE3=bytes), RGBA8.  Every (b) output is compared with (a)'s by torch.equal first (RGBA8: its
colour bytes, and its alpha byte with display_frames'); then the four legs alternate round by round under HIP events that span the whole
path.  Prints ms per frame (median, min .. max) and the ratio to (a); the condition is RGB8 (the store the library ships: packed) median <=
(a) median for every storage and background.

The TIMES leg (--legs times; not part of `all`): the same spiral and storages retimed from the loop's 25 fps to a 60 Hz display, loop time
tau_i = (i * 25 / 60) mod T, RGB8 frames as the product.  (a) the yardstick, the only retiming there was before the loop-time path: two path
calls (frames t0 and t1) into fp32 buffers, torch.lerp of rgb and alpha, baked.display_frames into the uint8 result -- an output cross-fade,
another picture but the same job; (b) ONE render_times_baked / _pool call into the display sink; (c), for the cost of the second frame, the
whole-frame path call of --legs display at t0.  First (b)'s float sink is compared on three frames with the float kernels on interpolated
texels (the comparison of tests/test_gpu_baked_times.py, bound 1e-5); then the three legs alternate round by round under HIP events that span
the whole path.  Prints ms per frame (median, min .. max), (b) / (a) -- the condition is (b) median <= (a) median on every storage -- and
(b) / (c).

The DISPARITY leg (--legs disparity; not part of `all`): the depth map beside the picture (include/vl3d.h "Disparity").  First the float
entry on the resident fp32 clip: (a) render_frame_run of the whole clip, (b) render_frame_run_disparity of it.  Then the spiral and the three
storages of the path leg: (a) ONE render_path_baked / _pool call into the float sink, (b) ONE render_path_disparity_baked / _pool call.  The
disparity call's alpha is compared with the colour call's by torch.equal first (the float entry: its zero pattern); the legs alternate round by
round under HIP events that span whole calls.  Prints ms per frame (median, min .. max) and (b) / (a); the expectation to check is
(b) median <= 1.05 (a) median -- the disparity call fetches the same texel lines, writes 8 instead of 16 bytes per pixel and computes less.

The RGBD leg (--legs rgbd; not part of `all`): colour AND depth from one launch (include/vl3d.h "RGB-D") on the same spiral and storages.  Per
storage and sink -- float (rgb, alpha, disp) and display (RGB8 + D16) -- (a) the colour path call plus the disparity path call of the same
source, the entries an RGB-D frame costs without it (for the display sink: the colour call's frames8 sink plus the fp32 disparity call; the
16-bit quantisation in torch that a consumer adds today is NOT counted), against (b) one RGB-D call.  (b)'s outputs are compared bit for
bit with (a)'s first.  A fourth pair: the loop-time RGB-D call (60 Hz times) against the loop-time colour call alone -- there is no depth twin.  ms per frame with
min..max, (b) / (a), bytes written per frame.

The TRIM leg (--legs trim; not part of `all`): BakedPool.trimmed() on the culled pair's model, in whose FLOAT stack, before it is baked, the
outermost --trim-invisible (0.25) of each plane's kept quads get the alpha logit -12 on the texels they can read and the outermost --trim-frozen
(0.5) of its dynamic quads repeat frame 0 (the shares of quads and of texels are printed).  The report (blocks, slots, bytes, quads), the ms of
trimmed() itself (5 calls), then the trimmed pool against the untrimmed one: the run of the whole clip and one path call of the spiral, outputs
compared bit for bit first, legs alternating round by round; the difference of the medians beside the trimmed leg's own min..max spread.

The OPEN leg (--legs open; not part of `all`; allocates neither stack): the scatter of a viewer package's atlases into the baked pool
(vl3d_pool_from_atlas_rgba8, baked.open_viewer_package).  The culled pair's quad map in the tile-exact layout (35 x 63 tiles of 21 x 21 texels:
planes of 735 x 1323), synthetic RGBA8 atlases packed like export._pack_tiles (atlas_grid, row major), resident on the device.  (a) the
yardstick, the only route to this pool without the kernel: per plane the atlases unpacked with torch gathers into (T,Hs,Ws,4) texels, then
PackedLayout.pack_plane_; (b) the T scatter calls.  The two pools are compared with torch.equal first; then (a) and (b) alternate under HIP
events.  Prints ms per pool and GB/s of pool written for both, their ratio (condition: (b) <= (a)), and -- separately -- the seconds
export.read_png takes for ONE dynamic atlas of this size on one thread (incompressible synthetic texels: an upper bound on inflate time)."""
import argparse
import json
import os
import statistics
import sys
import time

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
ap.add_argument("--legs", default="all", choices=["all", "dense", "culled", "path", "display", "times", "open", "trim", "disparity", "rgbd"])
ap.add_argument("--trim-invisible", type=float, default=0.25, help="--legs trim: the share of each plane's kept quads (the outermost of its blob) made invisible")
ap.add_argument("--trim-frozen", type=float, default=0.5, help="--legs trim: the share of each plane's dynamic quads (the outermost) that repeat frame 0")
ap.add_argument("--poses", type=int, default=120)
ap.add_argument("--keep", type=float, default=0.165)
ap.add_argument("--dyn", type=float, default=0.3)
ap.add_argument("--out", default="")
a = ap.parse_args()
assert a.warm >= 1 and a.iters >= a.rounds >= 1

import __graft_entry__ as ge  # noqa: E402
ge.build()
from videoloop3d_amd import synth  # noqa: E402
from videoloop3d_amd.baked import BakedPool, bake_texels, culled_texel_rgba8, display_frames, loop_times  # noqa: E402
from videoloop3d_amd.packed import PackedLayout  # noqa: E402
from videoloop3d_amd.render import (RenderSpec, depth_rows, render_frame_run, render_frame_run_baked, render_frame_run_baked_pool,  # noqa: E402
                                    render_frame_run_disparity, render_path_baked, render_path_baked_pool, render_path_disparity_baked,
                                    render_path_disparity_baked_pool, render_rgbd_baked, render_rgbd_baked_pool, render_times_baked,
                                    render_times_baked_pool)
from videoloop3d_amd.utils_mpi import compute_homography, make_depths  # noqa: E402

assert torch.cuda.is_available(), "profiles/baked_fwd.py measures on the MI355X"
dev = torch.device("cuda:0")
D, T, H, W = a.D, a.T, a.H, a.W
ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
homos = compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3),
                           make_depths(D, 1.0, 100.0).flip(0)[None])[0].to(dev)
spec = RenderSpec.mpv()
if a.legs != "open":
    stack = synth.make_plane_stack(D, T, H, W, seed=2, device=dev)
    baked = bake_texels(stack, "sigmoid", "sigmoid")
    out = (torch.empty((T, H, W, 3), device=dev), torch.empty((T, H, W), device=dev))


def ab(legs):
    """alternate the two legs round by round (and their order) under HIP events -> {leg: [ms per call of each round]}"""
    names = list(legs)
    for f in legs.values():
        for _ in range(a.warm):
            f()
    torch.cuda.synchronize()
    per = max(1, a.iters // a.rounds)
    ms = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in (names if r % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per):
                legs[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / per)
    return ms, per


res = {"config": {"D": D, "T": T, "H": H, "W": W, "warm": a.warm, "timed_calls_per_leg": max(1, a.iters // a.rounds) * a.rounds, "rounds": a.rounds,
                  "legs": a.legs},
       "stack_GB": {} if a.legs == "open" else {"float": stack.numel() * 4 / 1e9, "baked": baked.numel() / 1e9}}


def report(k, ms, per, bytes_px):
    med, lo = statistics.median(ms), min(ms)
    res[k] = {"ms_median": med, "ms_min": lo, "ms_max": max(ms), "Mpix_s": T * H * W / med / 1e3}
    line = f"{k:12s} forward: {med:7.3f} ms (min {lo:.3f}, max {max(ms):.3f} over {a.rounds} rounds of {per})  {res[k]['Mpix_s']:8.0f} Mpix/s"
    if bytes_px:
        res[k].update({"algorithmic_bytes_per_pixel": bytes_px, "fraction_of_8TBs": T * H * W * bytes_px / (med * 1e-3) / 8e12})
        line += f"  {bytes_px} B/pixel -> {res[k]['fraction_of_8TBs']:.3f} of 8 TB/s"
    print(line)


if a.legs in ("all", "dense"):
    ms, per = ab({"float": lambda: render_frame_run(stack, 0, T, homos, H, W, spec, out=out),
                  "baked": lambda: render_frame_run_baked(baked, 0, T, homos, H, W, spec, out=out)})
    report("float", ms["float"], per, 16 * D + 16)
    report("baked", ms["baked"], per, 4 * D + 16)
    res["speedup"] = res["float"]["ms_median"] / res["baked"]["ms_median"]
    res["byte_ratio"] = (16 * D + 16) / (4 * D + 16)
    print(f"baked is {res['speedup']:.2f}x the float forward (algorithmic byte ratio {res['byte_ratio']:.2f}x)")

def culled_maps():
    """the culled pair's quad maps: (keep, dyn) [D,35,63] bool on the device"""
    QH, QW = 35, 63                                       # 36 x 64 vertices
    qy, qx = torch.meshgrid(torch.arange(QH, device=dev), torch.arange(QW, device=dev), indexing="ij")
    n_keep = round(a.keep * QH * QW)
    n_dyn = round(a.dyn * n_keep)
    keep = torch.zeros((D, QH * QW), dtype=torch.bool, device=dev)
    dyn = torch.zeros_like(keep)
    for d in range(D):                                    # one coherent blob per plane: the quads nearest to its centre (in quad units of equal size on screen)
        cy, cx = (7 * d + 3) % QH, (11 * d + 5) % QW
        order = (((qy - cy) * (H / QH)) ** 2 + ((qx - cx) * (W / QW)) ** 2).flatten().argsort(stable=True)
        keep[d, order[:n_keep]] = True
        dyn[d, order[:n_dyn]] = True
    return keep.view(D, QH, QW), dyn.view(D, QH, QW)


def culled_model(baked):
    """the culled pair's model from the baked clip: (layout, pool, quad map uint8, BakedPool, the pool unpacked as a dense clip)"""
    keep, dyn = culled_maps()
    QH, QW = keep.shape[1:]
    lay = PackedLayout(keep, dyn, T, H, W)
    pool = torch.zeros((lay.n_slots * 64, 4), dtype=torch.uint8, device=dev)
    for d in range(D):
        lay.pack_plane_(pool, d, baked[d])
    qk = keep.to(torch.uint8).contiguous()
    bp = BakedPool(pool, lay, qk, spec, "", None, culled_texel_rgba8("sigmoid", "sigmoid"))
    dense = bp.unpack_frames(range(T))                    # the clip the dense leg reads: the SAME texels, culled_rgba8 where nothing is stored
    res["culled_map"] = {"QH": QH, "QW": QW, "kept": float(keep.float().mean()), "dynamic_of_kept": float(dyn.sum()) / float(keep.sum()),
                         "blocks_static": lay.n_static, "blocks_dynamic": lay.n_dynamic, "blocks_unstored": int((lay.blocks < 0).sum()),
                         "pool_bytes": bp.nbytes, "dense_baked_bytes": dense.numel()}
    return lay, pool, qk, bp, dense


def trim_edit_(stack):
    """--legs trim: something to trim in the culled pair's model, in the FLOAT stack before it is baked -- per plane the outermost --trim-invisible of
    the blob's kept quads get the alpha logit -12 (byte 0) on the texels they can read, the outermost --trim-frozen of its dynamic quads repeat
    frame 0 on theirs.  -> the shares, for the record"""
    from videoloop3d_amd import tiles
    keep, dyn = culled_maps()
    QH, QW = keep.shape[1:]
    qy, qx = torch.meshgrid(torch.arange(QH, device=dev), torch.arange(QW, device=dev), indexing="ij")
    invisible, frozen = torch.zeros_like(keep).view(D, -1), torch.zeros_like(keep).view(D, -1)
    for d in range(D):
        cy, cx = (7 * d + 3) % QH, (11 * d + 5) % QW      # culled_maps' blob centre and order
        order = (((qy - cy) * (H / QH)) ** 2 + ((qx - cx) * (W / QW)) ** 2).flatten().argsort(stable=True)
        n_keep, n_dyn = int(keep[d].sum()), int(dyn[d].sum())
        invisible[d, order[n_keep - round(a.trim_invisible * n_keep):n_keep]] = True
        frozen[d, order[n_dyn - round(a.trim_frozen * n_dyn):n_dyn]] = True
    inv_t = tiles.quad_to_texel_mask(invisible.view(D, QH, QW), H, W)
    fr_t = tiles.quad_to_texel_mask(frozen.view(D, QH, QW), H, W)
    for d in range(D):
        stack[d] = torch.where(fr_t[d, None, :, :, None], stack[d, :1], stack[d])
        stack[d, ..., 3].masked_fill_(inv_t[d, None], -12.0)
    return {"invisible_quads_of_kept": float(invisible.sum()) / float(keep.sum()), "frozen_quads_of_dynamic": float(frozen.sum()) / float(dyn.sum()),
            "invisible_texels_of_kept_texels": float(inv_t.sum()) / float(tiles.quad_to_texel_mask(keep, H, W).sum()),
            "frozen_texels_of_dynamic_texels": float(fr_t.sum()) / float(tiles.quad_to_texel_mask(dyn, H, W).sum())}


if a.legs == "trim":
    res["trim_model"] = trim_edit_(stack)
    baked = bake_texels(stack, "sigmoid", "sigmoid")
    print(f"trim model: the culled pair's map with {res['trim_model']}")

if a.legs in ("all", "culled"):
    del stack
    lay, pool, qk, bp, dense = culled_model(baked)
    del baked
    QH, QW = res["culled_map"]["QH"], res["culled_map"]["QW"]
    out2 = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    render_frame_run_baked(dense, 0, T, homos, H, W, spec, out=out, quad_keep=qk)
    render_frame_run_baked_pool(lay, pool, 0, T, homos, H, W, spec, out=out2, quad_keep=qk, culled_rgba8=bp.culled_rgba8)
    same = torch.equal(out[0], out2[0]) and torch.equal(out[1], out2[1])
    covered = float((out[1] > 0).float().mean())
    del out2
    res["culled_map"].update({"outputs_bit_equal": same, "covered_pixels": covered})
    print(f"culled map: {QH} x {QW} quads, {res['culled_map']['kept']:.3f} kept, {res['culled_map']['dynamic_of_kept']:.3f} of them dynamic; blocks "
          f"static {lay.n_static} / dynamic {lay.n_dynamic} / unstored {res['culled_map']['blocks_unstored']}; pool {bp.nbytes / 1e9:.3f} GB against "
          f"{dense.numel() / 1e9:.3f} GB dense baked ({dense.numel() / bp.nbytes:.1f}x); outputs bit-equal: {same}; covered pixels {covered:.3f}")
    ms, per = ab({"baked_culled": lambda: render_frame_run_baked(dense, 0, T, homos, H, W, spec, out=out, quad_keep=qk),
                  "baked_pool": lambda: render_frame_run_baked_pool(lay, pool, 0, T, homos, H, W, spec, out=out, quad_keep=qk, culled_rgba8=bp.culled_rgba8)})
    report("baked_culled", ms["baked_culled"], per, 0)
    report("baked_pool", ms["baked_pool"], per, 0)
    res["pool_over_dense_culled"] = res["baked_pool"]["ms_median"] / res["baked_culled"]["ms_median"]
    print(f"pool render is {res['pool_over_dense_culled']:.3f}x the dense culled baked render's time (bar: <= 1.05)")

if a.legs == "disparity":
    # the float entry while the fp32 clip is resident: the whole clip as one run, colour against disparity
    rows1 = depth_rows(tar_e.double() @ torch.linalg.inv(ref_e.double()), Kt, make_depths(D, 1.0, 100.0).flip(0)).to(dev)
    d_out = (torch.empty((T, H, W), device=dev), torch.empty((T, H, W), device=dev))
    legs = {"a_colour": lambda: render_frame_run(stack, 0, T, homos, H, W, spec, out=out),
            "b_disparity": lambda: render_frame_run_disparity(stack, 0, T, homos, rows1, H, W, spec, out=d_out)}
    for f in legs.values():
        f()
    same = torch.equal(out[1] == 0, d_out[1] == 0)
    ms, per = ab(legs)
    med = {k: statistics.median(v) for k, v in ms.items()}
    res["disparity"] = {"float": {"alpha_zero_pattern_equal": same, "covered_pixels": float((d_out[1] > 0).float().mean()), "max_disp": float(d_out[0].max()),
                                  "disparity_over_colour": med["b_disparity"] / med["a_colour"], "expectation_le_1.05": bool(med["b_disparity"] <= 1.05 * med["a_colour"]),
                                  "legs": {k: {"ms_per_frame_median": med[k] / T, "min": min(ms[k]) / T, "max": max(ms[k]) / T} for k in legs}}}
    for k in legs:
        print(f"disparity [float ] {k:12s} {med[k] / T:.4f} ms/frame ({min(ms[k]) / T:.4f} .. {max(ms[k]) / T:.4f}) over {a.rounds} rounds of {per} runs of {T}", flush=True)
    print(f"disparity [float ] alpha zero pattern equal {same}; (b) / (a) {med['b_disparity'] / med['a_colour']:.3f} -> "
          f"{'ok' if med['b_disparity'] <= 1.05 * med['a_colour'] else 'ABOVE 1.05'}", flush=True)
    del d_out, legs

if a.legs in ("path", "display", "times", "trim", "disparity", "rgbd"):
    import math
    del stack, out
    N = a.poses
    hs, es = [], []
    for i in range(N):                                    # the spiral of examples/playback.py around the benchmark camera's rotation
        ang = 2 * math.pi * i / N
        e = tar_e.clone()
        e[:3, 3] = torch.tensor([0.05 * math.cos(ang), 0.03 * math.sin(ang), 0.01 * math.sin(2 * ang)])
        es.append(e)
        hs.append(compute_homography(ref_e[None], Kr[None], e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3),
                                     make_depths(D, 1.0, 100.0).flip(0)[None])[0])
    path_homos = torch.stack(hs).float().to(dev)          # [N, D, 3, 3]
    cam, ts = list(range(N)), [i % T for i in range(N)]
    lay, pool, qk, bp, dense = culled_model(baked)
    kwp = dict(quad_keep=qk, culled_rgba8=bp.culled_rgba8)

if a.legs == "path":
    o_loop = (torch.empty((N, H, W, 3), device=dev), torch.empty((N, H, W), device=dev))
    o_path = (torch.empty_like(o_loop[0]), torch.empty_like(o_loop[1]))

    def loop_of(one):
        def f():
            for i in range(N):
                one(ts[i], path_homos[i], (o_loop[0][i:i + 1], o_loop[1][i:i + 1]))
        return f
    storages = {
        "dense": (loop_of(lambda t, h, o: render_frame_run_baked(baked, t, 1, h, H, W, spec, out=o)),
                  lambda: render_path_baked(baked, cam, ts, path_homos, H, W, spec, out=o_path)),
        "culled": (loop_of(lambda t, h, o: render_frame_run_baked(dense, t, 1, h, H, W, spec, out=o, quad_keep=qk)),
                   lambda: render_path_baked(dense, cam, ts, path_homos, H, W, spec, out=o_path, quad_keep=qk)),
        "pool": (loop_of(lambda t, h, o: render_frame_run_baked_pool(lay, pool, t, 1, h, H, W, spec, out=o, **kwp)),
                 lambda: render_path_baked_pool(lay, pool, cam, ts, path_homos, H, W, spec, out=o_path, **kwp)),
    }
    res["path"] = {"poses": N}
    for name, (loop, path) in storages.items():
        o_loop[0].fill_(-1.0), o_path[0].fill_(-2.0)
        loop()
        path()
        same = torch.equal(o_loop[0], o_path[0]) and torch.equal(o_loop[1], o_path[1])
        ms, per = ab({"loop": loop, "path": path})
        ml, mp = statistics.median(ms["loop"]), statistics.median(ms["path"])
        res["path"][name] = {"outputs_bit_equal": same, "covered_pixels": float((o_path[1] > 0).float().mean()),
                             "loop_ms_per_frame": {"median": ml / N, "min": min(ms["loop"]) / N, "max": max(ms["loop"]) / N},
                             "path_ms_per_frame": {"median": mp / N, "min": min(ms["path"]) / N, "max": max(ms["path"]) / N},
                             "path_over_loop": mp / ml, "condition_path_le_loop": bool(mp <= ml)}
        print(f"path [{name:6s}] bit-equal {same}; loop {ml / N:.4f} ms/frame ({min(ms['loop']) / N:.4f} .. {max(ms['loop']) / N:.4f}), "
              f"path {mp / N:.4f} ms/frame ({min(ms['path']) / N:.4f} .. {max(ms['path']) / N:.4f}) over {a.rounds} rounds of {per} paths of {N}; "
              f"path / loop {mp / ml:.3f} -> {'ok' if mp <= ml else 'MISSED'}")
if a.legs == "disparity":
    to_ref = torch.linalg.inv(ref_e.double())
    path_rows = depth_rows(torch.stack([e.double() @ to_ref for e in es]), Kt, make_depths(D, 1.0, 100.0).flip(0)).to(dev)      # [N, D, 3]
    o_c = (torch.empty((N, H, W, 3), device=dev), torch.empty((N, H, W), device=dev))
    o_d = (torch.empty((N, H, W), device=dev), torch.empty((N, H, W), device=dev))
    storages = {
        "dense": (lambda: render_path_baked(baked, cam, ts, path_homos, H, W, spec, out=o_c),
                  lambda: render_path_disparity_baked(baked, cam, ts, path_homos, path_rows, H, W, spec, out=o_d)),
        "culled": (lambda: render_path_baked(dense, cam, ts, path_homos, H, W, spec, out=o_c, quad_keep=qk),
                   lambda: render_path_disparity_baked(dense, cam, ts, path_homos, path_rows, H, W, spec, out=o_d, quad_keep=qk)),
        "pool": (lambda: render_path_baked_pool(lay, pool, cam, ts, path_homos, H, W, spec, out=o_c, **kwp),
                 lambda: render_path_disparity_baked_pool(lay, pool, cam, ts, path_homos, path_rows, H, W, spec, out=o_d, **kwp)),
    }
    res["disparity"]["poses"] = N
    for name, (colour, disparity) in storages.items():
        o_c[1].fill_(-1.0), o_d[1].fill_(-2.0)
        colour()
        disparity()
        same = torch.equal(o_c[1], o_d[1])
        ms, per = ab({"a_colour": colour, "b_disparity": disparity})
        ma, mb = statistics.median(ms["a_colour"]), statistics.median(ms["b_disparity"])
        res["disparity"][name] = {"alpha_bit_equal": same, "covered_pixels": float((o_d[1] > 0).float().mean()), "max_disp": float(o_d[0].max()),
                                  "colour_ms_per_frame": {"median": ma / N, "min": min(ms["a_colour"]) / N, "max": max(ms["a_colour"]) / N},
                                  "disparity_ms_per_frame": {"median": mb / N, "min": min(ms["b_disparity"]) / N, "max": max(ms["b_disparity"]) / N},
                                  "disparity_over_colour": mb / ma, "expectation_le_1.05": bool(mb <= 1.05 * ma)}
        print(f"disparity [{name:6s}] alpha bit-equal {same}; colour {ma / N:.4f} ms/frame ({min(ms['a_colour']) / N:.4f} .. {max(ms['a_colour']) / N:.4f}), "
              f"disparity {mb / N:.4f} ms/frame ({min(ms['b_disparity']) / N:.4f} .. {max(ms['b_disparity']) / N:.4f}) over {a.rounds} rounds of {per} paths of {N}; "
              f"(b) / (a) {mb / ma:.3f} -> {'ok' if mb <= 1.05 * ma else 'ABOVE 1.05'}", flush=True)
if a.legs == "rgbd":
    to_ref = torch.linalg.inv(ref_e.double())
    path_rows = depth_rows(torch.stack([e.double() @ to_ref for e in es]), Kt, make_depths(D, 1.0, 100.0).flip(0), normalise=(1.0, 100.0)).to(dev)
    tau = loop_times([i * 25.0 / 60.0 for i in range(N)], T)
    o_c = (torch.empty((N, H, W, 3), device=dev), torch.empty((N, H, W), device=dev))
    o_d = (torch.empty((N, H, W), device=dev), torch.empty((N, H, W), device=dev))
    o_r = (torch.empty((N, H, W, 3), device=dev), torch.empty((N, H, W), device=dev), torch.empty((N, H, W), device=dev))
    f_c, f_r = (torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(2))
    d16 = torch.empty((N, H, W), dtype=torch.uint16, device=dev)
    srcs = {
        "dense": (lambda **o: render_path_baked(baked, cam, ts, path_homos, H, W, spec, **o),
                  lambda: render_path_disparity_baked(baked, cam, ts, path_homos, path_rows, H, W, spec, out=o_d),
                  lambda **o: render_rgbd_baked(baked, path_homos, path_rows, H, W, spec, **o),
                  lambda **o: render_times_baked(baked, cam, tau, path_homos, H, W, spec, **o)),
        "culled": (lambda **o: render_path_baked(dense, cam, ts, path_homos, H, W, spec, quad_keep=qk, **o),
                   lambda: render_path_disparity_baked(dense, cam, ts, path_homos, path_rows, H, W, spec, out=o_d, quad_keep=qk),
                   lambda **o: render_rgbd_baked(dense, path_homos, path_rows, H, W, spec, quad_keep=qk, **o),
                   lambda **o: render_times_baked(dense, cam, tau, path_homos, H, W, spec, quad_keep=qk, **o)),
        "pool": (lambda **o: render_path_baked_pool(lay, pool, cam, ts, path_homos, H, W, spec, **kwp, **o),
                 lambda: render_path_disparity_baked_pool(lay, pool, cam, ts, path_homos, path_rows, H, W, spec, out=o_d, **kwp),
                 lambda **o: render_rgbd_baked_pool(lay, pool, path_homos, path_rows, H, W, spec, **kwp, **o),
                 lambda **o: render_times_baked_pool(lay, pool, cam, tau, path_homos, H, W, spec, **kwp, **o)),
    }
    px = H * W
    res["rgbd"] = {"poses": N, "bytes_written_per_frame": {"float_rgbd": px * 20, "float_colour_plus_disparity": px * (16 + 8),
                                                           "display_rgbd": px * 5, "display_colour_plus_disparity": px * (3 + 8)}}
    for name, (colour, disparity, rgbd, times) in srcs.items():
        # the outputs first: (b) has (a)'s bits
        colour(out=o_c), disparity(), rgbd(path=(cam, ts), out=o_r)
        same_f = torch.equal(o_r[0], o_c[0]) and torch.equal(o_r[1], o_c[1]) and torch.equal(o_r[2], o_d[0])
        colour(frames8=f_c), rgbd(path=(cam, ts), frames8=f_r, depth16=d16)
        same_d = torch.equal(f_r, f_c) and all(torch.equal(d16[i].to(torch.int32), (65535 * o_d[0][i].clamp(0, 1)).to(torch.int32)) for i in range(0, N, 17))
        pairs = {
            "float": {"a_colour_then_disparity": lambda: (colour(out=o_c), disparity()), "b_rgbd": lambda: rgbd(path=(cam, ts), out=o_r)},
            "display": {"a_colour8_then_disparity": lambda: (colour(frames8=f_c), disparity()),
                        "b_rgbd": lambda: rgbd(path=(cam, ts), frames8=f_r, depth16=d16)},
            "times_float": {"a_colour_times_alone": lambda: times(out=o_c), "b_rgbd_times": lambda: rgbd(times=(cam, tau), out=o_r)},
            "times_display": {"a_colour8_times_alone": lambda: times(frames8=f_c),
                              "b_rgbd_times": lambda: rgbd(times=(cam, tau), frames8=f_r, depth16=d16)},
        }
        res["rgbd"][name] = {"float_bit_equal": same_f, "display_bit_equal": same_d, "covered_pixels": float((o_d[1] > 0).float().mean())}
        for pair, legs in pairs.items():
            ms, per = ab(legs)
            med = {k: statistics.median(v) for k, v in ms.items()}
            first = next(iter(legs))
            res["rgbd"][name][pair] = {k: {"ms_per_frame_median": med[k] / N, "min": min(ms[k]) / N, "max": max(ms[k]) / N, "over_a": med[k] / med[first]}
                                       for k in legs}
            print(f"rgbd [{name:6s} | {pair:13s}] bit-equal float {same_f} display {same_d}; " +
                  "; ".join(f"{k} {med[k] / N:.4f} ms/frame ({min(ms[k]) / N:.4f} .. {max(ms[k]) / N:.4f}) x{med[k] / med[first]:.3f}" for k in legs) +
                  f" over {a.rounds} rounds of {per} paths of {N}", flush=True)
if a.legs == "display":
    o_f = (torch.empty((N, H, W, 3), device=dev), torch.empty((N, H, W), device=dev))
    f_a, f_3, f_4 = (torch.empty((N, H, W, c), dtype=torch.uint8, device=dev) for c in (3, 3, 4))
    paths = {"dense": lambda **o: render_path_baked(baked, cam, ts, path_homos, H, W, spec, **o),
             "culled": lambda **o: render_path_baked(dense, cam, ts, path_homos, H, W, spec, quad_keep=qk, **o),
             "pool": lambda **o: render_path_baked_pool(lay, pool, cam, ts, path_homos, H, W, spec, **kwp, **o)}
    res["display"] = {"poses": N, "shipped_rgb8_store": "packed"}
    for name, path in paths.items():
        for bg in (None, (0.2, 0.4, 0.6)):
            bg_dev = None if bg is None else torch.tensor(bg, dtype=torch.float32, device=dev)

            def leg_a():      # the route before the display output: fp32 frames, the torch epilogue, the copy into the uint8 result
                path(out=o_f)
                f_a[:] = display_frames(o_f[0], o_f[1], bg_dev, 3)

            def leg_b(store, frames):
                def f():
                    os.environ["VL3D_DISPLAY_STORE3"] = store
                    path(frames8=frames, bg=bg)
                return f
            legs = {"a_float_then_torch": leg_a, "b_rgb8_packed": leg_b("packed", f_3), "b_rgb8_bytes": leg_b("bytes", f_3),
                    "b_rgba8": leg_b("packed", f_4)}
            leg_a()
            same = {}
            for k in ("b_rgb8_packed", "b_rgb8_bytes"):
                f_3.fill_(0xAB)
                legs[k]()
                same[k] = torch.equal(f_3, f_a)
            f_4.fill_(0xAB)
            legs["b_rgba8"]()
            same["b_rgba8"] = torch.equal(f_4[..., :3], f_a) and torch.equal(f_4[..., 3], display_frames(o_f[0], o_f[1], None, 4)[..., 3])
            ms, per = ab(legs)
            med = {k: statistics.median(v) for k, v in ms.items()}
            key = f"{name}{'_bg' if bg else ''}"
            res["display"][key] = {"outputs_equal": same, "condition_rgb8_le_yardstick": bool(med["b_rgb8_packed"] <= med["a_float_then_torch"]),
                                   "legs": {k: {"ms_per_frame_median": med[k] / N, "min": min(ms[k]) / N, "max": max(ms[k]) / N,
                                                "over_yardstick": med[k] / med["a_float_then_torch"]} for k in legs}}
            for k in legs:
                verdict = "" if k != "b_rgb8_packed" else (" -> ok" if med[k] <= med["a_float_then_torch"] else " -> MISSED")
                print(f"display [{name:6s} {'bg   ' if bg else 'no bg'}] {k:20s} {med[k] / N:.4f} ms/frame ({min(ms[k]) / N:.4f} .. {max(ms[k]) / N:.4f}) "
                      f"{med[k] / med['a_float_then_torch']:.3f} of (a); equal to (a): {same.get(k, '-')}{verdict}", flush=True)
    os.environ.pop("VL3D_DISPLAY_STORE3", None)
if a.legs == "times":
    import numpy as np
    from videoloop3d_amd.render_video import retime
    tau = loop_times(retime(N, 60, 25), T)                # float32 [N] in [0, T)
    t0s = np.floor(tau).astype(np.int64)
    t1s = np.where(t0s + 1 < T, t0s + 1, 0)
    frac = torch.from_numpy(tau - t0s.astype(np.float32)).to(dev)
    o_0 = (torch.empty((N, H, W, 3), device=dev), torch.empty((N, H, W), device=dev))
    o_1 = (torch.empty_like(o_0[0]), torch.empty_like(o_0[1]))
    f_a, f_b, f_c = (torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(3))
    ident = RenderSpec.mpv(rgb_act="none", alpha_act="none")      # the oracle renders decoded texels: nothing to activate
    storages = {"dense": (lambda ts_, **o: render_path_baked(baked, cam, ts_, path_homos, H, W, spec, **o),
                          lambda **o: render_times_baked(baked, cam, tau, path_homos, H, W, spec, **o), baked, None),
                "culled": (lambda ts_, **o: render_path_baked(dense, cam, ts_, path_homos, H, W, spec, quad_keep=qk, **o),
                           lambda **o: render_times_baked(dense, cam, tau, path_homos, H, W, spec, quad_keep=qk, **o), dense, qk),
                "pool": (lambda ts_, **o: render_path_baked_pool(lay, pool, cam, ts_, path_homos, H, W, spec, **kwp, **o),
                         lambda **o: render_times_baked_pool(lay, pool, cam, tau, path_homos, H, W, spec, **kwp, **o), dense, qk)}
    res["times"] = {"poses": N, "fps_out": 60, "fps_loop": 25, "fractional_frames": int((frac > 0).sum())}
    for name, (path, times, clip, keep_map) in storages.items():
        bg = (0.2, 0.4, 0.6)
        bg_dev = torch.tensor(bg, dtype=torch.float32, device=dev)
        # (b) against the float kernels on interpolated texels, three frames: the first fractional one, the middle, the last
        times(out=o_0)
        worst = [0.0, 0.0]
        for i in (1, N // 2 + 1, N - 1):
            d0, d1 = clip[:, int(t0s[i])].float() / 255, clip[:, int(t1s[i])].float() / 255
            s1 = (d0 + float(frac[i]) * (d1 - d0))[:, None].contiguous()
            r, al = render_frame_run(s1, 0, 1, path_homos[i], H, W, ident, quad_keep=keep_map)
            worst = [max(worst[0], float((o_0[0][i] - r[0]).abs().max())), max(worst[1], float((o_0[1][i] - al[0]).abs().max()))]
            del d0, d1, s1, r, al
        parity_ok = worst[0] <= 1e-5 and worst[1] <= 1e-5

        def leg_a():      # two whole-frame path calls, the cross-fade and the display rule in torch
            path(t0s, out=o_0)
            path(t1s, out=o_1)
            f_a[:] = display_frames(torch.lerp(o_0[0], o_1[0], frac[:, None, None, None]), torch.lerp(o_0[1], o_1[1], frac[:, None, None]), bg_dev, 3)

        def leg_b():
            times(frames8=f_b, bg=bg)

        def leg_c():
            path(t0s, frames8=f_c, bg=bg)
        legs = {"a_two_paths_lerp_torch": leg_a, "b_times_rgb8": leg_b, "c_whole_frame_rgb8": leg_c}
        for f in legs.values():
            f()
        level = int((f_a.int() - f_b.int()).abs().max())      # a cross-fade of outputs is another picture: reported, not required to be 0
        ms, per = ab(legs)
        med = {k: statistics.median(v) for k, v in ms.items()}
        ok = med["b_times_rgb8"] <= med["a_two_paths_lerp_torch"]
        res["times"][name] = {"parity_max_abs": {"rgb": worst[0], "alpha": worst[1], "ok": parity_ok}, "max_level_diff_b_vs_a": level,
                              "condition_times_le_yardstick": bool(ok), "times_over_yardstick": med["b_times_rgb8"] / med["a_two_paths_lerp_torch"],
                              "times_over_whole_frame": med["b_times_rgb8"] / med["c_whole_frame_rgb8"],
                              "legs": {k: {"ms_per_frame_median": med[k] / N, "min": min(ms[k]) / N, "max": max(ms[k]) / N} for k in legs}}
        print(f"times [{name:6s}] parity with the float kernels on 3 frames: max |d rgb| {worst[0]:.3e}, |d alpha| {worst[1]:.3e} -> "
              f"{'ok' if parity_ok else 'MISSED'}; (b) against (a): max level diff {level}")
        for k in legs:
            print(f"times [{name:6s}] {k:24s} {med[k] / N:.4f} ms/frame ({min(ms[k]) / N:.4f} .. {max(ms[k]) / N:.4f})", flush=True)
        print(f"times [{name:6s}] (b) / (a) {med['b_times_rgb8'] / med['a_two_paths_lerp_torch']:.3f} -> {'ok' if ok else 'MISSED'}; "
              f"(b) / (c), the cost of the second frame: {med['b_times_rgb8'] / med['c_whole_frame_rgb8']:.3f}", flush=True)
if a.legs == "trim":
    # the trimmed pool against the untrimmed one of the same visit: the same kernels with fewer loads.  Outputs first, then the run of the whole clip
    # and one path call of the spiral, legs alternating
    del baked, dense
    times = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        lean = bp.trimmed()
        torch.cuda.synchronize(); times.append((time.perf_counter() - t0) * 1e3)
    res["trim"] = {"report": lean.trim_report, "trimmed_ms": {"median": statistics.median(times), "min": min(times), "max": max(times), "calls": len(times)},
                   "pool_MB": {"before": bp.nbytes / 1e6, "after": lean.nbytes / 1e6}}
    print(f"trimmed(): {res['trim']['report']}\n  pool {bp.nbytes / 1e6:.1f} -> {lean.nbytes / 1e6:.1f} MB; conversion {statistics.median(times):.2f} ms (min {min(times):.2f}, max {max(times):.2f} of {len(times)})")
    kwl = dict(quad_keep=lean.quad_keep, culled_rgba8=lean.culled_rgba8)
    o_a = (torch.empty((T, H, W, 3), device=dev), torch.empty((T, H, W), device=dev))
    o_b = (torch.empty_like(o_a[0]), torch.empty_like(o_a[1]))
    render_frame_run_baked_pool(lay, pool, 0, T, homos, H, W, spec, out=o_a, **kwp)
    render_frame_run_baked_pool(lean.layout, lean.pool, 0, T, homos, H, W, spec, out=o_b, **kwl)
    same_run = torch.equal(o_a[0], o_b[0]) and torch.equal(o_a[1], o_b[1])
    covered = float((o_a[1] > 0).float().mean())
    del o_b
    p_a = (torch.empty((N, H, W, 3), device=dev), torch.empty((N, H, W), device=dev))
    p_b = (torch.empty_like(p_a[0]), torch.empty_like(p_a[1]))
    render_path_baked_pool(lay, pool, cam, ts, path_homos, H, W, spec, out=p_a, **kwp)
    render_path_baked_pool(lean.layout, lean.pool, cam, ts, path_homos, H, W, spec, out=p_b, **kwl)
    same_path = torch.equal(p_a[0], p_b[0]) and torch.equal(p_a[1], p_b[1])
    del p_b
    res["trim"].update({"run_outputs_bit_equal": same_run, "path_outputs_bit_equal": same_path, "covered_pixels": covered})
    print(f"outputs bit-equal: run of {T} frames {same_run}, path of {N} poses {same_path}; covered pixels {covered:.3f}")
    assert same_run and same_path
    for what, legs in (("run", {"pool": lambda: render_frame_run_baked_pool(lay, pool, 0, T, homos, H, W, spec, out=o_a, **kwp),
                                "trimmed": lambda: render_frame_run_baked_pool(lean.layout, lean.pool, 0, T, homos, H, W, spec, out=o_a, **kwl)}),
                       ("path", {"pool": lambda: render_path_baked_pool(lay, pool, cam, ts, path_homos, H, W, spec, out=p_a, **kwp),
                                 "trimmed": lambda: render_path_baked_pool(lean.layout, lean.pool, cam, ts, path_homos, H, W, spec, out=p_a, **kwl)})):
        ms, per = ab(legs)
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(ms["trimmed"]) - min(ms["trimmed"])
        res["trim"][what] = {k: {"ms_median": med[k], "ms_min": min(ms[k]), "ms_max": max(ms[k])} for k in legs}
        res["trim"][what].update({"trimmed_minus_pool_ms": med["trimmed"] - med["pool"], "trimmed_leg_spread_ms": spread,
                                  "within_spread": med["trimmed"] - med["pool"] <= spread})
        print(f"{what}: pool {med['pool']:.3f} ms (min {min(ms['pool']):.3f}, max {max(ms['pool']):.3f}), trimmed {med['trimmed']:.3f} ms (min {min(ms['trimmed']):.3f}, "
              f"max {max(ms['trimmed']):.3f}) over {a.rounds} rounds of {per}; trimmed - pool {med['trimmed'] - med['pool']:+.3f} ms, the trimmed leg's spread {spread:.3f} ms")

if a.legs == "open":
    import tempfile
    import time
    from videoloop3d_amd.baked import atlas_tile_map, pool_from_atlas_
    from videoloop3d_amd.export import atlas_grid, read_png, write_png
    keep, dyn = culled_maps()
    QH, QW = keep.shape[1:]
    th = tw = 21                                          # 35 x 63 tiles of 21 x 21: planes of 735 x 1323 texels
    Hs, Ws = QH * th, QW * tw
    lay = PackedLayout(keep, dyn, T, Hs, Ws, (th, tw))
    culled = culled_texel_rgba8("sigmoid", "sigmoid")
    tile_src = torch.full((D * QH * QW,), -1, dtype=torch.int32)
    grids, atlases = [], []
    for mesh, mask in enumerate((keep & ~dyn, dyn)):      # tile k of a mesh = its k-th quad in (d, qy, qx) order, as export._pack_tiles numbers them
        idx = mask.flatten().nonzero()[:, 0].cpu()
        tile_src[idx] = (torch.arange(len(idx), dtype=torch.int32) << 1) | mesh
        gh, gw, _ = atlas_grid(len(idx))
        grids.append((gh, gw))
        atlases.append(torch.randint(0, 256, ((T if mesh else 1), gh * th, gw * tw, 4), dtype=torch.uint8, device=dev))
    static, dyn_all = atlases[0][0], atlases[1]
    tile_src = tile_src.view(D, QH, QW)
    tm = atlas_tile_map(tile_src, lay, tuple(static.shape[:2]), tuple(dyn_all.shape[1:3]))
    pool_k = torch.full((lay.n_slots * 64, 4), 0xAB, dtype=torch.uint8, device=dev)
    pool_t = torch.zeros_like(pool_k)
    # the yardstick's gather indices, per plane [Hs,Ws]: the texel's index in its (flattened) atlas, its mesh, kept or not -- built once, like tile_src
    yy, xx = torch.meshgrid(torch.arange(Hs, device=dev), torch.arange(Ws, device=dev), indexing="ij")
    src_t = tm.dev[:, yy // th, xx // tw].long()          # D,Hs,Ws
    k_t, mesh_t = (src_t >> 1).clamp_min(0), (src_t & 1).bool() & (src_t >= 0)
    gw_t = torch.where(mesh_t, grids[1][1], grids[0][1])
    aw_t = torch.where(mesh_t, dyn_all.shape[2], static.shape[1])
    flat_t = ((k_t // gw_t) * th + yy % th) * aw_t + (k_t % gw_t) * tw + xx % tw
    kept_t = src_t >= 0
    del src_t, k_t, gw_t, aw_t
    fill = torch.tensor([(culled >> (8 * k)) & 0xff for k in range(4)], dtype=torch.uint8, device=dev)
    static_f, dyn_f = static.view(-1, 4), dyn_all.view(T, -1, 4)

    def leg_torch():
        for d in range(D):
            s_idx = torch.where(mesh_t[d], 0, flat_t[d])
            d_idx = torch.where(mesh_t[d], flat_t[d], 0)
            plane = torch.where(mesh_t[d][None, ..., None], dyn_f[:, d_idx], static_f[s_idx][None])
            plane = torch.where(kept_t[d][None, ..., None], plane, fill)
            lay.pack_plane_(pool_t, d, plane)

    def leg_kernel():
        for t in range(T):
            pool_from_atlas_(lay, pool_k, tm, static, dyn_all[t], t, culled)
    leg_torch()
    leg_kernel()
    same = torch.equal(pool_k, pool_t)
    ms, per = ab({"a_torch_pack_plane": leg_torch, "b_pool_from_atlas": leg_kernel})
    pool_bytes = lay.n_slots * 256
    res["open"] = {"tile": [th, tw], "planes": [Hs, Ws], "slots": lay.n_slots, "pool_bytes": pool_bytes, "blocks_static": lay.n_static,
                   "blocks_dynamic": lay.n_dynamic, "static_atlas": list(static.shape[:2]), "dynamic_atlas": list(dyn_all.shape[1:3]),
                   "pools_equal": same}
    for k, v in ms.items():
        med = statistics.median(v)
        res["open"][k] = {"ms_median": med, "ms_min": min(v), "ms_max": max(v), "GB_s_pool_written": pool_bytes / med / 1e6}
        print(f"open {k:20s} {med:9.3f} ms per pool (min {min(v):.3f}, max {max(v):.3f} over {a.rounds} rounds of {per})  "
              f"{pool_bytes / med / 1e6:8.1f} GB/s of pool written ({pool_bytes / 1e6:.1f} MB)")
    ratio = statistics.median(ms["b_pool_from_atlas"]) / statistics.median(ms["a_torch_pack_plane"])
    res["open"]["kernel_over_torch"] = ratio
    print(f"open: pools equal {same}; kernel / torch route {ratio:.4f} -> {'ok' if ratio <= 1 else 'MISSED'} (condition: not slower than the torch route)")
    with tempfile.TemporaryDirectory() as tmp:            # PNG decode, reported separately: one dynamic atlas, one thread
        png = os.path.join(tmp, "0000.png")
        write_png(png, dyn_all[0].cpu().numpy())
        secs = []
        for _ in range(3):
            t0 = time.perf_counter()
            read_png(png)
            secs.append(time.perf_counter() - t0)
        res["open"]["png_decode"] = {"seconds_per_atlas_median": statistics.median(secs), "file_MB": os.path.getsize(png) / 1e6,
                                     "texel_MB": dyn_all[0].numel() / 1e6, "frames": T}
        print(f"open: read_png of one dynamic atlas ({dyn_all.shape[1]} x {dyn_all.shape[2]}, {os.path.getsize(png) / 1e6:.1f} MB file): "
              f"{statistics.median(secs) * 1e3:.1f} ms on one thread; x {T} frames = {statistics.median(secs) * T:.2f} s of decoding against "
              f"{statistics.median(ms['b_pool_from_atlas']):.3f} ms of scatter")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
