"""Row bands with per-plane source windows at the bench geometry (cfg3: D = 32, T = 50, 720p, synth.make_cameras, RenderSpec.mpv()).

  python profiles/plane_bands.py --plan             planner arithmetic (CPU): rows held, shared rows and halo bytes of both planners, N = 2 / 4 / 8
  python profiles/plane_bands.py --kernels          one MI355X: fwd / bwd time of band 3 of 8 from its union rows (dist.render_band) and from its
                                                    per-plane rows (dist.render_plane_band), the two interleaved, --reps each
  python profiles/plane_bands.py --world N          one sharded training step with gloo on ONE MI355X (N spawned ranks): render band, all-gather,
                                                    band gradient, backward, per-plane halo exchange; prints the frame checksum, the gradient sums and
                                                    the halo bytes of both planners (a dry run of the N > 1 path, not a timing)
"""
import argparse
import json
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

D, T, H, W = 32, 50, 720, 1280


def geometry():
    from videoloop3d_amd import synth
    from videoloop3d_amd.render import RenderSpec
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    homos = compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3),
                               make_depths(D, 1.0, 100.0).flip(0)[None])[0]
    return homos, RenderSpec.mpv()


def plan_table():
    from videoloop3d_amd.dist import halo_overlaps, plan_bands, plan_plane_bands, plane_halo_overlaps
    homos, spec = geometry()
    per_row = T * W * 16
    out = []
    for n in (2, 4, 8):
        ub, pb = plan_bands(homos, H, W, H, n, spec), plan_plane_bands(homos, H, W, H, n, spec)
        need = [sum(b - a for a, b in zip(p.src0, p.src1)) / D for p in pb]
        links = []
        for r in range(n - 1):
            u = dict((p, hi - lo) for p, lo, hi in halo_overlaps(ub, r))[r + 1]
            m = dict((p, (rows, nb)) for p, rows, nb in plane_halo_overlaps(pb, r, T=T, Ws=W))[r + 1]
            links.append({"link": [r, r + 1], "union_rows_per_plane": u, "plane_rows_per_plane": sum(h - l for l, h in m[0]) / D,
                          "union_bytes": u * D * per_row, "plane_bytes": m[1]})
        out.append({"N": n, "union_rows_held_max": max(b.src1 - b.src0 for b in ub), "plane_R_max": max(p.R for p in pb),
                    "plane_rows_needed_avg": sum(need) / n, "plane_rows_needed_max": max(need),
                    "resident_stack_bytes_max": {"union": max(b.src1 - b.src0 for b in ub) * D * per_row, "plane": max(p.R for p in pb) * D * per_row},
                    "links": links})
    return out


def kernels(reps):
    """the two band paths at the same band, interleaved rep by rep (a drift of the clock or of the neighbours' load hits both alike)"""
    import __graft_entry__ as ge
    ge.build()
    from videoloop3d_amd import synth
    from videoloop3d_amd.dist import plan_bands, plan_plane_bands, plane_row0_table, render_band, render_plane_band
    homos, spec = geometry()
    dev = torch.device("cuda:0")
    hd = homos.to(dev)
    ub, pb = plan_bands(homos, H, W, H, 8, spec)[3], plan_plane_bands(homos, H, W, H, 8, spec)[3]
    g = (synth.hash_uniform((T, ub.rows, W, 3), seed=5, device=dev) - 0.5)
    tab = plane_row0_table(pb, dev)
    stacks = {"render_band": synth.make_plane_stack(D, T, ub.src1 - ub.src0, W, seed=2, device=dev).requires_grad_(True),
              "render_plane_band": synth.make_plane_stack(D, T, pb.R, W, seed=2, device=dev).requires_grad_(True)}
    calls = {"render_band": lambda st: render_band(st, hd, ub, W, H, spec), "render_plane_band": lambda st: render_plane_band(st, hd, pb, W, H, spec, tab)}
    times = {k: ([], []) for k in calls}
    for i in range(reps + 3):
        for name, call in calls.items():
            st = stacks[name]
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            rgb, _ = call(st)
            e1.record()
            torch.autograd.grad(rgb, st, g)
            e2.record()
            torch.cuda.synchronize()
            if i >= 3:
                times[name][0].append(e0.elapsed_time(e1))
                times[name][1].append(e1.elapsed_time(e2))
    med = lambda v: sorted(v)[len(v) // 2]
    res = {name: {"stack_rows": stacks[name].shape[2], "fwd_ms_median": med(fw), "bwd_ms_median": med(bw), "fwd_ms_mean": sum(fw) / len(fw),
                  "bwd_ms_mean": sum(bw) / len(bw), "fwd_ms_min": min(fw), "bwd_ms_min": min(bw)} for name, (fw, bw) in times.items()}
    return {"band": "3 of 8", "rows": ub.rows, "reps": reps, "interleaved": True, **res}


def _bits_sum(t):
    return int(t.contiguous().view(torch.int32).to(torch.int64).sum().item())


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from videoloop3d_amd import synth
        from videoloop3d_amd.dist import all_gather_frame, exchange_plane_halo_grads, halo_overlaps, plan_bands, plan_plane_bands, \
            plane_halo_overlaps, render_plane_band
        homos, spec = geometry()
        dev = torch.device("cuda:0")
        pbands = plan_plane_bands(homos, H, W, H, world, spec)
        pb = pbands[rank]
        # the bench's stack values (synth.make_plane_stack(D, T, H, W, seed=2)), per plane rows [src0_d, src1_d) only, zero padding
        local = torch.zeros((D, T, pb.R, W, 4), dtype=torch.float32, device=dev)
        per_plane = T * H * W * 4
        for d in range(D):
            n = pb.src1[d] - pb.src0[d]
            for t in range(T):
                sl = synth.hash_uniform((n, W, 4), 2, device=dev, offset=d * per_plane + (t * H + pb.src0[d]) * W * 4) * 4.0 - 2.0
                sl[..., 3] -= 2.0
                local[d, t, :n] = sl
        local.requires_grad_(True)
        g = torch.stack([synth.hash_uniform((pb.rows, W, 3), 5, device=dev, offset=(t * H + pb.row0) * W * 3) for t in range(T)]) - 0.5
        rgb, _ = render_plane_band(local, homos.to(dev), pb, W, H, spec)
        frame = all_gather_frame(rgb.detach().cpu(), pbands)
        (gl,) = torch.autograd.grad(rgb, local, g)
        gl = exchange_plane_halo_grads(gl.cpu(), pbands)
        # gradient sums over a PARTITION of every plane's rows (rank r: its rows up to the next rank's first row of that plane)
        s, sa = 0.0, 0.0
        for d in range(D):
            hi = pbands[rank + 1].src0[d] if rank + 1 < world else pb.src1[d]
            part = gl[d, :, :max(0, min(hi, pb.src1[d]) - pb.src0[d])].double()
            s, sa = s + float(part.sum()), sa + float(part.abs().sum())
        sums = torch.tensor([s, sa], dtype=torch.float64)
        dist.all_reduce(sums)
        ub = plan_bands(homos, H, W, H, world, spec)
        union = {p: (hi - lo) * D * T * W * 16 for p, lo, hi in halo_overlaps(ub, rank)}
        plane = {p: nb for p, _, nb in plane_halo_overlaps(pbands, rank, T=T, Ws=W)}
        if rank == 0:
            out.put({"N": world, "frame_checksum": _bits_sum(frame), "grad_sums": sums.tolist(),
                     "halo_bytes_rank0": {"union": union, "plane": plane}, "R": pb.R})
    finally:
        dist.destroy_process_group()


def dry_run(world):
    import torch.multiprocessing as mp
    import __graft_entry__ as ge
    ge.build()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = q.get(timeout=900)
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--world", type=int, default=0)
    a = ap.parse_args()
    if a.plan:
        print(json.dumps(plan_table(), indent=1))
    if a.kernels:
        print(json.dumps(kernels(a.reps)))
    if a.world:
        print(json.dumps(dry_run(a.world)))
