"""Row bands with per-plane source windows on the MI355X (vl3d_render_fwd_plane_rows / _bwd_plane_rows through dist.render_plane_band):
every band rendered from its per-plane local rows is the full render's rows bit for bit, its gradient is the uniform-window band path's on
every texel both hold, the summed bands give the full gradient, and a two-rank gloo dry run on the one GPU reproduces the N = 1 step."""
import os
import socket

import pytest
import torch

from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _homos(D, H, W, scale=2.0):
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    tar_e = tar_e.clone()
    tar_e[:3, 3] *= scale
    h = compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3),
                           make_depths(D, 1.0, 100.0).flip(0)[None])[0]
    return torch.tensor([[1.0, 0, 3.0], [0, 1.0, 3.0], [0, 0, 1.0]]) @ h


SCENE = dict(D=6, T=3, Hs=150, Ws=96, H=144, W=90)      # T = 3: a frame pair and a lone frame


def _maxabs(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_plane_bands_render_the_full_frame_bits_and_gradient(dev, dtype):
    from videoloop3d_amd.dist import plan_bands, plan_plane_bands, plane_band_local, render_band, render_plane_band
    from videoloop3d_amd.render import RenderSpec, render_planes
    D, T, Hs, Ws, H, W = (SCENE[k] for k in ("D", "T", "Hs", "Ws", "H", "W"))
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=3, device=dev, dtype=dtype)
    homos = _homos(D, H, W)
    hd = homos.to(dev)
    spec = RenderSpec.mpv()
    full_in = stack.clone().requires_grad_(True)
    full, full_a = render_planes(full_in, hd, H, W, spec)
    g = (synth.hash_uniform((T, H, W, 3), seed=9) - 0.5).to(dev)
    (g_full,) = torch.autograd.grad(full, full_in, g)
    scale = float(g_full.float().abs().max())
    from videoloop3d_amd import render as R_
    for world in (1, 3, 4, 8):
        g_acc = torch.zeros(g_full.shape, dtype=torch.float32, device=dev)
        for pb, ub in zip(plan_plane_bands(homos, H, W, Hs, world, spec), plan_bands(homos, H, W, Hs, world, spec)):
            local = plane_band_local(stack, pb).requires_grad_(True)
            rgb, alpha = render_plane_band(local, hd, pb, W, Hs, spec)
            assert torch.equal(rgb, full[:, pb.row0:pb.row0 + pb.rows]), (world, pb.rank)
            assert torch.equal(alpha, full_a[:, pb.row0:pb.row0 + pb.rows]), (world, pb.rank)
            gb = g[:, pb.row0:pb.row0 + pb.rows]
            (gl,) = torch.autograd.grad(rgb, local, gb)
            assert int(R_.LAST_BWD_SCRATCH[:1].view(torch.int32).item()) == 1      # the owner-computes path took the call
            ul = stack[:, :, ub.src0:ub.src1].contiguous().requires_grad_(True)
            urgb, _ = render_band(ul, hd, ub, W, Hs, spec)
            (gu,) = torch.autograd.grad(urgb, ul, gb)
            for d in range(D):
                n = pb.src1[d] - pb.src0[d]
                assert bool((gl[d, :, n:] == 0).all())      # padding rows stay zero
                mine, theirs = gl[d, :, :n], gu[d, :, pb.src0[d] - ub.src0:pb.src1[d] - ub.src0]
                assert torch.equal(mine, theirs), (world, pb.rank, d, _maxabs(mine, theirs))      # the same owner-computes sums
                g_acc[d, :, pb.src0[d]:pb.src1[d]] += mine.float()
        assert _maxabs(g_acc, g_full.float()) <= (1e-5 if dtype == torch.float32 else 4e-3 * max(1.0, scale)), world


def test_plane_rows_refuses_other_conventions(dev):
    from videoloop3d_amd.render import RenderSpec, render_plane_rows
    local = torch.zeros((2, 1, 4, 8, 4), device=dev)
    with pytest.raises(RuntimeError, match="MPV convention"):
        render_plane_rows(local, torch.eye(3).expand(2, 3, 3).to(dev), torch.zeros(2, dtype=torch.int32, device=dev), 4, 8, 8, RenderSpec())


@pytest.mark.parametrize("bad", ["rgb_act", "variant", "uv_noise_seed"])
def test_plane_rows_entry_points_refuse_what_they_do_not_build(dev, bad):
    """descriptors the Python guard lets through (affine / hardcut / post) but the kernels are not built for: the C ABI refuses them, forward
    and backward, before anything is launched"""
    import ctypes
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd.render import RenderSpec, _desc, render_plane_rows
    D, T, R, Hs, Ws, H, W = 2, 1, 6, 12, 8, 4, 8
    local = torch.zeros((D, T, R, Ws, 4), device=dev)
    homos = torch.eye(3).expand(D, 3, 3).contiguous().to(dev)
    table = torch.zeros(D, dtype=torch.int32, device=dev)
    spec = {"rgb_act": RenderSpec.mpv(rgb_act="relu"), "variant": RenderSpec.mpv(variant=3),
            "uv_noise_seed": RenderSpec(pixel_center=0.5, coord_mode="affine", border="hardcut", act_order="post", uv_noise_seed=7)}[bad]
    with pytest.raises(RuntimeError, match="per-plane row windows"):
        render_plane_rows(local, homos, table, H, W, Hs, spec)
    desc = _desc(local, H, W, spec, 0, 0)
    desc.Hs = Hs
    out = torch.empty((T, H, W, 3), device=dev)
    a = torch.empty((T, H, W), device=dev)
    g = torch.empty_like(local)
    rc = L.lib().vl3d_render_bwd_plane_rows(desc, L.ptr(local), L.ptr(table), R, L.ptr(homos), L.ptr(out), L.ptr(a), L.ptr(out), None,
                                            L.ptr(g), None, 0, L.stream_ptr(dev))
    assert rc == 1 and b"per-plane row windows" in ctypes.string_at(L.lib().vl3d_last_error())


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dry_run_worker(rank, world, port, out):
    """one sharded training step on the GPU with gloo collectives: band render from per-plane local rows, all-gather of the composited bands,
    band gradient, backward, per-plane halo exchange"""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from videoloop3d_amd.dist import all_gather_frame, exchange_plane_halo_grads, plan_plane_bands, plane_band_local, render_plane_band
        from videoloop3d_amd.render import RenderSpec
        dev = torch.device("cuda:0")
        D, T, Hs, Ws, H, W = (SCENE[k] for k in ("D", "T", "Hs", "Ws", "H", "W"))
        spec = RenderSpec.mpv()
        homos = _homos(D, H, W)
        pbands = plan_plane_bands(homos, H, W, Hs, world, spec)
        pb = pbands[rank]
        stack = synth.make_plane_stack(D, T, Hs, Ws, seed=3)
        local = plane_band_local(stack, pb).to(dev).requires_grad_(True)
        rgb, _ = render_plane_band(local, homos.to(dev), pb, W, Hs, spec)
        frame = all_gather_frame(rgb.detach().cpu(), pbands)
        g = synth.hash_uniform((T, H, W, 3), seed=9) - 0.5
        (gl,) = torch.autograd.grad(rgb, local, g[:, pb.row0:pb.row0 + pb.rows].to(dev))
        g_done = exchange_plane_halo_grads(gl.cpu(), pbands)
        out.put((rank, frame, g_done, pb))
    finally:
        dist.destroy_process_group()


def test_gloo_dry_run_two_ranks_on_one_gpu(dev):
    import torch.multiprocessing as mp
    from videoloop3d_amd.render import RenderSpec, render_planes
    D, T, Hs, Ws, H, W = (SCENE[k] for k in ("D", "T", "Hs", "Ws", "H", "W"))
    stack = synth.make_plane_stack(D, T, Hs, Ws, seed=3, device=dev).requires_grad_(True)
    full, _ = render_planes(stack, _homos(D, H, W).to(dev), H, W, RenderSpec.mpv())
    g = (synth.hash_uniform((T, H, W, 3), seed=9) - 0.5).to(dev)
    (g_full,) = torch.autograd.grad(full, stack, g)
    full, g_full = full.detach().cpu(), g_full.cpu()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dry_run_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=300) for _ in range(world)]       # a rank that fails or hangs ends the test here, nothing is retried
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    for rank, frame, g_done, pb in res:
        assert torch.equal(frame, full), rank
        for d in range(D):
            n = pb.src1[d] - pb.src0[d]
            assert _maxabs(g_done[d, :, :n], g_full[d, :, pb.src0[d]:pb.src1[d]]) <= 1e-5, (rank, d)
    # replicas of a shared row: identical bits on both holders
    (_, _, g0, p0), (_, _, g1, p1) = sorted(res, key=lambda x: x[0])
    for d in range(D):
        lo, hi = max(p0.src0[d], p1.src0[d]), min(p0.src1[d], p1.src1[d])
        if hi > lo:
            assert torch.equal(g0[d, :, lo - p0.src0[d]:hi - p0.src0[d]], g1[d, :, lo - p1.src0[d]:hi - p1.src0[d]])
