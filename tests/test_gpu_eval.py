"""On-device evaluation (videoloop3d_amd.evaluations; scripts/script_evaluate_ours.py) on the MI355X: the per-view image statistics of
vl3d_eval_view against the reference's own metric code (golden G20, tests/golden/make_golden_r07.py) and against an fp64 torch restatement
of skimage's SSIM / PSNR and the script's dyn written here; the driver end to end on a synthetic MPMeshVid."""
import hashlib
import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as torchf

from videoloop3d_amd import evaluations as E
from videoloop3d_amd import render_video as RV
from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as ge
    ge.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ---- fp64 restatement (skimage structural_similarity / peak_signal_noise_ratio as evaluations/metrics.py calls them) -----------------------
def _reflect_index(n, r):
    """scipy.ndimage mode 'reflect' (half-sample symmetric) indices of positions -r .. n-1+r."""
    i = torch.arange(-r, n + r)
    i = torch.where(i < 0, -i - 1, i)
    return torch.where(i >= n, 2 * n - i - 1, i)


def _box7(x):
    """uniform_filter(size=7, mode='reflect') over the last two axes of x [N,h,w] (fp64)."""
    h, w = x.shape[-2:]
    xp = x[:, _reflect_index(h, 3).to(x.device)][:, :, _reflect_index(w, 3).to(x.device)]
    return torchf.avg_pool2d(xp[:, None], 7, stride=1)[:, 0]


def restated_metrics(gt, pred, mask=None):
    """script_evaluate_ours.py:156-178 in fp64 torch: (psnr, ssim, dyn)."""
    gt, pred = gt.double(), pred.double()
    Fm, h, w = min(len(gt), len(pred)), gt.shape[1], gt.shape[2]
    m = torch.ones((h, w), dtype=torch.float64, device=gt.device) if mask is None else torch.as_tensor(mask).double().to(gt.device)
    a = (gt[:Fm] / 255 * 2 - 1) * m[None, :, :, None]
    b = (pred[:Fm] / 255 * 2 - 1) * m[None, :, :, None]
    psnr, ssim = [], []
    for f in range(Fm):
        mse = ((a[f] - b[f]) ** 2).mean()
        rng = 2.0 if float(a[f].min()) < 0 else 1.0
        psnr.append(10 * math.log10(rng ** 2 / float(mse)) - 10 * math.log10(h * w / float(m.sum())) if float(mse) > 0 else math.inf)
        x, y = a[f].permute(2, 0, 1), b[f].permute(2, 0, 1)
        ux, uy = _box7(x), _box7(y)
        vx, vy, vxy = 49 / 48 * (_box7(x * x) - ux * ux), 49 / 48 * (_box7(y * y) - uy * uy), 49 / 48 * (_box7(x * y) - ux * uy)
        C1, C2 = (0.01 * 2) ** 2, (0.03 * 2) ** 2
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        ssim.append(float((S * m[None]).sum() / m.sum() / 3))
    dyn = float(((gt.std(0, unbiased=False) - pred.std(0, unbiased=False)) ** 2).mean())
    return float(np.mean(psnr)), float(np.mean(ssim)), dyn


def _close(got, want, psnr_tol=1e-6, ssim_tol=1e-7, dyn_rel=1e-9):
    (p, s, d), (p0, s0, d0) = got, want
    assert (p == p0) if math.isinf(p0) else abs(p - p0) <= psnr_tol, (p, p0)
    assert abs(s - s0) <= ssim_tol, (s, s0)
    assert abs(d - d0) <= dyn_rel * max(abs(d0), 1e-300) or d == d0, (d, d0)


# ---- G20: the reference's own metric code ------------------------------------------------------------------------------------------------
def _g20_inputs(g, v):
    F, T, H, W = (int(x) for x in g["shape"])
    gs, ps, pns, lo = (int(x) for x in g["views"][v])
    gt = synth.eval_clip(F, H, W, gs, lo=lo)
    pred = synth.eval_clip(T, H, W, ps, noise_seed=pns, lo=lo)
    mask = g[f"v{v}_mask"]
    h = hashlib.sha256()
    for a in (gt.numpy(), pred.numpy(), mask):
        h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == str(g[f"v{v}_sha256"]), "the G20 input recipe changed"
    return gt, pred, mask


@pytest.mark.parametrize("v", [0, 1])
def test_g20_view_metrics_match_the_reference(dev, golden, v):
    g = golden("g20_eval.npz")
    gt, pred, mask = _g20_inputs(g, v)
    c = int(g["crop"])
    gtd, predd = gt.to(dev), pred.to(dev)
    lm = mask.astype(np.float32)
    gtc, predc, mc = gtd[:, c:-c, c:-c], predd[:, c:-c, c:-c], lm[c:-c, c:-c]      # crop views, read in place
    psnr, ssim, dyn = E.view_image_metrics(gtc, predc, mc)
    assert abs(psnr - float(g[f"v{v}_psnr"])) <= 1e-6, (psnr, float(g[f"v{v}_psnr"]))
    assert abs(ssim - float(g[f"v{v}_ssim"])) <= 1e-7, (ssim, float(g[f"v{v}_ssim"]))
    assert abs(dyn - float(g[f"v{v}_dyn"])) <= 1e-9 * float(g[f"v{v}_dyn"]), (dyn, float(g[f"v{v}_dyn"]))
    assert E.static_metrics(gtc, predc, mc) == (psnr, ssim) and E.dynamic_error(gtc, predc) == dyn
    if v == 1:      # gt >= 128 inside the mask: skimage's data_range 1 (a different PSNR than with 2)
        assert int(gt[:, c:-c, c:-c].min()) >= 128
    # the compute_img_metric drop-in, called as the script calls the reference (:158-162)
    Fm = min(len(gtc), len(predc))
    g01, p01 = torch.tensor(gt[:Fm, c:-c, c:-c].numpy() / 255), torch.tensor(pred[:Fm, c:-c, c:-c].numpy() / 255)
    m1 = torch.tensor(mc[None])
    assert abs(E.compute_img_metric(g01, p01, "psnr", m1) - float(g[f"v{v}_psnr"])) <= 1e-6
    assert abs(E.compute_img_metric(g01, p01, "ssim", m1) - float(g[f"v{v}_ssim"])) <= 1e-7
    assert abs(E.compute_img_metric(g01, p01, "mse", m1[..., None]) - float(g[f"v{v}_mse"])) <= 1e-12
    # NN metrics at the script's configurations (G10 tolerance)
    gf, pf = gtc.permute(3, 0, 1, 2)[None].float(), predc.permute(3, 0, 1, 2)[None].float()
    comp, coh, loop = E.nn_metrics(gf, pf)
    for name, got in (("nnf", comp), ("nnb", coh), ("loop", loop)):
        want = g[f"v{v}_{name}"]
        assert len(got) == 3
        for a, b in zip(got, want):
            assert abs(a - float(b)) <= 2e-6 * max(1.0, abs(float(b))), (name, got, want)


def test_compute_nnerr_on_0_255_clips(dev, golden):
    """compute_nnerr on the script's 0..255 value range: G10's clips times 255 give G10's values times 255 (the NN search itself is
    scale-free; the default kernel's f16 norm pieces cannot hold 0..255 pixels, so the search runs on a power-of-two-scaled copy)."""
    g = golden("g10_nnerr.npz")
    x, y = torch.tensor(g["x"]).to(dev), torch.tensor(g["y"]).to(dev)
    for (ps, s, pt, st, mb) in [(5, 2, 3, 1, 13), (7, 2, 3, 2, 65), (3, 1, 3, 1, 9), (11, 4, 3, 1, 19)]:
        want = 255 * float(g[f"ps{ps}_s{s}_pt{pt}_st{st}_mb{mb}"])
        got = E.compute_nnerr(x * 255, y * 255, ps, s, pt, st, mb)
        assert abs(got - want) <= 2e-6 * want, (ps, s, pt, st, mb, got, want)
        assert E.compute_nnerr(x, y, ps, s, pt, st, mb) == E.compute_nnerr(x, y, ps, s, pt, st, mb)


# ---- the fp64 restatement ----------------------------------------------------------------------------------------------------------------
def _rand_u8(shape, seed, dev):
    return (synth.hash_uniform(shape, seed) * 256).clamp(max=255).to(torch.uint8).to(dev)


@pytest.mark.parametrize("F,T,h,w", [(5, 4, 9, 11), (7, 9, 47, 61), (60, 57, 280, 560)])
@pytest.mark.parametrize("masked", [False, True])
def test_view_metrics_match_the_fp64_restatement(dev, F, T, h, w, masked):
    gt = _rand_u8((F, h + 3, w + 5, 3), 1 + h, dev)[:, 2:2 + h, 1:1 + w]          # a crop view
    pred = (gt[:T].int() if T <= F else torch.cat([gt, gt[:T - F]]).int())
    pred = (pred + (_rand_u8((T, h, w, 3), 2 + w, dev).int() // 8 - 16)).clamp(0, 255).to(torch.uint8)
    mask = None
    if masked:
        mask = (synth.hash_uniform((h, w), 3) < 0.7).float()
        mask[0, :] = 1
        mask[:, -1] = 1
    got = E.view_image_metrics(gt, pred, mask)
    want = restated_metrics(gt, pred, mask)
    _close(got, want)
    assert 0 < got[1] < 1 and got[2] > 0
    again = E.view_image_metrics(gt, pred, mask)
    assert again == got                                            # bit for bit (fixed-order reductions)


def test_identical_videos_and_refusals(dev):
    gt = _rand_u8((6, 30, 40, 3), 9, dev)
    mask = (synth.hash_uniform((30, 40), 4) < 0.5).float()
    psnr, ssim, dyn = E.view_image_metrics(gt, gt.clone(), mask)
    assert psnr == math.inf and ssim == 1.0 and dyn == 0.0
    psnr, ssim, dyn = E.view_image_metrics(gt, gt.clone())
    assert psnr == math.inf and ssim == 1.0 and dyn == 0.0
    with pytest.raises(ValueError):
        E.view_image_metrics(gt[:, :6], gt[:, :6])
    with pytest.raises(ValueError):
        E.view_image_metrics(gt[:, :, :6], gt[:, :, :6])
    with pytest.raises(ValueError):
        E.view_image_metrics(gt, gt, torch.zeros(30, 40))
    with pytest.raises(ValueError):
        E.compute_img_metric(gt.cpu().double() / 255, gt.cpu().double() / 255 + 1e-3, "psnr", torch.ones(1, 30, 40))


def test_library_refuses_bad_descriptors(dev):
    """The C ABI's own checks (no device access happens on these)."""
    from videoloop3d_amd import _lib as L
    gt = torch.zeros((2, 10, 10, 3), dtype=torch.uint8, device=dev)
    out = torch.zeros(64, dtype=torch.float64, device=dev)

    def call(**kw):
        d = dict(F=2, T=2, row0=0, col0=0, h=10, w=10, gt_sf=300, gt_sr=30, pred_sf=300, pred_sr=30)
        d.update(kw)
        desc = L.EvalDesc(**d)
        return L.lib().vl3d_eval_view(desc, L.ptr(gt), L.ptr(gt), None, 0, L.ptr(out), L.ptr(out), L.ptr(out), L.ptr(out), L.ptr(out),
                                      L.stream_ptr(dev))
    assert call(h=6) == 1 and call(w=6) == 1 and call(F=0) == 1 and call(T=-1) == 1 and call(gt_sr=20) == 1 and call(pred_sf=100) == 1
    desc = L.EvalDesc(F=2, T=2, row0=0, col0=0, h=10, w=10, gt_sf=300, gt_sr=30, pred_sf=300, pred_sr=30)
    m = torch.zeros((10, 10), dtype=torch.uint8, device=dev)
    assert L.lib().vl3d_eval_view(desc, L.ptr(gt), L.ptr(gt), L.ptr(m), 0, L.ptr(out), L.ptr(out), L.ptr(out), L.ptr(out), L.ptr(out),
                                  L.stream_ptr(dev)) == 1           # an all-zero mask
    assert L.lib().vl3d_eval_view(desc, L.ptr(gt), None, None, 0, L.ptr(out), L.ptr(out), L.ptr(out), L.ptr(out), L.ptr(out),
                                  L.stream_ptr(dev)) == 1           # a null clip
    assert L.lib().vl3d_eval_scratch_bytes(L.EvalDesc(F=2, T=2, row0=0, col0=0, h=5, w=10, gt_sf=300, gt_sr=30, pred_sf=300, pred_sr=30)) == -1


# ---- the driver end to end ---------------------------------------------------------------------------------------------------------------
def _model_and_views(dev, golden, T=8, H=96, W=128, static=False):
    from videoloop3d_amd.MPV import MPMeshVid
    g = golden("g18_render_poses.npz")
    poses, intrins, bds, _, _ = RV.load_llff_poses(g["a_poses_bounds"], factor=2, recenter=True, bd_factor=(0.9, 1.1), render_frm=12)
    sc = np.diag([W / (2 * intrins[0, 0, 2]), H / (2 * intrins[0, 1, 2]), 1.0]).astype(np.float32)
    intrins = sc @ intrins
    ext, K, near, far = RV.reference_camera(poses, intrins, bds)
    args = types.SimpleNamespace(mpv_frm_num=T, mpv_isloop=True, mpi_h_scale=1.1, mpi_w_scale=1.1, mpi_d=6, atlas_grid_h=2, init_std=0.5,
                                 rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color="", scale_invariant=True,
                                 fp16=False, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1, sparsity_loss_weight=0.0,
                                 rgb_smooth_loss_weight=0.0, a_smooth_loss_weight=0.0, density_loss_weight=0.0, d_smooth_loss_weight=0.0,
                                 optimizer="adam", lrate=0.1, lrate_decay=30)
    model = MPMeshVid(args, H, W, ext, K.astype(np.float64), near, far).to(dev)
    with torch.no_grad():
        model.stack.copy_(synth.make_plane_stack(*model.stack.shape[:4], seed=5, device=dev) * 0.8)
        half = model.stack.shape[3] if static else model.stack.shape[3] // 2      # the left half of every plane static in time (all of it)
        model.stack[:, :, :, :half] = model.stack[:, :1, :, :half].clone()
    views = [0, 2]
    return model, RV.pose2extrin_np(poses[views]), intrins[views], H, W


@pytest.mark.parametrize("wrap", [False, True])
def test_evaluate_views_end_to_end(dev, golden, tmp_path, wrap):
    model, ext, K, H, W = _model_and_views(dev, golden)
    nerf = torch.nn.DataParallel(model, [0]) if wrap else model
    T = model.frm_num
    own = [RV.render_frames(nerf, H, W, np.repeat(ext[v:v + 1], T, 0), np.repeat(K[v:v + 1], T, 0), np.arange(T)) for v in range(2)]
    for v in range(2):
        assert float(own[v].float().std()) > 1.0
        assert 0 < float(E.loop_static_mask(own[v]).mean()) < 1
    # gt = the model's own renders: no completeness / coherence error, SSIM 1, no dyn error.  (Loop quality compares the seam clip -- the
    # last pt-1 frames followed by the first pt-1, :217-219 -- with gt: every window of it straddles the cut, which one pass of the loop does
    # not hold, so it is > 0 unless the loop is static in time; the static model below has every value 0.)
    res = E.evaluate_views(nerf, own, ext, K, crop=20)
    assert len(res) == 2
    for r in res:
        for k in ("nnf", "nnb") + tuple(f"{t}_{E._config_tag(c)}" for t in ("nnf", "nnb") for c in E.EVAL_PATCH_CONFIGS):
            assert r[k] == 0.0, (k, r[k])
        assert r["loop"] > 0
        assert r["ssim"] == 1.0 and r["dyn"] == 0.0 and r["psnr"] == math.inf and r["lpips"] == 0.0 and r["lpips_sw"] == 0.0
    smodel, _, _, _, _ = _model_and_views(dev, golden, static=True)
    snerf = torch.nn.DataParallel(smodel, [0]) if wrap else smodel
    sown = [RV.render_frames(snerf, H, W, np.repeat(ext[v:v + 1], T, 0), np.repeat(K[v:v + 1], T, 0), np.arange(T)) for v in range(2)]
    for r in E.evaluate_views(snerf, sown, ext, K, crop=20):
        for k in ("nnf", "nnb", "loop") + tuple(f"{t}_{E._config_tag(c)}" for t in ("nnf", "nnb", "loop") for c in E.EVAL_PATCH_CONFIGS):
            assert r[k] == 0.0, (k, r[k])
        assert r["ssim"] == 1.0 and r["dyn"] == 0.0 and r["psnr"] == math.inf
    # gt = perturbed renders (one more frame than the loop): the per-view numbers are the metric functions on render_frames' output
    gts = []
    for v in range(2):
        noise = (synth.hash_uniform((T + 1, H, W, 3), 40 + v, device=dev) * 11).long() - 5      # (below the loop mask's 15 levels)
        gts.append((torch.cat([own[v], own[v][:1]]).long() + noise).clamp(0, 255).to(torch.uint8).cpu().numpy())
    res = E.evaluate_views(nerf, gts, ext, K, crop=20)
    for v, r in enumerate(res):
        gt = torch.as_tensor(gts[v]).to(dev)
        m = E.loop_static_mask(gt)
        c = slice(20, -20)
        psnr, ssim, dyn = E.view_image_metrics(gt[:, c, c], own[v][:, c, c], m[c, c])
        assert (r["psnr"], r["ssim"], r["dyn"]) == (psnr, ssim, dyn)
        comp, coh, loop = E.nn_metrics(gt[:, c, c].permute(3, 0, 1, 2)[None].float(), own[v][:, c, c].permute(3, 0, 1, 2)[None].float())
        assert [r[f"nnf_{E._config_tag(cf)}"] for cf in E.EVAL_PATCH_CONFIGS] == comp
        assert [r[f"nnb_{E._config_tag(cf)}"] for cf in E.EVAL_PATCH_CONFIGS] == coh
        assert [r[f"loop_{E._config_tag(cf)}"] for cf in E.EVAL_PATCH_CONFIGS] == loop
        assert r["nnf"] == sum(comp) / 3 and r["nnb"] == sum(coh) / 3 and r["loop"] == sum(loop) / 3
        assert r["nnf"] > 0 and 0 < r["ssim"] < 1 and r["dyn"] > 0
    # metrics.txt
    path = tmp_path / "eval_metrics.txt"
    E.write_metrics_txt(str(path), "scene", res)
    lines = path.read_text().splitlines()
    assert lines[0] == ("name, nnf, nnb, dyn, lpips, lpips_sw, loop, psnr, ssim, nnf_p5s2pt7st1, nnf_p11s4pt5st1, nnf_p17s6pt3st1, "
                        "nnb_p5s2pt7st1, nnb_p11s4pt5st1, nnb_p17s6pt3st1, loop_p5s2pt7st1, loop_p11s4pt5st1, loop_p17s6pt3st1")
    assert len(lines) == 4
    rows = [ln.split(", ") for ln in lines[1:]]
    assert all(len(r) == 18 for r in rows) and [r[0] for r in rows] == ["scene_view0", "scene_view1", "scene"]
    vals = np.array([[float(x) for x in r[1:]] for r in rows])
    np.testing.assert_allclose(vals[2], vals[:2].mean(0), rtol=1e-12, atol=0)


def test_evaluate_from_poses_bounds(dev, golden, tmp_path):
    """evaluate(): LLFF poses -> test-view selection -> evaluate_views -> eval_metrics.txt (the whole of the script but the video files)."""
    from videoloop3d_amd.MPV import MPMeshVid
    g = golden("g18_render_poses.npz")
    pb = np.array(g["a_poses_bounds"])
    pb[:, 4], pb[:, 9], pb[:, 14] = 128 * 2, 160 * 2, pb[:, 14] * (160 * 2) / pb[:, 9]      # (H, W, f): 128 x 160 frames at factor 2
    args = types.SimpleNamespace(mpv_frm_num=8, mpv_isloop=True, mpi_h_scale=1.1, mpi_w_scale=1.1, mpi_d=4, atlas_grid_h=2, init_std=0.5,
                                 rgb_mlp_type="direct", rgb_activate="sigmoid", alpha_activate="sigmoid", bg_color="", scale_invariant=True,
                                 fp16=False, swd_patch_size=3, swd_patcht_size=3, swd_stride=2, swd_stridet=1, sparsity_loss_weight=0.0,
                                 rgb_smooth_loss_weight=0.0, a_smooth_loss_weight=0.0, density_loss_weight=0.0, d_smooth_loss_weight=0.0,
                                 optimizer="adam", lrate=0.1, lrate_decay=30, factor=2, near_factor=0.9, far_factor=1.1, test_view_idx="1,0")
    poses, intrins, bds, _, _ = RV.load_llff_poses(pb, factor=2, recenter=True, bd_factor=(0.9, 1.1))
    ext, K, near, far = RV.reference_camera(poses, intrins, bds)
    H, W = int(round(2 * intrins[0, 1, 2])), int(round(2 * intrins[0, 0, 2]))
    assert (H, W) == (128, 160)
    model = MPMeshVid(args, H, W, ext, K.astype(np.float64), near, far).to(dev)
    videos = [synth.eval_clip(9, H, W, 60 + v, noise=5).numpy() for v in range(len(pb))]      # (a static region for the loop mask)
    res = E.evaluate(model, args, pb, videos, dataname="synthetic", out_dir=str(tmp_path))
    assert len(res) == 2
    want = E.evaluate_views(model, [videos[1], videos[0]], RV.pose2extrin_np(poses[[1, 0]]), intrins[[1, 0]])
    assert res == want
    lines = (tmp_path / "eval_metrics.txt").read_text().splitlines()
    assert [ln.split(", ")[0] for ln in lines[1:]] == ["synthetic_view0", "synthetic_view1", "synthetic"]
