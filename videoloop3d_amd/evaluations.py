"""Drop-in for the reference's evaluations/NNMSE.py on the HIP patch-NN kernels.

`compute_nnerr(src, tar, ...)` = completeness / coherence / loop-quality NN error of scripts/script_evaluate_ours.py:201-246:
plain per-location temporal patch NN (alpha None), then mean |NN patch of tar - patch of src|, averaged per macro block
and then over macro blocks (the reference's macro-block loop changes the result here -- it is a mean of block means --
so the block structure of evaluations/NNMSE.py:31-58 is reproduced on the per-location errors)."""
import math

import numpy as np
import torch

from . import _lib as L
from .utils_vid import find_nn_indices, fit_patch


def compute_nnerr(src, tar, patch_size=7, stride=2, patcht_size=7, stridet=2, macro_block=65):
    """evaluations/NNMSE.py:7-58.  src, tar: [1,3,f,h,w] on the MI355X (any value range: [0, 1] renders or the script's 0..255 clips)
    -> python float."""
    t, h, w = src.shape[-3:]

    macro_block = fit_patch(macro_block, "macro_block", patch_size, stride)
    h = fit_patch(h, "patch_height", patch_size, stride)
    w = fit_patch(w, "patch_width", patch_size, stride)
    t = fit_patch(t, "frame_num", patcht_size, stridet)
    src = src[..., :t, :h, :w]
    tar = tar[..., :h, :w]
    with torch.no_grad():
        amax = float(torch.maximum(src.abs().max(), tar.abs().max()))
        if amax > 1:
            # the default NN kernel (split-f16 matrix cores) carries each pixel's squared norm as an f16 pair, which overflows beyond
            # ~147 per channel -- the evaluation script passes 0..255 clips (script_evaluate_ours.py:212-213): the search runs on the clips
            # scaled into [-1, 1] by a power of two (exact: the distances scale by one factor, the argmin is theirs), the errors below
            # on the clips as given
            src, tar = src.float().contiguous(), tar.float().contiguous()
            k = 2.0 ** -math.ceil(math.log2(amax))
            nn, desc, _, _ = find_nn_indices(src * k, tar * k, patch_size, patcht_size, stride, stridet, None)
            xv, yv = src[0], tar[0]          # the layout of the scaled copies: desc's strides hold
        else:
            nn, desc, xv, yv = find_nn_indices(src, tar, patch_size, patcht_size, stride, stridet, None)
        h_o, w_o, n1 = nn.shape
        err = torch.empty((h_o, w_o), dtype=torch.float32, device=xv.device)
        with torch.cuda.device(xv.device):
            L.check(L.lib().vl3d_patch_l1(desc, L.ptr(xv), L.ptr(yv), L.ptr(nn), L.ptr(err), L.stream_ptr(xv.device)),
                    "vl3d_patch_l1")
        per_loc = err.double() / (n1 * 3 * patcht_size * patch_size * patch_size)     # mean |.| of one location's patches
        macro_stride = macro_block - patch_size + stride
        lpb = macro_stride // stride                                                   # patch locations per macro block and axis
        errs = []
        for hs in np.arange(0, h - macro_block + macro_stride, macro_stride):
            for ws in np.arange(0, w - macro_block + macro_stride, macro_stride):
                b0, c0 = hs // stride, ws // stride
                errs.append(per_loc[b0:b0 + lpb, c0:c0 + lpb].mean())
        return float(torch.stack(errs).mean().item())


# ---- scripts/script_evaluate_ours.py on the device -------------------------------------------------------------------------------
# The script's patch configurations (:201-204) at compute_nnerr's default macro block (65): (patch_size, stride, patcht_size, stridet).
EVAL_PATCH_CONFIGS = ((5, 2, 7, 1), (11, 4, 5, 1), (17, 6, 3, 1))
EVAL_MACRO_BLOCK = 65


def _config_tag(cfg):
    p, s, pt, st = cfg
    return f"p{p}s{s}pt{pt}st{st}"


def metric_names():
    """The header of metrics.txt (script_evaluate_ours.py:249-252)."""
    tags = [_config_tag(c) for c in EVAL_PATCH_CONFIGS]
    return (["name", "nnf", "nnb", "dyn", "lpips", "lpips_sw", "loop", "psnr", "ssim"] + [f"nnf_{t}" for t in tags]
            + [f"nnb_{t}" for t in tags] + [f"loop_{t}" for t in tags])


def _clip_u8(x, name):
    """uint8 [F,h,w,3] device tensor (a crop view is read in place: pixel stride 3, channel stride 1)."""
    x = torch.as_tensor(x)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError(f"{name} must be uint8 [F,H,W,3], got {x.dtype} {tuple(x.shape)}")
    L.check_cuda(x)
    if x.stride(3) != 1 or x.stride(2) != 3:
        x = x.contiguous()
    return x


def _view_stats(gt_u8, pred_u8, mask):
    """vl3d_eval_view on one view -> (sse int64 [Fm], ssim_sum float64 [Fm], gt_min int32 [Fm], dyn_sum, mask ones, h, w) on the host."""
    gt, pred = _clip_u8(gt_u8, "gt"), _clip_u8(pred_u8, "pred")
    if gt.shape[1:] != pred.shape[1:]:
        raise ValueError(f"gt and pred frames differ in size: {tuple(gt.shape[1:])} vs {tuple(pred.shape[1:])}")
    if gt.device != pred.device:
        raise ValueError("gt and pred must be on the same device")
    F, h, w, _ = gt.shape
    T = pred.shape[0]
    if h < 7 or w < 7:
        raise ValueError(f"the evaluated frame is {h} x {w}: SSIM needs at least 7 x 7 (skimage's win_size)")
    if F < 1 or T < 1:
        raise ValueError("empty clip")
    dev = gt.device
    m_dev, ones = None, h * w
    if mask is not None:
        m = torch.as_tensor(mask)
        if m.numel() != h * w:
            raise ValueError(f"mask must be [h,w] = [{h},{w}] (or [1,h,w], [1,h,w,1]), got {tuple(m.shape)}")
        m = m.reshape(h, w).to(dev)
        if not bool(((m == 0) | (m == 1)).all()):
            raise ValueError("mask must hold only 0 and 1")
        m_dev = (m != 0).to(torch.uint8).contiguous()
        ones = int(m_dev.sum(dtype=torch.int64))
        if ones == 0:
            raise ValueError("the mask is all zero: no static region to score (the reference yields nan / -inf here)")
    desc = L.EvalDesc(F=F, T=T, row0=0, col0=0, h=h, w=w, gt_sf=gt.stride(0), gt_sr=gt.stride(1), pred_sf=pred.stride(0),
                      pred_sr=pred.stride(1))
    Fm = min(F, T)
    sse = torch.empty(Fm, dtype=torch.int64, device=dev)
    ssim_sum = torch.empty(Fm, dtype=torch.float64, device=dev)
    gt_min = torch.empty(Fm, dtype=torch.int32, device=dev)
    dyn_sum = torch.empty(1, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        scratch = torch.empty(max(0, int(L.lib().vl3d_eval_scratch_bytes(desc))), dtype=torch.uint8, device=dev)
        L.check(L.lib().vl3d_eval_view(desc, L.ptr(gt), L.ptr(pred), L.ptr(m_dev), ones, L.ptr(sse), L.ptr(ssim_sum), L.ptr(gt_min),
                                       L.ptr(dyn_sum), L.ptr(scratch), L.stream_ptr(dev)), "vl3d_eval_view")
    return sse.cpu().numpy(), ssim_sum.cpu().numpy(), gt_min.cpu().numpy(), float(dyn_sum.item()), ones, h, w


def view_image_metrics(gt_u8, pred_u8, mask=None):
    """Static PSNR / SSIM inside `mask` and the dyn error of one view, one pass of vl3d_eval_view over both clips ->
    (psnr, ssim, dyn) as python floats.

    gt_u8 uint8 [F,h,w,3], pred_u8 uint8 [T,h,w,3] on the MI355X (views allowed, e.g. the crop of a full frame: read in place); mask: 0/1
    [h,w] (any dtype; 1 = the static region) or None = all ones.  psnr / ssim: script_evaluate_ours.py:156-162, compute_img_metric over the
    first min(F, T) frames (metrics.py:15-89): the mean over frames of skimage's PSNR minus 10 log10(h w / sum m), and of the SSIM map's
    masked mean; a frame equal to its gt gives psnr inf, as numpy does.  dyn: :176-178, the mean over pixels and channels of
    (std_F(gt) - std_T(pred))^2 on 0..255 values.  An all-zero mask or a crop under 7 x 7 raises ValueError (the reference gives nan / -inf,
    resp. skimage's ValueError)."""
    sse, ssim_sum, gt_min, dyn_sum, ones, h, w = _view_stats(gt_u8, pred_u8, mask)
    n = h * w * 3
    with np.errstate(divide="ignore"):
        mse = sse.astype(np.float64) / (255.0 * 255.0 * n)
        data_range = np.where(gt_min < 0, 2.0, 1.0)       # skimage: the true image's dtype range, [-1, 1] when it dips below 0, else [0, 1]
        psnr = 10 * np.log10(data_range ** 2 / mse) - 10 * np.log10(h * w / ones)
    ssim = ssim_sum / ones / 3
    return float(np.mean(psnr)), float(np.mean(ssim)), dyn_sum / n


def static_metrics(gt_u8, pred_u8, mask=None):
    """(psnr, ssim) of view_image_metrics: script_evaluate_ours.py:149-164."""
    psnr, ssim, _ = view_image_metrics(gt_u8, pred_u8, mask)
    return psnr, ssim


def dynamic_error(gt_u8, pred_u8):
    """dyn of view_image_metrics: script_evaluate_ours.py:169-179."""
    return view_image_metrics(gt_u8, pred_u8)[2]


def _to_levels(x, name):
    """A tensor / array of k/255 values in [0, 1] -> uint8 k (on the input's device); anything else raises ValueError."""
    k = torch.as_tensor(x).double() * 255
    kr = k.round()
    if not bool(((k - kr).abs() <= 1e-6).all()) or not bool(((kr >= 0) & (kr <= 255)).all()):
        raise ValueError(f"{name} must hold values k/255, k in 0..255 (8-bit frames): the device metrics work on the integers")
    return kr.to(torch.uint8)


def compute_img_metric(im1t, im2t, metric="mse", mask=None, range01=True):
    """Drop-in for evaluations/metrics.py:15 (compute_img_metric) for "mse", "psnr" and "ssim" on 8-bit content.

    im1t (the true images), im2t: [B,H,W,3] in [0,1], every value k/255 (ValueError otherwise: what the evaluation script passes always
    is); mask: [1,H,W] or [1,H,W,1] (or [H,W]) of 0/1, or None (all ones; the reference itself fails without a mask).  Returns the mean over
    the B images as a python float.  "lpips" and range01=False raise NotImplementedError."""
    if metric not in ("mse", "psnr", "ssim", "lpips"):
        raise RuntimeError(f"img_utils:: metric {metric} not recognized")
    if metric == "lpips":
        raise NotImplementedError("lpips needs the torchvision / LPIPS backbone weights, which this package does not carry")
    if not range01:
        raise NotImplementedError("only range01=True (inputs in [0, 1]) is supported")
    a, b = _to_levels(im1t, "im1t"), _to_levels(im2t, "im2t")
    a, b = (x if x.is_cuda else x.to("cuda") for x in (a, b))
    if a.dim() != 4 or a.shape[-1] != 3 or a.shape != b.shape:
        raise ValueError(f"im1t / im2t must both be [B,H,W,3], got {tuple(a.shape)} and {tuple(b.shape)}")
    if mask is not None and torch.as_tensor(mask).dim() > 2 and torch.as_tensor(mask).shape[0] != 1:
        raise ValueError("mask must be one image: [1,H,W] or [1,H,W,1]")
    if metric == "mse":      # skimage's mean_squared_error on the [-1, 1] samples, times h w / sum m (metrics.py:66-72), mean over images
        sse, _, _, _, ones, h, w = _view_stats(a, b, mask)
        return float(np.mean(sse.astype(np.float64) / (255.0 * 255.0 * h * w * 3) * (h * w / ones)))
    psnr, ssim, _ = view_image_metrics(a, b, mask)
    return psnr if metric == "psnr" else ssim


def nn_metrics(gt, pred, configs=EVAL_PATCH_CONFIGS, macro_block=EVAL_MACRO_BLOCK):
    """script_evaluate_ours.py:201-246 on float 0..255 clips [1,3,f,h,w] on the MI355X -> (complete, coherent, loop), each a list with one
    value per configuration: completeness compute_nnerr(gt, pred), coherence compute_nnerr(pred, gt), and loop quality
    compute_nnerr(seam, gt) with the seam clip cat(pred[:, :, -pt+1:], pred[:, :, :pt-1]) (:217-220)."""
    complete, coherent, loop = [], [], []
    for (ps, s, pt, st) in configs:
        seam = torch.cat([pred[:, :, -pt + 1:], pred[:, :, :pt - 1]], dim=2)
        loop.append(compute_nnerr(seam, gt, ps, s, pt, st, macro_block))
    for (ps, s, pt, st) in configs:
        complete.append(compute_nnerr(gt, pred, ps, s, pt, st, macro_block))
        coherent.append(compute_nnerr(pred, gt, ps, s, pt, st, macro_block))
    return complete, coherent, loop


def _mean(x):
    return sum(x) / len(x)      # script_evaluate_ours.py:248


def loop_static_mask(gt_u8):
    """script_evaluate_ours.py:68-69: 1 - compute_loopable_mask(gt / 255) on the uncropped clip [F,H,W,3] -> float32 [H,W] (1 = static).
    videoloop3d_amd.train_3d.compute_loopable_mask restates cv2's arithmetic in torch (unpinned, see its docstring)."""
    from .train_3d import compute_loopable_mask
    v = torch.as_tensor(gt_u8)
    vid = (v.permute(0, 3, 1, 2).double() / 255)
    return 1 - compute_loopable_mask(vid).float()


def evaluate_views(nerf, gt_videos, extrins, intrins, crop=40, loopmasks=None, lpips=False, timings=None, baked=None):
    """script_evaluate_ours.py:108-246 for the test views: render every frame of the loop at each view's fixed camera, build the static
    mask, crop `crop` pixels off every border, score.  nerf: an MPMeshVid, bare or in nn.DataParallel (:82); gt_videos: uint8 [F,H,W,3] per
    view (arrays or tensors); extrins [V,4,4] world-to-camera, intrins [V,3,3]; loopmasks: the script's own masks (:68-69, uncropped,
    1 = static) instead of loop_static_mask.  Returns one dict per view: nnf / nnb / loop (means over the configurations), the nine
    per-configuration values, dyn, psnr, ssim, and lpips = lpips_sw = 0.0 -- not computed (the script's own value with COMPUTE_LPIPS off,
    :197-199).  timings: an optional dict that receives the seconds spent per stage (synchronised).
    baked (baked.BakedMPV / baked.BakedPool -- bake(model), bake_pool(model) or an opened viewer package): score the frames of the PLAYBACK
    model, render_frames(..., baked=baked) -- the picture that ships -- with the same metrics; `nerf` then only names the device and the clip
    length."""
    if lpips:
        raise NotImplementedError("LPIPS needs the torchvision / LPIPS backbone weights, which this package does not carry")
    import time
    from .render_video import render_frames
    module = getattr(nerf, "module", nerf)
    dev = next(module.parameters()).device
    extrins, intrins = np.asarray(extrins, dtype=np.float32), np.asarray(intrins, dtype=np.float32)
    frm = module.frm_num
    tm = timings if timings is not None else {}

    def tick(key, t0):
        torch.cuda.synchronize(dev)
        tm[key] = tm.get(key, 0.0) + time.perf_counter() - t0

    results = []
    for v, gt in enumerate(gt_videos):
        gt = torch.as_tensor(np.asarray(gt) if not torch.is_tensor(gt) else gt).to(dev)
        H, W = gt.shape[1:3]
        t0 = time.perf_counter()
        pred = render_frames(nerf, H, W, np.repeat(extrins[v:v + 1], frm, 0), np.repeat(intrins[v:v + 1], frm, 0), np.arange(frm), baked=baked)
        tick("render", t0)
        t0 = time.perf_counter()
        m = loop_static_mask(gt) if loopmasks is None else torch.as_tensor(np.asarray(loopmasks[v]), dtype=torch.float32)
        tick("mask", t0)
        c = slice(crop, -crop) if crop > 0 else slice(None)
        gtc, predc, mc = gt[:, c, c], pred[:, c, c], m[c, c]
        t0 = time.perf_counter()
        psnr, ssim, dyn = view_image_metrics(gtc, predc, mc)
        tick("static_dyn", t0)
        g = gtc.permute(3, 0, 1, 2)[None].float()
        p = predc.permute(3, 0, 1, 2)[None].float()
        complete, coherent, loop = [], [], []
        for cfg in EVAL_PATCH_CONFIGS:
            t0 = time.perf_counter()
            a, b, l = nn_metrics(g, p, (cfg,))
            complete += a
            coherent += b
            loop += l
            tick("nn_" + _config_tag(cfg), t0)
        r = {"nnf": _mean(complete), "nnb": _mean(coherent), "dyn": dyn, "lpips": 0.0, "lpips_sw": 0.0, "loop": _mean(loop),
             "psnr": psnr, "ssim": ssim}
        for tag, vals in (("nnf", complete), ("nnb", coherent), ("loop", loop)):
            for cfg, val in zip(EVAL_PATCH_CONFIGS, vals):
                r[f"{tag}_{_config_tag(cfg)}"] = val
        results.append(r)
    return results


def write_metrics_txt(path, dataname, results):
    """script_evaluate_ours.py:248-295: the header, one `{dataname}_view{i}` row per view, then the dataset row of means (the script's own
    order of additions).  Every number is written as str(float(v))."""
    tags = [_config_tag(c) for c in EVAL_PATCH_CONFIGS]
    n = len(tags)
    fmt = lambda vals: ", ".join(str(float(x)) for x in vals)
    forwards, backwards, loops = np.zeros(n + 1), np.zeros(n + 1), np.zeros(n + 1)
    with open(path, "w") as f:
        f.write(", ".join(metric_names()) + "\n")
        for i, r in enumerate(results):
            comp, coh, lq = ([r[f"{k}_{t}"] for t in tags] for k in ("nnf", "nnb", "loop"))
            f.write(f"{dataname}_view{i}, ")
            f.write(fmt([_mean(comp), _mean(coh), r["dyn"], r["lpips"], r["lpips_sw"], _mean(lq), r["psnr"], r["ssim"]]))
            f.write(", " + fmt(comp) + ", " + fmt(coh) + ", " + fmt(lq) + "\n")
            forwards[:n] += comp
            forwards[-1] += _mean(comp)
            backwards[:n] += coh
            backwards[-1] += _mean(coh)
            loops[:n] += lq
            loops[-1] += _mean(lq)
        V = len(results)
        forwards, backwards, loops = forwards / V, backwards / V, loops / V
        col = lambda k: [r[k] for r in results]
        f.write(f"{dataname}, ")
        f.write(fmt([forwards[-1], backwards[-1], _mean(col("dyn")), _mean(col("lpips")), _mean(col("lpips_sw")), loops[-1],
                     _mean(col("psnr")), _mean(col("ssim"))]))
        f.write(", " + fmt(forwards[:-1].tolist()) + ", " + fmt(backwards[:-1].tolist()) + ", " + fmt(loops[:-1].tolist()) + "\n")


def evaluate(nerf, args, poses_bounds, videos, ckpt=None, test_view_idx=None, dataname="", out_dir=None, loopmasks=None, timings=None, baked=None):
    """The whole of script_evaluate_ours.evaluate() but the disk I/O of the videos (mirrors render_video.render_video): LLFF poses ->
    test-view selection -> (optional) checkpoint -> evaluate_views -> `out_dir`/eval_metrics.txt.  videos: uint8 [F,H,W,3] per view, in
    view order (decoding mp4 is the caller's); nerf: the MPMeshVid built with render_video.reference_camera(...) of the same poses, bare or
    in nn.DataParallel.  baked: the playback model to score instead (evaluate_views).  Returns evaluate_views' list of dicts."""
    import os
    from .render_video import load_llff_poses, pose2extrin_np
    poses, intrins, _, _, _ = load_llff_poses(poses_bounds, factor=getattr(args, "factor", 1), recenter=True,
                                              bd_factor=(getattr(args, "near_factor", 1), getattr(args, "far_factor", 1)))
    tv = getattr(args, "test_view_idx", "") if test_view_idx is None else test_view_idx
    # '' = every view.  (The script reads V before assigning it at :58 -- a NameError there -- so only explicit lists ran in it.)
    views = list(map(int, tv.split(','))) if len(tv) > 0 else list(range(len(poses)))
    videos = [videos[i] for i in views]
    if loopmasks is not None:
        loopmasks = [loopmasks[i] for i in views]
    if ckpt is not None:
        sd = torch.load(ckpt, weights_only=False) if isinstance(ckpt, (str, os.PathLike)) else ckpt
        getattr(nerf, "module", nerf).init_from_mpi(sd['network_state_dict'])
    results = evaluate_views(nerf, videos, pose2extrin_np(poses[views]), intrins[views], loopmasks=loopmasks, timings=timings, baked=baked)
    if out_dir is not None:
        write_metrics_txt(os.path.join(out_dir, "eval_metrics.txt"), dataname, results)
    return results
