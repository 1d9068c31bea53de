"""Parity of the HIP looping-loss path (through the C ABI) against the reference goldens and the CPU oracle."""
import warnings

import numpy as np
import pytest
import torch

import loss_statement as LS
import patchnn_rows as PR
from oracle import vid_oracle as VO
from videoloop3d_amd import synth
from videoloop3d_amd import utils_vid as UV_MOD

pytestmark = pytest.mark.gpu
T_ = lambda a: torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def maxabs(a, b):
    return float((a.detach().double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def exact_distances(X, Y, max_bytes=1 << 30):
    """fp64 patch distances [B,n1,n2] for the top-2 gap criterion.  The direct form mean((x-y)^2) needs B*n1*n2*d doubles (82 MB per
    LOCATION at the cfg4 clip length with ps = 11 -- tens of TB for a 1080p strip: it once took a GPU box down with it), so beyond
    `max_bytes` the fp64 Gram form is used, chunked over locations: its cancellation error (~1e-13 here) is far below the 1e-5 gap."""
    B, n1 = X.shape[:2]
    n2 = Y.shape[1]
    d = X[0, 0].numel()
    if B * n1 * n2 * d * 8 <= max_bytes:
        return VO.patch_distances_exact(X, Y)
    out = torch.empty((B, n1, n2), dtype=torch.float64)
    step = max(1, int(max_bytes // max(1, (n1 + n2) * d * 8 * 3)))
    for b0 in range(0, B, step):
        x = X[b0:b0 + step].reshape(-1, n1, d).double()
        y = Y[b0:b0 + step].reshape(-1, n2, d).double()
        out[b0:b0 + step] = ((x * x).sum(-1)[:, :, None] + (y * y).sum(-1)[:, None, :] - 2.0 * (x @ y.transpose(1, 2))) / d
    return out


def nn_mismatch_is_near_tie(x, y, ps, pt, s, st, alpha, nn_gpu, rel_gap=1e-5):
    """NN parity criterion (SURVEY §7 'NN argmin parity'): indices must be identical wherever the top-2 gap of the
    exact (fp64) objective exceeds rel_gap * scale; returns (#mismatches, #unexplained)."""
    px = VO.extract_3Dpatches(x, ps, pt, s, st)
    b, c, d, h, w = px.shape
    B = h * w
    X = VO._to_location_major(px, B, pt, ps)
    Y = VO._to_location_major(VO.extract_3Dpatches(y, ps, pt, s, st), B, pt, ps)
    dist = raw = exact_distances(X, Y)
    if alpha is not None:
        dist = dist / (alpha + dist.min(1)[0][:, None])
    ref = torch.argmin(dist, dim=2)
    got = nn_gpu.cpu().long().reshape(B, -1)
    bad = (ref != got).nonzero()
    unexplained = 0
    for bi, i in bad.tolist():
        row = dist[bi, i]
        gap = abs(float(row[got[bi, i]] - row[ref[bi, i]]))
        # gap == 0 is an EXACT tie of the objective (alpha = 0: every column minimum scores q / q = 1.0, in fp64 as in fp32), which the
        # reference settles by torch.argmin's first-minimum rule: the other index is wrong, not a rounding matter
        # -- unless that column's minimum is itself a near-tie between two rows (then fp32 may hand the column to the other row)
        if gap == 0.0 and alpha is not None:
            col = raw[bi, :, ref[bi, i]]
            two = torch.topk(col, min(2, col.numel()), largest=False)[0]
            if two.numel() < 2 or float(two[1] - two[0]) > rel_gap * max(float(col.abs().max()), 1e-12):
                unexplained += 1
        elif gap > rel_gap * max(float(row.abs().max()), 1e-12):
            unexplained += 1
    return len(bad), unexplained


@pytest.mark.parametrize("ps,pt,s,st,al", [(5, 3, 2, 1, 1e10), (3, 3, 2, 1, 1e10), (5, 3, 2, 1, 0.5), (3, 2, 1, 2, 0.05)])
def test_g7_find_nn_and_merge(dev, golden, ps, pt, s, st, al):
    from videoloop3d_amd.utils_vid import FindNNpatchAndMerge
    g = golden("g7_merge.npz")
    key = f"ps{ps}_pt{pt}_s{s}_st{st}_a{al:g}"
    sm, w = FindNNpatchAndMerge(T_(g["x"]).to(dev), T_(g["y"]).to(dev), patch_size=ps, patcht_size=pt, stride=s,
                                stridet=st, alpha=al)
    assert sm.shape == tuple(g[key + "_sum"].shape) and w.shape == tuple(g[key + "_weight"].shape)
    assert maxabs(w, g[key + "_weight"]) == 0
    assert maxabs(sm, g[key + "_sum"]) <= 1e-5


@pytest.mark.parametrize("name,cfg", [
    ("ref", dict(macro_block=19, patch_size=11, stride=4, patcht_size=3, stridet=1, rou='-2', scaling=0.1, alpha=0.5, dist_fn='mse')),
    ("other", dict(macro_block=17, patch_size=3, stride=2, patcht_size=3, stridet=1, rou='-2', scaling=0.1, alpha=10000, dist_fn='mse')),
    ("trim", dict(macro_block=16, patch_size=5, stride=3, patcht_size=3, stridet=2, rou=0, scaling=0.2, alpha=10000, dist_fn='mse')),
])
def test_g8_lowmem_loss_value_and_grad(dev, golden, name, cfg):
    from videoloop3d_amd.utils_vid import Patch3DGPNNDirectLoss, Patch3DGPNNLowMemLoss
    g = golden("g8_loss.npz")
    x = T_(g["x"]).to(dev).requires_grad_(True)
    y = T_(g["y"]).to(dev)
    lm = Patch3DGPNNLowMemLoss()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        loss = lm(x, y, **cfg)
    if name == "trim":   # the reference warns when it trims (utils_vid.py:310-311)
        assert any("doesnot satisfy" in str(r.message) for r in rec)
    ref = float(g[name + "_loss"])
    assert loss.dim() == 0
    assert abs(loss.item() - ref) <= 1e-5 * max(1.0, abs(ref))
    assert maxabs(lm.last_weight, g[name + "_weight"]) == 0
    assert maxabs(lm.last_y2x, g[name + "_y2x"]) <= 1e-5
    (gx,) = torch.autograd.grad(loss, x)
    assert gx.shape == x.shape
    assert maxabs(gx, g[name + "_grad"]) <= 1e-8 + 1e-4 * float(np.abs(g[name + "_grad"]).max())
    if name != "trim":
        dcfg = {k: v for k, v in cfg.items() if k != "macro_block"}
        dl = Patch3DGPNNDirectLoss()(x.detach(), y, **dcfg)
        assert abs(dl.item() - ref) <= 1e-5 * max(1.0, abs(ref))


@pytest.mark.parametrize("shape,cfg", [
    ((12, 20, 63, 71), dict(ps=11, pt=3, s=4, st=1, alpha=0.5)),       # ref-view shipped cfg
    ((12, 20, 63, 71), dict(ps=3, pt=3, s=2, st=1, alpha=None)),       # other-view shipped cfg
    ((3, 3, 11, 11), dict(ps=11, pt=3, s=4, st=1, alpha=None)),        # exactly one patch, n1 = n2 = 1
    ((8, 5, 16, 20), dict(ps=4, pt=2, s=4, st=2, alpha=0.01)),         # stride == patch (no overlap), n2 < n1
    ((6, 30, 9, 9), dict(ps=1, pt=1, s=1, st=1, alpha=None)),          # 1x1x1 patches
])
def test_nn_and_fold_vs_oracle(dev, shape, cfg):
    from videoloop3d_amd.utils_vid import _nn_and_fold
    Tx, Ty, H, W = shape
    x = synth.make_video(Tx, H, W, seed=3)
    y = synth.make_video(Ty, H, W, seed=4)
    ps, pt, s, st, alpha = cfg["ps"], cfg["pt"], cfg["s"], cfg["st"], cfg["alpha"]
    so, wo, nno = VO.find_nn_and_merge(x, y, ps, pt, s, st, 1e10 if alpha is None else alpha, return_nn=True)
    sg, wg, nng = _nn_and_fold(x.to(dev), y.to(dev), ps, pt, s, st, alpha, normalize=False)
    nbad, unexplained = nn_mismatch_is_near_tie(x, y, ps, pt, s, st, alpha, nng)
    assert unexplained == 0
    assert maxabs(wg, wo) == 0
    if nbad == 0:
        assert (nng.cpu().long() == nno).all()
        assert maxabs(sg, so) <= 1e-5
    else:      # explained near-ties: the fold is held to the statement's fold (tests/loss_statement.py) at the kernel's OWN indices
        sk = LS.fold(y[0], nng.cpu().long(), ps, pt, s, st, Tx, torch.float32)[0]
        assert maxabs(sg, sk[None]) <= 1e-5


def test_strided_trimmed_views_need_no_copy(dev):
    """x[..., :t, :h, :w] views go to the kernel through strides; result equals the contiguous call."""
    from videoloop3d_amd.utils_vid import _nn_and_fold
    x = synth.make_video(10, 30, 33, seed=3, device=dev)
    y = synth.make_video(14, 30, 33, seed=4, device=dev)
    xs, ys = x[..., :9, :29, :31], y[..., :29, :31]
    a = _nn_and_fold(xs, ys, 5, 3, 2, 1, None, True)
    b = _nn_and_fold(xs.contiguous(), ys.contiguous(), 5, 3, 2, 1, None, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_g9_robust_kernels(dev, golden):
    from videoloop3d_amd.utils_vid import _RobustMean, robust_lossfun
    g = golden("g9_robust.npz")
    for rou in ['mse', 'abs', '0', '2', '-2', '1']:
        for sc in [0.1, 0.2]:
            x = T_(g["x"]).to(dev).requires_grad_(True)
            ref, refg = g[f"rou{rou}_s{sc}"], g[f"rou{rou}_s{sc}_grad"]
            loss = _RobustMean.apply(x, torch.zeros_like(x), rou, sc)
            assert abs(loss.item() - float(ref.mean())) <= 1e-5 * max(1.0, abs(float(ref.mean())))
            (gx,) = torch.autograd.grad(loss, x)
            assert maxabs(gx * x.numel(), refg) <= 1e-4 * max(1.0, float(np.abs(refg).max()))
            assert maxabs(robust_lossfun(x.detach(), rou, sc), ref) <= 1e-5 * max(1.0, float(np.abs(ref).max()))


def test_errors_are_python_exceptions(dev):
    from videoloop3d_amd.utils_vid import FindNNpatchAndMerge
    x = synth.make_video(8, 17, 17, seed=3, device=dev)
    with pytest.raises(RuntimeError, match="identical spatial size"):
        FindNNpatchAndMerge(x, synth.make_video(8, 17, 19, seed=4, device=dev), 5, 3, 2, 1)
    # the raw ABI wants x on the patch grid (the Python direct path floors it like UnfoldNd, test_g11_*)
    from videoloop3d_amd.utils_vid import _nn_and_fold
    with pytest.raises(RuntimeError, match="not trimmed"):
        _nn_and_fold(x[..., :16], synth.make_video(8, 17, 16, seed=4, device=dev), 5, 3, 2, 1, None, False)
    with pytest.raises(RuntimeError, match="dist_fn"):
        FindNNpatchAndMerge(x, x, 5, 3, 2, 1, dist_fn='ssim')


@pytest.mark.parametrize("H,W", [(180, 320), (720, 1280)])
def test_native_crop_loss_property(dev, H, W):
    """native training crop 180x320 (trimmed to 179x319) and the full 720p frame of the bench's loss leg, T=50+2, Ty=75:
    properties that need no oracle:
    vote counts equal the analytic patch-cover count; y2x values are convex combinations of y (within its range);
    x == a time-shifted copy of y gives zero loss with the exact shift recovered."""
    from videoloop3d_amd.utils_vid import Patch3DGPNNLowMemLoss, _nn_and_fold
    y = synth.make_video(75, H, W, seed=4, device=dev)
    x = y[:, :, 7:59].clone().requires_grad_(True)            # 52 frames = y shifted by 7
    for cfg in (dict(macro_block=65, patch_size=11, stride=4, patcht_size=3, stridet=1, rou='-2', scaling=0.1, alpha=10000),
                dict(macro_block=65, patch_size=3, stride=2, patcht_size=3, stridet=1, rou='-2', scaling=0.1, alpha=10000)):
        lm = Patch3DGPNNLowMemLoss()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss = lm(x, y, **cfg)
        assert loss.item() <= 1e-12
        ps, s = cfg["patch_size"], cfg["stride"]
        h, w = (H - ps) // s * s + ps, (W - ps) // s * s + ps
        _, _, nn = _nn_and_fold(x.detach()[..., :h, :w], y[..., :h, :w], ps, 3, s, 1, None, True)
        assert (nn == (torch.arange(50, device=dev, dtype=torch.int32) + 7)).all()
        # analytic cover count along one axis
        def cover(n, p, st):
            idx = torch.arange(n)
            lo = torch.clamp((idx - p + st) // st, min=0)
            hi = torch.clamp(idx // st, max=(n - p) // st)
            return (hi - lo + 1)
        ct = cover(52, 3, 1)[:, None, None] * cover(h, ps, s)[None, :, None] * cover(w, ps, s)[None, None, :]
        assert torch.equal(lm.last_weight[0, 0].cpu(), ct.float())
        assert float(lm.last_y2x.min()) >= 0.0 and float(lm.last_y2x.max()) < 1.0


def test_g6_get_nn_indices_low_memory(dev, golden):
    """materialised-patch NN (utils_vid.py:122-142, used by evaluations/NNMSE.py) vs the reference golden G6."""
    from videoloop3d_amd.utils_vid import extract_3Dpatches, get_NN_indices_low_memory
    g = golden("g6_nn.npz")
    X, Y = T_(g["X"]).to(dev), T_(g["Y"]).to(dev)
    for alpha, key in ((None, "nn_none"), (0.5, "nn_alpha05"), (0.005, "nn_alpha0005")):
        nn = get_NN_indices_low_memory(X, Y, alpha, 1024)
        assert nn.dtype == torch.long and nn.shape == tuple(g[key].shape)
        assert (nn.cpu().numpy() == g[key]).all()
    # extract_3Dpatches keeps the reference's (c,kt,kh,kw) channel order (golden G5)
    g5 = golden("g5_patches.npz")
    ramp = torch.arange(3 * 5 * 9 * 9, dtype=torch.float32, device=dev).reshape(1, 3, 5, 9, 9)
    assert maxabs(extract_3Dpatches(ramp, 3, 3, 2, 1), g5["p_3_3_2_1"]) == 0
    assert maxabs(extract_3Dpatches(ramp, 5, 2, 4, 2), g5["p_5_2_4_2"]) == 0


@pytest.mark.parametrize("variant", ["1", "2", "6", "0x806", "4"])
def test_patchnn_kernel_variants_agree(dev, variant, monkeypatch):
    """v2 (pixel-major staging, one location per workgroup; variant 1, the removed strided-staging kernel's number, runs it too), v4 (four
    locations per workgroup, VALU direct SSD) and v6 = variant 6 (the same workgroup on the half-precision matrix cores with split operands, |x|^2+|y|^2-2x.y like the reference; the
    default where it applies; 0x806: its workgroup-wide epilogue also without alpha instead of the per-wave one) pick the same neighbours up
    to exact-distance near-ties."""
    from videoloop3d_amd.utils_vid import _nn_and_fold
    monkeypatch.setattr(UV_MOD, "KERNEL_VARIANT", int(variant, 0))
    x = synth.make_video(12, 43, 51, seed=3)
    y = synth.make_video(20, 43, 51, seed=4)
    for ps, pt, s, st, alpha in ((11, 3, 4, 1, 0.5), (7, 3, 4, 1, None), (3, 3, 2, 1, None)):
        so, wo, nno = VO.find_nn_and_merge(x, y, ps, pt, s, st, 1e10 if alpha is None else alpha, return_nn=True)
        sg, wg, nng = _nn_and_fold(x.to(dev), y.to(dev), ps, pt, s, st, alpha, normalize=False)
        nbad, unexplained = nn_mismatch_is_near_tie(x, y, ps, pt, s, st, alpha, nng)
        assert unexplained == 0
        if nbad == 0:
            assert maxabs(sg, so) <= 1e-5


@pytest.mark.parametrize("tx,ty,ps,s,alpha", [(12, 100, 5, 2, 0.5), (62, 128, 7, 3, None), (50, 75, 11, 4, 0.5), (9, 17, 4, 1, 0.005),
                                               (82, 75, 5, 2, 0.5), (82, 122, 11, 4, 0.5), (122, 182, 7, 4, None), (126, 190, 3, 2, 0.5), (30, 192, 5, 3, None)])
def test_patchnn_matrix_core_tile_counts(dev, tx, ty, ps, s, alpha, monkeypatch):
    """The matrix-core kernel at all of its instantiations (<= 80 target frames: four locations per workgroup, hand-pipelined operand
    reads; <= 128: two locations; <= 192: one; x clips of <= 64 frames on four waves, <= 128 on eight -- cfg4's 80 / 120 and cfg5's
    120 / 180 frames), at the largest clips it takes, with a narrow last group and with alpha."""
    from videoloop3d_amd.utils_vid import _nn_and_fold
    monkeypatch.setattr(UV_MOD, "KERNEL_VARIANT", 6)
    H, W = ps + 5 * s, ps + 9 * s                        # 6 x 10 patch locations: the last group of a row is two locations wide
    x = synth.make_video(tx, H, W, seed=5)
    y = synth.make_video(ty, H, W, seed=6)
    sg, wg, nng = _nn_and_fold(x.to(dev), y.to(dev), ps, 3, s, 1, alpha, normalize=False)
    nbad, unexplained = nn_mismatch_is_near_tie(x, y, ps, 3, s, 1, alpha, nng)
    assert unexplained == 0
    assert nbad <= nng.numel() // 100


@pytest.mark.parametrize("case,reaches", PR.NEW_CASES, ids=["-".join(str(v) for v in inst) for _, inst in PR.NEW_CASES])
def test_patchnn_instantiations_no_other_test_reaches(dev, case, reaches, monkeypatch):
    """The rows of the launch tables that no other shape of this module launches (tests/test_patchnn_choice_cpu.py shows that, and that with
    these every row runs): each row first asks the chooser that it reaches the instantiation it is here for, then the criterion of
    test_patchnn_matrix_core_tile_counts at its 6 x 10 patch locations."""
    from videoloop3d_amd.utils_vid import _nn_and_fold, patchnn_choice
    tx, ty, ps, s, alpha, variant = case
    monkeypatch.setattr(UV_MOD, "KERNEL_VARIANT", variant)
    rc, c = patchnn_choice(PR.loss_desc(PR.rows_6x10([case[:5]], variant)[0]))
    assert rc == 0 and PR.instantiation(c) == reaches
    H, W = PR.frame(ps, s)
    x = synth.make_video(tx, H, W, seed=5)
    y = synth.make_video(ty, H, W, seed=6)
    sg, wg, nng = _nn_and_fold(x.to(dev), y.to(dev), ps, 3, s, 1, alpha, normalize=False)
    nbad, unexplained = nn_mismatch_is_near_tie(x, y, ps, 3, s, 1, alpha, nng)
    print(f"{case} -> {reaches}: {nbad} mismatches of {nng.numel()}, {unexplained} unexplained")
    assert unexplained == 0
    assert nbad <= nng.numel() // 100


def test_lowmem_loss_trims_inside_the_fused_op(dev):
    """The LowMem class trims x to the patch grid (utils_vid.py:307-320).  Here the fused op does it on the untrimmed tensor and writes
    the gradient in x's full shape: same loss and same gradient as slicing first (bit for bit), exact zeros outside the trimmed box."""
    from videoloop3d_amd.utils_vid import Patch3DGPNNLowMemLoss
    cfg = dict(macro_block=65, patch_size=5, stride=3, patcht_size=3, stridet=2, rou='-2', scaling=0.1, alpha=0.5)
    x0 = synth.make_video(10, 25, 31, seed=11).to(dev)            # trims to t 9, h 23, w 29
    y = synth.make_video(14, 25, 31, seed=12).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        xa = x0.clone().requires_grad_(True)
        la = Patch3DGPNNLowMemLoss()(xa, y, **cfg)
        (ga,) = torch.autograd.grad(la, xa)
        xb = x0.clone().requires_grad_(True)
        lb = Patch3DGPNNLowMemLoss()(xb[..., :9, :23, :29], y, **cfg)     # the caller slices: autograd's slice backward pads the gradient
        (gb,) = torch.autograd.grad(lb, xb)
    assert float(la) == float(lb)
    assert torch.equal(ga, gb)
    assert float(ga[..., 9:, :, :].abs().max()) == 0 and float(ga[..., 23:, :].abs().max()) == 0 and float(ga[..., 29:].abs().max()) == 0
    assert float(ga.abs().max()) > 0


@pytest.mark.parametrize("ps,s", [(11, 4), (3, 2), (7, 3), (5, 1)])
def test_fold_fixed_trip_covering_loops_equal_the_dynamic_ones(dev, ps, s, monkeypatch):
    """vote_fold_lds_k with NB x NB fixed-trip covering loops (at most 3 x 3 / 2 x 2 locations cover a pixel: the shipped configurations;
    locations that do not exist vote with weight 0) against the dynamic loops (variant bit 9; (5, 1) covers 5 x 5 and takes them anyway):
    loss, gradient, y2x and weight bit for bit, on frames with ragged borders."""
    from videoloop3d_amd.utils_vid import Patch3DGPNNLowMemLoss
    cfg = dict(macro_block=65, patch_size=ps, stride=s, patcht_size=3, stridet=1, rou='-2', scaling=0.1, alpha=0.5)
    x0 = synth.make_video(9, 61, 83, seed=21).to(dev)
    y = synth.make_video(12, 61, 83, seed=22).to(dev)
    out = []
    for variant in ("0", "0x200"):
        monkeypatch.setattr(UV_MOD, "KERNEL_VARIANT", int(variant, 0))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            xa = x0.clone().requires_grad_(True)
            L = Patch3DGPNNLowMemLoss()
            la = L(xa, y, **cfg)
            (ga,) = torch.autograd.grad(la, xa)
        out.append((float(la), ga, L.last_y2x.clone(), L.last_weight.clone()))
    assert out[0][0] == out[1][0]
    assert all(torch.equal(a, b) for a, b in zip(out[0][1:], out[1][1:]))
    assert float(out[0][1].abs().max()) > 0


def test_g10_compute_nnerr(dev, golden):
    """evaluations/NNMSE.compute_nnerr on the HIP patch-NN path vs the reference golden G10."""
    import warnings as _w
    from videoloop3d_amd.evaluations import compute_nnerr
    g = golden("g10_nnerr.npz")
    x, y = T_(g["x"]).to(dev), T_(g["y"]).to(dev)
    with _w.catch_warnings():
        _w.simplefilter("ignore")
        for (ps, s_, pt, st, mb) in [(5, 2, 3, 1, 13), (7, 2, 3, 2, 65), (3, 1, 3, 1, 9), (11, 4, 3, 1, 19)]:
            v = compute_nnerr(x, y, ps, s_, pt, st, mb)
            assert abs(v - float(g[f"ps{ps}_s{s_}_pt{pt}_st{st}_mb{mb}"])) <= 2e-6


@pytest.mark.parametrize("ps,pt,s,st,al", [(5, 3, 2, 1, 1e10), (3, 2, 2, 2, 0.5), (4, 3, 3, 1, 1e10)])
def test_g11_direct_path_takes_any_size(dev, golden, ps, pt, s, st, al):
    """`loss_name='gpnn'` is the parser default and its direct path takes x of any size (UnfoldNd floors the patch grid, FoldNd
    fills the full x.shape: utils_vid.py:206-229, 265-286) -- e.g. an even crop with the default stride 2.  Golden from the
    reference itself: outputs keep x's shape, uncovered voxels have y2x = 0 and weight 1e-10, the loss averages over all of x."""
    from videoloop3d_amd.utils_vid import FindNNpatchAndMerge, Patch3DGPNNDirectLoss
    g = golden("g11_direct_anysize.npz")
    key = f"ps{ps}_pt{pt}_s{s}_st{st}_a{al:g}"
    x = T_(g["x"]).to(dev).requires_grad_(True)
    y = T_(g["y"]).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # the direct path does not warn (it does not trim)
        sm, w = FindNNpatchAndMerge(x, y, patch_size=ps, patcht_size=pt, stride=s, stridet=st, alpha=al)
        L = Patch3DGPNNDirectLoss()
        loss = L(x, y, rou="-2", scaling=0.1, patch_size=ps, patcht_size=pt, stride=s, stridet=st, alpha=al)
    assert sm.shape == tuple(g[key + "_sum"].shape) and w.shape == tuple(g[key + "_weight"].shape)
    assert maxabs(w, g[key + "_weight"]) == 0
    assert maxabs(sm, g[key + "_sum"]) <= 1e-5
    assert maxabs(L.last_y2x, g[key + "_y2x"]) <= 1e-5 and L.last_y2x.shape == x.shape
    assert abs(float(loss.detach()) - float(g[key + "_loss"])) <= 1e-5 * max(1.0, abs(float(g[key + "_loss"])))
    (gx,) = torch.autograd.grad(loss, x)
    assert maxabs(gx, g[key + "_grad"]) <= 1e-8 + 1e-5 * float(np.abs(g[key + "_grad"]).max())


def test_y_scratch_cache_is_opt_in_and_invalidated_by_in_place_updates(dev):
    """The NN kernel's pixel-major copy of y is reused across calls only when the caller opts in with y_is_constant=True
    (utils_vid._patchnn_scratch); then an in-place change of y, a different view or a different tensor must rebuild it.  Without
    the opt-in every call re-copies y, so even writes that bypass the version counter (y.data.copy_) are seen."""
    from videoloop3d_amd import utils_vid as UV
    x = synth.make_video(8, 21, 25, seed=3, device=dev)
    y = synth.make_video(10, 21, 25, seed=4, device=dev)
    y2 = synth.make_video(10, 21, 25, seed=9, device=dev)
    ref = lambda yy: VO.find_nn_and_merge(x.cpu(), yy.cpu(), 5, 3, 2, 1, 1e10, return_nn=True)[2]
    plain = lambda yy: UV.find_nn_indices(x, yy, 5, 3, 2, 1, None)[0].cpu().long()
    yb = y.clone()
    assert torch.equal(plain(yb), ref(y))
    yb.data.copy_(y2)                                                   # bypasses the version counter
    assert torch.equal(plain(yb), ref(y2))
    run = lambda yy: UV.find_nn_indices(x, yy, 5, 3, 2, 1, None, y_is_constant=True)[0].cpu().long()
    a = run(y)
    assert torch.equal(run(y), a) and torch.equal(a, ref(y))            # second call: cache hit, same answer
    y.copy_(y2)                                                         # in-place: version counter bumps
    assert torch.equal(run(y), ref(y2))
    assert torch.equal(run(y2.clone()), ref(y2))                        # another tensor
    y3 = synth.make_video(12, 21, 25, seed=4, device=dev)
    assert torch.equal(run(y3[:, :, 2:]), ref(y3[:, :, 2:]))            # a view with an offset
    assert torch.equal(run(y3[:, :, :10]), ref(y3[:, :, :10]))          # same storage, different view


@pytest.mark.parametrize("case", ["video_smaller_than_patch", "clip_shorter_than_patch", "spatial_mismatch", "target_shorter_than_patch"])
def test_loss_refuses_what_the_reference_refuses(dev, case):
    """inputs no patch fits into, or patch grids that do not coincide: the reference's unfold / bmm raise RuntimeError
    (utils_vid.py:60-69, 213-217); here the ABI status becomes a RuntimeError as well -- no crash, no silent zero loss."""
    from videoloop3d_amd.utils_vid import Patch3DGPNNLowMemLoss, FindNNpatchAndMerge
    shapes = {"video_smaller_than_patch": ((1, 3, 6, 5, 9), (1, 3, 8, 5, 9)),
              "clip_shorter_than_patch": ((1, 3, 2, 15, 15), (1, 3, 8, 15, 15)),
              "spatial_mismatch": ((1, 3, 6, 15, 15), (1, 3, 8, 15, 19)),
              "target_shorter_than_patch": ((1, 3, 6, 15, 15), (1, 3, 2, 15, 15))}[case]
    x = synth.hash_uniform(shapes[0], seed=1).to(dev).requires_grad_(True)
    y = synth.hash_uniform(shapes[1], seed=2).to(dev)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(RuntimeError):
            FindNNpatchAndMerge(x, y, 7, 3, 2, 1)
        if case != "spatial_mismatch":                     # the loss class crops y to x's trimmed size first (utils_vid.py:319-320)
            with pytest.raises(RuntimeError):
                Patch3DGPNNLowMemLoss()(x, y, macro_block=15, patch_size=7, stride=2, patcht_size=3, stridet=1, rou="-2", scaling=0.1)


# ---- the shipped ref-view normaliser alpha = 0 (configs/mpv_base.txt:52 swd_alpha_ref = 0; utils_vid.py:122-142), golden G13 ---------------
def test_g13_alpha0_get_nn_indices_low_memory(dev, golden):
    from videoloop3d_amd.utils_vid import get_NN_indices_low_memory
    g6, g = golden("g6_nn.npz"), golden("g13_alpha0.npz")
    nn = get_NN_indices_low_memory(T_(g6["X"]).to(dev), T_(g6["Y"]).to(dev), 0, 1024)
    assert (nn.cpu().numpy() == g["a_nn_alpha0"]).all()


@pytest.mark.parametrize("variant", ["0", "1", "2", "6", "4"])
@pytest.mark.parametrize("ps,pt,s,st", [(5, 3, 2, 1), (3, 3, 2, 1), (3, 2, 1, 2)])
def test_g13_alpha0_find_nn_and_merge(dev, golden, ps, pt, s, st, variant, monkeypatch):
    from videoloop3d_amd.utils_vid import FindNNpatchAndMerge
    monkeypatch.setattr(UV_MOD, "KERNEL_VARIANT", int(variant, 0))
    g7, g = golden("g7_merge.npz"), golden("g13_alpha0.npz")
    sm, w = FindNNpatchAndMerge(T_(g7["x"]).to(dev), T_(g7["y"]).to(dev), patch_size=ps, patcht_size=pt, stride=s, stridet=st, alpha=0)
    assert maxabs(w, g[f"b_ps{ps}_pt{pt}_s{s}_st{st}_weight"]) == 0
    assert maxabs(sm, g[f"b_ps{ps}_pt{pt}_s{s}_st{st}_sum"]) <= 1e-5


@pytest.mark.parametrize("variant", ["0", "6", "4"])
def test_g13_alpha0_shipped_ref_view_loss_value_and_grad(dev, golden, variant, monkeypatch):
    """Patch3DGPNNLowMemLoss with the SHIPPED ref-view kwargs (ps 11, stride 4, pt 3, alpha = 0, rou '-2', scaling 0.1) against the reference."""
    from videoloop3d_amd.utils_vid import Patch3DGPNNDirectLoss, Patch3DGPNNLowMemLoss, find_nn_indices
    monkeypatch.setattr(UV_MOD, "KERNEL_VARIANT", int(variant, 0))
    g8, g = golden("g8_loss.npz"), golden("g13_alpha0.npz")
    x, y = T_(g8["x"]).to(dev).requires_grad_(True), T_(g8["y"]).to(dev)
    cfg = dict(macro_block=19, patch_size=11, stride=4, patcht_size=3, stridet=1, rou='-2', scaling=0.1, alpha=0, dist_fn='mse')
    lm = Patch3DGPNNLowMemLoss()
    loss = lm(x, y, **cfg)
    (gx,) = torch.autograd.grad(loss, x)
    ref = float(g["c_loss"])
    assert abs(loss.item() - ref) <= 1e-5 * max(1.0, abs(ref))
    assert maxabs(lm.last_weight, g["c_weight"]) == 0 and maxabs(lm.last_y2x, g["c_y2x"]) <= 1e-5
    assert maxabs(gx, g["c_grad"]) <= 1e-8 + 1e-4 * float(np.abs(g["c_grad"]).max())
    dl = Patch3DGPNNDirectLoss()(x.detach(), y, **{k: v for k, v in cfg.items() if k != "macro_block"})
    assert abs(dl.item() - ref) <= 1e-5 * max(1.0, abs(ref))
    nn, *_ = find_nn_indices(x.detach(), y, 11, 3, 4, 1, 0)
    assert (nn.cpu().numpy() == g["c_nn"]).all()


@pytest.mark.parametrize("variant", ["0", "1", "2", "6", "4"])
@pytest.mark.parametrize("ps,s", [(11, 4), (3, 2)])
def test_g13_alpha0_exact_ties_take_the_first_minimum(dev, golden, ps, s, variant, monkeypatch):
    """n2 > n1 at alpha = 0: most rows are decided by an EXACT tie at score 1.0 (the row is the minimum of several columns) and the
    reference keeps the first such column.  The kernels' per-column weight form scores a column minimum through its tie value."""
    from videoloop3d_amd.utils_vid import Patch3DGPNNLowMemLoss, find_nn_indices
    monkeypatch.setattr(UV_MOD, "KERNEL_VARIANT", int(variant, 0))
    g = golden("g13_alpha0.npz")
    x, y = T_(g["d_x"]).to(dev), T_(g["d_y"]).to(dev)
    nn, *_ = find_nn_indices(x, y, ps, 3, s, 1, 0)
    nbad, unexplained = nn_mismatch_is_near_tie(x.cpu(), y.cpu(), ps, 3, s, 1, 0, nn)
    assert unexplained == 0
    assert (nn.cpu().numpy() == g[f"d_ps{ps}_nn"]).all()
    xr = x.clone().requires_grad_(True)
    lm = Patch3DGPNNLowMemLoss()
    loss = lm(xr, y, macro_block=ps + 2 * s, patch_size=ps, stride=s, patcht_size=3, stridet=1, rou='-2', scaling=0.1, alpha=0)
    (gx,) = torch.autograd.grad(loss, xr)
    ref = float(g[f"d_ps{ps}_loss"])
    assert abs(loss.item() - ref) <= 1e-5 * max(1.0, abs(ref)) and maxabs(lm.last_y2x, g[f"d_ps{ps}_y2x"]) <= 1e-5
    assert maxabs(gx, g[f"d_ps{ps}_grad"]) <= 1e-8 + 1e-4 * float(np.abs(g[f"d_ps{ps}_grad"]).max())


@pytest.mark.parametrize("tx,ty,ps,s", [(52, 75, 11, 4), (52, 50, 11, 4), (82, 122, 11, 4), (122, 182, 7, 4), (52, 75, 3, 2)])
def test_alpha0_at_the_configured_clip_lengths(dev, tx, ty, ps, s):
    """alpha = 0 at the clip lengths of cfg3 (50 + 2 render frames vs 75 / 50 captured), cfg4 (80 / 120) and cfg5 (120 / 180), default
    kernel choice: exact ties follow the first-minimum rule, every other difference is a near-tie of the fp64 objective."""
    from videoloop3d_amd.utils_vid import _nn_and_fold
    H, W = ps + 5 * s, ps + 9 * s
    x, y = synth.make_video(tx, H, W, seed=7), synth.make_video(ty, H, W, seed=8)
    sg, wg, nng = _nn_and_fold(x.to(dev), y.to(dev), ps, 3, s, 1, 0, normalize=False)
    nbad, unexplained = nn_mismatch_is_near_tie(x, y, ps, 3, s, 1, 0, nng)
    assert unexplained == 0 and nbad <= nng.numel() // 100
    assert torch.isfinite(sg).all()


@pytest.mark.parametrize("variant", ["0", "4"])
def test_g13_alpha0_degenerate_input_documented_behaviour(dev, golden, variant, monkeypatch):
    """y holds exact copies of x frames (golden G13e records what the reference does there: negative column minima, NaN / +-inf scores,
    indices that follow cancellation noise).  DECISION for the HIP path: distances are never negative (direct SSD in v4, clamped Gram in v5),
    so a column whose minimum is exactly 0 scores NaN for the row(s) at distance 0 -- minimal, like torch.argmin -- and +inf for every
    other row; nothing is negative, the indices are valid and the loss is finite.  With the exact-SSD kernel (variant 4) every x patch
    that has an exact copy in y therefore picks its first copy."""
    from videoloop3d_amd.utils_vid import Patch3DGPNNLowMemLoss, find_nn_indices
    monkeypatch.setattr(UV_MOD, "KERNEL_VARIANT", int(variant, 0))
    g = golden("g13_alpha0.npz")
    x, y = T_(g["e_x"]).to(dev), T_(g["e_y"]).to(dev)
    nn, *_ = find_nn_indices(x, y, 5, 3, 2, 1, 0)
    n2 = y.shape[2] - 2
    assert int(nn.min()) >= 0 and int(nn.max()) < n2
    lm = Patch3DGPNNLowMemLoss()
    loss = lm(x.clone().requires_grad_(True), y, macro_block=9, patch_size=5, stride=2, patcht_size=3, stridet=1, rou='-2', scaling=0.1, alpha=0)
    assert np.isfinite(loss.item()) and torch.isfinite(lm.last_y2x).all()
    if variant == "4":
        # x patches 1..4 are y patches 4..7 (y = [4 random frames, x[1:7], 3 random frames], pt = 3)
        assert (nn[:, :, 1:5].cpu() == torch.arange(4, 8, dtype=torch.int32)).all()


def test_alpha0_full_720p_frame_windows(dev):
    """cfg3's loss shapes (52 x 75 frames, 720p, shipped ref-view kwargs incl. alpha = 0) on the whole frame: the indices of three windows of
    6 x 10 patch locations (a location only sees its own pixels) obey the parity criterion; votes are finite and inside y's range."""
    from videoloop3d_amd.utils_vid import _nn_and_fold
    ps, s = 11, 4
    H, W = (720 - ps) // s * s + ps, (1280 - ps) // s * s + ps
    x, y = synth.make_video(52, H, W, seed=3, device=dev), synth.make_video(75, H, W, seed=4, device=dev)
    y2x, w, nn = _nn_and_fold(x, y, ps, 3, s, 1, 0, normalize=True)
    assert int(nn.min()) >= 0 and int(nn.max()) < 73 and torch.isfinite(y2x).all()
    assert float(y2x.min()) >= 0.0 and float(y2x.max()) < 1.0
    for by, bx in ((0, 0), (87, 151), (172, 308)):
        r0, c0 = by * s, bx * s
        xc = x[..., r0:r0 + ps + 5 * s, c0:c0 + ps + 9 * s].cpu()
        yc = y[..., r0:r0 + ps + 5 * s, c0:c0 + ps + 9 * s].cpu()
        nbad, unexplained = nn_mismatch_is_near_tie(xc, yc, ps, 3, s, 1, 0, nn[by:by + 6, bx:bx + 10].contiguous())
        assert unexplained == 0 and nbad <= 30


def test_prepared_clip_crops_give_the_same_indices_and_loss(dev):
    """PreparedClip: the captured clip rewritten once into the NN kernel's form; a crop is named by its origin.  Indices, loss and gradient
    equal the per-call path bit for bit (same kernel, same operands), for crops at several origins incl. the clip's last rows / columns,
    both shipped patch shapes; last_y2x / last_weight materialise on demand."""
    from videoloop3d_amd.utils_vid import Patch3DGPNNLowMemLoss, PreparedClip, find_nn_indices
    Ty, Hf, Wf, h, w = 20, 61, 90, 35, 47
    clip = synth.make_video(Ty, Hf, Wf, seed=9, device=dev)
    pc = PreparedClip(clip)
    for (h0, w0) in ((0, 0), (13, 22), (Hf - h, Wf - w)):
        y = clip[..., h0:h0 + h, w0:w0 + w]
        x = synth.make_video(12, h, w, seed=10 + h0, device=dev).requires_grad_(True)
        for ps, s, al in ((11, 4, 0), (3, 2, 10000)):
            cfg = dict(macro_block=ps + 2 * s, patch_size=ps, stride=s, patcht_size=3, stridet=1, rou='-2', scaling=0.1, alpha=al)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                la, lb = Patch3DGPNNLowMemLoss(), Patch3DGPNNLowMemLoss()
                a = la(x, y, **cfg)
                b = lb(x, y, y_prepared=pc.crop(h0, w0), **cfg)
            (ga,), (gb,) = torch.autograd.grad(a, x), torch.autograd.grad(b, x)
            assert float(a) == float(b) and torch.equal(ga, gb)
            assert torch.equal(la.last_y2x, lb.last_y2x) and torch.equal(la.last_weight, lb.last_weight)
    with pytest.raises(RuntimeError, match="leaves the prepared clip"):
        find_nn_indices(x.detach()[..., :35, :47], clip[..., :35, :47], 3, 3, 2, 1, None, y_prepared=pc.crop(Hf - 10, 0))


@pytest.mark.parametrize("T,pad,h,w,ps,s,alpha", [(10, 2, 37, 53, 11, 4, 0.0), (9, 2, 30, 70, 3, 2, None), (50, 2, 45, 67, 5, 2, 0.5)])
def test_loss_prologue_writes_the_search_form_of_x(dev, T, pad, h, w, ps, s, alpha):
    """vl3d_loop_pad_fwd_gram: the loop-padded, gained video AND its gram16 form from one pass over the render's NHWC output -- the video
    equals vl3d_loop_pad_fwd's bit for bit, and the search on (x form, prepared clip) through vl3d_patchnn_grams returns the indices of the
    search that rewrites x itself, also when the loss trims x to the patch grid (the form keeps the untrimmed pitch and frame count)."""
    from videoloop3d_amd import _lib as L
    from videoloop3d_amd.MPV import _LoopPrologue
    from videoloop3d_amd.utils_vid import PreparedClip, PreparedX, find_nn_indices, fit_patch
    import warnings
    rgb = synth.hash_uniform((T, h, w, 3), seed=11, device=dev)
    res = synth.hash_uniform((14, 3, h, w), seed=12, device=dev)
    x0, g0 = _LoopPrologue.apply(rgb, res, pad, False)
    x1, g1 = _LoopPrologue.apply(rgb, res, pad, True)
    assert g0.numel() == 0 and g1.numel() * 4 == 16 * h * w * (T + pad) and torch.equal(x0, x1)
    y = res.permute(1, 0, 2, 3)[None].contiguous()
    yp = PreparedClip(y).crop(0, 0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        hh, ww, tt = fit_patch(h, "h", ps, s), fit_patch(w, "w", ps, s), fit_patch(T + pad, "t", 3, 1)
    xs, ys = x1[..., :tt, :hh, :ww], y[..., :hh, :ww]
    nn_a = find_nn_indices(xs, ys, ps, 3, s, 1, alpha, y_prepared=yp)[0]
    nn_b = find_nn_indices(xs, ys, ps, 3, s, 1, alpha, y_prepared=yp, x_prepared=PreparedX(g1, T + pad, h, w))[0]
    assert torch.equal(nn_a, nn_b)
    # ... and a form that does not belong to this x is refused by its dimensions, falling back to the rewrite
    nn_c = find_nn_indices(xs, ys, ps, 3, s, 1, alpha, y_prepared=yp, x_prepared=PreparedX(g1, tt - 1, h, w))[0]
    assert torch.equal(nn_a, nn_c)
