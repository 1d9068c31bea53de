"""The float training render -- vl3d_render_fwd / _bwd, their _reg, _mask, culled and fp16 instantiations, every backward family choose_bwd()
can return -- against the fp64 statement of tests/render_statement.py, on the exact-coordinate views (samples on texel centres and on both
closed plane edges, taps of weight exactly 2^-10, a 3x3-gather and a 2x2-gather view) and one perspective scene.  Bounds: per scene and
output m max |oracle fp32 - oracle fp64|, m = 16 on exact coordinates (about 2e-6 for the picture, 1e-6 for the gradient), 4 where the
oracle's fp32 coordinates round; no floor.  tests/test_render_statement_cpu.py shows what the comparison catches without a device.
Every test prints each bound and measured maximum; every backward asserts the kernel family that ran (render.last_bwd_choice) and the plan
word.  D = 4, T = 3, a 33 x 131 frame: three regions across and two down for every region shape, an odd T and an odd H."""
import dataclasses

import pytest
import torch

import render_statement as RS

pytestmark = pytest.mark.gpu

SIZES = {"1.0x": (RS.H, RS.W), "1.1x": (37, 145)}
VIEWS = RS.EXACT_VIEWS + ("perspective",)
NO = (False, False, False, False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def _views(size="1.0x", act=("sigmoid", "sigmoid")):
    return RS.views(*SIZES[size], act=act)


def _render(dev, scene, stack, obj, variant=0, half=False, reg=False, mask=None, gcu=False, window=(0, 0), backward=True):
    """one call of the product on the device -> (RS.Result on the host, last_bwd_choice(), plan word)"""
    import videoloop3d_amd.render as R
    spec = dataclasses.replace(scene.spec, variant=variant)
    s = stack.to(dev)
    s = (s.half() if half else s).requires_grad_(backward)
    homos = scene.homos.to(dev)
    keep = None if scene.keep is None else scene.keep.to(dev)
    asum = label = m = None
    if mask is not None:
        m = mask.to(dev).requires_grad_(backward)
        rgb, alpha, label, _, asum = R.render_planes_with_mask(s, m, homos, scene.H, scene.W, spec, with_regularisers=reg)
    elif reg:
        rgb, alpha, _, asum = R.render_planes_with_regularisers(s, homos, scene.H, scene.W, spec, window=window, quad_keep=keep, grad_culled_unwritten=gcu)
    else:
        rgb, alpha = R.render_planes(s, homos, scene.H, scene.W, spec, window=window, quad_keep=keep, grad_culled_unwritten=gcu)
    res = RS.Result(rgb, alpha, asum if reg else None, label)
    choice = word = None
    if backward:
        tot = (rgb * obj.g_rgb.to(dev)).sum() + (alpha * obj.g_alpha.to(dev)).sum()
        if reg:
            tot = tot + (asum * obj.g_asum.to(dev)).sum()
        if mask is not None:
            tot = tot + (label * obj.g_label.to(dev)).sum()
        g = torch.autograd.grad(tot, [s] + ([m] if mask is not None else []))
        res.grad = g[0]
        res.gmask = g[1] if mask is not None else None
        assert res.grad.dtype == s.dtype
        choice, word = R.last_bwd_choice(), int(R.LAST_BWD_SCRATCH.view(torch.int32)[0].item())
    return RS.Result(*(None if getattr(res, n) is None else getattr(res, n).detach().float().cpu() for n in RS.OUTPUTS)), choice, word


def _check_kernel(choice, word, expect, tag):
    """the intended kernel ran: expect = (family, width, rows, reg, mask, adam, cull, f16), the shape unread for the atomics kernel"""
    if expect[0] == "atomics":
        assert choice[0] == "atomics" and word == 0, (tag, choice, word)
    else:
        assert choice == expect and word == 1, (tag, choice, expect, word)


def _row(dev, scenes, expect, variant, Tn=RS.T, half=False, reg=False, with_mask=False, gcu=False, stack_of=RS.make_stack, tag="", names=None):
    """one kernel row on every scene of `scenes`: statement (cached by what defines it), one call, the kernel that ran, every output"""
    from videoloop3d_amd import tiles
    for sc in scenes:
        stack = stack_of(sc, Tn)
        stack = stack.half().float() if half else stack
        mask = RS.synth.hash_uniform((RS.D, Tn, sc.Hs, sc.Ws), seed=6) * 3 - 2 if with_mask else None
        obj = RS.objective(sc, Tn, asum=reg, label=with_mask)
        st = RS.statement(sc, stack, obj, mask, key=(sc.name, sc.Hs, sc.Ws, sc.spec, Tn, half, reg, with_mask, stack_of.__name__))
        texels = tiles.quad_to_texel_mask(sc.keep, sc.Hs, sc.Ws, sc.spec.tile) if gcu else None
        st = dataclasses.replace(st, half=half, texels=texels)
        got, choice, word = _render(dev, sc, stack, obj, variant, half, reg, mask, gcu)
        what = f"{tag} variant {variant} T {Tn} {sc.Hs}x{sc.Ws}" + (" fp16" if half else "") + (" asum" if reg else "") + (" gcu" if gcu else "")
        _check_kernel(choice, word, expect, (sc.name, what))
        assert float(st.r64.grad.abs().max()) > 1e-3
        st.check(what + f" -> {choice[0]} {choice[1]}x{choice[2]}", got, names)


# ---- dense fp32 ---------------------------------------------------------------------------------------------------------------------------------------
DENSE = {1: ("atomics",), 3: ("tile", 64, 16, False) + NO, 2: ("tile", 64, 8, False) + NO, 5: ("tile", 32, 16, False) + NO,
         6: ("pair", 32, 16, False) + NO, 7: ("pair12", 64, 12, False) + NO, 8: ("pair12", 64, 12, False) + NO, 0: ("pair12", 64, 12, False) + NO}


@pytest.mark.parametrize("variant", list(DENSE))
def test_dense_fp32(dev, variant):
    _row(dev, [_views()[v] for v in VIEWS], DENSE[variant], variant, tag="dense")


@pytest.mark.parametrize("variant,expect", [(0, ("tile", 64, 8, False) + NO), (3, ("tile", 64, 16, False) + NO)])
def test_dense_single_frame(dev, variant, expect):
    """T = 1: the flat 64 x 8 regions with the four-texel owner table by default, the 64 x 16 ones with the one-texel pass (variant 3)"""
    _row(dev, [_views()[v] for v in VIEWS], expect, variant, Tn=1, tag="dense")


def test_dense_larger_stack(dev):
    """a 1.1x stack leaves rule 4's `fits`: the 64 x 16 one-frame kernel, windows wider than 64 texels"""
    _row(dev, [_views("1.1x")[v] for v in VIEWS], ("tile", 64, 16, False) + NO, 0, tag="dense")


# ---- REG instantiations: the sparsity sums alone (smooth; the layer differences' sign kinks stay with the fp32 tests) -----------------------------------
REG = {0: ("pair", 32, 16, True) + NO, 3: ("tile", 64, 16, True) + NO, 5: ("tile", 32, 16, True) + NO, 1: ("atomics",)}


@pytest.mark.parametrize("variant", list(REG))
def test_reg_fp32(dev, variant):
    _row(dev, [_views()[v] for v in VIEWS], REG[variant], variant, reg=True, tag="reg")


# ---- fp16 stacks: the statement on the half-rounded values; gradient allowance B + 2^-11 |g64| + 2^-25 ---------------------------------------------------
F16 = (False, False, False, True)
HALF = {0: ("pair12", 64, 12, False) + F16, 8: ("pair12", 64, 12, False) + F16, 6: ("pair", 32, 16, False) + F16, 3: ("tile", 64, 16, False) + F16}


@pytest.mark.parametrize("variant", list(HALF))
def test_fp16(dev, variant):
    _row(dev, [_views()[v] for v in VIEWS], HALF[variant], variant, half=True, tag="fp16")


def test_fp16_reg_pairs(dev):
    _row(dev, [_views()[v] for v in VIEWS], ("pair", 32, 16, True) + F16, 0, half=True, reg=True, tag="fp16 reg")


# ---- quad maps: shared borders and tile-exact ------------------------------------------------------------------------------------------------------------
def _quad_expect(variant, gcu):
    cull = (False, False, True, False)
    if variant == 5 or (variant == 0 and gcu):
        return ("tile", 32, 16, gcu and variant == 5) + cull
    return ("tile", 64, 16, gcu) + cull


@pytest.mark.parametrize("gcu", [False, True])
@pytest.mark.parametrize("variant", [0, 3, 5])
def test_quad_maps(dev, variant, gcu):
    """tile-culled models: zero-filled culled texels, and grad_culled_unwritten compared on the texels of kept quads only"""
    _row(dev, list(RS.quad_scenes().values()), _quad_expect(variant, gcu), variant, gcu=gcu, tag="quad map")


# ---- the loop-mask channel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("variant,rows", [(0, 8), (3, 16)])
def test_mask_channel(dev, variant, rows, reg):
    """render_planes_with_mask: colours, label, (sparsity sums,) stack gradient and mask gradient"""
    _row(dev, [_views()[v] for v in VIEWS], ("tile", 64, rows, reg, True, False, False, False), variant, reg=reg, with_mask=True, tag="mask")


# ---- the utils_mpi convention ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,expect", [(0, ("pair12", 64, 12, False) + NO), (3, ("tile", 64, 16, False) + NO), (1, ("atomics",))])
def test_utils_mpi(dev, variant, expect):
    _row(dev, [RS.utils_mpi_scene(*SIZES["1.0x"])], expect, variant, tag="utils_mpi")


# ---- forward entries -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True])
def test_frame_run_inside_a_longer_clip(dev, half):
    """render_frame_run: frames 1 .. 3 of a clip of 5 read in place, and a run of one"""
    import videoloop3d_amd.render as R
    for size in SIZES:
        for sc in _views(size).values():
            clip = RS.make_stack(sc, 5)
            clip = clip.half().float() if half else clip
            on_dev = clip.to(dev).half() if half else clip.to(dev)
            for f0, n in ((1, 3), (4, 1)):
                st = RS.statement(sc, clip[:, f0:f0 + n].contiguous())
                rgb, alpha = R.render_frame_run(on_dev, f0, n, sc.homos.to(dev), sc.H, sc.W, sc.spec)
                st.check(f"frame run {f0}+{n} of 5 {size}" + (" fp16" if half else ""), RS.Result(rgb.cpu(), alpha.cpu()))


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("Tn", [1, 2, 5])
def test_frame_counts(dev, Tn, half):
    """T in {1, 2, 5}: a single frame, one pair, two pairs and a tail -- forward and default backward"""
    scenes = _views()
    for v in VIEWS:
        sc = scenes[v]
        stack = RS.make_stack(sc, Tn)
        stack = stack.half().float() if half else stack
        obj = RS.objective(sc, Tn)
        st = dataclasses.replace(RS.statement(sc, stack, obj), half=half)
        got, choice, word = _render(dev, sc, stack, obj, 0, half)
        assert word == 1 and choice[0] == ("tile" if Tn == 1 else "pair12"), choice
        st.check(f"T {Tn}" + (" fp16" if half else "") + f" -> {choice[0]} {choice[1]}x{choice[2]}", got)


@pytest.mark.parametrize("window", [(0, 0), (5, 64), (16, 3)])
def test_window_with_integer_offsets(dev, window):
    """window=(row0, col0): the 17 x 67 window at that corner of the 33 x 131 frame, forward and backward (a row band of a larger frame)"""
    h, w = 17, 67
    assert all(r + h <= RS.H and c + w <= RS.W for r, c in [window])
    for v, full in _views().items():
        sc = dataclasses.replace(full, H=h, W=w)
        stack = RS.make_stack(sc)
        # (the unsafe pixels of the window: the full frame's mask cropped -- the statement renders the full frame and crops)
        bad = RS.unsafe_mask(full)[window[0]:window[0] + h, window[1]:window[1] + w]
        obj = RS.objective(sc, unsafe=bad)
        r64 = RS.evaluate(sc, stack, obj, torch.float64, window=window)
        r32 = RS.evaluate(sc, stack, obj, torch.float32, window=window)
        st = RS.Statement(sc, r64, r32, ~bad)
        got, choice, word = _render(dev, sc, stack, obj, 0, window=window)
        assert word == 1
        st.check(f"window {window} -> {choice[0]} {choice[1]}x{choice[2]}", got)


# ---- value edges -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [3, 0, 6])
def test_saturated_logits(dev, variant):
    """logits from {-104, -40, -17, 0, 17, 40, 104} mixed into a normal stack: exp overflow and underflow in the sigmoid and its derivative,
    alphas of exactly 0 and 1 after rounding -- finite and within the bound, one-frame and pair kernels"""
    _row(dev, [_views()[v] for v in VIEWS], DENSE[variant], variant, stack_of=RS.edge_logit_stack, tag="saturated")


@pytest.mark.parametrize("convention", ["planar", "utils_mpi"])
@pytest.mark.parametrize("variant", [1, 3, 0])
def test_opaque_planes_with_identity_activations(dev, convention, variant):
    """alpha_act = rgb_act = 'none' (what a decoded viewer package renders with): alphas in [0.02, 0.9] and blocks of exactly 1.0, so some
    blended alphas are exactly 1 with planes behind them.  d/da of an opaque plane still holds -T (composite of the planes behind): torch's
    cumprod backward is exact at the zero, and so is the statement"""
    act = ("none", "none")
    scenes = [_views(act=act)[v] for v in VIEWS] if convention == "planar" else [RS.utils_mpi_scene(*SIZES["1.0x"], act=act)]
    for sc in scenes:
        if sc.exact_coverage:
            a = RS.evaluate(sc, RS.opaque_stack(sc), dtype=torch.float64)
            assert float(a.alpha.max()) >= 1.0 - 1e-12 and float(a.asum[..., 0].max()) > 1.0      # opaque, with planes in front or behind
    expect = ("atomics",) if variant == 1 else ("tile", 64, 16, False) + NO
    _row(dev, scenes, expect, variant, stack_of=RS.opaque_stack, tag=f"opaque {convention}")
