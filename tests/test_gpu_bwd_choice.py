"""Every backward variant gives the gradient bits of the 64 x 16 one-frame kernel -- and reaches the kernel include/vl3d.h names for it: the
choice vl3d_render_bwd_choice reports for each call is the table's (csrc/vl3d_render_bwd_choice.h), so the equal bits come from as many
different kernels as the table says.  One small scene: the shipped planar convention, D = 3, an odd T = 3 (the frame pairs get a tail frame),
a 33 x 131 frame on a stack of its own size -- at least three regions across and two down for every shape, inside the pair dispatch."""
import math

import pytest
import torch

from videoloop3d_amd import synth

pytestmark = pytest.mark.gpu

D, T, H, W = 3, 3, 33, 131
VARIANTS = (0, 2, 3, 5, 6, 7)


def expected(variant, reg):
    """(family, width, rows, REG) of a dense T >= 2 call of the shipped planar convention (fp32) whose stack is no larger than the frame, row
    by row from the table of choose_bwd()"""
    if not reg and variant in (0, 6, 7):                 # rule 4: frame pairs without regularisers
        return ("pair", 32, 16, False) if variant == 6 else ("pair12", 64, 12, False)
    if reg and variant == 0:                             # rule 5: with them the 32 x 16 pairs, by default only
        return ("pair", 32, 16, True)
    if variant == 5:                                     # rule 6: the narrow one-frame regions
        return ("tile", 32, 16, reg)
    if variant == 2 and not reg:                         # rule 7: the flat one-frame regions (no regularisers)
        return ("tile", 64, 8, False)
    return ("tile", 64, 16, reg)                         # rule 8


def _homos(D, H, W):
    from videoloop3d_amd.utils_mpi import compute_homography, make_depths
    ref_e, Kr, tar_e, Kt = synth.make_cameras(H, W)
    depths = make_depths(D, 1.0, 100.0).flip(0)
    return compute_homography(ref_e[None], Kr[None], tar_e[None], Kt[None], torch.tensor([0., 0., 1.]).expand(1, D, 3), depths[None])[0]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import __graft_entry__ as g
    g.build()
    return torch.device("cuda:0")


def test_every_variant_gives_variant_3s_bits_from_the_kernel_the_table_names(dev):
    import videoloop3d_amd.render as R
    assert H * 100 <= H * 107 and -(-W // 62) >= 3 and -(-W // 30) >= 3 and -(-H // 14) >= 2 and -(-H // 6) >= 2 and -(-H // 10) >= 2
    spec = dict(scale=(1.0, 1.0), offset=(-0.5, 0.25))
    stack = synth.make_plane_stack(D, T, H, W, seed=41, device=dev).requires_grad_(True)
    th = math.radians(2.0)
    Rz = torch.tensor([[math.cos(th) * 1.01, -math.sin(th), 1.0], [math.sin(th), math.cos(th) * 0.99, 0.5], [2e-5, -3e-5, 1.0]])
    homos = (_homos(D, H, W) @ Rz).to(dev)
    g_rgb = synth.hash_uniform((T, H, W, 3), seed=5, device=dev) - 0.5
    g_a = synth.hash_uniform((T, H, W), seed=6, device=dev) - 0.5
    reported = set()
    for reg in (False, True):
        grads = {}
        for v in VARIANTS:
            s = R.RenderSpec.mpv(variant=v, **spec)
            if reg:
                rgb, alpha, sums, asum = R.render_planes_with_regularisers(stack, homos, H, W, s)
                obj = (rgb * g_rgb).sum() + (alpha * g_a).sum() + 1e-4 * (sums * torch.tensor([1.0, 2.0, 3.0, 4.0], device=dev)).sum() + 1e-3 * asum.sum()
            else:
                rgb, alpha = R.render_planes(stack, homos, H, W, s)
                obj = (rgb * g_rgb).sum() + (alpha * g_a).sum()
            (grads[v],) = torch.autograd.grad(obj, stack)
            assert int(R.LAST_BWD_SCRATCH.view(torch.int32)[0].item()) == 1, (v, reg)        # the plan word: the owner-computes path ran
            c = R.last_bwd_choice()
            assert c == expected(v, reg) + (False, False, False, False), (v, reg)             # ... no MASK, ADAM, CULL, F16
            reported.add(c)
        ref = grads[3]
        assert float(ref.abs().max()) > 1e-3 and torch.isfinite(ref).all()
        for v in VARIANTS:
            assert torch.equal(grads[v], ref), (v, reg)
    assert len(reported) == len({expected(v, reg) for v in VARIANTS for reg in (False, True)}) == 8
