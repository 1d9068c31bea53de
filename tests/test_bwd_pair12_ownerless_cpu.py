"""The 64 x 12 frame-pair backward without the owner table (render_bwd_pair_k<..., BWD_64X12, OWNERLESS>, `variant` 8), without a GPU: what hipcc gives every
instantiation of it -- the shape is only worth having while TWO 768-thread workgroups share a CU, the budget worked out in
tests/test_bwd_pair12_resources_cpu.py: no scratch, at most 80 registers (6 waves per SIMD), at most half a CU's LDS -- and what the library's
chooser says of variant 8: the 64 x 12 frame pairs wherever the default takes them, the default's own choice everywhere else."""
import os
import shutil

import pytest

from pair_kernel_resources import HIPCC, LDS_PER_CU, SHAPE_64X12, VGPR_BUDGET_64X12 as VGPR_BUDGET, pair_kernels


def ownerless_kernels(unit):
    return [k for k in pair_kernels(unit) if k.shape == SHAPE_64X12 and k.ownerless]


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_ownerless_pair12_backward_fits_two_workgroups_per_cu():
    mine = ownerless_kernels("vl3d_render_c3_mpv_sig.hip")
    # fp32 and fp16 stacks of the shipped planar convention: render_bwd_pair_k<1,1,1,1,1,false | true,false,false,BWD_64X12,true>
    assert any(k.conv == (1, 1, 1, 1, 1) and not k.f16 for k in mine), f"the fp32 instantiation is missing: {sorted(k.name for k in mine)}"
    assert any(k.conv == (1, 1, 1, 1, 1) and k.f16 for k in mine), f"the fp16 instantiation is missing: {sorted(k.name for k in mine)}"
    for k in mine:
        print(f"{k.name}: VGPRs {k.vgprs} AGPRs {k.agprs} scratch {k.scratch} LDS {k.lds} occupancy {k.occupancy}")
        assert k.scratch == 0, k.name
        assert k.vgprs + k.agprs <= VGPR_BUDGET, f"{k.name}: {k.vgprs} + {k.agprs} registers allocate more than 80: fewer than 6 waves per SIMD, one workgroup per CU"
        assert k.lds <= LDS_PER_CU // 2, k.name


# the other translation units that instantiate the kernel (sigmoid / sigmoid conventions): utils_mpi (zeros / pre, zeros / post, hardcut / pre),
# the planar convention with per-plane records, and the bake rule
OTHER_UNITS = ["vl3d_render_c0_utils_zeros_pre.hip", "vl3d_render_c1_utils_zeros_post.hip", "vl3d_render_c2_utils_hardcut_pre.hip",
               "vl3d_render_c5_mpv_planes.hip", "vl3d_render_c6_mpv_baked.hip"]


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_ownerless_pair12_backward_in_the_other_units():
    """Every instantiation, in every unit: at most 80 registers and half a CU's LDS (two workgroups per CU everywhere).  No scratch in any
    instantiation policy auto can take -- fp32 stacks of the planar coordinate convention (COORD = 1, F16 = false): plain, per-plane records,
    bake rule.  The instantiations only `variant` 8 reaches are NOT all clean, and this pins how far: hipcc spills <0,0,0,.,.,true> 12,
    <0,0,0,.,.,false> 12, <0,0,1,.,.,false> 20, <0,1,0,.,.,false> 16 and the baked fp16 <1,1,2,.,.,true> 12 bytes per lane at the 80-register
    budget (with the owner table 12 / 0 / 0 / 8 / 0 there, and 8 in <0,1,0,.,.,true>) -- the reason the default keeps the table kernel
    for them (csrc/vl3d_render_bwd_choice.h).  More than 20 bytes anywhere is a regression."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(len(OTHER_UNITS)) as ex:
        found = list(ex.map(ownerless_kernels, OTHER_UNITS))
    seen = 0
    for unit, mine in zip(OTHER_UNITS, found):
        assert len({k.name for k in mine}) == 2 and {k.f16 for k in mine} == {False, True}, f"{unit}: an fp32 and an fp16 instantiation"
        for k in mine:
            print(f"{unit} {k.name}: VGPRs {k.vgprs} AGPRs {k.agprs} scratch {k.scratch} LDS {k.lds}")
            assert k.vgprs + k.agprs <= VGPR_BUDGET and k.lds <= LDS_PER_CU // 2, k.name
            default_can_take = k.conv[0] == 1 and not k.f16
            assert k.scratch == 0 if default_can_take else k.scratch <= 20, f"{unit} {k.name}: {k.scratch} bytes of scratch"
            seen += 1
    assert seen == 2 * len(OTHER_UNITS)


@pytest.fixture(scope="module")
def R():
    import __graft_entry__ as g
    g.build()
    from videoloop3d_amd import render
    return render


def desc_of(T=50, scale=1.0, variant=0, dtype=0, D=32, H=720, W=1280):
    from videoloop3d_amd.render import RenderSpec, _desc_dims
    return _desc_dims(D, T, int(H * scale), int(W * scale), H, W, RenderSpec.mpv(variant=variant), dtype)


FIELDS = ("family", "width", "rows", "reg", "mask", "adam", "cull", "f16", "owner4", "gather9")


def whole(c):
    return tuple(int(getattr(c, n)) for n in FIELDS)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f32", "f16"])
def test_cfg3_takes_the_64x12_pairs_at_variants_0_7_8(R, dtype):
    from videoloop3d_amd import _lib as L
    for v in (0, 7, 8):
        c = R.bwd_choice(desc_of(variant=v, dtype=dtype))
        assert (c.family, c.width, c.rows) == (L.BWD_FAMILY["pair12"], 64, 12), v
        assert (c.reg, c.mask, c.adam, c.cull, c.f16) == (0, 0, 0, 0, dtype), v


def test_variant_8_is_the_default_wherever_the_pairs_do_not_apply(R):
    """outside rule 4 (regularisers, a quad map, a single frame, a stack beyond 1.07x) variant 8 names no kernel of its own"""
    cases = [dict(dkw=dict(), ckw=dict(reg_grads=True)), dict(dkw=dict(), ckw=dict(quad_keep=True)), dict(dkw=dict(T=1), ckw=dict()),
             dict(dkw=dict(scale=1.1), ckw=dict())]
    for k in cases:
        got = whole(R.bwd_choice(desc_of(variant=8, **k["dkw"]), "render", **k["ckw"]))
        want = whole(R.bwd_choice(desc_of(variant=0, **k["dkw"]), "render", **k["ckw"]))
        assert got == want, k
        assert got[0] != 3, k      # ... and none of them is the 64 x 12 pair kernel
