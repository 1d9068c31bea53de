"""The 64 x 12 frame-pair backward without the owner table (render_bwd_pair12o_k, `variant` 8), without a GPU: what hipcc gives every
instantiation of it -- the shape is only worth having while TWO 768-thread workgroups share a CU, the budget worked out in
tests/test_bwd_pair12_resources_cpu.py: no scratch, at most 80 registers (6 waves per SIMD), at most half a CU's LDS -- and what the library's
chooser says of variant 8: the 64 x 12 frame pairs wherever the default takes them, the default's own choice everywhere else."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videoloop3d_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

VGPR_BUDGET = 80                 # 6 waves per SIMD: floor(512 / 80) = 6, floor(512 / 88) = 5
LDS_PER_CU = 160 * 1024


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_ownerless_pair12_backward_fits_two_workgroups_per_cu():
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"]
    out = subprocess.run([HIPCC] + flags + ["-c", os.path.join(CSRC, "vl3d_render_c3_mpv_sig.hip"), "-o", os.devnull],
                         capture_output=True, text=True).stderr
    blocks = [b for b in re.split(r"remark: Function Name: ", out) if re.match(r"\w*render_bwd_pair12o_k", b)]
    names = {b.split()[0] for b in blocks}
    # fp32 and fp16 stacks of the shipped planar convention: render_bwd_pair12o_k<1,1,1,1,1,false> and <...,true>
    assert any("ILi1ELi1ELi1ELi1ELi1ELb0EE" in n for n in names), f"the fp32 instantiation is missing: {sorted(names)}"
    assert any("ILi1ELi1ELi1ELi1ELi1ELb1EE" in n for n in names), f"the fp16 instantiation is missing: {sorted(names)}"
    for b in blocks:
        name = b.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        vgprs, agprs, scratch = num("VGPRs"), num("AGPRs"), num(r"ScratchSize \[bytes/lane\]")
        lds, occupancy = num(r"LDS Size \[bytes/block\]"), num(r"Occupancy \[waves/SIMD\]")
        print(f"{name}: VGPRs {vgprs} AGPRs {agprs} scratch {scratch} LDS {lds} occupancy {occupancy}")
        assert scratch == 0, name
        assert vgprs + agprs <= VGPR_BUDGET, f"{name}: {vgprs} + {agprs} registers allocate more than 80: fewer than 6 waves per SIMD, one workgroup per CU"
        assert lds <= LDS_PER_CU // 2, name


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
    budget (render_bwd_pair12_k spills 12 / 0 / 0 / 8 / 0 there, and 8 in <0,1,0,.,.,true>) -- the reason the default keeps the table kernel
    for them (csrc/vl3d_render_bwd_choice.h).  More than 20 bytes anywhere is a regression."""
    from concurrent.futures import ThreadPoolExecutor
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"]
    run = lambda u: subprocess.run([HIPCC] + flags + ["-c", os.path.join(CSRC, u), "-o", os.devnull], capture_output=True, text=True).stderr
    with ThreadPoolExecutor(len(OTHER_UNITS)) as ex:
        outs = list(ex.map(run, OTHER_UNITS))
    seen = 0
    for unit, out in zip(OTHER_UNITS, outs):
        blocks = [b for b in re.split(r"remark: Function Name: ", out) if re.match(r"\w*render_bwd_pair12o_k", b)]
        assert len({b.split()[0] for b in blocks}) == 2, f"{unit}: an fp32 and an fp16 instantiation"
        for b in blocks:
            name = b.split()[0]
            num = lambda key: int(re.search(key + r": (\d+)", b).group(1))
            vgprs, agprs, scratch, lds = num("VGPRs"), num("AGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]")
            print(f"{unit} {name}: VGPRs {vgprs} AGPRs {agprs} scratch {scratch} LDS {lds}")
            assert vgprs + agprs <= VGPR_BUDGET and lds <= LDS_PER_CU // 2, name
            default_can_take = "pair12o_kILi1E" in name and name.endswith("Lb0EEEvN18vl3d_render_detail10RenderArgsE")
            assert scratch == 0 if default_can_take else scratch <= 20, f"{unit} {name}: {scratch} bytes of scratch"
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
