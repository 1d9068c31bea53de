"""What hipcc gives the frame-pair backward in 64 x 12-pixel regions (render_bwd_pair_k<..., BWD_64X12, OWNERLESS = false>): the kernel is only worth its shape while TWO of its
768-thread workgroups share a CU.  Compiled as tests/pair_kernel_resources.py compiles the headline file; no GPU needed.

The register budget, from the occupancy rule of CDNA4's register file: a SIMD holds 512 registers per lane, allocated in granules of 8, so
waves per SIMD = min(8, floor(512 / alloc)) with alloc = ceil(VGPRs + AGPRs, 8).  Two workgroups of 768 threads are 24 waves on the CU's four
SIMDs = 6 waves per SIMD, i.e. floor(512 / alloc) >= 6  <=>  alloc <= 85  <=>  alloc <= 80 (the largest multiple of 8): at most **80** registers.
81 would allocate 88 -> 5 waves per SIMD -> 20 waves -> one workgroup.  The CU's 160 KiB of LDS must hold both workgroups: at most 81920 bytes
each.  Scratch: a spill at this budget is a finding to record, not something to ship (docs/kernels/K2_render_backward.md)."""
import os
import shutil

import pytest

from pair_kernel_resources import HIPCC, LDS_PER_CU, SHAPE_32X16, SHAPE_64X12, VGPR_BUDGET_64X12 as VGPR_BUDGET, pair_kernels


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_pair12_backward_fits_two_workgroups_per_cu():
    every = pair_kernels("vl3d_render_c3_mpv_sig.hip")
    # exactly ten frame-pair kernels in this unit: 32 x 16 regions F16 | REG | F16 + REG | REG + ADAM | ADAM | plain, 64 x 12 regions fp32 and
    # fp16 with the owner table and without it -- an eleventh is an instantiation nobody asked for
    want = {(f16, reg, adam, SHAPE_32X16, False) for f16, reg, adam in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 1, 1), (0, 0, 1))}
    want |= {(f16, 0, 0, SHAPE_64X12, ownerless) for f16 in (0, 1) for ownerless in (False, True)}
    assert len(every) == 10 and {(k.f16, k.reg, k.adam, k.shape, k.ownerless) for k in every} == want, [k.name for k in every]
    # with the owner table.  fp32 and fp16 stacks of the shipped planar convention: render_bwd_pair_k<1,1,1,1,1,false | true,false,false,BWD_64X12,false>
    mine = [k for k in every if k.shape == SHAPE_64X12 and not k.ownerless]
    assert any(k.conv == (1, 1, 1, 1, 1) and not k.f16 for k in mine), f"the fp32 instantiation is missing: {sorted(k.name for k in mine)}"
    for k in mine:
        print(f"{k.name}: VGPRs {k.vgprs} AGPRs {k.agprs} scratch {k.scratch} LDS {k.lds} occupancy {k.occupancy}")
        assert k.scratch == 0, k.name
        assert k.vgprs + k.agprs <= VGPR_BUDGET, f"{k.name}: {k.vgprs} + {k.agprs} registers allocate more than 80: fewer than 6 waves per SIMD, one workgroup per CU"
        assert k.lds <= LDS_PER_CU // 2, k.name
