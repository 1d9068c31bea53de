"""What hipcc gives the frame-pair backward in 64 x 12-pixel regions (render_bwd_pair12_k): the kernel is only worth its shape while TWO of its
768-thread workgroups share a CU.  Compiled like tests/test_kernel_schedule_canary.py compiles the headline file; no GPU needed.

The register budget, from the occupancy rule of CDNA4's register file: a SIMD holds 512 registers per lane, allocated in granules of 8, so
waves per SIMD = min(8, floor(512 / alloc)) with alloc = ceil(VGPRs + AGPRs, 8).  Two workgroups of 768 threads are 24 waves on the CU's four
SIMDs = 6 waves per SIMD, i.e. floor(512 / alloc) >= 6  <=>  alloc <= 85  <=>  alloc <= 80 (the largest multiple of 8): at most **80** registers.
81 would allocate 88 -> 5 waves per SIMD -> 20 waves -> one workgroup.  The CU's 160 KiB of LDS must hold both workgroups: at most 81920 bytes
each.  Scratch: a spill at this budget is a finding to record, not something to ship (docs/kernels/K2_render_backward.md)."""
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
def test_pair12_backward_fits_two_workgroups_per_cu():
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"]
    out = subprocess.run([HIPCC] + flags + ["-c", os.path.join(CSRC, "vl3d_render_c3_mpv_sig.hip"), "-o", os.devnull],
                         capture_output=True, text=True).stderr
    blocks = [b for b in re.split(r"remark: Function Name: ", out) if re.match(r"\w*render_bwd_pair12_k", b)]
    # fp32 and fp16 stacks of the shipped planar convention: render_bwd_pair12_k<1,1,1,1,1,false> and <...,true>
    names = {b.split()[0] for b in blocks}
    assert any("ILi1ELi1ELi1ELi1ELi1ELb0EE" in n for n in names), f"the fp32 instantiation is missing: {sorted(names)}"
    for b in blocks:
        name = b.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        vgprs, agprs, scratch = num("VGPRs"), num("AGPRs"), num(r"ScratchSize \[bytes/lane\]")
        lds, occupancy = num(r"LDS Size \[bytes/block\]"), num(r"Occupancy \[waves/SIMD\]")
        print(f"{name}: VGPRs {vgprs} AGPRs {agprs} scratch {scratch} LDS {lds} occupancy {occupancy}")
        assert scratch == 0, name
        assert vgprs + agprs <= VGPR_BUDGET, f"{name}: {vgprs} + {agprs} registers allocate more than 80: fewer than 6 waves per SIMD, one workgroup per CU"
        assert lds <= LDS_PER_CU // 2, name
