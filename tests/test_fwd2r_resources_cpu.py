"""What hipcc gives the row-pair forward (render_fwd2r_k: two pixel rows per thread that share their middle tap row, 64 x 16-pixel tiles).
Every convention's translation unit is compiled like tests/test_bwd_pair12_resources_cpu.py compiles the headline file; no GPU needed.

The register budget, from the occupancy rule of CDNA4's register file: a SIMD holds 512 registers per lane, so a kernel of at most **128**
registers (VGPRs + AGPRs) runs 4 waves per SIMD = two of its 512-thread workgroups per CU, the occupancy its __launch_bounds__(512, 4) asks
for and the frame-pair forward it replaces has.  The six tap loads of the next plane are the kernel's memory parallelism: a spill would put
scratch traffic into the very path the kernel exists to thin out, so scratch must be 0 (with frames t and t+1 in the thread as well hipcc
spilled 140 bytes per lane at this budget: docs/kernels/K1_render_forward.md)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videoloop3d_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

REG_BUDGET = 128                 # 4 waves per SIMD: floor(512 / 128) = 4, floor(512 / 136) = 3


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_fwd2r_fits_four_waves_per_simd_without_scratch():
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"]
    # every compiled convention (one translation unit each, in parallel): an instantiation that spills must not be built, let alone dispatched
    units = sorted(glob.glob(os.path.join(CSRC, "vl3d_render_c*.hip")))
    procs = [subprocess.Popen([HIPCC] + flags + ["-c", u, "-o", os.devnull], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True) for u in units]
    out = "".join(p.communicate()[1] for p in procs)
    assert all(p.returncode == 0 for p in procs), out[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", out)[1:] if re.match(r"\w*render_fwd2r_k", b)]
    # the fp32 stack of the shipped planar convention: render_fwd2r_k<1,1,1,1,1> (affine, hardcut, post, sigmoid, sigmoid)
    names = {b.split()[0] for b in blocks}
    assert any("ILi1ELi1ELi1ELi1ELi1EE" in n for n in names), f"the fp32 shipped-convention instantiation is missing: {sorted(names)}"
    for b in blocks:
        name = b.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        vgprs, agprs, scratch = num("VGPRs"), num("AGPRs"), num(r"ScratchSize \[bytes/lane\]")
        occupancy = num(r"Occupancy \[waves/SIMD\]")
        print(f"{name}: VGPRs {vgprs} AGPRs {agprs} scratch {scratch} occupancy {occupancy}")
        assert scratch == 0, name
        assert vgprs + agprs <= REG_BUDGET, f"{name}: {vgprs} + {agprs} registers: fewer than 4 waves per SIMD"
