"""What hipcc gives the kernels of the view-dependent colour head (csrc/vl3d_render_sh.hip: render_sh_fwd_k / render_sh_bwd_k, dense and
tile-culled), compiled like tests/test_fwd2r_resources_cpu.py compiles the render conventions; no GPU needed.

The budget is the project's standing one, from the occupancy rule of CDNA4's register file: a SIMD holds 512 registers per lane, so a kernel
of at most **128** registers (VGPRs + AGPRs) runs 4 waves per SIMD, the occupancy its __launch_bounds__(256, 4) asks for.  A tap of this head
is four 16-byte loads, contracted with the basis before the tent weights so that a thread holds one f4 per tap: a spill would put scratch
traffic into the path whose loads are its memory parallelism, so scratch must be 0."""
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
def test_sh_kernels_fit_four_waves_per_simd_without_scratch():
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"]
    p = subprocess.run([HIPCC] + flags + ["-c", os.path.join(CSRC, "vl3d_render_sh.hip"), "-o", os.devnull], stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if re.match(r"\w*render_sh_(fwd|bwd)_k", b)]
    names = sorted(b.split()[0] for b in blocks)
    # forward and backward, each dense (ILb0E) and tile-culled (ILb1E)
    assert len(names) == 4 and all(sum(k in n and c in n for n in names) == 1 for k in ("render_sh_fwd_k", "render_sh_bwd_k") for c in ("ILb0E", "ILb1E")), names
    for b in blocks:
        name = b.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        vgprs, agprs, scratch = num("VGPRs"), num("AGPRs"), num(r"ScratchSize \[bytes/lane\]")
        occupancy = num(r"Occupancy \[waves/SIMD\]")
        print(f"{name}: VGPRs {vgprs} AGPRs {agprs} scratch {scratch} occupancy {occupancy}")
        assert scratch == 0, name
        assert vgprs + agprs <= REG_BUDGET, f"{name}: {vgprs} + {agprs} registers: fewer than 4 waves per SIMD"
        assert occupancy >= 4, name
