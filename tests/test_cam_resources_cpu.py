"""What hipcc gives the kernels of the camera gradient (csrc/vl3d_render_cam.hip: render_bwd_homos_k in its two conventions and nine
activation pairs, warp_bwd_homos_k, cam_finish_k), compiled like tests/test_sh_resources_cpu.py compiles the view-dependent head; no GPU needed.

The budget is the project's standing one, from the occupancy rule of CDNA4's register file: a SIMD holds 512 registers per lane, so a kernel
of at most **128** registers (VGPRs + AGPRs) runs 4 waves per SIMD, the occupancy its __launch_bounds__(256, 4) asks for.  The kernel holds
two planes' taps (walk_planes' two slots) beside the composite state and the derivative weights; a spill would put scratch traffic into the
plane loop, so scratch must be 0.  (Two frames per thread, as the frame-pair backward holds them, do not fit: 48-200 bytes of scratch.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videoloop3d_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

REG_BUDGET = 128                 # 4 waves per SIMD: floor(512 / 128) = 4, floor(512 / 136) = 3
CONVENTIONS = ("ILi0ELi0ELi0E", "ILi1ELi1ELi1E")      # (utils_mpi, zeros, pre), (affine, hardcut, post)
ACT_PAIRS = 9                    # the activation table of vl3d_render_conv.inc


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_camera_gradient_kernels_fit_four_waves_per_simd_without_scratch():
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"]
    p = subprocess.run([HIPCC] + flags + ["-c", os.path.join(CSRC, "vl3d_render_cam.hip"), "-o", os.devnull], stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if re.match(r"\w*(render_bwd_homos_k|warp_bwd_homos_k|cam_finish_k)", b)]
    names = sorted(b.split()[0] for b in blocks)
    for conv in CONVENTIONS:
        assert sum("render_bwd_homos_k" + conv in n for n in names) == ACT_PAIRS, names
    assert sum("warp_bwd_homos_k" in n for n in names) == 1 and sum("cam_finish_k" in n for n in names) == 1 and len(names) == 2 * ACT_PAIRS + 2, names
    for b in blocks:
        name = b.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))      # noqa: E731
        vgprs, agprs, scratch = num("VGPRs"), num("AGPRs"), num(r"ScratchSize \[bytes/lane\]")
        occupancy = num(r"Occupancy \[waves/SIMD\]")
        print(f"{name}: VGPRs {vgprs} AGPRs {agprs} scratch {scratch} occupancy {occupancy}")
        assert scratch == 0, name
        assert vgprs + agprs <= REG_BUDGET, f"{name}: {vgprs} + {agprs} registers: fewer than 4 waves per SIMD"
        assert occupancy >= 4, name
