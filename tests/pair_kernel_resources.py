"""What hipcc reports for the instantiations of the frame-pair backward (render_bwd_pair_k) in one render translation unit, without a GPU:
compiled with the library's flags (device side only), parsed from -Rpass-analysis=kernel-resource-usage.  Shared by
test_kernel_schedule_canary.py, test_bwd_pair12_resources_cpu.py and test_bwd_pair12_ownerless_cpu.py; a unit is compiled once per session."""
import functools
import os
import re
import subprocess
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videoloop3d_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
         "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"]

VGPR_BUDGET_64X12 = 80           # 6 waves per SIMD: floor(512 / 80) = 6, floor(512 / 88) = 5 (test_bwd_pair12_resources_cpu.py)
LDS_PER_CU = 160 * 1024
SHAPE_32X16, SHAPE_64X12 = 2, 3  # BwdShape (csrc/vl3d_render_bwd_choice.h), as the mangled names carry it

# render_bwd_pair_k<COORD, BORDER, ORDER, RACT, AACT, F16, REG, ADAM, SHAPE, OWNERLESS>
_NAME = re.compile(r"\w*render_bwd_pair_kILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELb([01])ELb([01])ELb([01])ELN18vl3d_render_detail8BwdShapeE(\d)ELb([01])EEEv")
PairKernel = namedtuple("PairKernel", "name conv f16 reg adam shape ownerless vgprs agprs scratch lds occupancy")


@functools.lru_cache(maxsize=None)
def pair_kernels(unit):
    """every render_bwd_pair_k instantiation of csrc/<unit>, one PairKernel each"""
    out = subprocess.run([HIPCC] + FLAGS + ["-c", os.path.join(CSRC, unit), "-o", os.devnull], capture_output=True, text=True).stderr
    found = {}
    for b in re.split(r"remark: Function Name: ", out)[1:]:
        m = _NAME.match(b)
        if not m:
            continue
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))
        p = [int(v) for v in m.groups()]
        found[b.split()[0]] = PairKernel(b.split()[0], tuple(p[:5]), bool(p[5]), bool(p[6]), bool(p[7]), p[8], bool(p[9]), num("VGPRs"), num("AGPRs"),
                                         num(r"ScratchSize \[bytes/lane\]"), num(r"LDS Size \[bytes/block\]"), num(r"Occupancy \[waves/SIMD\]"))
    return tuple(found.values())
