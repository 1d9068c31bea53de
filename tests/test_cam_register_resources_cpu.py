"""What hipcc gives the kernels of the camera registration (csrc/vl3d_render_cam_register.hip: render_cam_register_k in its two conventions,
nine activation pairs and two parameter counts PN = 6, 8 -- mode and brightness are kernel arguments, not template parameters -- and
cam_register_finish_k), compiled like tests/test_cam_normal_resources_cpu.py compiles the normal equations; no GPU needed.

Beside what render_cam_normal_k holds over the plane loop the kernel keeps three accumulators of the long exposure's picture.  Hard conditions:
scratch 0 in EVERY instantiation, and at least 3 waves per SIMD (at most 168 registers).  Every instantiation reaches the occupancy its
render_cam_normal_k twin is built for, so the 15 four-wave cases are pinned: a sigmoid alpha, except PN = 8 under activate-then-sample
(docs/kernels/K2_render_backward.md, "Camera registration")."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videoloop3d_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

BUDGET = {4: 128, 3: 168}        # waves per SIMD -> registers: floor(512 / 128) = 4, floor(512 / 168) = 3
CONVENTIONS = ("ILi0ELi0ELi0E", "ILi1ELi1ELi1E")      # (utils_mpi, zeros, pre), (affine, hardcut, post)
ACT_PAIRS = 9                    # the activation table of vl3d_render_conv.inc
SIGMOID = 1                      # VL3D_ACT_SIGMOID
LDS = 4 * 4 * 80 * 4             # [4 waves][4 rows of lanes][five groups of 16 sums] floats


def waves_wanted(name):
    """the occupancy of the instantiation's render_cam_normal_k twin, from the mangled template arguments <COORD, BORDER, ORDER, RACT, AACT, PN>"""
    coord, border, order, ract, aact, pn = (int(v) for v in re.search(r"render_cam_register_kILi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)ELi(\d)E", name).groups())
    return 4 if (aact == SIGMOID and not (pn == 8 and order == 0)) else 3


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_registration_kernels_fit_their_occupancy_without_scratch():
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"]
    p = subprocess.run([HIPCC] + flags + ["-c", os.path.join(CSRC, "vl3d_render_cam_register.hip"), "-o", os.devnull], stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = [b for b in re.split(r"remark: [^\n]*Function Name: ", p.stderr)[1:] if re.match(r"\w*(render_cam_register_k|cam_register_finish_k)", b)]
    names = sorted(b.split()[0] for b in blocks)
    assert not any("render_cam_normal_k" in n or "cam_normal_finish_k" in n for n in names)
    for conv in CONVENTIONS:
        for pn in (6, 8):
            assert sum(bool(re.search("render_cam_register_k" + conv + rf"Li\dELi\dELi{pn}E", n)) for n in names) == ACT_PAIRS, names
    assert sum("cam_register_finish_k" in n for n in names) == 1 and len(names) == 4 * ACT_PAIRS + 1, names
    four = 0
    for b in blocks:
        name = b.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))      # noqa: E731
        vgprs, agprs, scratch = num("VGPRs"), num("AGPRs"), num(r"ScratchSize \[bytes/lane\]")
        occupancy, lds = num(r"Occupancy \[waves/SIMD\]"), num(r"LDS Size \[bytes/block\]")
        print(f"{name}: VGPRs {vgprs} AGPRs {agprs} scratch {scratch} occupancy {occupancy} LDS {lds}")
        assert scratch == 0, name
        if "finish" in name:
            continue
        assert vgprs + agprs <= BUDGET[3] and occupancy >= 3, f"{name}: {vgprs} + {agprs} registers: fewer than 3 waves per SIMD"
        assert lds == LDS, (name, lds)
        want = waves_wanted(name)
        four += want == 4
        assert vgprs + agprs <= BUDGET[want], f"{name}: {vgprs} + {agprs} registers: fewer than {want} waves per SIMD"
        assert occupancy >= want, name
    assert four == 5 + 5 + 5      # the five pairs with a sigmoid alpha: both conventions at PN = 6, the planar one at PN = 8
