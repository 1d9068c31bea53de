"""What hipcc gives the RGB-D kernels (csrc/vl3d_render_rgbd.hip: render_rgbd_baked_k, render_rgbd_baked_pool_k) beside their colour twins
(render_fwd_baked_k of csrc/vl3d_render_baked.hip, render_fwd_baked_pool_k of csrc/vl3d_render_baked_pool.hip), compiled as
tests/test_sh_resources_cpu.py compiles its unit; no GPU needed.

Every RGB-D kernel: scratch 0 -- the taps in flight are its memory parallelism, a spill would put scratch traffic between them.  Occupancy: at
least its colour twin's (the same NF, CULL, PATH; FloatOut beside RgbdFloat, DisplayOut beside RgbdDisplay), except the instantiations of
BELOW_TWIN: one more accumulator per frame, rho per slot and the second store take 2 to 8 registers, which crosses a step of 8 registers
per wave (64: 8 waves per SIMD, 72: 7, 80: 6) in five of the 24 kernels; there scratch stays 0 and the occupancy reached is asserted as it
stands in docs/kernels/K9_baked_playback.md "RGB-D"."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "videoloop3d_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (kernel, NF, CULL or None for the pool, PATH, sink) -> the occupancy reached, one below the twin's
BELOW_TWIN = {("clip", 1, True, "PathTime", "display"): 7, ("clip", 1, False, "PathTime", "display"): 7, ("clip", 2, False, "NoPath", "display"): 7,
              ("pool", 1, None, "PathTime", "float"): 7, ("pool", 2, None, "NoPath", "display"): 6}


def _remarks(units):
    """unit -> the resource remarks of its kernels; the units compile side by side"""
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
             "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only"]
    procs = {u: subprocess.Popen([HIPCC] + flags + ["-c", os.path.join(CSRC, u), "-o", os.devnull], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                                 text=True) for u in units}
    out = {}
    for u, p in procs.items():
        out[u] = p.communicate()[1]
        assert p.returncode == 0, out[u][-2000:]
    return out


def _resources(remarks, kernel):
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]:
        name = b.split()[0]
        m = re.search(r"\d+" + kernel + r"ILi(\d)E(?:Lb(\d)E)?NS_\d+(NoPath|PathIdx|PathTime)ENS_\d+(\w+?)EEEv", name)
        if not m:
            continue
        num = lambda key: int(re.search(key + r": (\d+)", b).group(1))      # noqa: E731
        sink = {"FloatOut": "float", "RgbdFloat": "float", "DisplayOut": "display", "RgbdDisplay": "display"}[m.group(4)]
        key = ("pool" if "pool" in kernel else "clip", int(m.group(1)), None if m.group(2) is None else bool(int(m.group(2))), m.group(3), sink)
        assert key not in out, key
        out[key] = dict(name=name, regs=num("VGPRs") + num("AGPRs"), scratch=num(r"ScratchSize \[bytes/lane\]"), occupancy=num(r"Occupancy \[waves/SIMD\]"))
    return out


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_rgbd_kernels_have_no_scratch_and_their_colour_twins_occupancy():
    rem = _remarks(["vl3d_render_rgbd.hip", "vl3d_render_baked.hip", "vl3d_render_baked_pool.hip"])
    rgbd = {**_resources(rem["vl3d_render_rgbd.hip"], "render_rgbd_baked_k"), **_resources(rem["vl3d_render_rgbd.hip"], "render_rgbd_baked_pool_k")}
    twin = {**_resources(rem["vl3d_render_baked.hip"], "render_fwd_baked_k"), **_resources(rem["vl3d_render_baked_pool.hip"], "render_fwd_baked_pool_k")}
    # a clip: (run pairs, run of one, path, loop time) x (dense, culled) x (float, display); a pool: the four selections x the two sinks
    assert len(rgbd) == 24 and len([k for k in rgbd if k[0] == "clip"]) == 16, sorted(rgbd)
    assert set(BELOW_TWIN) <= set(rgbd)
    for key, r in sorted(rgbd.items(), key=str):
        t = twin[key]
        print(f"{key}: registers {r['regs']} scratch {r['scratch']} occupancy {r['occupancy']}; colour twin: registers {t['regs']} occupancy {t['occupancy']}")
        assert r["scratch"] == 0, r["name"]
        if key in BELOW_TWIN:
            assert r["occupancy"] == BELOW_TWIN[key] and t["occupancy"] == BELOW_TWIN[key] + 1, (key, r, t)
        else:
            assert r["occupancy"] >= t["occupancy"], (key, r, t)
