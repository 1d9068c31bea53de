"""The depth of an RGB-D frame at a fractional loop time (include/vl3d.h "RGB-D") stated in fp64: the one output of csrc/vl3d_render_rgbd.hip
that no existing entry can vouch for -- its colour is the colour entry's, its depth at an integer frame the disparity entry's, bit for bit.
For tests/test_rgbd_statement_cpu.py (conditions on the statement alone) and tests/test_gpu_rgbd.py (the kernels against it).  Plain torch on
the CPU; nothing of the product beyond what tests/baked_statement.py and tests/disparity_statement.py import.

The statement.  The texels at loop time tau are baked_statement.render's: t = float32(tau) widened, t0 = floor(t), t1 = t0 + 1 or 0 at the
seam, f = t - t0, decoded[t0] + f (decoded[t1] - decoded[t0]) for every channel, alpha included -- in real arithmetic interpolate-then-filter
is the kernels' filter-then-interpolate.  Those one-frame values go through disparity_statement.render: the oracle's layers and composite
times rho_k = row_k . (x + c, y + c, 1).  The same evaluation with every tensor in float32 is "the statement in fp32".

Bound: disparity_statement.Statement's, B = 4 max |statement in fp32 - fp64| over the safe pixels, no floor.  Unsafe pixels:
baked_statement.unsafe_mask.  The 16-bit depth is held to |level - 65535 clamp(d64, 0, 1)| <= 65535 B + 1 (`levels_outside`): B is one to two
levels on the scenes of tests/disparity_models.py and the truncation one more, so a level-exact comparison with fp64 would test nothing; the
exact contract of depth16 is the fp32 formula on the float sink's disp of the same call (tests/test_gpu_rgbd.py).

Faults for the tests of the tests (`fault`): "alpha_of_t0" -- the alpha channel not interpolated; "rho_of_neighbour" -- every plane weighted
with the next plane's rho; "seam_to_t0" -- t1 = t0 at the loop seam in place of frame 0."""
import numpy as np
import torch

import baked_statement as BS
import disparity_statement as DS

FAULTS = ("alpha_of_t0", "rho_of_neighbour", "seam_to_t0")
LEVELS = 65535.0


def values_at(clip, time, dtype=torch.float64, fault=None):
    """the decoded texels [D,Hs,Ws,4] of `clip` [D,T,Hs,Ws,4] uint8 at `time`: an int frame, or a float loop time (interpolated) in `dtype`"""
    assert fault is None or fault in FAULTS, fault
    dec = clip.to(dtype) / 255.0
    if isinstance(time, (int, np.integer)):
        return dec[:, int(time)]
    t0, t1, f = BS.loop_time(time, clip.shape[1])
    if fault == "seam_to_t0" and t0 + 1 == clip.shape[1]:
        t1 = t0
    one = dec[:, t0] + torch.tensor(f, dtype=dtype) * (dec[:, t1] - dec[:, t0])
    if fault == "alpha_of_t0":
        one[..., 3] = dec[:, t0, ..., 3]
    return one


def render(scene, rows, cam, time, dtype=torch.float64, fault=None):
    """one output frame of a baked_statement.Scene: camera `cam` of scene.homos and rows [C,D,3] at `time` -> (disp [H,W], alpha [H,W])"""
    r = rows[cam]
    if fault == "rho_of_neighbour":
        r = r.roll(-1, 0)
    return DS.render(values_at(scene.clip, time, dtype, fault), scene.homos[cam], r, scene.H, scene.W, scene.spec, scene.keep, dtype)


def statement(scene, rows, sel, fault=None):
    """sel: [(cam, time)] -> disparity_statement.Statement of those output frames (fp64, its fp32 evaluation, the safe pixels)"""
    r64 = [render(scene, rows, c, t, torch.float64, fault) for c, t in sel]
    r32 = [render(scene, rows, c, t, torch.float32, fault) for c, t in sel]
    safe = torch.stack([~scene.unsafe(c) for c, _ in sel])
    return DS.Statement(scene.name, torch.stack([d for d, _ in r64]), torch.stack([a for _, a in r64]),
                        torch.stack([d for d, _ in r32]), torch.stack([a for _, a in r32]), safe)


def depth_levels(disp):
    """the rule of depth16 in torch, in the dtype of `disp`: trunc(65535 clip(disp, 0, 1)) -> int32"""
    return (LEVELS * disp.clamp(0, 1)).to(torch.int32)


def levels_outside(st, depth16):
    """(count, worst, tolerance): safe pixels whose level lies further than the tolerance 65535 B_disp + 1 from 65535 clamp(d64, 0, 1), and
    the largest distance"""
    got = depth16.detach().cpu().to(torch.int32).double()
    assert got.shape == st.disp.shape, (got.shape, st.disp.shape)
    d = (got - LEVELS * st.disp.clamp(0, 1)).abs()[st.safe]
    tol = LEVELS * st.bound[0] + 1.0
    return int((d > tol).sum()), (float(d.max()) if d.numel() else 0.0), tol
