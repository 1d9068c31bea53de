"""Records tests/golden/patchnn_scratch_bytes.npz: vl3d_patchnn_scratch_bytes of a GIVEN build of the library for clips of Tx, Ty = 3, 6, ...,
198 frames, two frame sizes and the temporal patch settings (pt, stridet) = (3, 1) and (2, 2).  The committed file was recorded from the
library built at the commit before the byte count was computed from the patch grid of csrc/vl3d_patchnn_choice.h (it was an expression of its
own in csrc/vl3d_loss.hip): check that commit out into a directory of its own, build it there
(python -c "import __graft_entry__ as g; g.build()"), and run, from this tree,
    python tests/golden/make_patchnn_scratch_bytes.py THAT_CHECKOUT/videoloop3d_amd/lib/libvl3d_hip.so
tests/test_patchnn_choice_cpu.py::test_scratch_bytes_are_what_they_were compares the current library with the file.  No GPU is touched."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from videoloop3d_amd._lib import LossDesc  # noqa: E402

FRAMES = list(range(3, 201, 3))
SIZES = [(31, 47), (719, 1279)]            # (H, W)
TEMPORAL = [(3, 1), (2, 2)]                # (pt, stridet)


def sweep(f):
    """f: vl3d_patchnn_scratch_bytes -> int64 [size][temporal][Tx][Ty]"""
    out = np.zeros((len(SIZES), len(TEMPORAL), len(FRAMES), len(FRAMES)), dtype=np.int64)
    d = LossDesc()
    d.ps, d.stride = 3, 2
    for a, (H, W) in enumerate(SIZES):
        for b, (pt, st) in enumerate(TEMPORAL):
            for i, Tx in enumerate(FRAMES):
                for j, Ty in enumerate(FRAMES):
                    d.Tx, d.Ty, d.H, d.W, d.pt, d.stridet = Tx, Ty, H, W, pt, st
                    out[a, b, i, j] = f(d)
    return out


def bind(lib):
    f = lib.vl3d_patchnn_scratch_bytes
    f.argtypes, f.restype = [C.POINTER(LossDesc)], C.c_int64
    return f


if __name__ == "__main__":
    np.savez_compressed(os.path.join(HERE, "patchnn_scratch_bytes.npz"), frames=np.array(FRAMES), sizes=np.array(SIZES),
                        temporal=np.array(TEMPORAL), bytes=sweep(bind(C.CDLL(sys.argv[1]))))
