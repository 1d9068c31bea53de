"""Records tests/golden/bwd_scratch_bytes.npz: vl3d_render_bwd_scratch_bytes of a GIVEN build of the library over frames of 1..200 x 1..200
pixels -- D = 1 and 32 with the stack at the frame's size, D = 32 with a stack of (ceil(1.1 H), W + 3) texels.  The committed file was
recorded from the library built at the commit before the scratch layout was sized from the shape table (csrc/vl3d_render_bwd_choice.h), where
the window records were a maximum over a literal list of tile interiors: check that commit out into a directory of its own, build it there
(python -c "import __graft_entry__ as g; g.build()"), and run, from this tree,
    python tests/golden/make_bwd_scratch_bytes.py THAT_CHECKOUT/videoloop3d_amd/lib/libvl3d_hip.so
tests/test_bwd_choice_cpu.py::test_scratch_bytes_are_what_they_were compares the current library with the file.  No GPU is touched."""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from videoloop3d_amd._lib import RenderDesc  # noqa: E402


def main(lib_path):
    f = C.CDLL(lib_path).vl3d_render_bwd_scratch_bytes
    f.argtypes, f.restype = [C.POINTER(RenderDesc)], C.c_int64
    Ds = [1, 32]
    same = np.zeros((len(Ds), 200, 200), dtype=np.int32)
    larger = np.zeros((200, 200), dtype=np.int32)
    d = RenderDesc()
    d.T = 1
    for i, D in enumerate(Ds):
        for H in range(1, 201):
            for W in range(1, 201):
                d.D, d.H, d.W, d.Hs, d.Ws = D, H, W, H, W
                same[i, H - 1, W - 1] = f(d)
                if D == 32:
                    d.Hs, d.Ws = (H * 11 + 9) // 10, W + 3
                    larger[H - 1, W - 1] = f(d)
    np.savez_compressed(os.path.join(HERE, "bwd_scratch_bytes.npz"), D=np.array(Ds), stack_is_frame=same, stack_larger=larger)


if __name__ == "__main__":
    main(sys.argv[1])
