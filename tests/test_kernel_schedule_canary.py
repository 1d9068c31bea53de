"""A tripwire, not a parity test: the register count hipcc gives the headline backward kernel.

Round 5 (docs/kernels/K2_render_backward.md, "A kernel-argument layout regression"): one more integer in `RenderArgs`, in front of the other
fields, changed NOTHING in the source of `render_bwd_pair_k` -- and hipcc compiled it to a different schedule (73 instead of 82 VGPRs, fewer
tap loads in flight) that measured 13.4-14.2 against 12.3-12.5 ms at cfg3.  The compiler's schedule of this kernel is sensitive to inputs
that have nothing to do with it, so a change of its register count is the cheapest signal that the schedule moved: when this test fails,
A/B the build against the previous one (profiles/r05d_ab_lib.sh) before updating the number."""
import os
import shutil

import pytest

from pair_kernel_resources import HIPCC, SHAPE_32X16, pair_kernels


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_headline_backward_keeps_its_schedule():
    # the plain fp32 frame-pair backward of the shipped planar convention in 32 x 16 regions, with the owner table:
    # render_bwd_pair_k<1,1,1,1,1,false,false,false,BWD_32X16,false>
    name = ("_ZN12_GLOBAL__N_117render_bwd_pair_kILi1ELi1ELi1ELi1ELi1ELb0ELb0ELb0ELN18vl3d_render_detail8BwdShapeE2ELb0EEEvNS1_10RenderArgsE")
    mine = [k for k in pair_kernels("vl3d_render_c3_mpv_sig.hip") if k.name == name]
    assert mine, "the frame-pair backward is no longer instantiated under this name (update the tripwire)"
    assert (mine[0].conv, mine[0].f16, mine[0].reg, mine[0].adam, mine[0].shape, mine[0].ownerless) == ((1, 1, 1, 1, 1), False, False, False, SHAPE_32X16, False)
    vgprs, scratch = mine[0].vgprs, mine[0].scratch
    assert scratch == 0
    assert vgprs == 82, (f"render_bwd_pair_k now takes {vgprs} VGPRs (82 when it measured 11.7-12.5 ms at cfg3): its schedule moved -- "
                         "A/B this build against the previous one (profiles/r05d_ab_lib.sh) before accepting the new number")
