// One sampling / compositing convention of the fused render = one translation unit (the stubs vl3d_render_c*.hip define
//   VL3D_CONV_FN      name of the entry point (declared in vl3d_render_core.h)
//   VL3D_CONV_COORD / VL3D_CONV_BORDER / VL3D_CONV_ORDER   the compile-time convention
//   VL3D_CONV_ACTS    0: (sigmoid, sigmoid) only -- the shipped activations (configs/mpv_base.txt:29-30), fp32 and fp16 stacks
//                     1: the pre-activated / rgb-linear pairs as well: (none, none), (none, sigmoid)
//                     2: every pair of the product's table EXCEPT (sigmoid, sigmoid)
// and include this file), so the conventions compile in parallel and the library only carries the instantiations a caller
// can reach.  Activation table: MPI.py:21-31, product subset in videoloop3d_amd/MPV.py:ACTIVATES.
#include "vl3d_render_core.h"

namespace vl3d_render_detail {

int VL3D_CONV_FN(bool bwd, const vl3d_render_desc *d, const RenderArgs &a, hipStream_t s) {
#define VL3D_CASE(R, A)                                                                                     \
    if (d->rgb_act == R && d->alpha_act == A) {                                                             \
        if (bwd) return launch<true, VL3D_CONV_COORD, VL3D_CONV_BORDER, VL3D_CONV_ORDER, R, A>(a, s);       \
        return launch<false, VL3D_CONV_COORD, VL3D_CONV_BORDER, VL3D_CONV_ORDER, R, A>(a, s);               \
    }
#if VL3D_CONV_ACTS != 2
    VL3D_CASE(VL3D_ACT_SIGMOID, VL3D_ACT_SIGMOID)
#endif
#if VL3D_CONV_ACTS >= 1
    VL3D_CASE(VL3D_ACT_NONE, VL3D_ACT_NONE)
    VL3D_CASE(VL3D_ACT_NONE, VL3D_ACT_SIGMOID)
#endif
#if VL3D_CONV_ACTS == 2
    VL3D_CASE(VL3D_ACT_CLAMP, VL3D_ACT_SIGMOID)
    VL3D_CASE(VL3D_ACT_RELU, VL3D_ACT_SIGMOID)
    VL3D_CASE(VL3D_ACT_ABS, VL3D_ACT_SIGMOID)
    VL3D_CASE(VL3D_ACT_CLAMP, VL3D_ACT_CLAMP)
    VL3D_CASE(VL3D_ACT_SIGMOID, VL3D_ACT_CLAMP)
    VL3D_CASE(VL3D_ACT_NONE, VL3D_ACT_CLAMP)
#endif
#undef VL3D_CASE
    vl3d_set_error("unsupported (rgb_act, alpha_act) pair for this (coord_mode, border_mode, act_order)");
    return VL3D_EUNSUPPORTED;
}

}  // namespace vl3d_render_detail
