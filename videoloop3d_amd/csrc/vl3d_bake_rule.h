// THE bake rule (include/vl3d.h "Baked playback"; the reference's export, scripts/script_export_mesh.py:117-191, activates the atlases,
// multiplies by 255, clips and truncates to 8 bits) as ONE device function.  Two callers: bake_rgba8_k (csrc/vl3d_render_baked.hip), which
// writes the texels a viewer package ships, and the render core's VL3D_ACT_BAKED order (csrc/vl3d_render_core.h: shade2), which trains under
// the picture those texels show.  Because both call this text, a tap's byte in the training forward is the byte vl3d_bake_rgba8 writes for
// that texel, bit for bit -- a texel within an ulp of a byte boundary cannot round one way in the bake and the other way in the render.
#pragma once
#include "vl3d_common.h"

namespace {

__device__ __forceinline__ float act_rt(int act, float v) {      // (the activation is uniform: a scalar branch)
    switch (act) {
    case VL3D_ACT_SIGMOID: return act_fwd<VL3D_ACT_SIGMOID>(v);
    case VL3D_ACT_RELU: return act_fwd<VL3D_ACT_RELU>(v);
    case VL3D_ACT_CLAMP: return act_fwd<VL3D_ACT_CLAMP>(v);
    case VL3D_ACT_ABS: return act_fwd<VL3D_ACT_ABS>(v);
    default: return v;
    }
}
__device__ __forceinline__ unsigned bake_channel(float a) {      // trunc(clip(a * 255, 0, 255)); a NaN bakes to 0 (fmaxf returns the number)
    return (unsigned)fminf(fmaxf(a * 255.0f, 0.0f), 255.0f);
}

}  // namespace
