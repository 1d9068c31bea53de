// What the two camera units share (csrc/vl3d_render_cam.hip: d loss / d homographies; csrc/vl3d_render_cam_normal.hip: the normal equations
// of a camera fit): the tile shape, the DPP sums over a row of 16 lanes, the slopes of the tent weights, the slot of walk_planes, and the
// descriptor rules of the entries -- one set of refusals for both.
#pragma once
#include <string>
#include "vl3d_render_args.h"

namespace vl3d_cam_detail {

using namespace vl3d_render_detail;

constexpr int CAM_TY = 4;            // 64 x 4 pixels per workgroup, one wave per row

// the sum over the wave's 64 lanes in every lane, a fixed order: within a row of 16 lanes by DPP (lane ^ 1, lane ^ 2 as quad permutations,
// then the mirrored half row and the mirrored row: after the quad sums every lane of a quad holds the same value, so the mirror image's is
// the other quad's), across the four rows by two cross-lane reads
__device__ __forceinline__ float cam_dpp_add(float v, int ctrl_sel) {
    const int i = __builtin_bit_cast(int, v);
    int o;
    switch (ctrl_sel) {
        case 0: o = __builtin_amdgcn_update_dpp(0, i, 0xB1, 0xf, 0xf, false); break;        // quad_perm [1, 0, 3, 2]
        case 1: o = __builtin_amdgcn_update_dpp(0, i, 0x4E, 0xf, 0xf, false); break;        // quad_perm [2, 3, 0, 1]
        case 2: o = __builtin_amdgcn_update_dpp(0, i, 0x141, 0xf, 0xf, false); break;       // row_half_mirror
        default: o = __builtin_amdgcn_update_dpp(0, i, 0x140, 0xf, 0xf, false); break;      // row_mirror
    }
    return v + __builtin_bit_cast(float, o);
}
__device__ __forceinline__ float cam_row_sum(float v) {      // the sum over the lane's row of 16 lanes, in each of them
    v = cam_dpp_add(v, 0); v = cam_dpp_add(v, 1); v = cam_dpp_add(v, 2); v = cam_dpp_add(v, 3);
    return v;
}
__device__ __forceinline__ float cam_wave_sum(float v) {
    v = cam_row_sum(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// derivative of the tent weights of the base tap (distance dl from the sample, dl = t - clamped floor) and of its right / lower neighbour
// with respect to the sample's coordinate, in the sample's cell [floor(t), floor(t) + 1).  A base clamped into [0, S - 2] is up to one
// texel away on either side: dl in [-1, 0) -- only the base tap is in reach, rising; [0, 1) -- the plain cell; [1, 2) -- only the
// neighbour is, falling.  `two`: the axis has a second tap (size > 1).
__device__ __forceinline__ void tent_slopes(float dl, bool two, float &d0, float &d1) {
    d0 = dl < 0.0f ? 1.0f : (dl < 1.0f ? -1.0f : 0.0f);
    d1 = (two && dl >= 0.0f) ? (dl < 1.0f ? 1.0f : (dl < 2.0f ? -1.0f : 0.0f)) : 0.0f;
}

struct CamSlot {
    Taps2 t;
    f4 v[4];
};

inline int unsupported(const char *who, const char *what) {
    vl3d_set_error((std::string(who) + ": " + what).c_str());
    return VL3D_EUNSUPPORTED;
}

inline bool aligned(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

inline int64_t cam_tiles(int32_t H, int32_t W) { return (int64_t)((W + 63) / 64) * ((H + CAM_TY - 1) / CAM_TY); }

// what vl3d_render_bwd_homos and vl3d_render_cam_normal refuse before they launch anything
inline int check_cam(const vl3d_render_desc *d, const uint8_t *quad_keep, int32_t QH, int32_t QW, const char *who) {
    VL3D_REQUIRE(d != nullptr, "null render desc");
    if (d->variant != 0) return refuse(who, "no kernel variants (desc->variant = 0)");
    if (!(d->D > 0 && d->T > 0 && d->Hs > 0 && d->Ws > 0 && d->H > 0 && d->W > 0)) return refuse(who, "non-positive render dims");
    if (d->D > 128) return refuse(who, "at most 128 planes");
    if (!(d->Hs < (1 << 24) && d->Ws < (1 << 24) && (int64_t)d->Hs * d->Ws * 16 < (1ll << 32))) return refuse(who, "frame too large for 32-bit byte offsets");
    if (cam_tiles(d->H, d->W) > 0x7fffffffll) return refuse(who, "tiles exceed the grid");
    if (!(d->rgb_act >= VL3D_ACT_NONE && d->rgb_act <= VL3D_ACT_ABS && d->alpha_act >= VL3D_ACT_NONE && d->alpha_act <= VL3D_ACT_ABS))
        return refuse(who, "rgb_act / alpha_act outside the activation table");
    if (d->stack_dtype != VL3D_F32) return unsupported(who, "fp32 stacks only");
    const bool planar = d->coord_mode == VL3D_COORD_AFFINE && d->border_mode == VL3D_BORDER_HARDCUT && d->act_order == VL3D_ACT_POST;
    const bool utils = d->coord_mode == VL3D_COORD_UTILS_MPI && d->border_mode == VL3D_BORDER_ZEROS && d->act_order == VL3D_ACT_PRE;
    if (!(planar || utils))
        return unsupported(who, "built for (affine, hardcut, post) -- the planar render -- and (utils_mpi, zeros, pre) -- the warp_homography chain -- only");
    if (d->uv_noise_seed != 0) return unsupported(who, "add_uv_noise is not built for the camera gradient (uv_noise_seed = 0)");
    if (quad_keep) {
        if (QH < 0 && QW < 0) return unsupported(who, "the tile-exact layout (a negative quad grid) is not built for the camera gradient");
        if (!(QH > 0 && QW > 0)) return refuse(who, "bad quad grid (both positive)");
        if (d->cull_row0 || d->cull_col0 || d->cull_Hs || d->cull_Ws) return unsupported(who, "the stack is the whole plane (desc->cull_* = 0)");
    }
    return VL3D_OK;
}

}  // namespace vl3d_cam_detail
