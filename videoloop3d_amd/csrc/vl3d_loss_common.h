// What the looping loss's translation units share (vl3d_loss.hip: the patch-NN search; vl3d_fold.hip: vote-fold and robust loss;
// vl3d_loop_prologue.hip): the descriptor check, the gram16 piece both writers of that form emit, the launch of a kernel with a large dynamic LDS.
#pragma once
#include "vl3d_common.h"
#include "vl3d_patchnn_choice.h"

static inline int check_loss(const vl3d_loss_desc *d) {
    VL3D_REQUIRE(d != nullptr, "null loss desc");
    if (vl3d_check_variant(d->variant) != VL3D_OK) return VL3D_EINVAL;
    VL3D_REQUIRE(d->Tx > 0 && d->Ty > 0 && d->H > 0 && d->W > 0, "loss: non-positive dims");
    VL3D_REQUIRE(d->ps > 0 && d->pt > 0 && d->stride > 0 && d->stridet > 0, "loss: non-positive patch config");
    VL3D_REQUIRE(d->H >= d->ps && d->W >= d->ps && d->Tx >= d->pt && d->Ty >= d->pt, "loss: input smaller than one patch");
    VL3D_REQUIRE((d->H - d->ps) % d->stride == 0 && (d->W - d->ps) % d->stride == 0 && (d->Tx - d->pt) % d->stridet == 0,
                 "loss: x is not trimmed to the patch grid (utils_vid.py:307-320)");
    return VL3D_OK;
}

// the gram16 form's 16-byte piece (layout: vl3d_loss.hip, patchnn6_k)
__device__ __forceinline__ uint4 gram16_piece(float a0, float a1, float a2, float s) {
    const float n = fmaf(a2, a2, fmaf(a1, a1, a0 * a0));
    const float u0 = a0 * s, u1 = a1 * s, u2 = a2 * s;
    const _Float16 h0 = (_Float16)u0, h1 = (_Float16)u1, h2 = (_Float16)u2, nh = (_Float16)n;
    const _Float16 l0 = (_Float16)(u0 - (float)h0), l1 = (_Float16)(u1 - (float)h1), l2 = (_Float16)(u2 - (float)h2), nl = (_Float16)(n - (float)nh);
    auto bits = [](_Float16 h) -> unsigned { return (unsigned)__builtin_bit_cast(unsigned short, h); };
    uint4 o;
    o.x = bits(h0) | (bits(h1) << 16);
    o.y = bits(l0) | (bits(l1) << 16);
    o.z = bits(h2) | (bits(l2) << 16);
    o.w = bits(nh) | (bits(nl) << 16);
    return o;
}

// launch a kernel that may ask for more than 64 KiB of dynamic LDS: it says so once per process, before its first launch
template <auto KERNEL, int CAP = 160 * 1024, typename... Args>
static int launch_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, Args... args) {
    static bool allowed = false;
    if (!allowed) {
        VL3D_HIP(hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, CAP));
        allowed = true;
    }
    hipLaunchKernelGGL(KERNEL, grid, block, lds, s, args...);
    return VL3D_OK;
}
