// Decode and blend of baked RGBA8 taps, shared by the two baked forwards (csrc/vl3d_render_baked.hip: a dense uint8 clip;
// csrc/vl3d_render_baked_pool.hip: the pool of 8 x 8-texel blocks behind the block table).  The two kernels must produce the same bits from
// the same texels, so the instruction sequence behind the taps lives here once: a channel is a byte of the texel word, the blend is one
// fmaf chain associated like shade2.  (The composite is a lambda over each kernel's own accumulators, spelt identically in both units.)
#pragma once
#include "vl3d_render_core.h"

namespace {

typedef unsigned u2w __attribute__((ext_vector_type(2)));
typedef u2w u2w_a4 __attribute__((aligned(4)));      // two 4-byte texels of a row: 4-byte aligned (x0 may be odd)

// the four taps of a sample: texels (x0, x0 + 1) of rows y0 and y0 + 1, one 8-byte load per row against a uniform plane base
struct BakedTaps { u2w r0, r1; };
template <int K>
__device__ __forceinline__ float chan(unsigned w) { return (float)((w >> (8 * K)) & 0xffu); }
// bilinear blend of the decoded taps; w255 = the tent weights * (1 / 255).  Associated like shade2: tap 3 first, then 2, 1, 0.
template <int K>
__device__ __forceinline__ float blend(const BakedTaps &v, f4 w255) {
    return fmaf(chan<K>(v.r0.x), w255[0], fmaf(chan<K>(v.r0.y), w255[1], fmaf(chan<K>(v.r1.x), w255[2], chan<K>(v.r1.y) * w255[3])));
}

}  // namespace
