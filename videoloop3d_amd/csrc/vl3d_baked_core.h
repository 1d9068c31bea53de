// What the two baked forwards share (csrc/vl3d_render_baked.hip: a dense uint8 clip; csrc/vl3d_render_baked_pool.hip: the pool of 8 x 8-texel
// blocks behind the block table).  The two kernels must produce the same bits from the same texels, so everything behind the fetch lives here
// once: the taps as two 8-byte words, the decode (a channel is a byte of the texel word), the blend (one fmaf chain associated like shade2),
// the composite state of one frame or a frame pair with its step, and the pixel store.  Each unit keeps its fetch, its kernel skeleton and
// its entry point; the plane list of a tile-culled model is PlaneList of vl3d_render_core.h, as in the float forward.
#pragma once
#include <type_traits>
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

// A camera path (vl3d_render_fwd_baked_path / _pool_path): output frame i of the launch has its own camera frame_cam[i] and its own frame
// frame_t[i] of the clip, both device int32[N].  NoPath: the kernels' one-camera form, (frame, camera) from the block index and the launch
// arguments -- an empty argument, so that the two forms are one kernel text.
struct NoPath {};
struct PathIdx {
    const int *frame_cam, *frame_t;
    int n_cams, n_t;      // cameras of the homographies / masks, frames of the clip (T_alloc; T_model of a pool)
};
// (cam, t) of output frame i as workgroup-uniform scalar loads; false -- the workgroup returns before any other load or store -- unless
// cam is in [0, n_cams) and t in [0, n_t): no index read from device memory ever forms an address outside the clip, the pool or the masks
__device__ __forceinline__ bool path_frame(const PathIdx &p, int i, int &cam, int &t) {
    cam = ((cint_p)p.frame_cam)[i];
    t = ((cint_p)p.frame_t)[i];
    return (unsigned)cam < (unsigned)p.n_cams && (unsigned)t < (unsigned)p.n_t;
}

// Front-to-back composite of a pixel's NF frames (one, or a frame pair) over the kernel's own accumulators: transmittance, colour and alpha
// per frame, five plain arrays the kernel declares and clears (T = 1, the rest 0) and this struct steps and stores -- a by-reference closure
// with a name.  OWNER is a type local to the kernel that uses it: like the lambda it replaces, every kernel instantiation gets a copy of its
// own.  Both choices are the register table's (docs/kernels/K9_baked_playback.md "The shared core"): two dense kernels sharing one
// instantiation cost the one-frame kernel 2 VGPRs, the accumulators as members of one struct (or cleared in here) the frame-pair kernel 6.
template <int NF, typename OWNER>
struct BakedComposite {
    static_assert(NF == 1 || NF == 2, "one frame or a frame pair per thread");
    float (&Tr)[NF], (&cr)[NF], (&cg)[NF], (&cb)[NF], (&A)[NF];
    __device__ __forceinline__ BakedComposite(float (&Tr_)[NF], float (&cr_)[NF], float (&cg_)[NF], float (&cb_)[NF], float (&A_)[NF])
        : Tr(Tr_), cr(cr_), cg(cg_), cb(cb_), A(A_) {}
    // one plane: t = the sample's tent weights and coverage (Taps2 / TapsI), v[f] = the taps of frame f.
    // The fused multiply-adds are spelt out and nothing else may be contracted: left to -ffp-contract=fast, hipcc fuses cb += w * c in the
    // frame-pair kernel and not in the one-frame kernel (where it packs the add with A += w instead), and a frame would depend, in its last
    // bit, on the length of the run it is rendered in.
    template <typename TAPS>
    __device__ __forceinline__ void operator()(const TAPS &t, const BakedTaps *v) const {
#pragma clang fp contract(off)
        const f4 w255 = t.w * (1.0f / 255.0f);      // the decode's 1 / 255, once per plane for every channel and frame
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const float al = blend<3>(v[f], w255) * t.cov;      // uncovered: a = 0 -> the plane drops out of the composite
            const float w = al * Tr[f];
            cr[f] = fmaf(w, blend<0>(v[f], w255), cr[f]); cg[f] = fmaf(w, blend<1>(v[f], w255), cg[f]); cb[f] = fmaf(w, blend<2>(v[f], w255), cb[f]);
            A[f] += w;
            Tr[f] *= (1.0f - al);
        }
    }
    // pixel (x, y) of frame t0, then of frame t0 + 1 under has1 (odd T: the last pair composites frame t0 twice and stores it once)
    __device__ __forceinline__ void store(const RenderArgs &a, int t0, int x, int y, bool has1) const {
        size_t pix = ((size_t)t0 * a.H + y) * a.W + x;
        a.rgb[pix * 3 + 0] = cr[0]; a.rgb[pix * 3 + 1] = cg[0]; a.rgb[pix * 3 + 2] = cb[0];
        a.alpha[pix] = A[0];
        if constexpr (NF == 2) {
            if (has1) {
                pix += (size_t)a.H * a.W;
                a.rgb[pix * 3 + 0] = cr[1]; a.rgb[pix * 3 + 1] = cg[1]; a.rgb[pix * 3 + 2] = cb[1];
                a.alpha[pix] = A[1];
            }
        }
    }
};

}  // namespace
