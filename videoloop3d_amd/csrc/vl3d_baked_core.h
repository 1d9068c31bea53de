// What the two baked forwards share (csrc/vl3d_render_baked.hip: a dense uint8 clip; csrc/vl3d_render_baked_pool.hip: the pool of 8 x 8-texel
// blocks behind the block table).  The two kernels must produce the same bits from the same texels, so everything behind the fetch lives here
// once: the taps as two 8-byte words, the decode (a channel is a byte of the texel word), the blend (one fmaf chain associated like shade2),
// the composite state of one frame or a frame pair with its step, and the pixel store.  Each unit keeps its fetch, its kernel skeleton and
// its entry point; the plane list of a tile-culled model is PlaneList of vl3d_render_core.h, as in the float forward.
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
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

// A camera path (the path selection of vl3d_render_fwd_baked / _pool): output frame i of the launch has its own camera frame_cam[i] and its own frame
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

// A camera path in LOOP TIME (vl3d_baked_times: vl3d_render_fwd_baked_times / _pool_times): output frame i shows the model at the real-valued time
// frame_time[i] in [0, n_t), device float[N] -- the linear interpolation of its texels between frame t0 = floor(time) and frame t1 = t0 + 1,
// which wraps to 0 at the loop seam, with f = time - t0 (exact in fp32).  One output frame per thread, TWO source frames.
struct PathTime {
    const int *frame_cam;
    const float *frame_time;
    int n_cams, n_t;
};
// (cam, t0, t1, f) of output frame i as two workgroup-uniform scalar loads; false -- the workgroup returns before any other load or store --
// unless cam is in [0, n_cams) and the time in [0, n_t).  A NaN fails both comparisons.  The conversion comes after the check, and t0 < n_t
// is checked once more as an integer (n_t >= 2^24 is not a float): t0 and t1 are frames of the model whatever device memory holds.
__device__ __forceinline__ bool path_frame(const PathTime &p, int i, int &cam, int &t0, int &t1, float &f) {
    cam = ((cint_p)p.frame_cam)[i];
    const float time = ((cfloat_p)p.frame_time)[i];
    if (!((unsigned)cam < (unsigned)p.n_cams && time >= 0.0f && time < (float)p.n_t)) return false;
    t0 = (int)time;
    if (!((unsigned)t0 < (unsigned)p.n_t)) return false;
    t1 = t0 + 1 < p.n_t ? t0 + 1 : 0;
    f = time - (float)t0;
    return true;
}
// frames a thread composites (NF) and source frames whose taps it fetches: NF, but two for the one output frame of a loop-time path
template <int NF, typename PATH>
constexpr int baked_sources() { return std::is_same<PATH, PathTime>::value ? 2 : NF; }

// Where a composited pixel goes.  FloatOut: a.rgb / a.alpha, fp32 -- an empty argument, so that the two sinks are one kernel text (as NoPath
// beside PathIdx).  DisplayOut (the display sink, vl3d_baked_out.frames): the frame a viewer shows, frames (N,H,W,channels) uint8, over the background
// bg when has_bg; pack3: the lane-packed RGB8 store instead of three byte stores per lane.  bg travels in the kernel arguments.
struct FloatOut {};
struct DisplayOut {
    uint8_t *frames;
    float bg[3];
    int has_bg, channels, pack3;
};
// What the display sink adds to the float sink's refusals (`who` in front of the message), and the sink itself.  bg: a HOST pointer to 3
// floats or null, read here -- no device read for it.  The RGB8 store is the lane-packed one; VL3D_DISPLAY_STORE3=bytes is the measurement
// hook of profiles/baked_fwd.py --legs display for the byte stores (read per call: the legs alternate inside one process).
inline int display_out_of(uint8_t *frames, int32_t channels, const float *bg, const char *who, DisplayOut &out) {
    const char *bad = nullptr;
    if (channels != 3 && channels != 4) bad = "channels must be 3 (RGB8) or 4 (RGBA8)";
    else if (!frames) bad = "null pointer (frames)";
    else if (channels == 4 && ((uintptr_t)frames & 3) != 0) bad = "RGBA8 frames must be 4-byte aligned";
    else if (bg && !(std::isfinite(bg[0]) && std::isfinite(bg[1]) && std::isfinite(bg[2]))) bad = "the background colour must be finite";
    if (bad) {
        vl3d_set_error((std::string(who) + ": " + bad).c_str());
        return VL3D_EINVAL;
    }
    const char *store3 = std::getenv("VL3D_DISPLAY_STORE3");
    out = DisplayOut{frames, {bg ? bg[0] : 0.0f, bg ? bg[1] : 0.0f, bg ? bg[2] : 0.0f}, bg != nullptr, channels,
                     !(store3 && std::strcmp(store3, "bytes") == 0)};
    return VL3D_OK;
}
// to8b of the reference's utils.py, (255 * clip(x, 0, 1)).astype(uint8): every operation rounded on its own, the conversion truncates
__device__ __forceinline__ unsigned display_byte(float x) {
#pragma clang fp contract(off)
    return (unsigned)(255.0f * fminf(fmaxf(x, 0.0f), 1.0f));
}
// the display rule of one pixel -> r | g << 8 | b << 16 | a << 24.  Over a background (MPV.py:455-461) x = c * A + bg * (-A + 1) in torch's
// order -- two products, the complement and one sum, none fused -- so that the bytes equal to8b of the float render's; the alpha byte is
// never composited.
__device__ __forceinline__ unsigned display_word(const DisplayOut &o, float r, float g, float b, float A) {
#pragma clang fp contract(off)
    if (o.has_bg) {
        const float om = (-A) + 1.0f;
        const float r1 = r * A, g1 = g * A, b1 = b * A;
        const float r2 = o.bg[0] * om, g2 = o.bg[1] * om, b2 = o.bg[2] * om;
        r = r1 + r2; g = g1 + g2; b = b1 + b2;
    }
    return display_byte(r) | display_byte(g) << 8 | display_byte(b) << 16 | display_byte(A) << 24;
}
// pixel `pix` (of N * H * W) of the display frames; x0w: the first column of the wave's 64-pixel row segment, W the row length.
// channels == 4: one aligned dword per lane.  channels == 3: three byte stores per lane, or (pack3) the wave's 192 contiguous bytes as 48
// dwords -- dword j = 3 q + m holds bytes of pixels 4 q + m and 4 q + m + 1, fetched from their lanes by two cross-lane reads -- when the
// segment is a full 64 pixels and starts 4-byte aligned: a wave-uniform condition under which every lane of the wave is here (no lane left
// at the x >= W return), so the cross-lane reads see live lanes; otherwise the byte stores.
__device__ __forceinline__ void display_store(const DisplayOut &o, size_t pix, int x0w, int W, unsigned w) {
    if (o.channels == 4) {
        reinterpret_cast<unsigned *>(o.frames)[pix] = w;
        return;
    }
    uint8_t *p = o.frames + pix * 3;
    if (o.pack3) {
        const int lane = (int)(threadIdx.x & 63);
        uint8_t *seg = p - (size_t)lane * 3;      // the wave's first byte: the same address in every lane
        const int fast = __builtin_amdgcn_readfirstlane((int)(x0w + 64 <= W && ((uintptr_t)seg & 3) == 0));
        if (fast) {
            const int q = lane / 3, m = lane - q * 3;      // (lanes 48 .. 63 read lanes they do not need and store nothing)
            const unsigned wa = (unsigned)__shfl((int)w, (4 * q + m) & 63), wb = (unsigned)__shfl((int)w, (4 * q + m + 1) & 63);
            if (lane < 48) reinterpret_cast<unsigned *>(seg)[lane] = ((wa & 0xffffffu) >> (8 * m)) | (wb << (24 - 8 * m));
            return;
        }
    }
    p[0] = (uint8_t)w; p[1] = (uint8_t)(w >> 8); p[2] = (uint8_t)(w >> 16);
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
    // one plane at a fractional loop time (PathTime): v[0], v[1] = the taps of frames t0 and t1, fr = time - t0.  Every channel, alpha
    // included, is c = fmaf(fr, b1 - b0, b0) of the two frames' blends, and c takes the place of the blend in the one-frame step above --
    // the same five statements, repeated here and not factored out: a helper both operators call moves the one-frame kernels' registers
    // (the register table, docs/kernels/K9_baked_playback.md).  Exact consequences: fr == 0 gives the bits of b0 (the product is a zero, b0
    // is never -0), equal taps give b1 - b0 = 0 and the bits of b0 at any fr.
    template <typename TAPS>
    __device__ __forceinline__ void operator()(const TAPS &t, const BakedTaps *v, float fr) const {
#pragma clang fp contract(off)
        static_assert(NF == 1, "a loop-time path renders one output frame per thread");
        const f4 w255 = t.w * (1.0f / 255.0f);
        const auto c = [&](auto k) {
#pragma clang fp contract(off)
            const float b0 = blend<decltype(k)::value>(v[0], w255), b1 = blend<decltype(k)::value>(v[1], w255);
            return fmaf(fr, b1 - b0, b0);
        };
        const float al = c(std::integral_constant<int, 3>{}) * t.cov;
        const float w = al * Tr[0];
        cr[0] = fmaf(w, c(std::integral_constant<int, 0>{}), cr[0]);
        cg[0] = fmaf(w, c(std::integral_constant<int, 1>{}), cg[0]);
        cb[0] = fmaf(w, c(std::integral_constant<int, 2>{}), cb[0]);
        A[0] += w;
        Tr[0] *= (1.0f - al);
    }
    // pixel (x, y) of frame t0, then of frame t0 + 1 under has1 (odd T: the last pair composites frame t0 twice and stores it once)
    __device__ __forceinline__ void store(const RenderArgs &a, const DisplayOut &o, int t0, int x, int y, bool has1) const {
        const size_t pix = ((size_t)t0 * a.H + y) * a.W + x;
        const int x0w = x - (int)(threadIdx.x & 63);
        display_store(o, pix, x0w, a.W, display_word(o, cr[0], cg[0], cb[0], A[0]));
        if constexpr (NF == 2) {
            if (has1) display_store(o, pix + (size_t)a.H * a.W, x0w, a.W, display_word(o, cr[1], cg[1], cb[1], A[1]));
        }
    }
    __device__ __forceinline__ void store(const RenderArgs &a, const FloatOut &, int t0, int x, int y, bool has1) const {
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

// The composite of a loop-time kernel: the one-frame composite with the fraction bound, so that the dense kernel's call composite(t, v)
// is one text for every PATH (a wrapper lambda around the two operators moves the one-frame kernels' registers).
template <typename OWNER>
struct BakedCompositeAt : BakedComposite<1, OWNER> {
    float fr = 0.0f;      // time - t0, set by the kernel once path_frame has given it
    using BakedComposite<1, OWNER>::BakedComposite;
    template <typename TAPS>
    __device__ __forceinline__ void operator()(const TAPS &t, const BakedTaps *v) const { BakedComposite<1, OWNER>::operator()(t, v, fr); }
};

}  // namespace
