// Disparity maps from the render kernels (include/vl3d.h "Disparity"): the blend-weighted inverse view depth the reference hands back beside
// the picture (MPV.py:385, 463-466, MPI.py:493-494, 563-566: variables['disp_norm']), from the float clip, the baked clip and the baked pool.
//
// For planar geometry the inverse view depth of plane k under an output pixel is affine in the pixel, rho_k = row_k . (x + c, y + c, 1), with
// row_k formed on the host (render.depth_rows), so a kernel needs the alpha of each plane, three floats per plane and one more accumulator:
//     disp = sum_k w_k rho_k,   alpha = sum_k w_k,   w_k = a_k prod_{j<k} (1 - a_j)
// Three kernels, forward only, each the skeleton of its colour twin -- 64 x 8 pixels per workgroup (one wave per 64-pixel row segment), XCD
// remap, the next plane's taps in flight while the current plane is composited (two register sets), the plane list of a tile-culled model --
// with ONE output pixel and ONE frame per thread:
//   * render_disp_fwd_k: a float clip (fp32 / fp16) read in place.  Per tap only the alpha lane is loaded (4 or 2 bytes of the 16- or 8-byte
//     texel); the logits are blended (the chain of shade2: tap 3 first), activated, times coverage.
//   * render_disp_baked_k: a baked RGBA8 clip, a run or a camera path.  The taps are the colour kernel's two 8-byte loads per sample (the
//     same texel lines), alpha = blend<3> of vl3d_baked_core.h.
//   * render_disp_baked_pool_k: the baked pool behind its block table; the fetch of csrc/vl3d_render_baked_pool.hip for one frame.
// Sample position, hard cut, kept-quad test, tile-exact quad offset and tent weights are make_taps2 / make_taps_i / plane_cull of
// vl3d_render_core.h, called with the colour kernels' arguments: colour and depth agree on every pixel's coverage.  The composite step is
// DispComposite below, held under fp contract(off) with its one fused multiply-add spelt out; its alpha statements are BakedComposite's, so
// the alpha of a baked source has the bits of the colour entry's float sink.
// No LDS, no scratch memory.  Bounds: a thread returns unless x < W and y < H, and stores at pixel (t * H + y) * W + x < N * H * W of disp
// (and alpha), 64-bit; a path workgroup whose camera or frame is out of range returns before any load or store (path_frame).
#include "vl3d_bake_rule.h"      // act_rt
#include "vl3d_baked_core.h"     // taps, decode, blend, the path selection: shared with the two baked colour units
#include "vl3d_render_args.h"

using namespace vl3d_render_detail;

namespace {

// what the disparity kernels take beside RenderArgs (whose rgb / alpha are not read): the affine rows, the two outputs, the activation
struct DispArgs {
    const float *rows;      // (D, 3); a path: (n_cams, D, 3)
    float *disp, *alpha;    // (N, H, W); alpha may be null
    int alpha_act;          // the float entry only
};

__device__ __forceinline__ float plane_rho(const float *rows, int d, float px, float py) {
    float r[3];
    load_uniform(rows + 3 * d, r);      // scalar loads, as the homographies
    return fmaf(r[0], px, fmaf(r[1], py, r[2]));
}

// Front-to-back composite of one pixel of one frame: transmittance, alpha and disparity.  Nothing may be contracted but the fmaf spelt out:
// the statements on Tr and A are BakedComposite's (vl3d_baked_core.h) and must give its bits.
struct DispComposite {
    float Tr = 1.0f, A = 0.0f, Dp = 0.0f;
    __device__ __forceinline__ void step(float al, float rho) {
#pragma clang fp contract(off)
        const float w = al * Tr;
        Dp = fmaf(w, rho, Dp);
        A += w;
        Tr *= (1.0f - al);
    }
    // a baked sample: the bilinear blend of the decoded alpha bytes, no activation (the 1 / 255 folded into the weights once per plane)
    template <typename TAPS>
    __device__ __forceinline__ void baked(const TAPS &t, const BakedTaps &v, float rho) {
#pragma clang fp contract(off)
        const f4 w255 = t.w * (1.0f / 255.0f);
        const float al = blend<3>(v, w255) * t.cov;      // uncovered: a = 0 -> the plane drops out of the composite
        step(al, rho);
    }
    // a float sample: the four alpha logits blended (associated like shade2: tap 3 first), activated, times coverage
    template <typename V>
    __device__ __forceinline__ void logits(const Taps2 &t, const V (&v)[4], int act, float rho) {
#pragma clang fp contract(off)
        const float s = fmaf((float)v[0], t.w[0], fmaf((float)v[1], t.w[1], fmaf((float)v[2], t.w[2], (float)v[3] * t.w[3])));
        const float al = act_rt(act, s) * t.cov;
        step(al, rho);
    }
    __device__ __forceinline__ void store(const RenderArgs &a, const DispArgs &o, int t, int x, int y) const {
        const size_t pix = ((size_t)t * a.H + y) * a.W + x;
        o.disp[pix] = Dp;
        if (o.alpha) o.alpha[pix] = A;
    }
};

// ---- the float clip -----------------------------------------------------------------------------------------------------------------------
// the alpha lanes of a sample's four taps: one lane offset, four uniform bases (load_taps2 of the colour forward, 4 or 2 bytes per tap)
template <bool F16>
struct AlphaLane { typedef float type; };
template <>
struct AlphaLane<true> { typedef _Float16 type; };

template <bool F16>
__device__ __forceinline__ void load_alpha_taps(const char *__restrict__ plane, const Taps2 &t, TapStep st, typename AlphaLane<F16>::type (&v)[4]) {
    typedef typename AlphaLane<F16>::type lane_t;
    const size_t o = F16 ? (size_t)(t.off >> 1) + 6 : (size_t)t.off + 12;      // the fourth lane of the texel
    v[0] = *reinterpret_cast<const lane_t *>(plane + o);
    v[1] = *reinterpret_cast<const lane_t *>(plane + st.dx + o);
    v[2] = *reinterpret_cast<const lane_t *>(plane + st.dy + o);
    v[3] = *reinterpret_cast<const lane_t *>(plane + st.dy + st.dx + o);
}

template <bool F16, bool CULL>
__global__ __launch_bounds__(512) void render_disp_fwd_k(RenderArgs a, DispArgs o, int tiles_x, int tiles_y) {
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, rest = b / tiles_x;
    const int tile_y = rest % tiles_y, t = rest / tiles_y;
    const int x = tile_x * 64 + (threadIdx.x & 63);
    const int y = tile_y * 8 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const size_t frame_b = (size_t)a.Hs * a.Ws * (F16 ? 8 : 16);
    const size_t plane_stride_b = (size_t)a.Tstride * frame_b;
    const char *plane = reinterpret_cast<const char *>(a.stack) + (size_t)t * frame_b;
    const TapStep st = make_tap_step<F16>(a.Hs, a.Ws);
    typedef typename AlphaLane<F16>::type lane_t;
    struct Slot {
        Taps2 t;
        lane_t v[4];
        float rho;
    } sA, sB;
    DispComposite c;
    auto fetch = [&](int d, Slot &s) {
        Taps2 &tp = s.t;
        float h[VL3D_HN];
        load_uniform(a.homos + VL3D_HS * d, h);
        if constexpr (CULL) tp = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy, plane_cull(a, d));
        else tp = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy);
        s.rho = plane_rho(o.rows, d, px, py);
        load_alpha_taps<F16>(plane + (size_t)d * plane_stride_b, tp, st, s.v);
        asm volatile("" ::: "memory");      // keep the loads here: hipcc otherwise sinks them below the composite
    };
    auto step = [&](const Slot &s, int) { c.logits(s.t, s.v, o.alpha_act, s.rho); };
    // the workgroup's plane list (cull_fwd_plan_k; a pixel inside a culled quad is uncovered, make_taps2) or every plane: the colour forward's
    // walk (walk_planes, vl3d_render_core.h)
    if constexpr (CULL) walk_planes(ListedPlanes(a.cull_masks, tile_y * tiles_x + tile_x), sA, sB, fetch, step);
    else walk_planes(DensePlanes{a.D}, sA, sB, fetch, step);
    c.store(a, o, t, x, y);
}

// ---- the baked clip -----------------------------------------------------------------------------------------------------------------------
// the taps of a dense clip: one 8-byte load per texel row against a uniform plane base (the colour kernel's fetch)
__device__ __forceinline__ BakedTaps load_baked(const char *__restrict__ plane, const Taps2 &t, unsigned row_b) {
    const size_t o = (size_t)(t.off >> 2);      // make_taps2 gives the byte offset of 16-byte texels
    return BakedTaps{*reinterpret_cast<const u2w_a4 *>(plane + o), *reinterpret_cast<const u2w_a4 *>(plane + row_b + o)};
}

// PATH = NoPath: frame t0 of the run a.stack starts at, one camera.  PATH = PathIdx: the block index's outermost factor is the OUTPUT frame;
// the workgroup reads its camera and its frame of the clip (path_frame: scalar loads, range-checked) and from them forms its homographies,
// rows, masks and texel base.
template <bool CULL, typename PATH>
__global__ __launch_bounds__(512) void render_disp_baked_k(RenderArgs a, DispArgs o, int tiles_x, int tiles_y, PATH path) {
    constexpr bool IS_PATH = !std::is_same<PATH, NoPath>::value;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, rest = b / tiles_x;
    const int tile_y = rest % tiles_y, t0 = rest / tiles_y;      // (a path: the output frame)
    int tile = tile_y * tiles_x + tile_x, src_t = t0;
    const float *homos = a.homos, *rows = o.rows;
    if constexpr (IS_PATH) {
        int cam;
        if (!path_frame(path, t0, cam, src_t)) return;      // uniform: nothing loaded, nothing stored
        homos += (size_t)cam * a.D * VL3D_HS;
        rows += (size_t)cam * a.D * 3;
        tile += cam * tiles_x * tiles_y;
    }
    const int x = tile_x * 64 + (threadIdx.x & 63);
    const int y = tile_y * 8 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const unsigned row_b = (unsigned)a.Ws * 4u;
    const size_t frame_b = (size_t)a.Hs * a.Ws * 4;
    const size_t plane_stride_b = (size_t)a.Tstride * frame_b;
    const char *base = reinterpret_cast<const char *>(a.stack) + (size_t)src_t * frame_b;
    struct Slot {
        Taps2 t;
        BakedTaps v;
        float rho;
    } sA, sB;
    DispComposite c;
    auto fetch = [&](int d, Slot &s) {
        Taps2 &tp = s.t;
        float h[VL3D_HN];
        load_uniform(homos + VL3D_HS * d, h);
        if constexpr (CULL) tp = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy, plane_cull(a, d));
        else tp = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy);
        s.rho = plane_rho(rows, d, px, py);
        s.v = load_baked(base + (size_t)d * plane_stride_b, tp, row_b);
        asm volatile("" ::: "memory");      // keep the loads here: hipcc otherwise sinks them below the composite
    };
    auto step = [&](const Slot &s, int) { c.baked(s.t, s.v, s.rho); };
    if constexpr (CULL) walk_planes(ListedPlanes(a.cull_masks, tile), sA, sB, fetch, step);
    else walk_planes(DensePlanes{a.D}, sA, sB, fetch, step);
    c.store(a, o, t0, x, y);
}

// ---- the baked pool -----------------------------------------------------------------------------------------------------------------------
constexpr int TSB = 8;                           // block side (vl3d_adam_window_tile())
constexpr unsigned SLOT_B = TSB * TSB * 4;       // bytes of a slot: 64 RGBA8 texels

struct PoolSrc {
    const int *blocks;           // [D][tiles_y][tiles_x]
    const char *pool;            // n_slots * SLOT_B bytes
    int tiles_y, tiles_x;
    int frame0;                  // first frame of the run, in the model's T frames
    unsigned culled;             // the texel a block without storage reads as
};

// one texel load behind a table entry, issued only under `e >= 0`: a block without storage is never dereferenced, its texels are `fill`
template <typename L, typename V>
__device__ __forceinline__ V pool_load(const PoolSrc &p, int e, unsigned in_b, size_t frame_b, V fill) {
    if (e < 0) return fill;
    return *reinterpret_cast<const L *>(p.pool + (size_t)(e >> 1) * SLOT_B + in_b + ((e & 1) ? frame_b : 0));
}

template <typename PATH>
__global__ __launch_bounds__(512) void render_disp_baked_pool_k(RenderArgs a, DispArgs o, PoolSrc p, int tiles_x, int tiles_y, PATH path) {
    constexpr bool IS_PATH = !std::is_same<PATH, NoPath>::value;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, rest = b / tiles_x;
    const int tile_y = rest % tiles_y, t0 = rest / tiles_y;      // (a path: the output frame)
    int tile = tile_y * tiles_x + tile_x, src_t = p.frame0 + t0;
    const float *homos = a.homos, *rows = o.rows;
    if constexpr (IS_PATH) {
        int cam;
        if (!path_frame(path, t0, cam, src_t)) return;      // uniform: nothing loaded, nothing stored
        homos += (size_t)cam * a.D * VL3D_HS;
        rows += (size_t)cam * a.D * 3;
        tile += cam * tiles_x * tiles_y;
    }
    const int x = tile_x * 64 + (threadIdx.x & 63);
    const int y = tile_y * 8 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const size_t frame_b = (size_t)src_t * SLOT_B;      // src_t in [0, T_model): slot + src_t is a slot of a dynamic block
    const size_t bplane_n = (size_t)p.tiles_y * p.tiles_x;
    struct Slot {
        TapsI t;
        BakedTaps v;
        float rho;
    } sA, sB;
    DispComposite c;
    auto fetch = [&](int d, Slot &s) {
        TapsI &tp = s.t;
        BakedTaps &v = s.v;
        float h[VL3D_HN];
        load_uniform(homos + VL3D_HS * d, h);
        tp = make_taps_i<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy, plane_cull(a, d));
        s.rho = plane_rho(rows, d, px, py);
        v = BakedTaps{u2w{0u, 0u}, u2w{0u, 0u}};
        // an uncovered pixel leaves the composite state untouched bit for bit (a = 0): nothing is fetched, and the step is skipped
        if (tp.cov != 0.0f) {
            // the base tap is clamped to x0 <= Ws - 2, y0 <= Hs - 2: rows y0, y0 + 1 and columns x0, x0 + 1 are texels of the plane, their
            // blocks entries of the table
            const int y1 = tp.y0 + 1;
            const int *brow0 = p.blocks + (size_t)d * bplane_n + (size_t)(tp.y0 / TSB) * p.tiles_x;
            const int *brow1 = brow0 + ((y1 % TSB) == 0 ? p.tiles_x : 0);
            const int bx = tp.x0 / TSB, bx1 = (tp.x0 + 1) / TSB;      // x0 + 1 <= Ws - 1: block bx1 exists
            const int e00 = brow0[bx], e10 = brow1[bx], e01 = brow0[bx1], e11 = brow1[bx1];
            const unsigned xin = (unsigned)(tp.x0 % TSB) * 4u;
            const unsigned in0 = (unsigned)(tp.y0 % TSB) * (TSB * 4u) + xin, in1 = (unsigned)(y1 % TSB) * (TSB * 4u) + xin;
            if (bx == bx1) {      // both texels of a row in one block: 8 contiguous bytes (4-byte aligned: x0 may be odd)
                v.r0 = pool_load<u2w_a4>(p, e00, in0, frame_b, u2w{p.culled, p.culled});
                v.r1 = pool_load<u2w_a4>(p, e10, in1, frame_b, u2w{p.culled, p.culled});
            } else {              // across a block seam: the right texel is column 0 of the next block
                v.r0 = u2w{pool_load<unsigned>(p, e00, in0, frame_b, p.culled), pool_load<unsigned>(p, e01, in0 - (TSB - 1) * 4u, frame_b, p.culled)};
                v.r1 = u2w{pool_load<unsigned>(p, e10, in1, frame_b, p.culled), pool_load<unsigned>(p, e11, in1 - (TSB - 1) * 4u, frame_b, p.culled)};
            }
        }
        asm volatile("" ::: "memory");      // keep the loads here: hipcc otherwise sinks them below the composite
    };
    auto step = [&](const Slot &s, int) {
        if (s.t.cov != 0.0f) c.baked(s.t, s.v, s.rho);
    };
    // two register sets: the next listed plane is fetched before the current one is composited; nothing is fetched past the end
    walk_planes_cond(ListedPlanes(a.cull_masks, tile), sA, sB, fetch, step);
    c.store(a, o, t0, x, y);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
int unsupported(const char *who, const char *bad) {
    vl3d_set_error((std::string(who) + ": " + bad).c_str());
    return VL3D_EUNSUPPORTED;
}

// what the three entries refuse before anything else.  The two VL3D_EUNSUPPORTED rows carry check_baked_desc's messages (vl3d_render_args.h).
int check_disp_desc(const vl3d_render_desc *desc, const char *who) {
    VL3D_REQUIRE(desc != nullptr, "null render desc");
    if (!(desc->coord_mode == VL3D_COORD_AFFINE && desc->border_mode == VL3D_BORDER_HARDCUT))
        return unsupported(who, "the planar MPV convention only (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT)");
    if (desc->uv_noise_seed != 0) return unsupported(who, "add_uv_noise is a training switch (uv_noise_seed = 0)");
    return VL3D_OK;
}

// rows, the outputs and the grid: the same for every source
int check_disp_io(const vl3d_render_desc *desc, const float *homos, const float *rows, const float *disp, const float *alpha, const char *who) {
    if (!(homos && rows && disp)) return refuse(who, "null pointer");
    if ((((uintptr_t)homos | (uintptr_t)rows | (uintptr_t)disp | (uintptr_t)alpha) & 3) != 0)
        return refuse(who, "homos, rows, disp and alpha must be 4-byte aligned");
    if (desc->D > 128) return refuse(who, "at most 128 planes (the plane masks are two 64-bit words)");
    if ((int64_t)((desc->W + 63) / 64) * ((desc->H + 7) / 8) * desc->T > 0x7fffffffll) return refuse(who, "tiles x frames exceed the grid");
    return VL3D_OK;
}

// the quad map of a tile-culled model into RenderArgs (nothing for a dense one)
int set_disp_cull(RenderArgs &a, const vl3d_render_desc *desc, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch, const char *who) {
    if (!quad_keep) return VL3D_OK;
    const int rc = check_cull_grid(desc, QH, QW, who);
    if (rc != VL3D_OK) return rc;
    if (!cull_scratch) return refuse(who, "tile culling needs vl3d_render_cull_scratch_bytes() of scratch");
    a.quad_keep = quad_keep;
    a.cull_masks = (const unsigned long long *)cull_scratch;
    set_cull_geometry(a, desc, QH, QW);
    return VL3D_OK;
}

}  // namespace

extern "C" int vl3d_render_disp_fwd(const vl3d_render_desc *desc, const void *stack, int32_t frame0, int32_t T_alloc, const float *homos,
                                    const float *rows, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch, float *disp,
                                    float *alpha, vl3d_stream_t stream) {
    const char *who = "vl3d_render_disp_fwd";
    int rc = check_disp_desc(desc, who);
    if (rc != VL3D_OK) return rc;
    if (desc->act_order != VL3D_ACT_POST)
        return unsupported(who, "the float clip is sampled, then activated (act_order VL3D_ACT_POST); a model trained under VL3D_ACT_BAKED bakes its "
                                "texels and takes vl3d_render_disp_baked");
    if (desc->variant != 0) return refuse(who, "no kernel variants (desc->variant = 0)");
    if (!(desc->D > 0 && desc->T > 0 && desc->Hs > 0 && desc->Ws > 0 && desc->H > 0 && desc->W > 0)) return refuse(who, "non-positive render dims");
    if (!(desc->Hs < (1 << 24) && desc->Ws < (1 << 24))) return refuse(who, "plane side too large (24-bit row arithmetic)");
    if (!((int64_t)desc->Hs * desc->Ws * 16 < (1ll << 32))) return refuse(who, "frame too large for 32-bit byte offsets");
    if (!(desc->stack_dtype == VL3D_F32 || desc->stack_dtype == VL3D_F16)) return refuse(who, "stack_dtype must be VL3D_F32 or VL3D_F16");
    if (!(desc->alpha_act >= VL3D_ACT_NONE && desc->alpha_act <= VL3D_ACT_ABS)) return refuse(who, "unknown activation");
    const bool f16 = desc->stack_dtype == VL3D_F16;
    if (!stack) return refuse(who, "null pointer");
    if (((uintptr_t)stack & (f16 ? 7 : 15)) != 0) return refuse(who, "the texels must be 16-byte aligned (fp32) or 8-byte aligned (fp16)");
    if ((rc = check_disp_io(desc, homos, rows, disp, alpha, who)) != VL3D_OK) return rc;
    if (T_alloc <= 0) return refuse(who, "T_alloc must be the clip length of the stack allocation");
    if (!(frame0 >= 0 && (int64_t)frame0 + desc->T <= T_alloc)) return refuse(who, "the run of frames leaves the clip");
    RenderArgs a = render_args_of(desc);
    if ((rc = set_disp_cull(a, desc, quad_keep, QH, QW, cull_scratch, who)) != VL3D_OK) return rc;
    a.Tstride = T_alloc;
    a.stack = reinterpret_cast<const float *>(reinterpret_cast<const char *>(stack) + (size_t)frame0 * desc->Hs * desc->Ws * (f16 ? 8 : 16));
    a.homos = homos;
    a.g_f16 = f16;
    const DispArgs o{rows, disp, alpha, desc->alpha_act};
    const int tiles_x = (a.W + 63) / 64, tiles_y = (a.H + 7) / 8;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles_x * tiles_y * a.T)), block(512);
    if (a.quad_keep) {
        launch_cull_fwd_plan<VL3D_COORD_AFFINE>(a, 8, tiles_x, tiles_y, s);
        if (f16) hipLaunchKernelGGL((render_disp_fwd_k<true, true>), grid, block, 0, s, a, o, tiles_x, tiles_y);
        else hipLaunchKernelGGL((render_disp_fwd_k<false, true>), grid, block, 0, s, a, o, tiles_x, tiles_y);
    } else {
        if (f16) hipLaunchKernelGGL((render_disp_fwd_k<true, false>), grid, block, 0, s, a, o, tiles_x, tiles_y);
        else hipLaunchKernelGGL((render_disp_fwd_k<false, false>), grid, block, 0, s, a, o, tiles_x, tiles_y);
    }
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_render_disp_baked(const vl3d_render_desc *desc, const uint8_t *baked, int32_t T_alloc, const float *homos, const float *rows,
                                      const vl3d_baked_frames *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch,
                                      float *disp, float *alpha, vl3d_stream_t stream) {
    const char *who = "vl3d_render_disp_baked";
    int rc = check_disp_desc(desc, who);
    if (rc != VL3D_OK) return rc;
    // a row's two taps are one 8-byte load, the two rows a constant step apart
    if ((rc = check_baked_desc(desc, 1ll << 28, "plane too large for 32-bit tap offsets", who)) != VL3D_OK) return rc;
    bool is_path = false;
    if ((rc = check_baked_frames(desc, sel, is_path, who)) != VL3D_OK) return rc;
    if (!baked) return refuse(who, "null pointer");
    if (((uintptr_t)baked & 3) != 0) return refuse(who, "the texels must be 4-byte aligned");
    if ((rc = check_disp_io(desc, homos, rows, disp, alpha, who)) != VL3D_OK) return rc;
    if (is_path) {
        if (!(T_alloc > 0)) return refuse(who, "a clip of T_alloc >= 1 frames");
    } else if (!(T_alloc > 0 && sel->frame0 >= 0 && (int64_t)sel->frame0 + desc->T <= T_alloc)) {
        return refuse(who, "the run of frames leaves the clip");
    }
    RenderArgs a = render_args_of(desc);      // (a path: a.T is the count of its output frames)
    if ((rc = set_disp_cull(a, desc, quad_keep, QH, QW, cull_scratch, who)) != VL3D_OK) return rc;
    a.Tstride = T_alloc;
    a.stack = reinterpret_cast<const float *>(baked + (is_path ? 0 : (size_t)sel->frame0 * desc->Hs * desc->Ws * 4));
    a.homos = homos;
    const DispArgs o{rows, disp, alpha, 0};
    const int tiles_x = (a.W + 63) / 64, tiles_y = (a.H + 7) / 8;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles_x * tiles_y * a.T)), block(512);
    const PathIdx path{sel->frame_cam, sel->frame_t, sel->n_cams, T_alloc};
    if (a.quad_keep) {
        if (is_path) {
            launch_cull_fwd_plan_cams<VL3D_COORD_AFFINE>(a, path.n_cams, 8, tiles_x, tiles_y, s);
            hipLaunchKernelGGL((render_disp_baked_k<true, PathIdx>), grid, block, 0, s, a, o, tiles_x, tiles_y, path);
        } else {
            launch_cull_fwd_plan<VL3D_COORD_AFFINE>(a, 8, tiles_x, tiles_y, s);
            hipLaunchKernelGGL((render_disp_baked_k<true, NoPath>), grid, block, 0, s, a, o, tiles_x, tiles_y, NoPath{});
        }
    } else if (is_path) {
        hipLaunchKernelGGL((render_disp_baked_k<false, PathIdx>), grid, block, 0, s, a, o, tiles_x, tiles_y, path);
    } else {
        hipLaunchKernelGGL((render_disp_baked_k<false, NoPath>), grid, block, 0, s, a, o, tiles_x, tiles_y, NoPath{});
    }
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_render_disp_baked_pool(const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t T_model,
                                           const float *homos, const float *rows, const vl3d_baked_frames *sel, const uint8_t *quad_keep,
                                           int32_t QH, int32_t QW, uint32_t culled_rgba8, void *cull_scratch, float *disp, float *alpha,
                                           vl3d_stream_t stream) {
    const char *who = "vl3d_render_disp_baked_pool";
    int rc = check_disp_desc(desc, who);
    if (rc != VL3D_OK) return rc;
    if ((rc = check_baked_desc(desc, INT64_MAX, "plane too large", who)) != VL3D_OK) return rc;
    bool is_path = false;
    if ((rc = check_baked_frames(desc, sel, is_path, who)) != VL3D_OK) return rc;
    if (!(blocks && pool && quad_keep && cull_scratch))
        return refuse(who, "null pointer (the quad map and vl3d_render_cull_scratch_bytes() of scratch are required)");
    if (!(((uintptr_t)pool & 3) == 0 && ((uintptr_t)blocks & 3) == 0)) return refuse(who, "the pool and the block table must be 4-byte aligned");
    if ((rc = check_disp_io(desc, homos, rows, disp, alpha, who)) != VL3D_OK) return rc;
    if (is_path) {
        if (!(T_model > 0)) return refuse(who, "a model of T_model >= 1 frames");
    } else if (!(T_model > 0 && sel->frame0 >= 0 && (int64_t)sel->frame0 + desc->T <= T_model)) {
        return refuse(who, "the run of frames leaves the model's T_model frames");
    }
    if (!(desc->cull_Hs == 0 && desc->cull_Ws == 0)) return refuse(who, "the pool holds whole planes (no desc->cull_* window)");
    RenderArgs a = render_args_of(desc);
    if ((rc = set_disp_cull(a, desc, quad_keep, QH, QW, cull_scratch, who)) != VL3D_OK) return rc;
    a.homos = homos;
    const DispArgs o{rows, disp, alpha, 0};
    const PoolSrc p{blocks, reinterpret_cast<const char *>(pool), (desc->Hs + TSB - 1) / TSB, (desc->Ws + TSB - 1) / TSB, is_path ? 0 : sel->frame0,
                    culled_rgba8};
    const int tiles_x = (a.W + 63) / 64, tiles_y = (a.H + 7) / 8;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(tiles_x * tiles_y * a.T)), block(512);
    if (is_path) {
        const PathIdx path{sel->frame_cam, sel->frame_t, sel->n_cams, T_model};
        launch_cull_fwd_plan_cams<VL3D_COORD_AFFINE>(a, path.n_cams, 8, tiles_x, tiles_y, s);
        hipLaunchKernelGGL((render_disp_baked_pool_k<PathIdx>), grid, block, 0, s, a, o, p, tiles_x, tiles_y, path);
    } else {
        launch_cull_fwd_plan<VL3D_COORD_AFFINE>(a, 8, tiles_x, tiles_y, s);
        hipLaunchKernelGGL((render_disp_baked_pool_k<NoPath>), grid, block, 0, s, a, o, p, tiles_x, tiles_y, NoPath{});
    }
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
