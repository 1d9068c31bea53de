// RGB-D frames of the baked playback model (include/vl3d.h "RGB-D"): colour AND disparity from ONE walk of the planes.
//
// vl3d_render_fwd_baked(_pool) gives the picture, vl3d_render_disp_baked(_pool) the depth map beside it; both walk the same planes, fetch the
// same texels and form the same per-plane alpha.  The two kernels of this unit are the colour kernels' skeletons -- render_fwd_baked_k (a
// dense or tile-culled clip) and render_fwd_baked_pool_k (the pool behind its block table): 64 x 8 pixels per workgroup, XCD remap, the next
// plane's taps in flight while the current plane is composited, frame pairs for a run, one output frame along a path, two source frames at a
// loop time -- with one more accumulator per frame:
//     disp = fmaf(w, rho, disp),   w = a T the weight colour uses,   rho = fmaf(rows[k][0], x + c, fmaf(rows[k][1], y + c, rows[k][2]))
// Reused as they are (vl3d_render_core.h, vl3d_baked_core.h): make_taps2 / make_taps_i / plane_cull, walk_planes / walk_planes_cond,
// path_frame, blend, the plan launches, display_word / display_store.  The composite is RgbdComposite below: BakedComposite's five statements
// spelt out again in the same order under fp contract(off) -- nothing is factored out of BakedComposite, whose comments record what that
// costs the one-frame colour kernels -- plus the one fmaf of DispComposite (csrc/vl3d_render_disp.hip).  So, bit for bit: rgb and alpha are
// the colour entry's float sink, the display frames its display sink, disp of a run or a path the disparity entry's.  A loop time has no depth
// twin: its alpha is the lerped c_3 * cov that the colour statements use, and that alpha weights rho.
// The 16-bit depth of the display sink: depth16 = (uint16) trunc(65535 * min(max(disp, 0), 1)), every operation rounded on its own; not
// divided by alpha, not composited over the background (an uncovered pixel reads 0: far).
// No LDS, no scratch memory.  Bounds: a thread returns unless x < W and y < H and stores at pixel (t * H + y) * W + x < N * H * W of every
// output, 64-bit; a path workgroup whose camera, frame or time is out of range returns before any load or store (path_frame).
#include "vl3d_baked_core.h"
#include "vl3d_render_args.h"

using namespace vl3d_render_detail;

namespace {

// ---- sinks ----------------------------------------------------------------------------------------------------------------------------------
// FLOAT: a.rgb / a.alpha (RenderArgs) and disp.  DISPLAY: the colour frames of DisplayOut and depth16 (N,H,W) uint16, one two-byte store per
// lane: a wave's 64 levels are 128 contiguous bytes.  (Lane-packed dwords under display_store's condition were measured beside them and were
// no faster on any storage: docs/kernels/K9_baked_playback.md "RGB-D".)
struct RgbdFloat { float *disp; };
struct RgbdDisplay {
    DisplayOut c;
    uint16_t *depth16;
};

__device__ __forceinline__ unsigned depth_level(float d) {
#pragma clang fp contract(off)
    return (unsigned)(65535.0f * fminf(fmaxf(d, 0.0f), 1.0f));
}

// rho_k under pixel (px, py) from the plane's row: the one expression of DispComposite's plane_rho (csrc/vl3d_render_disp.hip).  Where it is
// evaluated is the register table's choice (docs/kernels/K9_baked_playback.md "RGB-D"), the bits are the same: a loop-time kernel forms rho
// in the fetch and keeps one VGPR per slot (slot_rows / slot_rho on float[1]); the others keep the row's three scalars, SGPRs, in the slot
// and form rho in the step (float[3]).
__device__ __forceinline__ float rho_of(const float (&r)[3], float px, float py) { return fmaf(r[0], px, fmaf(r[1], py, r[2])); }
__device__ __forceinline__ void slot_rows(const float *rows, int d, float, float, float (&out)[3]) { load_uniform(rows + 3 * d, out); }
__device__ __forceinline__ void slot_rows(const float *rows, int d, float px, float py, float (&out)[1]) {
    float r[3];
    load_uniform(rows + 3 * d, r);      // scalar loads, as the homographies
    out[0] = rho_of(r, px, py);
}
__device__ __forceinline__ float slot_rho(const float (&r)[3], float px, float py) { return rho_of(r, px, py); }
__device__ __forceinline__ float slot_rho(const float (&r)[1], float, float) { return r[0]; }

// ---- the composite ------------------------------------------------------------------------------------------------------------------------
// BakedComposite (vl3d_baked_core.h) with a sixth accumulator: the kernel declares and clears the six arrays, this struct steps and stores
// them; OWNER is a type local to the kernel instantiation.  The statements on Tr, cr, cg, cb and A are BakedComposite's, in its order, and
// must give its bits; the statement on Dp is DispComposite's.
template <int NF, typename OWNER>
struct RgbdComposite {
    static_assert(NF == 1 || NF == 2, "one frame or a frame pair per thread");
    float (&Tr)[NF], (&cr)[NF], (&cg)[NF], (&cb)[NF], (&A)[NF], (&Dp)[NF];
    float fr = 0.0f;      // a loop time: time - t0
    __device__ __forceinline__ RgbdComposite(float (&Tr_)[NF], float (&cr_)[NF], float (&cg_)[NF], float (&cb_)[NF], float (&A_)[NF], float (&Dp_)[NF])
        : Tr(Tr_), cr(cr_), cg(cg_), cb(cb_), A(A_), Dp(Dp_) {}
    // one plane of NF frames: v[f] the taps of frame f, rho the plane's inverse view depth under this pixel
    template <typename TAPS>
    __device__ __forceinline__ void operator()(const TAPS &t, const BakedTaps *v, float rho) const {
#pragma clang fp contract(off)
        const f4 w255 = t.w * (1.0f / 255.0f);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const float al = blend<3>(v[f], w255) * t.cov;      // uncovered: a = 0 -> the plane drops out of the composite
            const float w = al * Tr[f];
            cr[f] = fmaf(w, blend<0>(v[f], w255), cr[f]); cg[f] = fmaf(w, blend<1>(v[f], w255), cg[f]); cb[f] = fmaf(w, blend<2>(v[f], w255), cb[f]);
            Dp[f] = fmaf(w, rho, Dp[f]);
            A[f] += w;
            Tr[f] *= (1.0f - al);
        }
    }
    // one plane at a fractional loop time: v[0], v[1] the taps of frames t0 and t1; every channel c = fmaf(fr, b1 - b0, b0), alpha included
    template <typename TAPS>
    __device__ __forceinline__ void at_time(const TAPS &t, const BakedTaps *v, float rho) const {
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
        Dp[0] = fmaf(w, rho, Dp[0]);
        A[0] += w;
        Tr[0] *= (1.0f - al);
    }
    // pixel (x, y) of frame t0, then of frame t0 + 1 under has1 (odd T: the last pair composites frame t0 twice and stores it once)
    __device__ __forceinline__ void store(const RenderArgs &a, const RgbdDisplay &o, int t0, int x, int y, bool has1) const {
        const size_t pix = ((size_t)t0 * a.H + y) * a.W + x;
        const int x0w = x - (int)(threadIdx.x & 63);
        display_store(o.c, pix, x0w, a.W, display_word(o.c, cr[0], cg[0], cb[0], A[0]));
        o.depth16[pix] = (uint16_t)depth_level(Dp[0]);
        if constexpr (NF == 2) {
            if (has1) {
                display_store(o.c, pix + (size_t)a.H * a.W, x0w, a.W, display_word(o.c, cr[1], cg[1], cb[1], A[1]));
                o.depth16[pix + (size_t)a.H * a.W] = (uint16_t)depth_level(Dp[1]);
            }
        }
    }
    __device__ __forceinline__ void store(const RenderArgs &a, const RgbdFloat &o, int t0, int x, int y, bool has1) const {
        size_t pix = ((size_t)t0 * a.H + y) * a.W + x;
        a.rgb[pix * 3 + 0] = cr[0]; a.rgb[pix * 3 + 1] = cg[0]; a.rgb[pix * 3 + 2] = cb[0];
        a.alpha[pix] = A[0];
        o.disp[pix] = Dp[0];
        if constexpr (NF == 2) {
            if (has1) {
                pix += (size_t)a.H * a.W;
                a.rgb[pix * 3 + 0] = cr[1]; a.rgb[pix * 3 + 1] = cg[1]; a.rgb[pix * 3 + 2] = cb[1];
                a.alpha[pix] = A[1];
                o.disp[pix] = Dp[1];
            }
        }
    }
};

// ---- the clip -----------------------------------------------------------------------------------------------------------------------------
// the taps of a dense clip: one 8-byte load per texel row against a uniform plane base (the colour kernel's fetch)
__device__ __forceinline__ BakedTaps load_baked(const char *__restrict__ plane, const Taps2 &t, unsigned row_b) {
    const size_t o = (size_t)(t.off >> 2);      // make_taps2 gives the byte offset of 16-byte texels
    return BakedTaps{*reinterpret_cast<const u2w_a4 *>(plane + o), *reinterpret_cast<const u2w_a4 *>(plane + row_b + o)};
}

// render_fwd_baked_k (csrc/vl3d_render_baked.hip) with `rows` beside the homographies: PATH = NoPath (a run, frame pairs for NF = 2),
// PathIdx (a camera path) or PathTime (a path in loop time: two source frames); OUT = RgbdFloat or RgbdDisplay.
template <int NF, bool CULL, typename PATH, typename OUT>
__global__ __launch_bounds__(512) void render_rgbd_baked_k(RenderArgs a, const float *rows, int tiles_x, int tiles_y, PATH path, OUT out) {
    constexpr bool IS_PATH = !std::is_same<PATH, NoPath>::value;
    constexpr bool IS_TIME = std::is_same<PATH, PathTime>::value;
    constexpr int NS = baked_sources<NF, PATH>();      // source frames fetched per thread
    constexpr bool RHO_IN_SLOT = IS_TIME;
    static_assert(!IS_PATH || NF == 1, "a camera path renders one frame per thread");
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, rest = b / tiles_x;
    const int tile_y = rest % tiles_y, t0 = (rest / tiles_y) * NF;      // (a path: the output frame)
    const bool has1 = NF == 2 && t0 + 1 < a.T;      // odd T: the last pair composites frame t0 twice and stores it once
    int tile = tile_y * tiles_x + tile_x, src_t = t0;
    [[maybe_unused]] int src_t1 = 0;          // a loop time: the second source frame and the fraction
    [[maybe_unused]] float frac = 0.0f;
    const float *homos = a.homos;
    if constexpr (IS_PATH) {
        int cam;
        if constexpr (IS_TIME) {
            if (!path_frame(path, t0, cam, src_t, src_t1, frac)) return;
        } else {
            if (!path_frame(path, t0, cam, src_t)) return;      // uniform: nothing loaded, nothing stored
        }
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
    const char *base[NS];
    base[0] = reinterpret_cast<const char *>(a.stack) + (size_t)src_t * frame_b;
    if constexpr (IS_TIME) base[1] = reinterpret_cast<const char *>(a.stack) + (size_t)src_t1 * frame_b;
    else if constexpr (NF == 2) base[1] = base[0] + (has1 ? frame_b : 0);
    float Tr[NF], cr[NF], cg[NF], cb[NF], A[NF], Dp[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) { Tr[f] = 1.0f; cr[f] = cg[f] = cb[f] = A[f] = Dp[f] = 0.0f; }
    struct Slot {
        Taps2 t;
        BakedTaps v[NS];
        float r[RHO_IN_SLOT ? 1 : 3];      // rho, or the plane's row as three scalars (slot_rows)
    } sA, sB;
    struct Owner;
    RgbdComposite<NF, Owner> composite(Tr, cr, cg, cb, A, Dp);
    composite.fr = frac;
    auto fetch = [&](int d, Slot &s) {
        Taps2 &t = s.t;
        BakedTaps *v = s.v;
        float h[VL3D_HN];
        load_uniform(homos + VL3D_HS * d, h);
        if constexpr (CULL) t = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy, plane_cull(a, d));
        else t = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy);
        slot_rows(rows, d, px, py, s.r);
#pragma unroll
        for (int f = 0; f < NS; ++f) v[f] = load_baked(base[f] + (size_t)d * plane_stride_b, t, row_b);
        asm volatile("" ::: "memory");      // keep the loads here: hipcc otherwise sinks them below the composite
    };
    auto step = [&](const Slot &s, int) {
        if constexpr (IS_TIME) composite.at_time(s.t, s.v, slot_rho(s.r, px, py));
        else composite(s.t, s.v, slot_rho(s.r, px, py));
    };
    if constexpr (CULL) walk_planes(ListedPlanes(a.cull_masks, tile), sA, sB, fetch, step);
    else walk_planes(DensePlanes{a.D}, sA, sB, fetch, step);
    composite.store(a, out, t0, x, y, has1);
}

// ---- the pool -----------------------------------------------------------------------------------------------------------------------------
constexpr int TSB = 8;                           // block side (vl3d_adam_window_tile())
constexpr unsigned SLOT_B = TSB * TSB * 4;       // bytes of a slot: 64 RGBA8 texels

struct PoolSrc {
    const int *blocks;           // [D][tiles_y][tiles_x]
    const char *pool;            // n_slots * SLOT_B bytes
    int tiles_y, tiles_x;
    int frame0;                  // first frame of the run, in the model's T frames
    unsigned culled;             // the texel a block without storage reads as
};

// the colour pool kernel's texel load (csrc/vl3d_render_baked_pool.hip): issued only under `e >= 0`; a static block, the odd tail or
// t1 == t0 serve both source frames from one fetch
template <int NS, typename L, typename V>
__device__ __forceinline__ void pool_load(const PoolSrc &p, int e, unsigned in_b, size_t frame_b, ptrdiff_t frame1_b, bool has1, V fill, V (&out)[NS]) {
#pragma unroll
    for (int f = 0; f < NS; ++f) out[f] = fill;
    if (e < 0) return;
    const char *b = p.pool + (size_t)(e >> 1) * SLOT_B + in_b + ((e & 1) ? frame_b : 0);
    out[0] = *reinterpret_cast<const L *>(b);
    if constexpr (NS == 2) {
        out[1] = out[0];
        if ((e & 1) && has1) out[1] = *reinterpret_cast<const L *>(b + frame1_b);
    }
}

// render_fwd_baked_pool_k with `rows` beside the homographies; an uncovered pixel fetches nothing and skips its step, as there
template <int NF, typename PATH, typename OUT>
__global__ __launch_bounds__(512) void render_rgbd_baked_pool_k(RenderArgs a, const float *rows, PoolSrc p, int tiles_x, int tiles_y, PATH path, OUT out) {
    constexpr bool IS_PATH = !std::is_same<PATH, NoPath>::value;
    constexpr bool IS_TIME = std::is_same<PATH, PathTime>::value;
    constexpr int NS = baked_sources<NF, PATH>();      // source frames fetched per thread
    constexpr bool RHO_IN_SLOT = IS_TIME;
    static_assert(!IS_PATH || NF == 1, "a camera path renders one frame per thread");
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, rest = b / tiles_x;
    const int tile_y = rest % tiles_y, t0 = (rest / tiles_y) * NF;      // (a path: the output frame)
    bool has1 = NF == 2 && t0 + 1 < a.T;      // odd T: the last pair composites frame t0 twice and stores it once
    int tile = tile_y * tiles_x + tile_x, src_t = p.frame0 + t0;
    ptrdiff_t frame1_b = SLOT_B;      // a pair: the next slot of a dynamic block
    [[maybe_unused]] float frac = 0.0f;
    const float *homos = a.homos;
    if constexpr (IS_PATH) {
        int cam;
        if constexpr (IS_TIME) {
            int src_t1;
            if (!path_frame(path, t0, cam, src_t, src_t1, frac)) return;
            has1 = src_t1 != src_t;      // (a model of one frame: t1 = t0)
            frame1_b = (ptrdiff_t)(src_t1 - src_t) * (ptrdiff_t)SLOT_B;      // both in [0, T_model): slot + t1 is a slot of the block
        } else {
            if (!path_frame(path, t0, cam, src_t)) return;      // uniform: nothing loaded, nothing stored
        }
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
    float Tr[NF], cr[NF], cg[NF], cb[NF], A[NF], Dp[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) { Tr[f] = 1.0f; cr[f] = cg[f] = cb[f] = A[f] = Dp[f] = 0.0f; }
    struct Slot {
        TapsI t;
        BakedTaps v[NS];
        float r[RHO_IN_SLOT ? 1 : 3];      // rho, or the plane's row as three scalars (slot_rows)
    } sA, sB;
    struct Owner;
    RgbdComposite<NF, Owner> state(Tr, cr, cg, cb, A, Dp);
    state.fr = frac;
    auto fetch = [&](int d, Slot &s) {
        TapsI &t = s.t;
        BakedTaps *v = s.v;
        float h[VL3D_HN];
        load_uniform(homos + VL3D_HS * d, h);
        t = make_taps_i<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy, plane_cull(a, d));
        slot_rows(rows, d, px, py, s.r);
#pragma unroll
        for (int f = 0; f < NS; ++f) v[f] = BakedTaps{u2w{0u, 0u}, u2w{0u, 0u}};
        // an uncovered pixel leaves the composite state untouched bit for bit (a = 0): nothing is fetched, and the step is skipped
        if (t.cov != 0.0f) {
            // the base tap is clamped to x0 <= Ws - 2, y0 <= Hs - 2: rows y0, y0 + 1 and columns x0, x0 + 1 are texels of the plane, their
            // blocks entries of the table
            const int y1 = t.y0 + 1;
            const int *brow0 = p.blocks + (size_t)d * bplane_n + (size_t)(t.y0 / TSB) * p.tiles_x;
            const int *brow1 = brow0 + ((y1 % TSB) == 0 ? p.tiles_x : 0);
            const int bx = t.x0 / TSB, bx1 = (t.x0 + 1) / TSB;      // x0 + 1 <= Ws - 1: block bx1 exists
            const int e00 = brow0[bx], e10 = brow1[bx], e01 = brow0[bx1], e11 = brow1[bx1];      // stage 1: four independent 4-byte loads
            const unsigned xin = (unsigned)(t.x0 % TSB) * 4u;
            const unsigned in0 = (unsigned)(t.y0 % TSB) * (TSB * 4u) + xin, in1 = (unsigned)(y1 % TSB) * (TSB * 4u) + xin;
            u2w r0[NS], r1[NS];
            if (bx == bx1) {      // both texels of a row in one block: 8 contiguous bytes (4-byte aligned: x0 may be odd)
                pool_load<NS, u2w_a4>(p, e00, in0, frame_b, frame1_b, has1, u2w{p.culled, p.culled}, r0);
                pool_load<NS, u2w_a4>(p, e10, in1, frame_b, frame1_b, has1, u2w{p.culled, p.culled}, r1);
            } else {              // across a block seam: the right texel is column 0 of the next block
                unsigned l0[NS], l1[NS], q0[NS], q1[NS];
                pool_load<NS, unsigned>(p, e00, in0, frame_b, frame1_b, has1, p.culled, l0);
                pool_load<NS, unsigned>(p, e01, in0 - (TSB - 1) * 4u, frame_b, frame1_b, has1, p.culled, q0);
                pool_load<NS, unsigned>(p, e10, in1, frame_b, frame1_b, has1, p.culled, l1);
                pool_load<NS, unsigned>(p, e11, in1 - (TSB - 1) * 4u, frame_b, frame1_b, has1, p.culled, q1);
#pragma unroll
                for (int f = 0; f < NS; ++f) { r0[f] = u2w{l0[f], q0[f]}; r1[f] = u2w{l1[f], q1[f]}; }
            }
#pragma unroll
            for (int f = 0; f < NS; ++f) v[f] = BakedTaps{r0[f], r1[f]};
        }
        asm volatile("" ::: "memory");      // keep the loads here: hipcc otherwise sinks them below the composite
    };
    auto composite_if = [&](const Slot &s, int) {
        if (s.t.cov != 0.0f) {
            if constexpr (IS_TIME) state.at_time(s.t, s.v, slot_rho(s.r, px, py));
            else state(s.t, s.v, slot_rho(s.r, px, py));
        }
    };
    walk_planes_cond(ListedPlanes(a.cull_masks, tile), sA, sB, fetch, composite_if);
    state.store(a, out, t0, x, y, NF == 2 && has1);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// exactly one selection
int check_rgbd_sel(const vl3d_baked_frames *sel, const vl3d_baked_times *times, const char *who) {
    if ((sel != nullptr) == (times != nullptr))
        return refuse(who, "exactly one of sel (a run or a path of frames) and times (a path in loop time)");
    return VL3D_OK;
}

// the sink: (rgb, alpha, disp) or (frames, depth16); the colour half of the display sink is display_out_of's
int rgbd_out_of(const vl3d_rgbd_out *out, const char *who, RgbdDisplay &disp) {
    if (!out) return refuse(who, "null pointer (out)");
    const bool fl = out->rgb || out->alpha || out->disp, dis = out->frames || out->depth16;
    if (fl && dis) return refuse(who, "out names both sinks (rgb, alpha and disp, or frames and depth16)");
    if (!fl && !dis) return refuse(who, "null pointer (out: rgb, alpha and disp, or frames and depth16)");
    if (fl) {
        if (!(out->rgb && out->alpha)) return refuse(who, "null pointer (out: rgb and alpha, or frames)");
        if (!out->disp) return refuse(who, "the float sink needs disp beside rgb and alpha");
        if (out->bg) return refuse(who, "a background colour belongs to the display sink (out->frames)");
        if ((((uintptr_t)out->rgb | (uintptr_t)out->alpha | (uintptr_t)out->disp) & 3) != 0) return refuse(who, "rgb, alpha and disp must be 4-byte aligned");
        return VL3D_OK;
    }
    const int rc = display_out_of(out->frames, out->channels, out->bg, who, disp.c);
    if (rc != VL3D_OK) return rc;
    if (!out->depth16) return refuse(who, "the display sink needs depth16 beside frames");
    if (((uintptr_t)out->depth16 & 1) != 0) return refuse(who, "depth16 must be 2-byte aligned");
    disp.depth16 = out->depth16;
    return VL3D_OK;
}

// what the disparity entries refuse beside the colour entries (their messages)
int check_rgbd_io(const vl3d_render_desc *desc, const float *homos, const float *rows, const char *who) {
    if (!(homos && rows)) return refuse(who, "null pointer");
    if ((((uintptr_t)homos | (uintptr_t)rows) & 3) != 0) return refuse(who, "homos and rows must be 4-byte aligned");
    if (desc->D > 128) return refuse(who, "at most 128 planes (the plane masks are two 64-bit words)");
    if ((int64_t)((desc->W + 63) / 64) * ((desc->H + 7) / 8) * desc->T > 0x7fffffffll) return refuse(who, "tiles x frames exceed the grid");
    return VL3D_OK;
}

// run / path / loop time x float / display -> f(NF, PATH, OUT)
template <typename F>
void dispatch_rgbd(const vl3d_render_desc *desc, const vl3d_baked_frames *sel, const vl3d_baked_times *times, bool is_path, int n_t,
                   const vl3d_rgbd_out *out, const RgbdDisplay &disp, const F &f) {
    const std::integral_constant<int, 1> one;      // frames per thread: pairs for a run of two or more, one along a path
    const std::integral_constant<int, 2> two;
    const RgbdFloat fo{out->disp};
    const bool fl = out->frames == nullptr;
    if (times) {
        const PathTime path{times->frame_cam, times->frame_time, times->n_cams, n_t};
        if (fl) f(one, path, fo);
        else f(one, path, disp);
    } else if (is_path) {
        const PathIdx path{sel->frame_cam, sel->frame_t, sel->n_cams, n_t};
        if (fl) f(one, path, fo);
        else f(one, path, disp);
    } else if (fl) {
        desc->T >= 2 ? f(two, NoPath{}, fo) : f(one, NoPath{}, fo);
    } else {
        desc->T >= 2 ? f(two, NoPath{}, disp) : f(one, NoPath{}, disp);
    }
}

}  // namespace

extern "C" int vl3d_render_rgbd_baked(const vl3d_render_desc *desc, const uint8_t *baked, int32_t T_alloc, const float *homos, const float *rows,
                                      const vl3d_baked_frames *sel, const vl3d_baked_times *times, const uint8_t *quad_keep, int32_t QH,
                                      int32_t QW, void *cull_scratch, const vl3d_rgbd_out *out, vl3d_stream_t stream) {
    const char *who = "vl3d_render_rgbd_baked";
    // a row's two taps are one 8-byte load, the two rows a constant step apart
    int rc = check_baked_desc(desc, 1ll << 28, "plane too large for 32-bit tap offsets", who);
    if (rc != VL3D_OK) return rc;
    if ((rc = check_rgbd_sel(sel, times, who)) != VL3D_OK) return rc;
    bool is_path = times != nullptr;
    RgbdDisplay disp{};
    if ((rc = times ? check_baked_times(desc, times, who) : check_baked_frames(desc, sel, is_path, who)) != VL3D_OK ||
        (rc = rgbd_out_of(out, who, disp)) != VL3D_OK)
        return rc;
    if (!baked) return refuse(who, "null pointer");
    if (((uintptr_t)baked & 3) != 0) return refuse(who, "the texels must be 4-byte aligned");
    if ((rc = check_rgbd_io(desc, homos, rows, who)) != VL3D_OK) return rc;
    if (is_path) {
        if (!(T_alloc > 0)) return refuse(who, "a clip of T_alloc >= 1 frames");
    } else if (!(T_alloc > 0 && sel->frame0 >= 0 && (int64_t)sel->frame0 + desc->T <= T_alloc)) {
        return refuse(who, "the run of frames leaves the clip");
    }
    RenderArgs a = render_args_of(desc);      // (a path: a.T is the count of its output frames)
    a.Tstride = T_alloc;
    a.stack = reinterpret_cast<const float *>(baked + (is_path ? 0 : (size_t)sel->frame0 * desc->Hs * desc->Ws * 4));
    a.homos = homos; a.rgb = out->rgb; a.alpha = out->alpha;
    if (quad_keep) {
        if ((rc = check_cull_grid(desc, QH, QW, who)) != VL3D_OK) return rc;
        if (!cull_scratch) return refuse(who, "tile culling needs vl3d_render_cull_scratch_bytes() of scratch");
        a.quad_keep = quad_keep;
        a.cull_masks = (const unsigned long long *)cull_scratch;
        set_cull_geometry(a, desc, QH, QW);
    }
    const int tiles_x = (a.W + 63) / 64, tiles_y = (a.H + 7) / 8;
    const hipStream_t s = (hipStream_t)stream;
    dispatch_rgbd(desc, sel, times, is_path, T_alloc, out, disp, [&](auto nf, const auto &path, const auto &o) {
        constexpr int NF = decltype(nf)::value;
        using PATH = std::decay_t<decltype(path)>;
        using OUT = std::decay_t<decltype(o)>;
        const dim3 grid((unsigned)(tiles_x * tiles_y * ((a.T + NF - 1) / NF))), block(512);
        if (a.quad_keep) {
            if constexpr (std::is_same<PATH, NoPath>::value) launch_cull_fwd_plan<VL3D_COORD_AFFINE>(a, 8, tiles_x, tiles_y, s);
            else launch_cull_fwd_plan_cams<VL3D_COORD_AFFINE>(a, path.n_cams, 8, tiles_x, tiles_y, s);
            hipLaunchKernelGGL((render_rgbd_baked_k<NF, true, PATH, OUT>), grid, block, 0, s, a, rows, tiles_x, tiles_y, path, o);
            return;
        }
        hipLaunchKernelGGL((render_rgbd_baked_k<NF, false, PATH, OUT>), grid, block, 0, s, a, rows, tiles_x, tiles_y, path, o);
    });
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_render_rgbd_baked_pool(const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t T_model,
                                           const float *homos, const float *rows, const vl3d_baked_frames *sel, const vl3d_baked_times *times,
                                           const uint8_t *quad_keep, int32_t QH, int32_t QW, uint32_t culled_rgba8, void *cull_scratch,
                                           const vl3d_rgbd_out *out, vl3d_stream_t stream) {
    const char *who = "vl3d_render_rgbd_baked_pool";
    int rc = check_baked_desc(desc, INT64_MAX, "plane too large", who);
    if (rc != VL3D_OK) return rc;
    if ((rc = check_rgbd_sel(sel, times, who)) != VL3D_OK) return rc;
    bool is_path = times != nullptr;
    RgbdDisplay disp{};
    if ((rc = times ? check_baked_times(desc, times, who) : check_baked_frames(desc, sel, is_path, who)) != VL3D_OK ||
        (rc = rgbd_out_of(out, who, disp)) != VL3D_OK)
        return rc;
    if (!(blocks && pool && quad_keep && cull_scratch))
        return refuse(who, "null pointer (the quad map and vl3d_render_cull_scratch_bytes() of scratch are required)");
    if (!(((uintptr_t)pool & 3) == 0 && ((uintptr_t)blocks & 3) == 0)) return refuse(who, "the pool and the block table must be 4-byte aligned");
    if ((rc = check_rgbd_io(desc, homos, rows, who)) != VL3D_OK) return rc;
    if (is_path) {
        if (!(T_model > 0)) return refuse(who, "a model of T_model >= 1 frames");
    } else if (!(T_model > 0 && sel->frame0 >= 0 && (int64_t)sel->frame0 + desc->T <= T_model)) {
        return refuse(who, "the run of frames leaves the model's T_model frames");
    }
    if (!(desc->cull_Hs == 0 && desc->cull_Ws == 0)) return refuse(who, "the pool holds whole planes (no desc->cull_* window)");
    if ((rc = check_cull_grid(desc, QH, QW, who)) != VL3D_OK) return rc;
    RenderArgs a = render_args_of(desc);      // (a.Tstride is not read: the pool has no frame stride)
    a.homos = homos; a.rgb = out->rgb; a.alpha = out->alpha;
    a.quad_keep = quad_keep;
    a.cull_masks = (const unsigned long long *)cull_scratch;
    set_cull_geometry(a, desc, QH, QW);
    const PoolSrc p{blocks, reinterpret_cast<const char *>(pool), (desc->Hs + TSB - 1) / TSB, (desc->Ws + TSB - 1) / TSB, is_path ? 0 : sel->frame0,
                    culled_rgba8};
    const int tiles_x = (a.W + 63) / 64, tiles_y = (a.H + 7) / 8;
    const hipStream_t s = (hipStream_t)stream;
    dispatch_rgbd(desc, sel, times, is_path, T_model, out, disp, [&](auto nf, const auto &path, const auto &o) {
        constexpr int NF = decltype(nf)::value;
        using PATH = std::decay_t<decltype(path)>;
        using OUT = std::decay_t<decltype(o)>;
        const dim3 grid((unsigned)(tiles_x * tiles_y * ((a.T + NF - 1) / NF))), block(512);
        if constexpr (std::is_same<PATH, NoPath>::value) launch_cull_fwd_plan<VL3D_COORD_AFFINE>(a, 8, tiles_x, tiles_y, s);
        else launch_cull_fwd_plan_cams<VL3D_COORD_AFFINE>(a, path.n_cams, 8, tiles_x, tiles_y, s);
        hipLaunchKernelGGL((render_rgbd_baked_pool_k<NF, PATH, OUT>), grid, block, 0, s, a, rows, p, tiles_x, tiles_y, path, o);
    });
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
