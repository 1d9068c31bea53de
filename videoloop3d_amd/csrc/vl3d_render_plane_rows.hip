// Row bands with per-plane source windows (include/vl3d.h "Row bands with PER-PLANE source windows"; videoloop3d_amd/dist.py
// plan_plane_bands): the rank's stack holds, for every plane d, only the rows [plane_row0[d], plane_row0[d] + R) its band can reach.
//
// The kernels are the dense render's (vl3d_render_core.h) with one change: the texel coordinate, the bilinear weights and the hard cut
// are those of the full-frame kernels (make_taps_i with the TRUE plane height), and the plane's integer origin is subtracted from the
// base tap's row index only -- subtracting it from the fp32 coordinate, or folding it into the homography, would be exact at these
// magnitudes only by luck.  The origin is uniform per plane: it is read through the constant address space (one scalar load per plane,
// an SGPR operand of the offset arithmetic).  A translation unit of its own, so that the headline kernels of vl3d_render_c*.hip compile
// exactly as before (their schedules are pinned by tests/test_kernel_schedule_canary.py).
#include "vl3d_render_args.h"

using vl3d_render_detail::RenderArgs;

namespace {

using namespace vl3d_render_detail;

constexpr int PR_COORD = VL3D_COORD_AFFINE, PR_BORDER = VL3D_BORDER_HARDCUT, PR_ORDER = VL3D_ACT_POST;
constexpr int PR_RACT = VL3D_ACT_SIGMOID, PR_AACT = VL3D_ACT_SIGMOID;
constexpr int PROWS = BWD_REGIONS[BWD_32X16].rows;      // region rows of its frame pairs: the dense render's 32 x 16 regions

// make_taps2 with the tap offset taken in the plane's local rows: local base row = global base row - r0, clamped into [0, R - 2] (a no-op
// for every sample of a band whose windows the planner built; it keeps a wrong table inside the allocation)
__device__ __forceinline__ Taps2 taps_plane_rows(const float *__restrict__ h, float px, float py, const RenderArgs &a, int r0, int R) {
    const TapsI ti = make_taps_i<PR_COORD, PR_BORDER>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy);
    Taps2 t;
    t.w = ti.w;
    t.cov = ti.cov; t.tx = ti.tx; t.ty = ti.ty;
    const int yl = min(max(ti.y0 - r0, 0), R - 2);
    t.off = (__umul24((unsigned)yl, (unsigned)a.Ws) + (unsigned)ti.x0) << 4;
    return t;
}

__device__ __forceinline__ int plane_origin(const int32_t *plane_row0, int d) { return ((cint_p)plane_row0)[d]; }

// Forward, two frames per thread: render_fwd2x_k's per-frame arithmetic instruction for instruction (the full-frame forward's bits).
template <bool F16>
__global__ __launch_bounds__(64 * 8, VL3D_FWD2X_MIN_WAVES) void render_fwd_plane_rows_k(RenderArgs a, const int32_t *plane_row0, int R, int tiles_x,
                                                                                       int tiles_y) {
    constexpr int TY = 8;
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, rest = b / tiles_x;
    const int tile_y = rest % tiles_y, t0 = (rest / tiles_y) * 2;
    const bool has1 = t0 + 1 < a.T;          // odd T: the last pair composites frame t0 twice and stores it once
    const int x = tile_x * 64 + (threadIdx.x & 63);
    const int y = tile_y * TY + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const size_t frame_b = (size_t)R * a.Ws * (F16 ? 8 : 16);      // local frames: R rows
    const size_t plane_stride_b = (size_t)a.T * frame_b;
    const char *plane0 = reinterpret_cast<const char *>(a.stack) + (size_t)t0 * frame_b;
    const char *plane1 = plane0 + (has1 ? frame_b : 0);
    float Tr0 = 1.0f, cr0 = 0.f, cg0 = 0.f, cb0 = 0.f, A0 = 0.f;
    float Tr1 = 1.0f, cr1 = 0.f, cg1 = 0.f, cb1 = 0.f, A1 = 0.f;
    const TapStep st = make_tap_step<F16>(a.Hs, a.Ws);
    typedef typename TapVal<F16, PR_ORDER>::type tapv_t;
    tapv_t vA0[4], vA1[4], vB0[4], vB1[4];
#define VL3D_COMPOSITE2(T_, V0_, V1_)                                        \
    {                                                                        \
        const f4 o0 = shade2<PR_ORDER, PR_RACT, PR_AACT>(T_, V0_);           \
        const f4 o1 = shade2<PR_ORDER, PR_RACT, PR_AACT>(T_, V1_);           \
        const float w0 = o0.w * Tr0, w1 = o1.w * Tr1;                        \
        cr0 += w0 * o0.x; cg0 += w0 * o0.y; cb0 += w0 * o0.z; A0 += w0;      \
        cr1 += w1 * o1.x; cg1 += w1 * o1.y; cb1 += w1 * o1.z; A1 += w1;      \
        Tr0 *= (1.0f - o0.w); Tr1 *= (1.0f - o1.w);                          \
    }
    Taps2 tA = taps_plane_rows(a.homos, px, py, a, plane_origin(plane_row0, 0), R), tB = tA;
    load_taps2<F16>(plane0, tA, st, vA0);
    load_taps2<F16>(plane1, tA, st, vA1);
    for (int d = 0;; d += 2) {
        {
            const int dn = min(d + 1, a.D - 1);
            float h[VL3D_HN];
            load_uniform(a.homos + VL3D_HS * dn, h);
            tB = taps_plane_rows(h, px, py, a, plane_origin(plane_row0, dn), R);
            load_taps2<F16>(plane0 + (size_t)dn * plane_stride_b, tB, st, vB0);
            load_taps2<F16>(plane1 + (size_t)dn * plane_stride_b, tB, st, vB1);
            asm volatile("" ::: "memory");   // keep the loads here: hipcc otherwise sinks them below the composite
        }
        VL3D_COMPOSITE2(tA, vA0, vA1)
        if (d + 1 >= a.D) break;
        {
            const int dn = min(d + 2, a.D - 1);
            float h[VL3D_HN];
            load_uniform(a.homos + VL3D_HS * dn, h);
            tA = taps_plane_rows(h, px, py, a, plane_origin(plane_row0, dn), R);
            load_taps2<F16>(plane0 + (size_t)dn * plane_stride_b, tA, st, vA0);
            load_taps2<F16>(plane1 + (size_t)dn * plane_stride_b, tA, st, vA1);
            asm volatile("" ::: "memory");
        }
        VL3D_COMPOSITE2(tB, vB0, vB1)
        if (d + 2 >= a.D) break;
    }
#undef VL3D_COMPOSITE2
    size_t pix = ((size_t)t0 * a.H + y) * a.W + x;
    a.rgb[pix * 3 + 0] = cr0; a.rgb[pix * 3 + 1] = cg0; a.rgb[pix * 3 + 2] = cb0;
    a.alpha[pix] = A0;
    if (has1) {
        pix += (size_t)a.H * a.W;
        a.rgb[pix * 3 + 0] = cr1; a.rgb[pix * 3 + 1] = cg1; a.rgb[pix * 3 + 2] = cb1;
        a.alpha[pix] = A1;
    }
}

// ---- Backward ----------------------------------------------------------------------------------------------------------------------------
// The owner-computes frame-pair path of the dense render (render_bwd_pair_k and its pre-passes, vl3d_render_core.h), on the local layout.
// Everything geometric stays in GLOBAL plane coordinates -- the plan's inverse homographies, the tiles' texel windows, the owner pixels, the
// staged texel coordinates of the gather -- so the gradient is that of the full-plane kernels bit for bit; only the addresses of the stack,
// the gradient and the owner table are taken in the plane's local rows [r0, r0 + R).  Local rows past the plane's last row are padding: the
// owner-table pass zero-fills them.  If bwd_plan_k finds the geometry outside the owner-computes preconditions, the gradient is zero-filled
// and the atomics sweep below takes the call (as vl3d_render_bwd does).

// the tiles' texel windows (bwd_windows_k, global rows) clipped to the rows a plane's local window holds: [r0, r0 + R)
__global__ __launch_bounds__(256) void clip_windows_k(int4 *win, int D, int ntiles, const int32_t *plane_row0, int R, const float *plan) {
    if (!reinterpret_cast<const int *>(plan)[0]) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ntiles * D) return;
    const int d = i % D, r0 = plane_row0[d];
    int4 rec = win[i];
    const int ww = rec.z & 0xffff, wh = (rec.z >> 16) & 0x3fff;
    const int y0 = max(rec.y, r0), y1 = min(rec.y + wh, r0 + R);
    if (ww == 0 || y1 <= y0) {      // nothing of this window is held here: an empty record whose corner is a valid local texel
        rec.x = 0; rec.y = r0; rec.z = 0;
    } else {
        rec.y = y0;
        rec.z = (rec.z & 0x40000000) | ww | ((y1 - y0) << 16);
    }
    win[i] = rec;
}

// bwd_owner_table_k over the local rows: the owner entry of local texel (x, k) of plane d is that of plane texel (x, r0 + k); texels no tile
// is certain to own, and the padding rows, get zero gradient for all T frames
template <bool F16>
__global__ __launch_bounds__(256) void owner_table_plane_rows_k(RenderArgs a, const int32_t *plane_row0, int R, int iw, int ih, int rh,
                                                                unsigned short *owner) {
    if (!reinterpret_cast<const int *>(a.plan)[0]) return;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int k = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int d = blockIdx.z;
    if (x >= a.Ws || k >= R) return;
    const int y = plane_origin(plane_row0, d) + k;
    const size_t frame = (size_t)R * a.Ws, lt = ((size_t)d * a.T * R + k) * a.Ws + x;      // local texel of frame 0
    bool zero = y >= a.Hs;
    if (!zero) {
        float qx, qy;
        owner_pixel(a.plan + PLAN_HDR + PLAN_REC * d, (float)x, (float)y, a.pc, a.col0, a.row0, qx, qy);
        const float rxf = fminf(fmaxf(rintf(qx), 0.0f), (float)(a.W - 1)), ryf = fminf(fmaxf(rintf(qy), 0.0f), (float)(a.H - 1));
        const int rx = (int)rxf, ry = (int)ryf;
        const int tx = (int)((rxf + 0.5f) * (1.0f / (float)iw)), ty = (int)((ryf + 0.5f) * (1.0f / (float)ih));
        const unsigned lc = (unsigned)((ry - ty * ih + rh) * 32 + (rx - tx * iw + rh));      // 32-wide regions: 9-bit slots
        owner[((size_t)d * R + k) * a.Ws + x] = (unsigned short)(((((unsigned)ty & 15u) << 3 | (unsigned)(tx & 7)) << 9) | lc);
        zero = !((qx > 0.5f) && (qx < (float)a.W - 1.5f) && (qy > 0.5f) && (qy < (float)a.H - 1.5f));
    }
    if (!zero) return;
    if constexpr (F16) {
        float2 *g = reinterpret_cast<float2 *>(a.g_stack) + lt;
        for (int t = 0; t < a.T; ++t, g += frame) *g = make_float2(0.f, 0.f);
    } else {
        float4 *g = reinterpret_cast<float4 *>(a.g_stack) + lt;
        for (int t = 0; t < a.T; ++t, g += frame) *g = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// pair_gather_plane (32 x 16 regions) with the window's texel index taken in local rows (win0) and its coordinates in global ones (tau)
template <bool F16>
__device__ __forceinline__ void gather_plane_rows(const RenderArgs &a, const float4 *sg0, const float4 *sg1, const float2 *st, int X0, int Y0, int r0,
                                                  int ww, int wh, bool apart, unsigned my_tile, unsigned e0, const unsigned short *oplane,
                                                  char *gplane0, size_t frame_b, bool has1, int col, int row) {
    constexpr int PW = 32;
    const unsigned win0 = (unsigned)((Y0 - r0) * a.Ws + X0);
    auto gather = [&](unsigned e, int wx, int wy, unsigned tix) {
        if ((e >> 9) != my_tile) return;
        const int lc = (int)(e & 511u);
        const f2 tau = f2{(float)(X0 + wx), (float)(Y0 + wy)};
        f4 acc0 = f4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
        if (apart) {
            const f2 c0 = *reinterpret_cast<const f2 *>(&st[lc]);
            const int li0 = lc - (tau.x < c0.x ? 1 : 0) - (tau.y < c0.y ? PW : 0);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int li = li0 + (k >> 1) * PW + (k & 1);
                const f2 dc = *reinterpret_cast<const f2 *>(&st[li]) - tau;
                const float wgt = tent_weight(dc.x) * tent_weight(dc.y);
                acc0 += *reinterpret_cast<const f4 *>(&sg0[li]) * wgt;
                acc1 += *reinterpret_cast<const f4 *>(&sg1[li]) * wgt;
            }
        } else {
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int li = lc + dy * PW + dx;
                    const f2 dc = *reinterpret_cast<const f2 *>(&st[li]) - tau;
                    const float wgt = tent_weight(dc.x) * tent_weight(dc.y);
                    if (__builtin_amdgcn_ballot_w64(wgt != 0.0f) == 0ull) continue;      // exact zeros for every texel of the wave
                    acc0 += *reinterpret_cast<const f4 *>(&sg0[li]) * wgt;
                    acc1 += *reinterpret_cast<const f4 *>(&sg1[li]) * wgt;
                }
        }
        store_grad_texel<F16>(gplane0, tix << 4, acc0);
        if (has1) store_grad_texel<F16>(gplane0 + frame_b, tix << 4, acc1);
    };
    if (row < wh && col < ww) gather(e0, col, row, win0 + (unsigned)(row * a.Ws + col));
    // rest of a window larger than 32 x 16: columns beyond 32 as a packed strip, rows beyond 16 one half-wave per row
    const int nec = ww - PW;
    if (nec > 0) {
        const int necp = min(nec, PW);
        const int sh = necp > 1 ? 32 - __builtin_clz((unsigned)(necp - 1)) : 0, rpg = PW >> sh, rmain = min(wh, PROWS);
        const int c = col & ((1 << sh) - 1), r = col >> sh;
        for (int wxb = PW; wxb < ww; wxb += (1 << sh))
            for (int wy0 = row * rpg; wy0 < rmain; wy0 += PROWS * rpg) {
                const int wy = wy0 + r, wx = wxb + c;
                if (c < necp && wx < ww && wy < rmain) {
                    const unsigned tix = win0 + (unsigned)(wy * a.Ws + wx);
                    gather(oplane[tix], wx, wy, tix);
                }
            }
    }
    for (int wy = row + PROWS; wy < wh; wy += PROWS)
        for (int wx = col; wx < ww; wx += PW) {
            const unsigned tix = win0 + (unsigned)(wy * a.Ws + wx);
            gather(oplane[tix], wx, wy, tix);
        }
}

// composite backward of one plane for one frame: VL3D_PAIR_GRAD of vl3d_render_core.h without the regularisers' term
#define VL3D_PR_GRAD(o, pre, Gr, Gg, Gb, gA, S, P, Tr, gv, ex)                                                                 \
    {                                                                                                                          \
        const float q = dot3p(Gr, o.x, Gg, o.y, Gb, o.z, gA);                                                                  \
        const float w = o.w * Tr;                                                                                              \
        P = fmaf(w, q, P);                                                                                                     \
        const float om = 1.0f - o.w;                                                                                           \
        const float behind = (om > 1e-12f) ? (S - P) * fast_rcp(om) : 0.0f;                                                    \
        gv = make_float4(fmaf(w, Gr, ex.x), fmaf(w, Gg, ex.y), fmaf(w, Gb, ex.z), fmaf(Tr, q, -behind) + ex.w);                \
        Tr *= om;                                                                                                              \
        if constexpr (ORDER == VL3D_ACT_POST)                                                                                  \
            gv = make_float4(gv.x * act_bwd<RACT>(pre.x, o.x), gv.y * act_bwd<RACT>(pre.y, o.y),                              \
                             gv.z * act_bwd<RACT>(pre.z, o.z), gv.w * act_bwd<AACT>(pre.w, o.w));                              \
    }

// render_bwd_pair_k (no regularisers, no fused optimiser step, 32 x 16 regions) on the local layout: per frame the arithmetic of the
// full-plane kernel in the same order
template <bool F16>
__global__ __launch_bounds__(32 * PROWS, VL3D_PAIR_MIN_WAVES) void render_bwd_pair_plane_rows_k(RenderArgs a, const int32_t *plane_row0, int R) {
    constexpr int PW = 32, PNT = PW * PROWS;
    if (!reinterpret_cast<const int *>(a.plan)[0]) return;
    __shared__ float4 s_g[2][2][PNT];   // [buffer][frame][pixel]
    __shared__ float2 s_t[2][PNT];
    const int tid = threadIdx.x, col = tid & (PW - 1), row = tid / PW;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = bid % a.tiles_x, rest = bid / a.tiles_x;
    const int tile_y = rest % a.tiles_y, t0 = (rest / a.tiles_y) * 2;
    const bool has1 = t0 + 1 < a.T;          // odd T: the last pair sweeps frame t0 twice and stores it once
    const int rx0 = tile_x * (PW - 2) - 1, ry0 = tile_y * (PROWS - 2) - 1;
    const int x = rx0 + col, y = ry0 + row;
    const bool inimg = (x >= 0) && (x < a.W) && (y >= 0) && (y < a.H);
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    constexpr size_t TEXB = F16 ? 8 : 16;
    const size_t frame_b = (size_t)R * a.Ws * TEXB;          // local frames: R rows
    const size_t plane_stride_b = (size_t)a.T * frame_b;
    const char *plane0 = reinterpret_cast<const char *>(a.stack) + (size_t)t0 * frame_b;
    char *gplane0 = reinterpret_cast<char *>(a.g_stack) + (size_t)t0 * frame_b;
    const size_t f1 = has1 ? frame_b : 0;
    float Gr0 = 0.f, Gg0 = 0.f, Gb0 = 0.f, gA0 = 0.f, S0 = 0.f, Gr1 = 0.f, Gg1 = 0.f, Gb1 = 0.f, gA1 = 0.f, S1 = 0.f;
    if (inimg) {
        size_t pix = ((size_t)t0 * a.H + y) * a.W + x;
        Gr0 = a.g_rgb[pix * 3 + 0]; Gg0 = a.g_rgb[pix * 3 + 1]; Gb0 = a.g_rgb[pix * 3 + 2];
        gA0 = a.g_alpha ? a.g_alpha[pix] : 0.0f;
        S0 = dot3p(Gr0, a.rgb[pix * 3 + 0], Gg0, a.rgb[pix * 3 + 1], Gb0, a.rgb[pix * 3 + 2], gA0 * a.alpha[pix]);
        if (has1) pix += (size_t)a.H * a.W;
        Gr1 = a.g_rgb[pix * 3 + 0]; Gg1 = a.g_rgb[pix * 3 + 1]; Gb1 = a.g_rgb[pix * 3 + 2];
        gA1 = a.g_alpha ? a.g_alpha[pix] : 0.0f;
        S1 = dot3p(Gr1, a.rgb[pix * 3 + 0], Gg1, a.rgb[pix * 3 + 1], Gb1, a.rgb[pix * 3 + 2], gA1 * a.alpha[pix]);
    }
    float Tr0 = 1.0f, P0 = 0.0f, Tr1 = 1.0f, P1 = 0.0f;
    const TapStep st = make_tap_step<F16>(a.Hs, a.Ws);
    const unsigned my_tile_id = (unsigned)(tile_y * a.tiles_x + tile_x);
    const unsigned my_tile = (unsigned)((tile_y & 15) << 3 | (tile_x & 7));
    const unsigned toff_thread = (unsigned)(row * a.Ws + col);
    const cint_p wrec = (cint_p)a.plan + plan_win_off(a.D) + (size_t)my_tile_id * a.D * 4;
    typedef typename TapVal<F16, PR_ORDER>::type tapv_t;
    for (int d = 0; d < a.D; ++d, plane0 += plane_stride_b, gplane0 += plane_stride_b) {
        float h[VL3D_HN];
        load_uniform(a.homos + VL3D_HS * d, h);
        const int r0 = plane_origin(plane_row0, d);
        const int X0 = wrec[4 * d], Y0 = wrec[4 * d + 1], wwh = wrec[4 * d + 2];
        const int ww = wwh & 0xffff, wh = (wwh >> 16) & 0x3fff;
        const bool apart = (wwh & 0x40000000) != 0;
        const int buf = d & 1;
        const unsigned short *oplane = a.owner + (size_t)d * R * a.Ws;
        const unsigned e0 = oplane[(unsigned)((Y0 - r0) * a.Ws + X0) + toff_thread];     // unconditional (padded table)
        float2 tc = make_float2(0.f, 0.f);
        float4 gv0 = make_float4(0.f, 0.f, 0.f, 0.f), gv1 = gv0;
        if (inimg) {
            const Taps2 tp = taps_plane_rows(h, px, py, a, r0, R);
            tapv_t tv0[4], tv1[4];
            load_taps2<F16>(plane0, tp, st, tv0);
            load_taps2<F16>(plane0 + f1, tp, st, tv1);
            f4 pre0, pre1;
            const f4 o0 = shade2<PR_ORDER, PR_RACT, PR_AACT>(tp, tv0, &pre0);
            const f4 o1 = shade2<PR_ORDER, PR_RACT, PR_AACT>(tp, tv1, &pre1);
            const f4 ex = f4{0.f, 0.f, 0.f, 0.f};
            constexpr int ORDER = PR_ORDER, RACT = PR_RACT, AACT = PR_AACT;
            VL3D_PR_GRAD(o0, pre0, Gr0, Gg0, Gb0, gA0, S0, P0, Tr0, gv0, ex)
            VL3D_PR_GRAD(o1, pre1, Gr1, Gg1, Gb1, gA1, S1, P1, Tr1, gv1, ex)
            tc = make_float2(tp.tx, tp.ty);
            if (!(tp.cov > 0.0f)) { gv0 = make_float4(0.f, 0.f, 0.f, 0.f); gv1 = gv0; }
        }
        s_t[buf][tid] = tc;
        s_g[buf][0][tid] = gv0;
        s_g[buf][1][tid] = gv1;
        __syncthreads();
        gather_plane_rows<F16>(a, s_g[buf][0], s_g[buf][1], s_t[buf], X0, Y0, r0, ww, wh, apart, my_tile, e0, oplane, gplane0, frame_b, has1, col, row);
    }
}

#undef VL3D_PR_GRAD

// the universal sweep for geometry outside the owner-computes preconditions: render_bwd_k's arithmetic per pixel and frame, scattered with
// atomics into the zero-filled local gradient (fp16: packed-half atomics, as render_bwd_k)
template <bool F16>
__global__ __launch_bounds__(TILE_X *TILE_Y) void render_bwd_plane_rows_scatter_k(RenderArgs a, const int32_t *plane_row0, int R) {
    if (a.plan && reinterpret_cast<const int *>(a.plan)[0]) return;   // the owner-computes path owns this call
    const int x = blockIdx.x * TILE_X + (threadIdx.x & (TILE_X - 1));
    const int y = blockIdx.y * TILE_Y + (threadIdx.x / TILE_X);
    const int t = blockIdx.z;
    if (x >= a.W || y >= a.H) return;
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    constexpr size_t TEXB = F16 ? 8 : 16;
    const size_t frame_b = (size_t)R * a.Ws * TEXB;
    const char *plane = reinterpret_cast<const char *>(a.stack) + (size_t)t * frame_b;
    char *gplane = reinterpret_cast<char *>(a.g_stack) + (size_t)t * frame_b;
    const size_t pix = ((size_t)t * a.H + y) * a.W + x;
    const float Gr = a.g_rgb[pix * 3 + 0], Gg = a.g_rgb[pix * 3 + 1], Gb = a.g_rgb[pix * 3 + 2];
    const float gA = a.g_alpha ? a.g_alpha[pix] : 0.0f;
    const float S = dot3p(Gr, a.rgb[pix * 3 + 0], Gg, a.rgb[pix * 3 + 1], Gb, a.rgb[pix * 3 + 2], gA * a.alpha[pix]);
    float Tr = 1.0f, P = 0.0f;
    const TapStep st = make_tap_step<F16>(a.Hs, a.Ws), gst = make_tap_step<false>(a.Hs, a.Ws);
    for (int d = 0; d < a.D; ++d, plane += (size_t)a.T * frame_b, gplane += (size_t)a.T * frame_b) {
        const Taps2 tp = taps_plane_rows(a.homos + VL3D_HS * d, px, py, a, plane_origin(plane_row0, d), R);
        if (tp.cov == 0.0f) continue;
        typename TapVal<F16, PR_ORDER>::type tv[4];
        f4 pre;
        load_taps2<F16>(plane, tp, st, tv);
        const f4 o = shade2<PR_ORDER, PR_RACT, PR_AACT>(tp, tv, &pre);
        const float q = dot3p(Gr, o.x, Gg, o.y, Gb, o.z, gA);
        const float w = o.w * Tr;
        P = fmaf(w, q, P);
        const float om = 1.0f - o.w;
        const float behind = (om > 1e-12f) ? (S - P) * fast_rcp(om) : 0.0f;
        f4 go = f4{w * Gr, w * Gg, w * Gb, fmaf(Tr, q, -behind)};
        Tr *= om;
        go = f4{go.x * act_bwd<PR_RACT>(pre.x, o.x), go.y * act_bwd<PR_RACT>(pre.y, o.y), go.z * act_bwd<PR_RACT>(pre.z, o.z),
                go.w * act_bwd<PR_AACT>(pre.w, o.w)};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (tp.w[i] != 0.0f)
                atomic_add_grad_texel<F16>(gplane, (size_t)tp.off + ((i & 1) ? gst.dx : 0u) + ((i & 2) ? gst.dy : 0u), go * tp.w[i]);
    }
}

// scratch: bwd_plan_k's records | one int4 window per (30 x 14-pixel tile, plane) | (256-byte aligned) owner table, one uint16 per local texel,
// padded like vl3d_render_bwd's (the gather's unconditional owner read runs up to 16 rows + 32 texels past a window's corner)
int64_t plane_rows_owner_off(const vl3d_render_desc *d) {
    const int64_t tiles = (int64_t)((d->W + 29) / 30) * ((d->H + 13) / 14);
    const int64_t b = (int64_t)plan_win_off(d->D) * sizeof(float) + tiles * d->D * 16;
    return (b + 255) & ~(int64_t)255;
}

int check_plane_rows_desc(const vl3d_render_desc *d, const int32_t *plane_row0, int32_t R) {
    VL3D_REQUIRE(d != nullptr && plane_row0 != nullptr, "null render desc or plane_row0 table");
    VL3D_REQUIRE(d->D > 0 && d->T > 0 && d->Hs > 0 && d->Ws > 0 && d->H > 0 && d->W > 0, "non-positive render dims");
    VL3D_REQUIRE(d->Hs >= 2 && R >= 2 && R <= d->Hs, "per-plane row windows: 2 <= R <= Hs");
    VL3D_REQUIRE((int64_t)R * d->Ws * 16 < (1ll << 32) && d->Hs < (1 << 24) && d->Ws < (1 << 24), "plane window too large for 32-bit byte offsets");
    VL3D_REQUIRE(d->stack_dtype == VL3D_F32 || (d->stack_dtype == VL3D_F16 && d->Ws >= 2), "stack_dtype must be VL3D_F32, or VL3D_F16 with Ws >= 2");
    VL3D_REQUIRE(d->coord_mode == VL3D_COORD_AFFINE && d->border_mode == VL3D_BORDER_HARDCUT && d->act_order == VL3D_ACT_POST &&
                     d->rgb_act == VL3D_ACT_SIGMOID && d->alpha_act == VL3D_ACT_SIGMOID,
                 "per-plane row windows: the planar MPV convention only (affine, hardcut, post, sigmoid / sigmoid)");
    VL3D_REQUIRE(d->variant == 0 && d->uv_noise_seed == 0 && d->grad_flags == 0 && d->cull_Hs == 0 && d->cull_Ws == 0,
                 "per-plane row windows: no kernel variants, uv noise or tile culling");
    return VL3D_OK;
}

}  // namespace

extern "C" int vl3d_render_fwd_plane_rows(const vl3d_render_desc *desc, const void *stack, const int32_t *plane_row0, int32_t R, const float *homos,
                                          float *rgb, float *alpha, vl3d_stream_t stream) {
    int rc = check_plane_rows_desc(desc, plane_row0, R);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(stack && homos && rgb && alpha, "null pointer passed to vl3d_render_fwd_plane_rows");
    RenderArgs a = render_args_of(desc);      // (a.uv_seed is 0: check_plane_rows_desc)
    a.g_f16 = desc->stack_dtype == VL3D_F16;
    a.stack = (const float *)stack; a.homos = homos; a.rgb = rgb; a.alpha = alpha;
    const int tiles_x = (a.W + 63) / 64, tiles_y = (a.H + 7) / 8;
    const dim3 grid((unsigned)(tiles_x * tiles_y * ((a.T + 1) / 2))), block(64 * 8);
    if (a.g_f16)
        hipLaunchKernelGGL(render_fwd_plane_rows_k<true>, grid, block, 0, (hipStream_t)stream, a, plane_row0, (int)R, tiles_x, tiles_y);
    else
        hipLaunchKernelGGL(render_fwd_plane_rows_k<false>, grid, block, 0, (hipStream_t)stream, a, plane_row0, (int)R, tiles_x, tiles_y);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int64_t vl3d_render_plane_rows_scratch_bytes(const vl3d_render_desc *desc, int32_t R) {
    if (!desc || desc->D <= 0 || desc->H <= 0 || desc->W <= 0 || desc->Ws <= 0 || R <= 0) return 0;
    return plane_rows_owner_off(desc) + ((int64_t)desc->D * R * desc->Ws + 16 * (int64_t)desc->Ws + 64) * 2;
}

extern "C" int vl3d_render_bwd_plane_rows(const vl3d_render_desc *desc, const void *stack, const int32_t *plane_row0, int32_t R, const float *homos,
                                          const float *rgb, const float *alpha, const float *grad_rgb, const float *grad_alpha, void *grad_stack,
                                          void *scratch, int64_t scratch_bytes, vl3d_stream_t stream) {
    int rc = check_plane_rows_desc(desc, plane_row0, R);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(stack && homos && rgb && alpha && grad_rgb && grad_stack, "null pointer passed to vl3d_render_bwd_plane_rows");
    const bool f16 = desc->stack_dtype == VL3D_F16;
    RenderArgs a = render_args_of(desc);      // (a.uv_seed is 0: check_plane_rows_desc)
    a.g_f16 = f16;
    a.stack = (const float *)stack; a.homos = homos;
    a.rgb = const_cast<float *>(rgb); a.alpha = const_cast<float *>(alpha);
    a.g_rgb = grad_rgb; a.g_alpha = grad_alpha; a.g_stack = (float *)grad_stack;
    const size_t texels = (size_t)desc->D * desc->T * R * desc->Ws;
    const hipStream_t s = (hipStream_t)stream;
    const dim3 agrid((a.W + TILE_X - 1) / TILE_X, (a.H + TILE_Y - 1) / TILE_Y, a.T), ablock(TILE_X * TILE_Y);
    if (!scratch || scratch_bytes < vl3d_render_plane_rows_scratch_bytes(desc, R)) {      // no plan: the atomics sweep on a cleared gradient
        a.plan = nullptr;
        VL3D_HIP(hipMemsetAsync(grad_stack, 0, texels * (f16 ? 8 : 16), s));
        if (f16) hipLaunchKernelGGL(render_bwd_plane_rows_scatter_k<true>, agrid, ablock, 0, s, a, plane_row0, (int)R);
        else hipLaunchKernelGGL(render_bwd_plane_rows_scatter_k<false>, agrid, ablock, 0, s, a, plane_row0, (int)R);
        VL3D_CHECK_LAUNCH();
        return VL3D_OK;
    }
    // owner-computes frame pairs (launch_pair's sequence): plan, windows (clipped to the local rows), owner table + zero fill, the pair kernel;
    // every kernel after the plan reads its feasibility flag, and the atomics sweep takes the call where it says no
    a.plan = (const float *)scratch;
    a.owner = reinterpret_cast<const unsigned short *>(reinterpret_cast<const char *>(scratch) + plane_rows_owner_off(desc));
    constexpr int RH = 1, IW = 32 - 2 * RH, IH = PROWS - 2 * RH;
    a.tiles_x = (a.W + IW - 1) / IW; a.tiles_y = (a.H + IH - 1) / IH;
    const int nwin = a.tiles_x * a.tiles_y * a.D;
    int *win = reinterpret_cast<int *>(const_cast<float *>(a.plan)) + plan_win_off(a.D);
    hipLaunchKernelGGL((bwd_plan_k<PR_COORD>), dim3(1), dim3(64), 0, s, a, 16, const_cast<float *>(a.plan));
    hipLaunchKernelGGL(bwd_fill_zero_if_infeasible_k, dim3(4096), dim3(256), 0, s, reinterpret_cast<float2 *>(grad_stack), texels * (f16 ? 1 : 2), a.plan);
    hipLaunchKernelGGL((bwd_windows_k<PR_COORD>), dim3((nwin + 255) / 256), dim3(256), 0, s, a, IW, IH, RH, a.tiles_x, a.tiles_y, win);
    hipLaunchKernelGGL(clip_windows_k, dim3((nwin + 255) / 256), dim3(256), 0, s, reinterpret_cast<int4 *>(win), a.D, a.tiles_x * a.tiles_y, plane_row0,
                       (int)R, a.plan);
    const dim3 ogrid((a.Ws + 63) / 64, (R + 3) / 4, a.D), pgrid((unsigned)(a.tiles_x * a.tiles_y * ((a.T + 1) / 2))), pblock(32 * PROWS);
    if (f16) {
        hipLaunchKernelGGL(owner_table_plane_rows_k<true>, ogrid, dim3(256), 0, s, a, plane_row0, (int)R, IW, IH, RH, const_cast<unsigned short *>(a.owner));
        hipLaunchKernelGGL(render_bwd_pair_plane_rows_k<true>, pgrid, pblock, 0, s, a, plane_row0, (int)R);
        hipLaunchKernelGGL(render_bwd_plane_rows_scatter_k<true>, agrid, ablock, 0, s, a, plane_row0, (int)R);
    } else {
        hipLaunchKernelGGL(owner_table_plane_rows_k<false>, ogrid, dim3(256), 0, s, a, plane_row0, (int)R, IW, IH, RH, const_cast<unsigned short *>(a.owner));
        hipLaunchKernelGGL(render_bwd_pair_plane_rows_k<false>, pgrid, pblock, 0, s, a, plane_row0, (int)R);
        hipLaunchKernelGGL(render_bwd_plane_rows_scatter_k<false>, agrid, ablock, 0, s, a, plane_row0, (int)R);
    }
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
