// Camera gradients of the fused render and of warp_homography: d loss / d homographies (include/vl3d.h vl3d_render_bwd_homos, vl3d_warp_bwd_homos).
//
// Replaces (reference, /root/reference): the autograd of utils_mpi.py:159-176 (warp_homography: grid_sample passes a gradient to its grid, and
// through it to `homos`) under the composite utils_mpi.py:92-107, and of the planar render MPV.py:351-454.
//
// Per output pixel (u, v) = (col0 + x + c, row0 + y + c), plane d and frame t: (X, Y, Z) = H_d (u, v, 1), tx = sx X / Z + ox, ty likewise.  The
// sample's derivative with respect to its coordinate is the derivative of the tent weights in the cell [floor(tx), floor(tx) + 1) -- ATen's
// grid_sample rule: floor carries no gradient, fx = tx - floor(tx) does -- with a tap outside the texture counting as 0:
//     ds/dtx = sum_taps value_i dwx_i wy_i,   ds/dty = sum_taps value_i wx_i dwy_i
// (values: the texels, or the activated texels under VL3D_ACT_PRE).  g_pre, the gradient of the loss with respect to the sampled values, is the
// quantity vl3d_render_bwd scatters with the tent weights: render_bwd_k's sweep, statement for statement -- make_taps2 (coordinates, hard cut,
// kept-quad test), shade2, the (S - P) rcp(1 - a) form of the planes behind with its look-ahead (composite_behind), act' under VL3D_ACT_POST.
// Coverage and quad membership are step functions: no gradient.  With g_tx = sum_t sum_c g_pre_c ds_c/dtx:
//     a = g_tx sx / Z,  b = g_ty sy / Z,  e = -(g_tx sx X + g_ty sy Y) / Z^2,   dL/dH_d = sum_pixels (a, b, e)^T (u, v, 1)
//
// One workgroup per tile of 64 x 4 pixels, one wave per pixel row; a thread takes the frames of its pixel one after the other and walks the
// planes front to back with walk_planes, the next plane's taps in flight.  (Two frames per thread, as the frame-pair kernels hold them, were
// tried: with the second set of prefetched taps hipcc spills 48-200 bytes per lane at the 128-register budget in every instantiation.)
// Reduction, no float atomics, the same bits on every call:
//   * per plane and frame, six sums over each row of 16 lanes with DPP adds (a butterfly: a fixed order).  The 64 lanes are consecutive
//     pixels of one pixel row, so sum a u = u0 sum a + sum a lane and sum a v = v sum a: (sum a, sum a lane) for each of a, b, e;
//   * each row of lanes adds them to its own slot of an LDS table [D][4 waves][4 rows][6], frame after frame;
//   * after the last frame the workgroup folds the slots in wave and row order (in fp64: u0 and v are exact) and stores one [D][9] partial;
//   * cam_finish_k: per record (plane, or image of a warp) 9 x 28 threads sum the partials of workgroups j, j + 28, ... in fp64, then the
//     28 sums in order, and write fp32.
#include "vl3d_render_cam_common.h"

using namespace vl3d_cam_detail;

namespace {

constexpr int CAM_FIN = 28;          // the finish kernel's strided sums per entry: 9 x 28 = 252 threads

struct CamArgs {
    float sxe, sye;        // d tx / d (X / Z), d ty / d (Y / Z): desc->sx, sy (affine), (Ws - 1) / Ws, (Hs - 1) / Hs (utils_mpi)
    float *partial;        // [workgroups][D][9]
};

template <int COORD, int BORDER, int ORDER, int RACT, int AACT>
__global__ __launch_bounds__(64 * CAM_TY, 4) void render_bwd_homos_k(RenderArgs a, CamArgs c, int tiles_x) {      // >= 4 waves per SIMD: <= 128 VGPRs
    extern __shared__ float red[];      // [D][CAM_TY waves][4 rows of 16 lanes][6 sums]: 384 bytes per plane
    for (int i = threadIdx.x; i < a.D * CAM_TY * 24; i += 64 * CAM_TY) red[i] = 0.0f;
    __syncthreads();
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, tile_y = b / tiles_x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = tile_x * 64 + lane, y = tile_y * CAM_TY + wv;
    const bool inside = x < a.W && y < a.H;      // (no thread leaves: the waves reduce across their lanes and the workgroup meets at the barrier)
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const size_t frame_b = (size_t)a.Hs * a.Ws * 16, plane_stride_b = (size_t)a.T * frame_b;
    const TapStep st = make_tap_step<false>(a.Hs, a.Ws);
    const float lanef = (float)lane;
    for (int t = 0; t < a.T; ++t) {
        const char *plane = reinterpret_cast<const char *>(a.stack) + (size_t)t * frame_b;
        const size_t pix = inside ? ((size_t)t * a.H + y) * a.W + x : 0;      // (a pixel outside the image reads pixel 0 and counts nothing)
        const float Gr = a.g_rgb[pix * 3 + 0], Gg = a.g_rgb[pix * 3 + 1], Gb = a.g_rgb[pix * 3 + 2];
        const float gA = a.g_alpha ? a.g_alpha[pix] : 0.0f;
        // S = sum_k w_k q_k with q_k = G.c_k + gA  ==  G.C + gA A from the saved forward outputs
        const float S = dot3p(Gr, a.rgb[pix * 3 + 0], Gg, a.rgb[pix * 3 + 1], Gb, a.rgb[pix * 3 + 2], gA * a.alpha[pix]);
        float Tr = 1.0f, P = 0.0f;
        auto fetch = [&](int d, CamSlot &s) {
            float h[VL3D_HN];
            load_uniform(a.homos + VL3D_HS * d, h);
            s.t = make_taps2<COORD, BORDER>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy, plane_cull(a, d), UvNoise{0u, d});
            load_taps2<false>(plane + (size_t)d * plane_stride_b, s.t, st, s.v);
            asm volatile("" ::: "memory");
        };
        auto step = [&](const CamSlot &s, int d) {
            const bool on = inside && s.t.cov != 0.0f;
            if (__builtin_amdgcn_ballot_w64(on) == 0) return;      // wave-uniform: no sample of the row segment is covered
            float va = 0.0f, vb = 0.0f, ve = 0.0f;
            if (on) {
                // the tent weights per axis (make_taps_i's statements on the coordinates it returns) and their slopes
                const float x0f = __builtin_amdgcn_fmed3f(floorf(s.t.tx), 0.0f, (float)max(a.Ws - 2, 0));
                const float y0f = __builtin_amdgcn_fmed3f(floorf(s.t.ty), 0.0f, (float)max(a.Hs - 2, 0));
                const float dx = s.t.tx - x0f, dy = s.t.ty - y0f;
                const float wx0 = tent_weight(dx), wx1 = tent_weight(dx - (a.Ws > 1 ? 1.0f : 3e38f));
                const float wy0 = tent_weight(dy), wy1 = tent_weight(dy - (a.Hs > 1 ? 1.0f : 3e38f));
                float sx0, sx1, sy0, sy1;
                tent_slopes(dx, a.Ws > 1, sx0, sx1);
                tent_slopes(dy, a.Hs > 1, sy0, sy1);
                const f4 Dx = f4{sx0, sx1, sx0, sx1} * f4{wy0, wy0, wy1, wy1}, Dy = f4{wx0, wx1, wx0, wx1} * f4{sy0, sy0, sy1, sy1};
                f4 pre;
                const f4 o = shade2<ORDER, RACT, AACT>(s.t, s.v, &pre);
                const float q = dot3p(Gr, o.x, Gg, o.y, Gb, o.z, gA);
                const float w = o.w * Tr;
                P = fmaf(w, q, P);
                const float om = 1.0f - o.w;
                // dL/da_k = T_k q_k - (sum_{j>k} w_j q_j) / (1 - a_k): render_bwd_k's statements
                float behind;
                if constexpr (AACT != VL3D_ACT_SIGMOID) {
                    behind = om >= BEHIND_QUOTIENT_FROM ? (S - P) * fast_rcp(om)
                                                        : Tr * composite_behind<COORD, BORDER, ORDER, RACT, AACT, false, true>(
                                                                   a, d, plane + (size_t)(d + 1) * plane_stride_b, plane_stride_b, px, py, st, Gr, Gg, Gb, gA, 0u);
                } else {
                    behind = (om > 1e-12f) ? (S - P) * fast_rcp(om) : 0.0f;
                }
                f4 go = f4{w * Gr, w * Gg, w * Gb, fmaf(Tr, q, -behind)};      // grad wrt the activated (c, a)
                Tr *= om;
                f4 dsx, dsy;      // d (sampled value) / d tx, d ty, per channel
                if constexpr (ORDER == VL3D_ACT_POST) {
                    go = f4{go.x * act_bwd<RACT>(pre.x, o.x), go.y * act_bwd<RACT>(pre.y, o.y), go.z * act_bwd<RACT>(pre.z, o.z),
                            go.w * act_bwd<AACT>(pre.w, o.w)};
                    dsx = s.v[0] * Dx[0] + (s.v[1] * Dx[1] + (s.v[2] * Dx[2] + s.v[3] * Dx[3]));
                    dsy = s.v[0] * Dy[0] + (s.v[1] * Dy[1] + (s.v[2] * Dy[2] + s.v[3] * Dy[3]));
                } else {
                    const f4 a0 = act4<RACT, AACT>(s.v[0]), a1 = act4<RACT, AACT>(s.v[1]), a2 = act4<RACT, AACT>(s.v[2]), a3 = act4<RACT, AACT>(s.v[3]);
                    dsx = a0 * Dx[0] + (a1 * Dx[1] + (a2 * Dx[2] + a3 * Dx[3]));
                    dsy = a0 * Dy[0] + (a1 * Dy[1] + (a2 * Dy[2] + a3 * Dy[3]));
                }
                const float gtx = fmaf(go.x, dsx.x, fmaf(go.y, dsx.y, fmaf(go.z, dsx.z, go.w * dsx.w)));
                const float gty = fmaf(go.x, dsy.x, fmaf(go.y, dsy.y, fmaf(go.z, dsy.z, go.w * dsy.w)));
                float h[VL3D_HN];
                load_uniform(a.homos + VL3D_HS * d, h);
                const float X = fmaf(h[0], px, fmaf(h[1], py, h[2])), Y = fmaf(h[3], px, fmaf(h[4], py, h[5])), Z = fmaf(h[6], px, fmaf(h[7], py, h[8]));
                const float rz = fast_rcp(Z);
                va = gtx * c.sxe * rz;
                vb = gty * c.sye * rz;
                ve = -fmaf(va, X, vb * Y) * rz;
            }
            // six sums over each row of 16 lanes (DPP adds alone); lane k < 6 of a row adds sum k to the row's own slot: nobody else touches it
            const float s0 = cam_row_sum(va), s1 = cam_row_sum(va * lanef), s2 = cam_row_sum(vb), s3 = cam_row_sum(vb * lanef),
                        s4 = cam_row_sum(ve), s5 = cam_row_sum(ve * lanef);
            const int k = lane & 15;
            if (k < 6) {
                const float sk = k == 0 ? s0 : (k == 1 ? s1 : (k == 2 ? s2 : (k == 3 ? s3 : (k == 4 ? s4 : s5))));
                red[((d * CAM_TY + wv) * 4 + (lane >> 4)) * 6 + k] += sk;
            }
        };
        CamSlot sA, sB;
        walk_planes(DensePlanes{a.D}, sA, sB, fetch, step);
    }
    __syncthreads();
    const double u0 = (double)(a.col0 + tile_x * 64) + (double)a.pc, v0 = (double)(a.row0 + tile_y * CAM_TY) + (double)a.pc;
    for (int i = threadIdx.x; i < a.D * 9; i += 64 * CAM_TY) {
        const int d = i / 9, e = i - 9 * d, r = e / 3, j = e - 3 * r;
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < CAM_TY; ++w) {      // wave order, then the wave's four rows of lanes in order
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float *rr = red + ((d * CAM_TY + w) * 4 + q) * 6;
                const double sa = (double)rr[2 * r], sl = (double)rr[2 * r + 1];
                s += j == 0 ? u0 * sa + sl : (j == 1 ? (v0 + (double)w) * sa : sa);
            }
        }
        c.partial[(size_t)b * a.D * 9 + i] = (float)s;
    }
}

// warp_homography (csrc/vl3d_ops.hip warp_taps: the utils_mpi coordinates at pixel centre 0, zeros border, C channel-planar images): the same
// sums with g_pre = the upstream gradient of image n itself.  Grid (tiles, N); partial [N][tiles][9].
__global__ __launch_bounds__(64 * CAM_TY) void warp_bwd_homos_k(int C, int Hs, int Ws, int h, int w, const float *__restrict__ homos,
                                                              const float *__restrict__ images, const float *__restrict__ gout,
                                                              float *__restrict__ partial, int tiles_x) {
    __shared__ float red[CAM_TY][6];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x, n = blockIdx.y;
    const int x = tile_x * 64 + lane, y = tile_y * CAM_TY + wv;
    const float *hm = homos + 9 * (size_t)n;
    float va = 0.0f, vb = 0.0f, ve = 0.0f;
    if (x < w && y < h) {
        const float px = (float)x, py = (float)y;
        const float X = hm[0] * px + hm[1] * py + hm[2], Y = hm[3] * px + hm[4] * py + hm[5], Z = hm[6] * px + hm[7] * py + hm[8];
        const float tx = texel_coord<VL3D_COORD_UTILS_MPI>(X / Z, (float)Ws / 2.0f, (float)(Ws - 1), 0.f, 0.f);
        const float ty = texel_coord<VL3D_COORD_UTILS_MPI>(Y / Z, (float)Hs / 2.0f, (float)(Hs - 1), 0.f, 0.f);
        if ((tx > -1.0f) && (tx < (float)Ws) && (ty > -1.0f) && (ty < (float)Hs)) {
            const float fx0 = floorf(tx), fy0 = floorf(ty), fx = tx - fx0, fy = ty - fy0;
            const int x0 = (int)fx0, y0 = (int)fy0;
            const bool xl = x0 >= 0, xr = x0 + 1 < Ws, yt = y0 >= 0, yb = y0 + 1 < Hs;
            const int base = y0 * Ws + x0;
            const size_t splane = (size_t)Hs * Ws, oplane = (size_t)h * w;
            const float *img = images + (size_t)n * C * splane;
            const float *go = gout + (size_t)n * C * oplane + (size_t)y * w + x;
            float gtx = 0.0f, gty = 0.0f;
            for (int ch = 0; ch < C; ++ch, img += splane, go += oplane) {
                const float s00 = (xl && yt) ? img[base] : 0.0f, s10 = (xr && yt) ? img[base + 1] : 0.0f;
                const float s01 = (xl && yb) ? img[base + Ws] : 0.0f, s11 = (xr && yb) ? img[base + Ws + 1] : 0.0f;
                const float g = *go;
                gtx = fmaf(g, fmaf(s11 - s01, fy, (s10 - s00) * (1.0f - fy)), gtx);
                gty = fmaf(g, fmaf(s11 - s10, fx, (s01 - s00) * (1.0f - fx)), gty);
            }
            const float rz = fast_rcp(Z);
            va = gtx * ((float)(Ws - 1) / (float)Ws) * rz;
            vb = gty * ((float)(Hs - 1) / (float)Hs) * rz;
            ve = -fmaf(va, X, vb * Y) * rz;
        }
    }
    const float lanef = (float)lane;
    const float s0 = cam_wave_sum(va), s1 = cam_wave_sum(va * lanef), s2 = cam_wave_sum(vb), s3 = cam_wave_sum(vb * lanef),
                s4 = cam_wave_sum(ve), s5 = cam_wave_sum(ve * lanef);
    if (lane == 0) {
        float *r = red[wv];
        r[0] = s0; r[1] = s1; r[2] = s2; r[3] = s3; r[4] = s4; r[5] = s5;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int e = threadIdx.x, r = e / 3, j = e - 3 * r;
        const double u0 = (double)(tile_x * 64), v0 = (double)(tile_y * CAM_TY);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < CAM_TY; ++k) {
            const double sa = (double)red[k][2 * r], sl = (double)red[k][2 * r + 1];
            s += j == 0 ? u0 * sa + sl : (j == 1 ? (v0 + (double)k) * sa : sa);
        }
        partial[((size_t)n * gridDim.x + blockIdx.x) * 9 + e] = (float)s;
    }
}

// record r (blockIdx.x): out[r][e] = sum over the workgroups' partials partial[wg * wg_stride + r * rec_stride + e], in fp64: thread (e, j)
// takes workgroups j, j + 28, ... in rising order, thread e then the 28 sums in order.  A fixed order: the same bits on every call.
__global__ __launch_bounds__(256) void cam_finish_k(const float *__restrict__ partial, int nwg, size_t wg_stride, size_t rec_stride,
                                                   float *__restrict__ out) {
    __shared__ double part[CAM_FIN][9];
    const int e = threadIdx.x % 9, j = threadIdx.x / 9;
    if (j < CAM_FIN) {
        const float *p = partial + (size_t)blockIdx.x * rec_stride + e;
        double s = 0.0;
        for (int wg = j; wg < nwg; wg += CAM_FIN) s += (double)p[(size_t)wg * wg_stride];
        part[j][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        double s = 0.0;
        for (int k = 0; k < CAM_FIN; ++k) s += part[k][threadIdx.x];
        out[(size_t)blockIdx.x * 9 + threadIdx.x] = (float)s;
    }
}

template <int COORD, int BORDER, int ORDER>
int launch_cam(const vl3d_render_desc *d, const RenderArgs &a, const CamArgs &c, int tiles_x, int tiles, hipStream_t s, const char *who) {
#define VL3D_CASE(R, A)                                                                                                             \
    if (d->rgb_act == R && d->alpha_act == A) {                                                                                     \
        hipLaunchKernelGGL((render_bwd_homos_k<COORD, BORDER, ORDER, R, A>), dim3(tiles), dim3(64 * CAM_TY),                       \
                           (size_t)d->D * CAM_TY * 24 * sizeof(float), s, a, c, tiles_x);                                          \
        return VL3D_OK;                                                                                                             \
    }
    // the activation table of the render conventions (vl3d_render_conv.inc)
    VL3D_CASE(VL3D_ACT_SIGMOID, VL3D_ACT_SIGMOID)
    VL3D_CASE(VL3D_ACT_NONE, VL3D_ACT_NONE)
    VL3D_CASE(VL3D_ACT_NONE, VL3D_ACT_SIGMOID)
    VL3D_CASE(VL3D_ACT_CLAMP, VL3D_ACT_SIGMOID)
    VL3D_CASE(VL3D_ACT_RELU, VL3D_ACT_SIGMOID)
    VL3D_CASE(VL3D_ACT_ABS, VL3D_ACT_SIGMOID)
    VL3D_CASE(VL3D_ACT_CLAMP, VL3D_ACT_CLAMP)
    VL3D_CASE(VL3D_ACT_SIGMOID, VL3D_ACT_CLAMP)
    VL3D_CASE(VL3D_ACT_NONE, VL3D_ACT_CLAMP)
#undef VL3D_CASE
    return unsupported(who, "unsupported (rgb_act, alpha_act) pair");
}

}  // namespace

extern "C" int64_t vl3d_render_bwd_homos_scratch_bytes(const vl3d_render_desc *desc) {
    if (!desc || desc->D <= 0 || desc->H <= 0 || desc->W <= 0) return 0;
    return cam_tiles(desc->H, desc->W) * desc->D * 9 * (int64_t)sizeof(float);
}

extern "C" int vl3d_render_bwd_homos(const vl3d_render_desc *desc, const void *stack, const float *homos, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                                     const float *rgb, const float *alpha, const float *grad_rgb, const float *grad_alpha, float *grad_homos,
                                     void *scratch, int64_t scratch_bytes, vl3d_stream_t stream) {
    const char *who = "vl3d_render_bwd_homos";
    if (!quad_keep) QH = QW = 0;
    int rc = check_cam(desc, quad_keep, QH, QW, who);
    if (rc != VL3D_OK) return rc;
    if (!(stack && homos && rgb && alpha && grad_rgb && grad_homos && scratch)) return refuse(who, "null pointer");
    if (!(aligned(stack, 16) && aligned(homos, 4) && aligned(rgb, 4) && aligned(alpha, 4) && aligned(grad_rgb, 4) && aligned(grad_alpha, 4) &&
          aligned(grad_homos, 4) && aligned(scratch, 4)))
        return refuse(who, "misaligned pointer (stack: 16 bytes; floats and scratch: 4)");
    if (scratch_bytes < vl3d_render_bwd_homos_scratch_bytes(desc)) return refuse(who, "scratch smaller than vl3d_render_bwd_homos_scratch_bytes");
    RenderArgs a = render_args_of(desc);
    a.stack = static_cast<const float *>(stack); a.homos = homos; a.rgb = const_cast<float *>(rgb); a.alpha = const_cast<float *>(alpha);
    a.g_rgb = grad_rgb; a.g_alpha = grad_alpha;
    a.quad_keep = quad_keep;
    if (quad_keep) set_cull_geometry(a, desc, QH, QW);
    const bool utils = desc->coord_mode == VL3D_COORD_UTILS_MPI;
    const CamArgs c{utils ? (float)(desc->Ws - 1) / (float)desc->Ws : desc->sx, utils ? (float)(desc->Hs - 1) / (float)desc->Hs : desc->sy,
                    static_cast<float *>(scratch)};
    const int tiles_x = (desc->W + 63) / 64, tiles = (int)cam_tiles(desc->H, desc->W);
    rc = utils ? launch_cam<VL3D_COORD_UTILS_MPI, VL3D_BORDER_ZEROS, VL3D_ACT_PRE>(desc, a, c, tiles_x, tiles, (hipStream_t)stream, who)
               : launch_cam<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, VL3D_ACT_POST>(desc, a, c, tiles_x, tiles, (hipStream_t)stream, who);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_finish_k, dim3(desc->D), dim3(256), 0, (hipStream_t)stream, c.partial, tiles, (size_t)desc->D * 9, (size_t)9, grad_homos);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int64_t vl3d_warp_bwd_homos_scratch_bytes(int32_t N, int32_t h, int32_t w) {
    if (N <= 0 || h <= 0 || w <= 0) return 0;
    return cam_tiles(h, w) * N * 9 * (int64_t)sizeof(float);
}

extern "C" int vl3d_warp_bwd_homos(int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t h, int32_t w, const float *homos, const float *images,
                                   const float *grad_out, float *grad_homos, void *scratch, int64_t scratch_bytes, vl3d_stream_t stream) {
    const char *who = "vl3d_warp_bwd_homos";
    if (!(N > 0 && C > 0 && Hs > 0 && Ws > 0 && h > 0 && w > 0)) return refuse(who, "non-positive dims");
    if (N > 65535) return refuse(who, "B*D > 65535");
    if (!((int64_t)Hs * Ws < (1ll << 31))) return refuse(who, "image too large for 32-bit texel indices");
    if (cam_tiles(h, w) > 0x7fffffffll) return refuse(who, "tiles exceed the grid");
    if (!(homos && images && grad_out && grad_homos && scratch)) return refuse(who, "null pointer");
    if (!(aligned(homos, 4) && aligned(images, 4) && aligned(grad_out, 4) && aligned(grad_homos, 4) && aligned(scratch, 4)))
        return refuse(who, "misaligned pointer (floats and scratch: 4 bytes)");
    if (scratch_bytes < vl3d_warp_bwd_homos_scratch_bytes(N, h, w)) return refuse(who, "scratch smaller than vl3d_warp_bwd_homos_scratch_bytes");
    const int tiles_x = (w + 63) / 64, tiles = (int)cam_tiles(h, w);
    float *partial = static_cast<float *>(scratch);
    hipLaunchKernelGGL(warp_bwd_homos_k, dim3(tiles, N), dim3(64 * CAM_TY), 0, (hipStream_t)stream, C, Hs, Ws, h, w, homos, images, grad_out, partial, tiles_x);
    VL3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_finish_k, dim3(N), dim3(256), 0, (hipStream_t)stream, partial, tiles, (size_t)9, (size_t)tiles * 9, grad_homos);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
