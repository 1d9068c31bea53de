// Camera normal equations of the fused render (include/vl3d.h vl3d_render_cam_normal): A = sum w J^T J, b = sum w J^T r, cost = sum w r^2 of
// the photometric residual r = rgb - target in P <= 8 camera parameters, given the homographies' tangents dhomos[k] = dH / d theta_k.
//
// The per-pixel Jacobian is not a contraction with one upstream gradient, so vl3d_render_bwd_homos cannot give it: this kernel carries the
// composite backward once per colour channel (upstream gradient e_c, alpha gradient 0).  Per pixel (u, v), plane d and frame t, with
// render_bwd_homos_k's statements (make_taps2, shade2, the (S - P) rcp(1 - a) form of the planes behind with its look-ahead, act' under
// VL3D_ACT_POST, tent_slopes), S_c = rgb_c and P_c the running front-to-back sum of channel c:
//     g_tx^(c) = sum_ch g_pre^(c)_ch ds_ch/dtx          (g_pre^(c): channel c of the sample with weight w = a T, alpha with T c_c - behind_c)
//     dtx_k = sx (dX_k - (X / Z) dZ_k) / Z,   (dX, dY, dZ)_k = dhomos[k][d] (u, v, 1),   dty_k likewise
//     J[c][k] += g_tx^(c) dtx_k + g_ty^(c) dty_k
// The tangents are uniform: scalar loads through the constant address space, like the homographies.
//
// Shape of the work: render_bwd_homos_k's -- tiles of 64 x 4 pixels, one wave per pixel row, walk_planes with the next plane's taps in
// flight, frames one after the other.  J[3][PN] stays in registers over a frame's planes; PN, the register count of the parameters, is a
// template parameter, 6 (a twist) or 8: a runtime P rounds up and the columns past P stay 0 (docs/kernels/K2_render_backward.md, "Camera
// normal equations", says what that buys).
// Reduction, no float atomics, the same bits on every call:
//   * after the last plane of a frame the thread forms the NS = PN (PN + 1) / 2 + PN + 1 products (upper triangle of A by rows, b, cost);
//     each is summed over the lane's row of 16 lanes by four DPP adds (cam_row_sum: a butterfly, a fixed order) -- no ds_bpermute;
//   * lane k of a row keeps sums k, k + 16, k + 32 and adds each group of 16 to the row's own slot of an LDS table [4 waves][4 rows][48]
//     (a slot has one writer: frame after frame in order; the four rows of a wave land in four different groups of 16 banks);
//   * after the last frame the workgroup folds the 16 slots in order in fp64 and stores one partial of NS doubles, laid out [NS][tiles] so that
//     the finish kernel's reads are contiguous;
//   * cam_normal_finish_k: one workgroup per sum, thread j adds the partials of workgroups j, j + 256, ... in rising order in fp64, then a
//     tree over the 256 threads in LDS (a fixed shape), and writes A[k][l], A[l][k], b[k] or cost.
#include "vl3d_render_cam_common.h"

using namespace vl3d_cam_detail;

namespace {

constexpr int NORM_SLOT = 48;        // floats per row-of-lanes slot: the 45 sums of PN = 8, rounded up to three groups of 16
constexpr int norm_sums(int pn) { return pn * (pn + 1) / 2 + pn + 1; }

struct NormArgs {
    float sxe, sye;              // d tx / d (X / Z), d ty / d (Y / Z): CamArgs' of the camera gradient
    const float *dhomos;         // [P][D][3][3]
    const float *target;         // (T,H,W,3)
    const float *weight;         // (T,H,W) or NULL
    double *partial;             // [NS][tiles]
    int P, tiles;
};

// waves per SIMD the kernel is compiled for.  J[3][PN] beside walk_planes' two tap slots fits the standing budget (128 registers, 4 waves) with
// a sigmoid alpha, but for PN = 8 under VL3D_ACT_PRE (the four activated taps are live beside the raw ones: 12 bytes of scratch at 128).
// The other alpha activations carry the look-ahead of composite_behind inside the plane loop (28-88 bytes of scratch at 128): those
// instantiations are compiled for 3 waves (<= 168 registers) rather than spill into the plane loop.
template <int ORDER, int AACT, int PN>
constexpr int norm_waves() { return (AACT == VL3D_ACT_SIGMOID && !(PN == 8 && ORDER == VL3D_ACT_PRE)) ? 4 : 3; }

template <int COORD, int BORDER, int ORDER, int RACT, int AACT, int PN>
__global__ __launch_bounds__(64 * CAM_TY, (norm_waves<ORDER, AACT, PN>())) void render_cam_normal_k(RenderArgs a, NormArgs c, int tiles_x) {
    constexpr int NS = norm_sums(PN);
    static_assert(NS <= NORM_SLOT, "a slot holds three groups of 16 sums");
    __shared__ float red[CAM_TY * 4 * NORM_SLOT];      // [wave][row of 16 lanes][sum]
    for (int i = threadIdx.x; i < CAM_TY * 4 * NORM_SLOT; i += 64 * CAM_TY) red[i] = 0.0f;
    __syncthreads();
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, tile_y = b / tiles_x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = tile_x * 64 + lane, y = tile_y * CAM_TY + wv;
    const bool inside = x < a.W && y < a.H;      // (no thread leaves: the waves reduce across their lanes and the workgroup meets at the barrier)
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const size_t frame_b = (size_t)a.Hs * a.Ws * 16, plane_stride_b = (size_t)a.T * frame_b;
    const TapStep st = make_tap_step<false>(a.Hs, a.Ws);
    const int k16 = lane & 15;
    float *slot = red + (wv * 4 + (lane >> 4)) * NORM_SLOT;
    for (int t = 0; t < a.T; ++t) {
        const char *plane = reinterpret_cast<const char *>(a.stack) + (size_t)t * frame_b;
        const size_t pix = inside ? ((size_t)t * a.H + y) * a.W + x : 0;      // (a pixel outside the image reads pixel 0 and counts nothing)
        const float Sr = a.rgb[pix * 3 + 0], Sg = a.rgb[pix * 3 + 1], Sb = a.rgb[pix * 3 + 2];      // S_c = sum_k w_k c_k: the saved forward picture
        float Tr = 1.0f, Pr = 0.0f, Pg = 0.0f, Pb = 0.0f;
        float J[3][PN];
#pragma unroll
        for (int k = 0; k < PN; ++k) J[0][k] = J[1][k] = J[2][k] = 0.0f;
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
            if (on) {
                // the tent weights per axis and their slopes: render_bwd_homos_k's statements
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
                const float w = o.w * Tr;
                Pr = fmaf(w, o.x, Pr); Pg = fmaf(w, o.y, Pg); Pb = fmaf(w, o.z, Pb);
                const float om = 1.0f - o.w;
                // d C_c / d a_k = T_k c_k - (sum_{j>k} w_j c_j) / (1 - a_k), per channel: render_bwd_k's statement with G = e_c, gA = 0
                float br, bg, bb;
                if constexpr (AACT != VL3D_ACT_SIGMOID) {
                    if (om >= BEHIND_QUOTIENT_FROM) {
                        const float rom = fast_rcp(om);
                        br = (Sr - Pr) * rom; bg = (Sg - Pg) * rom; bb = (Sb - Pb) * rom;
                    } else {      // near an opaque plane: the look-ahead, once per channel (rare: only these pixels pay)
                        br = bg = bb = 0.0f;
#pragma unroll 1
                        for (int ch = 0; ch < 3; ++ch) {
                            const float beh = Tr * composite_behind<COORD, BORDER, ORDER, RACT, AACT, false, true>(
                                                       a, d, plane + (size_t)(d + 1) * plane_stride_b, plane_stride_b, px, py, st, ch == 0 ? 1.0f : 0.0f,
                                                       ch == 1 ? 1.0f : 0.0f, ch == 2 ? 1.0f : 0.0f, 0.0f, 0u);
                            br = ch == 0 ? beh : br; bg = ch == 1 ? beh : bg; bb = ch == 2 ? beh : bb;
                        }
                    }
                } else {
                    const float rom = (om > 1e-12f) ? fast_rcp(om) : 0.0f;
                    br = (Sr - Pr) * rom; bg = (Sg - Pg) * rom; bb = (Sb - Pb) * rom;
                }
                // grad wrt the activated sample: channel c gets w from its own colour, alpha T c_c - behind_c
                float gc[3] = {w, w, w};
                float ga[3] = {fmaf(Tr, o.x, -br), fmaf(Tr, o.y, -bg), fmaf(Tr, o.z, -bb)};
                Tr *= om;
                f4 dsx, dsy;      // d (sampled value) / d tx, d ty, per channel
                if constexpr (ORDER == VL3D_ACT_POST) {
                    gc[0] *= act_bwd<RACT>(pre.x, o.x); gc[1] *= act_bwd<RACT>(pre.y, o.y); gc[2] *= act_bwd<RACT>(pre.z, o.z);
                    const float da = act_bwd<AACT>(pre.w, o.w);
                    ga[0] *= da; ga[1] *= da; ga[2] *= da;
                    dsx = s.v[0] * Dx[0] + (s.v[1] * Dx[1] + (s.v[2] * Dx[2] + s.v[3] * Dx[3]));
                    dsy = s.v[0] * Dy[0] + (s.v[1] * Dy[1] + (s.v[2] * Dy[2] + s.v[3] * Dy[3]));
                } else {
                    const f4 a0 = act4<RACT, AACT>(s.v[0]), a1 = act4<RACT, AACT>(s.v[1]), a2 = act4<RACT, AACT>(s.v[2]), a3 = act4<RACT, AACT>(s.v[3]);
                    dsx = a0 * Dx[0] + (a1 * Dx[1] + (a2 * Dx[2] + a3 * Dx[3]));
                    dsy = a0 * Dy[0] + (a1 * Dy[1] + (a2 * Dy[2] + a3 * Dy[3]));
                }
                const float gtx[3] = {fmaf(gc[0], dsx.x, ga[0] * dsx.w), fmaf(gc[1], dsx.y, ga[1] * dsx.w), fmaf(gc[2], dsx.z, ga[2] * dsx.w)};
                const float gty[3] = {fmaf(gc[0], dsy.x, ga[0] * dsy.w), fmaf(gc[1], dsy.y, ga[1] * dsy.w), fmaf(gc[2], dsy.z, ga[2] * dsy.w)};
                float h[VL3D_HN];
                load_uniform(a.homos + VL3D_HS * d, h);
                const float X = fmaf(h[0], px, fmaf(h[1], py, h[2])), Y = fmaf(h[3], px, fmaf(h[4], py, h[5])), Z = fmaf(h[6], px, fmaf(h[7], py, h[8]));
                const float rz = fast_rcp(Z);
                const float xz = X * rz, yz = Y * rz, cx = c.sxe * rz, cy = c.sye * rz;
#pragma unroll
                for (int k = 0; k < PN; ++k) {
                    if (k < c.P) {      // uniform
                        float dh[9];
                        load_uniform(c.dhomos + ((size_t)k * a.D + d) * 9, dh);
                        const float dX = fmaf(dh[0], px, fmaf(dh[1], py, dh[2])), dY = fmaf(dh[3], px, fmaf(dh[4], py, dh[5])),
                                    dZ = fmaf(dh[6], px, fmaf(dh[7], py, dh[8]));
                        const float dtx = cx * fmaf(-xz, dZ, dX), dty = cy * fmaf(-yz, dZ, dY);
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) J[ch][k] = fmaf(gtx[ch], dtx, fmaf(gty[ch], dty, J[ch][k]));
                    }
                }
            }
        };
        CamSlot sA, sB;
        walk_planes(DensePlanes{a.D}, sA, sB, fetch, step);
        // the frame's products: weight and residual of the pixel (nothing outside the image), then one row sum each
        const float wgt = inside ? (c.weight ? c.weight[pix] : 1.0f) : 0.0f;
        const float rr = inside ? Sr - c.target[pix * 3 + 0] : 0.0f, rg = inside ? Sg - c.target[pix * 3 + 1] : 0.0f,
                    rb = inside ? Sb - c.target[pix * 3 + 2] : 0.0f;
        float mine = 0.0f;
        int i = 0;      // (a constant in every use once the loops below are unrolled)
        auto deposit = [&](float prod) {
            const float s = cam_row_sum(prod);
            mine = (k16 == (i & 15)) ? s : mine;
            if ((i & 15) == 15 || i == NS - 1) {      // the group of 16 is complete: lane k of the row adds sum (group, k) to the row's own slot
                if ((i & ~15) + k16 < NS) slot[(i & ~15) + k16] += mine;
            }
            ++i;
        };
        float wJ[3][PN];
#pragma unroll
        for (int k = 0; k < PN; ++k) { wJ[0][k] = wgt * J[0][k]; wJ[1][k] = wgt * J[1][k]; wJ[2][k] = wgt * J[2][k]; }
#pragma unroll
        for (int k = 0; k < PN; ++k) {
#pragma unroll
            for (int l = k; l < PN; ++l) deposit(fmaf(wJ[0][k], J[0][l], fmaf(wJ[1][k], J[1][l], wJ[2][k] * J[2][l])));
        }
#pragma unroll
        for (int k = 0; k < PN; ++k) deposit(fmaf(wJ[0][k], rr, fmaf(wJ[1][k], rg, wJ[2][k] * rb)));
        deposit(wgt * fmaf(rr, rr, fmaf(rg, rg, rb * rb)));
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < CAM_TY * 4; ++q) s += (double)red[q * NORM_SLOT + threadIdx.x];      // wave order, then the wave's four rows of lanes in order
        c.partial[(size_t)threadIdx.x * c.tiles + b] = s;
    }
}

// sum e (blockIdx.x) of the PN layout -- the upper triangle of A by rows, then b, then the cost: thread j adds the partials of workgroups
// j, j + 256, ... in rising order, then a tree of fixed shape over the threads; out = A [P][P] (both triangles), b [P], cost.  A sum of a
// column past P is all zeros and has no place in `out`: its workgroup leaves.
__global__ __launch_bounds__(256) void cam_normal_finish_k(const double *__restrict__ partial, int tiles, int PN, int P, double *__restrict__ out) {
    __shared__ double part[256];
    const int e = blockIdx.x, NA = PN * (PN + 1) / 2;
    int k = 0, l = 0, where;
    if (e < NA) {
        int r = e;
        while (r >= PN - k) { r -= PN - k; ++k; }
        l = k + r;
        if (l >= P) return;
        where = k * P + l;
    } else if (e < NA + PN) {
        k = e - NA;
        if (k >= P) return;
        where = P * P + k;
    } else {
        where = P * P + P;
    }
    const double *p = partial + (size_t)e * tiles;
    double s = 0.0;
    for (int wg = threadIdx.x; wg < tiles; wg += 256) s += p[wg];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[where] = part[0];
        if (e < NA && l != k) out[l * P + k] = part[0];
    }
}

constexpr int norm_pn(int P) { return P <= 6 ? 6 : 8; }

template <int COORD, int BORDER, int ORDER, int PN>
int launch_normal(const vl3d_render_desc *d, const RenderArgs &a, const NormArgs &c, int tiles_x, hipStream_t s, const char *who) {
#define VL3D_CASE(R, A)                                                                                                             \
    if (d->rgb_act == R && d->alpha_act == A) {                                                                                     \
        hipLaunchKernelGGL((render_cam_normal_k<COORD, BORDER, ORDER, R, A, PN>), dim3(c.tiles), dim3(64 * CAM_TY), 0, s, a, c, tiles_x); \
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

template <int PN>
int launch_normal_conv(const vl3d_render_desc *d, const RenderArgs &a, const NormArgs &c, int tiles_x, hipStream_t s, const char *who) {
    return d->coord_mode == VL3D_COORD_UTILS_MPI ? launch_normal<VL3D_COORD_UTILS_MPI, VL3D_BORDER_ZEROS, VL3D_ACT_PRE, PN>(d, a, c, tiles_x, s, who)
                                                 : launch_normal<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, VL3D_ACT_POST, PN>(d, a, c, tiles_x, s, who);
}

}  // namespace

extern "C" int64_t vl3d_render_cam_normal_scratch_bytes(const vl3d_render_desc *desc, int32_t P) {
    if (!desc || desc->D <= 0 || desc->H <= 0 || desc->W <= 0 || P < 1 || P > 8) return 0;
    return cam_tiles(desc->H, desc->W) * norm_sums(norm_pn(P)) * (int64_t)sizeof(double);
}

extern "C" int vl3d_render_cam_normal(const vl3d_render_desc *desc, const void *stack, const float *homos, const float *dhomos, int32_t P,
                                      const uint8_t *quad_keep, int32_t QH, int32_t QW, const float *rgb, const float *target, const float *weight,
                                      double *out, void *scratch, int64_t scratch_bytes, vl3d_stream_t stream) {
    const char *who = "vl3d_render_cam_normal";
    if (!quad_keep) QH = QW = 0;
    int rc = check_cam(desc, quad_keep, QH, QW, who);
    if (rc != VL3D_OK) return rc;
    if (!(P >= 1 && P <= 8)) return refuse(who, "P (the number of camera parameters) must be in [1, 8]");
    if (!(stack && homos && dhomos && rgb && target && out && scratch)) return refuse(who, "null pointer");
    if (!(aligned(stack, 16) && aligned(homos, 4) && aligned(dhomos, 4) && aligned(rgb, 4) && aligned(target, 4) && aligned(weight, 4) &&
          aligned(out, 8) && aligned(scratch, 8)))
        return refuse(who, "misaligned pointer (stack: 16 bytes; out and scratch: 8; floats: 4)");
    if (scratch_bytes < vl3d_render_cam_normal_scratch_bytes(desc, P)) return refuse(who, "scratch smaller than vl3d_render_cam_normal_scratch_bytes");
    RenderArgs a = render_args_of(desc);
    a.stack = static_cast<const float *>(stack); a.homos = homos; a.rgb = const_cast<float *>(rgb);
    a.quad_keep = quad_keep;
    if (quad_keep) set_cull_geometry(a, desc, QH, QW);
    const bool utils = desc->coord_mode == VL3D_COORD_UTILS_MPI;
    const int tiles_x = (desc->W + 63) / 64, tiles = (int)cam_tiles(desc->H, desc->W);
    const NormArgs c{utils ? (float)(desc->Ws - 1) / (float)desc->Ws : desc->sx, utils ? (float)(desc->Hs - 1) / (float)desc->Hs : desc->sy,
                     dhomos, target, weight, static_cast<double *>(scratch), P, tiles};
    const int PN = norm_pn(P);
    rc = PN == 6 ? launch_normal_conv<6>(desc, a, c, tiles_x, (hipStream_t)stream, who) : launch_normal_conv<8>(desc, a, c, tiles_x, (hipStream_t)stream, who);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_normal_finish_k, dim3(norm_sums(PN)), dim3(256), 0, (hipStream_t)stream, c.partial, tiles, PN, P, out);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
