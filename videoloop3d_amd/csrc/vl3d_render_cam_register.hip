// Camera registration (include/vl3d.h vl3d_render_cam_register): the normal equations of vl3d_render_cam_normal for a target that is not the
// model's own picture frame for frame -- a clip of the same loop started at another time and exposed differently.  Two additions:
//   * long exposure (mode = VL3D_CAM_LONG_EXPOSURE): the residual is taken on the temporal mean, r = g mean_t C + beta - I, against ONE target
//     picture [H][W][3]; the Jacobian is the mean of the frames' Jacobians;
//   * brightness (photo = 1): a log gain a (g = exp a) and a bias beta are two more unknowns, columns g C and 1 beside the P columns g J.
// A [Q][Q], b [Q], cost with Q = P + 2 photo, evaluated at the given (a, beta).  With photo = 0 the point (a, beta) still shapes the residual.
//
// The per-pixel Jacobian is render_cam_normal_k's, statement for statement (make_taps2, shade2, the (S - P) rcp(1 - a) form with its look-ahead,
// act' under VL3D_ACT_POST, tent_slopes, the tangents by scalar loads): tiles of 64 x 4 pixels, one wave per pixel row, walk_planes, frames in
// order, J[3][PN] in registers.  What differs:
//   * in long-exposure mode J is not cleared between frames and three more accumulators hold sum_t C; both are scaled by 1 / T once after the
//     last frame, and the products are deposited once per pixel instead of once per frame;
//   * the brightness columns are not stored in J: they are g C and 1, formed at the deposit;
//   * the sums: first render_cam_normal_k's NS0 = PN (PN + 1) / 2 + PN + 1 (upper triangle of the P x P block by rows, b, cost), then, with
//     photo, 2 PN + 5 more -- (A[k][P], A[k][P+1]) for k < PN, A[P][P], A[P][P+1], A[P+1][P+1], b[P], b[P+1] -- which start a group of 16 of
//     their own.  PN = 8: 45 -> 48, + 21 = 69 of the 80 floats of a slot (five groups of 16); PN = 6: 28 -> 32, + 17 = 49.
// `mode` and `photo` are wave-uniform kernel arguments, not template parameters: they decide only whether J is cleared, when the deposit runs
// and whether its second block runs -- nothing inside the plane loop, where the registers are short -- so the instantiations stay
// render_cam_normal_k's 36 (2 conventions x 9 activation pairs x PN = 6, 8) instead of 144, and one build's register count covers all four
// combinations (docs/kernels/K2_render_backward.md, "Camera registration").
// Reduction as in render_cam_normal_k, no float atomics, the same bits on every call: DPP row sums (cam_row_sum), lane k of a row adds sum
// (group, k) to the row's own LDS slot (one writer), the workgroup folds its 16 slots in order in fp64 into one partial [NS][tiles], and
// cam_register_finish_k adds the partials in a fixed order in fp64.
#include <cmath>
#include "vl3d_render_cam_common.h"

using namespace vl3d_cam_detail;

namespace {

constexpr int REG_SLOT = 80;         // floats per row-of-lanes slot: five groups of 16
constexpr int reg_sums0(int pn) { return pn * (pn + 1) / 2 + pn + 1; }      // the sums without brightness: render_cam_normal_k's
constexpr int reg_sums1(int pn) { return 2 * pn + 5; }                      // the sums the two brightness columns add
constexpr int reg_off1(int pn) { return (reg_sums0(pn) + 15) & ~15; }        // where they start in a slot
constexpr int reg_sums(int pn, int photo) { return reg_sums0(pn) + (photo ? reg_sums1(pn) : 0); }

struct RegArgs {
    float sxe, sye;              // d tx / d (X / Z), d ty / d (Y / Z)
    const float *dhomos;         // [P][D][3][3]
    const float *target;         // per frame: (T,H,W,3); long exposure: (H,W,3)
    const float *weight;         // per frame: (T,H,W); long exposure: (H,W); or NULL
    double *partial;             // [NS][tiles]
    int P, tiles;
    int mode, photo;             // VL3D_CAM_PER_FRAME / VL3D_CAM_LONG_EXPOSURE; 0 / 1
    float gain, bias;            // g = exp(log_gain), beta
};

// waves per SIMD: render_cam_normal_k's rule (csrc/vl3d_render_cam_normal.hip, norm_waves)
template <int ORDER, int AACT, int PN>
constexpr int reg_waves() { return (AACT == VL3D_ACT_SIGMOID && !(PN == 8 && ORDER == VL3D_ACT_PRE)) ? 4 : 3; }

template <int COORD, int BORDER, int ORDER, int RACT, int AACT, int PN>
__global__ __launch_bounds__(64 * CAM_TY, (reg_waves<ORDER, AACT, PN>())) void render_cam_register_k(RenderArgs a, RegArgs c, int tiles_x) {
    constexpr int NS0 = reg_sums0(PN), NS1 = reg_sums1(PN), OFF1 = reg_off1(PN);
    static_assert(OFF1 + NS1 <= REG_SLOT, "a slot holds five groups of 16 sums");
    __shared__ float red[CAM_TY * 4 * REG_SLOT];      // [wave][row of 16 lanes][sum]
    for (int i = threadIdx.x; i < CAM_TY * 4 * REG_SLOT; i += 64 * CAM_TY) red[i] = 0.0f;
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
    float *slot = red + (wv * 4 + (lane >> 4)) * REG_SLOT;
    const bool longexp = c.mode != 0;      // uniform
    float J[3][PN];
    float Cr = 0.0f, Cg = 0.0f, Cb = 0.0f;      // long exposure: sum_t C
    for (int t = 0; t < a.T; ++t) {
        const char *plane = reinterpret_cast<const char *>(a.stack) + (size_t)t * frame_b;
        const size_t pix = inside ? ((size_t)t * a.H + y) * a.W + x : 0;      // (a pixel outside the image reads pixel 0 and counts nothing)
        const float Sr = a.rgb[pix * 3 + 0], Sg = a.rgb[pix * 3 + 1], Sb = a.rgb[pix * 3 + 2];      // S_c = sum_k w_k c_k: the saved forward picture
        float Tr = 1.0f, Pr = 0.0f, Pg = 0.0f, Pb = 0.0f;
        if (t == 0 || !longexp) {
#pragma unroll
            for (int k = 0; k < PN; ++k) J[0][k] = J[1][k] = J[2][k] = 0.0f;
            Cr = Cg = Cb = 0.0f;
        }
        Cr += Sr; Cg += Sg; Cb += Sb;
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
                // the tent weights per axis and their slopes: render_cam_normal_k's statements
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
                // d C_c / d a_k = T_k c_k - (sum_{j>k} w_j c_j) / (1 - a_k), per channel
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
        if (longexp && t != a.T - 1) continue;      // uniform: the long exposure deposits once, after the last frame
        // the products: the columns g J (long exposure: g mean_t J), the picture g C (g mean_t C), weight and residual of the pixel (nothing
        // outside the image), then one row sum each
        const float inv_t = longexp ? 1.0f / (float)a.T : 1.0f;      // (T = 1: 1, the per-frame mode's bits)
        const size_t tp = longexp ? (inside ? (size_t)y * a.W + x : 0) : pix;
        const float wgt = inside ? (c.weight ? c.weight[tp] : 1.0f) : 0.0f;
        const float gr = c.gain * (Cr * inv_t), gg = c.gain * (Cg * inv_t), gb = c.gain * (Cb * inv_t);
        const float rr = inside ? (gr + c.bias) - c.target[tp * 3 + 0] : 0.0f, rg = inside ? (gg + c.bias) - c.target[tp * 3 + 1] : 0.0f,
                    rb = inside ? (gb + c.bias) - c.target[tp * 3 + 2] : 0.0f;
        float mine = 0.0f;
        int i = 0;      // (a constant in every use once the loops below are unrolled)
        auto deposit = [&](float prod, int base, int n) {      // sum i of the block of n sums that starts at `base` in the slot
            const float s = cam_row_sum(prod);
            mine = (k16 == (i & 15)) ? s : mine;
            if ((i & 15) == 15 || i == n - 1) {      // the group of 16 is complete: lane k of the row adds sum (group, k) to the row's own slot
                if ((i & ~15) + k16 < n) slot[base + (i & ~15) + k16] += mine;
            }
            ++i;
        };
        const float sc = c.gain * inv_t;
        float gJ[3][PN], wJ[3][PN];
#pragma unroll
        for (int k = 0; k < PN; ++k) {
            gJ[0][k] = sc * J[0][k]; gJ[1][k] = sc * J[1][k]; gJ[2][k] = sc * J[2][k];
            wJ[0][k] = wgt * gJ[0][k]; wJ[1][k] = wgt * gJ[1][k]; wJ[2][k] = wgt * gJ[2][k];
        }
#pragma unroll
        for (int k = 0; k < PN; ++k) {
#pragma unroll
            for (int l = k; l < PN; ++l) deposit(fmaf(wJ[0][k], gJ[0][l], fmaf(wJ[1][k], gJ[1][l], wJ[2][k] * gJ[2][l])), 0, NS0);
        }
#pragma unroll
        for (int k = 0; k < PN; ++k) deposit(fmaf(wJ[0][k], rr, fmaf(wJ[1][k], rg, wJ[2][k] * rb)), 0, NS0);
        deposit(wgt * fmaf(rr, rr, fmaf(rg, rg, rb * rb)), 0, NS0);
        if (c.photo) {      // uniform: the columns g C and 1
            i = 0;
#pragma unroll
            for (int k = 0; k < PN; ++k) {
                deposit(fmaf(wJ[0][k], gr, fmaf(wJ[1][k], gg, wJ[2][k] * gb)), OFF1, NS1);
                deposit(wJ[0][k] + (wJ[1][k] + wJ[2][k]), OFF1, NS1);
            }
            deposit(wgt * fmaf(gr, gr, fmaf(gg, gg, gb * gb)), OFF1, NS1);
            deposit(wgt * (gr + (gg + gb)), OFF1, NS1);
            deposit(3.0f * wgt, OFF1, NS1);
            deposit(wgt * fmaf(gr, rr, fmaf(gg, rg, gb * rb)), OFF1, NS1);
            deposit(wgt * (rr + (rg + rb)), OFF1, NS1);
        }
    }
    __syncthreads();
    const int ns = NS0 + (c.photo ? NS1 : 0);
    if ((int)threadIdx.x < ns) {
        const int at = (int)threadIdx.x < NS0 ? (int)threadIdx.x : OFF1 + ((int)threadIdx.x - NS0);
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < CAM_TY * 4; ++q) s += (double)red[q * REG_SLOT + at];      // wave order, then the wave's four rows of lanes in order
        c.partial[(size_t)threadIdx.x * c.tiles + b] = s;
    }
}

// sum e (blockIdx.x) of the layout above: thread j adds the partials of workgroups j, j + 256, ... in rising order, then a tree of fixed shape
// over the threads; out = A [Q][Q] (both triangles), b [Q], cost, Q = P + 2 photo (the grid has the brightness sums only with photo).  A sum
// of a column in [P, PN) is all zeros and has no place in `out`: its workgroup leaves.
__global__ __launch_bounds__(256) void cam_register_finish_k(const double *__restrict__ partial, int tiles, int PN, int P, int Q, double *__restrict__ out) {
    __shared__ double part[256];
    const int e = blockIdx.x, NA = PN * (PN + 1) / 2, NS0 = NA + PN + 1;
    int where, mirror = -1;
    if (e < NA) {
        int k = 0, r = e;
        while (r >= PN - k) { r -= PN - k; ++k; }
        const int l = k + r;
        if (l >= P) return;
        where = k * Q + l;
        mirror = l * Q + k;
    } else if (e < NA + PN) {
        const int k = e - NA;
        if (k >= P) return;
        where = Q * Q + k;
    } else if (e == NA + PN) {
        where = Q * Q + Q;
    } else {
        const int j = e - NS0;
        if (j < 2 * PN) {      // A[k][P], A[k][P + 1]
            const int k = j >> 1, l = P + (j & 1);
            if (k >= P) return;
            where = k * Q + l;
            mirror = l * Q + k;
        } else if (j == 2 * PN) {
            where = P * Q + P;
        } else if (j == 2 * PN + 1) {
            where = P * Q + P + 1;
            mirror = (P + 1) * Q + P;
        } else if (j == 2 * PN + 2) {
            where = (P + 1) * Q + P + 1;
        } else {      // b[P], b[P + 1]
            where = Q * Q + P + (j - (2 * PN + 3));
        }
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
        if (mirror >= 0 && mirror != where) out[mirror] = part[0];
    }
}

constexpr int reg_pn(int P) { return P <= 6 ? 6 : 8; }

template <int COORD, int BORDER, int ORDER, int PN>
int launch_register(const vl3d_render_desc *d, const RenderArgs &a, const RegArgs &c, int tiles_x, hipStream_t s, const char *who) {
#define VL3D_CASE(R, A)                                                                                                               \
    if (d->rgb_act == R && d->alpha_act == A) {                                                                                       \
        hipLaunchKernelGGL((render_cam_register_k<COORD, BORDER, ORDER, R, A, PN>), dim3(c.tiles), dim3(64 * CAM_TY), 0, s, a, c, tiles_x); \
        return VL3D_OK;                                                                                                               \
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
int launch_register_conv(const vl3d_render_desc *d, const RenderArgs &a, const RegArgs &c, int tiles_x, hipStream_t s, const char *who) {
    return d->coord_mode == VL3D_COORD_UTILS_MPI ? launch_register<VL3D_COORD_UTILS_MPI, VL3D_BORDER_ZEROS, VL3D_ACT_PRE, PN>(d, a, c, tiles_x, s, who)
                                                 : launch_register<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT, VL3D_ACT_POST, PN>(d, a, c, tiles_x, s, who);
}

}  // namespace

extern "C" int64_t vl3d_render_cam_register_scratch_bytes(const vl3d_render_desc *desc, int32_t P, int32_t photo) {
    if (!desc || desc->D <= 0 || desc->H <= 0 || desc->W <= 0 || P < 1 || P > 8 || photo < 0 || photo > 1) return 0;
    return cam_tiles(desc->H, desc->W) * reg_sums(reg_pn(P), photo) * (int64_t)sizeof(double);
}

extern "C" int vl3d_render_cam_register(const vl3d_render_desc *desc, const void *stack, const float *homos, const float *dhomos, int32_t P,
                                        const uint8_t *quad_keep, int32_t QH, int32_t QW, const float *rgb, const float *target, const float *weight,
                                        int32_t mode, int32_t photo, float log_gain, float bias,
                                        double *out, void *scratch, int64_t scratch_bytes, vl3d_stream_t stream) {
    const char *who = "vl3d_render_cam_register";
    if (!quad_keep) QH = QW = 0;
    int rc = check_cam(desc, quad_keep, QH, QW, who);
    if (rc != VL3D_OK) return rc;
    if (!(P >= 1 && P <= 8)) return refuse(who, "P (the number of camera parameters) must be in [1, 8]");
    if (!(mode == VL3D_CAM_PER_FRAME || mode == VL3D_CAM_LONG_EXPOSURE)) return refuse(who, "mode must be VL3D_CAM_PER_FRAME or VL3D_CAM_LONG_EXPOSURE");
    if (!(photo == 0 || photo == 1)) return refuse(who, "photo must be 0 or 1");
    if (!(std::isfinite(log_gain) && std::isfinite(bias))) return refuse(who, "log_gain and bias must be finite");
    if (!(stack && homos && dhomos && rgb && target && out && scratch)) return refuse(who, "null pointer");
    if (!(aligned(stack, 16) && aligned(homos, 4) && aligned(dhomos, 4) && aligned(rgb, 4) && aligned(target, 4) && aligned(weight, 4) &&
          aligned(out, 8) && aligned(scratch, 8)))
        return refuse(who, "misaligned pointer (stack: 16 bytes; out and scratch: 8; floats: 4)");
    if (scratch_bytes < vl3d_render_cam_register_scratch_bytes(desc, P, photo))
        return refuse(who, "scratch smaller than vl3d_render_cam_register_scratch_bytes");
    const float gain = std::exp(log_gain);
    if (!std::isfinite(gain)) return refuse(who, "exp(log_gain) is not a finite float");
    RenderArgs a = render_args_of(desc);
    a.stack = static_cast<const float *>(stack); a.homos = homos; a.rgb = const_cast<float *>(rgb);
    a.quad_keep = quad_keep;
    if (quad_keep) set_cull_geometry(a, desc, QH, QW);
    const bool utils = desc->coord_mode == VL3D_COORD_UTILS_MPI;
    const int tiles_x = (desc->W + 63) / 64, tiles = (int)cam_tiles(desc->H, desc->W);
    const RegArgs c{utils ? (float)(desc->Ws - 1) / (float)desc->Ws : desc->sx, utils ? (float)(desc->Hs - 1) / (float)desc->Hs : desc->sy,
                    dhomos, target, weight, static_cast<double *>(scratch), P, tiles, mode, photo, gain, bias};
    const int PN = reg_pn(P);
    rc = PN == 6 ? launch_register_conv<6>(desc, a, c, tiles_x, (hipStream_t)stream, who) : launch_register_conv<8>(desc, a, c, tiles_x, (hipStream_t)stream, who);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(cam_register_finish_k, dim3(reg_sums(PN, photo)), dim3(256), 0, (hipStream_t)stream, c.partial, tiles, PN, P, P + 2 * photo, out);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
