// Stage 1's view-dependent colour head (rgb_mlp_type = "rgb_sh") on the fused render: include/vl3d.h vl3d_render_sh_fwd / _bwd.
//
// Replaces (reference, /root/reference): MPI.py:512-513, 526-537 (per-pixel ray directions into SphericalHarmoic_RGB, utils_mpi.py:50-61 with
// the degree-1 basis of eval_sh_bases, utils_mpi.py:365-383), inside the render MPI.py:452-594, and its autograd.
//
// Per output pixel with integer indices (x, y) of the frame (utils.py:182-193: linspace 0 .. W - 1, no half pixel -- the SAMPLE still sits at
// desc->pixel_center):  d = normalize(M (x, y, 1)^T),  b = (C0, -C1 d_y, C1 d_z, -C1 d_x), once per pixel, outside the plane loop.
// Per plane: the taps of the planar convention (make_taps2: the float forward's own sample position, hard cut, kept-quad test and tent weights);
// every tap is four aligned 16-byte loads -- (R0, G0, B0, alpha) of `stack`, then the three (r, g, b, 0) coefficient vectors of `stack_sh` --
// contracted with the basis BEFORE the tent weights (the contraction is linear), so a thread holds one tap's 64 bytes and one f4 per tap;
// then activation x coverage and the front-to-back composite of render_fwd2_k, statement for statement (with stack_sh = 0 the alpha and the
// alpha sums are the shipped kernel's bits).
// Backward: the atomics form of render_bwd_k (one sweep with the saved outputs); per tap with tent weight w
//     d/d coef_{c,k} += w b_k g_pre_c,   d/d alpha += w g_pre_a,   g_pre = act'(pre) g_layer
// added with global_atomic_add_f32 to gradients the entry cleared, a wave-instruction carrying the whole 16-float records of 4 pixels (transposed
// through the wave's own LDS rows: 5.3x the rate of one float per lane and texel at 720p); lane 3 of grad_stack_sh is never touched: an exact
// 0.  Float atomic sums depend on arrival order: this gradient is not bit-reproducible.  A completeness path at T = 1 (docs/kernels/K7_stage1.md, "the view-dependent colour head").
#include <string>
#include "vl3d_render_args.h"

using namespace vl3d_render_detail;

namespace {

constexpr float SH_C0 = 0.28209479177387814f, SH_C1 = 0.4886025119029199f;      // utils_mpi.py:321-322
constexpr int SH_TY = 4;                                                          // 64 x 4 pixels per workgroup, one wave per row segment

struct ShArgs {
    const float *sh;        // stack_sh (D,1,Hs,Ws,3,4)
    const float *ray_m;     // device float[9]: inverse(E)[:3,:3] inverse(K), row-major
    float *g_sh;            // backward: grad_stack_sh, cleared by the entry
    int rgb_act, alpha_act;
};

__device__ __forceinline__ float act_any(int act, float v) {      // (uniform switch: a scalar branch)
    switch (act) {
        case VL3D_ACT_SIGMOID: return act_fwd<VL3D_ACT_SIGMOID>(v);
        case VL3D_ACT_RELU: return act_fwd<VL3D_ACT_RELU>(v);
        case VL3D_ACT_CLAMP: return act_fwd<VL3D_ACT_CLAMP>(v);
        case VL3D_ACT_ABS: return act_fwd<VL3D_ACT_ABS>(v);
        default: return v;
    }
}
__device__ __forceinline__ float act_bwd_any(int act, float v, float o) {
    switch (act) {
        case VL3D_ACT_SIGMOID: return act_bwd<VL3D_ACT_SIGMOID>(v, o);
        case VL3D_ACT_RELU: return act_bwd<VL3D_ACT_RELU>(v, o);
        case VL3D_ACT_CLAMP: return act_bwd<VL3D_ACT_CLAMP>(v, o);
        case VL3D_ACT_ABS: return act_bwd<VL3D_ACT_ABS>(v, o);
        default: return 1.0f;
    }
}

// the degree-1 basis of frame pixel (ix, iy).  Every operation scales exactly with a power of two in M, so M and 2 M give the same bits.
__device__ __forceinline__ f4 sh_basis(const float *ray_m, int ix, int iy) {
    float m[9];
    load_uniform(ray_m, m);
    const float fx = (float)ix, fy = (float)iy;
    const float dx = fmaf(m[0], fx, fmaf(m[1], fy, m[2])), dy = fmaf(m[3], fx, fmaf(m[4], fy, m[5])), dz = fmaf(m[6], fx, fmaf(m[7], fy, m[8]));
    const float rn = 1.0f / sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
    return f4{SH_C0, -SH_C1 * (dy * rn), SH_C1 * (dz * rn), -SH_C1 * (dx * rn)};
}

// one tap: the texel's 64 bytes -> (r, g, b of this view before the activation, alpha logit)
__device__ __forceinline__ f4 sh_tap(const char *__restrict__ p0, const char *__restrict__ psh, f4 b) {
    const f4 v0 = *reinterpret_cast<const f4 *>(p0);
    const f4 v1 = *reinterpret_cast<const f4 *>(psh), v2 = *reinterpret_cast<const f4 *>(psh + 16), v3 = *reinterpret_cast<const f4 *>(psh + 32);
    return f4{fmaf(v3.x, b.w, fmaf(v2.x, b.z, fmaf(v1.x, b.y, v0.x * b.x))), fmaf(v3.y, b.w, fmaf(v2.y, b.z, fmaf(v1.y, b.y, v0.y * b.x))),
              fmaf(v3.z, b.w, fmaf(v2.z, b.z, fmaf(v1.z, b.y, v0.z * b.x))), v0.w};      // (lane 3 of stack_sh is reserved: never read into a value)
}

// the four contracted taps blended with the tent weights, associated like shade2's blend (tap 3 first, then fma 2, 1, 0)
__device__ __forceinline__ f4 sh_sample(const char *__restrict__ plane, const char *__restrict__ shplane, const Taps2 &t, TapStep st, f4 b) {
    const size_t o = t.off, o3 = (size_t)t.off * 3;
    const size_t dx = st.dx, dy = st.dy;
    f4 s = sh_tap(plane + o + dy + dx, shplane + o3 + 3 * (dy + dx), b) * t.w[3];
    s = __builtin_elementwise_fma(sh_tap(plane + o + dy, shplane + o3 + 3 * dy, b), f4{t.w[2], t.w[2], t.w[2], t.w[2]}, s);
    s = __builtin_elementwise_fma(sh_tap(plane + o + dx, shplane + o3 + 3 * dx, b), f4{t.w[1], t.w[1], t.w[1], t.w[1]}, s);
    s = __builtin_elementwise_fma(sh_tap(plane + o, shplane + o3, b), f4{t.w[0], t.w[0], t.w[0], t.w[0]}, s);
    return s;
}

__device__ __forceinline__ f4 sh_activate(const ShArgs &s, f4 pre, float cov) {
    f4 o = f4{act_any(s.rgb_act, pre.x), act_any(s.rgb_act, pre.y), act_any(s.rgb_act, pre.z), act_any(s.alpha_act, pre.w)};
    o.w *= cov;      // uncovered: a = 0 -> the plane drops out of the composite
    return o;
}

template <bool CULL>
__global__ __launch_bounds__(64 * SH_TY, 4) void render_sh_fwd_k(RenderArgs a, ShArgs s, int tiles_x) {      // >= 4 waves per SIMD: <= 128 VGPRs
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, tile_y = b / tiles_x;
    const int x = tile_x * 64 + (threadIdx.x & 63);
    const int y = tile_y * SH_TY + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const f4 bs = sh_basis(s.ray_m, a.col0 + x, a.row0 + y);
    const size_t frame_b = (size_t)a.Hs * a.Ws * 16;
    const char *plane = reinterpret_cast<const char *>(a.stack), *shplane = reinterpret_cast<const char *>(s.sh);
    const TapStep st = make_tap_step<false>(a.Hs, a.Ws);
    float Tr = 1.0f, cr = 0.f, cg = 0.f, cb = 0.f, A = 0.f, n1 = 0.f, n2 = 0.f;
    for (int d = 0; d < a.D; ++d, plane += frame_b, shplane += 3 * frame_b) {
        float h[VL3D_HN];
        load_uniform(a.homos + VL3D_HS * d, h);
        const Taps2 tp = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy,
                                                                            CULL ? plane_cull(a, d) : QuadCull{nullptr, 0, 0, 0.f, 0.f, 0.f, 0.f, 0});
        // a plane no pixel of the wave's row segment is covered by (outside the frame, or culled quads only) fetches nothing: every one of its
        // samples has a = 0, so skipping it changes no bit of the composite
        if (__builtin_amdgcn_ballot_w64(tp.cov != 0.0f) == 0) continue;
        const f4 o = sh_activate(s, sh_sample(plane, shplane, tp, st, bs), tp.cov);
        const float w = o.w * Tr;
        cr += w * o.x; cg += w * o.y; cb += w * o.z; A += w;
        n1 += o.w; n2 = fmaf(o.w, o.w, n2);
        Tr *= (1.0f - o.w);
    }
    const size_t pix = (size_t)y * a.W + x;
    a.rgb[pix * 3 + 0] = cr; a.rgb[pix * 3 + 1] = cg; a.rgb[pix * 3 + 2] = cb;
    a.alpha[pix] = A;
    if (a.asum) { a.asum[pix * 2 + 0] = n1; a.asum[pix * 2 + 1] = n2; }
}

// Backward: render_bwd_k's sweep (the saved outputs give sum_{j>k} w_j q_j) with the atomics SHAPED.  A texel's gradient is a record of 16 floats -- (r0, g0, b0, alpha) for grad_stack, then the 12 floats of
// its grad_stack_sh texel -- and per tap the wave transposes its 64 records through LDS (lane p writes its 16 floats at [16 p], a plain read of
// float [64 j + lane] is float (lane & 15) of pixel 4 j + (lane >> 4)), so that one global_atomic_add_f32 wave-instruction carries whole
// records of 4 pixels: 16 + 48 contiguous bytes per texel, neighbouring pixels' texels contiguous, instead of one float in each of 64 texels.
// Every lane of the wave serves other pixels' floats, so no lane leaves the loop: pixels outside the image and uncovered samples carry the
// offset ~0 (nothing is added).  The wave's LDS rows are its own: a wave-level fence orders its writes and reads, no workgroup barrier.
template <bool CULL>
__global__ __launch_bounds__(64 * SH_TY, 4) void render_sh_bwd_k(RenderArgs a, ShArgs s, int tiles_x) {      // >= 4 waves per SIMD: <= 128 VGPRs
    __shared__ float rec[SH_TY][64 * 16];
    __shared__ unsigned rec_off[SH_TY][64];
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = (b % tiles_x) * 64 + lane;
    const int y = (b / tiles_x) * SH_TY + wv;
    const bool inside = x < a.W && y < a.H;
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const f4 bs = sh_basis(s.ray_m, a.col0 + x, a.row0 + y);
    const size_t frame_b = (size_t)a.Hs * a.Ws * 16;
    const char *plane = reinterpret_cast<const char *>(a.stack), *shplane = reinterpret_cast<const char *>(s.sh);
    char *gplane = reinterpret_cast<char *>(a.g_stack), *gshplane = reinterpret_cast<char *>(s.g_sh);
    const TapStep st = make_tap_step<false>(a.Hs, a.Ws);
    const size_t pix = inside ? (size_t)y * a.W + x : 0;      // (a pixel outside the image reads pixel 0's values and adds nothing)
    const float Gr = a.g_rgb[pix * 3 + 0], Gg = a.g_rgb[pix * 3 + 1], Gb = a.g_rgb[pix * 3 + 2];
    const float gA = a.g_alpha ? a.g_alpha[pix] : 0.0f;
    const float S = dot3p(Gr, a.rgb[pix * 3 + 0], Gg, a.rgb[pix * 3 + 1], Gb, a.rgb[pix * 3 + 2], gA * a.alpha[pix]);
    const float gN1 = a.g_asum ? a.g_asum[pix * 2 + 0] : 0.0f, gN2 = a.g_asum ? 2.0f * a.g_asum[pix * 2 + 1] : 0.0f;
    float Tr = 1.0f, P = 0.0f;
    f4 *my = reinterpret_cast<f4 *>(&rec[wv][lane * 16]);
    const int f = lane & 15;                                  // the float of the record this lane adds: 0-3 grad_stack, 4-15 grad_stack_sh
    const bool adds = f < 4 || (f & 3) != 3;                  // (lane 3 of a stack_sh vector is reserved: never touched)
    for (int d = 0; d < a.D; ++d, plane += frame_b, shplane += 3 * frame_b, gplane += frame_b, gshplane += 3 * frame_b) {
        float h[VL3D_HN];
        load_uniform(a.homos + VL3D_HS * d, h);
        const Taps2 tp = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy,
                                                                            CULL ? plane_cull(a, d) : QuadCull{nullptr, 0, 0, 0.f, 0.f, 0.f, 0.f, 0});
        const bool on = inside && tp.cov != 0.0f;
        if (__builtin_amdgcn_ballot_w64(on) == 0) continue;      // wave-uniform: no sample of the row segment is covered
        f4 gp = f4{0.f, 0.f, 0.f, 0.f};
        if (on) {
            const f4 pre = sh_sample(plane, shplane, tp, st, bs);
            const f4 o = sh_activate(s, pre, tp.cov);
            const float q = dot3p(Gr, o.x, Gg, o.y, Gb, o.z, gA);
            const float w = o.w * Tr;
            P = fmaf(w, q, P);
            const float om = 1.0f - o.w;
            const float behind = (om > 1e-12f) ? (S - P) * fast_rcp(om) : 0.0f;
            const f4 go = f4{w * Gr, w * Gg, w * Gb, fmaf(Tr, q, -behind) + fmaf(gN2, o.w, gN1)};
            Tr *= om;
            gp = f4{go.x * act_bwd_any(s.rgb_act, pre.x, o.x), go.y * act_bwd_any(s.rgb_act, pre.y, o.y),
                    go.z * act_bwd_any(s.rgb_act, pre.z, o.z), go.w * act_bwd_any(s.alpha_act, pre.w, o.w)};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float wi = on ? tp.w[i] : 0.0f;
            const f4 c = gp * wi;
            my[0] = f4{c.x * bs.x, c.y * bs.x, c.z * bs.x, c.w};
            my[1] = f4{c.x * bs.y, c.y * bs.y, c.z * bs.y, 0.f};
            my[2] = f4{c.x * bs.z, c.y * bs.z, c.z * bs.z, 0.f};
            my[3] = f4{c.x * bs.w, c.y * bs.w, c.z * bs.w, 0.f};
            rec_off[wv][lane] = wi != 0.0f ? tp.off + ((i & 1) ? st.dx : 0u) + ((i & 2) ? st.dy : 0u) : 0xffffffffu;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 4
            for (int j = 0; j < 16; ++j) {
                const unsigned off = rec_off[wv][4 * j + (lane >> 4)];
                const float v = rec[wv][64 * j + lane];
                if (off != 0xffffffffu && adds) {
                    float *dst = f < 4 ? reinterpret_cast<float *>(gplane + (size_t)off) + f
                                       : reinterpret_cast<float *>(gshplane + 3 * (size_t)off) + (f - 4);
                    atomicAdd(dst, v);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
}

int unsupported(const char *who, const char *what) {
    vl3d_set_error((std::string(who) + ": " + what).c_str());
    return VL3D_EUNSUPPORTED;
}

// texels are read and written as 16-byte vectors; everything else as floats (homos and ray_m may be two parts of one upload)
bool aligned(const void *p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// what both entries refuse before they launch anything
int check_sh(const vl3d_render_desc *d, const uint8_t *quad_keep, int32_t QH, int32_t QW, const char *who) {
    VL3D_REQUIRE(d != nullptr, "null render desc");
    if (d->variant != 0) return refuse(who, "no kernel variants (desc->variant = 0)");
    if (!(d->D > 0 && d->T > 0 && d->Hs > 0 && d->Ws > 0 && d->H > 0 && d->W > 0)) return refuse(who, "non-positive render dims");
    if (d->D > 128) return refuse(who, "at most 128 planes");
    if (!(d->Hs < (1 << 24) && d->Ws < (1 << 24) && (int64_t)d->Hs * d->Ws * 16 < (1ll << 32))) return refuse(who, "frame too large for 32-bit byte offsets");
    if ((int64_t)((d->W + 63) / 64) * ((d->H + SH_TY - 1) / SH_TY) > 0x7fffffffll) return refuse(who, "tiles exceed the grid");
    if (!(d->rgb_act >= VL3D_ACT_NONE && d->rgb_act <= VL3D_ACT_ABS && d->alpha_act >= VL3D_ACT_NONE && d->alpha_act <= VL3D_ACT_ABS))
        return refuse(who, "rgb_act / alpha_act outside the activation table");
    if (d->T != 1) return unsupported(who, "the view-dependent colour head is stage 1's: a static MPI, T = 1 (MPV.py:431-434 never passes view directions)");
    if (d->stack_dtype != VL3D_F32) return unsupported(who, "fp32 stacks only");
    if (!(d->coord_mode == VL3D_COORD_AFFINE && d->border_mode == VL3D_BORDER_HARDCUT && d->act_order == VL3D_ACT_POST))
        return unsupported(who, "the planar MPI convention only -- (affine, hardcut, post) (MPI.py:452-594)");
    if (d->uv_noise_seed != 0) return unsupported(who, "add_uv_noise is not built for the view-dependent head (uv_noise_seed = 0)");
    if (quad_keep) {
        if (QH < 0 && QW < 0) return unsupported(who, "the tile-exact layout (a negative quad grid) is not built for the view-dependent head");
        if (!(QH > 0 && QW > 0)) return refuse(who, "bad quad grid (both positive)");
        if (d->cull_row0 || d->cull_col0 || d->cull_Hs || d->cull_Ws) return unsupported(who, "the stack is the whole plane (desc->cull_* = 0)");
    }
    return VL3D_OK;
}

}  // namespace

extern "C" int vl3d_render_sh_fwd(const vl3d_render_desc *desc, const float *stack, const float *stack_sh, const float *homos, const float *ray_m,
                                  const uint8_t *quad_keep, int32_t QH, int32_t QW, float *rgb, float *alpha, float *alpha_sums,
                                  vl3d_stream_t stream) {
    const char *who = "vl3d_render_sh_fwd";
    if (!quad_keep) QH = QW = 0;
    int rc = check_sh(desc, quad_keep, QH, QW, who);
    if (rc != VL3D_OK) return rc;
    if (!(stack && stack_sh && homos && ray_m && rgb && alpha)) return refuse(who, "null pointer");
    if (!(aligned(stack, 16) && aligned(stack_sh, 16) && aligned(homos, 4) && aligned(ray_m, 4) && aligned(rgb, 4) && aligned(alpha, 4) && aligned(alpha_sums, 4)))
        return refuse(who, "misaligned pointer (stack, stack_sh: 16 bytes; floats: 4)");
    RenderArgs a = render_args_of(desc);
    a.stack = stack; a.homos = homos; a.rgb = rgb; a.alpha = alpha; a.asum = alpha_sums;
    a.quad_keep = quad_keep;
    if (quad_keep) set_cull_geometry(a, desc, QH, QW);
    const ShArgs s{stack_sh, ray_m, nullptr, desc->rgb_act, desc->alpha_act};
    const int tiles_x = (desc->W + 63) / 64, tiles_y = (desc->H + SH_TY - 1) / SH_TY;
    if (quad_keep) hipLaunchKernelGGL(render_sh_fwd_k<true>, dim3(tiles_x * tiles_y), dim3(64 * SH_TY), 0, (hipStream_t)stream, a, s, tiles_x);
    else hipLaunchKernelGGL(render_sh_fwd_k<false>, dim3(tiles_x * tiles_y), dim3(64 * SH_TY), 0, (hipStream_t)stream, a, s, tiles_x);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_render_sh_bwd(const vl3d_render_desc *desc, const float *stack, const float *stack_sh, const float *homos, const float *ray_m,
                                  const uint8_t *quad_keep, int32_t QH, int32_t QW, const float *rgb, const float *alpha, const float *grad_rgb,
                                  const float *grad_alpha, const float *grad_alpha_sums, float *grad_stack, float *grad_stack_sh,
                                  vl3d_stream_t stream) {
    const char *who = "vl3d_render_sh_bwd";
    if (!quad_keep) QH = QW = 0;
    int rc = check_sh(desc, quad_keep, QH, QW, who);
    if (rc != VL3D_OK) return rc;
    if (!(stack && stack_sh && homos && ray_m && rgb && alpha && grad_rgb && grad_stack && grad_stack_sh)) return refuse(who, "null pointer");
    if (!(aligned(stack, 16) && aligned(stack_sh, 16) && aligned(grad_stack, 16) && aligned(grad_stack_sh, 16) && aligned(homos, 4) && aligned(ray_m, 4) &&
          aligned(rgb, 4) && aligned(alpha, 4) && aligned(grad_rgb, 4) && aligned(grad_alpha, 4) && aligned(grad_alpha_sums, 4)))
        return refuse(who, "misaligned pointer (stack, stack_sh and their gradients: 16 bytes; floats: 4)");
    RenderArgs a = render_args_of(desc);
    a.stack = stack; a.homos = homos; a.rgb = const_cast<float *>(rgb); a.alpha = const_cast<float *>(alpha);
    a.g_rgb = grad_rgb; a.g_alpha = grad_alpha; a.g_asum = grad_alpha_sums; a.g_stack = grad_stack;
    a.quad_keep = quad_keep;
    if (quad_keep) set_cull_geometry(a, desc, QH, QW);
    const ShArgs s{stack_sh, ray_m, grad_stack_sh, desc->rgb_act, desc->alpha_act};
    // the sums are formed with atomics: both gradients start from 0 (texels no covered sample reads, and lane 3 of grad_stack_sh, stay exactly 0)
    const size_t texels = (size_t)desc->D * desc->Hs * desc->Ws;
    VL3D_HIP(hipMemsetAsync(grad_stack, 0, texels * 16, (hipStream_t)stream));
    VL3D_HIP(hipMemsetAsync(grad_stack_sh, 0, texels * 48, (hipStream_t)stream));
    const int tiles_x = (desc->W + 63) / 64, tiles_y = (desc->H + SH_TY - 1) / SH_TY;
    if (quad_keep) hipLaunchKernelGGL(render_sh_bwd_k<true>, dim3(tiles_x * tiles_y), dim3(64 * SH_TY), 0, (hipStream_t)stream, a, s, tiles_x);
    else hipLaunchKernelGGL(render_sh_bwd_k<false>, dim3(tiles_x * tiles_y), dim3(64 * SH_TY), 0, (hipStream_t)stream, a, s, tiles_x);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
