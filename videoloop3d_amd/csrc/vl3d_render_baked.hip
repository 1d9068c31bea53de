// The playback model (include/vl3d.h "Baked playback"): what the viewer package ships and what a player shows.
//
// The reference's export (scripts/script_export_mesh.py:117-191) activates the atlases, multiplies by 255, clips and truncates to 8 bits; a
// player then filters those 8-bit texels bilinearly, AFTER the activation.  Two kernels:
//   * bake_rgba8_k: the bake rule u8 = uint8(trunc(clip(act(s) * 255, 0, 255))), elementwise over the activation table of vl3d_common.h;
//     one 16-byte load and one 4-byte store per fp32 texel (two texels per 16-byte load of an fp16 stack).
//   * render_fwd_baked_k: the forward of MPV.py:351-454 on a (D, T_alloc, Hs, Ws, 4) uint8 stack.  Sample position, hard cut, kept-quad test,
//     tile-exact quad offset and the tent weights are make_taps2 / plane_cull of vl3d_render_core.h -- the float forward's own device functions,
//     called with the float forward's own arguments, so the two renders cannot disagree about the coverage of a pixel --, the plane list of a
//     tile-culled model is cull_fwd_plan_k's.  What differs is the instruction stream behind the taps: a texel is 4 bytes, the two taps of a
//     texel row are ONE 8-byte load (the base tap's x0 <= Ws - 2), a channel is a byte of that word ((w >> 8k) & 0xff: v_cvt_f32_ubyte<k>),
//     the 1 / 255 of the decode is folded into the four blend weights once per plane, and nothing is activated.  The launch shape is the float
//     forward's: 64 x 8 pixels per workgroup, XCD remap, two frames per thread for T >= 2 (an odd tail frame composited twice, stored once).
// Forward only: a baked model is not trained.
#include "vl3d_bake_rule.h"
#include "vl3d_baked_core.h"      // taps, decode, blend, composite step and pixel store: shared with csrc/vl3d_render_baked_pool.hip
#include "vl3d_render_args.h"

using namespace vl3d_render_detail;

namespace {

// ---- bake ---------------------------------------------------------------------------------------------------------------------------------
// (act_rt and bake_channel -- THE bake rule -- live in vl3d_bake_rule.h: the render core's VL3D_ACT_BAKED order calls the same text)
__device__ __forceinline__ unsigned bake_texel(f4 s, int ract, int aact) {
    return bake_channel(act_rt(ract, s.x)) | bake_channel(act_rt(ract, s.y)) << 8 | bake_channel(act_rt(ract, s.z)) << 16 |
           bake_channel(act_rt(aact, s.w)) << 24;
}

template <bool F16>
__global__ __launch_bounds__(256) void bake_rgba8_k(int64_t n, const char *__restrict__ stack, int ract, int aact, unsigned *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one 16-byte load: a texel (fp32) or two (fp16)
    if constexpr (F16) {
        const int64_t t0 = i * 2;
        if (t0 >= n) return;
        if (t0 + 1 < n) {
            typedef _Float16 h8 __attribute__((ext_vector_type(8)));
            const h8 v = *reinterpret_cast<const h8 *>(stack + t0 * 8);
            out[t0] = bake_texel(f4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]}, ract, aact);
            out[t0 + 1] = bake_texel(f4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]}, ract, aact);
        } else {      // odd texel count: the last texel alone (8 bytes)
            out[t0] = bake_texel(__builtin_convertvector(*reinterpret_cast<const h4 *>(stack + t0 * 8), f4), ract, aact);
        }
    } else {
        if (i >= n) return;
        out[i] = bake_texel(*reinterpret_cast<const f4 *>(stack + i * 16), ract, aact);
    }
}

// ---- render -------------------------------------------------------------------------------------------------------------------------------
// the taps of a dense clip: one 8-byte load per texel row against a uniform plane base
__device__ __forceinline__ BakedTaps load_baked(const char *__restrict__ plane, const Taps2 &t, unsigned row_b) {
    const size_t o = (size_t)(t.off >> 2);      // make_taps2 gives the byte offset of 16-byte texels
    return BakedTaps{*reinterpret_cast<const u2w_a4 *>(plane + o), *reinterpret_cast<const u2w_a4 *>(plane + row_b + o)};
}

// PATH = NoPath: frames t0 .. of the run a.stack starts at, one camera (a.homos, a.cull_masks of one plan).
// PATH = PathIdx (a camera path, sel->frame_cam / frame_t): the block index's outermost factor is the OUTPUT frame i; the workgroup reads its camera and
// its frame of the clip (path_frame: scalar loads, range-checked) and from them forms its homography, mask and texel bases.  One frame per
// thread: from there on the one-frame kernel.
// PATH = PathTime (a path in loop time, vl3d_baked_times): as PathIdx, but the workgroup reads a real-valued time and fetches the taps of
// TWO frames, t0 and t1 (t1 wraps to 0 at the seam), which the composite interpolates by f before its one-frame step.
// OUT = FloatOut: rgb / alpha fp32 at a.rgb / a.alpha.  OUT = DisplayOut (out->frames): the 8-bit display frame over
// the background, written by the same launch (vl3d_baked_core.h); everything in front of the store is the one text.
template <int NF, bool CULL, typename PATH = NoPath, typename OUT = FloatOut>
__global__ __launch_bounds__(512) void render_fwd_baked_k(RenderArgs a, int tiles_x, int tiles_y, PATH path, OUT out) {
    constexpr bool IS_PATH = !std::is_same<PATH, NoPath>::value;
    constexpr bool IS_TIME = std::is_same<PATH, PathTime>::value;
    constexpr int NS = baked_sources<NF, PATH>();      // source frames fetched per thread
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
    float Tr[NF], cr[NF], cg[NF], cb[NF], A[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) { Tr[f] = 1.0f; cr[f] = cg[f] = cb[f] = A[f] = 0.0f; }
    struct Slot {
        Taps2 t;
        BakedTaps v[NS];
    } sA, sB;
    struct Owner;      // a type of this kernel instantiation alone: its own copy of the composite (vl3d_baked_core.h)
    std::conditional_t<IS_TIME, BakedCompositeAt<Owner>, const BakedComposite<NF, Owner>> composite(Tr, cr, cg, cb, A);
    if constexpr (IS_TIME) composite.fr = frac;
    auto fetch = [&](int d, Slot &s) {
        Taps2 &t = s.t;
        BakedTaps *v = s.v;
        float h[VL3D_HN];
        load_uniform(homos + VL3D_HS * d, h);
        if constexpr (CULL) t = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy, plane_cull(a, d));
        else t = make_taps2<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy);
#pragma unroll
        for (int f = 0; f < NS; ++f) v[f] = load_baked(base[f] + (size_t)d * plane_stride_b, t, row_b);
        asm volatile("" ::: "memory");      // keep the loads here: hipcc otherwise sinks them below the composite
    };
    auto step = [&](const Slot &s, int) { composite(s.t, s.v); };
    // the workgroup's plane list (cull_fwd_plan_k; a pixel inside a culled quad is uncovered, make_taps2) or every plane: walk_planes
    // (vl3d_render_core.h), the float forward's walk
    if constexpr (CULL) walk_planes(ListedPlanes(a.cull_masks, tile), sA, sB, fetch, step);
    else walk_planes(DensePlanes{a.D}, sA, sB, fetch, step);
    composite.store(a, out, t0, x, y, has1);
}

bool known_act(int act) { return act >= VL3D_ACT_NONE && act <= VL3D_ACT_ABS; }

}  // namespace

extern "C" int vl3d_bake_rgba8(int64_t n_texels, const void *stack, int32_t stack_dtype, int32_t rgb_act, int32_t alpha_act, uint8_t *out,
                               vl3d_stream_t stream) {
    VL3D_REQUIRE(n_texels > 0 && n_texels < (1ll << 38), "vl3d_bake_rgba8: texel count out of range");
    VL3D_REQUIRE(stack && out, "vl3d_bake_rgba8: null pointer");
    VL3D_REQUIRE(stack_dtype == VL3D_F32 || stack_dtype == VL3D_F16, "vl3d_bake_rgba8: stack_dtype must be VL3D_F32 or VL3D_F16");
    VL3D_REQUIRE(known_act(rgb_act) && known_act(alpha_act), "vl3d_bake_rgba8: unknown activation");
    VL3D_REQUIRE(((uintptr_t)stack & 15) == 0 && ((uintptr_t)out & 3) == 0, "vl3d_bake_rgba8: stack must be 16-byte aligned, out 4-byte aligned");
    const bool f16 = stack_dtype == VL3D_F16;
    const int64_t threads = f16 ? (n_texels + 1) / 2 : n_texels;
    const dim3 grid((unsigned)ceil_div64(threads, 256)), block(256);
    if (f16) hipLaunchKernelGGL((bake_rgba8_k<true>), grid, block, 0, (hipStream_t)stream, n_texels, (const char *)stack, rgb_act, alpha_act, (unsigned *)out);
    else hipLaunchKernelGGL((bake_rgba8_k<false>), grid, block, 0, (hipStream_t)stream, n_texels, (const char *)stack, rgb_act, alpha_act, (unsigned *)out);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

// two 64-bit plane masks per (camera, 64 x 8 pixel workgroup): [n_cams][tiles_y * tiles_x][2]
extern "C" int64_t vl3d_render_path_cull_scratch_bytes(const vl3d_render_desc *desc, int32_t n_cams) {
    if (!desc || desc->H <= 0 || desc->W <= 0 || n_cams <= 0) return 0;
    return (int64_t)n_cams * ((desc->W + 63) / 64) * ((desc->H + 7) / 8) * 16;
}

namespace {

// The one body of the two entries: the refusals, RenderArgs, then the plan launch of a tile-culled model (the float forward's plan over its
// 64 x 8 tiles: one camera's, or all cameras' of a path in one launch) and the render launch on <NF, CULL, PATH, OUT> as the selection --
// `sel` (a run or a path of frames) or `times` (a path in loop time), exactly one of them -- and `out` name them.
int render_fwd_baked(const char *who, const vl3d_render_desc *desc, const uint8_t *baked, int32_t T_alloc, const float *homos,
                     const vl3d_baked_frames *sel, const vl3d_baked_times *times, bool by_time, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                     void *cull_scratch, const vl3d_baked_out *out, vl3d_stream_t stream) {
    // a row's two taps are one 8-byte load, the two rows a constant step apart
    int rc = check_baked_desc(desc, 1ll << 28, "plane too large for 32-bit tap offsets", who);
    if (rc != VL3D_OK) return rc;
    bool is_path = by_time;
    if ((rc = by_time ? check_baked_times(desc, times, who) : check_baked_frames(desc, sel, is_path, who)) != VL3D_OK ||
        (rc = check_baked_out(out, who)) != VL3D_OK)
        return rc;
    if (!(baked && homos)) return refuse(who, "null pointer");
    if (((uintptr_t)baked & 3) != 0) return refuse(who, "the texels must be 4-byte aligned");
    DisplayOut disp;
    if (out->frames && (rc = display_out_of(out->frames, out->channels, out->bg, who, disp)) != VL3D_OK) return rc;
    if (is_path) {
        if (!(T_alloc > 0)) return refuse(who, "a clip of T_alloc >= 1 frames");
    } else if (!(T_alloc > 0 && sel->frame0 >= 0 && sel->frame0 + desc->T <= T_alloc)) {
        return refuse(who, "the run of frames leaves the clip");
    }
    RenderArgs a = render_args_of(desc);      // (a.uv_seed is 0, checked above; a path: a.T is the count of its output frames)
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
    auto launch = [&](auto nf, const auto &path, const auto &o) {
        constexpr int NF = decltype(nf)::value;
        using PATH = std::decay_t<decltype(path)>;
        using OUT = std::decay_t<decltype(o)>;
        const dim3 grid((unsigned)(tiles_x * tiles_y * ((a.T + NF - 1) / NF))), block(512);
        if (a.quad_keep) {
            if constexpr (std::is_same<PATH, NoPath>::value) launch_cull_fwd_plan<VL3D_COORD_AFFINE>(a, 8, tiles_x, tiles_y, s);
            else launch_cull_fwd_plan_cams<VL3D_COORD_AFFINE>(a, path.n_cams, 8, tiles_x, tiles_y, s);
            hipLaunchKernelGGL((render_fwd_baked_k<NF, true, PATH, OUT>), grid, block, 0, s, a, tiles_x, tiles_y, path, o);
            return;
        }
        hipLaunchKernelGGL((render_fwd_baked_k<NF, false, PATH, OUT>), grid, block, 0, s, a, tiles_x, tiles_y, path, o);
    };
    const std::integral_constant<int, 1> one;      // frames per thread: pairs for a run of two or more, one along a path
    const std::integral_constant<int, 2> two;
    if (by_time) {
        const PathTime path{times->frame_cam, times->frame_time, times->n_cams, T_alloc};
        if (!out->frames) launch(one, path, FloatOut{});
        else launch(one, path, disp);
    } else {
        const PathIdx path{sel->frame_cam, sel->frame_t, sel->n_cams, T_alloc};
        if (!is_path && !out->frames) desc->T >= 2 ? launch(two, NoPath{}, FloatOut{}) : launch(one, NoPath{}, FloatOut{});
        else if (!is_path) desc->T >= 2 ? launch(two, NoPath{}, disp) : launch(one, NoPath{}, disp);
        else if (!out->frames) launch(one, path, FloatOut{});
        else launch(one, path, disp);
    }
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

}  // namespace

extern "C" int vl3d_render_fwd_baked(const vl3d_render_desc *desc, const uint8_t *baked, int32_t T_alloc, const float *homos,
                                     const vl3d_baked_frames *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch,
                                     const vl3d_baked_out *out, vl3d_stream_t stream) {
    return render_fwd_baked("vl3d_render_fwd_baked", desc, baked, T_alloc, homos, sel, nullptr, false, quad_keep, QH, QW, cull_scratch, out, stream);
}

extern "C" int vl3d_render_fwd_baked_times(const vl3d_render_desc *desc, const uint8_t *baked, int32_t T_alloc, const float *homos,
                                           const vl3d_baked_times *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW, void *cull_scratch,
                                           const vl3d_baked_out *out, vl3d_stream_t stream) {
    return render_fwd_baked("vl3d_render_fwd_baked_times", desc, baked, T_alloc, homos, nullptr, sel, true, quad_keep, QH, QW, cull_scratch, out,
                            stream);
}
