// The playback model of a PACKED tile-culled model (include/vl3d.h "Baked playback"; videoloop3d_amd/baked.py: BakedPool).
//
// vl3d_render_fwd_baked renders a dense (D, T, Hs, Ws, 4) uint8 clip: T copies of every static texel and slots for culled ones.  This unit
// renders the same picture from the baked POOL: RGBA8 blocks of 8 x 8 texels (256 bytes) behind the block table of packed.PackedLayout,
// [D][ceil(Hs/8)][ceil(Ws/8)] int32 = -1 (no kept quad reads the block: not stored) | slot << 1 | dynamic (a static block owns one slot,
// a dynamic block T consecutive ones) -- the static and the dynamic atlas of the viewer package, a quarter of the float pool.
//   * coverage and taps: make_taps_i / plane_cull of vl3d_render_core.h with the arguments the dense baked kernel passes to make_taps2
//     (which is make_taps_i plus a byte offset), the workgroups' plane lists by cull_fwd_plan_k;
//   * decode, blend, composite, pixel store: chan / blend / BakedComposite of vl3d_baked_core.h, the dense kernel's own -- the image is the
//     dense baked render of the unpacked texels, bit for bit;
//   * fetch: per texel row one 4-byte table entry (shared by the 64 texels of a block) and ONE 8-byte load of texels (x0, x0 + 1) when they
//     lie in one block (x0 % 8 != 7), else a second entry and two 4-byte loads across the seam.  A static block is fetched once for both
//     frames of a pair, a dynamic block at `frame` and `frame + 1`; a tap in a block without storage is `culled_rgba8` from a register; a
//     pixel the plane does not cover (cov == 0) issues no load at all and leaves the composite state untouched.
// Launch shape of the dense baked kernel: 64 x 8 pixels per workgroup, XCD remap, frame pairs for T >= 2 (an odd tail frame composited twice
// and stored once), the next plane's taps fetched before the current plane is composited (two register sets).  Forward only.
#include "vl3d_baked_core.h"
#include "vl3d_render_args.h"

using namespace vl3d_render_detail;

namespace {

constexpr int TSB = 8;                           // block side (vl3d_adam_window_tile())
constexpr unsigned SLOT_B = TSB * TSB * 4;       // bytes of a slot: 64 RGBA8 texels

struct PoolSrc {
    const int *blocks;           // [D][tiles_y][tiles_x]
    const char *pool;            // n_slots * SLOT_B bytes
    int tiles_y, tiles_x;
    int frame0;                  // first frame of the run, in the model's T frames
    unsigned culled;             // the texel a block without storage reads as
};

// The fetch of a sample, in two stages so that a thread waits ONCE per stage: first the table entries of both texel rows (and of the blocks to
// their right, which are the same blocks unless the tap pair crosses a seam), then every texel load behind them.  A texel load is issued
// only under `e >= 0`: a block without storage is never dereferenced, its texels are `culled` from a register.
// `in_b`: the texel's byte inside its block; `frame_b`: the byte step to the first source frame of a dynamic block, `frame1_b`: the step
// from there to the second (a frame pair: SLOT_B, a constant; a loop time: (t1 - t0) slots, negative across the seam).
template <int NS, typename L, typename V>      // NS: source frames; L: the type loaded (its alignment), V: the value kept
__device__ __forceinline__ void pool_load(const PoolSrc &p, int e, unsigned in_b, size_t frame_b, ptrdiff_t frame1_b, bool has1, V fill, V (&out)[NS]) {
#pragma unroll
    for (int f = 0; f < NS; ++f) out[f] = fill;
    if (e < 0) return;
    const char *b = p.pool + (size_t)(e >> 1) * SLOT_B + in_b + ((e & 1) ? frame_b : 0);
    out[0] = *reinterpret_cast<const L *>(b);
    if constexpr (NS == 2) {
        out[1] = out[0];      // a static block, the odd tail, or t1 == t0: the one fetch serves both frames
        if ((e & 1) && has1) out[1] = *reinterpret_cast<const L *>(b + frame1_b);
    }
}

// PATH = NoPath: frames p.frame0 + t0 .. of one camera.  PATH = PathIdx (a camera path, sel->frame_cam / frame_t): the block index's outermost factor is
// the OUTPUT frame; camera and frame of the model come from path_frame (scalar loads, range-checked), as in the dense path kernel.
// PATH = PathTime (a path in loop time): the taps of frames t0 and t1 of the model -- a static or unstored entry fetched once (or read from
// the register) for both, a dynamic entry at slot + t0 and slot + t1 --, interpolated by the composite.
// OUT: FloatOut, or the DisplayOut of out->frames (vl3d_baked_core.h), as in the dense kernel.
template <int NF, typename PATH = NoPath, typename OUT = FloatOut>
__global__ __launch_bounds__(512) void render_fwd_baked_pool_k(RenderArgs a, PoolSrc p, int tiles_x, int tiles_y, PATH path, OUT out) {
    constexpr bool IS_PATH = !std::is_same<PATH, NoPath>::value;
    constexpr bool IS_TIME = std::is_same<PATH, PathTime>::value;
    constexpr int NS = baked_sources<NF, PATH>();      // source frames fetched per thread
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
        tile += cam * tiles_x * tiles_y;
    }
    const int x = tile_x * 64 + (threadIdx.x & 63);
    const int y = tile_y * 8 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const size_t frame_b = (size_t)src_t * SLOT_B;
    const size_t bplane_n = (size_t)p.tiles_y * p.tiles_x;
    float Tr[NF], cr[NF], cg[NF], cb[NF], A[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) { Tr[f] = 1.0f; cr[f] = cg[f] = cb[f] = A[f] = 0.0f; }
    struct Slot {
        TapsI t;
        BakedTaps v[NS];
    } sA, sB;
    struct Owner;      // a type of this kernel instantiation alone: its own copy of the composite (vl3d_baked_core.h)
    const BakedComposite<NF, Owner> state(Tr, cr, cg, cb, A);
    auto fetch = [&](int d, Slot &s) {
        TapsI &t = s.t;
        BakedTaps *v = s.v;
        float h[VL3D_HN];
        load_uniform(homos + VL3D_HS * d, h);
        t = make_taps_i<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy, plane_cull(a, d));
#pragma unroll
        for (int f = 0; f < NS; ++f) v[f] = BakedTaps{u2w{0u, 0u}, u2w{0u, 0u}};
        // an uncovered pixel (outside the plane's extent or inside a culled quad) adds +0 to every accumulator and multiplies T by 1 in the
        // dense kernel: its state is untouched bit for bit, so nothing is fetched (and composite_if skips it)
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
            if (bx == bx1) {      // x0 % 8 != 7: both texels of a row in one block, 8 contiguous bytes (4-byte aligned: x0 may be odd)
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
    // (an uncovered pixel's composite step changes no bit of the state -- see fetch --: skipped)
    auto composite_if = [&](const Slot &s, int) {
        if (s.t.cov != 0.0f) {
            if constexpr (IS_TIME) state(s.t, s.v, frac);
            else state(s.t, s.v);
        }
    };
    // the workgroup's plane list (cull_fwd_plan_k); a pixel inside a culled quad is uncovered (make_taps_i).  Two register sets: the next
    // listed plane is fetched before the current one is composited; nothing is fetched past the end (walk_planes_cond, vl3d_render_core.h)
    walk_planes_cond(ListedPlanes(a.cull_masks, tile), sA, sB, fetch, composite_if);
    state.store(a, out, t0, x, y, NF == 2 && has1);
}

}  // namespace

namespace {

// The one body of the two entries: the refusals, RenderArgs and PoolSrc, then the plan launch (the float forward's plan over its 64 x 8 tiles:
// one camera's, or all cameras' of a path in one launch) and the render launch on <NF, PATH, OUT> as the selection -- `sel` (a run or a path
// of frames) or `times` (a path in loop time), exactly one of them -- and `out` name them.
int render_fwd_baked_pool(const char *who, const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t T_model,
                          const float *homos, const vl3d_baked_frames *sel, const vl3d_baked_times *times, bool by_time, const uint8_t *quad_keep,
                          int32_t QH, int32_t QW, uint32_t culled_rgba8, void *cull_scratch, const vl3d_baked_out *out, vl3d_stream_t stream) {
    int rc = check_baked_desc(desc, INT64_MAX, "plane too large", who);
    if (rc != VL3D_OK) return rc;
    bool is_path = by_time;
    if ((rc = by_time ? check_baked_times(desc, times, who) : check_baked_frames(desc, sel, is_path, who)) != VL3D_OK ||
        (rc = check_baked_out(out, who)) != VL3D_OK)
        return rc;
    if (!(blocks && pool && homos && quad_keep && cull_scratch))
        return refuse(who, "null pointer (the quad map and vl3d_render_cull_scratch_bytes() of scratch are required)");
    if (!(((uintptr_t)pool & 3) == 0 && ((uintptr_t)blocks & 3) == 0)) return refuse(who, "the pool and the block table must be 4-byte aligned");
    DisplayOut disp;
    if (out->frames && (rc = display_out_of(out->frames, out->channels, out->bg, who, disp)) != VL3D_OK) return rc;
    if (is_path) {
        if (!(T_model > 0)) return refuse(who, "a model of T_model >= 1 frames");
    } else if (!(T_model > 0 && sel->frame0 >= 0 && (int64_t)sel->frame0 + desc->T <= T_model)) {
        return refuse(who, "the run of frames leaves the model's T_model frames");
    }
    if (!(desc->cull_Hs == 0 && desc->cull_Ws == 0)) return refuse(who, "the pool holds whole planes (no desc->cull_* window)");
    if ((rc = check_cull_grid(desc, QH, QW, who)) != VL3D_OK) return rc;
    RenderArgs a = render_args_of(desc);      // (a.uv_seed is 0, checked above; a.Tstride is not read: the pool has no frame stride)
    a.homos = homos; a.rgb = out->rgb; a.alpha = out->alpha;
    a.quad_keep = quad_keep;
    a.cull_masks = (const unsigned long long *)cull_scratch;
    set_cull_geometry(a, desc, QH, QW);
    const PoolSrc p{blocks, reinterpret_cast<const char *>(pool), (desc->Hs + TSB - 1) / TSB, (desc->Ws + TSB - 1) / TSB, is_path ? 0 : sel->frame0,
                    culled_rgba8};
    const int tiles_x = (a.W + 63) / 64, tiles_y = (a.H + 7) / 8;
    const hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto nf, const auto &path, const auto &o) {
        constexpr int NF = decltype(nf)::value;
        using PATH = std::decay_t<decltype(path)>;
        using OUT = std::decay_t<decltype(o)>;
        const dim3 grid((unsigned)(tiles_x * tiles_y * ((a.T + NF - 1) / NF))), block(512);
        if constexpr (std::is_same<PATH, NoPath>::value) launch_cull_fwd_plan<VL3D_COORD_AFFINE>(a, 8, tiles_x, tiles_y, s);
        else launch_cull_fwd_plan_cams<VL3D_COORD_AFFINE>(a, path.n_cams, 8, tiles_x, tiles_y, s);
        hipLaunchKernelGGL((render_fwd_baked_pool_k<NF, PATH, OUT>), grid, block, 0, s, a, p, tiles_x, tiles_y, path, o);
    };
    const std::integral_constant<int, 1> one;      // frames per thread: pairs for a run of two or more, one along a path
    const std::integral_constant<int, 2> two;
    if (by_time) {
        const PathTime path{times->frame_cam, times->frame_time, times->n_cams, T_model};
        if (!out->frames) launch(one, path, FloatOut{});
        else launch(one, path, disp);
    } else {
        const PathIdx path{sel->frame_cam, sel->frame_t, sel->n_cams, T_model};
        if (!is_path && !out->frames) desc->T >= 2 ? launch(two, NoPath{}, FloatOut{}) : launch(one, NoPath{}, FloatOut{});
        else if (!is_path) desc->T >= 2 ? launch(two, NoPath{}, disp) : launch(one, NoPath{}, disp);
        else if (!out->frames) launch(one, path, FloatOut{});
        else launch(one, path, disp);
    }
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

}  // namespace

extern "C" int vl3d_render_fwd_baked_pool(const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t T_model,
                                          const float *homos, const vl3d_baked_frames *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                                          uint32_t culled_rgba8, void *cull_scratch, const vl3d_baked_out *out, vl3d_stream_t stream) {
    return render_fwd_baked_pool("vl3d_render_fwd_baked_pool", desc, blocks, pool, T_model, homos, sel, nullptr, false, quad_keep, QH, QW, culled_rgba8,
                                 cull_scratch, out, stream);
}

extern "C" int vl3d_render_fwd_baked_pool_times(const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t T_model,
                                                const float *homos, const vl3d_baked_times *sel, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                                                uint32_t culled_rgba8, void *cull_scratch, const vl3d_baked_out *out, vl3d_stream_t stream) {
    return render_fwd_baked_pool("vl3d_render_fwd_baked_pool_times", desc, blocks, pool, T_model, homos, nullptr, sel, true, quad_keep, QH, QW,
                                 culled_rgba8, cull_scratch, out, stream);
}
