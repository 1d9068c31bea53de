// The playback model of a PACKED tile-culled model (include/vl3d.h "Baked playback"; videoloop3d_amd/baked.py: BakedPool).
//
// vl3d_render_fwd_baked renders a dense (D, T, Hs, Ws, 4) uint8 clip: T copies of every static texel and slots for culled ones.  This unit
// renders the same picture from the baked POOL: RGBA8 blocks of 8 x 8 texels (256 bytes) behind the block table of packed.PackedLayout,
// [D][ceil(Hs/8)][ceil(Ws/8)] int32 = -1 (no kept quad reads the block: not stored) | slot << 1 | dynamic (a static block owns one slot,
// a dynamic block T consecutive ones) -- the static and the dynamic atlas of the viewer package, a quarter of the float pool.
//   * coverage and taps: make_taps_i / plane_cull of vl3d_render_core.h with the arguments the dense baked kernel passes to make_taps2
//     (which is make_taps_i plus a byte offset), the workgroups' plane lists by cull_fwd_plan_k;
//   * decode, blend, composite: chan / blend of vl3d_baked_core.h and the dense kernel's composite, text for text -- the image is the dense
//     baked render of the unpacked texels, bit for bit;
//   * fetch: per texel row one 4-byte table entry (shared by the 64 texels of a block) and ONE 8-byte load of texels (x0, x0 + 1) when they
//     lie in one block (x0 % 8 != 7), else a second entry and two 4-byte loads across the seam.  A static block is fetched once for both
//     frames of a pair, a dynamic block at `frame` and `frame + 1`; a tap in a block without storage is `culled_rgba8` from a register; a
//     pixel the plane does not cover (cov == 0) issues no load at all and leaves the composite state untouched.
// Launch shape of the dense baked kernel: 64 x 8 pixels per workgroup, XCD remap, frame pairs for T >= 2 (an odd tail frame composited twice
// and stored once), the next plane's taps fetched before the current plane is composited (two register sets).  Forward only.
#include "vl3d_baked_core.h"

using vl3d_render_detail::RenderArgs;

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
// `in_b`: the texel's byte inside its block; `frame_b`: the byte step to the run's first frame of a dynamic block.
template <int NF, typename L, typename V>      // L: the type loaded (its alignment), V: the value kept
__device__ __forceinline__ void pool_load(const PoolSrc &p, int e, unsigned in_b, size_t frame_b, bool has1, V fill, V (&out)[NF]) {
#pragma unroll
    for (int f = 0; f < NF; ++f) out[f] = fill;
    if (e < 0) return;
    const char *b = p.pool + (size_t)(e >> 1) * SLOT_B + in_b + ((e & 1) ? frame_b : 0);
    out[0] = *reinterpret_cast<const L *>(b);
    if constexpr (NF == 2) {
        out[1] = out[0];      // a static block, or the odd tail: the one fetch serves both frames
        if ((e & 1) && has1) out[1] = *reinterpret_cast<const L *>(b + SLOT_B);
    }
}

template <int NF>
__global__ __launch_bounds__(512) void render_fwd_baked_pool_k(RenderArgs a, PoolSrc p, int tiles_x, int tiles_y) {
    static_assert(NF == 1 || NF == 2, "one frame or a frame pair per thread");
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    const int tile_x = b % tiles_x, rest = b / tiles_x;
    const int tile_y = rest % tiles_y, t0 = (rest / tiles_y) * NF;
    const bool has1 = NF == 2 && t0 + 1 < a.T;      // odd T: the last pair composites frame t0 twice and stores it once
    const int x = tile_x * 64 + (threadIdx.x & 63);
    const int y = tile_y * 8 + (threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const float px = (float)(a.col0 + x) + a.pc, py = (float)(a.row0 + y) + a.pc;
    const size_t frame_b = (size_t)(p.frame0 + t0) * SLOT_B;
    const size_t bplane_n = (size_t)p.tiles_y * p.tiles_x;
    float Tr[NF], cr[NF], cg[NF], cb[NF], A[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) { Tr[f] = 1.0f; cr[f] = cg[f] = cb[f] = A[f] = 0.0f; }
    BakedTaps vA[NF], vB[NF];
    // the dense baked kernel's composite (csrc/vl3d_render_baked.hip), text for text: the fused multiply-adds are spelt out and nothing else
    // may be contracted, so that a frame has the same bits in a pair, alone, and in the dense render
    auto composite = [&](const TapsI &t, const BakedTaps *v) {
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
    };
    auto fetch = [&](int d, TapsI &t, BakedTaps *v) {
        float h[VL3D_HN];
        load_uniform(a.homos + VL3D_HS * d, h);
        t = make_taps_i<VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT>(h, px, py, a.Hs, a.Ws, a.sx, a.sy, a.ox, a.oy, plane_cull(a, d));
#pragma unroll
        for (int f = 0; f < NF; ++f) v[f] = BakedTaps{u2w{0u, 0u}, u2w{0u, 0u}};
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
            u2w r0[NF], r1[NF];
            if (bx == bx1) {      // x0 % 8 != 7: both texels of a row in one block, 8 contiguous bytes (4-byte aligned: x0 may be odd)
                pool_load<NF, u2w_a4>(p, e00, in0, frame_b, has1, u2w{p.culled, p.culled}, r0);
                pool_load<NF, u2w_a4>(p, e10, in1, frame_b, has1, u2w{p.culled, p.culled}, r1);
            } else {              // across a block seam: the right texel is column 0 of the next block
                unsigned l0[NF], l1[NF], q0[NF], q1[NF];
                pool_load<NF, unsigned>(p, e00, in0, frame_b, has1, p.culled, l0);
                pool_load<NF, unsigned>(p, e01, in0 - (TSB - 1) * 4u, frame_b, has1, p.culled, q0);
                pool_load<NF, unsigned>(p, e10, in1, frame_b, has1, p.culled, l1);
                pool_load<NF, unsigned>(p, e11, in1 - (TSB - 1) * 4u, frame_b, has1, p.culled, q1);
#pragma unroll
                for (int f = 0; f < NF; ++f) { r0[f] = u2w{l0[f], q0[f]}; r1[f] = u2w{l1[f], q1[f]}; }
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) v[f] = BakedTaps{r0[f], r1[f]};
        }
        asm volatile("" ::: "memory");      // keep the loads here: hipcc otherwise sinks them below the composite
    };
    auto composite_if = [&](const TapsI &t, const BakedTaps *v) {
        if (t.cov != 0.0f) composite(t, v);
    };
    // the workgroup's plane list (cull_fwd_plan_k): two 64-bit words in SGPRs, scalar bit scans; a pixel inside a culled quad is uncovered
    // (make_taps_i), so walking only the listed planes changes no result
    const unsigned long long *mk = a.cull_masks + (size_t)(tile_y * tiles_x + tile_x) * 2;
    unsigned long long m0 = ((const __attribute__((address_space(4))) unsigned long long *)mk)[0];
    unsigned long long m1 = ((const __attribute__((address_space(4))) unsigned long long *)mk)[1];
    auto next = [&]() {
        int d = -1;
        if (m0) { d = __builtin_ctzll(m0); m0 &= m0 - 1; }
        else if (m1) { d = 64 + __builtin_ctzll(m1); m1 &= m1 - 1; }
        return d;
    };
    TapsI tA, tB;
    const int dA = next();
    if (dA >= 0) {
        fetch(dA, tA, vA);
        for (;;) {      // two register sets: the next listed plane is fetched before the current one is composited; nothing is fetched past the end
            const int dB = next();
            if (dB >= 0) fetch(dB, tB, vB);
            composite_if(tA, vA);
            if (dB < 0) break;
            const int dC = next();
            if (dC >= 0) fetch(dC, tA, vA);
            composite_if(tB, vB);
            if (dC < 0) break;
        }
    }
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

template <int NF>
void launch_baked_pool(const RenderArgs &a, const PoolSrc &p, hipStream_t s) {
    const int tiles_x = (a.W + 63) / 64, tiles_y = (a.H + 7) / 8;
    const dim3 grid((unsigned)(tiles_x * tiles_y * ((a.T + NF - 1) / NF))), block(512);
    // the float forward's plan (frame independent, its 64 x 8 tiles), then the plane-list kernel
    auto *masks = const_cast<unsigned long long *>(a.cull_masks);
    (void)hipMemsetAsync(masks, 0, (size_t)tiles_x * tiles_y * 16, s);
    const int n = tiles_x * tiles_y * a.D;
    hipLaunchKernelGGL((cull_fwd_plan_k<VL3D_COORD_AFFINE>), dim3((n + 255) / 256), dim3(256), 0, s, a, 8, tiles_x, tiles_y, masks);
    hipLaunchKernelGGL((render_fwd_baked_pool_k<NF>), grid, block, 0, s, a, p, tiles_x, tiles_y);
}

}  // namespace

extern "C" int vl3d_render_fwd_baked_pool(const vl3d_render_desc *desc, const int32_t *blocks, const uint8_t *pool, int32_t frame0,
                                          int32_t T_model, const float *homos, const uint8_t *quad_keep, int32_t QH, int32_t QW,
                                          uint32_t culled_rgba8, void *cull_scratch, float *rgb, float *alpha, vl3d_stream_t stream) {
    VL3D_REQUIRE(desc != nullptr, "null render desc");
    VL3D_REQUIRE(desc->variant == 0, "vl3d_render_fwd_baked_pool: no kernel variants (desc->variant = 0)");
    VL3D_REQUIRE(desc->D > 0 && desc->T > 0 && desc->H > 0 && desc->W > 0, "vl3d_render_fwd_baked_pool: non-positive render dims");
    // the base tap is clamped to (Ws - 2, Hs - 2) and its right / lower neighbours are read unconditionally: planes of at least 2 x 2 texels
    VL3D_REQUIRE(desc->Hs >= 2 && desc->Ws >= 2, "vl3d_render_fwd_baked_pool: planes of at least 2 x 2 texels");
    VL3D_REQUIRE(desc->Hs < (1 << 24) && desc->Ws < (1 << 24), "vl3d_render_fwd_baked_pool: plane too large");
    VL3D_REQUIRE(desc->stack_dtype == VL3D_U8, "vl3d_render_fwd_baked_pool: stack_dtype must be VL3D_U8 (the baked RGBA8 texels of vl3d_bake_rgba8)");
    VL3D_REQUIRE(desc->coord_mode == VL3D_COORD_AFFINE && desc->border_mode == VL3D_BORDER_HARDCUT,
                 "vl3d_render_fwd_baked_pool: the planar MPV convention only (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT)");
    VL3D_REQUIRE(desc->uv_noise_seed == 0, "vl3d_render_fwd_baked_pool: add_uv_noise is a training switch (uv_noise_seed = 0)");
    VL3D_REQUIRE(blocks && pool && homos && quad_keep && cull_scratch && rgb && alpha,
                 "vl3d_render_fwd_baked_pool: null pointer (the quad map and vl3d_render_cull_scratch_bytes() of scratch are required)");
    VL3D_REQUIRE(((uintptr_t)pool & 3) == 0 && ((uintptr_t)blocks & 3) == 0, "vl3d_render_fwd_baked_pool: the pool and the block table must be 4-byte aligned");
    VL3D_REQUIRE(T_model > 0 && frame0 >= 0 && (int64_t)frame0 + desc->T <= T_model,
                 "vl3d_render_fwd_baked_pool: the run of frames leaves the model's T_model frames");
    VL3D_REQUIRE((QH > 0 && QW > 0) || (QH < 0 && QW < 0 && desc->Hs % (-QH) == 0 && desc->Ws % (-QW) == 0 && desc->Hs / (-QH) >= 2 && desc->Ws / (-QW) >= 2),
                 "vl3d_render_fwd_baked_pool: bad quad grid (both positive, or both negative for the tile-exact layout: whole tiles of at least 2 x 2 texels)");
    VL3D_REQUIRE(desc->D <= 128, "tile culling supports at most 128 planes");
    VL3D_REQUIRE(desc->cull_Hs == 0 && desc->cull_Ws == 0, "vl3d_render_fwd_baked_pool: the pool holds whole planes (no desc->cull_* window)");
    RenderArgs a{};
    a.D = desc->D; a.T = desc->T; a.Hs = desc->Hs; a.Ws = desc->Ws; a.H = desc->H; a.W = desc->W;
    a.row0 = desc->row0; a.col0 = desc->col0;
    a.pc = desc->pixel_center; a.sx = desc->sx; a.sy = desc->sy; a.ox = desc->ox; a.oy = desc->oy;
    a.homos = homos; a.rgb = rgb; a.alpha = alpha;
    a.quad_keep = quad_keep;
    a.cull_masks = (const unsigned long long *)cull_scratch;
    a.q_Hs = desc->Hs; a.q_Ws = desc->Ws; a.q_x0 = 0.0f; a.q_y0 = 0.0f;
    if (QH < 0) {      // tile-exact layout (include/vl3d.h): |QH| x |QW| tiles, every quad owning its border texels
        a.QH = -QH; a.QW = -QW;
        a.q_th = a.q_Hs / a.QH; a.q_tw = a.q_Ws / a.QW;
        a.q_inv_cw = 1.0f / (float)(a.q_tw - 1);
        a.q_inv_ch = 1.0f / (float)(a.q_th > 1 ? a.q_th - 1 : 1);
    } else {
        a.QH = QH; a.QW = QW;
        a.q_inv_cw = (float)QW / (float)(a.q_Ws - 1);
        a.q_inv_ch = (float)QH / (float)(a.q_Hs - 1);
    }
    const PoolSrc p{blocks, reinterpret_cast<const char *>(pool), (desc->Hs + TSB - 1) / TSB, (desc->Ws + TSB - 1) / TSB, frame0, culled_rgba8};
    if (desc->T >= 2) launch_baked_pool<2>(a, p, (hipStream_t)stream);
    else launch_baked_pool<1>(a, p, (hipStream_t)stream);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
