// Which kernel the render backward runs, as a value: the policy a caller's desc->variant names, the one table of region shapes, and
// choose_bwd() -- a pure function of the call's facts.  Host only: no HIP in here (plain g++ -std=c++17 compiles it; the stand-alone program
// tests/bwd_choice_cases.cpp runs it under the sanitizers).  launch_t<true, ...> (vl3d_render_core.h) switches on the choice, the scratch
// layout (vl3d_render.hip) is sized from the table, vl3d_render_bwd_choice() (include/vl3d.h) shows the choice to tests.
#pragma once
#include <stdint.h>
#include "vl3d.h"

namespace vl3d_render_detail {

// ---- the policy: what desc->variant bits 0-3 ask for at an entry point ----------------------------------------------------------------
enum BwdPolicy : int {
    BWD_NONE = 0,      // no owner-computes path for this call: the atomics kernel alone, on a gradient the entry cleared
    BWD_AUTO,          // the measured default of every rule below
    BWD_TILE16,        // one frame per thread, 64 x 16 regions
    BWD_FLAT8,         // one frame per thread, flat 64 x 8 regions
    BWD_NARROW32,      // one frame per thread, 32 x 16 regions
    BWD_PAIRS32,       // frame pairs in 32 x 16 regions wherever BWD_AUTO takes frame pairs
    BWD_PAIRS64X12,    // frame pairs in 64 x 12 regions wherever BWD_AUTO takes frame pairs, WITH the owner table (render_bwd_pair_k<..., BWD_64X12>)
    BWD_PAIRS64X12O,   // ... without the owner table (its OWNERLESS instantiation): every gather thread computes its texel's owner pixel
};
struct BwdSetting {
    BwdPolicy policy;
    bool gather9;      // never take the 2x2 gather (variant 4: the 3x3 gather is the definition the 2x2 one must equal bit for bit)
    bool owner4;       // a single frame may build its owner table four texels per thread (variants 3 and 4 keep the one-texel pass)
};

// (entry point, desc->variant & 0xf) -> policy.  `tile_ok`: the caller passed vl3d_render_bwd_scratch_bytes() of scratch and no uv noise
// (add_uv_noise: a jittered tap can leave the 1-pixel halo the owner-computes kernels stage -- the atomics kernel takes the call).
//   vl3d_render_bwd (dense or with a quad map): 0 auto, 1 atomics, 2 flat 64 x 8, 5 narrow 32 x 16, 6 / 7 / 8 pairs 32 x 16 / 64 x 12 with the owner table / 64 x 12 without it,
//                             every other value 64 x 16
//   vl3d_render_bwd_mask:     1 atomics, 3 / 4 the 16 rows, every other value the flat 64 x 8 regions: 512 threads at that instantiation's
//                             128-register budget are TWO workgroups per CU -- stage-1 iterations +3.3 % at the reference's crop, +2 % for a
//                             720p frame (profiles/r05d_s1_mask_rows.txt), same bits
//   vl3d_render_bwd_adam:     (the entry admits 0 for a dense model, 0 / 3 / 5 with a quad map, and refuses short scratch and uv noise)
//                             dense auto; tile-culled 3 the 64-wide regions, else the narrow ones; always the 2x2 gather and per-texel records
inline BwdSetting bwd_setting_of(int entry, int bv, bool tile_ok, bool has_quad_map) {
    BwdSetting s{BWD_NONE, bv == 4, bv != 3 && bv != 4};
    if (entry == VL3D_BWD_ENTRY_ADAM) {
        s.gather9 = s.owner4 = false;
        s.policy = has_quad_map ? (bv == 3 ? BWD_TILE16 : BWD_NARROW32) : BWD_AUTO;
    } else if (bv == 1 || !tile_ok) {
        s.policy = BWD_NONE;
    } else if (entry == VL3D_BWD_ENTRY_MASK) {
        s.policy = (bv == 3 || bv == 4) ? BWD_TILE16 : BWD_FLAT8;
    } else {
        s.policy = bv == 0 ? BWD_AUTO : bv == 2 ? BWD_FLAT8 : bv == 5 ? BWD_NARROW32 : bv == 6 ? BWD_PAIRS32 : bv == 7 ? BWD_PAIRS64X12 : bv == 8 ? BWD_PAIRS64X12O : BWD_TILE16;
    }
    return s;
}

// ---- the region shapes: THE list.  A workgroup is width x rows threads; with the 1-pixel halo every kernel uses it owns the interior -------
enum BwdShape : int { BWD_64X16 = 0, BWD_64X8, BWD_32X16, BWD_64X12, BWD_NSHAPES };
struct BwdRegion { int width, rows; };
constexpr BwdRegion BWD_REGIONS[BWD_NSHAPES] = {{64, 16}, {64, 8}, {32, 16}, {64, 12}};
constexpr int BWD_HALO = 1;
constexpr int bwd_interior_w(int shape) { return BWD_REGIONS[shape].width - 2 * BWD_HALO; }
constexpr int bwd_interior_h(int shape) { return BWD_REGIONS[shape].rows - 2 * BWD_HALO; }
// bits of an owner-table entry that index a pixel of the region (the tile code sits above them)
constexpr int bwd_slot_bits(int shape) { return BWD_REGIONS[shape].width * BWD_REGIONS[shape].rows > 512 ? 10 : 9; }

// The most (tile, plane) window records any shape needs for an H x W frame: the scratch layout's size (vl3d_render_bwd_scratch_bytes).
// SIZING ONLY: two interiors of the 2-pixel halo no kernel uses any more (60 x 12, 28 x 12) stay in the maximum, because the byte count is
// ABI -- callers allocate by it and an entry takes the owner-computes path only when given that many -- and without them it shrinks for
// some frames (H = 13, W = 61: 3 tiles instead of 6).
constexpr BwdRegion BWD_SIZING_ONLY_INTERIORS[] = {{60, 12}, {28, 12}};
inline int64_t bwd_max_tiles(int H, int W) {
    auto ntiles = [&](int iw, int ih) { return (int64_t)((W + iw - 1) / iw) * ((H + ih - 1) / ih); };
    int64_t tiles = 0;
    for (int s = 0; s < BWD_NSHAPES; ++s) tiles = ntiles(bwd_interior_w(s), bwd_interior_h(s)) > tiles ? ntiles(bwd_interior_w(s), bwd_interior_h(s)) : tiles;
    for (const BwdRegion &r : BWD_SIZING_ONLY_INTERIORS) tiles = ntiles(r.width, r.rows) > tiles ? ntiles(r.width, r.rows) : tiles;
    return tiles;
}

// what BWD_AUTO takes where rule 4 gives it the 64 x 12 frame pairs: the kernel without the owner table (true) or with it, by the stack's
// texel type.  In process on one resident cfg3 stack (profiles/ab_inproc.py --variants 7,8,7): fp32 11.995 -> 11.634 ms (-3.0 %, 26x the
// spread of the repeated leg); fp16 9.194 -> 9.457 ms (+2.9 %: half the bytes per texel, and the owner arithmetic is no longer hidden).
// Measured under the planar convention; the utils_mpi cross-check convention keeps the table kernel whatever the type (its texel coordinates
// cost a reciprocal more, and two of its table-free instantiations spill 12 bytes at the 80-register budget where the table kernel's do not)
constexpr bool BWD_PAIR12_AUTO_OWNERLESS_F32 = true, BWD_PAIR12_AUTO_OWNERLESS_F16 = false;

// ---- the choice -------------------------------------------------------------------------------------------------------------------------
struct BwdChoice {
    int family;        // VL3D_BWD_ATOMICS | _TILE (render_bwd_tile_k) | _PAIR | _PAIR12 (render_bwd_pair_k in 32 x 16 | 64 x 12 regions)
    BwdShape shape;    // (unread for VL3D_BWD_ATOMICS)
    bool reg, mask, adam, cull, f16;      // the instantiation: layer regularisers' 128-register build, fifth channel, fused step, quad map, fp16 texels
    bool owner4;       // the owner table is built four texels per thread (bwd_owner_table4_k)
    bool ownerless;    // VL3D_BWD_PAIR12 only: no owner table (render_bwd_pair_k<..., OWNERLESS> behind bwd_zero_unowned_k).  Internal: vl3d_bwd_choice does not show it
};

// what the launch switches on: the instantiations differ in these (CULL and F16 are arguments of the chosen launch)
constexpr int bwd_key(int family, int shape, bool reg, bool mask = false, bool adam = false) {
    return family | shape << 2 | (int)reg << 5 | (int)mask << 6 | (int)adam << 7;
}
inline int bwd_key(const BwdChoice &c) { return bwd_key(c.family, c.shape, c.reg, c.mask, c.adam); }

struct BwdFacts {
    int coord, border, order, ract, aact;      // the compiled convention (VL3D_COORD_AFFINE_PLANES: VL3D_COORD_AFFINE with 16-float records)
    bool f16;
    int plane_record;                          // floats per plane of the homography table (VL3D_HS: 9, or 16 with per-plane transforms)
    int T, H, W, Hs, Ws;
    BwdSetting set;
    bool reg, mask, adam, qk, gcu;             // g_reg || g_asum | mask channel | fused optimiser step | quad map | grad_culled_unwritten
};

// First match wins.  The figures are the measurements each rule rests on.
inline BwdChoice choose_bwd(const BwdFacts &f) {
    const bool sig = f.ract == VL3D_ACT_SIGMOID && f.aact == VL3D_ACT_SIGMOID;
    // rule 4's own test (its comment is there): the calls that take the plain frame pairs
    const bool fits = (int64_t)f.Hs * 100 <= (int64_t)f.H * 107 || (int64_t)f.Ws * 100 <= (int64_t)f.W * 107;
    const bool plain_pairs = sig && f.T >= 2 && !f.qk && !f.adam && !f.mask && !f.reg && fits;
    // variant 8 names a kernel of rule 4 only: everywhere else it is the default (6 and 7, older, are variant 3 there)
    const BwdPolicy p = f.set.policy == BWD_PAIRS64X12O && !plain_pairs ? BWD_AUTO : f.set.policy;
    // the convention stage 1 and stage 2 ship (MPI.py / MPV.py planar path, sigmoid / sigmoid, fp32): the loop-mask channel, the fused step
    // and the narrow / flat one-frame shapes are built for it alone (the last three with 9-float plane records)
    const bool shipped = f.coord == VL3D_COORD_AFFINE && f.border == VL3D_BORDER_HARDCUT && f.order == VL3D_ACT_POST && sig && !f.f16;
    const bool shipped9 = shipped && f.plane_record == 9;
    BwdChoice c{VL3D_BWD_TILE, BWD_64X16, false, false, false, false, false, false, false};
    // (a single frame: four texels per thread; the fused optimiser step keeps its per-texel records)
    c.owner4 = f.T == 1 && !f.adam && f.set.owner4;
    // 0
    if (p == BWD_NONE) { c.family = VL3D_BWD_ATOMICS; c.owner4 = false; return c; }
    // 1: one frame per thread, fifth channel in the sweep and the gather (dense models only: the entry point refuses a quad map).  Flat 64 x 8
    // regions: 512 threads at this instantiation's 128-register budget are TWO workgroups per CU -- the 1024-thread regions run alone on theirs
    if (f.mask && shipped) { c.shape = p == BWD_FLAT8 ? BWD_64X8 : BWD_64X16; c.reg = f.reg; c.mask = true; return c; }
    if (f.adam && shipped9) {
        c.adam = true;
        // 2: tile-culled models, one frame per thread (the frame pairs are built for dense stacks).  32-wide regions unless variant 3 asks for
        // the 64-wide ones: two workgroups per CU, 0.60 against 0.71 ms per iteration of the tile-culled schedule,
        // docs/kernels/K2_render_backward.md round 5
        if (f.qk) { c.shape = p == BWD_TILE16 ? BWD_64X16 : BWD_32X16; c.reg = c.cull = true; return c; }
        // 3: the dense fused step rides the frame pairs -- the one-frame form measured 202 against 213-218 it/s
        c.family = VL3D_BWD_PAIR; c.shape = BWD_32X16; c.reg = f.reg;
        return c;
    }
    if (sig && f.T >= 2 && !f.qk) {
        // 4: two frames per thread, dense stacks without layer regularisers, when a 30 x 14-pixel tile's texel window fits the 32 x 16 threads
        // of its workgroup -- judged by the sizes alone (the homographies live on the device): along one axis at least the stack is no larger
        // than the frame (+7 %) -- full frames and row bands (dist.render_band: full width, rows = band + halo) of a stack at the frame's
        // resolution.  Beyond that the extra gather passes of the small tiles cost more than the pairs save (1.1x: 13.3 ms tile kernel,
        // 13.9 ms pairs): crops of a larger stack and the reference's 1.1x stacks keep the 64 x 16 tile kernel.
        // Two region shapes: 64 x 12 (62 x 10 owned, 768 threads) is the default, 32 x 16 the kernel it replaced there
        // (variant 6 keeps it: the A/B partner and the reference of the bitwise tests; variant 7 forces the 64 x 12 regions).
        // The 64 x 12 regions come with the owner table (variant 7) and without it (render_bwd_pair_k's OWNERLESS instantiations, variant 8: the
        // gather computes each texel's owner pixel -- VALU the kernel has to spare for memory instructions it has not); BWD_PAIR12_AUTO_OWNERLESS_*
        // say which of the two the default takes (docs/kernels/K2_render_backward.md, "64 x 12 pairs without the owner table").
        if ((p == BWD_AUTO || p == BWD_PAIRS32 || p == BWD_PAIRS64X12 || p == BWD_PAIRS64X12O) && !f.reg && fits) {
            c.family = p == BWD_PAIRS32 ? VL3D_BWD_PAIR : VL3D_BWD_PAIR12;
            c.shape = p == BWD_PAIRS32 ? BWD_32X16 : BWD_64X12;
            c.f16 = f.f16;
            c.ownerless = p == BWD_PAIRS64X12O ||
                          (p == BWD_AUTO && f.coord != VL3D_COORD_UTILS_MPI && (f.f16 ? BWD_PAIR12_AUTO_OWNERLESS_F16 : BWD_PAIR12_AUTO_OWNERLESS_F32));
            return c;
        }
        // 5: with the layer regularisers the pair kernel wins at every stack size (round 3, in process: 15.7 ms against 20.0 ms for the
        // one-frame tile kernel on a 1.1x stack, 15.4 against 19.6 ms at the frame's resolution: decoding the forward's sign words is
        // frame-pair work the tile kernel does once per frame).  The utils_mpi cross-check convention keeps the tile kernel: its texel
        // coordinates cost a reciprocal more and the pair instantiation spilled 8-28 bytes at 128 VGPRs.
        if (f.coord != VL3D_COORD_UTILS_MPI && p == BWD_AUTO && f.reg) {
            c.family = VL3D_BWD_PAIR; c.shape = BWD_32X16; c.reg = true; c.f16 = f.f16;
            return c;
        }
    }
    // 6: 32-wide one-frame regions (variant 5): half the workgroup, twice as many of them ... and the default of a tile-culled call under
    // VL3D_GRAD_CULLED_UNWRITTEN, which SKIPS the planes a tile cannot see: cfg3 at 16.5 % kept quads 3.7 ms at the plain kernel's register
    // budget (70 VGPRs, three workgroups per CU), 4.5-4.8 ms in the instantiation with the regularisers' 128 (variant 5), 5.1 ms in its 64-wide
    // form, profiles/r05b_cull_lean.txt.  A per-tile work list of the swept planes -- bit masks written by bwd_windows_k, scalar bit scans
    // instead of one record load per skipped plane -- measured the same 4.49 ms / 0.60 ms per schedule iteration: the skipped planes' scalar
    // loads are hidden, not built
    if (shipped9 && (p == BWD_NARROW32 || (p == BWD_AUTO && f.qk && f.gcu))) {
        c.shape = BWD_32X16; c.reg = f.reg || (p == BWD_NARROW32 && f.qk && f.gcu); c.cull = f.qk;
        return c;
    }
    // 7: flat 64 x 8 one-frame regions (512 threads, four workgroups per CU at the plain kernel's 64 registers) for a SINGLE frame (cfg2, the
    // stage-1 shape): 2520 workgroups on 1024 slots instead of 1092 on 512 -- the x1.33 halo costs less than the 2.13-round tail of the 16-row
    // regions: backward 0.380 against 0.394 ms at 720p, D = 32, same bits (profiles/r05d_cfg2_rows.txt; 10 rows 0.442, 12 rows 0.393: measured,
    // not instantiated).  Variant 2 forces them at any T (round 1 measured them 18.9 vs 16.8 ms at cfg3), variant 3 keeps the 16 rows.
    if (shipped9 && !f.reg && !f.qk && (p == BWD_FLAT8 || (p == BWD_AUTO && f.T == 1))) { c.shape = BWD_64X8; return c; }
    // 8: the 64 x 16 tile kernel.  Layer regularisers and / or sparsity sums: the REG instantiation (128-VGPR budget); a tile-culled call
    // whose consumer never reads culled texels takes it too -- it is the one that SKIPS the planes a tile cannot see instead of zero-filling them
    c.reg = f.reg || (f.qk && f.gcu); c.cull = f.qk; c.f16 = f.f16;
    return c;
}

}  // namespace vl3d_render_detail
