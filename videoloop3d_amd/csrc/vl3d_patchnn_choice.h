// Which kernel the patch nearest-neighbour search and the vote-fold run, as values: the patch grid every loss entry derives from its descriptor,
// the tables of instantiations, choose_patchnn() and choose_fold() -- pure functions of a call's facts -- and the scratch size.  Host only: no
// HIP in here (plain g++ -std=c++17 compiles it; the stand-alone program tests/patchnn_choice_cases.cpp runs it under the sanitizers).  The
// entry points (vl3d_loss.hip, vl3d_fold.hip) switch on the choice; vl3d_patchnn_choice() / vl3d_vote_fold_choice() (include/vl3d.h) show it to
// tests.
#pragma once
#include <stdint.h>
#include "vl3d.h"

namespace vl3d_loss_detail {

// ---- the patch grid (include/vl3d.h, "Looping loss"): derived ONCE from a descriptor check_loss() has admitted ------------------------------
constexpr int TI = 4, TJ = 4;      // per-thread register tile of frame pairs (kernels 2 and 4)
struct PatchGrid {
    int h_o, w_o, n1, n2;
    int TxU;             // frames of x actually covered by patches
    int TxP, TyP;        // TxU / Ty padded to multiples of TI / TJ
    int K;               // 3 * ps * ps
};
inline PatchGrid patch_grid_of(const vl3d_loss_desc *d) {
    PatchGrid g{};
    g.h_o = (d->H - d->ps) / d->stride + 1;
    g.w_o = (d->W - d->ps) / d->stride + 1;
    g.n1 = (d->Tx - d->pt) / d->stridet + 1;
    g.n2 = (d->Ty - d->pt) / d->stridet + 1;
    g.TxU = (g.n1 - 1) * d->stridet + d->pt;
    g.TxP = (g.TxU + TI - 1) / TI * TI;
    g.TyP = (d->Ty + TJ - 1) / TJ * TJ;
    g.K = 3 * d->ps * d->ps;
    return g;
}

// ---- LDS limits (bytes of dynamic LDS per workgroup on a 160-KiB CU) ------------------------------------------------------------------------
constexpr int LDS_NN2_TARGET = 48 * 1024;      // kernel 2's staging chunk aims at three workgroups per CU
constexpr int LDS_3_PER_CU = 53 * 1024;        // three workgroups per CU (the fold's first choice; kernel 6 stages two halves of it)
constexpr int LDS_2_PER_CU = 79 * 1024;
constexpr int LDS_MAX = 150 * 1024;            // one workgroup per CU: the most any of these kernels asks for
constexpr int FOLD_BUDGETS[] = {LDS_3_PER_CU, LDS_2_PER_CU, LDS_MAX};

// ---- the tables ------------------------------------------------------------------------------------------------------------------------------
// kernel 6 (split-f16 matrix cores): a wave holds TYT 16-frame y tiles of NL neighbouring locations; x in 16 NW frames (NW = 4 / 8 waves);
// XS = 16 (tiles abut, workgroup-wide epilogue) or 14 (tiles overlap by pt - 1, every wave finishes its own patches).  3 x 2 x 2 instantiations.
struct NN6Shape { int tyt, nl; };
constexpr NN6Shape NN6_SHAPES[] = {{5, 4}, {8, 2}, {12, 1}};
constexpr int NN6_KX = 3;                                                           // DMA pieces per wave and stage: x ...
constexpr int nn6_ky(int tyt) { return tyt == 5 ? 4 : (tyt == 8 ? 6 : 7); }        // ... and y
// kernel 4 (vector ALU, NL4 locations per workgroup): one 4 x 4 frame-pair tile per thread; <RUNSUM, threads> instantiations
constexpr int NL4 = 4;
constexpr int NN4_THREADS[] = {256, 512, 1024};
// kernel 2 (one location per workgroup)
constexpr int NN_THREADS = 256;

// LDS-staged fold: tile shapes {FT_W, FT_H, threads}.  The whole Ty column of a tile has to sit in LDS (an NN index may point at
// any frame), so the tile area sets the LDS footprint and with it how many workgroups share a CU.  A 32x8 tile of a 75-frame clip
// (77 KiB + indices) runs ONE workgroup per CU, whose staging and voting phases never overlap with another's: 1.55 ms at 720p.
// 64x2 (three workgroups per CU, 256-byte row segments) measured 1.20 ms, 32x4 1.27, 32x2 1.28, 64x1 1.60 in one process
// (profiles/ab_fold.py; outputs bit-equal across shapes).  The narrower shapes are for clips whose columns do not fit otherwise.
struct FoldShape { int fw, fh, nt; };
constexpr FoldShape fold_shapes[] = {{64, 2, 512}, {32, 4, 512}, {32, 2, 256}, {64, 1, 256}, {32, 1, 256}};
constexpr int N_FOLD_SHAPES = sizeof(fold_shapes) / sizeof(fold_shapes[0]);
// most patch locations b (b*stride <= last, b*stride + ps - 1 >= first) covering a span of f pixels that starts at a multiple of f
inline int fold_cover(int f, int ps, int stride) {
    int most = 0;
    for (int k = 0; k < stride; ++k) {
        const int first = (k + stride * ps) * f, last = first + f - 1;      // every residue of the tile origin, away from the border
        const int n = last / stride - (first - ps + stride) / stride + 1;
        most = n > most ? n : most;
    }
    return most;
}
inline int64_t fold_lds_bytes(const vl3d_loss_desc *d, int n1, const FoldShape &sh) {
    const int nby_max = fold_cover(sh.fh, d->ps, d->stride), nbx_max = fold_cover(sh.fw, d->ps, d->stride);
    // y columns + three zero frames | index rows of the covering locations + one row pointing at the zero frames
    return ((int64_t)(d->Ty + 3) * sh.fw * sh.fh + ((int64_t)nby_max * nbx_max + 1) * n1) * 4;
}

// ---- the scratch of vl3d_patchnn / vl3d_patchnn_prepared (ABI: callers allocate by it) -----------------------------------------------------
// the larger of the two layouts: kernel 6's gram16 (16 bytes per pixel and frame) and the pixel-major copies of kernels 2 and 4 (3 floats,
// frames padded to TI / TJ)
inline int64_t patchnn_scratch_bytes(const vl3d_loss_desc *d) {
    if (!d || d->H <= 0 || d->W <= 0 || d->stridet <= 0) return 0;
    const PatchGrid g = patch_grid_of(d);
    const int64_t gram16 = 16 * ((int64_t)g.TxU + d->Ty), pixel_major = 12 * ((int64_t)g.TxP + g.TyP);
    return (int64_t)d->H * d->W * (gram16 > pixel_major ? gram16 : pixel_major);
}

// ---- the search's choice -------------------------------------------------------------------------------------------------------------------
struct PatchNNFacts {
    const vl3d_loss_desc *d;      // admitted by check_loss()
    int entry;                    // VL3D_NN_ENTRY_PLAIN (vl3d_patchnn) | _PREPARED (y in gram16 form) | _GRAMS (x and y in gram16 form)
    bool has_scratch;
    int x_pitch, x_frames;        // _GRAMS: pixels per row / frames per pixel of the x clip in memory
    int y_pitch;                  // _PREPARED, _GRAMS: pixels per row of the prepared y clip
};
struct PatchNNChoice : vl3d_nn_choice {
    int status;                   // VL3D_OK | VL3D_EINVAL | VL3D_EUNSUPPORTED
    const char *msg;              // static text for vl3d_set_error when status != VL3D_OK
};
constexpr int nn6_key(int tyt, int nw, int xs) { return tyt | nw << 8 | xs << 16; }      // what the kernel-6 launch switches on

// First match wins.  desc->variant bits 0-3 (pv): 0 the default, 6 / 4 / 2 name a kernel, 1 and every value not named below run kernel 2.
inline PatchNNChoice choose_patchnn(const PatchNNFacts &f) {
    const vl3d_loss_desc *d = f.d;
    const PatchGrid g = patch_grid_of(d);
    const bool x_gram = f.entry == VL3D_NN_ENTRY_GRAMS, prepared = f.entry != VL3D_NN_ENTRY_PLAIN;
    const int pv = d->variant & 0xf;
    PatchNNChoice c{};
    auto refuse = [&c](int status, const char *msg) { c = PatchNNChoice{}; c.status = status; c.msg = msg; return c; };

    // 0: kernel 2's plan comes first at every entry: LDS (floats) = Xs[KC][TxP] | Ys[KC][TyP] | E[TxP][TyP] | colmin[n2], the k = 3 ps^2 terms
    // staged KC at a time -- 32 at least where that fits, 8 at the very least.  A frame-pair matrix that leaves no room for 8 fits no kernel.
    const int64_t fixed = ((int64_t)g.TxP * g.TyP + g.n2) * 4, per_k = (int64_t)(g.TxP + g.TyP) * 4;
    if (fixed + 8 * per_k > LDS_MAX) return refuse(VL3D_EINVAL, "loss: Tx*Ty frame-pair matrix does not fit in LDS (Tx*Ty too large for these kernels)");
    int64_t budget2 = LDS_NN2_TARGET;
    if (fixed + 32 * per_k > budget2) budget2 = fixed + 32 * per_k < LDS_MAX ? fixed + 32 * per_k : LDS_MAX;
    const int kc_fit = (int)((budget2 - fixed) / per_k);
    c.kc = kc_fit < g.K ? kc_fit : g.K;
    const int64_t lds2 = fixed + c.kc * per_k;

    // 1: the search reads copies of the videos in its own layouts: without a scratch buffer to keep them in there is no kernel (the one that
    // gathered strided row segments -- 13.0 ms at 720p, almost all of it staging -- ran only here and was removed)
    if (f.entry == VL3D_NN_ENTRY_PLAIN && !f.has_scratch)
        return refuse(VL3D_EINVAL, "vl3d_patchnn: scratch is NULL: pass a buffer of vl3d_patchnn_scratch_bytes(desc) bytes");
    if (f.entry == VL3D_NN_ENTRY_PREPARED && !f.has_scratch)
        return refuse(VL3D_EINVAL, "vl3d_patchnn_prepared: needs the scratch buffer (x's gram16 copy)");
    if (prepared && pv != 0 && pv != 6) return refuse(VL3D_EINVAL, "vl3d_patchnn: prepared (gram16) inputs run on the default kernel only");

    // 2: kernel 6's plan: instantiation, stage size, LDS bytes.  x in at most 16 NW frames, y in at most 16 TYT.
    const int FX = g.TxU, FY = d->Ty, TyT = (FY + 15) / 16;
    const int Wx = x_gram ? f.x_pitch : d->W, FXm = x_gram ? f.x_frames : g.TxU, Wy = prepared ? f.y_pitch : d->W;
    // every wave finishes its own 14 patches (no alpha, three-frame patches at temporal stride 1, and the clip fits the overlapping tiles: the
    // column minima of the alpha path need all rows); variant bit 11 (0x800): the workgroup-wide epilogue also without alpha (cross-checks)
    const int nw14 = FX <= 58 ? 4 : 8;
    const int xs = (!(d->variant & 0x800) && !d->use_alpha && d->pt == 3 && d->stridet == 1 && g.n1 <= 14 * nw14 && FX <= 14 * nw14 + 2) ? 14 : 16;
    const int nw = xs == 14 ? nw14 : (FX <= 64 ? 4 : 8);
    NN6Shape sh = NN6_SHAPES[2];
    for (int i = 2; i >= 0; --i)
        if (TyT <= NN6_SHAPES[i].tyt) sh = NN6_SHAPES[i];
    const int RWc = d->ps + (sh.nl - 1) * d->stride;
    const int64_t cell = (int64_t)16 * (FX + FY), over = (int64_t)(16 * sh.tyt - FY + 16 * nw) * 16;      // (the tiles' over-read past the last cell)
    const int64_t pieces_x = (int64_t)NN6_KX * nw * 64, pieces_y = (int64_t)nn6_ky(sh.tyt) * nw * 64;    // KX / KY pieces per wave
    int ch = (int)((LDS_3_PER_CU / 2) / (cell * d->ps));
    ch = ch < 1 ? 1 : (ch > RWc ? RWc : ch);
    while (ch > 1 && ((int64_t)ch * d->ps * FX > pieces_x || (int64_t)ch * d->ps * FY > pieces_y)) --ch;
    const int64_t stage = 2 * (int64_t)ch * d->ps * cell + over;
    const int EP = ((g.TyP + 3) & ~7) + 4;
    const int64_t ebuf = xs == 16 ? (int64_t)g.TxP * g.TyP : (int64_t)nw * 17 * EP;
    const int64_t epi = (ebuf + (int64_t)sh.nl * (3 * ((g.n2 + 3) & ~3) + g.TyP + 16 * nw)) * 4;
    const int64_t lds6 = stage > epi ? stage : epi;
    const bool fits6 = FX <= 16 * nw && TyT <= 12 && lds6 <= LDS_MAX && (int64_t)ch * d->ps * FX <= pieces_x && (int64_t)ch * d->ps * FY <= pieces_y &&
                       ((int64_t)d->ps * Wx + ch) * FXm < (1 << 24) && ((int64_t)d->ps * Wy + ch) * FY < (1 << 24) &&      // 24-bit DMA offsets
                       16 * nw + g.TyP <= 64 * nw;                                                                          // side threads
    // kernel 4 has a thread per frame-pair tile
    const int ntiles4 = (g.TxP / TI) * (g.TyP / TJ);
    const bool v4_has_tiles = ntiles4 <= NN4_THREADS[2];
    // 3: kernel 6 wherever the clip lengths fit its instantiations -- prepared inputs have no other kernel, variant 6 asks for it, and it is
    // the default except with ONE location per workgroup where kernel 4 has a thread per tile: there kernel 4's four locations win (82 x 150
    // frames: 41 | 56 it/s, so kernel 4 keeps the one-location-per-wave case)
    if (fits6 && (prepared || pv == 6 || (pv == 0 && !(sh.nl == 1 && v4_has_tiles)))) {
        c.kernel = 6; c.tyt = sh.tyt; c.nl = sh.nl; c.nw = nw; c.xs = xs; c.ch = ch; c.threads = 64 * nw;
        c.lds_bytes = (int32_t)lds6; c.scratch_layout = VL3D_NN_LAYOUT_GRAM16;
        return c;
    }
    if (prepared)
        return refuse(VL3D_EUNSUPPORTED, "vl3d_patchnn_prepared: these clip lengths / this frame width are outside the matrix-core kernel's range; use vl3d_patchnn");
    if (pv == 3 || pv == 6)
        return refuse(VL3D_EINVAL, "vl3d_patchnn: variant 3 (the fp32 matrix-core kernel) was removed in round 5; variant 6 needs clip lengths within the matrix-core kernel's range");
    c.scratch_layout = VL3D_NN_LAYOUT_PIXEL_MAJOR;
    // 4: kernel 4 (NL4 locations per workgroup, column sums; the default and variant 4) whenever one thread per frame-pair tile suffices: 256
    // threads for the shipped clips, 512 / 1024 for longer ones.  Its epilogue aliases the staging buffers.
    const int RWc4 = d->ps + (NL4 - 1) * d->stride;
    const int64_t stage4 = (int64_t)RWc4 * 3 * (g.TxP + g.TyP), epi4 = (int64_t)g.TxP * g.TyP + 3 * (g.n2 + 3);
    const int64_t lds4 = (stage4 > epi4 ? stage4 : epi4) * 4;
    if ((pv == 0 || pv == 4) && v4_has_tiles && lds4 <= LDS_MAX) {
        c.kernel = 4;
        c.threads = ntiles4 <= NN4_THREADS[0] ? NN4_THREADS[0] : (ntiles4 <= NN4_THREADS[1] ? NN4_THREADS[1] : NN4_THREADS[2]);
        // running sums pay when ps >= 2 * stride: a column is shared by >= 2 locations on average (ps 11 / stride 4: 2.75; ps 3 / stride 2:
        // 1.5) -- but the running-sum form needs 6 registers more than the 128 a 1024-thread workgroup has: per-column adds there
        c.runsum = d->ps >= 2 * d->stride && c.threads < NN4_THREADS[2];
        c.lds_bytes = (int32_t)lds4;
        return c;
    }
    // 5: kernel 2 (variants 1 and 2 by name, long clips by need)
    c.kernel = 2; c.threads = NN_THREADS; c.lds_bytes = (int32_t)lds2;
    return c;
}

// ---- the fold's choice ---------------------------------------------------------------------------------------------------------------------
struct FoldChoice : vl3d_fold_choice {
    int status;
    const char *msg;
};
// `fused`: vl3d_vote_fold_robust* (the staged kernel or nothing); else vl3d_vote_fold (desc->variant bits 0-3 == 1: the unstaged kernel).
// The staged shape: variant bits 12-15 (measurement hook: shape index + 1) when that shape fits; else the first shape that leaves room for
// three workgroups per CU, then two, then one.
inline FoldChoice choose_fold(const vl3d_loss_desc *d, bool fused) {
    FoldChoice c{};
    if (d->Tx > 65535) { c.status = VL3D_EINVAL; c.msg = "vl3d_vote_fold: Tx > 65535"; return c; }
    const int n1 = patch_grid_of(d).n1;
    int shape = -1;
    const int forced = ((d->variant >> 12) & 15) - 1;
    if (forced >= 0 && forced < N_FOLD_SHAPES && fold_lds_bytes(d, n1, fold_shapes[forced]) <= LDS_MAX) shape = forced;
    for (int budget : FOLD_BUDGETS)
        for (int i = 0; i < N_FOLD_SHAPES && shape < 0; ++i)
            if (fold_lds_bytes(d, n1, fold_shapes[i]) <= budget) shape = i;
    c.status = VL3D_OK;
    if (shape < 0 && fused) {
        c.status = VL3D_EUNSUPPORTED; c.msg = "vl3d_vote_fold_robust: tile does not fit LDS; use vl3d_vote_fold + vl3d_robust_fwd/bwd";
        return c;
    }
    if (shape < 0 || (!fused && (d->variant & 0xf) == 1)) { c.shape = -1; c.threads = 256; return c; }      // the unstaged kernel: one thread per voxel
    c.staged = 1; c.shape = shape; c.fw = fold_shapes[shape].fw; c.fh = fold_shapes[shape].fh; c.threads = fold_shapes[shape].nt;
    c.lds_bytes = (int32_t)fold_lds_bytes(d, n1, fold_shapes[shape]);
    // fixed-trip covering loops for the patch-major form when a pixel has at most 2 x 2 / 3 x 3 covering locations (the shipped
    // configurations); variant bit 9 keeps the dynamic loops (A/B, cross-checks: same bits)
    const int cover = (d->ps + d->stride - 1) / d->stride;
    const bool slide = d->pt == 3 && d->stridet == 1 && !(d->variant & 0x200);
    c.nb = slide && cover == 3 ? 3 : (slide && cover <= 2 ? 2 : 0);
    return c;
}

}  // namespace vl3d_loss_detail
