// From a render descriptor to the kernels' arguments, host side: the one place where vl3d_render_desc becomes RenderArgs and where the
// quad grid of a tile-culled model is checked and turned into the kernels' quotients.  Every render entry point (vl3d_render.hip, _packed,
// _baked, _baked_pool, _plane_rows, _label) starts from these; what an entry adds -- its own refusals, the frame offset of a run, g_f16 --
// stays at the entry.  The two baked entries also share their descriptor, selection and sink rules: the last section.
#pragma once
#include <string>
#include "vl3d_render_core.h"

namespace vl3d_render_detail {

// dims, window, pixel centre, texel transform and jitter seed; every pointer and option zero.  Tstride = T: an entry that reads a run of
// frames of a longer clip sets its own.
inline RenderArgs render_args_of(const vl3d_render_desc *d) {
    RenderArgs a{};
    a.D = d->D; a.T = d->T; a.Hs = d->Hs; a.Ws = d->Ws; a.H = d->H; a.W = d->W;
    a.Tstride = d->T;
    a.row0 = d->row0; a.col0 = d->col0;
    a.pc = d->pixel_center; a.sx = d->sx; a.sy = d->sy; a.ox = d->ox; a.oy = d->oy;
    a.uv_seed = d->uv_noise_seed;
    return a;
}

// the quad grid is laid over the whole plane; the stack may be a texel window of it (desc->cull_*: crop-aware training renders
// from a compact copy of the window the crop can reach, videoloop3d_amd/optim.py)
inline void set_cull_geometry(RenderArgs &a, const vl3d_render_desc *desc, int32_t QH, int32_t QW) {
    const bool win = desc->cull_Hs > 0 && desc->cull_Ws > 0;
    a.q_Hs = win ? desc->cull_Hs : desc->Hs;
    a.q_Ws = win ? desc->cull_Ws : desc->Ws;
    a.q_x0 = win ? (float)desc->cull_col0 : 0.0f;
    a.q_y0 = win ? (float)desc->cull_row0 : 0.0f;
    a.q_th = a.q_tw = 0;
    if (QH < 0 && QW < 0) {
        // TILE-EXACT layout (include/vl3d.h): the plane is |QH| x |QW| tiles of th x tw texels, every quad owning its border row / column; the
        // homography + (sx, ox) give LATTICE coordinates (a quad spans tw - 1 of them), the kernels add the quad index (make_taps_i)
        a.QH = -QH; a.QW = -QW;
        a.q_th = a.q_Hs / a.QH; a.q_tw = a.q_Ws / a.QW;
        a.q_inv_cw = 1.0f / (float)(a.q_tw > 1 ? a.q_tw - 1 : 1);
        a.q_inv_ch = 1.0f / (float)(a.q_th > 1 ? a.q_th - 1 : 1);
        return;
    }
    a.QH = QH; a.QW = QW;
    a.q_inv_cw = (float)QW / (float)(a.q_Ws > 1 ? a.q_Ws - 1 : 1);
    a.q_inv_ch = (float)QH / (float)(a.q_Hs > 1 ? a.q_Hs - 1 : 1);
}

// a refusal: `who: bad` as the error message
inline int refuse(const char *who, const char *bad) {
    vl3d_set_error((std::string(who) + ": " + bad).c_str());
    return VL3D_EINVAL;
}

// the rules every culled entry shares, `who` in front of the message: the signs of the grid, whole tiles of at least 2 x 2 texels in the
// tile-exact layout (of the plane the grid lies over: cull_Hs / cull_Ws when set), the stack window inside that plane, two 64-bit plane masks
inline int check_cull_grid(const vl3d_render_desc *desc, int32_t QH, int32_t QW, const char *who) {
    const char *bad = nullptr;
    const int pH = desc->cull_Hs > 0 ? desc->cull_Hs : desc->Hs, pW = desc->cull_Ws > 0 ? desc->cull_Ws : desc->Ws;
    if (!((QH > 0 && QW > 0) || (QH < 0 && QW < 0)))
        bad = "bad quad grid (both positive, or both negative for the tile-exact layout)";
    else if (QH < 0 && !(pH % (-QH) == 0 && pW % (-QW) == 0 && pH / (-QH) >= 2 && pW / (-QW) >= 2))
        bad = "bad quad grid (tile-exact layout: the plane must be |QH| x |QW| whole tiles of at least 2 x 2 texels)";
    else if (!((desc->cull_Hs == 0 && desc->cull_Ws == 0) ||
               (desc->cull_row0 >= 0 && desc->cull_col0 >= 0 && desc->cull_row0 + desc->Hs <= desc->cull_Hs && desc->cull_col0 + desc->Ws <= desc->cull_Ws)))
        bad = "the stack window (cull_row0, cull_col0) + (Hs, Ws) leaves the plane (cull_Hs, cull_Ws)";
    else if (desc->D > 128)
        bad = "tile culling supports at most 128 planes";
    return bad ? refuse(who, bad) : VL3D_OK;
}

// ---- baked playback (csrc/vl3d_render_baked.hip, vl3d_render_baked_pool.hip): the rules the two entries share, `who` in front ----------
// the descriptor of a baked render.  `max_texels`, `too_large`: the unit's own bound on a plane and its message (the dense clip forms 32-bit
// tap offsets, the pool does not)
inline int check_baked_desc(const vl3d_render_desc *desc, int64_t max_texels, const char *too_large, const char *who) {
    VL3D_REQUIRE(desc != nullptr, "null render desc");
    const char *bad = nullptr;
    if (desc->variant != 0) bad = "no kernel variants (desc->variant = 0)";
    else if (!(desc->D > 0 && desc->T > 0 && desc->H > 0 && desc->W > 0)) bad = "non-positive render dims";
    // the base tap is clamped to (Ws - 2, Hs - 2) and its right / lower neighbours are read unconditionally
    else if (!(desc->Hs >= 2 && desc->Ws >= 2)) bad = "planes of at least 2 x 2 texels";
    else if (!(desc->Hs < (1 << 24) && desc->Ws < (1 << 24) && (int64_t)desc->Hs * desc->Ws < max_texels)) bad = too_large;
    else if (desc->stack_dtype != VL3D_U8) bad = "stack_dtype must be VL3D_U8 (the baked RGBA8 texels of vl3d_bake_rgba8)";
    else if (!(desc->coord_mode == VL3D_COORD_AFFINE && desc->border_mode == VL3D_BORDER_HARDCUT))
        bad = "the planar MPV convention only (VL3D_COORD_AFFINE, VL3D_BORDER_HARDCUT)";
    else if (desc->uv_noise_seed != 0) bad = "add_uv_noise is a training switch (uv_noise_seed = 0)";
    return bad ? refuse(who, bad) : VL3D_OK;
}

// the selection: a run (no index pointers, n_cams = 0) or a camera path (both index pointers, n_cams in [1, 65535], tiles x frames inside
// the grid); `is_path` says which
inline int check_baked_frames(const vl3d_render_desc *desc, const vl3d_baked_frames *sel, bool &is_path, const char *who) {
    const char *bad = nullptr;
    if (!sel) bad = "null pointer (sel)";
    else if (!sel->frame_cam != !sel->frame_t || (!sel->frame_cam && sel->n_cams != 0))
        bad = "sel is neither a run (frame_cam = frame_t = NULL, n_cams = 0) nor a path (frame_cam, frame_t: device int32[desc->T], n_cams >= 1)";
    else if (sel->frame_cam && !(sel->n_cams >= 1 && sel->n_cams <= 65535)) bad = "n_cams must be in [1, 65535]";
    else if (sel->frame_cam && (int64_t)((desc->W + 63) / 64) * ((desc->H + 7) / 8) * desc->T > 0x7fffffffll) bad = "tiles x frames exceed the grid";
    if (bad) return refuse(who, bad);
    is_path = sel->frame_cam != nullptr;
    return VL3D_OK;
}

// the selection of a path in loop time: both pointers, reserved = 0, n_cams in [1, 65535], tiles x frames inside the grid
inline int check_baked_times(const vl3d_render_desc *desc, const vl3d_baked_times *sel, const char *who) {
    const char *bad = nullptr;
    if (!sel) bad = "null pointer (sel)";
    else if (!sel->frame_cam) bad = "null pointer (sel->frame_cam: device int32[desc->T])";
    else if (!sel->frame_time) bad = "null pointer (sel->frame_time: device float[desc->T])";
    else if (sel->reserved != 0) bad = "sel->reserved must be 0";
    else if (!(sel->n_cams >= 1 && sel->n_cams <= 65535)) bad = "n_cams must be in [1, 65535]";
    else if ((int64_t)((desc->W + 63) / 64) * ((desc->H + 7) / 8) * desc->T > 0x7fffffffll) bad = "tiles x frames exceed the grid";
    return bad ? refuse(who, bad) : VL3D_OK;
}

// the sink: exactly one of (rgb and alpha) or frames -- the display sink's own rules are display_out_of's (vl3d_baked_core.h)
inline int check_baked_out(const vl3d_baked_out *out, const char *who) {
    const char *bad = nullptr;
    if (!out) bad = "null pointer (out)";
    else if (out->frames && (out->rgb || out->alpha)) bad = "out names both sinks (rgb and alpha, or frames)";
    else if (!out->frames && !(out->rgb && out->alpha)) bad = "null pointer (out: rgb and alpha, or frames)";
    else if (!out->frames && out->bg) bad = "a background colour belongs to the display sink (out->frames)";
    return bad ? refuse(who, bad) : VL3D_OK;
}

}  // namespace vl3d_render_detail
