// Which path a video conversion runs, as a value: the descriptor check, the rule's integer tables and choose_video() -- a pure function of
// the call's facts.  Host only: no HIP in here (plain g++ -std=c++17 compiles it).  vl3d_video.hip switches on the choice;
// vl3d_video_choice() (include/vl3d.h) shows it to tests.
#pragma once
#include <stdint.h>
#include "vl3d.h"

namespace vl3d_video_detail {

// ---- the rule's integers (y4m.encode_coefs / y4m.decode_coefs; tests/test_y4m_cpu.py holds this table to them) ---------------------------
struct VideoCoefs {
    int32_t enc[9], off[3];      // rows Y, U, V at 2^16; offsets
    int32_t dec[9], y0;          // per output channel (cy at 2^21, cu, cv at 2^17); luma offset
};
constexpr VideoCoefs VIDEO_COEFS[2][2] = {      // [matrix][full_range]
    {{{16829, 33039, 6416, -9714, -19071, 28785, 28784, -24103, -4681}, {16, 128, 128},
      {2441889, 0, 209194, 2441889, -51349, -106557, 2441889, 264403, 0}, 16},      // BT.601 limited
     {{19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329}, {0, 128, 128},
      {2097152, 0, 183763, 2097152, -45107, -93603, 2097152, 232260, 0}, 0}},       // BT.601 full
    {{{11966, 40254, 4064, -6596, -22189, 28785, 28784, -26145, -2639}, {16, 128, 128},
      {2441889, 0, 234978, 2441889, -27951, -69849, 2441889, 276877, 0}, 16},       // BT.709 limited
     {{13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005}, {0, 128, 128},
      {2097152, 0, 206412, 2097152, -24553, -61358, 2097152, 243217, 0}, 0}},       // BT.709 full
};

constexpr int VIDEO_STRIP = 16;          // luma pixels of a row a wide thread owns: one 16-byte access of Y
constexpr int VIDEO_THREADS = 256;
constexpr int64_t VIDEO_MAX_PIXELS = 2147483647;      // N H W: every thread index and every workgroup count fits int32

struct VideoChoice {
    int status;
    const char *msg;      // static text for vl3d_set_error when status != VL3D_OK
    int wide, strip, rows, threads;
    int64_t items;        // threads with work
    int32_t blocks;
    int ch, cw;           // chroma plane size
};

inline bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// the descriptor's refusals, then the path.  `rgb`: the dense RGB side; `decode`: vl3d_yuv8_to_rgb.
inline VideoChoice choose_video(const vl3d_video_desc *d, const void *rgb, bool decode) {
    VideoChoice c{VL3D_EINVAL, nullptr, 0, 0, 0, VIDEO_THREADS, 0, 0, 0, 0};
    const char *who_rgb = decode ? "vl3d_yuv8_to_rgb: null rgb (the frames to write)" : "vl3d_rgb8_to_yuv8: null rgb (the frames to read)";
    if (!d) { c.msg = "video conversion: null descriptor"; return c; }
    if (!rgb) { c.msg = who_rgb; return c; }
    if (!d->y || !d->u || !d->v) { c.msg = "video conversion: a null plane pointer (desc->y, u, v)"; return c; }
    if (d->N < 1 || d->H < 1 || d->W < 1) { c.msg = "video conversion: N, H and W must be at least 1"; return c; }
    if (d->chroma != VL3D_CHROMA_444 && d->chroma != VL3D_CHROMA_420) { c.msg = "video conversion: desc->chroma is VL3D_CHROMA_444 or VL3D_CHROMA_420"; return c; }
    if (d->siting_x != VL3D_SITING_CENTER && d->siting_x != VL3D_SITING_LEFT) { c.msg = "video conversion: desc->siting_x is VL3D_SITING_CENTER or VL3D_SITING_LEFT"; return c; }
    if (d->matrix != VL3D_MATRIX_BT601 && d->matrix != VL3D_MATRIX_BT709) { c.msg = "video conversion: desc->matrix is VL3D_MATRIX_BT601 or VL3D_MATRIX_BT709"; return c; }
    if (d->full_range != 0 && d->full_range != 1) { c.msg = "video conversion: desc->full_range is 0 (limited) or 1 (full)"; return c; }
    if (d->sink != VL3D_SINK_U8 && d->sink != VL3D_SINK_F32) { c.msg = "video conversion: desc->sink is VL3D_SINK_U8 or VL3D_SINK_F32"; return c; }
    if (d->path != VL3D_VIDEO_PATH_AUTO && d->path != VL3D_VIDEO_PATH_BYTE) { c.msg = "video conversion: desc->path is VL3D_VIDEO_PATH_AUTO or VL3D_VIDEO_PATH_BYTE"; return c; }
    const bool f32 = decode && d->sink == VL3D_SINK_F32;
    if (f32 ? d->channels != 3 : (d->channels != 3 && d->channels != 4)) {
        c.msg = f32 ? "vl3d_yuv8_to_rgb: the float sink is [N,3,H,W]: desc->channels must be 3" : "video conversion: desc->channels must be 3 (RGB8) or 4 (RGBA8)";
        return c;
    }
    const int64_t pixels = (int64_t)d->N * d->H * d->W;
    if (pixels > VIDEO_MAX_PIXELS) { c.msg = "video conversion: N * H * W exceeds 2^31 - 1, the grid limit: convert the frames in several calls"; return c; }
    const bool c420 = d->chroma == VL3D_CHROMA_420;
    c.ch = c420 ? (d->H + 1) / 2 : d->H;
    c.cw = c420 ? (d->W + 1) / 2 : d->W;
    const int64_t frame = (int64_t)d->H * d->W + 2 * (int64_t)c.ch * c.cw;
    if (d->frame_stride < frame) { c.msg = "video conversion: desc->frame_stride is smaller than a frame (H W + 2 ch cw bytes)"; return c; }
    if (f32 && !aligned(rgb, 4)) { c.msg = "vl3d_yuv8_to_rgb: the float sink is not 4-byte aligned"; return c; }

    // wide: every 16-byte access of Y and of the RGB side and every 8-byte access of U / V is aligned, in every row of every frame
    const bool wide = d->path == VL3D_VIDEO_PATH_AUTO && d->W % VIDEO_STRIP == 0 && (!c420 || d->H % 2 == 0) && aligned(rgb, 16)
                      && aligned(d->y, 16) && aligned(d->u, c420 ? 8 : 16) && aligned(d->v, c420 ? 8 : 16) && d->frame_stride % 16 == 0;
    c.wide = wide ? 1 : 0;
    if (wide) {
        c.strip = VIDEO_STRIP;
        c.rows = c420 ? 2 : 1;
        c.items = pixels / (c.strip * c.rows);
    } else if (decode) {
        c.strip = c.rows = 1;                          // a thread per pixel
        c.items = pixels;
    } else {
        c.strip = c.rows = c420 ? 2 : 1;               // a thread per chroma sample: its 2 x 2 block, clipped to the frame
        c.items = (int64_t)d->N * c.ch * c.cw;
    }
    c.blocks = (int32_t)((c.items + VIDEO_THREADS - 1) / VIDEO_THREADS);
    c.status = VL3D_OK;
    return c;
}

}  // namespace vl3d_video_detail
