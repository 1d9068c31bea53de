// K10 -- video I/O: 8-bit RGB frames <-> planar Y'CbCr as a YUV4MPEG2 payload holds it (include/vl3d.h "Video I/O",
// docs/kernels/K10_video_io.md).  Two stand-alone stream kernels per direction; nothing here is shared with the render kernels.
//
// THE RULE is y4m.rgb8_to_yuv8 / y4m.yuv8_to_rgb8 (integers only); enc_byte() and dec_byte() below are its two formulas and every kernel
// of this file stores what they return, so the wide and the byte path cannot differ in a byte.
//
// Paths (chosen per launch by choose_video(), vl3d_video_choice.h):
//   wide   a thread owns a strip of 16 luma pixels x 2 rows (1 row at 4:4:4).  Encode: 48 (RGB8) or 64 (RGBA8) bytes loaded per row as
//          16-byte accesses, 16 bytes of Y stored per row, 8 bytes each of U and V (16 at 4:4:4).  Decode: the mirror image -- 16 bytes of
//          Y per row, 8 bytes of each chroma row it blends (plus the two neighbour samples, single bytes), 48 / 64 bytes of RGB stored per
//          row, or 3 x 64 bytes of float.  Lane i sits 16 luma pixels after lane i - 1: a wave covers 1024 consecutive pixels of a row
//          pair, every byte of every line it touches is used.
//   byte   everything else (odd W or H, W not a multiple of 16, planes at odd addresses, a stride that is no multiple of 16): single-byte
//          accesses.  Encode: a thread per chroma sample owns its 2 x 2 block clipped to the frame; decode: a thread per pixel.
// Plain C++ loads and stores; no LDS, no atomics, no cross-lane traffic; every thread is independent.
//
// Bounds that cannot be crossed.  A thread's item index is below c.items (choose_video) or it returns before any access.
//   byte encode  items = N ch cw -> (n, cj, ci) with n < N, cj < ch, ci < cw.  Loads: rows min(2 cj + k, H - 1), columns min(2 ci + k, W - 1)
//                (k in {0, 1}; at 4:4:4 row cj, column ci): inside the frame.  Y is stored only where 2 cj + k < H and 2 ci + k < W; U and V at
//                cj cw + ci < ch cw.
//   byte decode  items = N H W -> (n, r, x), r < H, x < W.  Chroma rows r >> 1 <= ch - 1 and its neighbour clamped to [0, ch - 1]; columns
//                likewise in [0, cw - 1].  One pixel stored at (n, r, x).
//   wide         W = 16 m, and at 4:2:0 H = 2 h: items = N (H / rows) m -> (n, j, s), j < H / rows, s < m.  Luma rows rows j + k < H, columns
//                16 s .. 16 s + 15 < W.  Chroma (4:2:0): row j and its neighbours clamped to [0, ch - 1]; columns 8 s .. 8 s + 7 < cw = 8 m, the
//                neighbour columns max(8 s - 1, 0) and min(8 s + 8, cw - 1).  All offsets are 64-bit; frame n of a plane starts at
//                n frame_stride, and (N - 1) frame_stride + frame bytes is what the caller allocated (the entry refuses a stride below the
//                frame).  The RGB side is dense: pixel index < N H W <= 2^31 - 1.
#include "vl3d_common.h"
#include "vl3d_video_choice.h"

namespace {
using namespace vl3d_video_detail;

struct VideoArgs {
    int32_t N, H, W, ch, cw;
    int64_t stride;
    uint8_t *y, *u, *v;
    int64_t items;
    VideoCoefs k;
    int32_t we0, we1, wo0, wo1;      // decode, 4:2:0, horizontal weights x 4: even column (own, left neighbour), odd column (own, right neighbour)
};

// clamp((acc >> SHIFT), 0, 255), written as the clamp of the accumulator FIRST and the shift second (the same value: both steps are
// monotone).  In the other order hipcc fuses pairs of bytes into the packed shift-and-saturate instruction of gfx950 and assumes the upper
// half of its result to be zero, which the bytes the wide kernels pack next to it showed it is not (docs/kernels/K10_video_io.md, "A
// packing hazard").
template <int SHIFT>
__device__ __forceinline__ uint32_t shift_clamp_byte(int32_t acc) {
    constexpr int32_t top = (256 << SHIFT) - 1;
    acc = acc < 0 ? 0 : (acc > top ? top : acc);
    return (uint32_t)acc >> SHIFT;
}

// the encode formula: row `i` of the matrix on (r, g, b) -- single samples (shift 16) or 2 x 2 sums (shift 18)
template <int SHIFT>
__device__ __forceinline__ uint32_t enc_byte(const VideoCoefs &k, int i, int32_t r, int32_t g, int32_t b) {
    const int32_t acc = k.enc[3 * i] * r + k.enc[3 * i + 1] * g + k.enc[3 * i + 2] * b + (k.off[i] << SHIFT) + (1 << (SHIFT - 1));
    return shift_clamp_byte<SHIFT>(acc);
}

// the decode formula: channel c from the luma byte and 16 x chroma
__device__ __forceinline__ uint32_t dec_byte(const VideoCoefs &k, int c, int32_t Y, int32_t U16, int32_t V16) {
    const int32_t acc = k.dec[3 * c] * (Y - k.y0) + k.dec[3 * c + 1] * (U16 - 2048) + k.dec[3 * c + 2] * (V16 - 2048) + (1 << 20);
    return shift_clamp_byte<21>(acc);
}

__device__ __forceinline__ float unit_of(uint32_t b) { return (float)b / 255.0f; }      // IEEE division: the rule's byte / 255

__device__ __forceinline__ uint32_t word_byte(const uint32_t *w, int b) { return (w[b >> 2] >> ((b & 3) * 8)) & 255u; }

// ---- encode, byte path: a thread per chroma sample --------------------------------------------------------------------------------------
template <bool C420>
__global__ void __launch_bounds__(VIDEO_THREADS) rgb8_to_yuv8_byte_k(VideoArgs a, const uint8_t *__restrict__ rgb, int C) {
    const int64_t idx = (int64_t)blockIdx.x * VIDEO_THREADS + threadIdx.x;
    if (idx >= a.items) return;
    const uint32_t id = (uint32_t)idx;      // items <= N H W <= 2^31 - 1
    const int ci = (int)(id % (uint32_t)a.cw);
    const uint32_t t = id / (uint32_t)a.cw;
    const int cj = (int)(t % (uint32_t)a.ch), n = (int)(t / (uint32_t)a.ch);
    const int64_t f = (int64_t)n * a.stride;
    if constexpr (!C420) {
        const uint8_t *p = rgb + (((int64_t)n * a.H + cj) * a.W + ci) * C;
        const int32_t r = p[0], g = p[1], b = p[2];
        const int64_t o = f + (int64_t)cj * a.W + ci;
        a.y[o] = (uint8_t)enc_byte<16>(a.k, 0, r, g, b);
        a.u[o] = (uint8_t)enc_byte<16>(a.k, 1, r, g, b);
        a.v[o] = (uint8_t)enc_byte<16>(a.k, 2, r, g, b);
    } else {
        int32_t sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int yy = 2 * cj + dy, xx = 2 * ci + dx;
                const int yc = yy < a.H ? yy : a.H - 1, xc = xx < a.W ? xx : a.W - 1;
                const uint8_t *p = rgb + (((int64_t)n * a.H + yc) * a.W + xc) * C;
                const int32_t r = p[0], g = p[1], b = p[2];
                sr += r; sg += g; sb += b;
                if (yy < a.H && xx < a.W) a.y[f + (int64_t)yy * a.W + xx] = (uint8_t)enc_byte<16>(a.k, 0, r, g, b);
            }
        }
        const int64_t o = f + (int64_t)cj * a.cw + ci;
        a.u[o] = (uint8_t)enc_byte<18>(a.k, 1, sr, sg, sb);
        a.v[o] = (uint8_t)enc_byte<18>(a.k, 2, sr, sg, sb);
    }
}

// ---- encode, wide path: a thread per strip of 16 luma pixels x ROWS rows -----------------------------------------------------------------
template <int C, bool C420>
__global__ void __launch_bounds__(VIDEO_THREADS) rgb8_to_yuv8_wide_k(VideoArgs a, const uint8_t *__restrict__ rgb) {
    constexpr int ROWS = C420 ? 2 : 1, NW = 4 * C;      // 16 pixels of C bytes = NW words
    const int64_t idx = (int64_t)blockIdx.x * VIDEO_THREADS + threadIdx.x;
    if (idx >= a.items) return;
    const int m = a.W / VIDEO_STRIP;
    const uint32_t id = (uint32_t)idx;      // items <= N H W <= 2^31 - 1
    const int s = (int)(id % (uint32_t)m);
    const uint32_t t = id / (uint32_t)m;
    const int hj = a.H / ROWS;
    const int j = (int)(t % (uint32_t)hj), n = (int)(t / (uint32_t)hj);
    const int64_t f = (int64_t)n * a.stride;
    int32_t sr[8] = {}, sg[8] = {}, sb[8] = {};
#pragma unroll
    for (int dy = 0; dy < ROWS; ++dy) {
        const int row = ROWS * j + dy;
        const uint4 *src = reinterpret_cast<const uint4 *>(rgb + (((int64_t)n * a.H + row) * a.W + VIDEO_STRIP * s) * C);
        uint32_t w[NW];
#pragma unroll
        for (int q = 0; q < C; ++q) {
            const uint4 x = src[q];
            w[4 * q] = x.x; w[4 * q + 1] = x.y; w[4 * q + 2] = x.z; w[4 * q + 3] = x.w;
        }
        uint32_t yw[4] = {}, uw[4] = {}, vw[4] = {};
#pragma unroll
        for (int p = 0; p < VIDEO_STRIP; ++p) {
            const int32_t r = (int32_t)word_byte(w, C * p), g = (int32_t)word_byte(w, C * p + 1), b = (int32_t)word_byte(w, C * p + 2);
            yw[p >> 2] |= enc_byte<16>(a.k, 0, r, g, b) << ((p & 3) * 8);
            if constexpr (C420) {
                sr[p >> 1] += r; sg[p >> 1] += g; sb[p >> 1] += b;
            } else {
                uw[p >> 2] |= enc_byte<16>(a.k, 1, r, g, b) << ((p & 3) * 8);
                vw[p >> 2] |= enc_byte<16>(a.k, 2, r, g, b) << ((p & 3) * 8);
            }
        }
        const int64_t o = f + (int64_t)row * a.W + VIDEO_STRIP * s;
        *reinterpret_cast<uint4 *>(a.y + o) = make_uint4(yw[0], yw[1], yw[2], yw[3]);
        if constexpr (!C420) {
            *reinterpret_cast<uint4 *>(a.u + o) = make_uint4(uw[0], uw[1], uw[2], uw[3]);
            *reinterpret_cast<uint4 *>(a.v + o) = make_uint4(vw[0], vw[1], vw[2], vw[3]);
        }
    }
    if constexpr (C420) {
        uint32_t uw[2] = {}, vw[2] = {};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uw[i >> 2] |= enc_byte<18>(a.k, 1, sr[i], sg[i], sb[i]) << ((i & 3) * 8);
            vw[i >> 2] |= enc_byte<18>(a.k, 2, sr[i], sg[i], sb[i]) << ((i & 3) * 8);
        }
        const int64_t o = f + (int64_t)j * a.cw + 8 * s;
        *reinterpret_cast<uint2 *>(a.u + o) = make_uint2(uw[0], uw[1]);
        *reinterpret_cast<uint2 *>(a.v + o) = make_uint2(vw[0], vw[1]);
    }
}

// ---- decode, byte path: a thread per pixel -----------------------------------------------------------------------------------------------
template <bool C420, bool F32>
__global__ void __launch_bounds__(VIDEO_THREADS) yuv8_to_rgb_byte_k(VideoArgs a, void *__restrict__ out, int C) {
    const int64_t idx = (int64_t)blockIdx.x * VIDEO_THREADS + threadIdx.x;
    if (idx >= a.items) return;
    const uint32_t id = (uint32_t)idx;      // items = N H W <= 2^31 - 1
    const int x = (int)(id % (uint32_t)a.W);
    const uint32_t t = id / (uint32_t)a.W;
    const int r = (int)(t % (uint32_t)a.H), n = (int)(t / (uint32_t)a.H);
    const int64_t f = (int64_t)n * a.stride;
    const int32_t Y = a.y[f + (int64_t)r * a.W + x];
    int32_t U16, V16;
    if constexpr (!C420) {
        const int64_t o = f + (int64_t)r * a.W + x;
        U16 = 16 * (int32_t)a.u[o];
        V16 = 16 * (int32_t)a.v[o];
    } else {
        const int ja = r >> 1, ia = x >> 1;
        int jb = ja + (r & 1) * 2 - 1, ib = ia + (x & 1) * 2 - 1;
        jb = jb < 0 ? 0 : (jb > a.ch - 1 ? a.ch - 1 : jb);
        ib = ib < 0 ? 0 : (ib > a.cw - 1 ? a.cw - 1 : ib);
        const int32_t w0 = (x & 1) ? a.wo0 : a.we0, w1 = (x & 1) ? a.wo1 : a.we1;
        const int64_t ra = f + (int64_t)ja * a.cw, rb = f + (int64_t)jb * a.cw;
        U16 = w0 * (3 * (int32_t)a.u[ra + ia] + (int32_t)a.u[rb + ia]) + w1 * (3 * (int32_t)a.u[ra + ib] + (int32_t)a.u[rb + ib]);
        V16 = w0 * (3 * (int32_t)a.v[ra + ia] + (int32_t)a.v[rb + ia]) + w1 * (3 * (int32_t)a.v[ra + ib] + (int32_t)a.v[rb + ib]);
    }
    if constexpr (F32) {
        float *o = static_cast<float *>(out);
        const int64_t plane = (int64_t)a.H * a.W, at = (int64_t)n * 3 * plane + (int64_t)r * a.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[at + c * plane] = unit_of(dec_byte(a.k, c, Y, U16, V16));
    } else {
        uint8_t *o = static_cast<uint8_t *>(out) + idx * C;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)dec_byte(a.k, c, Y, U16, V16);
        if (C == 4) o[3] = 255;
    }
}

// ---- decode, wide path: a thread per strip of 16 luma pixels x ROWS rows -------------------------------------------------------------------
// C: 3 / 4 the uint8 sink's channels, 0 the float sink
template <int C, bool C420>
__global__ void __launch_bounds__(VIDEO_THREADS) yuv8_to_rgb_wide_k(VideoArgs a, void *__restrict__ out) {
    constexpr int ROWS = C420 ? 2 : 1;
    const int64_t idx = (int64_t)blockIdx.x * VIDEO_THREADS + threadIdx.x;
    if (idx >= a.items) return;
    const int m = a.W / VIDEO_STRIP;
    const uint32_t id = (uint32_t)idx;      // items <= N H W <= 2^31 - 1
    const int s = (int)(id % (uint32_t)m);
    const uint32_t t = id / (uint32_t)m;
    const int hj = a.H / ROWS;
    const int j = (int)(t % (uint32_t)hj), n = (int)(t / (uint32_t)hj);
    const int64_t f = (int64_t)n * a.stride;

    // 4:2:0: the three chroma rows this row pair blends, columns 8 s - 1 .. 8 s + 8 (clamped) at slots 0 .. 9
    int32_t cu[3][10], cv[3][10];
    if constexpr (C420) {
        const int il = 8 * s - 1 < 0 ? 0 : 8 * s - 1, ir = 8 * s + 8 > a.cw - 1 ? a.cw - 1 : 8 * s + 8;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            int jj = j + q - 1;
            jj = jj < 0 ? 0 : (jj > a.ch - 1 ? a.ch - 1 : jj);
            const int64_t ro = f + (int64_t)jj * a.cw;
            const uint2 pu = *reinterpret_cast<const uint2 *>(a.u + ro + 8 * s), pv = *reinterpret_cast<const uint2 *>(a.v + ro + 8 * s);
            const uint32_t wu[2] = {pu.x, pu.y}, wv[2] = {pv.x, pv.y};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                cu[q][i + 1] = (int32_t)word_byte(wu, i);
                cv[q][i + 1] = (int32_t)word_byte(wv, i);
            }
            cu[q][0] = a.u[ro + il]; cu[q][9] = a.u[ro + ir];
            cv[q][0] = a.v[ro + il]; cv[q][9] = a.v[ro + ir];
        }
    }
#pragma unroll
    for (int dy = 0; dy < ROWS; ++dy) {
        const int row = ROWS * j + dy;
        const int64_t o = f + (int64_t)row * a.W + VIDEO_STRIP * s;
        const uint4 py = *reinterpret_cast<const uint4 *>(a.y + o);
        const uint32_t wy[4] = {py.x, py.y, py.z, py.w};
        uint32_t wu[4] = {}, wv[4] = {};
        int32_t vu[10], vv[10];      // 4:2:0: the vertical blend x 4 at the ten columns
        if constexpr (C420) {
            const int nb = dy == 0 ? 0 : 2;      // even luma row: the chroma row above; odd: the one below
#pragma unroll
            for (int i = 0; i < 10; ++i) {
                vu[i] = 3 * cu[1][i] + cu[nb][i];
                vv[i] = 3 * cv[1][i] + cv[nb][i];
            }
        } else {
            const uint4 pu = *reinterpret_cast<const uint4 *>(a.u + o), pv = *reinterpret_cast<const uint4 *>(a.v + o);
            wu[0] = pu.x; wu[1] = pu.y; wu[2] = pu.z; wu[3] = pu.w;
            wv[0] = pv.x; wv[1] = pv.y; wv[2] = pv.z; wv[3] = pv.w;
        }
        uint32_t ow[C == 0 ? 1 : 4 * C] = {};
        float of[C == 0 ? 3 : 1][C == 0 ? VIDEO_STRIP : 1];
#pragma unroll
        for (int p = 0; p < VIDEO_STRIP; ++p) {
            const int32_t Y = (int32_t)word_byte(wy, p);
            int32_t U16, V16;
            if constexpr (C420) {
                const int i = (p >> 1) + 1, nbr = (p & 1) ? i + 1 : i - 1;
                const int32_t w0 = (p & 1) ? a.wo0 : a.we0, w1 = (p & 1) ? a.wo1 : a.we1;
                U16 = w0 * vu[i] + w1 * vu[nbr];
                V16 = w0 * vv[i] + w1 * vv[nbr];
            } else {
                U16 = 16 * (int32_t)word_byte(wu, p);
                V16 = 16 * (int32_t)word_byte(wv, p);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t b = dec_byte(a.k, c, Y, U16, V16);
                if constexpr (C == 0) of[c][p] = unit_of(b);
                else ow[(C * p + c) >> 2] |= b << (((C * p + c) & 3) * 8);
            }
            if constexpr (C == 4) ow[p] |= 255u << 24;
        }
        if constexpr (C == 0) {
            float *dst = static_cast<float *>(out);
            const int64_t plane = (int64_t)a.H * a.W, at = (int64_t)n * 3 * plane + (int64_t)row * a.W + VIDEO_STRIP * s;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<float4 *>(dst + at + c * plane + 4 * q) = make_float4(of[c][4 * q], of[c][4 * q + 1], of[c][4 * q + 2], of[c][4 * q + 3]);
            }
        } else {
            uint4 *dst = reinterpret_cast<uint4 *>(static_cast<uint8_t *>(out) + (((int64_t)n * a.H + row) * a.W + VIDEO_STRIP * s) * C);
#pragma unroll
            for (int q = 0; q < C; ++q) dst[q] = make_uint4(ow[4 * q], ow[4 * q + 1], ow[4 * q + 2], ow[4 * q + 3]);
        }
    }
}

VideoArgs video_args(const vl3d_video_desc *d, const VideoChoice &c) {
    VideoArgs a;
    a.N = d->N; a.H = d->H; a.W = d->W; a.ch = c.ch; a.cw = c.cw;
    a.stride = d->frame_stride;
    a.y = d->y; a.u = d->u; a.v = d->v;
    a.items = c.items;
    a.k = VIDEO_COEFS[d->matrix][d->full_range];
    const bool left = d->siting_x == VL3D_SITING_LEFT;
    a.we0 = left ? 4 : 3; a.we1 = left ? 0 : 1;
    a.wo0 = left ? 2 : 3; a.wo1 = left ? 2 : 1;
    return a;
}

}  // namespace

extern "C" int vl3d_video_coefs(int32_t matrix, int32_t full_range, int32_t *enc, int32_t *dec) {
    VL3D_REQUIRE(enc != nullptr && dec != nullptr, "vl3d_video_coefs: null output");
    VL3D_REQUIRE((matrix == VL3D_MATRIX_BT601 || matrix == VL3D_MATRIX_BT709) && (full_range == 0 || full_range == 1),
                 "vl3d_video_coefs: matrix is VL3D_MATRIX_BT601 or VL3D_MATRIX_BT709, full_range 0 or 1");
    const VideoCoefs &k = VIDEO_COEFS[matrix][full_range];
    for (int i = 0; i < 9; ++i) { enc[i] = k.enc[i]; dec[i] = k.dec[i]; }
    for (int i = 0; i < 3; ++i) enc[9 + i] = k.off[i];
    dec[9] = k.y0;
    return VL3D_OK;
}

extern "C" int vl3d_video_choice(const vl3d_video_desc *desc, const void *rgb, int32_t decode, vl3d_video_path *out) {
    VL3D_REQUIRE(out != nullptr, "vl3d_video_choice: null out");
    *out = vl3d_video_path{0, 0, 0, 0, 0};
    const VideoChoice c = choose_video(desc, rgb, decode != 0);
    if (c.status != VL3D_OK) {
        vl3d_set_error(c.msg);
        return c.status;
    }
    *out = vl3d_video_path{c.wide, c.strip, c.rows, c.threads, c.blocks};
    return VL3D_OK;
}

extern "C" int vl3d_rgb8_to_yuv8(const vl3d_video_desc *desc, const uint8_t *rgb, vl3d_stream_t stream) {
    const VideoChoice c = choose_video(desc, rgb, false);
    if (c.status != VL3D_OK) {
        vl3d_set_error(c.msg);
        return c.status;
    }
    const VideoArgs a = video_args(desc, c);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)c.blocks), block(VIDEO_THREADS);
    const bool c420 = desc->chroma == VL3D_CHROMA_420;
    if (!c.wide) {
        if (c420) rgb8_to_yuv8_byte_k<true><<<grid, block, 0, st>>>(a, rgb, desc->channels);
        else rgb8_to_yuv8_byte_k<false><<<grid, block, 0, st>>>(a, rgb, desc->channels);
    } else if (desc->channels == 3) {
        if (c420) rgb8_to_yuv8_wide_k<3, true><<<grid, block, 0, st>>>(a, rgb);
        else rgb8_to_yuv8_wide_k<3, false><<<grid, block, 0, st>>>(a, rgb);
    } else {
        if (c420) rgb8_to_yuv8_wide_k<4, true><<<grid, block, 0, st>>>(a, rgb);
        else rgb8_to_yuv8_wide_k<4, false><<<grid, block, 0, st>>>(a, rgb);
    }
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_yuv8_to_rgb(const vl3d_video_desc *desc, void *rgb, vl3d_stream_t stream) {
    const VideoChoice c = choose_video(desc, rgb, true);
    if (c.status != VL3D_OK) {
        vl3d_set_error(c.msg);
        return c.status;
    }
    const VideoArgs a = video_args(desc, c);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)c.blocks), block(VIDEO_THREADS);
    const bool c420 = desc->chroma == VL3D_CHROMA_420, f32 = desc->sink == VL3D_SINK_F32;
    if (!c.wide) {
        if (c420 && f32) yuv8_to_rgb_byte_k<true, true><<<grid, block, 0, st>>>(a, rgb, 3);
        else if (c420) yuv8_to_rgb_byte_k<true, false><<<grid, block, 0, st>>>(a, rgb, desc->channels);
        else if (f32) yuv8_to_rgb_byte_k<false, true><<<grid, block, 0, st>>>(a, rgb, 3);
        else yuv8_to_rgb_byte_k<false, false><<<grid, block, 0, st>>>(a, rgb, desc->channels);
    } else if (f32) {
        if (c420) yuv8_to_rgb_wide_k<0, true><<<grid, block, 0, st>>>(a, rgb);
        else yuv8_to_rgb_wide_k<0, false><<<grid, block, 0, st>>>(a, rgb);
    } else if (desc->channels == 3) {
        if (c420) yuv8_to_rgb_wide_k<3, true><<<grid, block, 0, st>>>(a, rgb);
        else yuv8_to_rgb_wide_k<3, false><<<grid, block, 0, st>>>(a, rgb);
    } else {
        if (c420) yuv8_to_rgb_wide_k<4, true><<<grid, block, 0, st>>>(a, rgb);
        else yuv8_to_rgb_wide_k<4, false><<<grid, block, 0, st>>>(a, rgb);
    }
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
