// Looping loss for gfx950, part 3: the loss prologue of MPMeshVid.forward (render -> loop-padded, gained video, with its gram16 form for the
// search, vl3d_loss.hip) and the in-place scale of the fused loss's gradient.
#include "vl3d_loss_common.h"

// x *= *scale, skipped entirely (one scalar load per wave, no traffic) when the scale is exactly 1: the upstream gradient of a loss that is
// differentiated directly is 1, and the fused looping loss has its gradient buffer ready since the forward
__global__ __launch_bounds__(256) void scale_inplace_k(int64_t n4, float4 *__restrict__ x, const float *__restrict__ scale) {
    const float s = *scale;
    if (s == 1.0f) return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 v = x[i];
        v.x *= s; v.y *= s; v.z *= s; v.w *= s;
        x[i] = v;
    }
}

extern "C" int vl3d_scale_inplace(int64_t n, float *x, const float *scale, vl3d_stream_t stream) {
    VL3D_REQUIRE(n > 0 && (n & 3) == 0 && x && scale, "vl3d_scale_inplace: n must be a positive multiple of 4 (16-byte aligned buffer)");
    const int64_t n4 = n / 4;
    const unsigned blocks = (unsigned)(ceil_div64(n4, 256) < 8192 ? ceil_div64(n4, 256) : 8192);
    hipLaunchKernelGGL(scale_inplace_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n4, reinterpret_cast<float4 *>(x), scale);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

// ---------------------------------------------------------------------------------------------------
// The loss prologue of MPMeshVid.forward (MPV.py:484-507): NHWC render -> loop-padded, scale-invariant-gained video for the loss.
//   rgb_pad = cat(rgb, rgb[:pad]);  scale = (exp(mean(log((mean_f res + .01) / (mean_t rgb.detach() + .01)))) + 3) / 4;  x = rgb_pad * scale
// was cat + mul (two copies of the padded clip), two frame means, five scalar kernels, and in the backward mul, two slices, an add and the
// NCHW -> NHWC copy the render backward needs -- ~20 launches around kernels that take 0.1-0.2 ms at the training crop.  Here: one kernel
// for the log-ratio sum, one that writes x [3,T+pad,h,w] from rgb [T,h,w,3], one that folds the pad frames' gradient back into
// g_rgb [T,h,w,3] (the gain has no gradient: the reference detaches rgb in it).
// res (F,3,h,w) through strides in floats (r_sf frame, r_sc channel, r_sr row; unit column stride): a crop of the captured clip needs no copy
__global__ __launch_bounds__(256) void loop_gain_k(int T, int F, int64_t hw, int w, const float *__restrict__ rgb, const float *__restrict__ res,
                                                   int64_t r_sf, int64_t r_sc, int64_t r_sr, double *__restrict__ log_sum) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float v = 0.f;
    if (p < hw) {
        float r0 = 0.f, r1 = 0.f, r2 = 0.f, y0 = 0.f, y1 = 0.f, y2 = 0.f;
        const float *rp = rgb + p * 3;
#pragma unroll 4
        for (int t = 0; t < T; ++t, rp += hw * 3) { r0 += rp[0]; r1 += rp[1]; r2 += rp[2]; }
        const int64_t py = p / w, px = p - py * w;
        const float *yp = res + py * r_sr + px;
#pragma unroll 4
        for (int f = 0; f < F; ++f, yp += r_sf) { y0 += yp[0]; y1 += yp[r_sc]; y2 += yp[2 * r_sc]; }
        const float it = 1.0f / (float)T, jf = 1.0f / (float)F;
        v = __logf((y0 * jf + 0.01f) / (r0 * it + 0.01f)) + __logf((y1 * jf + 0.01f) / (r1 * it + 0.01f)) + __logf((y2 * jf + 0.01f) / (r2 * it + 0.01f));
    }
    __shared__ float red[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(log_sum, (double)((red[0] + red[1]) + (red[2] + red[3])));
}

__device__ __forceinline__ float loop_gain(const double *log_sum, int64_t hw) {
    if (!log_sum) return 1.0f;
    return (__expf((float)(*log_sum / (double)(3 * hw))) + 3.0f) * 0.25f;
}

__global__ __launch_bounds__(256) void loop_pad_fwd_k(int T, int pad, int64_t hw, const float *__restrict__ rgb, const double *__restrict__ log_sum,
                                                      float *__restrict__ x) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int t = blockIdx.y, ts = t < T ? t : t - T;
    if (p >= hw) return;
    const float g = loop_gain(log_sum, hw);
    const float *rp = rgb + ((int64_t)ts * hw + p) * 3;
    const int64_t frames = T + pad;
    x[((int64_t)0 * frames + t) * hw + p] = rp[0] * g;
    x[((int64_t)1 * frames + t) * hw + p] = rp[1] * g;
    x[((int64_t)2 * frames + t) * hw + p] = rp[2] * g;
}

// ... and the same with the NN kernel's gram16 form of x written beside the video: the render's NHWC output is read ONCE for the loss's
// two layouts (the separate video -> gram16 pass re-read x: 0.30 of the 1.66 ms of a 720p search).  A workgroup takes 64 pixels of a row
// through all T + pad frames in groups of 16: lanes over pixels read 768 contiguous bytes per frame, write x coalesced per channel, the
// tile goes through LDS, 16 lanes = the 16 frames of a pixel write 256 contiguous bytes of pieces.
__global__ __launch_bounds__(256) void loop_pad_fwd_gram_k(int T, int pad, int H, int W, const float *__restrict__ rgb, const double *__restrict__ log_sum,
                                                           float *__restrict__ x, uint4 *__restrict__ xg) {
    __shared__ float tile[3][16][65];
    const int row = blockIdx.y, x0 = blockIdx.x * 64, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int F = T + pad, G = (F + 15) >> 4;
    const int64_t hw = (int64_t)H * W;
    const float gain = loop_gain(log_sum, hw);
    const int px = min(x0 + lane, W - 1);
    const bool inx = x0 + lane < W;
    float pre[12];
    auto load = [&](int f0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int j = wave + 4 * k, c = j >> 4, f = f0 + (j & 15), ts = f < T ? f : f - T;
            pre[k] = f < F ? rgb[(((int64_t)ts * H + row) * W + px) * 3 + c] * gain : 0.5f;
        }
    };
    load(0);
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int j = wave + 4 * k, c = j >> 4, f = g * 16 + (j & 15);
            if (f < F && inx) x[((int64_t)c * F + f) * hw + (int64_t)row * W + px] = pre[k];
            tile[c][j & 15][lane] = pre[k] - 0.5f;
        }
        __syncthreads();
        if (g + 1 < G) load((g + 1) * 16);
        const int m = lane & 15, f = g * 16 + m;
        for (int p = wave * 4 + (lane >> 4); p < 64; p += 16)
            if (x0 + p < W && f < F)
                xg[((size_t)row * W + x0 + p) * F + f] = gram16_piece(tile[0][m][p], tile[1][m][p], tile[2][m][p], 1.0f);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void loop_pad_bwd_k(int T, int pad, int64_t hw, const float *__restrict__ gx, int64_t gx_sc, int64_t gx_st,
                                                      const double *__restrict__ log_sum, float *__restrict__ g_rgb) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int t = blockIdx.y;
    if (p >= hw) return;
    const float g = loop_gain(log_sum, hw);
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        v[c] = gx[c * gx_sc + t * gx_st + p];
        if (t < pad) v[c] += gx[c * gx_sc + (T + t) * gx_st + p];
    }
    float *o = g_rgb + ((int64_t)t * hw + p) * 3;
    o[0] = v[0] * g; o[1] = v[1] * g; o[2] = v[2] * g;
}

extern "C" int vl3d_loop_gain_strided(int32_t T, int32_t F, int32_t h, int32_t w, const float *rgb, const float *res, int64_t r_sf, int64_t r_sc,
                                      int64_t r_sr, double *log_sum, vl3d_stream_t stream) {
    VL3D_REQUIRE(T > 0 && F > 0 && h > 0 && w > 0 && rgb && res && log_sum, "vl3d_loop_gain: bad arguments");
    const int64_t hw = (int64_t)h * w;
    VL3D_HIP(hipMemsetAsync(log_sum, 0, sizeof(double), (hipStream_t)stream));
    hipLaunchKernelGGL(loop_gain_k, dim3((unsigned)ceil_div64(hw, 256)), dim3(256), 0, (hipStream_t)stream, T, F, hw, w, rgb, res, r_sf, r_sc, r_sr,
                       log_sum);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_loop_gain(int32_t T, int32_t F, int32_t h, int32_t w, const float *rgb, const float *res, double *log_sum,
                              vl3d_stream_t stream) {
    const int64_t hw = (int64_t)(h > 0 ? h : 0) * (w > 0 ? w : 0);
    return vl3d_loop_gain_strided(T, F, h, w, rgb, res, 3 * hw, hw, w, log_sum, stream);
}

extern "C" int vl3d_loop_pad_fwd(int32_t T, int32_t pad, int32_t h, int32_t w, const float *rgb, const double *log_sum, float *x,
                                 vl3d_stream_t stream) {
    VL3D_REQUIRE(T > 0 && pad >= 0 && pad <= T && T + pad <= 65535 && h > 0 && w > 0 && rgb && x, "vl3d_loop_pad_fwd: bad arguments");
    const int64_t hw = (int64_t)h * w;
    hipLaunchKernelGGL(loop_pad_fwd_k, dim3((unsigned)ceil_div64(hw, 256), (unsigned)(T + pad)), dim3(256), 0, (hipStream_t)stream, T, pad, hw, rgb,
                       log_sum, x);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_loop_pad_fwd_gram(int32_t T, int32_t pad, int32_t h, int32_t w, const float *rgb, const double *log_sum, float *x, float *x_gram,
                                      vl3d_stream_t stream) {
    VL3D_REQUIRE(T > 0 && pad >= 0 && pad <= T && T + pad <= 65535 && h > 0 && w > 0 && rgb && x && x_gram, "vl3d_loop_pad_fwd_gram: bad arguments");
    hipLaunchKernelGGL(loop_pad_fwd_gram_k, dim3((unsigned)((w + 63) / 64), (unsigned)h), dim3(256), 0, (hipStream_t)stream, T, pad, h, w, rgb, log_sum, x,
                       reinterpret_cast<uint4 *>(x_gram));
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_loop_pad_bwd(int32_t T, int32_t pad, int32_t h, int32_t w, const float *grad_x, int64_t gx_sc, int64_t gx_st,
                                 const double *log_sum, float *grad_rgb, vl3d_stream_t stream) {
    VL3D_REQUIRE(T > 0 && pad >= 0 && pad <= T && T <= 65535 && h > 0 && w > 0 && grad_x && grad_rgb, "vl3d_loop_pad_bwd: bad arguments");
    const int64_t hw = (int64_t)h * w;
    hipLaunchKernelGGL(loop_pad_bwd_k, dim3((unsigned)ceil_div64(hw, 256), (unsigned)T), dim3(256), 0, (hipStream_t)stream, T, pad, hw, grad_x, gx_sc,
                       gx_st, log_sum, grad_rgb);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
