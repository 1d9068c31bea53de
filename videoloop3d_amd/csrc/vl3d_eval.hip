// Per-view image statistics of the evaluation script (include/vl3d.h "Evaluation"; scripts/script_evaluate_ours.py:149-181 with
// evaluations/metrics.py:15-89 and skimage's structural_similarity / peak_signal_noise_ratio as the reference calls them).
//
// One pass over both uint8 clips.  A workgroup owns a TILE_H x TILE_W tile of the crop for every frame:
//   * per frame f < min(F, T): the tile and its 3-pixel halo (scipy.ndimage 'reflect' = half-sample symmetric border) of both clips go to
//     LDS as the integers w = (2u - 255) m (the reference's sample a = (2u/255 - 1) m is w / 255); per channel a horizontal then a vertical
//     7-tap pass gives the window sums of w, z, w^2, z^2, wz EXACTLY in int32; the SSIM of the pixel follows in fp64 from those sums with
//     the scale 255 * 49 cancelled; SSE and the minimum of w are exact integers;
//   * every frame of each clip (F != T allowed): sum u and sum u^2 per pixel and channel in registers (dyn = temporal std difference).
// Per-frame partials land in the caller's scratch as [workgroup][frame]; a second, small launch adds them over the workgroups in a fixed
// order (no float atomics: two calls give the same bits).
#include "vl3d_common.h"

namespace {

constexpr int TILE_W = 64, TILE_H = 8, HALO = 3, WIN = 7;
constexpr int LW = TILE_W + 2 * HALO, LH = TILE_H + 2 * HALO;      // 70 x 14 staged samples per channel and clip
constexpr int NT = 256;                                              // 4 waves; a thread owns column t % 64, rows 2 (t / 64) and +1
constexpr int MAX_FRAMES = 32768;                                    // 65025 * MAX_FRAMES < 2^31: sum u^2 stays an int32

// skimage: data_range = 2 (float images), K1 = 0.01, K2 = 0.03, win 7 (NP = 49, cov_norm = 49 / 48).  With every moment written over the
// integer window sums (ux = Sw / (49 * 255), ...), numerator and denominator of S are both scaled by (49 * 255)^2 (and the variance terms
// by 48 more): C1 -> C1 (49 * 255)^2, C2 -> 48 C2 (49 * 255)^2.
constexpr double KSCALE = 49.0 * 255.0;
constexpr double C1S = (0.01 * 2.0) * (0.01 * 2.0) * KSCALE * KSCALE;
constexpr double C2S48 = 48.0 * (0.03 * 2.0) * (0.03 * 2.0) * KSCALE * KSCALE;

// scipy.ndimage mode='reflect' (d c b a | a b c d | d c b a) for i in [-3, n + 2]; tile positions past the crop are clamped first (their
// outputs are never used, their loads must stay inside it)
__device__ __forceinline__ int reflect_idx(int i, int n) {
    i = i > n + HALO - 1 ? n + HALO - 1 : i;
    return i < 0 ? -i - 1 : (i >= n ? 2 * n - i - 1 : i);
}

__device__ __forceinline__ double ssim_of(int sw, int sz, int sww, int szz, int swz) {
    const long long w = sw, z = sz;
    const double a1 = (double)(2 * w * z) + C1S;
    const double b1 = (double)(w * w + z * z) + C1S;
    const double a2 = (double)(98 * (49 * (long long)swz - w * z)) + C2S48;
    const double b2 = (double)(49 * (49 * (long long)sww - w * w + 49 * (long long)szz - z * z)) + C2S48;
    return (a1 * a2) / (b1 * b2);
}

template <typename V>
__device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_down(v, off, 64));
    return v;
}

struct EvalArgs {
    const uint8_t *gt, *pred, *mask;
    int64_t gt_sf, gt_sr, pred_sf, pred_sr;      // byte strides (frame, row); pixel stride 3, channel stride 1
    int F, T, Fm, h, w;
    int64_t *part_sse;                           // [nblk][Fm]
    double *part_ssim;                           // [nblk][Fm]
    double *part_dyn;                            // [nblk]
    int32_t *part_min;                           // [nblk][Fm]
};

__global__ __launch_bounds__(NT) void eval_stats_k(EvalArgs a) {
    __shared__ short s_w[2][3][LH][LW];          // masked w of gt (0) / pred (1)
    __shared__ int s_h[5][LH][TILE_W];           // horizontal 7-sums of one channel: w, z, w^2, z^2, wz
    __shared__ uint8_t s_m[LH][LW];
    __shared__ double r_d[NT / 64];
    __shared__ long long r_l[NT / 64];
    __shared__ int r_i[NT / 64];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int bx0 = blockIdx.x * TILE_W, by0 = blockIdx.y * TILE_H;
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    const int h = a.h, w = a.w;

    for (int i = tid; i < LH * LW; i += NT) {
        const int r = i / LW, c = i - r * LW;
        s_m[r][c] = a.mask ? (a.mask[(int64_t)reflect_idx(by0 + r - HALO, h) * w + reflect_idx(bx0 + c - HALO, w)] != 0) : 1;
    }

    // own pixels: column cx, rows py[0..1]
    const int cx = bx0 + lane;
    int py[2];
    bool own[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        py[k] = by0 + 2 * wid + k;
        own[k] = cx < w && py[k] < h;
    }
    int g1[2][3] = {}, g2[2][3] = {}, p1[2][3] = {}, p2[2][3] = {};

    const int nf = a.F > a.T ? a.F : a.T;
    for (int f = 0; f < nf; ++f) {
        // dyn: raw 0..255 samples of the own pixels, every frame of each clip
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!own[k]) continue;
            const int64_t px = (int64_t)py[k], off = (int64_t)cx * 3;
            if (f < a.F) {
                const uint8_t *g = a.gt + f * a.gt_sf + px * a.gt_sr + off;
#pragma unroll
                for (int c = 0; c < 3; ++c) { const int u = g[c]; g1[k][c] += u; g2[k][c] += u * u; }
            }
            if (f < a.T) {
                const uint8_t *p = a.pred + f * a.pred_sf + px * a.pred_sr + off;
#pragma unroll
                for (int c = 0; c < 3; ++c) { const int u = p[c]; p1[k][c] += u; p2[k][c] += u * u; }
            }
        }
        if (f >= a.Fm) continue;      // uniform over the workgroup

        __syncthreads();              // s_m ready (first frame) / the previous frame's s_w and s_h consumed
        for (int i = tid; i < 2 * LH * LW * 3; i += NT) {
            const int v = i / (LH * LW * 3), rem = i - v * (LH * LW * 3);
            const int r = rem / (LW * 3), rem2 = rem - r * (LW * 3), c = rem2 / 3, ch = rem2 - c * 3;
            const int gy = reflect_idx(by0 + r - HALO, h), gx = reflect_idx(bx0 + c - HALO, w);
            const uint8_t *src = v == 0 ? a.gt + f * a.gt_sf + (int64_t)gy * a.gt_sr : a.pred + f * a.pred_sf + (int64_t)gy * a.pred_sr;
            const int u = src[(int64_t)gx * 3 + ch];
            s_w[v][ch][r][c] = (short)(s_m[r][c] ? 2 * u - 255 : 0);
        }
        __syncthreads();

        double ssim_acc = 0.0;
        long long sse = 0;
        int mn = 255;
        for (int ch = 0; ch < 3; ++ch) {
            for (int i = tid; i < LH * TILE_W; i += NT) {
                const int r = i / TILE_W, c = i - r * TILE_W;
                int sw = 0, sz = 0, sww = 0, szz = 0, swz = 0;
#pragma unroll
                for (int d = 0; d < WIN; ++d) {
                    const int x = s_w[0][ch][r][c + d], y = s_w[1][ch][r][c + d];
                    sw += x; sz += y; sww += x * x; szz += y * y; swz += x * y;
                }
                s_h[0][r][c] = sw; s_h[1][r][c] = sz; s_h[2][r][c] = sww; s_h[3][r][c] = szz; s_h[4][r][c] = swz;
            }
            __syncthreads();
            const int r0 = 2 * wid;
            int v[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                int s = 0;
#pragma unroll
                for (int d = 0; d < WIN; ++d) s += s_h[q][r0 + d][lane];
                v[q] = s;
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                if (k == 1) {
#pragma unroll
                    for (int q = 0; q < 5; ++q) v[q] += s_h[q][r0 + WIN][lane] - s_h[q][r0][lane];
                }
                if (!own[k]) continue;
                const int yl = r0 + k + HALO, xl = lane + HALO;
                if (s_m[yl][xl]) ssim_acc += ssim_of(v[0], v[1], v[2], v[3], v[4]);
                const int x = s_w[0][ch][yl][xl], y = s_w[1][ch][yl][xl];
                sse += (long long)((x - y) * (x - y));
                mn = min(mn, x);
            }
            __syncthreads();          // s_h is rewritten by the next channel
        }

        ssim_acc = wave_sum(ssim_acc);
        sse = wave_sum(sse);
        mn = wave_min(mn);
        if (lane == 0) { r_d[wid] = ssim_acc; r_l[wid] = sse; r_i[wid] = mn; }
        __syncthreads();
        if (tid == 0) {
            const int64_t o = (int64_t)blk * a.Fm + f;
            a.part_ssim[o] = (r_d[0] + r_d[1]) + (r_d[2] + r_d[3]);
            a.part_sse[o] = (r_l[0] + r_l[1]) + (r_l[2] + r_l[3]);
            a.part_min[o] = min(min(r_i[0], r_i[1]), min(r_i[2], r_i[3]));
        }
    }

    // population std per pixel and channel: sqrt(n sum u^2 - (sum u)^2) / n, the radicand an exact integer
    double dyn = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!own[k]) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long vg = (long long)a.F * g2[k][c] - (long long)g1[k][c] * g1[k][c];
            const long long vp = (long long)a.T * p2[k][c] - (long long)p1[k][c] * p1[k][c];
            const double d = sqrt((double)vg) / a.F - sqrt((double)vp) / a.T;
            dyn += d * d;
        }
    }
    dyn = wave_sum(dyn);
    __syncthreads();
    if (lane == 0) r_d[wid] = dyn;
    __syncthreads();
    if (tid == 0) a.part_dyn[blk] = (r_d[0] + r_d[1]) + (r_d[2] + r_d[3]);
}

// one thread per frame (and one for dyn): the workgroups' partials added in workgroup order
__global__ __launch_bounds__(256) void eval_finish_k(int nblk, int Fm, const int64_t *__restrict__ part_sse, const double *__restrict__ part_ssim,
                                                     const double *__restrict__ part_dyn, const int32_t *__restrict__ part_min, int64_t *__restrict__ sse,
                                                     double *__restrict__ ssim_sum, int32_t *__restrict__ gt_min, double *__restrict__ dyn_sum) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < Fm) {
        long long s = 0;
        double q = 0.0;
        int m = 255;
        for (int b = 0; b < nblk; ++b) {
            const int64_t o = (int64_t)b * Fm + i;
            s += part_sse[o];
            q += part_ssim[o];
            m = min(m, part_min[o]);
        }
        sse[i] = s;
        ssim_sum[i] = q;
        gt_min[i] = m;
    } else if (i == Fm) {
        double d = 0.0;
        for (int b = 0; b < nblk; ++b) d += part_dyn[b];
        *dyn_sum = d;
    }
}

int64_t grid_blocks(const vl3d_eval_desc *d, int *gx, int *gy) {
    *gx = (int)ceil_div64(d->w, TILE_W);
    *gy = (int)ceil_div64(d->h, TILE_H);
    return (int64_t)*gx * *gy;
}

int check_desc(const vl3d_eval_desc *d) {
    VL3D_REQUIRE(d != nullptr, "eval: null descriptor");
    VL3D_REQUIRE(d->F > 0 && d->T > 0 && d->F <= MAX_FRAMES && d->T <= MAX_FRAMES, "eval: frame counts must lie in 1 .. 32768");
    VL3D_REQUIRE(d->h >= WIN && d->w >= WIN, "eval: the crop must be at least 7 x 7 (skimage's win_size)");
    VL3D_REQUIRE(d->h <= 65535 * TILE_H && d->w <= (1 << 24), "eval: crop too large");
    VL3D_REQUIRE(d->row0 >= 0 && d->col0 >= 0, "eval: negative crop origin");
    VL3D_REQUIRE(d->gt_sr >= 3 * (int64_t)(d->col0 + d->w) && d->pred_sr >= 3 * (int64_t)(d->col0 + d->w),
                 "eval: row stride shorter than the crop's last column");
    VL3D_REQUIRE(d->gt_sf >= d->gt_sr * (int64_t)(d->row0 + d->h) && d->pred_sf >= d->pred_sr * (int64_t)(d->row0 + d->h),
                 "eval: frame stride shorter than the crop's last row");
    return VL3D_OK;
}

}  // namespace

extern "C" int64_t vl3d_eval_scratch_bytes(const vl3d_eval_desc *d) {
    if (check_desc(d) != VL3D_OK) return -1;
    int gx, gy;
    const int64_t nblk = grid_blocks(d, &gx, &gy), Fm = d->F < d->T ? d->F : d->T;
    return nblk * Fm * (8 + 8 + 4) + nblk * 8;
}

extern "C" int vl3d_eval_view(const vl3d_eval_desc *d, const uint8_t *gt, const uint8_t *pred, const uint8_t *mask, int64_t mask_ones,
                              int64_t *sse, double *ssim_sum, int32_t *gt_min, double *dyn_sum, void *scratch, vl3d_stream_t stream) {
    const int rc = check_desc(d);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(gt && pred && sse && ssim_sum && gt_min && dyn_sum && scratch, "eval: null pointer");
    VL3D_REQUIRE(mask == nullptr || (mask_ones > 0 && mask_ones <= (int64_t)d->h * d->w),
                 "eval: the mask must hold between 1 and h*w ones (an all-zero mask has no masked PSNR / SSIM)");
    int gx, gy;
    const int nblk = (int)grid_blocks(d, &gx, &gy);
    const int Fm = d->F < d->T ? d->F : d->T;
    EvalArgs a;
    a.gt = gt + (int64_t)d->row0 * d->gt_sr + (int64_t)d->col0 * 3;
    a.pred = pred + (int64_t)d->row0 * d->pred_sr + (int64_t)d->col0 * 3;
    a.mask = mask;
    a.gt_sf = d->gt_sf; a.gt_sr = d->gt_sr; a.pred_sf = d->pred_sf; a.pred_sr = d->pred_sr;
    a.F = d->F; a.T = d->T; a.Fm = Fm; a.h = d->h; a.w = d->w;
    char *s = (char *)scratch;
    a.part_sse = (int64_t *)s;
    a.part_ssim = (double *)(s + (int64_t)nblk * Fm * 8);
    a.part_dyn = (double *)(s + (int64_t)nblk * Fm * 16);
    a.part_min = (int32_t *)(s + (int64_t)nblk * Fm * 16 + (int64_t)nblk * 8);
    hipLaunchKernelGGL(eval_stats_k, dim3((unsigned)gx, (unsigned)gy), dim3(NT), 0, (hipStream_t)stream, a);
    VL3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(eval_finish_k, dim3((unsigned)ceil_div64(Fm + 1, 256)), dim3(256), 0, (hipStream_t)stream, nblk, Fm, a.part_sse,
                       a.part_ssim, a.part_dyn, a.part_min, sse, ssim_sum, gt_min, dyn_sum);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
