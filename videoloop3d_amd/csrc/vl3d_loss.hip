// Looping loss for gfx950, part 1: the per-location temporal patch nearest-neighbour search (K3).  The vote-fold of the matched patches (K4)
// and the robust loss (K5) are in vl3d_fold.hip, the loop prologue in vl3d_loop_prologue.hip; WHICH kernel a search runs is decided in
// vl3d_patchnn_choice.h (choose_patchnn: host only, testable without a GPU) -- the entry points here check, choose, switch and launch.
//
// Replaces (reference): utils_vid.py:60-69 (extract_3Dpatches / unfoldNd), :72-86 (efficient_compute_distances), :109-142 (column mins +
// argmin).
//
// Formulation (SURVEY §7 "Gram vs box-filter"): patches are never materialised.  For a spatial location
// b the frame-pair energy  E[i',j'] = sum_{c,kh,kw} (x[c,i',.] - y[c,j',.])^2  is accumulated once
// (3*ps^2 terms per pair), and the patch distance is its temporal diagonal sum
// dist[i,j] = sum_kt E[i*st+kt, j*st+kt] / (3*pt*ps^2): pt-fold fewer flops than the patch-level Gram and
// no |x|^2+|y|^2-2xy cancellation (never negative).
#include "vl3d_loss_common.h"
#include <utility>

using namespace vl3d_loss_detail;      // the patch grid, the instantiation tables (NN_THREADS, TI, TJ, NL4, NN6_KX, nn6_ky), the choice

namespace {

// ---------------------------------------------------------------------------------------------------
// K3 v2: the same frame-pair-energy formulation fed from a PIXEL-MAJOR copy of the videos.
// video_to_pixel_major_k rewrites [3][T][H][W] (strided) as [H][W][3][TP] (TP = T padded to 4, zero filled) so that
// everything a patch location needs -- all frames of its ps x ps x 3 pixels -- is ps contiguous runs of ps*3*TP floats:
// the staging becomes fully coalesced float4 traffic (v1 gathered 44-byte row segments per frame: 13.0 ms at 720p for
// the ref-view configuration, almost all of it in the staging loads).
__global__ __launch_bounds__(256) void video_to_pixel_major_k(const float *__restrict__ v, int64_t sc, int64_t st, int64_t sr,
                                                              int T, int TP, int H, int W, float *__restrict__ out) {
    __shared__ float tile[64][65];      // [channel-frame chunk][pixel] (+1 pad: conflict-free transposed reads)
    const int row = blockIdx.y, x0 = blockIdx.x * 64, tid = threadIdx.x;
    const int CF = 3 * TP;
    for (int cf0 = 0; cf0 < CF; cf0 += 64) {
        // read: lanes over pixels (coalesced along the row), 4 (c,f) pairs per pass
        for (int j = tid >> 6; j < 64; j += 4) {
            const int cf = cf0 + j, c = cf / TP, f = cf - c * TP, x = x0 + (tid & 63);
            float val = 0.f;
            if (cf < CF && f < T && x < W) val = v[c * sc + f * st + (int64_t)row * sr + x];
            tile[j][tid & 63] = val;
        }
        __syncthreads();
        // write: lanes over (c,f) (contiguous in the pixel-major layout)
        for (int p = tid >> 6; p < 64; p += 4) {
            const int cf = cf0 + (tid & 63), x = x0 + p;
            if (cf < CF && x < W) out[((size_t)row * W + x) * CF + cf] = tile[tid & 63][p];
        }
        __syncthreads();
    }
}

struct NN2Args {
    const float *xt, *yt;   // pixel-major [H][W][3][TxP] / [H][W][3][TyP]
    int32_t *nn;
    int W, ps, pt, stride, stridet, h_o, w_o, n1, n2;
    int TxP, TyP, K, KC;
    int PX, PY;             // v6: frames per pixel of the gram16 copies of x / y (exact)
    int Wy;                 // v6: pixels per row of the gram16 y (== W, or the full frame's width when y is a crop of a prepared clip)
    int Wx, FXm;            // v6: pixels per row / frames per pixel of the gram16 x IN MEMORY (== W / PX, or the untrimmed clip's when the loss prologue wrote it)
    int use_alpha;
    float alpha, dnorm;
    int ablate;   // measurement only: 1 skip epilogue, 2 skip compute, 4 skip staging loads
};

// LDS layout (floats): Xs[KC][TxP] | Ys[KC][TyP] | E[TxP][TyP] | colmin[n2]
__global__ __launch_bounds__(NN_THREADS) void patchnn2_k(NN2Args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Xs = smem;
    float *Ys = Xs + (size_t)a.KC * a.TxP;
    float *E = Ys + (size_t)a.KC * a.TyP;
    float *colmin = E + (size_t)a.TxP * a.TyP;
    const int b = blockIdx.x, by = b / a.w_o, bx = b % a.w_o;
    const int r0 = by * a.stride, c0 = bx * a.stride, tid = threadIdx.x;
    const int tiles_j = a.TyP / TJ, ntiles = (a.TxP / TI) * tiles_j;
    const int rowk = a.ps * 3;                      // k = (r*ps + q)*3 + c : one patch row = rowk consecutive k, contiguous in memory
    const int x4 = a.TxP / 4, y4 = a.TyP / 4;
    for (int i = tid; i < a.TxP * a.TyP; i += NN_THREADS) E[i] = 0.f;
    for (int k0 = 0; k0 < a.K; k0 += a.KC) {
        const int kc = min(a.KC, a.K - k0);
        __syncthreads();
        for (int i = tid; i < kc * x4; i += NN_THREADS) {
            const int kk = i / x4, f4 = i - kk * x4, k = k0 + kk, r = k / rowk, rem = k - r * rowk;
            const float4 *src = reinterpret_cast<const float4 *>(a.xt + (((size_t)(r0 + r) * a.W + c0) * 3 + rem) * a.TxP);
            reinterpret_cast<float4 *>(Xs + (size_t)kk * a.TxP)[f4] = src[f4];
        }
        for (int i = tid; i < kc * y4; i += NN_THREADS) {
            const int kk = i / y4, f4 = i - kk * y4, k = k0 + kk, r = k / rowk, rem = k - r * rowk;
            const float4 *src = reinterpret_cast<const float4 *>(a.yt + (((size_t)(r0 + r) * a.W + c0) * 3 + rem) * a.TyP);
            reinterpret_cast<float4 *>(Ys + (size_t)kk * a.TyP)[f4] = src[f4];
        }
        __syncthreads();
        for (int tile = tid; tile < ntiles; tile += NN_THREADS) {
            const int ti = (tile / tiles_j) * TI, tj = (tile % tiles_j) * TJ;
            float acc[TI][TJ];
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) acc[i][j] = 0.f;
            for (int kk = 0; kk < kc; ++kk) {
                const float4 xv = *reinterpret_cast<const float4 *>(Xs + kk * a.TxP + ti);
                const float4 yv = *reinterpret_cast<const float4 *>(Ys + kk * a.TyP + tj);
                const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, ya[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int j = 0; j < TJ; ++j) {
                        const float df = xa[i] - ya[j];
                        acc[i][j] += df * df;
                    }
            }
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) E[(ti + i) * a.TyP + tj + j] += acc[i][j];
        }
    }
    __syncthreads();
    // epilogue on all 256 threads: 4 lanes share one row (column) and scan a quarter each, then combine by shuffles.
    // dist = sum_kt E[.][.] / d (utils_vid.py:82-84); normaliser alpha + min_i dist (:133-134); first minimum wins (:141).
    const int sub = tid & 3;
    if (a.use_alpha) {
        for (int j = tid >> 2; j < a.n2; j += NN_THREADS / 4) {
            float m = INFINITY;
            for (int i = sub; i < a.n1; i += 4) {
                float sacc = 0.f;
                for (int kt = 0; kt < a.pt; ++kt) sacc += E[(i * a.stridet + kt) * a.TyP + j * a.stridet + kt];
                m = fminf(m, sacc / a.dnorm);
            }
            m = fminf(m, __shfl_xor(m, 1, 64));
            m = fminf(m, __shfl_xor(m, 2, 64));
            if (sub == 0) colmin[j] = a.alpha + m;
        }
        __syncthreads();
    }
    for (int i0 = 0; i0 < a.n1; i0 += NN_THREADS / 4) {      // uniform trip count: every lane takes part in the shuffles
        const int i = i0 + (tid >> 2);
        const int q = (a.n2 + 3) / 4, j0 = sub * q, j1 = min(a.n2, j0 + q);
        float best = INFINITY;
        int bj = j0;
        bool best_nan = false;
        if (i < a.n1) {
            for (int j = j0; j < j1; ++j) {
                float sacc = 0.f;
                for (int kt = 0; kt < a.pt; ++kt) sacc += E[(i * a.stridet + kt) * a.TyP + j * a.stridet + kt];
                float v = sacc / a.dnorm;
                if (a.use_alpha) v = v / colmin[j];           // utils_vid.py:140
                const bool vn = (v != v);                      // torch.argmin: first minimum, NaN counts as minimal
                if (!best_nan && (vn || v < best)) { best = v; bj = j; best_nan = vn; }
            }
        }
        // combine the 4 quarters in ascending-j order so that ties keep the lowest index
#pragma unroll
        for (int step = 1; step <= 2; step <<= 1) {
            const float ob = __shfl_xor(best, step, 64);
            const int oj = __shfl_xor(bj, step, 64);
            const int on = __shfl_xor((int)best_nan, step, 64);
            const bool other_lower = (sub & step) != 0;      // the partner holds the lower-j range
            bool take;
            if (best_nan || on) take = on && (!best_nan || other_lower);
            else take = (ob < best) || (ob == best && other_lower);
            if (take) { best = ob; bj = oj; best_nan = on != 0; }
        }
        if (i < a.n1 && sub == 0) a.nn[(size_t)b * a.n1 + i] = bj;
    }
}

// colmin + argmin over one location's frame-pair energies E [TxP][TyP] in LDS (utils_vid.py:133-141): with s(i, j) = sum_kt E(i + kt, j + kt),
// the reference's score is (s / d) / (alpha + min_i s / d); first minimum wins, NaN counts as minimal (torch.argmin).  Scaling by a
// positive constant commutes with min and argmin, so the column minimum is taken over the raw sums and each column gets ONE weight
// w_j = (1 / d) / (alpha + min_i s / d): a score is s * w_j -- three LDS reads, two adds and a multiply per frame pair instead of two
// fp32 divisions (which were most of the epilogue's instructions).  Without alpha the raw sums are compared.  The rounding differs
// from the reference's two divisions by an ulp, i.e. only between exact near-ties -- EXCEPT at the column minimum itself: there the
// reference's score is q / (alpha + q) with q = m / d bit-identical in numerator and denominator, which for the shipped ref-view
// alpha = 0 (configs/mpv_base.txt:52) is EXACTLY 1.0 in every column, the smallest score a row can have; a row that is the minimum of
// several columns (certain when n2 > n1) is decided by torch.argmin's first-minimum rule among exact ties.  s * w_j is 1 +- an ulp, so
// an entry equal to its column's minimum takes the tie score t_j = (m / d) / (alpha + m / d) formed with true divisions instead
// (1.0 at alpha = 0; NaN = minimal for m = 0, as 0 / 0 is in the reference).  colw: [3][n2p] = weights | minima | tie scores.
// Whole workgroup, 4 lanes per row / column.
// PREINIT: the caller has set colw[0..n2) to +inf (bit pattern) behind a barrier already
template <int NTHR, bool PREINIT = false>
__device__ __forceinline__ void nn_epilogue(const NN2Args &a, const float *E, float *colw, int n2p, size_t b, int tid, int sub) {
    float *colm = colw + n2p, *colt = colw + 2 * n2p;
    if (a.pt == 3 && a.stridet == 1) {
        // every shipped configuration: three-frame patches at temporal stride 1.  s(i, j..j+3) needs E(i, j..j+3), E(i+1, j+1..j+4) and
        // E(i+2, j+2..j+5): whole 16-byte LDS reads (the rows are 16-byte aligned, TyP is a multiple of 4), the upper halves carried
        // from one group of four columns to the next -- 3/4 of an LDS read per frame pair instead of 3, same additions in the same order.
        const int TyP = a.TyP;
        const float4 *E4 = reinterpret_cast<const float4 *>(E);
        if (a.use_alpha) {
            // column minima: a thread takes four adjacent columns of every nrg-th row; the row groups meet in an LDS integer min
            // (the sums are >= +0 or NaN: their bit patterns order like the values and NaN never wins, as with fminf)
            int *cmi = reinterpret_cast<int *>(colw);
            if (!PREINIT) {
                for (int j = tid; j < a.n2; j += NTHR) cmi[j] = 0x7f800000;
                __syncthreads();
            }
            const int ngrp = TyP / 4, nrg = NTHR / ngrp, jg = tid % ngrp, ig = tid / ngrp;
            if (ig < nrg) {
                float m0 = INFINITY, m1 = INFINITY, m2 = INFINITY, m3 = INFINITY;
                for (int i = ig; i < a.n1; i += nrg) {
                    const float4 *p = E4 + (i * TyP) / 4 + jg;
                    const float4 c0 = p[0], l1 = p[TyP / 4], h1 = p[TyP / 4 + 1], l2 = p[TyP / 2], h2 = p[TyP / 2 + 1];
                    m0 = fminf(m0, (c0.x + l1.y) + l2.z);
                    m1 = fminf(m1, (c0.y + l1.z) + l2.w);
                    m2 = fminf(m2, (c0.z + l1.w) + h2.x);
                    m3 = fminf(m3, (c0.w + h1.x) + h2.y);
                }
                const int j = jg * 4;
                if (j < a.n2) atomicMin(cmi + j, __float_as_int(m0));
                if (j + 1 < a.n2) atomicMin(cmi + j + 1, __float_as_int(m1));
                if (j + 2 < a.n2) atomicMin(cmi + j + 2, __float_as_int(m2));
                if (j + 3 < a.n2) atomicMin(cmi + j + 3, __float_as_int(m3));
            }
            __syncthreads();
            const float inv_d = 1.0f / a.dnorm;
            for (int j = tid; j < a.n2; j += NTHR) {
                const float m = colw[j], q = m / a.dnorm;
                colm[j] = m;
                colt[j] = q / (a.alpha + q);
                colw[j] = inv_d / (a.alpha + q);
            }
            __syncthreads();
        }
        const int q4 = ((a.n2 + 3) / 4 + 3) & ~3, j0 = sub * q4, j1 = min(a.n2, j0 + q4);     // quarters of whole column groups
        for (int i0 = 0; i0 < a.n1; i0 += NTHR / 4) {      // uniform trip count: every lane takes part in the shuffles
            const int i = i0 + (tid >> 2);
            float best = INFINITY;
            int bj = j0;
            bool best_nan = false;
            if (i < a.n1 && j0 < j1) {
                const float4 *p = E4 + (i * TyP + j0) / 4;
                float4 l1 = p[TyP / 4], l2 = p[TyP / 2];
                for (int jb = j0; jb < j1; jb += 4, ++p) {
                    const float4 c0 = p[0], h1 = p[TyP / 4 + 1], h2 = p[TyP / 2 + 1];
                    float sa[4] = {(c0.x + l1.y) + l2.z, (c0.y + l1.z) + l2.w, (c0.z + l1.w) + h2.x, (c0.w + h1.x) + h2.y};
                    if (a.use_alpha) {
                        const float4 w = *reinterpret_cast<const float4 *>(colw + jb), m = *reinterpret_cast<const float4 *>(colm + jb);
                        const float4 t = *reinterpret_cast<const float4 *>(colt + jb);
                        sa[0] = sa[0] == m.x ? t.x : sa[0] * w.x; sa[1] = sa[1] == m.y ? t.y : sa[1] * w.y;
                        sa[2] = sa[2] == m.z ? t.z : sa[2] * w.z; sa[3] = sa[3] == m.w ? t.w : sa[3] * w.w;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float v = sa[u];
                        const bool vn = (v != v);
                        if (jb + u < j1 && !best_nan && (vn || v < best)) { best = v; bj = jb + u; best_nan = vn; }
                    }
                    l1 = h1; l2 = h2;
                }
            }
            // combine the 4 quarters in ascending-j order so that ties keep the lowest index
#pragma unroll
            for (int step = 1; step <= 2; step <<= 1) {
                const float ob = __shfl_xor(best, step, 64);
                const int oj = __shfl_xor(bj, step, 64);
                const int on = __shfl_xor((int)best_nan, step, 64);
                const bool other_lower = (sub & step) != 0;      // the partner holds the lower-j range
                bool take;
                if (best_nan || on) take = on && (!best_nan || other_lower);
                else take = (ob < best) || (ob == best && other_lower);
                if (take) { best = ob; bj = oj; best_nan = on != 0; }
            }
            if (i < a.n1 && sub == 0) a.nn[b * a.n1 + i] = bj;
        }
        return;
    }
    if (a.use_alpha) {
        const float inv_d = 1.0f / a.dnorm;
        for (int j = tid >> 2; j < a.n2; j += NTHR / 4) {
            float m = INFINITY;
            const float *e0 = E + j * a.stridet;
            // four rows per batch: their LDS reads are in flight together (the workgroup is four waves: nothing else hides the latency)
            int i = sub;
            for (; i + 12 < a.n1; i += 16) {
                float sa[4] = {0.f, 0.f, 0.f, 0.f};
                for (int kt = 0; kt < a.pt; ++kt)
#pragma unroll
                    for (int u = 0; u < 4; ++u) sa[u] += e0[((i + 4 * u) * a.stridet + kt) * a.TyP + kt];
                m = fminf(fminf(m, fminf(sa[0], sa[1])), fminf(sa[2], sa[3]));
            }
            for (; i < a.n1; i += 4) {
                float sacc = 0.f;
                for (int kt = 0; kt < a.pt; ++kt) sacc += e0[(i * a.stridet + kt) * a.TyP + kt];
                m = fminf(m, sacc);
            }
            m = fminf(m, __shfl_xor(m, 1, 64));
            m = fminf(m, __shfl_xor(m, 2, 64));
            if (sub == 0) {
                const float q = m / a.dnorm;
                colm[j] = m;
                colt[j] = q / (a.alpha + q);
                colw[j] = inv_d / (a.alpha + q);
            }
        }
        __syncthreads();
    }
    for (int i0 = 0; i0 < a.n1; i0 += NTHR / 4) {      // uniform trip count: every lane takes part in the shuffles
        const int i = i0 + (tid >> 2);
        const int qn = (a.n2 + 3) / 4, j0 = sub * qn, j1 = min(a.n2, j0 + qn);
        float best = INFINITY;
        int bj = j0;
        bool best_nan = false;
        if (i < a.n1) {
            const float *e0 = E + (i * a.stridet) * a.TyP;
            int j = j0;
            for (; j + 3 < j1; j += 4) {                       // four columns per batch, compared in ascending order
                float sa[4] = {0.f, 0.f, 0.f, 0.f};
                for (int kt = 0; kt < a.pt; ++kt)
#pragma unroll
                    for (int u = 0; u < 4; ++u) sa[u] += e0[kt * a.TyP + (j + u) * a.stridet + kt];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float v = a.use_alpha ? (sa[u] == colm[j + u] ? colt[j + u] : sa[u] * colw[j + u]) : sa[u];
                    const bool vn = (v != v);
                    if (!best_nan && (vn || v < best)) { best = v; bj = j + u; best_nan = vn; }
                }
            }
            for (; j < j1; ++j) {
                float sacc = 0.f;
                for (int kt = 0; kt < a.pt; ++kt) sacc += e0[kt * a.TyP + j * a.stridet + kt];
                const float v = a.use_alpha ? (sacc == colm[j] ? colt[j] : sacc * colw[j]) : sacc;
                const bool vn = (v != v);
                if (!best_nan && (vn || v < best)) { best = v; bj = j; best_nan = vn; }
            }
        }
        // combine the 4 quarters in ascending-j order so that ties keep the lowest index
#pragma unroll
        for (int step = 1; step <= 2; step <<= 1) {
            const float ob = __shfl_xor(best, step, 64);
            const int oj = __shfl_xor(bj, step, 64);
            const int on = __shfl_xor((int)best_nan, step, 64);
            const bool other_lower = (sub & step) != 0;      // the partner holds the lower-j range
            bool take;
            if (best_nan || on) take = on && (!best_nan || other_lower);
            else take = (ob < best) || (ob == best && other_lower);
            if (take) { best = ob; bj = oj; best_nan = on != 0; }
        }
        if (i < a.n1 && sub == 0) a.nn[b * a.n1 + i] = bj;
    }
}

// ---------------------------------------------------------------------------------------------------
// K3 v4: NL = 4 neighbouring patch locations per workgroup, column-sum formulation.
// The 4 locations (by, bx0..bx0+3) share a ps x (ps + 3*stride) pixel region.  Per region row, the row (all columns,
// channels and frames: ONE contiguous run in the pixel-major layout) is staged once; for every region column q the
// frame-pair energy of that column  C = sum_c (x - y)^2  is formed once per thread tile and added to the accumulators of
// the (up to ceil(ps/stride)) locations whose window contains q.  Versus one location per workgroup (v2) this halves the
// VALU work (ps=11, stride=4: 23 columns instead of 44 per row), halves the staging traffic and amortises the per-workgroup
// fixed costs over 4 locations; E lives in registers for the whole K loop (no LDS read-modify-write per chunk).

// NTHR: 256 threads for the shipped clips (one 4x4 frame-pair tile per thread), 512 / 1024 for longer ones (cfg4 / cfg5)
template <bool RUNSUM, int NTHR = NN_THREADS>
__global__ __launch_bounds__(NTHR) void patchnn4_k(NN2Args a, int H_unused, int groups_x) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int RWc = a.ps + (NL4 - 1) * a.stride;               // region width in pixels
    float *Xs = smem;                                           // [RWc*3][TxP]
    float *Ys = Xs + (size_t)RWc * 3 * a.TxP;                   // [RWc*3][TyP]
    float *E = smem;                                            // [TxP][TyP], one location at a time in the epilogue: ALIASES the
                                                                // staging buffers (dead by then) -> 35 KiB instead of 51 KiB of LDS
                                                                // for the ref-view cfg = 4 workgroups per CU instead of 3
    float *colmin = E + (size_t)a.TxP * a.TyP;
    const int g = blockIdx.x, by = g / groups_x, bx0 = (g % groups_x) * NL4;
    const int r0 = by * a.stride, c0 = bx0 * a.stride, tid = threadIdx.x;
    const int cols = min(RWc, a.W - c0);                        // the last group of a row may be narrower
    const int nloc = min(NL4, a.w_o - bx0);
    const int tiles_j = a.TyP / TJ, ntiles = (a.TxP / TI) * tiles_j;
    const bool has_tile = tid < ntiles;
    // thread -> frame-pair tile: y tiles fastest.  (19 y tiles for the shipped 75-frame clips put slots 16..18 of a ds_read_b128 lane
    // group on the banks of slots 0..2 -- SQ_LDS_BANK_CONFLICT is 0.75-0.85 of the LDS-active cycles, profiles/r02_pmc_summary.txt --
    // but the conflict-free alternative, x tiles fastest (13 <= 16), measured 1-3 % SLOWER in process (profiles/ab_loss.py, variant
    // 0x80: ref 3.99 vs 3.96 ms, other 3.16 vs 3.07 ms): the LDS is not what this kernel waits for.  Kept selectable for A/B.)
    const int tiles_i = a.TxP / TI;
    const bool i_fast = VL3D_ABLATE(a.ablate, 8) && tiles_i <= 16 && tiles_j > 16;
    const int ti = has_tile ? (i_fast ? tid % tiles_i : tid / tiles_j) * TI : 0, tj = has_tile ? (i_fast ? tid / tiles_i : tid % tiles_j) * TJ : 0;
    float acc[NL4][TI * TJ];
#pragma unroll
    for (int l = 0; l < NL4; ++l)
#pragma unroll
        for (int e = 0; e < TI * TJ; ++e) acc[l][e] = 0.f;
    const int x4 = cols * 3 * a.TxP / 4, y4 = cols * 3 * a.TyP / 4;
    for (int r = 0; r < a.ps; ++r) {
        __syncthreads();
        const float4 *xsrc = reinterpret_cast<const float4 *>(a.xt + ((size_t)(r0 + r) * a.W + c0) * 3 * a.TxP);
        const float4 *ysrc = reinterpret_cast<const float4 *>(a.yt + ((size_t)(r0 + r) * a.W + c0) * 3 * a.TyP);
        for (int i = tid; i < x4; i += NTHR) reinterpret_cast<float4 *>(Xs)[i] = xsrc[i];
        for (int i = tid; i < y4; i += NTHR) reinterpret_cast<float4 *>(Ys)[i] = ysrc[i];
        __syncthreads();
        if (has_tile) {
            // running sum R of the column energies along the row; location l's share of this row is R(window end) - R(before
            // window start): 16 adds per column + two snapshots per location and row instead of 16 adds per (column, covering
            // location).  R restarts every row, so the difference loses at most ~log2(23 columns) bits of a 24-bit sum.
            float R[TI * TJ];
#pragma unroll
            for (int e = 0; e < TI * TJ; ++e) R[e] = 0.f;
            for (int q = 0; q < cols; ++q) {
                if constexpr (RUNSUM) {
#pragma unroll
                    for (int l = 0; l < NL4; ++l)
                        if (q == l * a.stride) {               // window of location l starts at this column (uniform)
#pragma unroll
                            for (int e = 0; e < TI * TJ; ++e) acc[l][e] -= R[e];
                        }
                } else {                                       // few covering locations per column: plain per-column energy
#pragma unroll
                    for (int e = 0; e < TI * TJ; ++e) R[e] = 0.f;
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float4 xv = *reinterpret_cast<const float4 *>(Xs + (q * 3 + c) * a.TxP + ti);
                    const float4 yv = *reinterpret_cast<const float4 *>(Ys + (q * 3 + c) * a.TyP + tj);
                    const float xa[4] = {xv.x, xv.y, xv.z, xv.w}, ya[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
                    for (int i = 0; i < TI; ++i)
#pragma unroll
                        for (int j = 0; j < TJ; ++j) {
                            const float df = xa[i] - ya[j];
                            R[i * TJ + j] = fmaf(df, df, R[i * TJ + j]);
                        }
                }
                if constexpr (RUNSUM) {
#pragma unroll
                    for (int l = 0; l < NL4; ++l)
                        if (q == l * a.stride + a.ps - 1) {    // ... and ends at this one
#pragma unroll
                            for (int e = 0; e < TI * TJ; ++e) acc[l][e] += R[e];
                        }
                } else {
#pragma unroll
                    for (int l = 0; l < NL4; ++l) {
                        const int ql = q - l * a.stride;       // column inside location l's window?
                        if (ql >= 0 && ql < a.ps) {
#pragma unroll
                            for (int e = 0; e < TI * TJ; ++e) acc[l][e] += R[e];
                        }
                    }
                }
            }
        }
    }
    // epilogue, one location at a time through the shared E buffer
    const int sub = tid & 3;
#pragma unroll
    for (int l = 0; l < NL4; ++l) {
        if (l >= nloc) break;                                    // uniform
        __syncthreads();
        if (has_tile) {
#pragma unroll
            for (int i = 0; i < TI; ++i)
#pragma unroll
                for (int j = 0; j < TJ; ++j) E[(ti + i) * a.TyP + tj + j] = fmaxf(acc[l][i * TJ + j], 0.0f);   // (a difference of running sums: >= -rounding)
        }
        __syncthreads();
        const size_t b = (size_t)by * a.w_o + bx0 + l;
        nn_epilogue<NTHR>(a, E, colmin, (a.n2 + 3) & ~3, b, tid, sub);
    }
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// floor(n / d) for 0 <= n < 2^16, 0 < d < 2^12 through the hardware reciprocal: (n + 1/2) / d is at least 1 / (2 d) away from any
// integer, far more than the reciprocal's relative error times the quotient
__device__ __forceinline__ int fdiv_small(int n, int d) { return (int)(((float)n + 0.5f) * __builtin_amdgcn_rcpf((float)d)); }

__device__ __forceinline__ void lds_dma16(const float4 *g, float *lds_wave_uniform) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                     (__attribute__((address_space(3))) void *)lds_wave_uniform, 16, 0, 0);
}

// ---------------------------------------------------------------------------------------------------
// K3 v6: the v4 workgroup (NL neighbouring locations, a shared ps x (ps + (NL - 1) stride) region, running sums along the region's columns,
// E through the shared epilogue) with the frame-pair energies on the HALF-PRECISION matrix cores at fp32-class accuracy and the region staged
// by LDS-DMA, one stage of CHC columns x all ps rows in flight behind the one being contracted.  (Rounds 2-4 ran this workgroup on
// v_mfma_f32_16x16x4_f32 -- `patchnn5_k`, the vector rate: 32 cycles per 16x16x4 issue, 2.0-2.1 ms at 720p; removed in round 5, its numbers are
// in DESIGN.)  v_mfma_f32_16x16x32_f16 contracts 32 k in 16-17 cycles (16x the rate, MI355X_MICROARCH.md).  The cross term of  e(ti, tj) = |u(ti)|^2 + |v(tj)|^2 - 2 u(ti).v(tj)  is formed from a two-term
// split of every value, u = hi + lo with hi = f16(u), lo = f16(u - hi) (11 + 11 mantissa bits; f16 subnormals are kept by the conversion
// and by the matrix cores, measured in profiles/microbench/dma_f16.hip), as  hi.hi' + hi.lo' + lo.hi'  accumulated in fp32 (the dropped
// lo.lo' is < 2^-24 of the product: an fp32 rounding).  The two norms are fp32 sums on the side.
// gram16 form (video_to_gram16_k): per pixel and frame ONE 16-byte piece  [h0 h1 | l0 l1 | h2 l2 | nh nl]  -- the split of the three
// channels (x: u = x - 1/2; y: -2 v, v = y - 1/2) and of the norm n = sum_c u_c^2 (y: sum_c v_c^2; 22 bits, below the rounding of the fp32 window
// sum it enters) -- pixel-major [H][W][T], so a region row is one contiguous run for the LDS-DMA (strided lanes cost 5x:
// dma_f16.hip) and any crop origin of a prepared clip is valid.
// One MFMA covers TWO cells (pixels) of a region column for a 16 x 16 frame-pair tile: its four 8-element k blocks (lane >> 4) are
//   kb 0: cell a, A = [h0 h1 h0 h1 h2 h2 0 0]   kb 1: cell a, A = [l0 l1 0 0 l2 0 0 0]   kb 2 / 3: the same for cell b
// against B = the RAW y piece [h0' h1' l0' l1' h2' l2' nh' nl'] in all four: kb 0 gives h.h' + h.l', kb 1 gives l.h', and the norm
// halves meet zeros.  The A blocks come out of the raw x piece in three instructions (a select, a mask, a byte permute with a per-lane
// selector): 9 of 16 k slots carry products, 5.5 issues of 17 cycles per 11-pixel column and tile instead of 11 of 32.
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

template <bool IS_Y>
__global__ __launch_bounds__(256) void video_to_gram16_k(const float *__restrict__ v, int64_t sc, int64_t st, int64_t sr,
                                                         int T, int H, int W, uint4 *__restrict__ out) {
    __shared__ float tile[3][16][65];      // [channel][frame of the group][pixel] (+1 pad: conflict-free transposed reads)
    const int row = blockIdx.y, x0 = blockIdx.x * 64, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = (T + 15) >> 4;
    float pre[12];
    const float *src = v + (int64_t)row * sr + min(x0 + lane, W - 1);
    auto load = [&](int f0) {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int j = wave + 4 * k, c = j >> 4, f = f0 + (j & 15);
            pre[k] = f < T ? src[c * sc + f * st] : 0.5f;
        }
    };
    load(0);
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int j = wave + 4 * k;
            tile[j >> 4][j & 15][lane] = pre[k] - 0.5f;
        }
        __syncthreads();
        if (g + 1 < G) load((g + 1) * 16);
        // write: 16 lanes = the 16 frames of one pixel = 256 contiguous bytes; 4 pixels per wave and pass
        const int m = lane & 15, f = g * 16 + m;
        for (int p = wave * 4 + (lane >> 4); p < 64; p += 16)
            if (x0 + p < W && f < T)
                out[((size_t)row * W + x0 + p) * T + f] = gram16_piece(tile[0][m][p], tile[1][m][p], tile[2][m][p], IS_Y ? -2.0f : 1.0f);
        __syncthreads();
    }
}

template <int J>
__device__ __forceinline__ void nn6_issue_tile(u32x4_t &dst, unsigned addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(J * 256) : "memory");
}
template <int N, int... Js>
__device__ __forceinline__ void nn6_issue_tiles(u32x4_t (&b)[N], unsigned addr, std::integer_sequence<int, Js...>) {
    (nn6_issue_tile<Js>(b[Js], addr), ...);
}

// One wave's rows of a location, no alpha, pt = 3, stridet = 1: s(i, j) = E(i, j) + E(i + 1, j + 1) + E(i + 2, j + 2) over the wave's slab
// E [16][EP]; first minimum over j; 4 lanes per row, each a quarter of whole column groups.  The slab holds fmaxf(., 0) of finite sums:
// no NaN can reach the comparison (a NaN accumulator is stored as 0), so it is a plain `<` -- a compare, an index select and a min per
// column instead of the NaN-aware form's seven instructions.  Returns the index (valid in the lanes with sub == 0).
__device__ __forceinline__ int nn_argmin_rows3(const float *E, int EP, int n2, int i, bool active, int sub) {
    const float4 *E4 = reinterpret_cast<const float4 *>(E);
    const int q4 = ((n2 + 3) / 4 + 3) & ~3, j0 = sub * q4, j1 = min(n2, j0 + q4);
    float best = INFINITY;
    int bj = j0;
    if (active && j0 < j1) {
        const float4 *p = E4 + (i * EP + j0) / 4;
        float4 l1 = p[EP / 4], l2 = p[EP / 2];
        int jb = j0;
        for (; jb + 3 < j1; jb += 4, ++p) {
            const float4 c0 = p[0], h1 = p[EP / 4 + 1], h2 = p[EP / 2 + 1];
            const float sa[4] = {(c0.x + l1.y) + l2.z, (c0.y + l1.z) + l2.w, (c0.z + l1.w) + h2.x, (c0.w + h1.x) + h2.y};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                bj = sa[u] < best ? jb + u : bj;
                best = fminf(best, sa[u]);
            }
            l1 = h1; l2 = h2;
        }
        if (jb < j1) {                                            // the quarter's last, partial group
            const float4 c0 = p[0], h1 = p[EP / 4 + 1], h2 = p[EP / 2 + 1];
            const float sa[4] = {(c0.x + l1.y) + l2.z, (c0.y + l1.z) + l2.w, (c0.z + l1.w) + h2.x, (c0.w + h1.x) + h2.y};
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (jb + u < j1) {
                    bj = sa[u] < best ? jb + u : bj;
                    best = fminf(best, sa[u]);
                }
        }
    }
#pragma unroll
    for (int step = 1; step <= 2; step <<= 1) {      // combine the 4 quarters in ascending-j order so that ties keep the lowest index
        const float ob = __shfl_xor(best, step, 64);
        const int oj = __shfl_xor(bj, step, 64);
        const bool other_lower = (sub & step) != 0;
        const bool take = (ob < best) || (ob == best && other_lower);
        if (take) { best = ob; bj = oj; }
    }
    return bj;
}

// NN2Args: PX / PY = frames per pixel of the gram16 x / y (exact, no padding); xt / yt = the gram16 buffers (16-byte pieces).
// One operand register set: a second one (the reads of chunk c + 1 in flight during the MFMAs of chunk c) takes 202 registers = two waves
// per SIMD and measured 1.76 / 1.93 ms against 1.54 / 1.47 ms with three (720p, ref / other cfg): the other waves hide the reads better.
// XS: first x frame of wave w is XS * w.  16: the waves' tiles abut, the epilogue runs workgroup-wide through the shared E.  14: the
// tiles overlap by pt - 1 = 2 frames, so wave w holds every frame pair of its 14 patches: each wave finishes its own rows through a
// private 16-row slab, no workgroup barrier between the locations (no alpha, pt = 3, stridet = 1 only: the column minima of the alpha
// path need all rows -- a two-phase per-wave form of it, minima through an LDS integer min behind one barrier and the slabs written twice,
// measured 1.46 against 1.41 ms at 720p and was not kept).
#ifdef VL3D_NN6_FLAT_NORMS
#define VL3D_NN6_NSTEP 0u
#else
#define VL3D_NN6_NSTEP nstep2
#endif
template <int TYT, int NL, int NW, int XS>
__global__ __launch_bounds__(64 * NW, TYT == 5 ? 3 : 2) void patchnn6_k(NN2Args a, int groups_x, int CHC) {
    constexpr int NTHR = 64 * NW, NXT = 16 * NW;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int KX = NN6_KX, KY = nn6_ky(TYT);                // DMA pieces per wave and stage at most (their source offsets live in registers)
    const int RWc = a.ps + (NL - 1) * a.stride;                 // region width in pixels
    const int FX = a.PX, FY = a.PY;
    const int xs4 = CHC * a.ps * FX, ys4 = CHC * a.ps * FY;       // 16-byte pieces per stage and part
    const int ybase = xs4 * 4, bufF = (xs4 + ys4) * 4;            // (floats)
    const int n2p = (a.n2 + 3) & ~3;
    const int EP = XS == 16 ? a.TyP : (((a.TyP + 3) & ~7) + 4);  // slab row pitch: 4 EP = 16 mod 32 banks (the two lane groups of a store never meet)
    float *E = smem;                                            // XS 16: [TxP][TyP], one location at a time; XS 14: NW slabs [17][EP]: aliases the staging
    float *colw = E + (XS == 16 ? (size_t)a.TxP * a.TyP : (size_t)NW * 17 * EP);
    float *sy = colw + NL * 3 * n2p;                            // [NL][TyP] y norms of the locations   (colw: [NL][3][n2p])
    float *sx = sy + NL * a.TyP;                                // [NL][NXT] x norms
    const int g = blockIdx.x, by = g / groups_x, bx0 = (g % groups_x) * NL;
    const int r0 = by * a.stride, c0 = bx0 * a.stride, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cols = min(RWc, a.W - c0);
    const int nloc = min(NL, a.w_o - bx0);
    f32x4_t acc[NL][TYT], R[TYT];
#pragma unroll
    for (int l = 0; l < NL; ++l)
#pragma unroll
        for (int j = 0; j < TYT; ++j) acc[l][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < TYT; ++j) R[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // norms on the side: thread tid < FX sums frame tid of x, thread NXT + f frame f of y (one LDS word + one dot2 per cell, in the MFMAs' shadow)
    const bool xside = tid < FX, yside = tid >= NXT && tid - NXT < FY;
    float an[NL], Rn = 0.f;
#pragma unroll
    for (int l = 0; l < NL; ++l) an[l] = 0.f;
    int offx[KX], offy[KY];
#pragma unroll
    for (int k = 0; k < KX; ++k) {
        const int idx = (wave + NW * k) * 64 + lane, cc = fdiv_small(idx, a.ps * FX), rem = idx - cc * a.ps * FX, r = fdiv_small(rem, FX);
        offx[k] = idx < xs4 ? ((r * a.Wx + cc) * a.FXm + (rem - r * FX)) | (cc << 24) : -1;
    }
#pragma unroll
    for (int k = 0; k < KY; ++k) {
        const int idx = (wave + NW * k) * 64 + lane, cc = fdiv_small(idx, a.ps * FY), rem = idx - cc * a.ps * FY, r = fdiv_small(rem, FY);
        offy[k] = idx < ys4 ? ((r * a.Wy + cc) * FY + (rem - r * FY)) | (cc << 24) : -1;
    }
    const int S = (cols + CHC - 1) / CHC;                       // stages
    auto issue = [&](int st) {
        const int q0 = st * CHC, nc = min(CHC, cols - q0);
        float *dst = smem + (st & 1) * bufF;
        const float4 *xsrc = reinterpret_cast<const float4 *>(a.xt) + ((size_t)r0 * a.Wx + c0 + q0) * a.FXm;
        const float4 *ysrc = reinterpret_cast<const float4 *>(a.yt) + ((size_t)r0 * a.Wy + c0 + q0) * FY;
#pragma unroll
        for (int k = 0; k < KX; ++k)
            if (offx[k] >= 0 && (offx[k] >> 24) < nc) lds_dma16(xsrc + (offx[k] & 0xffffff), dst + (wave + NW * k) * 256);
#pragma unroll
        for (int k = 0; k < KY; ++k)
            if (offy[k] >= 0 && (offy[k] >> 24) < nc) lds_dma16(ysrc + (offy[k] & 0xffffff), dst + ybase + (wave + NW * k) * 256);
    };
    // operand fragments: lane = frame (lane & 15) + 16 * k block; k blocks 0 / 1 read cell a of the chunk, 2 / 3 cell b -- 16 lanes x 16 bytes
    // of one pixel's frames are 256 contiguous bytes: conflict-free ds_read_b128
    const int kb = lane >> 4;
    const bool lo_blk = (kb & 1) != 0;
    const unsigned ymask = lo_blk ? 0u : 0xffffffffu;           // A.y = (h0 h1) in the h block, 0 in the l block
    const unsigned zsel = lo_blk ? 0x0c0c0302u : 0x01000100u;   // A.z = (h2 h2) / (l2 0) out of the piece's (h2 l2)
    const unsigned cellx = (unsigned)FX * 16u, celly = (unsigned)FY * 16u;
    const int nch = (a.ps + 1) >> 1;
    const bool odd = (a.ps & 1) != 0;
    // per-lane byte steps from chunk to chunk; into the LAST chunk of an odd column the lanes of cell b step one cell only (they re-read the
    // column's last cell, their A block is zeroed)
    const unsigned xstep2 = 2u * cellx, ystep2 = 2u * celly;
    const unsigned xstepL = (odd && kb >= 2) ? cellx : xstep2, ystepL = (odd && kb >= 2) ? celly : ystep2;
    const unsigned nstep2 = xside ? xstep2 : (yside ? ystep2 : 0u);
    const f16x2_t ones = {(_Float16)1.0f, (_Float16)1.0f};
    if (!VL3D_ABLATE(a.ablate, 4)) issue(0);
    for (int st = 0; st < S; ++st) {
        __syncthreads();                                         // stage st has landed; everyone is done with the other buffer
        if (st + 1 < S && !VL3D_ABLATE(a.ablate, 4)) issue(st + 1);
        if VL3D_ABLATE(a.ablate, 2) continue;
        const int q0 = st * CHC, nc = min(CHC, cols - q0);
        const float *buf = smem + (st & 1) * bufF;
        for (int cc = 0; cc < nc; ++cc) {
            const int q = q0 + cc;
#pragma unroll
            for (int l = 0; l < NL; ++l)
                if (q == l * a.stride) {      // window of location l starts at this column (uniform): acc = R(end) - R(before start)
#pragma unroll
                    for (int j = 0; j < TYT; ++j) acc[l][j] -= R[j];
                    an[l] -= Rn;
                }
            const bool one_cell = a.ps == 1;
            unsigned xad = (unsigned)reinterpret_cast<uintptr_t>(buf) + (unsigned)(cc * a.ps * FX + XS * wave + (lane & 15)) * 16u + ((kb >= 2 && !one_cell) ? cellx : 0u);
            unsigned yad = (unsigned)reinterpret_cast<uintptr_t>(buf + ybase) + (unsigned)(cc * a.ps * FY + (lane & 15)) * 16u + ((kb >= 2 && !one_cell) ? celly : 0u);
            unsigned nad0 = xside ? (unsigned)reinterpret_cast<uintptr_t>(buf) + (unsigned)(cc * a.ps * FX + tid) * 16u + 12u
                                  : (yside ? (unsigned)reinterpret_cast<uintptr_t>(buf + ybase) + (unsigned)(cc * a.ps * FY + tid - NXT) * 16u + 12u
                                           : (unsigned)reinterpret_cast<uintptr_t>(buf));
#ifdef VL3D_NN6_FLAT_NORMS      // measurement build only (WRONG norms): every lane reads one and the same word -- prices the bank conflicts of the side threads' reads
            nad0 = (unsigned)reinterpret_cast<uintptr_t>(buf);
#endif
            unsigned nad1 = nad0 + (VL3D_NN6_NSTEP >> 1);
            // The reads and their wait are asm statements fenced by scheduling barriers, or hipcc folds them back next to their use.
            {
                u32x4_t a0, b0[TYT];
                unsigned n00, n01;
                constexpr auto tiles = std::make_integer_sequence<int, TYT>{};
#define VL3D_NN6_ISSUE(A, N0, N1, B)                                                                      \
    asm volatile("ds_read_b128 %0, %3\n\tds_read_b32 %1, %4\n\tds_read_b32 %2, %5"                        \
                 : "=&v"(A), "=&v"(N0), "=&v"(N1) : "v"(xad), "v"(nad0), "v"(nad1) : "memory");           \
    nn6_issue_tiles(B, yad, tiles);                                                                       \
    __builtin_amdgcn_sched_barrier(0)
#define VL3D_NN6_WAIT(A, N0, N1, B)                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                    \
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(A), "+v"(N0), "+v"(N1)::"memory");                         \
    _Pragma("unroll") for (int j = 0; j < TYT; ++j) asm volatile("" : "+v"(B[j])::"memory")
#define VL3D_NN6_NEXT(C)      /* addresses of chunk C + 1 */                                             \
    {                                                                                                     \
        const bool last_ = (C) + 2 >= nch;                                                                \
        xad += last_ ? xstepL : xstep2; yad += last_ ? ystepL : ystep2;                                   \
        nad0 += VL3D_NN6_NSTEP; nad1 += VL3D_NN6_NSTEP;                                                   \
    }
#define VL3D_NN6_MMA(C, A, N0, N1, B)                                                                     \
    {                                                                                                     \
        u32x4_t s_;                                                                                       \
        s_.x = lo_blk ? A.y : A.x;                                                                        \
        s_.y = A.x & ymask;                                                                               \
        s_.z = __builtin_amdgcn_perm(A.z, A.z, zsel);                                                     \
        s_.w = 0u;                                                                                        \
        const bool odd_ = 2 * (C) + 1 >= a.ps;            /* (uniform) the chunk's second cell does not exist */ \
        if (odd_ && kb >= 2) { s_.x = 0u; s_.y = 0u; s_.z = 0u; }                                         \
        const f16x8_t af_ = __builtin_bit_cast(f16x8_t, s_);                                              \
        _Pragma("unroll") for (int j = 0; j < TYT; ++j)                                                   \
            R[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af_, __builtin_bit_cast(f16x8_t, B[j]), R[j], 0, 0, 0); \
        Rn = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, N0), ones, Rn, false);                    \
        if (!odd_) Rn = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2_t, N1), ones, Rn, false);         \
    }
                for (int c = 0; c < nch; ++c) {
                    VL3D_NN6_ISSUE(a0, n00, n01, b0);
                    VL3D_NN6_WAIT(a0, n00, n01, b0);
                    VL3D_NN6_MMA(c, a0, n00, n01, b0);
                    VL3D_NN6_NEXT(c);
                }
#undef VL3D_NN6_ISSUE
#undef VL3D_NN6_WAIT
#undef VL3D_NN6_NEXT
#undef VL3D_NN6_MMA
            }
#pragma unroll
            for (int l = 0; l < NL; ++l)
                if (q == l * a.stride + a.ps - 1) {   // ... and ends at this one
#pragma unroll
                    for (int j = 0; j < TYT; ++j) acc[l][j] += R[j];
                    an[l] += Rn;
                }
        }
    }
    // epilogue.  C/D layout of a 16x16 tile: col = lane & 15, row = (lane >> 4) * 4 + reg
    const int sub = tid & 3;
    __syncthreads();                                             // the staging buffers are dead from here on
    if (xside) {
#pragma unroll
        for (int l = 0; l < NL; ++l) sx[l * NXT + tid] = an[l];
    } else if (tid < NXT) {
#pragma unroll
        for (int l = 0; l < NL; ++l) sx[l * NXT + tid] = 0.f;
    }
    if (tid >= NXT && tid - NXT < a.TyP) {
#pragma unroll
        for (int l = 0; l < NL; ++l) sy[l * a.TyP + tid - NXT] = yside ? an[l] : 0.f;
    }
    if constexpr (XS == 16) {
        // one location at a time through the shared E buffer, the whole workgroup on it
        for (int j = tid; j < NL * n2p; j += NTHR) reinterpret_cast<int *>(colw)[(j / n2p) * 3 * n2p + j % n2p] = 0x7f800000;     // column minima start at +inf
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= nloc) break;                                    // uniform
            __syncthreads();                                         // sx / sy written / the previous location's E read
            float syv[TYT];
#pragma unroll
            for (int j = 0; j < TYT; ++j) syv[j] = sy[l * a.TyP + min(j * 16 + (lane & 15), a.TyP - 1)];
            const float4 sxv = *reinterpret_cast<const float4 *>(sx + l * NXT + wave * 16 + (lane >> 4) * 4);
            const float sxa[4] = {sxv.x, sxv.y, sxv.z, sxv.w};
#pragma unroll
            for (int j = 0; j < TYT; ++j)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int row = wave * 16 + (lane >> 4) * 4 + rr, col = j * 16 + (lane & 15);
                    if (row < a.TxP && col < a.TyP) E[row * a.TyP + col] = fmaxf(acc[l][j][rr] + (sxa[rr] + syv[j]), 0.0f);
                }
            __syncthreads();
            const size_t b = (size_t)by * a.w_o + bx0 + l;
            if VL3D_ABLATE(a.ablate, 1) { if (tid < a.n1) a.nn[b * a.n1 + tid] = 0; continue; }
            nn_epilogue<NTHR, true>(a, E, colw + l * 3 * n2p, n2p, b, tid, sub);
        }
    } else {
        // every wave finishes the 14 patches whose frames it holds, through its own slab: no workgroup barrier between the locations
        __syncthreads();                                         // sx / sy written
        float *Ew = E + wave * 17 * EP;
        const int i0 = XS * wave, nrow = min(XS, a.n1 - i0);      // (may be <= 0: a wave past the last patch)
        const int irow = lane >> 2;
        float sxa[NL][4];
#pragma unroll
        for (int l = 0; l < NL; ++l)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) sxa[l][rr] = sx[l * NXT + min(i0 + (lane >> 4) * 4 + rr, NXT - 1)];
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            if (l >= nloc) break;                                    // uniform
            float syv[TYT];
#pragma unroll
            for (int j = 0; j < TYT; ++j) syv[j] = sy[l * a.TyP + min(j * 16 + (lane & 15), a.TyP - 1)];
#pragma unroll
            for (int j = 0; j < TYT; ++j)
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    const int col = j * 16 + (lane & 15);
                    if (col < a.TyP) Ew[((lane >> 4) * 4 + rr) * EP + col] = fmaxf(acc[l][j][rr] + (sxa[l][rr] + syv[j]), 0.0f);
                }
            const size_t b = (size_t)by * a.w_o + bx0 + l;
            if VL3D_ABLATE(a.ablate, 1) { if (lane < nrow) a.nn[b * a.n1 + i0 + lane] = 0; continue; }
            const int bj = nn_argmin_rows3(Ew, EP, a.n2, irow, irow < nrow, sub);
            if (irow < nrow && sub == 0) a.nn[b * a.n1 + i0 + irow] = bj;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// get_NN_indices_low_memory on MATERIALISED patches (utils_vid.py:122-142; used by evaluations/NNMSE.py:45-56):
// X [B,n1,d], Y [B,n2,d] dense.  One workgroup per batch entry b; dist[i][j] = sum_k (X[b,i,k]-Y[b,j,k])^2 / d kept in LDS.
// API-parity kernel (the training loss never materialises patches); plain VALU, K staged in chunks.
__global__ __launch_bounds__(256) void nn_vectors_k(const float *__restrict__ X, const float *__restrict__ Y, int n1, int n2, int d,
                                                    int use_alpha, float alpha, int64_t *__restrict__ nn, int KC) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *Xs = smem;                       // [n1][KC+1]
    float *Ys = Xs + (size_t)n1 * (KC + 1); // [n2][KC+1]
    float *E = Ys + (size_t)n2 * (KC + 1);  // [n1][n2]
    float *colmin = E + (size_t)n1 * n2;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *xb = X + (size_t)b * n1 * d, *yb = Y + (size_t)b * n2 * d;
    for (int i = tid; i < n1 * n2; i += 256) E[i] = 0.f;
    for (int k0 = 0; k0 < d; k0 += KC) {
        const int kc = min(KC, d - k0);
        __syncthreads();
        for (int i = tid; i < n1 * kc; i += 256) { const int f = i / kc, k = i - f * kc; Xs[f * (KC + 1) + k] = xb[(size_t)f * d + k0 + k]; }
        for (int i = tid; i < n2 * kc; i += 256) { const int f = i / kc, k = i - f * kc; Ys[f * (KC + 1) + k] = yb[(size_t)f * d + k0 + k]; }
        __syncthreads();
        for (int p = tid; p < n1 * n2; p += 256) {
            const int i = p / n2, j = p - i * n2;
            float acc = 0.f;
            for (int k = 0; k < kc; ++k) { const float df = Xs[i * (KC + 1) + k] - Ys[j * (KC + 1) + k]; acc += df * df; }
            E[p] += acc;
        }
    }
    __syncthreads();
    const float dn = (float)d;
    if (use_alpha) {
        for (int j = tid; j < n2; j += 256) {
            float m = INFINITY;
            for (int i = 0; i < n1; ++i) m = fminf(m, E[i * n2 + j] / dn);
            colmin[j] = alpha + m;
        }
        __syncthreads();
    }
    for (int i = tid; i < n1; i += 256) {
        float best = INFINITY;
        int bj = 0;
        bool best_nan = false;
        for (int j = 0; j < n2; ++j) {
            float v = E[i * n2 + j] / dn;
            if (use_alpha) v = v / colmin[j];
            const bool vn = (v != v);
            if (!best_nan && (vn || v < best)) { best = v; bj = j; best_nan = vn; }
        }
        nn[(size_t)b * n1 + i] = bj;
    }
}

}  // namespace

extern "C" int64_t vl3d_patchnn_scratch_bytes(const vl3d_loss_desc *d) { return patchnn_scratch_bytes(d); }

extern "C" int vl3d_patchnn_choice(const vl3d_loss_desc *desc, int32_t entry, int32_t has_scratch, int32_t x_pitch, int32_t x_frames, int32_t y_pitch,
                                   vl3d_nn_choice *out) {
    VL3D_REQUIRE(out != nullptr && entry >= VL3D_NN_ENTRY_PLAIN && entry <= VL3D_NN_ENTRY_GRAMS,
                 "vl3d_patchnn_choice: null out, or entry is not VL3D_NN_ENTRY_PLAIN, _PREPARED or _GRAMS");
    *out = vl3d_nn_choice{};
    const int rc = check_loss(desc);
    if (rc != VL3D_OK) return rc;
    const PatchNNChoice c = choose_patchnn({desc, entry, has_scratch != 0, x_pitch, x_frames, y_pitch});
    if (c.status != VL3D_OK) vl3d_set_error(c.msg);
    else *out = c;
    return c.status;
}

// ---- one launch table per kernel ----------------------------------------------------------------------------------------------------------
template <int TYT, int NL, int NW, int XS>
static int launch_nn6(const PatchNNChoice &c, const NN2Args &b, hipStream_t s) {
    const int groups_x = (b.w_o + NL - 1) / NL;
    return launch_big_lds<patchnn6_k<TYT, NL, NW, XS>>(dim3((unsigned)(groups_x * b.h_o)), dim3(64 * NW), c.lds_bytes, s, b, groups_x, c.ch);
}
template <bool RUNSUM, int NTHR>
static int launch_nn4(const PatchNNChoice &c, const NN2Args &b, int H, hipStream_t s) {
    const int groups_x = (b.w_o + NL4 - 1) / NL4;
    return launch_big_lds<patchnn4_k<RUNSUM, NTHR>>(dim3((unsigned)(groups_x * b.h_o)), dim3(NTHR), c.lds_bytes, s, b, H, groups_x);
}
static int launch_nn(const PatchNNChoice &c, const NN2Args &b, int H, hipStream_t s) {
    if (c.kernel == 2) return launch_big_lds<patchnn2_k>(dim3((unsigned)(b.h_o * b.w_o)), dim3(NN_THREADS), c.lds_bytes, s, b);
    if (c.kernel == 4) {
        switch (c.threads * 2 + c.runsum) {
        case 256 * 2 + 1: return launch_nn4<true, 256>(c, b, H, s);
        case 256 * 2: return launch_nn4<false, 256>(c, b, H, s);
        case 512 * 2 + 1: return launch_nn4<true, 512>(c, b, H, s);
        case 512 * 2: return launch_nn4<false, 512>(c, b, H, s);
        case 1024 * 2: return launch_nn4<false, 1024>(c, b, H, s);
        }
    }
    if (c.kernel == 6) {
        switch (nn6_key(c.tyt, c.nw, c.xs)) {
#define VL3D_NN6_CASE(I, NW, XS) case nn6_key(NN6_SHAPES[I].tyt, NW, XS): return launch_nn6<NN6_SHAPES[I].tyt, NN6_SHAPES[I].nl, NW, XS>(c, b, s);
#define VL3D_NN6_ROW(I) VL3D_NN6_CASE(I, 4, 14) VL3D_NN6_CASE(I, 4, 16) VL3D_NN6_CASE(I, 8, 14) VL3D_NN6_CASE(I, 8, 16)
            VL3D_NN6_ROW(0) VL3D_NN6_ROW(1) VL3D_NN6_ROW(2)
#undef VL3D_NN6_CASE
#undef VL3D_NN6_ROW
        }
    }
    vl3d_set_error("vl3d_patchnn: the choice names no instantiation of the launch tables");
    return VL3D_EINVAL;
}

// Check, choose, lay out, launch.  x_gram / y_gram != nullptr: that video arrives in kernel 6's own gram16 form (vl3d_video_to_gram_major /
// vl3d_loop_pad_fwd_gram), y as the crop at (y_row0, y_col0) of a clip whose rows are y_pitch pixels long -- the captured video is constant
// training data, so it is rewritten once per pyramid level and not once per iteration; the render's x is written in that form by the loss prologue
static int patchnn_impl(const vl3d_loss_desc *desc, const float *x, const float *x_gram, int32_t x_pitch, int32_t x_frames, const float *y,
                        const float *y_gram, int32_t y_pitch, int32_t y_row0, int32_t y_col0, int32_t *nn, void *scratch, vl3d_stream_t stream) {
    int rc = check_loss(desc);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE((x || x_gram) && (y || y_gram) && nn, "vl3d_patchnn: null pointer");
    const int entry = x_gram ? VL3D_NN_ENTRY_GRAMS : (y_gram ? VL3D_NN_ENTRY_PREPARED : VL3D_NN_ENTRY_PLAIN);
    const PatchNNChoice c = choose_patchnn({desc, entry, scratch != nullptr, x_pitch, x_frames, y_pitch});
    if (c.status != VL3D_OK) {
        vl3d_set_error(c.msg);
        return c.status;
    }
    hipStream_t s = (hipStream_t)stream;
    const PatchGrid g = patch_grid_of(desc);
    const int H = desc->H, W = desc->W, Ty = desc->Ty;
    NN2Args b{};
    b.nn = nn; b.W = W; b.ps = desc->ps; b.pt = desc->pt; b.stride = desc->stride; b.stridet = desc->stridet;
    b.h_o = g.h_o; b.w_o = g.w_o; b.n1 = g.n1; b.n2 = g.n2; b.TxP = g.TxP; b.TyP = g.TyP; b.K = g.K; b.KC = c.kc;
    b.use_alpha = desc->use_alpha; b.alpha = desc->alpha;
    b.dnorm = (float)(3 * desc->pt * desc->ps * desc->ps);      // divisor d (utils_vid.py:83-84 divides)
    b.Wy = y_gram ? y_pitch : W;
    b.ablate = (desc->variant >> 4) & 15;
    // the copies of x and y in the layout the chosen kernel reads.  variant bit 8: the y half of the scratch still holds this y from the previous call
    const dim3 tg((W + 63) / 64, H);
    const bool y_kept = (desc->variant & 0x100) != 0;
    if (c.scratch_layout == VL3D_NN_LAYOUT_GRAM16) {
        uint4 *xs = (uint4 *)scratch;
        if (!x_gram) hipLaunchKernelGGL(video_to_gram16_k<false>, tg, dim3(256), 0, s, x, desc->x_sc, desc->x_st, desc->x_sr, g.TxU, H, W, xs);
        b.xt = x_gram ? x_gram : reinterpret_cast<const float *>(xs);
        if (y_gram) {
            b.yt = reinterpret_cast<const float *>(reinterpret_cast<const uint4 *>(y_gram) + ((size_t)y_row0 * b.Wy + y_col0) * Ty);
        } else {
            // (the y copy sits behind the x copy of the largest x this scratch can hold: its place does not depend on x_gram)
            uint4 *yd = xs + (size_t)H * W * g.TxU;
            if (!y_kept) hipLaunchKernelGGL(video_to_gram16_k<true>, tg, dim3(256), 0, s, y, desc->y_sc, desc->y_st, desc->y_sr, Ty, H, W, yd);
            b.yt = reinterpret_cast<const float *>(yd);
        }
        b.PX = g.TxU; b.PY = Ty;
        b.Wx = x_gram ? x_pitch : W; b.FXm = x_gram ? x_frames : g.TxU;
    } else {
        float *xt = (float *)scratch, *yt = xt + (size_t)H * W * 3 * g.TxP;
        hipLaunchKernelGGL(video_to_pixel_major_k, tg, dim3(256), 0, s, x, desc->x_sc, desc->x_st, desc->x_sr, g.TxU, g.TxP, H, W, xt);
        if (!y_kept) hipLaunchKernelGGL(video_to_pixel_major_k, tg, dim3(256), 0, s, y, desc->y_sc, desc->y_st, desc->y_sr, Ty, g.TyP, H, W, yt);
        b.xt = xt; b.yt = yt;
    }
    rc = launch_nn(c, b, H, s);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_patchnn(const vl3d_loss_desc *desc, const float *x, const float *y, int32_t *nn, void *scratch,
                            vl3d_stream_t stream) {
    return patchnn_impl(desc, x, nullptr, 0, 0, y, nullptr, 0, 0, 0, nn, scratch, stream);
}

extern "C" int64_t vl3d_gram_major_bytes(int32_t T, int32_t H, int32_t W) {
    if (T <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)H * W * T * 16;
}

extern "C" int vl3d_video_to_gram_major(const float *y, int64_t sc, int64_t st, int64_t sr, int32_t T, int32_t H, int32_t W, float *out,
                                        vl3d_stream_t stream) {
    VL3D_REQUIRE(y && out && T > 0 && H > 0 && W > 0, "vl3d_video_to_gram_major: null pointer / non-positive dims");
    hipLaunchKernelGGL(video_to_gram16_k<true>, dim3((W + 63) / 64, H), dim3(256), 0, (hipStream_t)stream, y, sc, st, sr, T, H, W, (uint4 *)out);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_patchnn_prepared(const vl3d_loss_desc *desc, const float *x, const float *y_gram, int32_t y_pitch, int32_t y_rows,
                                     int32_t y_row0, int32_t y_col0, int32_t *nn, void *scratch, vl3d_stream_t stream) {
    VL3D_REQUIRE(desc && y_gram, "vl3d_patchnn_prepared: null pointer");
    VL3D_REQUIRE(y_row0 >= 0 && y_col0 >= 0 && y_row0 + desc->H <= y_rows && y_col0 + desc->W <= y_pitch,
                 "vl3d_patchnn_prepared: the crop (y_row0, y_col0) + (H, W) leaves the prepared clip (y_rows, y_pitch)");
    return patchnn_impl(desc, x, nullptr, 0, 0, nullptr, y_gram, y_pitch, y_row0, y_col0, nn, scratch, stream);
}

extern "C" int vl3d_patchnn_grams(const vl3d_loss_desc *desc, const float *x_gram, int32_t x_pitch, int32_t x_rows, int32_t x_frames, const float *y_gram,
                                  int32_t y_pitch, int32_t y_rows, int32_t y_row0, int32_t y_col0, int32_t *nn, vl3d_stream_t stream) {
    VL3D_REQUIRE(desc && x_gram && y_gram, "vl3d_patchnn_grams: null pointer");
    VL3D_REQUIRE(desc->H <= x_rows && desc->W <= x_pitch && desc->Tx <= x_frames, "vl3d_patchnn_grams: desc (Tx, H, W) leaves the x clip (x_frames, x_rows, x_pitch)");
    VL3D_REQUIRE(y_row0 >= 0 && y_col0 >= 0 && y_row0 + desc->H <= y_rows && y_col0 + desc->W <= y_pitch,
                 "vl3d_patchnn_grams: the crop (y_row0, y_col0) + (H, W) leaves the prepared clip (y_rows, y_pitch)");
    return patchnn_impl(desc, nullptr, x_gram, x_pitch, x_frames, nullptr, y_gram, y_pitch, y_row0, y_col0, nn, nullptr, stream);
}

extern "C" int vl3d_nn_vectors(int64_t B, int32_t n1, int32_t n2, int32_t d, const float *X, const float *Y, int32_t use_alpha,
                               float alpha, int64_t *nn, vl3d_stream_t stream) {
    VL3D_REQUIRE(B > 0 && B < (1ll << 31) && n1 > 0 && n2 > 0 && d > 0 && X && Y && nn, "vl3d_nn_vectors: bad arguments");
    const size_t fixed = ((size_t)n1 * n2 + n2) * sizeof(float);
    VL3D_REQUIRE(fixed + (size_t)(n1 + n2) * 5 * sizeof(float) <= 150 * 1024, "vl3d_nn_vectors: n1*n2 distance matrix does not fit in LDS");
    int kc = (int)((150 * 1024 - fixed) / ((size_t)(n1 + n2) * sizeof(float))) - 1;
    if (kc > 64) kc = 64;
    if (kc > d) kc = d;
    const size_t lds = fixed + (size_t)(n1 + n2) * (kc + 1) * sizeof(float);
    const int rc = launch_big_lds<nn_vectors_k>(dim3((unsigned)B), dim3(256), lds, (hipStream_t)stream, X, Y, n1, n2, d, use_alpha, alpha, nn, kc);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
