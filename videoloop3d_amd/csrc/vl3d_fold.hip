// Looping loss for gfx950, part 2: vote-fold of the matched patches (K4), the robust loss (K5) and the NN-error metric's patch sums.
// The search that produces the indices is vl3d_loss.hip; WHICH fold kernel runs is decided in vl3d_patchnn_choice.h (choose_fold: host only).
//
// Replaces (reference): utils_vid.py:206-229 (FindNNpatchAndMerge / FoldNd), :10-26 + :348 (robust_lossfun().mean()).
#include "vl3d_loss_common.h"

using namespace vl3d_loss_detail;      // the patch grid, fold_shapes[], the choice

namespace {

// robust loss (utils_vid.py:10-26)
struct Rho {
    int kind;      // 0 mse, 1 abs, 2 log1p (rou==0), 3 quadratic (rou==2), 4 general
    float scale, b, d, coef;
    float inv_scale, inv_b;      // host reciprocals for the fused kernel (the two IEEE quotients by constants were ~20 instructions per voxel)
};

__device__ __forceinline__ float rho_f(const Rho &r, float e) {
    switch (r.kind) {
        case 0: return e * e;
        case 1: return fabsf(e);
        case 2: { float s = (e / r.scale); return log1pf(s * s * 0.5f); }
        case 3: { float s = (e / r.scale); return 0.5f * s * s; }
        default: { float s = (e / r.scale); s = s * s; return r.coef * (powf(s / r.b + 1.0f, 0.5f * r.d) - 1.0f) * (r.scale * 10.0f); }
    }
}

__device__ __forceinline__ float rho_g(const Rho &r, float e) {
    switch (r.kind) {
        case 0: return 2.0f * e;
        case 1: return e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f);
        case 2: { float s = e / r.scale; return (s / r.scale) / (1.0f + 0.5f * s * s); }
        case 3: return e / (r.scale * r.scale);
        default: {   // d/de (b/d)((s/b+1)^(d/2)-1)*10*scale, s=(e/scale)^2  ->  10*(e/scale)*(s/b+1)^(d/2-1)
            float s = e / r.scale;
            return 10.0f * s * powf(s * s / r.b + 1.0f, 0.5f * r.d - 1.0f);
        }
    }
}

// value and derivative together (the fused fold kernel): the general Barron case shares one log2/exp2 pair,
// (s^2/b+1)^(d/2) = exp2(d/2 * log2(u)) and the derivative's power is that over u -- instead of two powf calls
__device__ __forceinline__ void rho_fg(const Rho &r, float e, float &f, float &g) {
    if (r.kind == 4) {
        const float s = e * r.inv_scale;
        const float u = fmaf(s * s, r.inv_b, 1.0f);
        const float p = __builtin_amdgcn_exp2f(0.5f * r.d * __builtin_amdgcn_logf(u));
        f = r.coef * (p - 1.0f) * (r.scale * 10.0f);
        g = 10.0f * s * p * __builtin_amdgcn_rcpf(u);
    } else {
        f = rho_f(r, e);
        g = rho_g(r, e);
    }
}

struct FoldArgs {
    const float *y;
    const int32_t *nn;
    float *sum, *weight;
    int Tx, H, W, ps, pt, stride, stridet, h_o, w_o, n1;
    int64_t y_sc, y_st, y_sr;
    int normalize;
    // fused robust loss (vl3d_vote_fold_robust): x (strided like the loss desc), per-element gradient rho'(x - y2x) * gscale and
    // the loss sum, all optional (x == nullptr: plain fold)
    const float *x;
    int64_t x_sc, x_st, x_sr;
    Rho rho;
    float gscale;
    float *gx;
    int64_t gx_sc, gx_st, gx_sr;      // strides of gx (channel, frame, row), unit column stride
    double *loss_sum;
};

__global__ __launch_bounds__(256) void vote_fold_k(FoldArgs a) {
    const int xi = blockIdx.x * 64 + (threadIdx.x & 63);
    const int eta = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int tau = blockIdx.z;
    if (xi >= a.W || eta >= a.H) return;
    // covering patch rows/cols: by*s <= eta < by*s+ps
    const int by_hi = min(a.h_o - 1, eta / a.stride);
    const int by_lo = max(0, (eta - a.ps + a.stride) / a.stride);   // ceil((eta-ps+1)/s) for eta-ps+1 > 0
    const int bx_hi = min(a.w_o - 1, xi / a.stride);
    const int bx_lo = max(0, (xi - a.ps + a.stride) / a.stride);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    int cnt = 0;
    const int64_t pix = (int64_t)eta * a.y_sr + xi;
    for (int kt = 0; kt < a.pt; ++kt) {
        const int ts = tau - kt;
        if (ts < 0 || (ts % a.stridet) != 0) continue;
        const int i = ts / a.stridet;
        if (i >= a.n1) continue;
        for (int by = by_lo; by <= by_hi; ++by)
            for (int bx = bx_lo; bx <= bx_hi; ++bx) {
                const int j = a.nn[((size_t)by * a.w_o + bx) * a.n1 + i];
                const int64_t off = (int64_t)(j * a.stridet + kt) * a.y_st + pix;
                s0 += a.y[off];
                s1 += a.y[a.y_sc + off];
                s2 += a.y[2 * a.y_sc + off];
                ++cnt;
            }
    }
    const float wgt = fmaxf((float)cnt, 1e-10f);                  // utils_vid.py:228
    const size_t o = ((size_t)tau * a.H + eta) * a.W + xi;
    const size_t cs = (size_t)a.Tx * a.H * a.W;
    if (a.normalize) { s0 /= wgt; s1 /= wgt; s2 /= wgt; }
    a.sum[o] = s0; a.sum[cs + o] = s1; a.sum[2 * cs + o] = s2;
    a.weight[o] = wgt;
}

// vote-fold, LDS-staged: one workgroup = a FT_W x FT_H pixel tile of ONE channel.  The y columns of the tile (all Ty
// frames) and the NN indices of every patch location covering the tile are staged in LDS once; each thread then produces
// its pixel's whole temporal column (all Tx frames) from LDS: the gather of utils_vid.py:217 + FoldNd (:218-227) without
// any scattered global access.  (v1 -- one thread per voxel reading y and nn through L2 -- measured 12.3 ms at 720p.)
// Tile shapes (FT_W x FT_H pixels, FT_NT threads = pixels x FT_G temporal groups): see fold_shapes[] below.

// NB > 0 (patch-major form only): a pixel is covered by at most NB x NB patch locations (NB = ceil(ps / stride): 3 for the shipped ref view,
// 2 for the other views).  The covering loops then have a FIXED trip count -- a location that does not exist reads its index from a
// row of the table that points at three all-zero frames behind the staged column, i.e. votes 0 -- so a row of NB index reads is issued
// together and its 3 NB vote reads behind them together, instead of one dependent index -> vote chain per location under dynamic
// loop bounds (the PMC pass had the kernel waiting in 66 % of its wave-cycles and VALU bound on the address arithmetic,
// profiles/r03_pmc_summary.txt).  y + 0 == y: same sums, same order.
template <int FT_W, int FT_H, int FT_NT, int NB = 0>
__global__ __launch_bounds__(FT_NT) void vote_fold_lds_k(FoldArgs a, int Ty) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NP = FT_W * FT_H, FT_G = FT_NT / NP, NT = FT_NT;
    float *ys = smem;                                            // [Ty + 3][NP]: the tile's y columns, then three zero frames
    int *nns = reinterpret_cast<int *>(smem + (size_t)(Ty + 3) * NP);   // [nby][nbx][n1], then n1 indices of the zero frames
    const int tid = threadIdx.x, pix = tid % NP, grp = tid / NP, lx = pix % FT_W, ly = pix / FT_W;
    const int x0 = blockIdx.x * FT_W, y0 = blockIdx.y * FT_H, c = blockIdx.z;
    const int xi = x0 + lx, eta = y0 + ly;
    // patch locations covering any pixel of the tile
    const int y1 = min(y0 + FT_H, a.H) - 1, x1 = min(x0 + FT_W, a.W) - 1;
    const int tby0 = max(0, (y0 - a.ps + a.stride) / a.stride), tby1 = min(a.h_o - 1, y1 / a.stride);
    const int tbx0 = max(0, (x0 - a.ps + a.stride) / a.stride), tbx1 = min(a.w_o - 1, x1 / a.stride);
    const int nby = tby1 - tby0 + 1, nbx = tbx1 - tbx0 + 1;
    // stage y[c, :, tile] (row segments of FT_W floats) and the nn indices
    const bool inb = (xi < a.W) && (eta < a.H);
    const float *ysrc = a.y + (int64_t)c * a.y_sc + (int64_t)min(eta, a.H - 1) * a.y_sr + min(xi, a.W - 1);
    // Each temporal group owns a contiguous run of frames (see below).  The x values the fused loss needs do not depend on the
    // staging: the first four of this thread's column are requested BEFORE it and the rest stay four frames ahead of their use, so
    // the column's global reads are never exposed one by one between the LDS chains.
    const bool slide = (a.pt == 3 && a.stridet == 1);
    const int chunk = (a.Tx + FT_G - 1) / FT_G, t0 = slide ? grp * chunk : grp, t1 = slide ? min(a.Tx, t0 + chunk) : a.Tx;
    const int tstep = slide ? 1 : FT_G;
    const float *xsrc = a.x ? a.x + (int64_t)c * a.x_sc + (int64_t)min(eta, a.H - 1) * a.x_sr + min(xi, a.W - 1) : nullptr;
    // (the prefetch pointer walks by a frame step: no 64-bit multiply per load)
    const int64_t xstep = (int64_t)tstep * a.x_st;
    const float *xnext = xsrc ? xsrc + (int64_t)t0 * a.x_st : nullptr;
    int tnext = t0;
    auto xload = [&]() -> float {
#if defined(VL3D_FOLD_ABLATE) && (VL3D_FOLD_ABLATE & 4)      // measurement build only (WRONG values): every fourth lane moves its four pixels' x as ONE 16-byte load
        float v = 0.f;
        if (xnext && tnext < t1 && (tid & 3) == 0 && xi + 3 < a.W) {
            const float4 q = *reinterpret_cast<const float4 *>(reinterpret_cast<uintptr_t>(xnext) & ~(uintptr_t)15);
            v = q.x + q.y + q.z + q.w;
        }
#else
        const float v = (xnext && tnext < t1) ? *xnext : 0.f;
#endif
        xnext += xstep; tnext += tstep;
        return v;
    };
    // queue depth: measured (profiles/fold_time.py, round 6): with votes and staging ablated the kernel still took 0.77 of its 1.0 ms -- its x / gx /
    // y2x streams run one 256-byte row segment per wave and request, so the bytes in flight (requests ahead x 24 waves per CU) set the rate
    // (same box, 720p, ms: other views 0.884 / 0.830 / 0.792 / 0.944 at 4 / 8 / 13 / 16 requests ahead; the ref view's NB = 3 instantiation
    // sits at its register budget for three workgroups per CU and loses with every deeper queue: 0.898 / 0.913 / 1.038 / 1.056)
#ifdef VL3D_FOLD_XQ
    constexpr int XQ = VL3D_FOLD_XQ;
#else
    constexpr int XQ = NB >= 3 ? 4 : 12;
#endif
    float xq[XQ];
#pragma unroll
    for (int k = 0; k < XQ; ++k) xq[k] = xload();
    {   // (source pointer and LDS slot walk by a group step: no 64-bit multiply per frame)
        const float *yf = ysrc + (int64_t)grp * a.y_st;
        const int64_t ystep = (int64_t)FT_G * a.y_st;
        float *yd = ys + grp * NP + pix;
#pragma unroll 8
#if defined(VL3D_FOLD_ABLATE) && (VL3D_FOLD_ABLATE & 2)      // measurement build only: no staging loads
        for (int f = grp; f < Ty; f += FT_G, yd += FT_G * NP) *yd = 0.25f;
#else
        for (int f = grp; f < Ty; f += FT_G, yf += ystep, yd += FT_G * NP) *yd = *yf;
#endif
    }
    // the covering locations' index rows: a run of n1 consecutive ints per location -- rows of the tile's locations are contiguous in nn
    // along bx, so a (by) row of the table is ONE contiguous run of nbx * n1 ints: no division per element
    {
        const int run = nbx * a.n1, mul = slide ? NP : 1;
        for (int by = 0; by < nby; ++by) {
            const int32_t *src = a.nn + ((size_t)(tby0 + by) * a.w_o + tbx0) * a.n1;
            int *dst = nns + by * run;
            for (int i = tid; i < run; i += NT) dst[i] = src[i] * mul;
        }
        for (int i = tid; i < 3 * NP; i += NT) ys[Ty * NP + i] = 0.f;
        for (int i = tid; i < a.n1; i += NT) nns[nby * run + i] = Ty * mul;
    }
    __syncthreads();
    float lacc = 0.f;
    if (inb) {
    const int by_hi = min(a.h_o - 1, eta / a.stride), by_lo = max(0, (eta - a.ps + a.stride) / a.stride);
    const int bx_hi = min(a.w_o - 1, xi / a.stride), bx_lo = max(0, (xi - a.ps + a.stride) / a.stride);
    const int npatch = (by_hi - by_lo + 1) * (bx_hi - bx_lo + 1);
    const size_t cs = (size_t)a.Tx * a.H * a.W, fs = (size_t)a.H * a.W;
    float *out = a.sum + (size_t)c * cs + (size_t)eta * a.W + xi;      // (a.sum == nullptr, fused loss only: y2x / weight stay in registers)
    float *wout = a.weight + (size_t)eta * a.W + xi;
    const int *nn0 = nns + ((by_lo - tby0) * nbx + (bx_lo - tbx0)) * a.n1;
    const float *ysp = ys + pix;
    float *gxp = a.x ? a.gx + (int64_t)c * a.gx_sc + (int64_t)t0 * a.gx_st + (int64_t)eta * a.gx_sr + xi : nullptr;      // walks by a frame step
    const int64_t gxstep = (int64_t)tstep * a.gx_st;
    // Each temporal group owns a contiguous run of frames.  With pt == 3 and stridet == 1 (every shipped configuration) the
    // votes are accumulated patch-major: patch i votes for frames i, i+1, i+2, so its NN index is read from LDS ONCE and the
    // three frame sums slide through registers (w0 = frame i, complete after patch i) -- a third of the index reads and of the
    // address arithmetic of the frame-major form below, and the same summation order per frame (kt = 2, 1, 0 -> patches i-2, i-1, i).
    float w0 = 0.f, w1 = 0.f, w2 = 0.f;
    constexpr int NBB = NB > 0 ? NB * NB : 1;
    int loc_off[NBB];            // NB > 0: index rows of the covering locations relative to nn0 (the zero-frame row for one that does not exist)
    if constexpr (NB > 0) {
        const int zero_row = (int)(nns + nby * nbx * a.n1 - nn0);
#pragma unroll
        for (int k = 0; k < NBB; ++k) {
            const int by = k / NB, bx = k % NB;
            const bool ok = by <= by_hi - by_lo && bx <= bx_hi - bx_lo;
            loc_off[k] = ok ? (by * nbx + bx) * a.n1 : zero_row;
        }
    }
    for (int tau = slide ? t0 - 2 : t0; tau < t1; tau += tstep) {
        float s = 0.f;
        int cnt = 0;
        if (slide) {
            const int i = tau;                                     // patch index == first frame it votes for
#if defined(VL3D_FOLD_ABLATE) && (VL3D_FOLD_ABLATE & 1)      // measurement build only: no votes
            if (false) {
#else
            if (i >= 0 && i < a.n1) {
#endif
                if constexpr (NB > 0) {
                    // one row of locations at a time: NB index reads together, then their 3 NB vote reads together (all NB x NB at once
                    // needed 102 registers for NB = 3 -- two workgroups per CU instead of three)
#pragma unroll
                    for (int r = 0; r < NB; ++r) {
                        int idx[NB];
#pragma unroll
                        for (int q = 0; q < NB; ++q) idx[q] = nn0[loc_off[r * NB + q] + i];
#pragma unroll
                        for (int q = 0; q < NB; ++q) {
                            const float *yp = ysp + idx[q];
                            w0 += yp[0]; w1 += yp[NP]; w2 += yp[2 * NP];
                        }
                        if (NB > 2 && r + 1 < NB) __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
                const int *nrow = nn0 + i;
                for (int by = by_lo; by <= by_hi; ++by, nrow += nbx * a.n1) {
                    const int *np = nrow;
                    for (int bx = bx_lo; bx <= bx_hi; ++bx, np += a.n1) {
                        const float *yp = ysp + *np;                    // staged as index * NP
                        w0 += yp[0]; w1 += yp[NP]; w2 += yp[2 * NP];
                    }
                }
                }
            }
            s = w0; w0 = w1; w1 = w2; w2 = 0.f;
            if (tau < t0) continue;
            cnt = npatch * (min(tau, a.n1 - 1) - max(tau - 2, 0) + 1);
        } else {
        for (int kt = 0; kt < a.pt; ++kt) {
            const int ts = tau - kt;
            if (ts < 0 || (ts % a.stridet) != 0) continue;
            const int i = ts / a.stridet;
            if (i >= a.n1) continue;
            const int *nrow = nn0 + i;
            for (int by = by_lo; by <= by_hi; ++by, nrow += nbx * a.n1) {
                const int *np = nrow;
                for (int bx = bx_lo; bx <= bx_hi; ++bx, np += a.n1) s += ysp[(*np * a.stridet + kt) * NP];
            }
            cnt += npatch;
        }
        }
        const float wgt = fmaxf((float)cnt, 1e-10f);                  // utils_vid.py:228
        // (the vote count is a small integer: s * rcp(count) is within an ulp of the reference's quotient, a fifth of its instructions)
        const float v = a.normalize ? s * __builtin_amdgcn_rcpf(wgt) : s;
        if (a.sum) {      // uniform
            out[(size_t)tau * fs] = v;
            if (c == 0) wout[(size_t)tau * fs] = wgt;
        }
        if (a.x) {      // robust_lossfun(x - y2x) and its derivative while y2x is in a register (utils_vid.py:348)
            const float e = xq[0] - v;
#pragma unroll
            for (int k = 0; k + 1 < XQ; ++k) xq[k] = xq[k + 1];
            xq[XQ - 1] = xload();
            float f, g;
            rho_fg(a.rho, e, f, g);
            lacc += f;
#if defined(VL3D_FOLD_ABLATE) && (VL3D_FOLD_ABLATE & 4)      // measurement build only: ... and their gx as ONE 16-byte store
            if ((tid & 3) == 0 && xi + 3 < a.W) *reinterpret_cast<float4 *>(reinterpret_cast<uintptr_t>(gxp) & ~(uintptr_t)15) = make_float4(g, g, g, g);
#else
            *gxp = g * a.gscale;
#endif
            gxp += gxstep;
        }
    }
    }
    if (a.x) {          // block sum of the loss -> one double atomic
        __shared__ float red[FT_NT / 64];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) lacc += __shfl_down(lacc, off, 64);
        if ((tid & 63) == 0) red[tid >> 6] = lacc;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int i = 0; i < NT / 64; ++i) t += (double)red[i];
            atomicAdd(a.loss_sum, t);
        }
    }
}

__global__ __launch_bounds__(256) void robust_fwd_k(int64_t n, const float *__restrict__ x, const float *__restrict__ y2x,
                                                    Rho r, double *__restrict__ out) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        acc += rho_f(r, x[i] - y2x[i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, (double)red[0] + (double)red[1] + (double)red[2] + (double)red[3]);
}

__global__ __launch_bounds__(256) void robust_bwd_k(int64_t n, const float *__restrict__ x, const float *__restrict__ y2x,
                                                    Rho r, const float *__restrict__ gout, float inv_n,
                                                    float *__restrict__ gx) {
    const float g = (*gout) * inv_n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        gx[i] = rho_g(r, x[i] - y2x[i]) * g;
}

Rho make_rho(int kind, float rou, float scale) {
    Rho r{};
    r.scale = scale;
    if (kind == VL3D_RHO_MSE) r.kind = 0;
    else if (kind == VL3D_RHO_ABS) r.kind = 1;
    else if (rou == 0.0f) r.kind = 2;
    else if (rou == 2.0f) r.kind = 3;
    else {
        r.kind = 4;
        const float eps = 1e-6f;
        r.b = fabsf(rou - 2.0f) + eps;
        r.d = rou >= 0.f ? rou + eps : rou - eps;
        r.coef = r.b / r.d;
        r.inv_b = 1.0f / r.b;
    }
    r.inv_scale = 1.0f / scale;
    return r;
}

}  // namespace

extern "C" int vl3d_vote_fold_choice(const vl3d_loss_desc *desc, int32_t fused, vl3d_fold_choice *out) {
    VL3D_REQUIRE(out != nullptr, "vl3d_vote_fold_choice: null out");
    *out = vl3d_fold_choice{};
    const int rc = check_loss(desc);
    if (rc != VL3D_OK) return rc;
    const FoldChoice c = choose_fold(desc, fused != 0);
    if (c.status != VL3D_OK) vl3d_set_error(c.msg);
    else *out = c;
    return c.status;
}

template <int FW, int FH, int NT, int NB>
static int launch_fold_lds(const FoldChoice &c, const vl3d_loss_desc *desc, const FoldArgs &a, hipStream_t s) {
    dim3 grid((desc->W + FW - 1) / FW, (desc->H + FH - 1) / FH, 3);
    return launch_big_lds<vote_fold_lds_k<FW, FH, NT, NB>, 159 * 1024>(grid, dim3(NT), c.lds_bytes, s, a, desc->Ty);
}
// the descriptor's part of the argument block, then the kernel choose_fold() names (rows of fold_shapes[] x the covering-loop forms)
static int launch_fold(const FoldChoice &c, const vl3d_loss_desc *desc, FoldArgs &a, hipStream_t s) {
    const PatchGrid g = patch_grid_of(desc);
    a.Tx = desc->Tx; a.H = desc->H; a.W = desc->W; a.ps = desc->ps; a.pt = desc->pt;
    a.stride = desc->stride; a.stridet = desc->stridet;
    a.h_o = g.h_o; a.w_o = g.w_o; a.n1 = g.n1;
    a.y_sc = desc->y_sc; a.y_st = desc->y_st; a.y_sr = desc->y_sr;
    if (!c.staged) {
        dim3 grid((desc->W + 63) / 64, (desc->H + 3) / 4, desc->Tx);
        hipLaunchKernelGGL(vote_fold_k, grid, dim3(256), 0, s, a);
        return VL3D_OK;
    }
    switch (c.shape * 4 + c.nb) {
#define VL3D_FOLD_ROW(I, NB) case I * 4 + NB: return launch_fold_lds<fold_shapes[I].fw, fold_shapes[I].fh, fold_shapes[I].nt, NB>(c, desc, a, s);
#define VL3D_FOLD_ROWS(I) VL3D_FOLD_ROW(I, 0) VL3D_FOLD_ROW(I, 2) VL3D_FOLD_ROW(I, 3)
        VL3D_FOLD_ROWS(0) VL3D_FOLD_ROWS(1) VL3D_FOLD_ROWS(2) VL3D_FOLD_ROWS(3) VL3D_FOLD_ROWS(4)
#undef VL3D_FOLD_ROWS
#undef VL3D_FOLD_ROW
    }
    static_assert(N_FOLD_SHAPES == 5, "launch_fold's rows are fold_shapes[]");
    vl3d_set_error("vl3d_vote_fold: the choice names no instantiation of the launch table");
    return VL3D_EINVAL;
}

extern "C" int vl3d_vote_fold(const vl3d_loss_desc *desc, const float *y, const int32_t *nn, float *sum, float *weight,
                              int32_t normalize, vl3d_stream_t stream) {
    int rc = check_loss(desc);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(y && nn && sum && weight, "vl3d_vote_fold: null pointer");
    const FoldChoice c = choose_fold(desc, false);
    VL3D_REQUIRE(c.status == VL3D_OK, c.msg);
    FoldArgs a{};
    a.y = y; a.nn = nn; a.sum = sum; a.weight = weight;
    a.normalize = normalize;
    rc = launch_fold(c, desc, a, (hipStream_t)stream);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_vote_fold_robust_strided(const vl3d_loss_desc *desc, const float *y, const int32_t *nn, const float *x, int32_t kind,
                                             float rou, float scale, float *y2x, float *weight, float *grad_x, int64_t gx_sc,
                                             int64_t gx_st, int64_t gx_sr, double *loss_sum, vl3d_stream_t stream) {
    int rc = check_loss(desc);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(y && nn && x && grad_x && loss_sum, "vl3d_vote_fold_robust: null pointer");
    VL3D_REQUIRE((y2x == nullptr) == (weight == nullptr), "vl3d_vote_fold_robust: y2x and weight are written together or not at all");
    VL3D_REQUIRE(kind >= 0 && kind <= 2 && scale != 0.0f, "vl3d_vote_fold_robust: bad rho kind / scale");
    VL3D_REQUIRE(gx_sr >= desc->W && gx_st >= 0 && gx_sc >= 0, "vl3d_vote_fold_robust: bad grad_x strides");
    const FoldChoice c = choose_fold(desc, true);
    if (c.status != VL3D_OK) {
        vl3d_set_error(c.msg);
        return c.status;
    }
    FoldArgs a{};
    a.y = y; a.nn = nn; a.sum = y2x; a.weight = weight;
    a.normalize = 1;
    a.x = x; a.x_sc = desc->x_sc; a.x_st = desc->x_st; a.x_sr = desc->x_sr;
    a.rho = make_rho(kind, rou, scale);
    a.gscale = 1.0f / (3.0f * (float)desc->Tx * (float)desc->H * (float)desc->W);     // d(mean)/d(element)
    a.gx = grad_x; a.gx_sc = gx_sc; a.gx_st = gx_st; a.gx_sr = gx_sr; a.loss_sum = loss_sum;
    VL3D_HIP(hipMemsetAsync(loss_sum, 0, sizeof(double), (hipStream_t)stream));
    rc = launch_fold(c, desc, a, (hipStream_t)stream);
    if (rc != VL3D_OK) return rc;
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_vote_fold_robust(const vl3d_loss_desc *desc, const float *y, const int32_t *nn, const float *x, int32_t kind,
                                     float rou, float scale, float *y2x, float *weight, float *grad_x, double *loss_sum,
                                     vl3d_stream_t stream) {
    if (!desc) { vl3d_set_error("vl3d_vote_fold_robust: null descriptor"); return VL3D_EINVAL; }
    const int64_t fs = (int64_t)desc->H * desc->W;
    return vl3d_vote_fold_robust_strided(desc, y, nn, x, kind, rou, scale, y2x, weight, grad_x, fs * desc->Tx, fs, desc->W, loss_sum, stream);
}

extern "C" int vl3d_robust_fwd(int64_t n, const float *x, const float *y2x, int32_t kind, float rou, float scale,
                               double *loss_sum, vl3d_stream_t stream) {
    VL3D_REQUIRE(n > 0 && x && y2x && loss_sum, "vl3d_robust_fwd: bad arguments");
    VL3D_REQUIRE(kind >= 0 && kind <= 2 && scale != 0.0f, "vl3d_robust_fwd: bad rho kind / scale");
    VL3D_HIP(hipMemsetAsync(loss_sum, 0, sizeof(double), (hipStream_t)stream));
    const unsigned blocks = (unsigned)(ceil_div64(n, 256) < 4096 ? ceil_div64(n, 256) : 4096);
    hipLaunchKernelGGL(robust_fwd_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, x, y2x, make_rho(kind, rou, scale),
                       loss_sum);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

extern "C" int vl3d_robust_bwd(int64_t n, const float *x, const float *y2x, int32_t kind, float rou, float scale,
                               const float *grad_out, float inv_n, float *grad_x, vl3d_stream_t stream) {
    VL3D_REQUIRE(n > 0 && x && y2x && grad_out && grad_x, "vl3d_robust_bwd: bad arguments");
    VL3D_REQUIRE(kind >= 0 && kind <= 2 && scale != 0.0f, "vl3d_robust_bwd: bad rho kind / scale");
    const unsigned blocks = (unsigned)(ceil_div64(n, 256) < 4096 ? ceil_div64(n, 256) : 4096);
    hipLaunchKernelGGL(robust_bwd_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, x, y2x, make_rho(kind, rou, scale),
                       grad_out, inv_n, grad_x);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}

// ---------------------------------------------------------------------------------------------------
// NN-error metric support (evaluations/NNMSE.py:45-56): per patch location b
//   err[b] = sum_i sum_{c,kt,kh,kw} | y[c, nn_b[i]*st+kt, .] - x[c, i*st+kt, .] |   (the caller normalises / groups by macro block)
__global__ __launch_bounds__(256) void patch_l1_k(const float *__restrict__ x, const float *__restrict__ y, const int32_t *__restrict__ nn,
                                                  int ps, int pt, int stride, int stridet, int w_o, int n1, int64_t x_sc, int64_t x_st,
                                                  int64_t x_sr, int64_t y_sc, int64_t y_st, int64_t y_sr, float *__restrict__ err) {
    __shared__ float red[4];
    const int b = blockIdx.x, by = b / w_o, bx = b % w_o, r0 = by * stride, c0 = bx * stride;
    const int per = 3 * pt * ps * ps, total = n1 * per;
    float acc = 0.f;
    for (int e = threadIdx.x; e < total; e += 256) {
        const int i = e / per, k = e - i * per;
        const int c = k / (pt * ps * ps), r1 = k - c * pt * ps * ps, kt = r1 / (ps * ps), r2 = r1 - kt * ps * ps, kh = r2 / ps, kw = r2 - kh * ps;
        const int j = nn[(size_t)b * n1 + i];
        const int64_t sp = (int64_t)(r0 + kh);
        const float xv = x[c * x_sc + (int64_t)(i * stridet + kt) * x_st + sp * x_sr + c0 + kw];
        const float yv = y[c * y_sc + (int64_t)(j * stridet + kt) * y_st + sp * y_sr + c0 + kw];
        acc += fabsf(yv - xv);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) err[b] = red[0] + red[1] + red[2] + red[3];
}

extern "C" int vl3d_patch_l1(const vl3d_loss_desc *desc, const float *x, const float *y, const int32_t *nn, float *err,
                             vl3d_stream_t stream) {
    int rc = check_loss(desc);
    if (rc != VL3D_OK) return rc;
    VL3D_REQUIRE(x && y && nn && err, "vl3d_patch_l1: null pointer");
    const PatchGrid g = patch_grid_of(desc);
    hipLaunchKernelGGL(patch_l1_k, dim3((unsigned)(g.h_o * g.w_o)), dim3(256), 0, (hipStream_t)stream, x, y, nn, desc->ps, desc->pt,
                       desc->stride, desc->stridet, g.w_o, g.n1, desc->x_sc, desc->x_st, desc->x_sr, desc->y_sc, desc->y_st, desc->y_sr, err);
    VL3D_CHECK_LAUNCH();
    return VL3D_OK;
}
