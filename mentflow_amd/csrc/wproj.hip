// Weighted projection histograms for gfx950: the counterparts of the six projection kernels of kde.hip for particles that carry
// a weight each (importance weights of the annealed / sequential Monte-Carlo samplers, macro-particle charges).
//   1-D KDE      S[p,k]   = sum_n w_n exp(-((x_n . V_p - c_k) / sigma)^2 / 2)
//   2-D KDE      S[p,a,b] = sum_n w_n Kx_na Ky_nb
//   backward     gx_n = w_n * (the unweighted gx_n),   gw_n = sum_p sum_k gS[p,k] K_pk(x_n)          (one launch for both)
//   hard bins    sums[p,k] = sum of w_n over the rows whose projection falls into bin k   (torch.histogram(weight=...))
//
// Everything about the window — row loads, projection, centre bin, plain and factorised Gaussian window, dead corner cells,
// the 2^-50 fixed point, the flush and the finishing arithmetic — is kde_window.h, shared with kde.hip; the launch shapes are
// those of kde_plan.h for the unweighted kernel of the same sizes (a weight costs no LDS).  What is new is one float load per
// particle and one multiply per finished window value.
//
// Fixed point with weights.  to_fix takes values in [0, 1], so the forwards accumulate (w_n / w_max) K with w_max the largest
// valid weight, read from a DEVICE scalar (the caller forms it with a device-side reduction: no host synchronisation), and the
// finishing kernel multiplies w_max back in.  w_n / w_max <= 1 is a correctly rounded division, clamped to 1 should a caller
// pass a w_max below its largest weight.  The 8 192-particle bound per workgroup and the shift rule of fix_flush carry over
// unchanged: sums are exact integers, independent of the order of particles and workgroups, bitwise reproducible.  With all
// weights 1 every product is exact and the result equals the unweighted kernel's bit for bit; a common power-of-two factor
// passes through w_max and scales the result exactly.
// A contribution (w_n / w_max) K below 2^-50 rounds to zero: a particle 2^50 times lighter than the heaviest one is not seen,
// and a bin's total carries an absolute error of at most (particles in its window) * 2^-50 * w_max.
//
// Invalid weights.  A weight that is not finite and positive (0, negative, NaN, +-inf) contributes nothing to S and gets
// gx = 0; the caller leaves it out of w_max.  gw is the plain kernel sum for every row whose weight is valid or zero (a zero
// weight can grow) and 0 for a negative, NaN or infinite one.  NaN / infinite coordinates give an empty window as in kde.hip.
// If w_max is not finite and positive (no valid weight) S is all zero.
//
// The backward kernels use no atomics: gS staged in LDS, lanes split as in kde.hip (CH lanes per particle in 1-D, NPT particles
// per thread in 2-D), partial rows summed by a fixed butterfly.  Either output may be NULL; `accumulate` covers both.
#include "kde_window.h"

namespace mf {

constexpr float WPROJ_FLT_MAX = 3.4028234663852886e38f;

__device__ __forceinline__ bool weight_valid(float w) { return w > 0.0f && w <= WPROJ_FLT_MAX; }   // NaN compares false
// w / w_max in [0, 1] for to_fix; 0 for an invalid weight or an invalid w_max
__device__ __forceinline__ float weight_ratio(float w, float wmax) {
    return (weight_valid(w) && weight_valid(wmax)) ? fminf(w / wmax, 1.0f) : 0.0f;
}
// the weight the backward multiplies gx with, and whether a row gets a gw at all
__device__ __forceinline__ float weight_or_zero(float w) { return weight_valid(w) ? w : 0.0f; }
__device__ __forceinline__ bool weight_can_grow(float w) { return w >= 0.0f && w <= WPROJ_FLT_MAX; }

// ------------------------------------------------------------------------------------------------ 1-D forward
// grid, block and LDS as proj_kde1d_fwd_kernel
template <int RT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void proj_wkde1d_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ wmax_p, int64_t n, int d,
    const float* __restrict__ V, int P, int Pg, const float* __restrict__ coords, int B, float inv_sigma, int Rrt,
    u64* __restrict__ Sacc, int per_wg, int gshift) {
    MF_DYN_SMEM(u64, lds);
    u64* img = lds;
    float* Vl = reinterpret_cast<float*>(img + (size_t)Pg * B);
    float* cl = Vl + Pg * KDE_VS;
    const int p_begin = blockIdx.y * Pg;
    const int np = min(Pg, P - p_begin);
    const int R = RT > 0 ? RT : Rrt;
    for (int i = threadIdx.x; i < np * B; i += BLOCK) img[i] = 0;
    stage_vrows<BLOCK>(Vl, V, p_begin, np, d);
    for (int i = threadIdx.x; i < B; i += BLOCK) cl[i] = coords[i];
    __syncthreads();
    const float wmax = wmax_p[0];
    const float c0 = cl[0];
    const float delta = cl[1] - cl[0];
    const float inv_delta = 1.0f / delta;
    const float s = delta * inv_sigma;
    const bool fact_ok = RT > 0 && s >= 2.0f && s <= 2.6f;                  // see proj_kde1d_fwd_kernel
    const GaussGamma<(RT > 0 ? RT : 2)> gm = gauss_gamma<(RT > 0 ? RT : 2)>(fact_ok ? s : 2.0f);
    const int64_t p_lo = (int64_t)blockIdx.x * per_wg;
    const int64_t p_hi = min(n, p_lo + per_wg);
    for (int64_t p = p_lo + threadIdx.x; p < p_hi; p += BLOCK) {
        const float wn = weight_ratio(wt[p], wmax);
        if (wn == 0.0f) continue;
        float xv[KDE_DMAX];
        load_row(x, p, d, xv);
        for (int q = 0; q < np; ++q) {
            float vq[KDE_DMAX];
            load_vrow(Vl, q, vq);
            const float u = project8(xv, vq);
            const int kc = centre_bin(u, c0, inv_delta, B, R);
            u64* row = img + (size_t)q * B;
            if (fact_ok) {
                float w[2 * (RT > 0 ? RT : 2) + 1];
                gauss_window<(RT > 0 ? RT : 2)>(u, cl, kc, B, inv_sigma, s, gm, w);
#pragma unroll
                for (int j = -RT; j <= RT; ++j) {
                    const int k = kc + j;
                    if (k >= 0 && k < B) {
                        const u64 f = to_fix(wn * w[j + RT]);
                        if (f != 0) atomicAdd(&row[k], f);
                    }
                }
            } else {
                for (int j = -R; j <= R; ++j) {
                    const int k = kc + j;
                    if (k >= 0 && k < B) {
                        const u64 f = to_fix(wn * gauss_weight((u - cl[k]) * inv_sigma));
                        if (f != 0) atomicAdd(&row[k], f);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < np * B; i += BLOCK) fix_flush(Sacc + (int64_t)p_begin * B + i, img[i], gshift);
}

// S[i] = fp32(acc[i] * 2^(shift-50) * w_max)
__global__ __launch_bounds__(KDE_BLOCK) void wacc_to_float_kernel(const u64* __restrict__ Sacc, float* __restrict__ S,
                                                                   int64_t total, double unit,
                                                                   const float* __restrict__ wmax_p) {
    const float wmax = wmax_p[0];
    const double scaled = unit * (weight_valid(wmax) ? (double)wmax : 0.0);     // unit is a power of two: exact
    for (int64_t i = (int64_t)blockIdx.x * KDE_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * KDE_BLOCK)
        S[i] = fix_value(Sacc[i], scaled);
}

// ------------------------------------------------------------------------------------------------ 1-D backward
// grid, block, LDS and lane splitting as proj_kde1d_bwd_kernel; dk collects sum_k gS K beside du
template <int RT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void proj_wkde1d_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, int64_t n, int d, const float* __restrict__ V, int P, int Pg,
    const float* __restrict__ coords, int B, float inv_sigma, int R, const float* __restrict__ gS, float* __restrict__ gx,
    float* __restrict__ gw, int accumulate, int CH) {
    MF_DYN_SMEM(float, lds);
    float* img = lds;
    float* Vl = img + Pg * B;
    float* cl = Vl + Pg * KDE_VS;
    for (int i = threadIdx.x; i < B; i += BLOCK) cl[i] = coords[i];
    __syncthreads();
    const float c0 = cl[0];
    const float delta = cl[1] - cl[0];
    const float inv_delta = 1.0f / delta;
    const int per_wg = BLOCK / CH;
    const int chunk = threadIdx.x % CH;
    const int64_t p = (int64_t)blockIdx.x * per_wg + threadIdx.x / CH;
    const bool valid = p < n;
    float xv[KDE_DMAX], gv[KDE_DMAX];
    load_row(x, valid ? p : 0, d, xv);
#pragma unroll
    for (int j = 0; j < KDE_DMAX; ++j) gv[j] = 0.0f;
    float gk = 0.0f;
    for (int p_begin = 0; p_begin < P; p_begin += Pg) {
        const int np = min(Pg, P - p_begin);
        __syncthreads();
        for (int i = threadIdx.x; i < np * B; i += BLOCK) img[i] = gS[(int64_t)p_begin * B + i];
        stage_vrows<BLOCK>(Vl, V, p_begin, np, d);
        __syncthreads();
        for (int q = chunk; q < np; q += CH) {
            float vq[KDE_DMAX];
            load_vrow(Vl, q, vq);
            const float u = project8(xv, vq);
            const int kc = centre_bin(u, c0, inv_delta, B, R);
            float du = 0.0f, dk = 0.0f;
            if (RT > 0 && kc >= RT && kc < B - RT) {
                // interior particle: the whole window inside the grid (see proj_kde1d_bwd_kernel)
                const float* cp = cl + (kc - RT);
                const float* gp = img + q * B + (kc - RT);
#pragma unroll
                for (int j = 0; j <= 2 * RT; ++j) {
                    const float r = (u - cp[j]) * inv_sigma;
                    du += gp[j] * gauss_weight(r) * (-r * inv_sigma);
                    dk += gp[j] * gauss_weight(r);
                }
            } else if (RT > 0) {
                // bins outside [0, B) read a clamped bin and are masked (NaN / inf rows: every term masked, exactly 0)
#pragma unroll
                for (int j = -RT; j <= RT; ++j) {
                    const int k = kc + j;
                    const int kk = min(max(k, 0), B - 1);
                    const float r = (u - cl[kk]) * inv_sigma;
                    const float term = img[q * B + kk] * gauss_weight(r) * (-r * inv_sigma);
                    const float kern = img[q * B + kk] * gauss_weight(r);
                    du += (k == kk) ? term : 0.0f;
                    dk += (k == kk) ? kern : 0.0f;
                }
            } else {
                for (int j = -R; j <= R; ++j) {
                    const int k = kc + j;
                    if (k >= 0 && k < B) {
                        const float r = (u - cl[k]) * inv_sigma;
                        du = fmaf(img[q * B + k] * gauss_weight(r), -r * inv_sigma, du);
                        dk = fmaf(img[q * B + k], gauss_weight(r), dk);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < KDE_DMAX; ++j) gv[j] = fmaf(du, vq[j], gv[j]);
            gk += dk;
        }
    }
    for (int m = 1; m < CH; m <<= 1) {
#pragma unroll
        for (int j = 0; j < KDE_DMAX; ++j) gv[j] += __shfl_xor(gv[j], m);
        gk += __shfl_xor(gk, m);
    }
    if (valid && chunk == 0) {
        const float wr = wt[p];
        const float wv = weight_or_zero(wr);
        if (gx) {
#pragma unroll
            for (int j = 0; j < KDE_DMAX; ++j)
                if (j < d) {
                    const float g = wv > 0.0f ? wv * gv[j] : 0.0f;          // select: an invalid weight never meets gv
                    gx[p * d + j] = accumulate ? gx[p * d + j] + g : g;
                }
        }
        if (gw) {
            const float g = weight_can_grow(wr) ? gk : 0.0f;
            gw[p] = accumulate ? gw[p] + g : g;
        }
    }
}

// ------------------------------------------------------------------------------------------------ 2-D forward
// grid, block, LDS and register budget as proj_kde2d_fwd_kernel.  The weight goes into the finished y window once per
// particle and projection (2 R + 1 multiplies), so that a cell costs the one multiply wx * wy it costs unweighted.
template <int RT, int BLOCK>
__global__ __launch_bounds__(BLOCK) MF_WAVES_PER_SIMD(8, 8) void proj_wkde2d_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ wmax_p, int64_t n, int d,
    const float* __restrict__ V0, const float* __restrict__ V1, int P, int Pg, const float* __restrict__ coords_x, int Bx,
    float inv_sx, int Rx, const float* __restrict__ coords_y, int By, float inv_sy, int Ry, u64* __restrict__ Sacc,
    int per_wg, int gshift) {
    MF_DYN_SMEM(u64, lds);
    const int BB = Bx * By;
    u64* img = lds;
    float* V0l = reinterpret_cast<float*>(img + (size_t)Pg * BB);
    float* V1l = V0l + Pg * KDE_VS;
    float* cxl = V1l + Pg * KDE_VS;
    float* cyl = cxl + Bx;
    const int p_begin = blockIdx.y * Pg;
    const int np = min(Pg, P - p_begin);
    for (int i = threadIdx.x; i < np * BB; i += BLOCK) img[i] = 0;
    stage_vrows<BLOCK>(V0l, V0, p_begin, np, d);
    stage_vrows<BLOCK>(V1l, V1, p_begin, np, d);
    for (int i = threadIdx.x; i < Bx; i += BLOCK) cxl[i] = coords_x[i];
    for (int i = threadIdx.x; i < By; i += BLOCK) cyl[i] = coords_y[i];
    __syncthreads();
    const float wmax = wmax_p[0];
    const float cx0 = cxl[0], dx = cxl[1] - cxl[0], inv_dx = 1.0f / dx, ssx = dx * inv_sx;
    const float cy0 = cyl[0], dy = cyl[1] - cyl[0], inv_dy = 1.0f / dy, ssy = dy * inv_sy;
    constexpr int RW = RT > 0 ? RT : 2;
    const bool fact_ok = RT > 0 && ssx >= 2.0f && ssx <= 2.6f && ssy >= 2.0f && ssy <= 2.6f;     // see proj_kde1d_fwd_kernel
    const GaussGamma<RW> gmx = gauss_gamma<RW>(fact_ok ? ssx : 2.0f), gmy = gauss_gamma<RW>(fact_ok ? ssy : 2.0f);
    const int64_t p_lo = (int64_t)blockIdx.x * per_wg;
    const int64_t p_hi = min(n, p_lo + per_wg);
    for (int64_t p = p_lo + threadIdx.x; p < p_hi; p += BLOCK) {
        const float wn = weight_ratio(wt[p], wmax);
        if (wn == 0.0f) continue;
        float xv[KDE_DMAX];
        load_row(x, p, d, xv);
        for (int q = 0; q < np; ++q) {
            float v0[KDE_DMAX], v1[KDE_DMAX];
            load_vrow(V0l, q, v0);
            load_vrow(V1l, q, v1);
            const float u0 = project8(xv, v0);
            const float u1 = project8(xv, v1);
            const int ka = centre_bin(u0, cx0, inv_dx, Bx, Rx);
            const int kb = centre_bin(u1, cy0, inv_dy, By, Ry);
            u64* im = img + (size_t)q * BB;
            if (fact_ok) {
                float wx[2 * RW + 1], wy[2 * RW + 1];
                gauss_window<RW>(u0, cxl, ka, Bx, inv_sx, ssx, gmx, wx);
                gauss_window<RW>(u1, cyl, kb, By, inv_sy, ssy, gmy, wy);
#pragma unroll
                for (int j = 0; j < 2 * RW + 1; ++j) wy[j] *= wn;
#pragma unroll
                for (int i = -RT; i <= RT; ++i) {
                    const int a = ka + i;
                    if (a < 0 || a >= Bx) continue;
                    u64* row = im + a * By;
#pragma unroll
                    for (int j = -RT; j <= RT; ++j) {
                        if (kde2d_dead_cell(i, j)) continue;
                        const int b = kb + j;
                        if (b >= 0 && b < By) {
                            const u64 f = to_fix(wx[i + RW] * wy[j + RW]);
                            if (f != 0) atomicAdd(&row[b], f);
                        }
                    }
                }
            } else {
                float wy[2 * KDE_RMAX2D + 1];
#pragma unroll
                for (int j = 0; j < 2 * KDE_RMAX2D + 1; ++j) {
                    const int b = kb - Ry + j;
                    float w = 0.0f;
                    if (j <= 2 * Ry && b >= 0 && b < By) w = wn * gauss_weight((u1 - cyl[b]) * inv_sy);
                    wy[j] = w;
                }
                for (int i = 0; i <= 2 * Rx; ++i) {
                    const int a = ka - Rx + i;
                    if (a < 0 || a >= Bx) continue;
                    const float wx = gauss_weight((u0 - cxl[a]) * inv_sx);
                    u64* row = im + a * By;
#pragma unroll
                    for (int j = 0; j < 2 * KDE_RMAX2D + 1; ++j) {
                        const int b = kb - Ry + j;
                        if (j <= 2 * Ry && b >= 0 && b < By) {
                            const u64 f = to_fix(wx * wy[j]);
                            if (f != 0) atomicAdd(&row[b], f);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < np * BB; i += BLOCK) fix_flush(Sacc + (int64_t)p_begin * BB + i, img[i], gshift);
}

// ------------------------------------------------------------------------------------------------ 2-D backward
// as proj_kde2d_bwd_kernel; dk collects sum_ab gS Kx Ky beside du0, du1
template <int RT, int BLOCK, int NPT>
__global__ __launch_bounds__(BLOCK) void proj_wkde2d_bwd_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, int64_t n, int d, const float* __restrict__ V0,
    const float* __restrict__ V1, int P, int Pg, const float* __restrict__ coords_x, int Bx, float inv_sx, int Rx,
    const float* __restrict__ coords_y, int By, float inv_sy, int Ry, const float* __restrict__ gS, float* __restrict__ gx,
    float* __restrict__ gw, int accumulate) {
    MF_DYN_SMEM(float, lds);
    const int BB = Bx * By;
    float* img = lds;
    float* V0l = img + Pg * BB;
    float* V1l = V0l + Pg * KDE_VS;
    float* cxl = V1l + Pg * KDE_VS;
    float* cyl = cxl + Bx;
    for (int i = threadIdx.x; i < Bx; i += BLOCK) cxl[i] = coords_x[i];
    for (int i = threadIdx.x; i < By; i += BLOCK) cyl[i] = coords_y[i];
    __syncthreads();
    const float cx0 = cxl[0], inv_dx = 1.0f / (cxl[1] - cxl[0]);
    const float cy0 = cyl[0], inv_dy = 1.0f / (cyl[1] - cyl[0]);
    constexpr int RW = RT > 0 ? RT : 1;
    const float ssx = (cxl[1] - cxl[0]) * inv_sx, ssy = (cyl[1] - cyl[0]) * inv_sy;
    const bool fact_ok = RT > 0 && ssx >= 2.0f && ssx <= 2.6f && ssy >= 2.0f && ssy <= 2.6f;
    const int64_t base = (int64_t)blockIdx.x * BLOCK * NPT + threadIdx.x;
    float xv[NPT][KDE_DMAX], gv[NPT][KDE_DMAX], gk[NPT];
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
        const int64_t p = base + (int64_t)t * BLOCK;
        load_row(x, p < n ? p : n - 1, d, xv[t]);
#pragma unroll
        for (int j = 0; j < KDE_DMAX; ++j) gv[t][j] = 0.0f;
        gk[t] = 0.0f;
    }
    for (int p_begin = 0; p_begin < P; p_begin += Pg) {
        const int np = min(Pg, P - p_begin);
        __syncthreads();
        for (int i = threadIdx.x; i < np * BB; i += BLOCK) img[i] = gS[(int64_t)p_begin * BB + i];
        stage_vrows<BLOCK>(V0l, V0, p_begin, np, d);
        stage_vrows<BLOCK>(V1l, V1, p_begin, np, d);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NPT; ++t) {
            for (int q = 0; q < np; ++q) {
                float v0[KDE_DMAX], v1[KDE_DMAX];
                load_vrow(V0l, q, v0);
                load_vrow(V1l, q, v1);
                const float u0 = project8(xv[t], v0);
                const float u1 = project8(xv[t], v1);
                const int ka = centre_bin(u0, cx0, inv_dx, Bx, Rx);
                const int kb = centre_bin(u1, cy0, inv_dy, By, Ry);
                const float* im = img + q * BB;
                float du0 = 0.0f, du1 = 0.0f, dk = 0.0f;
                if (fact_ok) {
                    // same cells as the forward (dead corners skipped); out-of-range bins read a clamped bin, masked
                    float wy[2 * RW + 1], dyw[2 * RW + 1];
                    int bidx[2 * RW + 1];
#pragma unroll
                    for (int j = -RT; j <= RT; ++j) {
                        const int b = kb + j;
                        const int bb = min(max(b, 0), By - 1);
                        const bool ok = b == bb;
                        const float r = (u1 - cyl[bb]) * inv_sy;
                        const float w = ok ? gauss_weight(r) : 0.0f;       // select, not multiply: NaN rows stay out
                        wy[j + RW] = w;
                        dyw[j + RW] = ok ? -r * inv_sy * w : 0.0f;
                        bidx[j + RW] = bb;
                    }
#pragma unroll
                    for (int i = -RT; i <= RT; ++i) {
                        const int a = ka + i;
                        const int aa = min(max(a, 0), Bx - 1);
                        const float* row = im + aa * By;
                        float sa = 0.0f, sb = 0.0f;
#pragma unroll
                        for (int j = -RT; j <= RT; ++j) {
                            if (kde2d_dead_cell(i, j)) continue;
                            const float g = row[bidx[j + RW]];
                            sa = fmaf(g, wy[j + RW], sa);
                            sb = fmaf(g, dyw[j + RW], sb);
                        }
                        const float r = (u0 - cxl[aa]) * inv_sx;
                        const float w = gauss_weight(r);
                        const float tx = -r * inv_sx * w * sa, ty = w * sb, tk = w * sa;
                        du0 += (a == aa) ? tx : 0.0f;
                        du1 += (a == aa) ? ty : 0.0f;
                        dk += (a == aa) ? tk : 0.0f;
                    }
                } else {
                    float wy[2 * KDE_RMAX2D + 1], dyv[2 * KDE_RMAX2D + 1];
#pragma unroll
                    for (int j = 0; j < 2 * KDE_RMAX2D + 1; ++j) {
                        const int b = kb - Ry + j;
                        float w = 0.0f, dw = 0.0f;
                        if (j <= 2 * Ry && b >= 0 && b < By) {
                            const float r = (u1 - cyl[b]) * inv_sy;
                            w = gauss_weight(r);
                            dw = -r * inv_sy * w;
                        }
                        wy[j] = w;
                        dyv[j] = dw;
                    }
                    for (int i = 0; i <= 2 * Rx; ++i) {
                        const int a = ka - Rx + i;
                        if (a < 0 || a >= Bx) continue;
                        const float r = (u0 - cxl[a]) * inv_sx;
                        const float wx = gauss_weight(r);
                        const float dwx = -r * inv_sx * wx;
                        const float* row = im + a * By;
                        float sa = 0.0f, sb = 0.0f;
#pragma unroll
                        for (int j = 0; j < 2 * KDE_RMAX2D + 1; ++j) {
                            const int b = kb - Ry + j;
                            if (j <= 2 * Ry && b >= 0 && b < By) {
                                const float g = row[b];
                                sa = fmaf(g, wy[j], sa);
                                sb = fmaf(g, dyv[j], sb);
                            }
                        }
                        du0 = fmaf(dwx, sa, du0);
                        du1 = fmaf(wx, sb, du1);
                        dk = fmaf(wx, sa, dk);
                    }
                }
#pragma unroll
                for (int j = 0; j < KDE_DMAX; ++j) gv[t][j] = fmaf(du0, v0[j], fmaf(du1, v1[j], gv[t][j]));
                gk[t] += dk;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NPT; ++t) {
        const int64_t p = base + (int64_t)t * BLOCK;
        if (p < n) {
            const float wr = wt[p];
            const float wv = weight_or_zero(wr);
            if (gx) {
#pragma unroll
                for (int j = 0; j < KDE_DMAX; ++j)
                    if (j < d) {
                        const float g = wv > 0.0f ? wv * gv[t][j] : 0.0f;
                        gx[p * d + j] = accumulate ? gx[p * d + j] + g : g;
                    }
            }
            if (gw) {
                const float g = weight_can_grow(wr) ? gk[t] : 0.0f;
                gw[p] = accumulate ? gw[p] + g : g;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ hard-binned weighted sums
// Bin search of proj_hist{1,2}d_kernel (edge_bin: out of range ignored, last bin right-inclusive); the sums are accumulated in
// the fixed point of the KDE forwards, so they too are exact and order independent, and weights 1 give the integer counts.
// grid (G, ngroups): workgroup (bx, by) takes particles [bx * per_wg, (bx + 1) * per_wg), per_wg <= 8192.
// LDS: [Pg*B] u64 image | [Pg*d] V | [B+1] edges
__global__ __launch_bounds__(KDE_BLOCK) void proj_whist1d_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ wmax_p, int64_t n, int d,
    const float* __restrict__ V, int P, int Pg, const float* __restrict__ edges, int B, u64* __restrict__ Sacc, int per_wg,
    int gshift) {
    MF_DYN_SMEM(u64, lds);
    u64* img = lds;
    float* Vl = reinterpret_cast<float*>(img + (size_t)Pg * B);
    float* el = Vl + Pg * d;
    const int p_begin = blockIdx.y * Pg;
    const int np = min(Pg, P - p_begin);
    for (int i = threadIdx.x; i < np * B; i += KDE_BLOCK) img[i] = 0;
    for (int i = threadIdx.x; i < np * d; i += KDE_BLOCK) Vl[i] = V[p_begin * d + i];
    for (int i = threadIdx.x; i <= B; i += KDE_BLOCK) el[i] = edges[i];
    __syncthreads();
    const float wmax = wmax_p[0];
    const float inv_delta = 1.0f / (el[1] - el[0]);
    const int64_t p_lo = (int64_t)blockIdx.x * per_wg;
    const int64_t p_hi = min(n, p_lo + per_wg);
    for (int64_t p = p_lo + threadIdx.x; p < p_hi; p += KDE_BLOCK) {
        const u64 f = to_fix(weight_ratio(wt[p], wmax));
        if (f == 0) continue;
        float xv[KDE_DMAX];
        load_row(x, p, d, xv);
        for (int q = 0; q < np; ++q) {
            const int k = edge_bin(project(xv, Vl + q * d, d), el, B, inv_delta);
            if (k >= 0) atomicAdd(&img[q * B + k], f);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < np * B; i += KDE_BLOCK) fix_flush(Sacc + (int64_t)p_begin * B + i, img[i], gshift);
}

// LDS: [Pg*Bx*By] u64 image | [Pg*d] V0 | [Pg*d] V1 | [Bx+1] edges_x | [By+1] edges_y
__global__ __launch_bounds__(KDE_BLOCK) void proj_whist2d_kernel(
    const float* __restrict__ x, const float* __restrict__ wt, const float* __restrict__ wmax_p, int64_t n, int d,
    const float* __restrict__ V0, const float* __restrict__ V1, int P, int Pg, const float* __restrict__ edges_x, int Bx,
    const float* __restrict__ edges_y, int By, u64* __restrict__ Sacc, int per_wg, int gshift) {
    MF_DYN_SMEM(u64, lds);
    const int BB = Bx * By;
    u64* img = lds;
    float* V0l = reinterpret_cast<float*>(img + (size_t)Pg * BB);
    float* V1l = V0l + Pg * d;
    float* exl = V1l + Pg * d;
    float* eyl = exl + Bx + 1;
    const int p_begin = blockIdx.y * Pg;
    const int np = min(Pg, P - p_begin);
    for (int i = threadIdx.x; i < np * BB; i += KDE_BLOCK) img[i] = 0;
    for (int i = threadIdx.x; i < np * d; i += KDE_BLOCK) {
        V0l[i] = V0[p_begin * d + i];
        V1l[i] = V1[p_begin * d + i];
    }
    for (int i = threadIdx.x; i <= Bx; i += KDE_BLOCK) exl[i] = edges_x[i];
    for (int i = threadIdx.x; i <= By; i += KDE_BLOCK) eyl[i] = edges_y[i];
    __syncthreads();
    const float wmax = wmax_p[0];
    const float inv_dx = 1.0f / (exl[1] - exl[0]);
    const float inv_dy = 1.0f / (eyl[1] - eyl[0]);
    const int64_t p_lo = (int64_t)blockIdx.x * per_wg;
    const int64_t p_hi = min(n, p_lo + per_wg);
    for (int64_t p = p_lo + threadIdx.x; p < p_hi; p += KDE_BLOCK) {
        const u64 f = to_fix(weight_ratio(wt[p], wmax));
        if (f == 0) continue;
        float xv[KDE_DMAX];
        load_row(x, p, d, xv);
        for (int q = 0; q < np; ++q) {
            const int a = edge_bin(project(xv, V0l + q * d, d), exl, Bx, inv_dx);
            const int b = edge_bin(project(xv, V1l + q * d, d), eyl, By, inv_dy);
            if (a >= 0 && b >= 0) atomicAdd(&img[q * BB + a * By + b], f);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < np * BB; i += KDE_BLOCK) fix_flush(Sacc + (int64_t)p_begin * BB + i, img[i], gshift);
}

}  // namespace mf

using namespace mf;

// ================================================================================================= C ABI
// What every weighted entry point checks, BEFORE the plan does any arithmetic on the sizes: the pointers it reads or writes and
// the sizes the kernels index with in int.
// (No ProfScope here: the per-kernel timers of mf_prof_enable / mf_prof_report have one slot per kind of common.h, whose order
// _lib.PROF_KERNELS mirrors, and the weighted launches must not be booked on the unweighted kernels' slots.  The weighted
// kernels are therefore not seen by mf_prof_report; tools/bench_wproj.py times them with device events.)
static int wproj_check(const char* who, const void* x, const void* w, int64_t n, int P, int64_t bins) {
    if (n > 0 && (!x || !w)) return fail("%s: x and w must be given for n > 0", who);
    if (P >= 1 && bins >= 1 && (int64_t)P * bins > 0x7fffffff) return fail("%s: P * bins = %lld exceeds 2^31 - 1", who, (long long)P * bins);
    return 0;
}
static int sigma_check(const char* who, float sigma) {
    if (!(sigma > 0.0f) || !(sigma <= WPROJ_FLT_MAX)) return fail("%s: sigma must be finite and positive (got %g)", who, (double)sigma);
    return 0;
}
static int radius2d_check(const char* who, int rx, int ry) {
    if (rx < 0 || ry < 0) return fail("%s: a truncation radius is >= 0 (got %d, %d)", who, rx, ry);
    return 0;
}

static int wfix_finish(const u64* Sacc, float* S, int64_t total, int shift, const float* wmax, void* stream) {
    MF_LAUNCH(wacc_to_float_kernel, grid_for(total, KDE_BLOCK, 1024), KDE_BLOCK, 0, stream, Sacc, S, total,
              KDE_FIX_INV * (double)((u64)1 << shift), wmax);
    return check_launch("wacc_to_float");
}

extern "C" int mf_proj_wkde1d_fwd(const float* x, const float* w, const float* wmax, int64_t n, int d, const float* V, int P,
                                   const float* coords, int B, float sigma, int radius, float* S, void* ws, void* stream) {
    KdePlan p;
    if (wproj_check("mf_proj_wkde1d_fwd", x, w, n, P, B) || sigma_check("mf_proj_wkde1d_fwd", sigma)) return 1;
    if (launch_plan(KDE1D_FWD, n, d, P, B, 1, radius, radius, p)) return 1;
    if (!wmax || !V || !coords || !S || !ws) return fail("mf_proj_wkde1d_fwd: wmax, V, coords, S and ws must be given");
    u64* Sfix = reinterpret_cast<u64*>(ws);
    if (hipMemsetAsync(Sfix, 0, sizeof(u64) * (size_t)P * B, (hipStream_t)stream) != hipSuccess) return fail("memset ws");
    if (n > 0) {
        pick_window_block(p, [&](auto RT, auto BL) {
            MF_ALLOW_DYN_SMEM((proj_wkde1d_fwd_kernel<RT, BL>), p.smem);
            MF_LAUNCH((proj_wkde1d_fwd_kernel<RT, BL>), dim3((unsigned)p.grid_x, p.groups), BL, p.smem, stream, x, w, wmax, n, d, V,
                      P, p.Pg, coords, B, 1.0f / sigma, kde_radius_1d(radius, B), Sfix, p.per_wg, p.shift);
        });
        if (check_launch("mf_proj_wkde1d_fwd")) return 1;
    }
    return wfix_finish(Sfix, S, (int64_t)P * B, p.shift, wmax, stream);
}

extern "C" int mf_proj_wkde1d_bwd(const float* x, const float* w, int64_t n, int d, const float* V, int P, const float* coords,
                                   int B, float sigma, int radius, const float* gS, float* gx, float* gw, int accumulate,
                                   void* stream) {
    KdePlan p;
    if (wproj_check("mf_proj_wkde1d_bwd", x, w, n, P, B) || sigma_check("mf_proj_wkde1d_bwd", sigma)) return 1;
    if (launch_plan(KDE1D_BWD, n, d, P, B, 1, radius, radius, p)) return 1;
    if (!V || !coords || !gS) return fail("mf_proj_wkde1d_bwd: V, coords and gS must be given");
    if (!gx && !gw) return fail("mf_proj_wkde1d_bwd: at least one of gx and gw must be given");
    if (n == 0) return 0;
    pick_window_block(p, [&](auto RT, auto BL) {
        MF_ALLOW_DYN_SMEM((proj_wkde1d_bwd_kernel<RT, BL>), p.smem);
        MF_LAUNCH((proj_wkde1d_bwd_kernel<RT, BL>), dim3((unsigned)p.grid_x), BL, p.smem, stream, x, w, n, d, V, P, p.Pg, coords, B,
                  1.0f / sigma, kde_radius_1d(radius, B), gS, gx, gw, accumulate, p.split);
    });
    return check_launch("mf_proj_wkde1d_bwd");
}

extern "C" int mf_proj_wkde2d_fwd(const float* x, const float* w, const float* wmax, int64_t n, int d, const float* V0,
                                   const float* V1, int P, const float* coords_x, int Bx, float sigma_x, int radius_x,
                                   const float* coords_y, int By, float sigma_y, int radius_y, float* S, void* ws,
                                   void* stream) {
    KdePlan p;
    if (wproj_check("mf_proj_wkde2d_fwd", x, w, n, P, (int64_t)Bx * By) || sigma_check("mf_proj_wkde2d_fwd", sigma_x) ||
        sigma_check("mf_proj_wkde2d_fwd", sigma_y) || radius2d_check("mf_proj_wkde2d_fwd", radius_x, radius_y))
        return 1;
    if (launch_plan(KDE2D_FWD, n, d, P, Bx, By, radius_x, radius_y, p)) return 1;
    if (!wmax || !V0 || !V1 || !coords_x || !coords_y || !S || !ws)
        return fail("mf_proj_wkde2d_fwd: wmax, V0, V1, coords_x, coords_y, S and ws must be given");
    u64* Sfix = reinterpret_cast<u64*>(ws);
    if (hipMemsetAsync(Sfix, 0, sizeof(u64) * (size_t)P * Bx * By, (hipStream_t)stream) != hipSuccess) return fail("memset ws");
    if (n > 0) {
        pick_window_block(p, [&](auto RT, auto BL) {
            MF_ALLOW_DYN_SMEM((proj_wkde2d_fwd_kernel<RT, BL>), p.smem);
            MF_LAUNCH((proj_wkde2d_fwd_kernel<RT, BL>), dim3((unsigned)p.grid_x, p.groups), BL, p.smem, stream, x, w, wmax, n, d, V0,
                      V1, P, p.Pg, coords_x, Bx, 1.0f / sigma_x, radius_x, coords_y, By, 1.0f / sigma_y, radius_y, Sfix, p.per_wg,
                      p.shift);
        });
        if (check_launch("mf_proj_wkde2d_fwd")) return 1;
    }
    return wfix_finish(Sfix, S, (int64_t)P * Bx * By, p.shift, wmax, stream);
}

extern "C" int mf_proj_wkde2d_bwd(const float* x, const float* w, int64_t n, int d, const float* V0, const float* V1, int P,
                                   const float* coords_x, int Bx, float sigma_x, int radius_x, const float* coords_y, int By,
                                   float sigma_y, int radius_y, const float* gS, float* gx, float* gw, int accumulate,
                                   void* stream) {
    KdePlan p;
    if (wproj_check("mf_proj_wkde2d_bwd", x, w, n, P, (int64_t)Bx * By) || sigma_check("mf_proj_wkde2d_bwd", sigma_x) ||
        sigma_check("mf_proj_wkde2d_bwd", sigma_y) || radius2d_check("mf_proj_wkde2d_bwd", radius_x, radius_y))
        return 1;
    if (launch_plan(KDE2D_BWD, n, d, P, Bx, By, radius_x, radius_y, p)) return 1;
    if (!V0 || !V1 || !coords_x || !coords_y || !gS) return fail("mf_proj_wkde2d_bwd: V0, V1, coords_x, coords_y and gS must be given");
    if (!gx && !gw) return fail("mf_proj_wkde2d_bwd: at least one of gx and gw must be given");
    if (n == 0) return 0;
    pick_window_block(p, [&](auto RT, auto BL) {
        pick<1, 2, 4>(p.split, [&](auto NP) {
            MF_ALLOW_DYN_SMEM((proj_wkde2d_bwd_kernel<RT, BL, NP>), p.smem);
            MF_LAUNCH((proj_wkde2d_bwd_kernel<RT, BL, NP>), dim3((unsigned)p.grid_x), BL, p.smem, stream, x, w, n, d, V0, V1, P,
                      p.Pg, coords_x, Bx, 1.0f / sigma_x, radius_x, coords_y, By, 1.0f / sigma_y, radius_y, gS, gx, gw, accumulate);
        });
    });
    return check_launch("mf_proj_wkde2d_bwd");
}

// geometry of the hard-binned sums: as many 64-bit images, with their projection vectors, as fit the 96 KiB of the counts
// kernels beside the edges; particles split over workgroups of at most KDE_MAX_PER_WG (fixed-point headroom) by the rule of
// the KDE forwards
static int whist_geometry(int64_t n, int P, int64_t bins, int per_proj_floats, int fixed_floats, int* Pg, int* groups,
                          int* per_wg, size_t* smem) {
    const size_t budget = sizeof(float) * KDE_LDS_FLOATS, fixed = sizeof(float) * (size_t)fixed_floats;
    const size_t per_proj = sizeof(u64) * (size_t)bins + sizeof(float) * (size_t)per_proj_floats;
    if (fixed + per_proj > budget) return fail("histogram image of %lld bins exceeds the LDS budget", (long long)bins);
    size_t g = (budget - fixed) / per_proj;
    if (g > (size_t)P) g = (size_t)P;
    *Pg = (int)g;
    *groups = (P + *Pg - 1) / *Pg;
    *per_wg = kde_per_wg(n, *groups, KDE_BLOCK, 4);
    *smem = per_proj * g + fixed;
    return 0;
}

extern "C" int mf_proj_whist1d_sums(const float* x, const float* w, const float* wmax, int64_t n, int d, const float* V, int P,
                                     const float* edges, int B, float* sums, void* ws, void* stream) {
    if (wproj_check("mf_proj_whist1d_sums", x, w, n, P, B) || kde_check(n, d, P, B)) return 1;
    if (!wmax || !V || !edges || !sums || !ws) return fail("mf_proj_whist1d_sums: wmax, V, edges, sums and ws must be given");
    int Pg, groups, per_wg;
    size_t smem;
    if (whist_geometry(n, P, B, d, B + 1, &Pg, &groups, &per_wg, &smem)) return 1;
    u64* Sfix = reinterpret_cast<u64*>(ws);
    if (hipMemsetAsync(Sfix, 0, sizeof(u64) * (size_t)P * B, (hipStream_t)stream) != hipSuccess) return fail("memset ws");
    const int shift = kde_global_shift(n);
    if (n > 0) {
        MF_ALLOW_DYN_SMEM(proj_whist1d_kernel, smem);
        MF_LAUNCH(proj_whist1d_kernel, dim3((unsigned)((n + per_wg - 1) / per_wg), groups), KDE_BLOCK, smem, stream, x, w, wmax, n,
                  d, V, P, Pg, edges, B, Sfix, per_wg, shift);
        if (check_launch("mf_proj_whist1d_sums")) return 1;
    }
    return wfix_finish(Sfix, sums, (int64_t)P * B, shift, wmax, stream);
}

extern "C" int mf_proj_whist2d_sums(const float* x, const float* w, const float* wmax, int64_t n, int d, const float* V0,
                                     const float* V1, int P, const float* edges_x, int Bx, const float* edges_y, int By,
                                     float* sums, void* ws, void* stream) {
    if (wproj_check("mf_proj_whist2d_sums", x, w, n, P, (int64_t)Bx * By) || kde_check(n, d, P, Bx) || kde_check(n, d, P, By))
        return 1;
    if (!wmax || !V0 || !V1 || !edges_x || !edges_y || !sums || !ws)
        return fail("mf_proj_whist2d_sums: wmax, V0, V1, edges_x, edges_y, sums and ws must be given");
    int Pg, groups, per_wg;
    size_t smem;
    if (whist_geometry(n, P, (int64_t)Bx * By, 2 * d, Bx + By + 2, &Pg, &groups, &per_wg, &smem)) return 1;
    u64* Sfix = reinterpret_cast<u64*>(ws);
    if (hipMemsetAsync(Sfix, 0, sizeof(u64) * (size_t)P * Bx * By, (hipStream_t)stream) != hipSuccess) return fail("memset ws");
    const int shift = kde_global_shift(n);
    if (n > 0) {
        MF_ALLOW_DYN_SMEM(proj_whist2d_kernel, smem);
        MF_LAUNCH(proj_whist2d_kernel, dim3((unsigned)((n + per_wg - 1) / per_wg), groups), KDE_BLOCK, smem, stream, x, w, wmax, n,
                  d, V0, V1, P, Pg, edges_x, Bx, edges_y, By, Sfix, per_wg, shift);
        if (check_launch("mf_proj_whist2d_sums")) return 1;
    }
    return wfix_finish(Sfix, sums, (int64_t)P * Bx * By, shift, wmax, stream);
}
