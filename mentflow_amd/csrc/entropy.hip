// Sample-based entropy estimators on gfx950: the Kozachenko-Leonenko k-nearest-neighbour estimate and the covariance
// (Gaussian-volume) estimate, both with their adjoints in x.
//
// Reference chain replaced (paths relative to austin-hoover/ment-flow):
//   KNNEntropyEstimator(prior=None, k=5)           mentflow/entropy.py:41-50  (declared there, forward not implemented)
//   CovarianceEntropyEstimator(prior=None, pad)    mentflow/entropy.py:27-38  (torch.cov + torch.det on the samples)
//
// kNN:  H = -[psi(N) - psi(k) + ln c_d + (d / N) sum_i ln rho_k(i)],  c_d = pi^(d/2) / Gamma(d/2 + 1),  rho_k(i) the Euclidean
// distance of x_i to its k-th nearest OTHER point of the batch.  Rules that make the result unique:
//   * rho^2 = sum_c (x_ic - x_jc)^2 from direct differences in fp32, c ascending, one fma per term (never the Gram form);
//   * neighbours are ordered by (rho^2, index); candidates are always met in ascending index order, so a strict `<` on rho^2
//     implements that order however the candidate range is cut into chunks;
//   * ln rho = 0.5 ln max(rho^2, FLT_MIN), the logarithm taken in fp64; a floored term has zero gradient;
//   * a candidate at a NaN or infinite squared distance is never a neighbour.  A point with fewer than k candidates at finite
//     distance gets rho^2 = +inf and itself as the neighbour: H is then non-finite, every index stays inside [0, N).
//
// Kernels
//   knn_partial_kernel<DP, KL>  one query per lane in registers, workgroup (q, c) scans candidate chunk c for 256 queries:
//                               tiles of 256 candidates staged in LDS and read at the same address by every lane (broadcast),
//                               four candidates per step, a KL-entry sorted (rho^2, index) list per lane updated by selects
//                               behind one `min of four < entry k` test.  DP >= d is the padded feature count (zero columns add
//                               exact zeros), KL >= k the list length: both are template parameters so that the point and the
//                               list stay in registers (no scratch memory: the kernel states a register budget of 128 VGPRs,
//                               four waves per SIMD).
//   knn_merge_kernel<KL>        merges the chunks' lists per query in chunk order, takes entry k, writes idx / rho2 and the
//                               workgroup's fp64 sum of ln rho (fixed-shape tree).
//   knn_finish_kernel           one workgroup: the workgroup sums in a fixed order, then H.
//   knn_bwd_kernel<DP>          one point per lane: its own term, then a pass over idx[] (LDS tiles of index, weight and
//                               coordinates, ascending i') that adds the terms of the points whose k-th neighbour it is.  No
//                               atomics of any kind.
//   cov_moments_kernel          workgroup (g, a): fp64 partials of sum x_a and sum x_a x_b, b >= a (products of two fp32 are
//                               exact in fp64).
//   cov_tail_kernel             one workgroup: partials in a fixed order, then covariance, determinant and inverse by
//                               Gauss-Jordan elimination with partial pivoting in fp64 (d <= 16), H and the row-scaling
//                               matrix of the adjoint.  No host synchronisation.
//   cov_bwd_kernel              gx[n] = g * A (x_n - mu) in fp64, rounded once.
//
// Determinism: no float atomics; every sum has a fixed order, so every output is bitwise reproducible, and idx / rho2 do not
// depend on the number of candidate chunks.
#include <float.h>
#include <math.h>

#include "common.h"

namespace mf {

constexpr int ENT_DMAX = 16;                // the flow kernels' feature limit
constexpr int ENT_KMAX = 16;
constexpr int ENT_BLOCK = 256;              // queries per workgroup
constexpr int ENT_TILE = 256;               // candidates per LDS tile (16 KiB at DP = 16)
constexpr int ENT_CHUNK_MIN = 1024;         // fewest candidates worth a workgroup of their own
constexpr int ENT_BWD_BLOCK = 128;          // 196 workgroups at 25 000 points
constexpr int ENT_BWD_TILE = 256;           // points per LDS tile of the backward (18 KiB at DP = 16)
constexpr int COV_GMAX = 64;                // workgroups per moment row
constexpr int COV_STRIDE = ENT_DMAX + 1;    // sum x_a, then sum x_a x_b for b = 0..15
constexpr int ENT_NO_IDX = 0x7FFFFFFF;

// sorted insert of (r, j) into the ascending list; equal r keeps the entries already present in front (they have the lower
// index).  Selects only: a candidate that does not qualify (r >= worst, or NaN) changes nothing.
template <int KL>
__device__ __forceinline__ void knn_insert(float (&lr)[KL], int (&li)[KL], float r, int j) {
#pragma unroll
    for (int s = KL - 1; s > 0; --s) {
        const bool up = r < lr[s - 1];
        const bool here = r < lr[s];
        li[s] = up ? li[s - 1] : (here ? j : li[s]);
        lr[s] = up ? lr[s - 1] : (here ? r : lr[s]);
    }
    const bool first = r < lr[0];
    li[0] = first ? j : li[0];
    lr[0] = first ? r : lr[0];
}

template <int DP>
__device__ __forceinline__ float dist2(const float (&q)[DP], const float* __restrict__ cp) {
    float a = 0.0f;
#pragma unroll
    for (int c = 0; c < DP; ++c) {
        const float t = q[c] - cp[c];
        a = fmaf(t, t, a);
    }
    return a;
}

// entry k of the list (k is uniform): the bar a candidate has to pass
template <int KL>
__device__ __forceinline__ float knn_bar(const float (&lr)[KL], int k) {
    float t = lr[KL - 1];
#pragma unroll
    for (int s = 0; s < KL - 1; ++s) t = (s == k - 1) ? lr[s] : t;
    return t;
}

// SELF: the tile may hold the lane's own point, which is no candidate.  Only the first k entries of the list are the chunk's k
// nearest: a candidate enters only if it beats entry k, so what falls beyond entry k is never looked at again.
template <int DP, int KL, bool SELF>
__device__ __forceinline__ void knn_scan_tile(const float (&q)[DP], const float* __restrict__ s, int cnt, int j0, int self, int k,
                                              float (&lr)[KL], int (&li)[KL], float& bar) {
    for (int jj = 0; jj < cnt; jj += 4) {            // the tile is padded to a multiple of four with +inf candidates
        float r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            r[u] = dist2<DP>(q, s + (jj + u) * DP);
            if (SELF) r[u] = (j0 + jj + u == self) ? INFINITY : r[u];
        }
        const float m = fminf(fminf(r[0], r[1]), fminf(r[2], r[3]));      // fminf drops NaN
        if (m < bar) {                               // rare once the list has settled: the wave skips all four inserts
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (r[u] < bar) {
                    knn_insert<KL>(lr, li, r[u], j0 + jj + u);
                    bar = knn_bar<KL>(lr, k);
                }
            }
        }
    }
}

// part_r2 / part_idx: [chunk][k][n]
template <int DP, int KL>
__global__ __launch_bounds__(ENT_BLOCK) MF_WAVES_PER_SIMD(1, 4) void knn_partial_kernel(const float* __restrict__ x, int n, int d,
                                                                                        int k, int chunk_len,
                                                                                        float* __restrict__ part_r2,
                                                                                        int* __restrict__ part_idx) {
    __shared__ __attribute__((aligned(16))) float s[ENT_TILE * DP];
    const int q0 = (int)blockIdx.x * ENT_BLOCK;
    const int i = q0 + (int)threadIdx.x;
    const bool valid = i < n;
    float q[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) q[c] = (valid && c < d) ? x[(int64_t)i * d + c] : 0.0f;
    float lr[KL];
    int li[KL];
#pragma unroll
    for (int t = 0; t < KL; ++t) {
        lr[t] = INFINITY;
        li[t] = ENT_NO_IDX;
    }
    float bar = INFINITY;
    const int j_begin = (int)min((int64_t)blockIdx.y * chunk_len, (int64_t)n);
    const int j_end = (int)min((int64_t)j_begin + chunk_len, (int64_t)n);
    for (int t0 = j_begin; t0 < j_end; t0 += ENT_TILE) {
        const int cnt = min(ENT_TILE, j_end - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < ENT_TILE * DP; e += ENT_BLOCK) {
            const int jj = e / DP, c = e % DP;
            s[e] = jj < cnt ? (c < d ? x[(int64_t)(t0 + jj) * d + c] : 0.0f) : (c == 0 ? INFINITY : 0.0f);
        }
        __syncthreads();
        if (t0 < q0 + ENT_BLOCK && t0 + ENT_TILE > q0)       // workgroup-uniform
            knn_scan_tile<DP, KL, true>(q, s, cnt, t0, i, k, lr, li, bar);
        else
            knn_scan_tile<DP, KL, false>(q, s, cnt, t0, i, k, lr, li, bar);
    }
    if (valid) {
#pragma unroll
        for (int t = 0; t < KL; ++t) {
            if (t < k) {
                const int64_t o = ((int64_t)blockIdx.y * k + t) * n + i;
                part_r2[o] = lr[t];
                part_idx[o] = li[t];
            }
        }
    }
}

// fixed-shape tree over the workgroup; every thread has to call it
template <int B>
__device__ __forceinline__ double ent_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = B / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

template <int KL>
__global__ __launch_bounds__(ENT_BLOCK) void knn_merge_kernel(const float* __restrict__ part_r2, const int* __restrict__ part_idx,
                                                              int n, int k, int nchunks, int* __restrict__ idx,
                                                              float* __restrict__ rho2, double* __restrict__ block_sums) {
    __shared__ double red[ENT_BLOCK];
    const int i = (int)blockIdx.x * ENT_BLOCK + (int)threadIdx.x;
    double term = 0.0;
    if (i < n) {
        float lr[KL];
        int li[KL];
#pragma unroll
        for (int t = 0; t < KL; ++t) {
            lr[t] = INFINITY;
            li[t] = ENT_NO_IDX;
        }
        for (int c = 0; c < nchunks; ++c) {          // ascending chunks = ascending candidate indices
#pragma unroll
            for (int t = 0; t < KL; ++t) {
                if (t < k) {                         // a chunk's list is its k nearest, no more
                    const int64_t o = ((int64_t)c * k + t) * n + i;
                    knn_insert<KL>(lr, li, part_r2[o], part_idx[o]);
                }
            }
        }
        float rk = INFINITY;
        int ik = ENT_NO_IDX;
#pragma unroll
        for (int t = 0; t < KL; ++t) {
            rk = (t == k - 1) ? lr[t] : rk;
            ik = (t == k - 1) ? li[t] : ik;
        }
        if (ik < 0 || ik >= n) {                     // fewer than k candidates at finite distance
            ik = i;
            rk = INFINITY;
        }
        idx[i] = ik;
        rho2[i] = rk;
        term = 0.5 * log((double)fmaxf(rk, FLT_MIN));
    }
    const double tot = ent_block_sum<ENT_BLOCK>(term, red);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = tot;
}

// H = c0 + c1 * S
__global__ __launch_bounds__(ENT_BLOCK) void knn_finish_kernel(const double* __restrict__ block_sums, int nblocks, double c0,
                                                               double c1, float* __restrict__ H, double* __restrict__ S) {
    __shared__ double red[ENT_BLOCK];
    double t = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += ENT_BLOCK) t += block_sums[b];
    const double tot = ent_block_sum<ENT_BLOCK>(t, red);
    if (threadIdx.x == 0) {
        *S = tot;
        *H = (float)(c0 + c1 * tot);
    }
}

__device__ __forceinline__ float knn_weight(float r2) { return (r2 > FLT_MIN && r2 < INFINITY) ? 1.0f / r2 : 0.0f; }

// Tiles of ENT_BWD_TILE points (index of the k-th neighbour, weight, coordinates) are staged in LDS; a lane compares four
// neighbour indices per step with its own and, on the rare match, takes the term's operands from LDS as well.
template <int DP>
__global__ __launch_bounds__(ENT_BWD_BLOCK) void knn_bwd_kernel(const float* __restrict__ x, int n, int d,
                                                                const int* __restrict__ idx, const float* __restrict__ rho2,
                                                                const float* __restrict__ coef, float cscale,
                                                                float* __restrict__ gx) {
    __shared__ __attribute__((aligned(16))) int sidx[ENT_BWD_TILE];
    __shared__ float sw[ENT_BWD_TILE];
    __shared__ __attribute__((aligned(16))) float sx[ENT_BWD_TILE * DP];
    const int i = (int)blockIdx.x * ENT_BWD_BLOCK + (int)threadIdx.x;
    const bool valid = i < n;
    const int me = valid ? i : -2;                   // matches no entry of idx[] and no padding
    float q[DP], acc[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) {
        q[c] = (valid && c < d) ? x[(int64_t)i * d + c] : 0.0f;
        acc[c] = 0.0f;
    }
    if (valid) {
        int j = idx[i];
        if (j < 0 || j >= n) j = i;
        const float w = knn_weight(rho2[i]);
#pragma unroll
        for (int c = 0; c < DP; ++c)
            if (c < d) acc[c] = w * (q[c] - x[(int64_t)j * d + c]);
    }
    for (int t0 = 0; t0 < n; t0 += ENT_BWD_TILE) {
        const int cnt = min(ENT_BWD_TILE, n - t0);
        __syncthreads();
        for (int e = threadIdx.x; e < ENT_BWD_TILE; e += ENT_BWD_BLOCK) {
            sidx[e] = e < cnt ? idx[t0 + e] : -1;
            sw[e] = e < cnt ? knn_weight(rho2[t0 + e]) : 0.0f;
        }
        for (int e = threadIdx.x; e < ENT_BWD_TILE * DP; e += ENT_BWD_BLOCK) {
            const int jj = e / DP, c = e % DP;
            sx[e] = (jj < cnt && c < d) ? x[(int64_t)(t0 + jj) * d + c] : 0.0f;
        }
        __syncthreads();
        for (int jj = 0; jj < cnt; jj += 4) {
            int v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = sidx[jj + u];
            if (v[0] == me || v[1] == me || v[2] == me || v[3] == me) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (v[u] == me) {                 // ascending i': a fixed order of the row's terms
                        const float w = sw[jj + u];
                        const float* xp = sx + (jj + u) * DP;
#pragma unroll
                        for (int c = 0; c < DP; ++c) acc[c] = fmaf(w, q[c] - xp[c], acc[c]);
                    }
                }
            }
        }
    }
    if (valid) {
        const float g = coef[0] * cscale;
#pragma unroll
        for (int c = 0; c < DP; ++c)
            if (c < d) gx[(int64_t)i * d + c] = g * acc[c];
    }
}

// ------------------------------------------------------------------------------------------------ covariance estimator
// partial[(g * d + a) * COV_STRIDE + 0] = sum x_a,  [.. + 1 + b] = sum x_a x_b for b >= a, over the rows of workgroup g
__global__ __launch_bounds__(ENT_BLOCK) void cov_moments_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                double* __restrict__ partial) {
    __shared__ double red[ENT_BLOCK];
    const int a = blockIdx.y;
    double sa = 0.0, sab[ENT_DMAX];
#pragma unroll
    for (int b = 0; b < ENT_DMAX; ++b) sab[b] = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * ENT_BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * ENT_BLOCK) {
        const double xa = (double)x[p * d + a];
        sa += xa;
#pragma unroll
        for (int b = 0; b < ENT_DMAX; ++b)
            if (b >= a && b < d) sab[b] += xa * (double)x[p * d + b];
    }
    double* out = partial + ((int64_t)blockIdx.x * d + a) * COV_STRIDE;
    const double ta = ent_block_sum<ENT_BLOCK>(sa, red);
    if (threadIdx.x == 0) out[0] = ta;
#pragma unroll
    for (int b = 0; b < ENT_DMAX; ++b) {
        if (b >= a && b < d) {                       // workgroup-uniform
            const double tb = ent_block_sum<ENT_BLOCK>(sab[b], red);
            if (threadIdx.x == 0) out[1 + b] = tb;
        }
    }
}

// aux = [mu[d], A[d][d]] with A = -eps / (eps + pad) / (N - 1) * C^-1; a singular C (zero pivot) gives det = 0 and A = 0
__global__ __launch_bounds__(ENT_BLOCK) void cov_tail_kernel(const double* __restrict__ partial, int G, int64_t n, int d,
                                                             double pad, float* __restrict__ H, double* __restrict__ aux) {
    __shared__ double mom[ENT_DMAX * COV_STRIDE];
    __shared__ double aug[ENT_DMAX][2 * ENT_DMAX];
    for (int e = threadIdx.x; e < d * COV_STRIDE; e += ENT_BLOCK) {
        const int a = e / COV_STRIDE, r = e % COV_STRIDE;
        double t = 0.0;
        if (r == 0 || (r - 1 >= a && r - 1 < d))
            for (int g = 0; g < G; ++g) t += partial[((int64_t)g * d + a) * COV_STRIDE + r];
        mom[e] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double N = (double)n;
    bool finite = true;
    for (int a = 0; a < d; ++a)
        for (int b = a; b < d; ++b) {
            const double c = (mom[a * COV_STRIDE + 1 + b] - mom[a * COV_STRIDE] * mom[b * COV_STRIDE] / N) / (N - 1.0);
            aug[a][b] = aug[b][a] = c;
            finite = finite && fabs(c) < (double)INFINITY;
        }
    for (int a = 0; a < d; ++a)
        for (int b = 0; b < d; ++b) aug[a][d + b] = a == b ? 1.0 : 0.0;
    double det = finite ? 1.0 : (double)NAN;     // a NaN / inf coordinate: H is NaN whatever the elimination would meet first
    for (int col = 0; col < d && finite; ++col) {
        int piv = col;
        for (int r = col + 1; r < d; ++r)
            if (fabs(aug[r][col]) > fabs(aug[piv][col])) piv = r;
        if (piv != col) {
            for (int c = 0; c < 2 * d; ++c) {
                const double t = aug[col][c];
                aug[col][c] = aug[piv][c];
                aug[piv][c] = t;
            }
            det = -det;
        }
        const double p = aug[col][col];
        det *= p;
        if (p == 0.0 || p != p) break;
        const double ip = 1.0 / p;
        for (int c = 0; c < 2 * d; ++c) aug[col][c] *= ip;
        for (int r = 0; r < d; ++r) {
            if (r == col) continue;
            const double f = aug[r][col];
            for (int c = 0; c < 2 * d; ++c) aug[r][c] -= f * aug[col][c];
        }
    }
    const double eps = sqrt(det);                    // NaN for a negative determinant, as in the reference
    *H = (float)(-3.0 * log(2.0 * M_PI * M_E) - log(eps + pad));
    const double f = (det > 0.0 && det < (double)INFINITY) ? -eps / (eps + pad) / (N - 1.0) : 0.0;
    for (int a = 0; a < d; ++a) aux[a] = mom[a * COV_STRIDE] / N;
    for (int a = 0; a < d; ++a)
        for (int b = 0; b < d; ++b) aux[d + a * d + b] = f != 0.0 ? f * aug[a][d + b] : 0.0;
}

__global__ __launch_bounds__(ENT_BLOCK) void cov_bwd_kernel(const float* __restrict__ x, int64_t n, int d,
                                                            const double* __restrict__ aux, const float* __restrict__ coef,
                                                            float* __restrict__ gx) {
    __shared__ double sa[ENT_DMAX + ENT_DMAX * ENT_DMAX];
    for (int e = threadIdx.x; e < d + d * d; e += ENT_BLOCK) sa[e] = aux[e];
    __syncthreads();
    const double g = (double)coef[0];
    for (int64_t p = (int64_t)blockIdx.x * ENT_BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * ENT_BLOCK) {
        double t[ENT_DMAX];
#pragma unroll
        for (int b = 0; b < ENT_DMAX; ++b) t[b] = b < d ? (double)x[p * d + b] - sa[b] : 0.0;
        for (int a = 0; a < d; ++a) {
            double acc = 0.0;
#pragma unroll
            for (int b = 0; b < ENT_DMAX; ++b)
                if (b < d) acc = fma(sa[d + a * d + b], t[b], acc);
            gx[p * d + a] = (float)(g * acc);
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
struct KnnPlan {
    int kl;              // list length: 1, 4, 8 or 16
    int dp;              // padded feature count: 2, 4, 6, 8, 12 or 16
    int qblocks;
    int chunk_len, nchunks;
};

static int knn_check(const char* who, int64_t n, int d, int k) {
    if (k < 1 || k > ENT_KMAX) return fail("%s supports 1 <= k <= %d neighbours (got %d)", who, ENT_KMAX, k);
    if (d < 1 || d > ENT_DMAX) return fail("%s supports 1 <= ndim <= %d (got %d)", who, ENT_DMAX, d);
    if (n <= k) return fail("%s needs more points than neighbours: N > k (got N = %lld, k = %d)", who, (long long)n, k);
    if (n >= ((int64_t)1 << 31) / (2 * ENT_DMAX)) return fail("%s: %lld points are too many", who, (long long)n);
    return 0;
}

// chunks = 0: as many candidate chunks as fill the GPU (about 8 workgroups per CU), none shorter than ENT_CHUNK_MIN
static int knn_plan(const char* who, int64_t n, int d, int k, int chunks, KnnPlan* p) {
    if (knn_check(who, n, d, k)) return 1;
    if (chunks < 0 || chunks > 65535) return fail("%s: the chunk override must be 0 (default) or 1..65535 (got %d)", who, chunks);
    p->kl = k == 1 ? 1 : (k <= 4 ? 4 : (k <= 8 ? 8 : 16));
    p->dp = d <= 2 ? 2 : (d <= 4 ? 4 : (d <= 6 ? 6 : (d <= 8 ? 8 : (d <= 12 ? 12 : 16))));
    p->qblocks = (int)((n + ENT_BLOCK - 1) / ENT_BLOCK);
    int64_t want = chunks;
    if (want == 0) {
        want = (NUM_CU * 8 + p->qblocks - 1) / p->qblocks;
        const int64_t most = n / ENT_CHUNK_MIN;
        if (want > most) want = most;
    }
    if (want < 1) want = 1;
    if (want > n) want = n;
    p->chunk_len = (int)((n + want - 1) / want);
    p->nchunks = (int)((n + p->chunk_len - 1) / p->chunk_len);
    return 0;
}

// psi at a positive integer: the harmonic sum below 16, the asymptotic series (error < 1e-14) from there on
static double digamma_int(int64_t n) {
    if (n < 16) {
        double s = -0.57721566490153286061;
        for (int64_t m = 1; m < n; ++m) s += 1.0 / (double)m;
        return s;
    }
    const double x = (double)n, x2 = 1.0 / (x * x);
    return log(x) - 0.5 / x - x2 * (1.0 / 12.0 - x2 * (1.0 / 120.0 - x2 * (1.0 / 252.0 - x2 / 240.0)));
}

template <int DP>
static void launch_knn_partial(const KnnPlan& p, const float* x, int n, int d, int k, float* pr, int* pi, void* stream) {
    const dim3 grid((unsigned)p.qblocks, (unsigned)p.nchunks);
    switch (p.kl) {
        case 1: MF_LAUNCH((knn_partial_kernel<DP, 1>), grid, ENT_BLOCK, 0, stream, x, n, d, k, p.chunk_len, pr, pi); break;
        case 4: MF_LAUNCH((knn_partial_kernel<DP, 4>), grid, ENT_BLOCK, 0, stream, x, n, d, k, p.chunk_len, pr, pi); break;
        case 8: MF_LAUNCH((knn_partial_kernel<DP, 8>), grid, ENT_BLOCK, 0, stream, x, n, d, k, p.chunk_len, pr, pi); break;
        default: MF_LAUNCH((knn_partial_kernel<DP, 16>), grid, ENT_BLOCK, 0, stream, x, n, d, k, p.chunk_len, pr, pi); break;
    }
}

}  // namespace mf

using namespace mf;

// ================================================================================================= C ABI
extern "C" int64_t mf_knn_entropy_ws_bytes(int64_t n, int d, int k, int chunks) {
    KnnPlan p;
    if (knn_plan("mf_knn_entropy_ws_bytes", n, d, k, chunks, &p)) return -1;
    return 8 * (int64_t)p.qblocks + 8 * (int64_t)p.nchunks * k * n;
}

extern "C" int mf_knn_entropy_fwd(const float* x, int64_t n, int d, int k, int chunks, float* H, double* sum_ln_rho,
                                  int32_t* idx, float* rho2, void* ws, void* stream) {
    KnnPlan p;
    if (knn_plan("mf_knn_entropy_fwd", n, d, k, chunks, &p)) return 1;
    if (ws == nullptr) return fail("mf_knn_entropy_fwd: the workspace is missing");
    double* block_sums = reinterpret_cast<double*>(ws);
    float* pr = reinterpret_cast<float*>(block_sums + p.qblocks);
    int* pi = reinterpret_cast<int*>(pr + (int64_t)p.nchunks * k * n);
    const int ni = (int)n;
    switch (p.dp) {
        case 2: launch_knn_partial<2>(p, x, ni, d, k, pr, pi, stream); break;
        case 4: launch_knn_partial<4>(p, x, ni, d, k, pr, pi, stream); break;
        case 6: launch_knn_partial<6>(p, x, ni, d, k, pr, pi, stream); break;
        case 8: launch_knn_partial<8>(p, x, ni, d, k, pr, pi, stream); break;
        case 12: launch_knn_partial<12>(p, x, ni, d, k, pr, pi, stream); break;
        default: launch_knn_partial<16>(p, x, ni, d, k, pr, pi, stream); break;
    }
    if (check_launch("mf_knn_entropy_fwd (search)")) return 1;
    const float* cpr = pr;
    const int* cpi = pi;
    switch (p.kl) {
        case 1: MF_LAUNCH(knn_merge_kernel<1>, p.qblocks, ENT_BLOCK, 0, stream, cpr, cpi, ni, k, p.nchunks, idx, rho2, block_sums); break;
        case 4: MF_LAUNCH(knn_merge_kernel<4>, p.qblocks, ENT_BLOCK, 0, stream, cpr, cpi, ni, k, p.nchunks, idx, rho2, block_sums); break;
        case 8: MF_LAUNCH(knn_merge_kernel<8>, p.qblocks, ENT_BLOCK, 0, stream, cpr, cpi, ni, k, p.nchunks, idx, rho2, block_sums); break;
        default: MF_LAUNCH(knn_merge_kernel<16>, p.qblocks, ENT_BLOCK, 0, stream, cpr, cpi, ni, k, p.nchunks, idx, rho2, block_sums); break;
    }
    if (check_launch("mf_knn_entropy_fwd (merge)")) return 1;
    // H = -[psi(N) - psi(k) + ln c_d] - (d / N) S
    const double ln_cd = 0.5 * d * log(M_PI) - lgamma(0.5 * d + 1.0);
    const double c0 = -(digamma_int(n) - digamma_int(k) + ln_cd);
    const double c1 = -(double)d / (double)n;
    MF_LAUNCH(knn_finish_kernel, 1, ENT_BLOCK, 0, stream, (const double*)block_sums, p.qblocks, c0, c1, H, sum_ln_rho);
    return check_launch("mf_knn_entropy_fwd (finish)");
}

extern "C" int mf_knn_entropy_bwd(const float* x, int64_t n, int d, const int32_t* idx, const float* rho2, const float* coef,
                                  float cscale, float* gx, void* stream) {
    if (knn_check("mf_knn_entropy_bwd", n, d, 1)) return 1;
    const int ni = (int)n;
    const int blocks = (int)((n + ENT_BWD_BLOCK - 1) / ENT_BWD_BLOCK);
    const int dp = d <= 2 ? 2 : (d <= 4 ? 4 : (d <= 6 ? 6 : (d <= 8 ? 8 : (d <= 12 ? 12 : 16))));
    switch (dp) {
        case 2: MF_LAUNCH(knn_bwd_kernel<2>, blocks, ENT_BWD_BLOCK, 0, stream, x, ni, d, idx, rho2, coef, cscale, gx); break;
        case 4: MF_LAUNCH(knn_bwd_kernel<4>, blocks, ENT_BWD_BLOCK, 0, stream, x, ni, d, idx, rho2, coef, cscale, gx); break;
        case 6: MF_LAUNCH(knn_bwd_kernel<6>, blocks, ENT_BWD_BLOCK, 0, stream, x, ni, d, idx, rho2, coef, cscale, gx); break;
        case 8: MF_LAUNCH(knn_bwd_kernel<8>, blocks, ENT_BWD_BLOCK, 0, stream, x, ni, d, idx, rho2, coef, cscale, gx); break;
        case 12: MF_LAUNCH(knn_bwd_kernel<12>, blocks, ENT_BWD_BLOCK, 0, stream, x, ni, d, idx, rho2, coef, cscale, gx); break;
        default: MF_LAUNCH(knn_bwd_kernel<16>, blocks, ENT_BWD_BLOCK, 0, stream, x, ni, d, idx, rho2, coef, cscale, gx); break;
    }
    return check_launch("mf_knn_entropy_bwd");
}

static int cov_check(const char* who, int64_t n, int d) {
    if (d < 1 || d > ENT_DMAX) return fail("%s supports 1 <= ndim <= %d (got %d)", who, ENT_DMAX, d);
    if (n < 2) return fail("%s needs at least two points (got %lld)", who, (long long)n);
    return 0;
}

static int cov_groups(int64_t n) {
    const int64_t g = (n + 4 * ENT_BLOCK - 1) / (4 * ENT_BLOCK);
    return (int)(g < 1 ? 1 : (g > COV_GMAX ? COV_GMAX : g));
}

extern "C" int64_t mf_cov_entropy_ws_doubles(int64_t n, int d) {
    if (cov_check("mf_cov_entropy_ws_doubles", n, d)) return -1;
    return (int64_t)cov_groups(n) * d * COV_STRIDE;
}

extern "C" int mf_cov_entropy_fwd(const float* x, int64_t n, int d, double pad, float* H, double* aux, double* ws,
                                  void* stream) {
    if (cov_check("mf_cov_entropy_fwd", n, d)) return 1;
    if (ws == nullptr) return fail("mf_cov_entropy_fwd: the workspace is missing");
    const int G = cov_groups(n);
    MF_LAUNCH(cov_moments_kernel, dim3((unsigned)G, (unsigned)d), ENT_BLOCK, 0, stream, x, n, d, ws);
    if (check_launch("mf_cov_entropy_fwd (moments)")) return 1;
    MF_LAUNCH(cov_tail_kernel, 1, ENT_BLOCK, 0, stream, (const double*)ws, G, n, d, pad, H, aux);
    return check_launch("mf_cov_entropy_fwd (tail)");
}

extern "C" int mf_cov_entropy_bwd(const float* x, int64_t n, int d, const double* aux, const float* coef, float* gx,
                                  void* stream) {
    if (cov_check("mf_cov_entropy_bwd", n, d)) return 1;
    int64_t g = (n + ENT_BLOCK - 1) / ENT_BLOCK;
    if (g > NUM_CU * 8) g = NUM_CU * 8;
    MF_LAUNCH(cov_bwd_kernel, (unsigned)g, ENT_BLOCK, 0, stream, x, n, d, aux, coef, gx);
    return check_launch("mf_cov_entropy_bwd");
}
