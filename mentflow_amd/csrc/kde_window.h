// What the projection kernels of kde.hip and their weighted counterparts in wproj.hip share: the row loads and projections, the
// centre-bin search, the Gaussian window (plain and factorised), the 2^-50 fixed-point conversion / flush / finishing
// arithmetic, the hard-bin search, and the host-side pieces of the launchers (argument checks, the process-wide plan of
// kde_plan.h and the dispatch over the built kernel instances).  Stated once here; both translation units include it.
#pragma once
#include <type_traits>

#include "common.h"
#include "kde_plan.h"

namespace mf {

constexpr int KDE_DMAX = 8;          // phase-space dimension limit of the projection kernels
constexpr int KDE_BLOCK = 256;
constexpr int KDE_LDS_FLOATS = 24576;   // 96 KiB histogram image per workgroup

__device__ __forceinline__ void load_row(const float* __restrict__ x, int64_t p, int d, float (&xv)[KDE_DMAX]) {
#pragma unroll
    for (int j = 0; j < KDE_DMAX; ++j) xv[j] = (j < d) ? x[p * d + j] : 0.0f;
}

__device__ __forceinline__ float project(const float (&xv)[KDE_DMAX], const float* __restrict__ v, int d) {
    float u = 0.0f;
#pragma unroll
    for (int j = 0; j < KDE_DMAX; ++j)
        if (j < d) u = fmaf(xv[j], v[j], u);
    return u;
}

// centre bin of u on the uniform grid of bin centres (c0, delta); clamped so the window loop is empty when far out
__device__ __forceinline__ int centre_bin(float u, float c0, float inv_delta, int B, int R) {
    float t = (u - c0) * inv_delta;
    t = fminf(fmaxf(t, -(float)(R + 2)), (float)(B + R + 1));   // NaN -> lower clamp -> empty window
    return (int)rintf(t);
}

typedef unsigned long long u64;
constexpr double KDE_FIX_INV = 1.0 / 1125899906842624.0; // 2^-50: fixed-point quantum of the LDS histogram image
constexpr float KDE_FIX_MIN = 8.8817841970012523e-16f;   // 2^-50: smaller weights round down to zero
constexpr float KDE_EXP2_SCALE = 0.7213475204444817f;    // log2(e) / 2:  exp(-r^2/2) = exp2(-KDE_EXP2_SCALE r^2)

__device__ __forceinline__ float gauss_weight(float r) { return __builtin_amdgcn_exp2f(-KDE_EXP2_SCALE * r * r); }

// w in [0, 1] -> round-down 2^-50 fixed point (exact split: high 18 bits and low 32 bits of w * 2^50)
__device__ __forceinline__ u64 to_fix(float w) {
    const float t = w * 262144.0f;
    const unsigned hi = (unsigned)t;
    const unsigned lo = (unsigned)((t - (float)hi) * 4294967296.0f);
    return ((u64)hi << 32) | (u64)lo;
}

// flush of one workgroup's bin total v (2^-50 units, < 2^64) into the bin's 64-bit global accumulator: ONE integer atomic
// per non-zero bin and workgroup.  The global sum of n particles needs log2(n) more bits than a weight, so the
// accumulator is kept in 2^(shift-50) units with shift = max(0, ceil(log2 n) - 13): EXACT (shift 0) up to 8192 particles
// per call, 2^-43 units at 2 M, 2^-40 at 16 M.  The dropped bits cost at most one unit per flush: relative to a bin
// total that is n * 2^-76 / (density * bin width), 2e-6 of a 1e-10 density at 2 M particles — far below the reference's
// own 1e-12 padding — and integer addition keeps the result independent of the order of the workgroups.
__device__ __forceinline__ void fix_flush(u64* __restrict__ acc, u64 v, int shift) {
    v >>= shift;
    if (v != 0) atomicAdd(acc, v);
}

// the finishing kernels' arithmetic: a bin's accumulator (2^(shift-50) units, unit = 2^(shift-50)) -> fp32, rounded once
__device__ __forceinline__ float fix_value(u64 acc, double unit) { return (float)((double)acc * unit); }

// Gaussian window, partly factorised.  With kc the centre bin of u, r0 = (u - c_kc) / sigma and s = delta / sigma, bin
// kc + j of a UNIFORM grid sits at r_j = r0 - j s and
//     w_j = exp(-r_j^2 / 2) = A rho^j gam_j,   A = exp(-r0^2/2),  rho = exp(s r0),  gam_j = exp(-j^2 s^2 / 2).
// The table of bin centres is not exactly uniform (every centre is rounded separately: |dr| <= 4.4e-6), and the loss
// gradient dD/dS = 1 - m / ghat cancels to ~1e-2 near convergence, so a 1e-6 relative error in a bin total shows up as
// 1e-4 in the parameter gradients.  The three bins that carry 99.97 % of a particle's weight — j = 0, +1, -1 — are
// therefore evaluated from the table exactly as the reference does ((u - c_k) / sigma, one v_exp each); only |j| >= 2
// (weights <= 3.4e-4 at s = 2) use the factorised form: 5 v_exp (quarter rate) per particle and projection instead of
// 2 RT + 1 = 9, residual error ~1e-9 of a bin total.  |s r0| <= s^2 / 2, and RT = 4 is only used for bandwidths in
// (0.389, 0.5] bin widths (s in [2, 2.57]): rho^4 <= 5.4e5, nothing overflows.
template <int RT>
struct GaussGamma {
    float g[RT + 1];
};
template <int RT>
__device__ __forceinline__ GaussGamma<RT> gauss_gamma(float s) {
    GaussGamma<RT> gm;
#pragma unroll
    for (int j = 0; j <= RT; ++j) gm.g[j] = __builtin_amdgcn_exp2f(-KDE_EXP2_SCALE * (float)(j * j) * s * s);
    return gm;
}
// cl: table of bin centres; kc may lie up to RT + 2 bins outside [0, B) (then every bin that is read through a clamped
// index is out of range and never used by the caller)
template <int RT>
__device__ __forceinline__ void gauss_window(float u, const float* cl, int kc, int B, float inv_sigma, float s,
                                             const GaussGamma<RT>& gm, float (&w)[2 * RT + 1]) {
    static_assert(RT >= 2, "factorised tail needs at least two bins per side");
    const int k0 = min(max(kc, 0), B - 1), kp = min(max(kc + 1, 0), B - 1), km = min(max(kc - 1, 0), B - 1);
    const float r0 = fmaf((float)(k0 - kc), s, (u - cl[k0]) * inv_sigma);     // virtual centre when kc is outside
    const float A = __builtin_amdgcn_exp2f(-KDE_EXP2_SCALE * r0 * r0);
    w[RT] = A;
    w[RT + 1] = gauss_weight((u - cl[kp]) * inv_sigma);
    w[RT - 1] = gauss_weight((u - cl[km]) * inv_sigma);
    const float e = 2.0f * KDE_EXP2_SCALE * s * r0;
    const float rp = __builtin_amdgcn_exp2f(e), rm = __builtin_amdgcn_exp2f(-e);
    float pp = A * rp, pm = A * rm;
#pragma unroll
    for (int j = 2; j <= RT; ++j) {
        pp *= rp;
        pm *= rm;
        w[RT + j] = pp * gm.g[j];
        w[RT - j] = pm * gm.g[j];
    }
}

__device__ __forceinline__ void load_vrow(const float* Vl, int q, float (&v)[KDE_DMAX]) {
    const float4 a = *reinterpret_cast<const float4*>(Vl + q * KDE_VS);
    const float4 b = *reinterpret_cast<const float4*>(Vl + q * KDE_VS + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ float project8(const float (&xv)[KDE_DMAX], const float (&v)[KDE_DMAX]) {
    float u = 0.0f;
#pragma unroll
    for (int j = 0; j < KDE_DMAX; ++j) u = fmaf(xv[j], v[j], u);     // columns >= d: xv = 0, v = 0
    return u;
}
template <int BLOCK>
__device__ __forceinline__ void stage_vrows(float* Vl, const float* __restrict__ V, int p_begin, int np, int d) {
    for (int i = threadIdx.x; i < np * KDE_VS; i += BLOCK) {
        const int q = i / KDE_VS, j = i - q * KDE_VS;
        Vl[i] = (j < d) ? V[(p_begin + q) * d + j] : 0.0f;
    }
}

// Window cells (i, j) bins away from the centre cell whose weight is below the 2^-50 quantum WHATEVER the position of
// the particle inside its cell: (|i| - 1/2)^2 + (|j| - 1/2)^2 > 2 * 50 ln 2 / s^2 with s >= 2 (radius-4 windows), i.e.
// > 17.33 bins^2 — the four corners (4,4) and the eight (4,3)/(3,4) cells.  They are never visited.
__device__ __forceinline__ constexpr bool kde2d_dead_cell(int i, int j) {
    const int a = i < 0 ? -i : i, b = j < 0 ? -j : j;
    return (a >= 1 && b >= 1) && ((2 * a - 1) * (2 * a - 1) + (2 * b - 1) * (2 * b - 1) > 69);   // 4 * 17.33
}

// torch.histogram / np.histogramdd bin search: bin k iff edges[k] <= u < edges[k+1], last bin right-inclusive.
__device__ __forceinline__ int edge_bin(float u, const float* e, int B, float inv_delta) {
    if (!(u >= e[0]) || !(u <= e[B])) return -1;
    int k = (int)((u - e[0]) * inv_delta);
    k = max(0, min(k, B - 1));
    while (k > 0 && u < e[k]) --k;
    while (k < B - 1 && u >= e[k + 1]) ++k;
    return k;
}

// ------------------------------------------------------------------------------------------------ host side of the launchers
static inline int grid_for(int64_t n, int per_block, int cap) {
    int64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

static inline int kde_check(int64_t n, int d, int P, int B) {
    if (n < 0 || d < 1 || d > KDE_DMAX) return fail("projection kernels support 1 <= d <= %d (got d=%d)", KDE_DMAX, d);
    if (P < 1 || B < 2) return fail("need P >= 1 and at least 2 bins (P=%d, bins=%d)", P, B);
    return 0;
}

// The launch shape of the KDE launchers is decided in kde_plan.h, with the tuning variables as read once per process.
static_assert(KDE_CUS == NUM_CU, "kde_plan.h plans for the chip of common.h");
inline int process_plan(int kernel, int64_t n, int P, int Bx, int By, int radius_x, int radius_y, KdePlan& p) {
    static const KdeKnobs knobs = kde_knobs_from_env();
    return kde_plan(kernel, n, P, Bx, By, radius_x, radius_y, knobs, p) ? 0 : fail("%s", p.err);
}
inline int launch_plan(int kernel, int64_t n, int d, int P, int Bx, int By, int radius_x, int radius_y, KdePlan& p) {
    if (d < 1 || d > KDE_DMAX) return fail("projection kernels support 1 <= d <= %d (got d=%d)", KDE_DMAX, d);
    return process_plan(kernel, n, P, Bx, By, radius_x, radius_y, p);
}

// f(std::integral_constant<int, V>) for the V of the list that v equals.  kde_plan returns no other value: the last one is not tested.
template <int V, int... Rest, class F>
static void pick(int v, F&& f) {
    if constexpr (sizeof...(Rest) > 0) {
        if (v != V) return pick<Rest...>(v, f);
    }
    f(std::integral_constant<int, V>{});
}
// the built instances: window {4, 0} x block {256, 512, 1024} (2-D backward: x particles per thread {1, 2, 4})
template <class F>
static void pick_window_block(const KdePlan& p, F&& f) {
    pick<4, 0>(p.window, [&](auto RT) { pick<256, 512, 1024>(p.block, [&](auto BL) { f(RT, BL); }); });
}

}  // namespace mf
