// The resampling stage of a sequential Monte Carlo sampler on classical MENT's density, on gfx950: systematic resampling of
// `chains` weighted states split into `groups` islands of S = chains / groups consecutive chains, decided per island by its own
// effective sample size, on the device.  The moves between two resampling stages are mf_ais_ment_steps (ais.hip), which takes
// and returns nothing but x and logw.  The reference has no counterpart.
//
// Two launches.  smc_island_kernel, one workgroup per island: with m = max logw over the island and w_i = exp(logw_i - m) in
// fp64 (a logw that is not finite counts as weight 0),
//   S1 = sum w,  S2 = sum w^2,  ess = S1^2 / S2,  log mean weight = m + log(S1 / S),
//   the island resamples  iff  S1 > 0 and ess < (double)ess_threshold * S,
// and if it does, the inclusive prefix sums P_i go to scratch.  Every sum has the fixed order of ment_prefix_kernel (ment.hip):
// thread t owns the contiguous segment [t * per, (t + 1) * per), per = ceil(S / SMC_THREADS), and sums it from its first
// element on; thread 0 adds the segment totals in thread order; P_i = (total of the segments before t) + (the segment's own
// running sum up to i).  So P is non-decreasing, P_i == P_{i-1} bit for bit where w_i == 0, and P_{S-1} == S1 bit for bit.
// smc_gather_kernel, one lane per new row j of an island that resamples: with c = S1 / S and u clamped into [0, 1 - 2^-53], the
// parent is the first i with
//   fma(-(double)j, c, P_i) > u * c,
// which is P_i > (u + j) c without the rounding of u + j: with equal weights (w = 1, P_i = i + 1, c = 1, all exact) the parent
// of row j is j for every u in [0, 1).  The test is monotone in i (binary search) and in j (parents do not decrease), and a state
// of weight 0 is never the first to pass it.  Where rounding lets no i pass, the parent is the first i with P_i == S1: the last
// state whose weight moved the prefix, which is the last state of weight > 0 unless the weights after it are lost in the
// rounding of S1.  x_out[j] = x[parent] bitwise, logw[j] = the island's log mean weight (logsumexp(logw) - log S is kept).  An
// island that does not resample copies its rows, gets identity parents and keeps its logw bits.  No atomics.
#include "ment_chain.h"

namespace mf {

constexpr int SMC_THREADS = 1024;                         // one workgroup per island: 64 elements per thread at S = 65 536
constexpr double SMC_UMAX = 1.0 - 1.1102230246251565e-16; // 1 - 2^-53

__device__ __forceinline__ double smc_weight(double lw, double m) {
    return (lw > -INFINITY && lw < INFINITY) ? exp(lw - m) : 0.0;     // NaN fails both comparisons
}

__global__ __launch_bounds__(SMC_THREADS) void smc_island_kernel(const double* __restrict__ logw, int64_t S, float ess_threshold,
                                                                 double* __restrict__ stats, double* __restrict__ scratch) {
    __shared__ double seg1[SMC_THREADS];
    __shared__ double seg2[SMC_THREADS];
    __shared__ double tot[2];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * S;
    const double* lw = logw + base;
    const int64_t per = (S + SMC_THREADS - 1) / SMC_THREADS;
    const int64_t a = min((int64_t)t * per, S);
    const int64_t b = min(a + per, S);
    // the maximum (exact in any order)
    double m = -INFINITY;
    for (int64_t i = a; i < b; ++i) {
        const double v = lw[i];
        if (v > m && v < INFINITY) m = v;
    }
    seg1[t] = m;
    __syncthreads();
    for (int s = SMC_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) seg1[t] = fmax(seg1[t], seg1[t + s]);
        __syncthreads();
    }
    m = seg1[0];
    __syncthreads();
    // S1 and S2: segment sums, then the segment totals in thread order
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = a; i < b; ++i) {
        const double w = smc_weight(lw[i], m);
        s1 += w;
        s2 += w * w;
    }
    seg1[t] = s1;
    seg2[t] = s2;
    __syncthreads();
    if (t == 0) {
        double run1 = 0.0, run2 = 0.0;
        for (int i = 0; i < SMC_THREADS; ++i) {
            const double v = seg1[i];
            seg1[i] = run1;
            run1 += v;
            run2 += seg2[i];
        }
        tot[0] = run1;
        tot[1] = run2;
    }
    __syncthreads();
    const double S1 = tot[0], S2 = tot[1];
    const double ess = S1 > 0.0 ? S1 * S1 / S2 : 0.0;
    const bool go = S1 > 0.0 && ess < (double)ess_threshold * (double)S;
    if (t == 0) {
        double* st = stats + (int64_t)blockIdx.x * 4;
        st[0] = S1 > 0.0 ? m + log(S1 / (double)S) : -INFINITY;
        st[1] = ess;
        st[2] = go ? 1.0 : 0.0;
        st[3] = m;
    }
    if (!go) return;
    const double before = seg1[t];
    double run = 0.0;
    for (int64_t i = a; i < b; ++i) {
        run += smc_weight(lw[i], m);
        scratch[base + i] = before + run;
    }
}

template <int V>
struct SmcVec;
template <>
struct SmcVec<1> {
    typedef float type;
};
template <>
struct SmcVec<2> {
    typedef float2 type;
};
template <>
struct SmcVec<4> {
    typedef float4 type;
};

// rows are copied in pieces of V floats (V divides d, and the host has checked the alignment of both arrays)
template <int V>
__global__ __launch_bounds__(MENT_BLOCK) void smc_gather_kernel(const float* __restrict__ x, float* __restrict__ x_out,
                                                                int64_t chains, int d, int64_t S, double* __restrict__ logw,
                                                                const double* __restrict__ u, int32_t* __restrict__ ancestors,
                                                                const double* __restrict__ stats,
                                                                const double* __restrict__ scratch) {
    typedef typename SmcVec<V>::type vec;
    const int64_t row = (int64_t)blockIdx.x * MENT_BLOCK + threadIdx.x;
    if (row >= chains) return;
    const int64_t g = row / S;
    const int64_t j = row - g * S;
    int64_t parent = row;
    if (stats[g * 4 + 2] != 0.0) {
        const double* P = scratch + g * S;
        const double S1 = P[S - 1];
        const double c = S1 / (double)S;
        double uu = u[g];
        if (!(uu >= 0.0)) uu = 0.0;                        // a NaN too
        if (uu > SMC_UMAX) uu = SMC_UMAX;
        const double rhs = uu * c;
        const double nj = -(double)j;
        // first i in [0, S) that passes; hi == S: none
        int64_t lo = 0, hi = S;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (fma(nj, c, P[mid]) > rhs) hi = mid;
            else lo = mid + 1;
        }
        if (lo == S) {                                     // rounding: the first i with P_i == S1
            lo = 0;
            hi = S - 1;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (P[mid] >= S1) hi = mid;
                else lo = mid + 1;
            }
        }
        parent = g * S + lo;
        logw[row] = stats[g * 4];
    }
    ancestors[row] = (int32_t)parent;
    const vec* src = reinterpret_cast<const vec*>(x + parent * d);
    vec* dst = reinterpret_cast<vec*>(x_out + row * d);
    for (int k = 0; k < d / V; ++k) dst[k] = src[k];
}

}  // namespace mf

using namespace mf;

extern "C" int mf_smc_resample(const float* x, float* x_out, int64_t chains, int d, int64_t groups, double* logw, const double* u,
                               float ess_threshold, int32_t* ancestors, double* stats, double* scratch, void* stream) {
    if (d < 1 || d > MENT_DMAX) return fail("smc: 1 <= ndim <= %d expected (got %d)", MENT_DMAX, d);
    if (chains < 0 || chains > 2147483647LL - MENT_BLOCK) return fail("smc: bad chain count %lld", (long long)chains);
    if (groups < 1 || groups > 2147483647LL) return fail("smc: groups >= 1 expected (got %lld)", (long long)groups);
    if (chains % groups != 0)
        return fail("smc: chains must be a multiple of groups (got %lld and %lld)", (long long)chains, (long long)groups);
    if (chains == 0) return 0;
    if (x == nullptr || x_out == nullptr || logw == nullptr || u == nullptr || ancestors == nullptr || stats == nullptr ||
        scratch == nullptr)
        return fail("smc: x, x_out, logw, u, ancestors, stats and scratch must not be null");
    if (x == x_out) return fail("smc: x_out must not be x (rows are gathered, not moved in place)");
    const int64_t S = chains / groups;
    MF_LAUNCH(smc_island_kernel, (int)groups, SMC_THREADS, 0, stream, logw, S, ess_threshold, stats, scratch);
    const int G = (int)((chains + MENT_BLOCK - 1) / MENT_BLOCK);
    const uintptr_t both = (uintptr_t)x | (uintptr_t)x_out;
    if (d % 4 == 0 && both % 16 == 0)
        MF_LAUNCH(smc_gather_kernel<4>, G, MENT_BLOCK, 0, stream, x, x_out, chains, d, S, logw, u, ancestors, stats, scratch);
    else if (d % 2 == 0 && both % 8 == 0)
        MF_LAUNCH(smc_gather_kernel<2>, G, MENT_BLOCK, 0, stream, x, x_out, chains, d, S, logw, u, ancestors, stats, scratch);
    else
        MF_LAUNCH(smc_gather_kernel<1>, G, MENT_BLOCK, 0, stream, x, x_out, chains, d, S, logw, u, ancestors, stats, scratch);
    return check_launch("mf_smc_resample");
}
