// Metropolis-adjusted Langevin chains on the density of classical MENT, on gfx950: the proposals of mcmc.hip's random walk
// pushed along the gradient of the log-density, which ment_logp_point.h delivers with the value in one pass over the slots.  The
// reference has no such sampler.
//
// The layout is that of mcmc.hip.  One lane per chain; the chain's state x[d <= 8], its log-density l = logp(x) and the gradient
// g = grad logp(x) live in registers for the whole launch; descriptors (and the tables, under the rule of ment_slots.h) are
// staged in LDS once per workgroup.  With s_j = scale[j], a_j = s_j^2 / 2 and c_j = drift_clip s_j, per step t (global index
// step_offset + t), all in fp32:
//   drift_j(x) = min(max(a_j g_j(x), -c_j), c_j)             (truncated per axis: h' / h is unbounded next to a zero of a table)
//   y_j  = fma(s_j, z_j, x_j + drift_j(x))                   z = noise[t][0..d)[c]
//   (ly, gy) = logp_point(y)                                 (the bits mf_ment_logprob returns for y)
//   r_j  = ((x_j - y_j) - drift_j(y)) / s_j                  (the residual of the reverse move; that of the forward one is z_j)
//   D    = (ly - l) + (sum z_j^2 - sum r_j^2) / 2            u = noise[t][d][c]
//   accept  iff  ly > -inf ? (l == -inf || log u < D) : (ly == -inf && l == -inf),  and never with a NaN in z or u.
// The truncated drift is a deterministic function of the state alone, so the Metropolis correction is exact.  The conventions are
// those of mcmc.hip: a chain inside the support never leaves it; a chain outside it (l == -inf, whose gradient row is 0: no drift)
// random-walks and takes the first point inside; a NaN ly (a NaN in the noise) or a NaN u is rejected, so the state stays finite;
// u == 0 accepts whenever D > -inf.  The test is made on sums of logarithms: where the fp32 product that mcmc.hip compares has
// left fp32's range (a hundred factors of 1e-3) l is still finite and the rule still the Metropolis rule.
//
// l and g are recomputed from x at entry: nothing but x crosses launches, and tables that changed between calls are picked up.
// Nothing in a chain depends on another chain or on how the steps are cut into launches (keeping is decided by the global step
// index alone): outputs are bitwise reproducible and 40 steps in one launch equal 4 launches of 10.  No atomics.
#include "ment_chain.h"
#include "ment_logp_point.h"

namespace mf {

// The fields of ChainArgs plus logp and drift_clip, in the order the kernel was measured with: the order is the layout of the
// kernel arguments, and with logp behind d the kernel measured 1.5-2 % slower (profiles/ment_refactor_ab.json).
struct MalaArgs {
    const float* noise;     // [steps][d + 1][chains]
    const float* scale;     // [d] proposal scale per axis
    float* out;             // [n_keep][chains][d] or null
    float* logp;            // [chains] or null: logp of the final states
    int64_t steps;
    int64_t keep_t;         // as in ChainArgs
    int64_t keep_row;
    int64_t keep_every;
    int chains;
    int d;
    float drift_clip;       // the drift moves a chain by at most drift_clip proposal standard deviations per axis
};

__device__ __forceinline__ float mala_drift(float g, float s, float clip) {
    const float a = 0.5f * s * s, c = clip * s;
    return fminf(fmaxf(a * g, -c), c);
}

template <bool TAB_LDS>
__global__ __launch_bounds__(MENT_BLOCK) void mala_ment_steps_kernel(float* __restrict__ x, MalaArgs ma, SlotArgs sa,
                                                                     int* __restrict__ accepted) {
    MF_DYN_SMEM(float, lds);
    float* desc;
    int* meta;
    const float* tab = stage_slots<TAB_LDS>(sa, lds, desc, meta);
    const int c = blockIdx.x * MENT_BLOCK + threadIdx.x;
    if (c >= ma.chains) return;                       // after the barrier of stage_slots
    const int d = ma.d;
    const float clip = ma.drift_clip;
    const float inv_a2 = prior_inv_a2(sa);
    float xv[MENT_DMAX], sc[MENT_DMAX], g[MENT_DMAX];
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j) {
        xv[j] = (j < d) ? x[(int64_t)c * d + j] : 0.0f;
        sc[j] = (j < d) ? ma.scale[j] : 0.0f;
    }
    float lp = logp_point<true>(xv, d, desc, meta, tab, sa, inv_a2, g);
    int acc = 0;
    const int64_t row = ma.chains;                     // floats per noise row
    int64_t keep_t = ma.keep_t, keep_row = ma.keep_row;
    for (int64_t t = 0; t < ma.steps; ++t) {
        const float* nz = chain_noise(ma, t, c);
        float yv[MENT_DMAX], gy[MENT_DMAX];
        float zz = 0.0f;
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) {
            yv[j] = 0.0f;
            if (j < d) {
                const float z = nz[j * row];
                yv[j] = fmaf(sc[j], z, xv[j] + mala_drift(g[j], sc[j], clip));
                zz = fmaf(z, z, zz);
            }
        }
        const float u = nz[d * row];
        const float lp_new = logp_point<true>(yv, d, desc, meta, tab, sa, inv_a2, gy);
        float rr = 0.0f;
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) {
            if (j < d) {
                const float r = ((xv[j] - yv[j]) - mala_drift(gy[j], sc[j], clip)) / sc[j];
                rr = fmaf(r, r, rr);
            }
        }
        const float delta = (lp_new - lp) + 0.5f * (zz - rr);
        bool accept = lp_new > -INFINITY ? (lp == -INFINITY || logf(u) < delta) : (lp_new == -INFINITY && lp == -INFINITY);
        accept = accept && u == u && zz == zz;         // NaN noise never moves a chain, wherever the chain is
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) {
            xv[j] = accept ? yv[j] : xv[j];
            g[j] = accept ? gy[j] : g[j];
        }
        lp = accept ? lp_new : lp;
        acc += accept ? 1 : 0;
        chain_keep(ma, t, c, xv, keep_t, keep_row);
    }
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j)
        if (j < d) x[(int64_t)c * d + j] = xv[j];
    accepted[c] += acc;
    if (ma.logp != nullptr) ma.logp[c] = lp;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_mala_ment_steps(float* x, int64_t chains, int d, int nslot, const float* desc, const int32_t* meta,
                                  const float* tables, int64_t table_floats, int prior_kind, float prior_a,
                                  float prior_lognorm, const float* noise, int64_t steps, int64_t step_offset,
                                  const float* scale, float drift_clip, int64_t keep_from, int64_t keep_every, float* out,
                                  int32_t* accepted, float* logp, void* stream) {
    size_t smem;
    bool tl;
    if (slot_geometry(d, nslot, table_floats, prior_kind, &smem, &tl)) return 1;
    MalaArgs ma;
    if (chain_args("mala", chains, d, noise, steps, step_offset, scale, keep_from, keep_every, out, &ma)) return 1;
    if (!(drift_clip >= 0.0f)) return fail("mala: drift_clip must be >= 0 (got %g)", (double)drift_clip);
    if (chains == 0) return 0;
    const SlotArgs sa = slot_args(nslot, desc, meta, tables, table_floats, prior_kind, prior_a, prior_lognorm);
    ma.logp = logp;
    ma.drift_clip = drift_clip;
    const int G = (int)((chains + MENT_BLOCK - 1) / MENT_BLOCK);
    MF_LAUNCH_TAB(tl, mala_ment_steps_kernel<true>, mala_ment_steps_kernel<false>, G, MENT_BLOCK, smem, stream, x, ma, sa,
                  accepted);
    return check_launch("mf_mala_ment_steps");
}
