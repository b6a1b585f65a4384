// Random-walk Metropolis-Hastings chains on the density of classical MENT (the product of Lagrange functions of ment.hip times
// the prior), on gfx950: a particle sampler that needs point evaluations only, where GridSampler needs the density on every
// cell of a dense grid (res^d cells).  The reference has no such sampler.
//
// One lane per chain.  The chain's state x[d <= 8] and its density p live in registers for the whole launch; descriptors (and
// the tables, under the rule of ment_slots.h) are staged in LDS once per workgroup.  Per step t (global index
// g = step_offset + t):
//   y = fma(scale, noise[t][0..d)[c], x)                     (fp32, one rounding per axis)
//   p_new = prob(y)                                          (prob_point: the bits mf_ment_prob returns)
//   u = noise[t][d][c]
//   accept  iff  p_new > 0 ? u * p < p_new : (p_new == 0 && p == 0)
// so a chain inside the support never leaves it, a chain outside it (p == 0) random-walks until it finds it, and a NaN p_new
// (a NaN in the noise) or a NaN u is rejected: the state stays finite.  The noise comes from the caller ([steps][d + 1][chains],
// chain fastest: a wave reads 64 consecutive floats per row), so torch.manual_seed fixes a run.
//
// p is recomputed from x at entry: no density buffer crosses the ABI, and p is right when the tables changed between calls.
// Nothing in a chain depends on another chain or on how the steps are cut into launches (keeping is decided by g alone):
// outputs are bitwise reproducible and 40 steps in one launch equal 4 launches of 10.  No atomics.
#include "ment_chain.h"

namespace mf {

template <bool TAB_LDS>
__global__ __launch_bounds__(MENT_BLOCK) void mcmc_ment_steps_kernel(float* __restrict__ x, ChainArgs ma, SlotArgs sa,
                                                                     int* __restrict__ accepted) {
    MF_DYN_SMEM(float, lds);
    float* desc;
    int* meta;
    const float* tab = stage_slots<TAB_LDS>(sa, lds, desc, meta);
    const int c = blockIdx.x * MENT_BLOCK + threadIdx.x;
    if (c >= ma.chains) return;                       // after the barrier of stage_slots
    const int d = ma.d;
    float xv[MENT_DMAX], sc[MENT_DMAX];
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j) {
        xv[j] = (j < d) ? x[(int64_t)c * d + j] : 0.0f;
        sc[j] = (j < d) ? ma.scale[j] : 0.0f;
    }
    float p = prob_point(xv, d, desc, meta, tab, sa);
    int acc = 0;
    const int64_t row = ma.chains;                     // floats per noise row
    int64_t keep_t = ma.keep_t, keep_row = ma.keep_row;
    for (int64_t t = 0; t < ma.steps; ++t) {
        const float* nz = chain_noise(ma, t, c);
        float yv[MENT_DMAX];
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) {
            yv[j] = (j < d) ? fmaf(sc[j], nz[j * row], xv[j]) : 0.0f;
        }
        const float u = nz[d * row];
        const float p_new = prob_point(yv, d, desc, meta, tab, sa);
        const bool accept = p_new > 0.0f ? (u * p < p_new) : (p_new == 0.0f && p == 0.0f);
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) xv[j] = accept ? yv[j] : xv[j];
        p = accept ? p_new : p;
        acc += accept ? 1 : 0;
        chain_keep(ma, t, c, xv, keep_t, keep_row);
    }
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j)
        if (j < d) x[(int64_t)c * d + j] = xv[j];
    accepted[c] += acc;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_mcmc_ment_steps(float* x, int64_t chains, int d, int nslot, const float* desc, const int32_t* meta,
                                  const float* tables, int64_t table_floats, int prior_kind, float prior_a,
                                  float prior_lognorm, const float* noise, int64_t steps, int64_t step_offset,
                                  const float* scale, int64_t keep_from, int64_t keep_every, float* out, int32_t* accepted,
                                  void* stream) {
    size_t smem;
    bool tl;
    if (slot_geometry(d, nslot, table_floats, prior_kind, &smem, &tl)) return 1;
    ChainArgs ma;
    if (chain_args("mcmc", chains, d, noise, steps, step_offset, scale, keep_from, keep_every, out, &ma)) return 1;
    if (chains == 0) return 0;
    const SlotArgs sa = slot_args(nslot, desc, meta, tables, table_floats, prior_kind, prior_a, prior_lognorm);
    const int G = (int)((chains + MENT_BLOCK - 1) / MENT_BLOCK);
    MF_LAUNCH_TAB(tl, mcmc_ment_steps_kernel<true>, mcmc_ment_steps_kernel<false>, G, MENT_BLOCK, smem, stream, x, ma, sa,
                  accepted);
    return check_launch("mf_mcmc_ment_steps");
}
