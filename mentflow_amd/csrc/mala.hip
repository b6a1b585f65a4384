// Metropolis-adjusted Langevin chains on the density of classical MENT, on gfx950: the proposals of mcmc.hip's random walk
// pushed along the gradient of the log-density, which ment_logp_point.h delivers with the value in one pass over the slots.  The
// reference has no such sampler.
//
// The layout is that of mcmc.hip.  One lane per chain; the chain's state x[d <= 8], its log-density l = logp(x) and the gradient
// g = grad logp(x) live in registers for the whole launch; descriptors (and the tables, under the rule of ment_slots.h) are
// staged in LDS once per workgroup.  Step t (global index step_offset + t) is langevin_step of ment_langevin.h, which states the
// fp32 operation order, the acceptance rule and its conventions, on the plain target l = logp, g = grad logp (LogpTarget).
//
// l and g are recomputed from x at entry: nothing but x crosses launches, and tables that changed between calls are picked up.
// Nothing in a chain depends on another chain or on how the steps are cut into launches (keeping is decided by the global step
// index alone): outputs are bitwise reproducible and 40 steps in one launch equal 4 launches of 10.  No atomics.
#include "ment_langevin.h"

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

template <bool TAB_LDS>
__global__ __launch_bounds__(MENT_BLOCK) void mala_ment_steps_kernel(float* __restrict__ x, MalaArgs ma, SlotArgs sa,
                                                                     int* __restrict__ accepted) {
    MF_DYN_SMEM(float, lds);
    float* desc;
    int* meta;
    const float* tab = stage_slots<TAB_LDS>(sa, lds, desc, meta);
    const int c = blockIdx.x * MENT_BLOCK + threadIdx.x;
    if (c >= ma.chains) return;                       // after the barrier of stage_slots
    const LogpTarget tg{ma.d, desc, meta, tab, sa, prior_inv_a2(sa)};
    LogpTarget::Point p;
    float sc[MENT_DMAX];
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j) {
        p.x[j] = (j < ma.d) ? x[(int64_t)c * ma.d + j] : 0.0f;
        sc[j] = (j < ma.d) ? ma.scale[j] : 0.0f;
    }
    tg.eval(p);
    int acc = 0;
    int64_t keep_t = ma.keep_t, keep_row = ma.keep_row;
    for (int64_t t = 0; t < ma.steps; ++t) {
        acc += langevin_step(tg, ma, t, c, sc, p) ? 1 : 0;
        chain_keep(ma, t, c, p.x, keep_t, keep_row);
    }
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j)
        if (j < ma.d) x[(int64_t)c * ma.d + j] = p.x[j];
    accepted[c] += acc;
    if (ma.logp != nullptr) ma.logp[c] = p.lp;
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
