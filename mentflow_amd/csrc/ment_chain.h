// What the chain samplers on classical MENT's density (mcmc.hip, mala.hip, ais.hip) have in common: one lane per chain, the noise
// layout [steps][d + 1][chains], which steps are kept and where they go.  The random walk's rule is in mcmc.hip, the Langevin
// transition of the other two is stated in ment_langevin.h.  The helpers take any argument struct with the fields of ChainArgs:
// MalaArgs (mala.hip) and AisArgs (ais.hip) keep a field order of their own.
#pragma once
#include "ment_slots.h"

namespace mf {

struct ChainArgs {
    const float* noise;     // [steps][d + 1][chains]
    const float* scale;     // [d] proposal scale per axis
    float* out;             // [n_keep][chains][d] or null
    int64_t steps;
    int64_t keep_t;         // first step t of this launch that is kept (>= steps: none), formed on the host from step_offset,
    int64_t keep_row;       // keep_from and keep_every, and the row of `out` it goes to
    int64_t keep_every;
    int chains;
    int d;
};

// chain c's noise of step t: axis j at [j * chains], the uniform at [d * chains]
template <class Args>
__device__ __forceinline__ const float* chain_noise(const Args& ca, int64_t t, int c) {
    return ca.noise + t * (ca.d + 1) * ca.chains + c;
}

// writes the state to `out` if step t is the next kept one, and moves on to the one after
template <class Args>
__device__ __forceinline__ void chain_keep(const Args& ca, int64_t t, int c, const float (&xv)[MENT_DMAX], int64_t& keep_t,
                                           int64_t& keep_row) {
    if (t != keep_t) return;
    float* o = ca.out + (keep_row * ca.chains + c) * ca.d;
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j)
        if (j < ca.d) o[j] = xv[j];
    keep_t += ca.keep_every;
    ++keep_row;
}

// checks the chain arguments of entry point `who` ("mcmc", "mala", "ais": the prefix of its messages) and fills the ChainArgs
// fields of *ca
template <class Args>
static int chain_args(const char* who, int64_t chains, int d, const float* noise, int64_t steps, int64_t step_offset,
                      const float* scale, int64_t keep_from, int64_t keep_every, float* out, Args* ca) {
    if (chains < 0 || chains > 2147483647LL - MENT_BLOCK) return fail("%s: bad chain count %lld", who, (long long)chains);
    if (steps < 0 || step_offset < 0 || keep_from < 0) return fail("%s: steps, step_offset and keep_from must be >= 0", who);
    if (keep_every < 1) return fail("%s: keep_every must be >= 1 (got %lld)", who, (long long)keep_every);
    const int64_t lim = (int64_t)1 << 40;              // keeps the step arithmetic far from overflow
    if (steps > lim || step_offset > lim || keep_from > lim || keep_every > lim) return fail("%s: step counts beyond 2^40", who);
    ca->noise = noise;
    ca->scale = scale;
    ca->out = out;
    ca->steps = steps;
    // step g = step_offset + t is kept iff g >= keep_from and (g - keep_from) % keep_every == 0, as row (g - keep_from) / keep_every
    const int64_t k0 = step_offset - keep_from;
    const int64_t r = k0 > 0 ? k0 % keep_every : 0;
    ca->keep_t = k0 <= 0 ? -k0 : (r == 0 ? 0 : keep_every - r);
    ca->keep_row = k0 <= 0 ? 0 : (k0 + keep_every - 1) / keep_every;
    if (out == nullptr) ca->keep_t = steps;           // nothing is kept
    ca->keep_every = keep_every;
    ca->chains = (int)chains;
    ca->d = d;
    return 0;
}

}  // namespace mf
