// The Metropolis-adjusted Langevin transition: one proposal along the truncated gradient, its Metropolis correction on logarithms,
// and the select of what the chain carries.  mala.hip takes langevin_step on the MENT log-density (LogpTarget); ais.hip shares
// langevin_drift and this statement of the rule, and spells the step out on its tempered target (its header says why).
// The target comes as a template parameter and gives
//   Target::Point                  a state x[] and what the chain carries with it (the plain target: lp and g)
//   eval(p)                        fills the rest of p from p.x
//   value(p)                       l, the log of the density the transition is reversible for
//   grad(p, l, j)                  d l / d x_j
//   Target::select(accept, p, q)   p = accept ? q : p, the state and the gradient in ONE loop over the axes
//
// fp32 operation order, stated here once (tests/_mala_fp64.py restates it).  With s_j = scale[j], a_j = 0.5 s_j s_j and
// c_j = drift_clip s_j, z = noise[t][0..d)[c] and u = noise[t][d][c]:
//   drift_j(x) = min(max(a_j g_j(x), -c_j), c_j)             (truncated per axis: h' / h is unbounded next to a zero of a table)
//   y_j  = fma(s_j, z_j, x_j + drift_j(x))
//   r_j  = ((x_j - y_j) - drift_j(y)) / s_j                  (the residual of the reverse move; that of the forward one is z_j)
//   D    = (l(y) - l(x)) + 0.5 (zz - rr)                     zz = sum z_j^2, rr = sum r_j^2, both by fma from axis 0 on
//   accept  iff  l(y) > -inf ? (l(x) == -inf || log u < D) : (l(y) == -inf && l(x) == -inf),  and never with a NaN in z or u.
// The truncated drift is a deterministic function of the state alone, so the Metropolis correction is exact.  The conventions are
// those of mcmc.hip: a chain inside the support never leaves it; a chain outside it (l == -inf, whose gradient row is 0: no drift)
// random-walks and takes the first point inside; a NaN l(y) (a NaN in the noise) or a NaN u is rejected, so the state stays
// finite; u == 0 accepts whenever D > -inf.  The test is made on sums of logarithms: where the fp32 product that mcmc.hip compares
// has left fp32's range (a hundred factors of 1e-3) l is still finite and the rule still the Metropolis rule.
#pragma once
#include "ment_chain.h"
#include "ment_logp_point.h"

namespace mf {

__device__ __forceinline__ float langevin_drift(float g, float s, float clip) {
    const float a = 0.5f * s * s, c = clip * s;
    return fminf(fmaxf(a * g, -c), c);
}

// The plain target: the MENT log-density itself, as logp_point<true> gives it (the bits mf_ment_logprob returns).  It holds
// what logp_point reads, as stage_slots returned it.
struct LogpTarget {
    struct Point {
        float x[MENT_DMAX], g[MENT_DMAX], lp;
    };
    int d;
    const float* desc;
    const int* meta;
    const float* tab;
    const SlotArgs& sa;
    float inv_a2;

    __device__ __forceinline__ void eval(Point& p) const { p.lp = logp_point<true>(p.x, d, desc, meta, tab, sa, inv_a2, p.g); }
    __device__ __forceinline__ float value(const Point& p) const { return p.lp; }
    __device__ __forceinline__ float grad(const Point& p, float, int j) const { return p.g[j]; }
    static __device__ __forceinline__ void select(bool accept, Point& p, const Point& q) {
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) {
            p.x[j] = accept ? q.x[j] : p.x[j];
            p.g[j] = accept ? q.g[j] : p.g[j];
        }
        p.lp = accept ? q.lp : p.lp;
    }
};

// Step t of chain c, at p, of a launch with the arguments ca (the fields of ChainArgs and drift_clip); returns whether it moved.
template <class Target, class Args>
__device__ __forceinline__ bool langevin_step(const Target& tg, const Args& ca, int64_t t, int c, const float (&sc)[MENT_DMAX],
                                              typename Target::Point& p) {
    const float* nz = chain_noise(ca, t, c);
    const int64_t row = ca.chains;                     // floats per noise row
    const int d = ca.d;
    const float clip = ca.drift_clip;
    const float l = tg.value(p);
    typename Target::Point q;
    float zz = 0.0f;
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j) {
        q.x[j] = 0.0f;
        if (j < d) {
            const float z = nz[j * row];
            q.x[j] = fmaf(sc[j], z, p.x[j] + langevin_drift(tg.grad(p, l, j), sc[j], clip));
            zz = fmaf(z, z, zz);
        }
    }
    const float u = nz[d * row];
    tg.eval(q);
    const float l_new = tg.value(q);
    float rr = 0.0f;
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j) {
        if (j < d) {
            const float r = ((p.x[j] - q.x[j]) - langevin_drift(tg.grad(q, l_new, j), sc[j], clip)) / sc[j];
            rr = fmaf(r, r, rr);
        }
    }
    const float delta = (l_new - l) + 0.5f * (zz - rr);
    bool accept = l_new > -INFINITY ? (l == -INFINITY || logf(u) < delta) : (l_new == -INFINITY && l == -INFINITY);
    accept = accept && u == u && zz == zz;             // NaN noise never moves a chain, wherever the chain is
    Target::select(accept, p, q);
    return accept;
}

}  // namespace mf
