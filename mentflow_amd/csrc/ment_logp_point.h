// Log-density of classical MENT and its gradient at ONE point, shared by the kernels of ment_logp.hip (one lane per point) and
// mala.hip (one lane per chain, the point is the chain's state or its proposal).  Both call logp_point, so both return the same
// bits for the same point; the factors come from slot_value of ment_slots.h.  Conventions,
// range handling and the gradient are described at the top of ment_logp.hip.
#pragma once
#include "ment_slots.h"

namespace mf {

constexpr int LOGP_RENORM = 16;        // slots between renormalisations of the running product (a mantissa is >= 1/2)

// 1 / prior_a^2 of a Gaussian prior (0 otherwise): formed once per launch and handed to logp_point
__device__ __forceinline__ float prior_inv_a2(const SlotArgs& sa) {
    return sa.prior_kind == 1 ? 1.0f / (sa.prior_a * sa.prior_a) : 0.0f;
}

// logp at xv (xv[d..8) = 0); when GRAD, g[0..d) = d logp / dx, the row of a -inf point 0 and that of a NaN point NaN
// (g[d..8) carries no meaning).  desc / meta / tab as stage_slots returns them.
template <bool GRAD>
__device__ __forceinline__ float logp_point(const float (&xv)[MENT_DMAX], int d, const float* __restrict__ desc,
                                            const int* __restrict__ meta, const float* __restrict__ tab, const SlotArgs& sa,
                                            float inv_a2, float (&g)[MENT_DMAX]) {
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j) g[j] = 0.0f;
    float m = 1.0f;                 // running product of the factors' mantissas; NaN once a factor was NaN
    int e = 0;                      // running sum of their exponents
    bool dead = false;              // a zero factor: logp = -inf
    for (int s = 0; s < sa.nslot; ++s) {
        const float* ds = desc + s * MENT_DESC;
        float h0, h1;
        const float h = clamp_factor(slot_value<GRAD>(xv, d, ds, meta + s * MENT_META, tab, h0, h1));
        if (h != h) {
            m = h;
            break;
        }
        if (h == 0.0f) {
            dead = true;
            break;
        }
        int eh;
        m *= frexpf(h, &eh);
        e += eh;
        if ((s & (LOGP_RENORM - 1)) == LOGP_RENORM - 1) {
            m = frexpf(m, &eh);
            e += eh;
        }
        if (GRAD) {
            const float r = h < 1.0e10f ? __frcp_rn(h) : 0.0f;      // on the upper clamp the factor is a constant
            const float c0 = h0 * r, c1 = h1 * r;
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j)
                if (j < d) g[j] = fmaf(c0, ds[j], g[j]);
            if (meta[s * MENT_META] == 2) {
#pragma unroll
                for (int j = 0; j < MENT_DMAX; ++j)
                    if (j < d) g[j] = fmaf(c1, ds[8 + j], g[j]);
            }
        }
    }
    float lp;
    if (dead) {
        lp = -INFINITY;
    } else if (m != m) {
        lp = m;
    } else {
        int em;
        m = frexpf(m, &em);
        lp = fmaf((float)(e + em), 0.693147180559945f, logf(m));
        if (sa.prior_kind == 1) {               // prior.Gaussian.log_prob(x), the argument of prior_factor's exp
            float q = 0.0f;
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j)
                if (j < d) q = q + xv[j] * xv[j];
            lp += sa.prior_lognorm - (0.5f * q) / (sa.prior_a * sa.prior_a);
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j) g[j] = fmaf(-xv[j], inv_a2, g[j]);
        } else if (sa.prior_kind == 2) {        // uniform density on [-a, a]^d
            bool inside = true;
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j)
                if (j < d) inside = inside && fabsf(xv[j]) <= sa.prior_a;
            lp = inside ? lp + sa.prior_lognorm : -INFINITY;
        }
    }
    if (GRAD) {
        const bool out = lp == -INFINITY, nan = lp != lp;
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j)
            if (j < d) g[j] = out ? 0.0f : (nan ? lp : g[j]);
    }
    return lp;
}

}  // namespace mf
