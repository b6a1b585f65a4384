// Slot machinery of classical MENT shared by every MENT kernel (ment.hip, ment_logp.hip, ment_tabgrad.hip, mcmc.hip, mala.hip):
// the slot arguments, the evaluation of one slot at one point, the product of Lagrange functions
// and the density built on it, the prior, the staging of descriptors (and tables) into LDS, the host-side checks of the slot
// arguments and the dispatch on where the tables live.  The slot layout and the density are described at the top of ment.hip.
#pragma once
#include "common.h"

namespace mf {

constexpr int MENT_DMAX = 8;           // phase-space dimension limit (KDE_DMAX of the projection kernels)
constexpr int MENT_BLOCK = 256;
constexpr int MENT_DESC = 24;          // floats per slot descriptor (see include/mentflow_hip.h)
constexpr int MENT_META = 4;           // ints per slot descriptor
constexpr int MENT_MAX_SLOTS = 512;
// Tables join the descriptors in LDS only while both fit in 40 KiB: four 256-thread workgroups (16 waves, 4 per SIMD) then
// share a CU's 160 KiB, enough to hide the table reads of the other waves.  A larger block would leave fewer waves per CU
// for LDS reads that the L2 serves about as well (the 6 x 85^2 corner tables, 173 KB, run from global memory and L2).
constexpr int MENT_TAB_LDS_FLOATS = 10240;

struct SlotArgs {
    const float* desc;      // [nslot][MENT_DESC]
    const int* meta;        // [nslot][MENT_META]: ndim (1|2), Bx, By, table offset
    const float* tables;    // concatenated [Bx] or [Bx, By] tables
    int nslot;
    int table_floats;
    int prior_kind;         // 0 none, 1 Gaussian N(0, a^2 I), 2 uniform on [-a, a]^d
    float prior_a;
    float prior_lognorm;
};

__device__ __forceinline__ float clamp_factor(float h) {
    return (h != h) ? h : fminf(fmaxf(h, 0.0f), 1.0e10f);
}

// position of u on a uniform centre grid: false outside [c0, cl] (NaN handled by the caller)
__device__ __forceinline__ bool grid_pos(float u, float c0, float cl, float inv_d, int B, int& i, float& w) {
    if (!(u >= c0 && u <= cl)) return false;
    const float s = (u - c0) * inv_d;
    i = min((int)s, B - 2);
    w = fminf(s - (float)i, 1.0f);
    return true;
}

// h of one slot at xv and, when GRAD, its partials along the slot's projected axes.  hipcc contracts a * b + c, and which
// product of a sum it fuses follows the shape of the code around it: the bits of the partials rest on this function's form.
template <bool GRAD>
__device__ __forceinline__ float slot_value(const float (&xv)[MENT_DMAX], int d, const float* __restrict__ ds,
                                            const int* __restrict__ ms, const float* __restrict__ tab, float& h0, float& h1) {
    float u0 = 0.0f;
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j)
        if (j < d) u0 = fmaf(xv[j], ds[j], u0);
    const float* t = tab + ms[3];
    h0 = 0.0f;
    h1 = 0.0f;
    if (ms[0] == 1) {
        int i;
        float w;
        if (u0 != u0) return u0;
        if (!grid_pos(u0, ds[16], ds[17], ds[18], ms[1], i, w)) return 0.0f;
        const float a = t[i], b = t[i + 1];
        if (GRAD) h0 = (b - a) * ds[18];
        return a * (1.0f - w) + b * w;
    }
    float u1 = 0.0f;
#pragma unroll
    for (int j = 0; j < MENT_DMAX; ++j)
        if (j < d) u1 = fmaf(xv[j], ds[8 + j], u1);
    int i, k;
    float wx, wy;
    const int By = ms[2];
    if (u0 != u0 || u1 != u1) return u0 + u1;
    if (!grid_pos(u0, ds[16], ds[17], ds[18], ms[1], i, wx) || !grid_pos(u1, ds[19], ds[20], ds[21], By, k, wy)) return 0.0f;
    const float* r0 = t + i * By + k;
    const float* r1 = r0 + By;
    const float v00 = r0[0], v01 = r0[1], v10 = r1[0], v11 = r1[1];
    if (GRAD) {
        h0 = ((v10 - v00) * (1.0f - wy) + (v11 - v01) * wy) * ds[18];
        h1 = ((v01 - v00) * (1.0f - wx) + (v11 - v10) * wx) * ds[21];
    }
    return v00 * ((1.0f - wx) * (1.0f - wy)) + v01 * ((1.0f - wx) * wy) + v10 * (wx * (1.0f - wy)) + v11 * (wx * wy);
}

// product of the clamped factors over the slots; a product that has reached 0 skips the remaining slots.  The factor is that of
// slot_value<false>, written out: through that function the grid kernels measured 0.1-0.3 % slower (profiles/ment_refactor_ab.json)
__device__ __forceinline__ float slot_product(const float (&xv)[MENT_DMAX], int d, const float* __restrict__ desc,
                                              const int* __restrict__ meta, const float* __restrict__ tab, int nslot) {
    float prob = 1.0f;
    for (int s = 0; s < nslot; ++s) {
        if (prob == 0.0f) break;
        const float* ds = desc + s * MENT_DESC;
        const int* ms = meta + s * MENT_META;
        float u0 = 0.0f;
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j)
            if (j < d) u0 = fmaf(xv[j], ds[j], u0);
        const float* t = tab + ms[3];
        float h;
        if (ms[0] == 1) {
            int i;
            float w;
            if (u0 != u0) h = u0;
            else if (!grid_pos(u0, ds[16], ds[17], ds[18], ms[1], i, w)) h = 0.0f;
            else h = t[i] * (1.0f - w) + t[i + 1] * w;
        } else {
            float u1 = 0.0f;
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j)
                if (j < d) u1 = fmaf(xv[j], ds[8 + j], u1);
            int i, k;
            float wx, wy;
            const int By = ms[2];
            if (u0 != u0 || u1 != u1) h = u0 + u1;
            else if (!grid_pos(u0, ds[16], ds[17], ds[18], ms[1], i, wx) || !grid_pos(u1, ds[19], ds[20], ds[21], By, k, wy))
                h = 0.0f;
            else {
                const float* r0 = t + i * By + k;
                const float* r1 = r0 + By;
                h = r0[0] * ((1.0f - wx) * (1.0f - wy)) + r0[1] * ((1.0f - wx) * wy) + r1[0] * (wx * (1.0f - wy))
                    + r1[1] * (wx * wy);
            }
        }
        prob *= clamp_factor(h);
    }
    return prob;
}

__device__ __forceinline__ float prior_factor(const float (&xv)[MENT_DMAX], int d, int kind, float a, float lognorm) {
    if (kind == 1) {                        // exp(prior.Gaussian.log_prob(x))
        float q = 0.0f;
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j)
            if (j < d) q = q + xv[j] * xv[j];
        return expf(lognorm - (0.5f * q) / (a * a));
    }
    if (kind == 2) {                        // uniform density on [-a, a]^d
        bool inside = true;
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j)
            if (j < d) inside = inside && fabsf(xv[j]) <= a;
        return inside ? expf(lognorm) : 0.0f;
    }
    return 1.0f;
}

// the density at xv: the bits mf_ment_prob returns (desc / meta / tab as stage_slots returns them)
__device__ __forceinline__ float prob_point(const float (&xv)[MENT_DMAX], int d, const float* __restrict__ desc,
                                            const int* __restrict__ meta, const float* __restrict__ tab, const SlotArgs& sa) {
    float prob = slot_product(xv, d, desc, meta, tab, sa.nslot);
    if (prob != 0.0f) prob *= prior_factor(xv, d, sa.prior_kind, sa.prior_a, sa.prior_lognorm);
    return prob;
}

// Descriptors (+ tables when TAB_LDS) into LDS; returns the table pointer every lane reads.
template <bool TAB_LDS>
__device__ __forceinline__ const float* stage_slots(const SlotArgs& sa, float* lds, float*& desc, int*& meta) {
    desc = lds;
    meta = reinterpret_cast<int*>(lds + sa.nslot * MENT_DESC);
    for (int i = threadIdx.x; i < sa.nslot * MENT_DESC; i += MENT_BLOCK) desc[i] = sa.desc[i];
    for (int i = threadIdx.x; i < sa.nslot * MENT_META; i += MENT_BLOCK) meta[i] = sa.meta[i];
    float* tl = lds + sa.nslot * (MENT_DESC + MENT_META);
    if (TAB_LDS)
        for (int i = threadIdx.x; i < sa.table_floats; i += MENT_BLOCK) tl[i] = sa.tables[i];
    __syncthreads();
    return TAB_LDS ? tl : sa.tables;
}

// Launches the tables-in-LDS or the tables-in-global-memory instance of a kernel template, as slot_geometry decided.
#define MF_LAUNCH_TAB(tab_lds, k_lds, k_global, grid, block, smem, stream, ...)  \
    do {                                                                          \
        if (tab_lds) {                                                            \
            MF_ALLOW_DYN_SMEM(k_lds, smem);                                       \
            MF_LAUNCH((k_lds), grid, block, smem, stream, __VA_ARGS__);           \
        } else {                                                                  \
            MF_ALLOW_DYN_SMEM(k_global, smem);                                    \
            MF_LAUNCH((k_global), grid, block, smem, stream, __VA_ARGS__);        \
        }                                                                         \
    } while (0)

// checks the slot arguments; *lds_bytes = dynamic LDS of the launch, *tab_lds = whether the tables go there
static int slot_geometry(int d, int nslot, int64_t table_floats, int prior_kind, size_t* lds_bytes, bool* tab_lds) {
    if (d < 1 || d > MENT_DMAX) return fail("MENT kernels support 1 <= ndim <= %d (got %d)", MENT_DMAX, d);
    if (nslot < 0 || nslot > MENT_MAX_SLOTS) return fail("MENT kernels take 0..%d slots per launch (got %d)", MENT_MAX_SLOTS, nslot);
    if (table_floats < 0 || table_floats >= (int64_t)1 << 31) return fail("bad table size %lld", (long long)table_floats);
    if (prior_kind < 0 || prior_kind > 2) return fail("bad prior kind %d", prior_kind);
    const int64_t desc = (int64_t)nslot * (MENT_DESC + MENT_META);
    *tab_lds = desc + table_floats <= MENT_TAB_LDS_FLOATS;
    *lds_bytes = sizeof(float) * (size_t)(desc + (*tab_lds ? table_floats : 0));
    if (*lds_bytes == 0) *lds_bytes = sizeof(float);
    return 0;
}

static SlotArgs slot_args(int nslot, const float* desc, const int32_t* meta, const float* tables, int64_t table_floats,
                          int prior_kind, float prior_a, float prior_lognorm) {
    SlotArgs sa;
    sa.desc = desc;
    sa.meta = meta;
    sa.tables = tables;
    sa.nslot = nslot;
    sa.table_floats = (int)table_floats;
    sa.prior_kind = prior_kind;
    sa.prior_a = prior_a;
    sa.prior_lognorm = prior_lognorm;
    return sa;
}

}  // namespace mf
