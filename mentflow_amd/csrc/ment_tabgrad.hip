// Gradient of classical MENT's log-density with respect to its Lagrange TABLES on gfx950: the adjoint of mf_ment_logprob
// (ment_logp.hip) in `tables`.  The reference has no counterpart (its interpolators are scipy on the host).
//
// In the log-parametrisation the gradient is a histogram of RESPONSIBILITIES.  A point in cell (i, w) of a 1-D slot sees
// h = a (1 - w) + b w with the cell's two node values a, b, and
//     d log h / d log a = a (1 - w) / h,      d log h / d log b = b w / h,
// both in [0, 1], summing to 1 (four such terms for a 2-D slot).  So
//     grad_log[e] = sum_n weight[n] rho_e(n),      grad_tab[e] = grad_log[e] / tables[e].
//
// One lane per point, striding as ment_logprob_kernel does.  Projections and cells come from the fmaf chain and the grid_pos
// calls of slot_value (ment_slots.h), restated here because the kernel needs the cell itself: the cell is that of the forward.  A row takes part iff its
// logp (as the forward returned it) is finite and its weight is not zero, so every slot of a live row has a positive factor.
//
// Accumulation is FIXED POINT (kde.hip's scheme, signed): with P = 2^ceil(log2 wmax) >= max |weight| and
// F = min(50, 62 - ceil(log2 max(n, 2))), a contribution is round((weight / P) rho 2^F), at most 2^F in magnitude, added as a
// two's-complement 64-bit integer: n of them stay below 2^62.  Integer sums do not depend on their order: the result is bitwise
// reproducible and independent of the grid.  No floating-point atomics.  A finishing kernel scales by P 2^-F in fp64 and
// rounds to fp32 once.
//
// Two instances, chosen by the rule that puts the forward's tables into LDS (slot_geometry):
//   LDS     descriptors, tables and a 64-bit integer image of the tables in LDS; 64-bit LDS integer atomics (3.4-3.9
//           lane-ops/clk/CU with 16 waves per CU, 2.6-2.75 with 4: measured, see the top of kde.hip), one 64-bit integer global
//           atomic per non-zero entry and workgroup at the end.
//   global  descriptors in LDS, tables read from global memory, 64-bit integer global atomics straight into `acc`.
#include <float.h>

#include "ment_slots.h"

namespace mf {

typedef unsigned long long u64;

// LDS instance.  The rule is the forward's (descriptors + tables <= MENT_TAB_LDS_FLOATS = 40 KiB), so the image (two words per
// table entry) is at most 80 KiB and a workgroup at most 120 KiB of the CU's 160 KiB: no second budget to keep in step.  The C4
// shape (100 slots x 64 bins: 11.2 KB descriptors, 25.6 KB tables, 51.2 KB image = 88 KB) leaves room for ONE workgroup per
// CU, and the kernel is LDS-atomic bound, which lives on waves in flight (kde.hip: 16 waves per CU reach the full atomic rate,
// 4 waves three quarters of it) - so the workgroup is 1024 lanes: 16 waves per CU from a single workgroup.  Registers are no
// constraint at that size (the limit is 128 VGPRs).  The global instance has no image and keeps MENT_BLOCK.
constexpr int TABGRAD_LDS_BLOCK = 1024;

// ceil(log2 wmax) of a positive finite wmax; false for 0, NaN and inf (nothing is added then)
__device__ __forceinline__ bool tabgrad_exponent(float wmax, int& pe) {
    pe = 0;
    if (!(wmax > 0.0f && wmax <= FLT_MAX)) return false;
    int e;
    const float m = frexpf(wmax, &e);                      // wmax = m 2^e, m in [1/2, 1)
    pe = (m == 0.5f) ? e - 1 : e;
    return true;
}

// one responsibility into the integer image: wn = weight / P in [-1, 1]
__device__ __forceinline__ void tabgrad_add(u64* __restrict__ img, int e, float wn, float rho, int F) {
    rho = fminf(fmaxf(rho, 0.0f), 1.0f);                   // a no-op up to rounding for non-negative tables; NaN -> 0
    const long long c = (long long)rintf(ldexpf(wn * rho, F));
    if (c != 0) atomicAdd(img + e, (u64)c);
}

template <bool LDS, int BLOCK>
__global__ __launch_bounds__(BLOCK) void ment_tabgrad_kernel(const float* __restrict__ x, int64_t n, int d, SlotArgs sa,
                                                             const float* __restrict__ logp, const float* __restrict__ weight,
                                                             const float* __restrict__ wmax, int F, int img_offset,
                                                             u64* __restrict__ acc, int32_t* __restrict__ status) {
    MF_DYN_SMEM(float, lds);
    float* desc = lds;
    int* meta = reinterpret_cast<int*>(lds + sa.nslot * MENT_DESC);
    for (int i = threadIdx.x; i < sa.nslot * MENT_DESC; i += BLOCK) desc[i] = sa.desc[i];
    for (int i = threadIdx.x; i < sa.nslot * MENT_META; i += BLOCK) meta[i] = sa.meta[i];
    const float* tab = sa.tables;
    u64* img = acc;
    if (LDS) {
        float* tl = lds + sa.nslot * (MENT_DESC + MENT_META);
        img = reinterpret_cast<u64*>(lds + img_offset);   // img_offset is even: 8-byte aligned
        for (int i = threadIdx.x; i < sa.table_floats; i += BLOCK) {
            tl[i] = sa.tables[i];
            img[i] = 0;
        }
        tab = tl;
    }
    __syncthreads();
    int pe;
    const bool active = tabgrad_exponent(wmax[0], pe);
    bool poison = false;
    for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * BLOCK) {
        const float lp = logp[p], wt = weight[p];
        if (lp != lp) {                                    // a NaN row: poison unless the caller masked it (NaN != 0 holds)
            poison = poison || wt != 0.0f;
            continue;
        }
        if (!(fabsf(lp) <= FLT_MAX)) continue;             // outside the support: nothing, whatever the weight
        if (!(fabsf(wt) <= FLT_MAX)) {
            poison = true;
            continue;
        }
        if (wt == 0.0f || !active) continue;
        const float wn = fminf(fmaxf(ldexpf(wt, -pe), -1.0f), 1.0f);      // exact; the clamp only guards a wmax that is too small
        float xv[MENT_DMAX];
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) xv[j] = (j < d) ? x[p * d + j] : 0.0f;
        for (int s = 0; s < sa.nslot; ++s) {
            const float* ds = desc + s * MENT_DESC;
            const int* ms = meta + s * MENT_META;
            float u0 = 0.0f;
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j)
                if (j < d) u0 = fmaf(xv[j], ds[j], u0);
            const int off = ms[3];
            if (ms[0] == 1) {
                int i;
                float w;
                if (u0 != u0 || !grid_pos(u0, ds[16], ds[17], ds[18], ms[1], i, w)) continue;
                const float a = tab[off + i], b = tab[off + i + 1];
                const float h = a * (1.0f - w) + b * w;
                if (!(h > 0.0f && h < 1.0e10f)) continue;  // on the upper clamp a constant; h <= 0 or NaN guards the division
                const float r = __frcp_rn(h);
                tabgrad_add(img, off + i, wn, a * (1.0f - w) * r, F);
                tabgrad_add(img, off + i + 1, wn, b * w * r, F);
            } else {
                float u1 = 0.0f;
#pragma unroll
                for (int j = 0; j < MENT_DMAX; ++j)
                    if (j < d) u1 = fmaf(xv[j], ds[8 + j], u1);
                int i, k;
                float wx, wy;
                const int By = ms[2];
                if (u0 != u0 || u1 != u1) continue;
                if (!grid_pos(u0, ds[16], ds[17], ds[18], ms[1], i, wx) || !grid_pos(u1, ds[19], ds[20], ds[21], By, k, wy))
                    continue;
                const int e = off + i * By + k;
                const float c00 = tab[e] * ((1.0f - wx) * (1.0f - wy)), c01 = tab[e + 1] * ((1.0f - wx) * wy);
                const float c10 = tab[e + By] * (wx * (1.0f - wy)), c11 = tab[e + By + 1] * (wx * wy);
                const float h = c00 + c01 + c10 + c11;
                if (!(h > 0.0f && h < 1.0e10f)) continue;
                const float r = __frcp_rn(h);
                tabgrad_add(img, e, wn, c00 * r, F);
                tabgrad_add(img, e + 1, wn, c01 * r, F);
                tabgrad_add(img, e + By, wn, c10 * r, F);
                tabgrad_add(img, e + By + 1, wn, c11 * r, F);
            }
        }
    }
    if (poison) status[0] = 1;                             // every writer stores the same value
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < sa.table_floats; i += BLOCK) {
            const u64 v = img[i];
            if (v != 0) atomicAdd(acc + i, v);             // one integer atomic per non-zero entry and workgroup
        }
    }
}

__global__ __launch_bounds__(MENT_BLOCK) void ment_tabgrad_zero_kernel(u64* __restrict__ acc, int64_t count,
                                                                       int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * MENT_BLOCK + threadIdx.x;
    if (i < count) acc[i] = 0;
    if (i == 0) status[0] = 0;
}

// acc (2^(pe - F) units, two's complement) -> grad_log, grad_tab; wmax == NULL stands for 0 (no points)
__global__ __launch_bounds__(MENT_BLOCK) void ment_tabgrad_finish_kernel(const u64* __restrict__ acc, int64_t count,
                                                                         const float* __restrict__ tables,
                                                                         const float* __restrict__ wmax, int F,
                                                                         float* __restrict__ grad_log,
                                                                         float* __restrict__ grad_tab,
                                                                         int32_t* __restrict__ status) {
    const int64_t i = (int64_t)blockIdx.x * MENT_BLOCK + threadIdx.x;
    const float wm = wmax ? wmax[0] : 0.0f;
    int pe;
    const bool active = tabgrad_exponent(wm, pe);
    if (i == 0 && !(fabsf(wm) <= FLT_MAX)) status[0] = 1;  // NaN or inf: a non-finite weight on a live row
    if (i >= count) return;
    const double g = active ? ldexp((double)(long long)acc[i], pe - F) : 0.0;
    grad_log[i] = (float)g;
    if (grad_tab) {
        const float t = tables[i];
        grad_tab[i] = t > 0.0f ? (float)(g / (double)t) : 0.0f;    // a zero entry is outside MENT's support and stays there
    }
}

}  // namespace mf

using namespace mf;

extern "C" int mf_ment_logprob_tables_bwd(const float* x, int64_t n, int d, int nslot, const float* desc, const int32_t* meta,
                                          const float* tables, int64_t table_floats, const float* logp, const float* weight,
                                          const float* wmax, unsigned long long* acc, float* grad_log, float* grad_tab,
                                          int32_t* status, void* stream) {
    size_t smem;
    bool tl;
    if (slot_geometry(d, nslot, table_floats, 0, &smem, &tl)) return 1;
    if (n < 0) return fail("negative point count");
    const int zb = table_floats > 0 ? (int)((table_floats + MENT_BLOCK - 1) / MENT_BLOCK) : 1;
    MF_LAUNCH(ment_tabgrad_zero_kernel, zb, MENT_BLOCK, 0, stream, acc, table_floats, status);
    int lg = 1;                                            // ceil(log2 max(n, 2))
    while (lg < 62 && ((int64_t)1 << lg) < n) ++lg;
    const int F = 62 - lg < 50 ? 62 - lg : 50;
    if (n > 0) {
        const SlotArgs sa = slot_args(nslot, desc, meta, tables, table_floats, 0, 0.0f, 0.0f);
        if (tl) {
            const int img_offset = (int)((smem / sizeof(float) + 1) & ~(size_t)1);
            const size_t bytes = sizeof(float) * (size_t)img_offset + sizeof(u64) * (size_t)table_floats;
            int64_t per_cu = (int64_t)(160 * 1024 / bytes);
            if (per_cu > 2) per_cu = 2;                    // 2048 lanes: the CU's 32 waves
            int64_t blocks = (n + TABGRAD_LDS_BLOCK - 1) / TABGRAD_LDS_BLOCK;
            if (blocks > NUM_CU * per_cu) blocks = NUM_CU * per_cu;
            MF_ALLOW_DYN_SMEM((ment_tabgrad_kernel<true, TABGRAD_LDS_BLOCK>), bytes);
            MF_LAUNCH((ment_tabgrad_kernel<true, TABGRAD_LDS_BLOCK>), (int)blocks, TABGRAD_LDS_BLOCK, bytes, stream, x, n, d, sa,
                      logp, weight, wmax, F, img_offset, acc, status);
        } else {
            int64_t blocks = (n + MENT_BLOCK - 1) / MENT_BLOCK;
            if (blocks > NUM_CU * 8) blocks = NUM_CU * 8;
            MF_ALLOW_DYN_SMEM((ment_tabgrad_kernel<false, MENT_BLOCK>), smem);
            MF_LAUNCH((ment_tabgrad_kernel<false, MENT_BLOCK>), (int)blocks, MENT_BLOCK, smem, stream, x, n, d, sa, logp, weight,
                      wmax, F, 0, acc, status);
        }
    }
    const int fb = table_floats > 0 ? (int)((table_floats + MENT_BLOCK - 1) / MENT_BLOCK) : 1;
    MF_LAUNCH(ment_tabgrad_finish_kernel, fb, MENT_BLOCK, 0, stream, (const u64*)acc, table_floats, tables,
              n > 0 ? wmax : (const float*)nullptr, F, grad_log, grad_tab, status);
    return check_launch("mf_ment_logprob_tables_bwd");
}
