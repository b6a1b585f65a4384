// Classical MENT (maximum-entropy tomography) on gfx950: the product of Lagrange functions at particles, at the cells of an
// implicit tensor grid or at the points of a line / plane integral, and inverse-CDF sampling of a gridded density.
//
// Reference chain replaced (paths relative to austin-hoover/ment-flow):
//   LagrangeFunction.__call__ (scipy RegularGridInterpolator, linear)   mentflow/ment.py:20-52
//   MENT.prob / MENT._simulate_integrate                                 mentflow/ment.py:225-318
//   GridSampler.__call__ / sample_hist / sample_hist_bins                mentflow/sample.py:26-113
//
// Slots.  One slot is one (transform, diagnostic) pair: one or two projection rows u = r . x (the rows of the transform's
// matrix the diagnostic reads), a uniform grid of bin centres per projected axis and the slot's table of Lagrange-function
// values at those centres.  Every evaluation point runs through ALL slots of a launch (the density is their product), so a
// grid is read or written once per evaluation.  Descriptors (rows, grids) always sit in LDS; the concatenated tables too when
// they fit next to them in MENT_TAB_LDS_FLOATS, else they are read from global memory, where a few hundred KiB stay L2-resident.
// h(u) is linear (1-D) or bilinear (2-D) on the centre grid, 0 outside the closed hull [c_0, c_{B-1}] (scipy's fill_value=0,
// bounds_error=False), NaN for a NaN coordinate, and each factor is clamped to [0, 1e10] (ment.py:231).  A point whose product
// has reached 0 skips its remaining slots: its projections all carry the same x, so a NaN coordinate already made the first
// factor NaN.
//
// Determinism: no float atomics anywhere.  Sums (per-block sums of the sampling weights, per-bin integrals) are fp64, each
// thread's share in a fixed order, then a fixed-shape tree per block, then a fixed-order pass over the blocks: every output
// is bitwise reproducible from launch to launch.
#include "ment_slots.h"   // SlotArgs, prob_point, stage_slots, slot_geometry, slot_args, MF_LAUNCH_TAB

namespace mf {

constexpr int MENT_CELLS_PER_BLOCK = 1024;   // cells per sampling block (4 per thread)
constexpr int MENT_INT_PER_BLOCK = 4096;     // integration points per workgroup of the integrate kernel
constexpr int MENT_SCAN_THREADS = 1024;

__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = MENT_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// sampling weight of a cell: sample_hist_bins draws from ravel(hist) + 1e-15 (sample.py:28)
__device__ __forceinline__ double cell_weight(float p) { return (double)(p + 1.0e-15f); }

// ------------------------------------------------------------------------------------------------ K1: explicit points
template <bool TAB_LDS>
__global__ __launch_bounds__(MENT_BLOCK) void ment_prob_points_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                      SlotArgs sa, int multiply, float* __restrict__ out) {
    MF_DYN_SMEM(float, lds);
    float* desc;
    int* meta;
    const float* tab = stage_slots<TAB_LDS>(sa, lds, desc, meta);
    for (int64_t p = (int64_t)blockIdx.x * MENT_BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * MENT_BLOCK) {
        float xv[MENT_DMAX];
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) xv[j] = (j < d) ? x[p * d + j] : 0.0f;
        const float prob = prob_point(xv, d, desc, meta, tab, sa);
        out[p] = multiply ? out[p] * prob : prob;
    }
}

// ------------------------------------------------------------------------------------------------ K2: implicit grid
struct GridArgs {
    const float* coords;          // concatenated per-axis cell centres
    unsigned shape[MENT_DMAX];
    int off[MENT_DMAX];
    int d;
    int64_t ncells;               // < 2^31
};

__device__ __forceinline__ void grid_point(const GridArgs& g, unsigned q, float (&xv)[MENT_DMAX]) {
#pragma unroll
    for (int j = MENT_DMAX - 1; j >= 0; --j) {
        if (j < g.d) {
            const unsigned k = q % g.shape[j];
            q /= g.shape[j];
            xv[j] = g.coords[g.off[j] + (int)k];
        } else {
            xv[j] = 0.0f;
        }
    }
}

// block b covers cells [b * 1024, (b + 1) * 1024): thread t takes b * 1024 + t + 256 k, k = 0..3 (coalesced stores)
template <bool TAB_LDS>
__global__ __launch_bounds__(MENT_BLOCK) void ment_prob_grid_kernel(GridArgs g, SlotArgs sa, float* __restrict__ prob_out,
                                                                    double* __restrict__ block_sums) {
    MF_DYN_SMEM(float, lds);
    __shared__ double red[MENT_BLOCK];
    float* desc;
    int* meta;
    const float* tab = stage_slots<TAB_LDS>(sa, lds, desc, meta);
    const int64_t base = (int64_t)blockIdx.x * MENT_CELLS_PER_BLOCK;
    double acc = 0.0;
    for (int k = 0; k < MENT_CELLS_PER_BLOCK / MENT_BLOCK; ++k) {
        const int64_t q = base + threadIdx.x + (int64_t)k * MENT_BLOCK;
        if (q >= g.ncells) break;
        float xv[MENT_DMAX];
        grid_point(g, (unsigned)q, xv);
        const float prob = prob_point(xv, g.d, desc, meta, tab, sa);
        prob_out[q] = prob;
        acc += cell_weight(prob);
    }
    const double t = block_sum_f64(acc, red);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = t;
}

// the same per-block sums of the sampling weights for a given histogram (sample_hist on any tensor)
__global__ __launch_bounds__(MENT_BLOCK) void ment_block_sums_kernel(const float* __restrict__ prob, int64_t ncells,
                                                                     double* __restrict__ block_sums) {
    __shared__ double red[MENT_BLOCK];
    const int64_t base = (int64_t)blockIdx.x * MENT_CELLS_PER_BLOCK;
    double acc = 0.0;
    for (int k = 0; k < MENT_CELLS_PER_BLOCK / MENT_BLOCK; ++k) {
        const int64_t q = base + threadIdx.x + (int64_t)k * MENT_BLOCK;
        if (q >= ncells) break;
        acc += cell_weight(prob[q]);
    }
    const double t = block_sum_f64(acc, red);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = t;
}

// ------------------------------------------------------------------------------------------------ K3: inverse CDF
// One workgroup: prefix[b] = sum of block_sums[0..b) (fp64), prefix[nb] = total.  Thread t owns a contiguous segment, its
// segment totals are scanned by thread 0 in order, then each thread writes its segment's prefixes: a fixed order.
__global__ __launch_bounds__(MENT_SCAN_THREADS) void ment_prefix_kernel(const double* __restrict__ block_sums, int64_t nb,
                                                                        double* __restrict__ prefix) {
    __shared__ double seg[MENT_SCAN_THREADS];
    const int64_t per = (nb + MENT_SCAN_THREADS - 1) / MENT_SCAN_THREADS;
    const int64_t a = (int64_t)threadIdx.x * per;
    const int64_t b = min(a + per, nb);
    double s = 0.0;
    for (int64_t i = a; i < b; ++i) s += block_sums[i];
    seg[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double run = 0.0;
        for (int i = 0; i < MENT_SCAN_THREADS; ++i) {
            const double v = seg[i];
            seg[i] = run;
            run += v;
        }
        prefix[nb] = run;
    }
    __syncthreads();
    double run = seg[threadIdx.x];
    for (int64_t i = a; i < b; ++i) {
        prefix[i] = run;
        run += block_sums[i];
    }
}

struct SampleArgs {
    unsigned shape[MENT_DMAX];
    int eoff[MENT_DMAX];         // offsets of the per-axis edge arrays (shape + 1 each) in `edges`
    int d;
    int noise;
};

__global__ __launch_bounds__(MENT_BLOCK) void ment_sample_kernel(const float* __restrict__ prob, int64_t ncells,
                                                                 const double* __restrict__ prefix, int64_t nb,
                                                                 const float* __restrict__ edges, SampleArgs sa,
                                                                 const float* __restrict__ rnd, int64_t size,
                                                                 float* __restrict__ x) {
    const int stride = 1 + 2 * sa.d;
    for (int64_t s = (int64_t)blockIdx.x * MENT_BLOCK + threadIdx.x; s < size; s += (int64_t)gridDim.x * MENT_BLOCK) {
        const float* r = rnd + s * stride;
        const double target = (double)r[0] * prefix[nb];
        // largest block b with prefix[b] <= target
        int64_t lo = 0, hi = nb - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (prefix[mid] <= target) lo = mid;
            else hi = mid - 1;
        }
        const int64_t c0 = lo * MENT_CELLS_PER_BLOCK;
        const int64_t c1 = min(c0 + MENT_CELLS_PER_BLOCK, ncells);
        double run = prefix[lo];
        int64_t cell = c1 - 1;                     // rounding left the target beyond the last cell: take the last
        for (int64_t c = c0; c < c1; ++c) {
            run += cell_weight(prob[c]);
            if (target < run) {
                cell = c;
                break;
            }
        }
        unsigned q = (unsigned)cell;
        for (int j = sa.d - 1; j >= 0; --j) {
            const unsigned k = q % sa.shape[j];
            q /= sa.shape[j];
            const float lb = edges[sa.eoff[j] + (int)k];
            const float ub = edges[sa.eoff[j] + (int)k + 1];
            float v = lb + (ub - lb) * r[1 + j];                          // random_uniform(lb, ub)
            if (sa.noise) {
                const float delta = ub - lb;
                v += 0.5f * (-delta + (delta - (-delta)) * r[1 + sa.d + j]);   // 0.5 * random_uniform(-delta, delta)
            }
            x[s * sa.d + j] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------ K4: integrate
// Point (b, t) of a slot's line / plane integral: u[meas axes] = centres of bin b (ij order), u[other axes] = integration
// point t (ascending axes, ij order), x = Minv u.  Grid (nchunks, nbins); partial[b][chunk] in fp64.
struct IntArgs {
    float minv[MENT_DMAX * MENT_DMAX];
    const float* coords;         // concatenated per-axis coordinates, axis order 0..d-1
    int off[MENT_DMAX];
    unsigned count[MENT_DMAX];
    unsigned stride[MENT_DMAX];  // axis j's index = (bin or t) / stride[j] % count[j]
    unsigned meas_mask;          // bit j: axis j is measured (indexed by the bin), else integrated (by t)
    int d;
    int64_t npoints;             // integration points per bin (< 2^31)
    int nchunks;
};

template <bool TAB_LDS>
__global__ __launch_bounds__(MENT_BLOCK) void ment_integrate_kernel(IntArgs ia, SlotArgs sa, double* __restrict__ partial) {
    MF_DYN_SMEM(float, lds);
    __shared__ double red[MENT_BLOCK];
    float* desc;
    int* meta;
    const float* tab = stage_slots<TAB_LDS>(sa, lds, desc, meta);
    const unsigned bin = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * MENT_INT_PER_BLOCK;
    double acc = 0.0;
    for (int k = 0; k < MENT_INT_PER_BLOCK / MENT_BLOCK; ++k) {
        const int64_t t = t0 + threadIdx.x + (int64_t)k * MENT_BLOCK;
        if (t >= ia.npoints) break;
        float uv[MENT_DMAX];
#pragma unroll
        for (int j = 0; j < MENT_DMAX; ++j) {
            const unsigned q = ((ia.meas_mask >> j) & 1u) ? bin : (unsigned)t;
            uv[j] = (j < ia.d) ? ia.coords[ia.off[j] + (int)((q / ia.stride[j]) % ia.count[j])] : 0.0f;
        }
        float xv[MENT_DMAX];
#pragma unroll
        for (int i = 0; i < MENT_DMAX; ++i) {
            float v = 0.0f;
#pragma unroll
            for (int j = 0; j < MENT_DMAX; ++j)
                if (i < ia.d && j < ia.d) v = fmaf(ia.minv[i * MENT_DMAX + j], uv[j], v);
            xv[i] = v;
        }
        acc += (double)prob_point(xv, ia.d, desc, meta, tab, sa);
    }
    const double s = block_sum_f64(acc, red);
    if (threadIdx.x == 0) partial[(int64_t)bin * ia.nchunks + blockIdx.x] = s;
}

__global__ __launch_bounds__(MENT_BLOCK) void ment_integrate_finish_kernel(const double* __restrict__ partial, int nbins,
                                                                           int nchunks, float* __restrict__ pred) {
    const int b = blockIdx.x * MENT_BLOCK + threadIdx.x;
    if (b >= nbins) return;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += partial[(int64_t)b * nchunks + c];
    pred[b] = (float)s;
}

static int grid_blocks(int64_t n, int per_block, int cap) {
    int64_t g = (n + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

}  // namespace mf

using namespace mf;

// ================================================================================================= C ABI
extern "C" int64_t mf_ment_blocks(int64_t ncells) {
    return ncells <= 0 ? 0 : (ncells + MENT_CELLS_PER_BLOCK - 1) / MENT_CELLS_PER_BLOCK;
}

extern "C" int64_t mf_ment_integrate_ws_doubles(int64_t nbins, int64_t npoints) {
    if (nbins <= 0 || npoints <= 0) return 0;
    return nbins * ((npoints + MENT_INT_PER_BLOCK - 1) / MENT_INT_PER_BLOCK);
}

extern "C" int mf_ment_prob(const float* x, int64_t n, int d, int nslot, const float* desc, const int32_t* meta,
                            const float* tables, int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm,
                            int multiply, float* out, void* stream) {
    size_t smem;
    bool tl;
    if (slot_geometry(d, nslot, table_floats, prior_kind, &smem, &tl)) return 1;
    if (n < 0) return fail("negative point count");
    if (n == 0) return 0;
    const SlotArgs sa = slot_args(nslot, desc, meta, tables, table_floats, prior_kind, prior_a, prior_lognorm);
    const int G = grid_blocks(n, MENT_BLOCK, NUM_CU * 16);
    MF_LAUNCH_TAB(tl, ment_prob_points_kernel<true>, ment_prob_points_kernel<false>, G, MENT_BLOCK, smem, stream, x, n, d, sa,
                  multiply, out);
    return check_launch("mf_ment_prob");
}

static int grid_shape(int d, const int64_t* shape, int64_t* ncells) {
    if (d < 1 || d > MENT_DMAX) return fail("MENT grids have 1..%d axes (got %d)", MENT_DMAX, d);
    int64_t n = 1;
    for (int j = 0; j < d; ++j) {
        if (shape[j] < 1) return fail("grid axis %d has %lld cells", j, (long long)shape[j]);
        n *= shape[j];
        if (n > 2147483647LL) return fail("MENT grids hold at most 2^31 - 1 cells");
    }
    *ncells = n;
    return 0;
}

extern "C" int mf_ment_prob_grid(const float* coords, const int64_t* shape, int d, int nslot, const float* desc,
                                 const int32_t* meta, const float* tables, int64_t table_floats, int prior_kind, float prior_a,
                                 float prior_lognorm, float* prob, double* block_sums, void* stream) {
    size_t smem;
    bool tl;
    int64_t ncells;
    if (slot_geometry(d, nslot, table_floats, prior_kind, &smem, &tl) || grid_shape(d, shape, &ncells)) return 1;
    GridArgs g;
    int off = 0;
    for (int j = 0; j < MENT_DMAX; ++j) {
        g.shape[j] = j < d ? (unsigned)shape[j] : 1u;
        g.off[j] = off;
        if (j < d) off += (int)shape[j];
    }
    g.coords = coords;
    g.d = d;
    g.ncells = ncells;
    const SlotArgs sa = slot_args(nslot, desc, meta, tables, table_floats, prior_kind, prior_a, prior_lognorm);
    const int64_t nb = mf_ment_blocks(ncells);
    MF_LAUNCH_TAB(tl, ment_prob_grid_kernel<true>, ment_prob_grid_kernel<false>, dim3((unsigned)nb), MENT_BLOCK, smem, stream, g,
                  sa, prob, block_sums);
    return check_launch("mf_ment_prob_grid");
}

extern "C" int mf_ment_block_sums(const float* prob, int64_t ncells, double* block_sums, void* stream) {
    if (ncells < 1 || ncells > 2147483647LL) return fail("MENT grids hold 1 .. 2^31 - 1 cells (got %lld)", (long long)ncells);
    MF_LAUNCH(ment_block_sums_kernel, dim3((unsigned)mf_ment_blocks(ncells)), MENT_BLOCK, 0, stream, prob, ncells, block_sums);
    return check_launch("mf_ment_block_sums");
}

extern "C" int mf_ment_sample(const float* prob, const int64_t* shape, int d, const double* block_sums, double* prefix,
                              const float* edges, const float* rnd, int64_t size, int noise, float* x, void* stream) {
    int64_t ncells;
    if (grid_shape(d, shape, &ncells)) return 1;
    if (size < 0) return fail("negative sample count");
    const int64_t nb = mf_ment_blocks(ncells);
    MF_LAUNCH(ment_prefix_kernel, 1, MENT_SCAN_THREADS, 0, stream, block_sums, nb, prefix);
    if (check_launch("mf_ment_sample (prefix)")) return 1;
    if (size == 0) return 0;
    SampleArgs sa;
    int off = 0;
    for (int j = 0; j < MENT_DMAX; ++j) {
        sa.shape[j] = j < d ? (unsigned)shape[j] : 1u;
        sa.eoff[j] = off;
        if (j < d) off += (int)shape[j] + 1;
    }
    sa.d = d;
    sa.noise = noise != 0;
    MF_LAUNCH(ment_sample_kernel, grid_blocks(size, MENT_BLOCK, NUM_CU * 16), MENT_BLOCK, 0, stream, prob, ncells,
              (const double*)prefix, nb, edges, sa, rnd, size, x);
    return check_launch("mf_ment_sample");
}

extern "C" int mf_ment_integrate(int d, const float* minv, const float* coords, const int64_t* counts, int nmeas,
                                 const int32_t* meas_axes, int nslot, const float* desc, const int32_t* meta,
                                 const float* tables, int64_t table_floats, int prior_kind, float prior_a, float prior_lognorm,
                                 double* partial, float* pred, void* stream) {
    size_t smem;
    bool tl;
    if (slot_geometry(d, nslot, table_floats, prior_kind, &smem, &tl)) return 1;
    if (nmeas < 1 || nmeas > 2 || nmeas > d) return fail("integrate: 1 or 2 measured axes (got %d of %d)", nmeas, d);
    IntArgs ia;
    unsigned mask = 0;
    for (int k = 0; k < nmeas; ++k) {
        const int ax = meas_axes[k];
        if (ax < 0 || ax >= d || ((mask >> ax) & 1u)) return fail("integrate: bad measured axis %d", ax);
        mask |= 1u << ax;
    }
    int off = 0;
    int64_t nbins = 1, npoints = 1;
    for (int j = 0; j < MENT_DMAX; ++j) {
        ia.off[j] = off;
        ia.count[j] = 1u;
        ia.stride[j] = 1u;
        if (j >= d) continue;
        if (counts[j] < 1) return fail("integrate: axis %d has %lld points", j, (long long)counts[j]);
        ia.count[j] = (unsigned)counts[j];
        off += (int)counts[j];
        if ((mask >> j) & 1u) nbins *= counts[j];
        else npoints *= counts[j];
        if (nbins > 65535 || npoints > 2147483647LL) return fail("integrate: too many bins or integration points");
    }
    // ij order within each group: the measured axes in the order given (first slowest), the integrated ones ascending
    int64_t st = 1;
    for (int k = nmeas - 1; k >= 0; --k) {
        ia.stride[meas_axes[k]] = (unsigned)st;
        st *= counts[meas_axes[k]];
    }
    st = 1;
    for (int j = d - 1; j >= 0; --j) {
        if ((mask >> j) & 1u) continue;
        ia.stride[j] = (unsigned)st;
        st *= counts[j];
    }
    ia.meas_mask = mask;
    for (int i = 0; i < MENT_DMAX * MENT_DMAX; ++i) ia.minv[i] = 0.0f;
    ia.coords = coords;
    ia.d = d;
    ia.npoints = npoints;
    ia.nchunks = (int)((npoints + MENT_INT_PER_BLOCK - 1) / MENT_INT_PER_BLOCK);
    // Minv arrives as a host [d, d] array: it travels in the kernel arguments
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) ia.minv[i * MENT_DMAX + j] = minv[i * d + j];
    const SlotArgs sa = slot_args(nslot, desc, meta, tables, table_floats, prior_kind, prior_a, prior_lognorm);
    const dim3 grid((unsigned)ia.nchunks, (unsigned)nbins);
    MF_LAUNCH_TAB(tl, ment_integrate_kernel<true>, ment_integrate_kernel<false>, grid, MENT_BLOCK, smem, stream, ia, sa, partial);
    if (check_launch("mf_ment_integrate")) return 1;
    MF_LAUNCH(ment_integrate_finish_kernel, grid_blocks(nbins, MENT_BLOCK, 1 << 20), MENT_BLOCK, 0, stream,
              (const double*)partial, (int)nbins, ia.nchunks, pred);
    return check_launch("mf_ment_integrate (finish)");
}
