// Sliced Wasserstein distance on gfx950: projections of two point clouds onto P directions, a segmented ascending key sort
// and the quantile integral  W_p^p = int_0^1 |F_u^-1(q) - F_v^-1(q)|^p dq  per projection.
//
// Reference chain replaced (paths relative to austin-hoover/ment-flow):
//   SlicedWassersteindDistance.__call__ (torch.matmul + POT's ot.lp.wasserstein_1d on the host)   mentflow/loss.py:20-42
//
// Kernels
//   swd_project_kernel      u[p, n] = sum_k x[n, k] dir[k, p], projection-major so that every projection is one contiguous
//                           segment; the directions sit in LDS, a particle row is read once and feeds all P outputs.
//   segsort_tile_kernel     floats -> order-preserving unsigned keys, one tile of 2^t keys per workgroup sorted by a bitonic
//                           network in registers (16 keys per thread) and LDS (the tail of a segment is padded with the
//                           largest key).
//   segsort_partition_kernel / segsort_merge_kernel
//                           ceil(log2(tiles)) merge-path passes between two buffers: one thread per output chunk finds the
//                           chunk's diagonal split by binary search, then a workgroup loads the two input pieces of its chunk
//                           into LDS, every thread splits its own diagonal there and merges 8 keys serially, and the chunk is
//                           stored coalesced.  The last stage maps the keys back to floats.
//   swd_cost_kernel / swd_cost_finish_kernel
//                           one thread per element of the larger set; element k owns the quantile interval (k/n, (k+1)/n] and
//                           meets at most two elements of the other set, with weights formed exactly in int64.
//
//   swd_cost_bwd_large_kernel / swd_cost_bwd_small_kernel / swd_project_bwd_kernel
//                           the adjoint: d dist / d (sorted projections) in closed form, stored at the position each key came
//                           from (the sort kernels are templates: the 64-bit instance carries key << 32 | position), and its
//                           back-projection onto the points.
//
// Ordering: torch.sort's.  NaN (any sign, any payload) maps to the largest key and comes out last as a quiet NaN; -0.0 sorts
// in front of +0.0 (they compare equal).  The keys-only sort has a unique result, and so has the pair sort, whose composites
// are unique (ties by ascending position): no stability argument needed for either.
//
// Determinism: no float atomics.  The sort is a fixed network + merges of unique outcome; the cost sums are fp64, each thread's
// share in a fixed order, a fixed-shape tree per workgroup, then a fixed-order pass over the workgroup partials (the pattern of
// ment_integrate): every output is bitwise reproducible from launch to launch.
#include "common.h"

namespace mf {

constexpr int SWD_DMAX = 8;                 // feature limit of the projection kernels (KDE_DMAX)
constexpr int SWD_BLOCK = 256;
constexpr int SWD_PCHUNK = 1024;            // directions staged per workgroup (32 KiB of LDS at most)
// Default tile: 4096 keys = 16 KiB of LDS per 256-thread workgroup, so eight workgroups (32 waves, the CU's limit) share the
// 160 KiB of a CU and hide each other's barriers and LDS round trips.
constexpr int SORT_TILE_LOG2 = 12;
// Default pair tile: 4096 composites = 34 KiB of LDS, four workgroups (16 waves, 4 per SIMD) per CU.  The network is bound by
// LDS bandwidth, which 4 waves per SIMD saturate for ds_read_b64 / ds_write_b64, and a 2^11 tile (8 workgroups) pays for its
// occupancy with one more merge pass over 16 bytes per element.  Swept as well: 100 x 50 000 keys take
// 0.251 / 0.232 / 0.219 ms at 2^10 / 2^11 / 2^12.
constexpr int SORT_PAIR_TILE_LOG2 = 12;
constexpr int SORT_TILE_LOG2_MIN = 4;
constexpr int SORT_TILE_LOG2_MAX = 12;         // 16 keys per thread, 256 threads
constexpr int SORT_MERGE_CHUNK = 2048;      // outputs per merge workgroup: 8.25 KiB of LDS
constexpr int SORT_MERGE_PER_THREAD = 8;    // keys each thread merges serially
constexpr int COST_PER_BLOCK = 4096;        // elements of the larger set per workgroup (16 per thread)
constexpr uint32_t KEY_LAST = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t key_map(float f) {
    if (f != f) return KEY_LAST;
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

__device__ __forceinline__ float key_unmap(uint32_t k) {
    const uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu);     // KEY_LAST -> 0x7FFFFFFF, a quiet NaN
    return __builtin_bit_cast(float, b);
}

// ------------------------------------------------------------------------------------------------ projection
__global__ __launch_bounds__(SWD_BLOCK) void swd_project_kernel(const float* __restrict__ x, int64_t n, int d,
                                                                const float* __restrict__ dir, int P, float* __restrict__ u) {
    MF_DYN_SMEM(float, sdir);               // [pc][SWD_DMAX], zero beyond d
    const int p0 = (int)blockIdx.y * SWD_PCHUNK;
    const int pc = min(P - p0, SWD_PCHUNK);
    for (int i = threadIdx.x; i < pc * SWD_DMAX; i += SWD_BLOCK) {
        const int p = i / SWD_DMAX, k = i % SWD_DMAX;
        sdir[i] = k < d ? dir[(int64_t)k * P + p0 + p] : 0.0f;
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * SWD_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * SWD_BLOCK) {
        float xv[SWD_DMAX];
#pragma unroll
        for (int k = 0; k < SWD_DMAX; ++k) xv[k] = (k < d) ? x[i * d + k] : 0.0f;
        for (int p = 0; p < pc; ++p) {
            const float* dp = sdir + p * SWD_DMAX;
            float acc = 0.0f;
#pragma unroll
            for (int k = 0; k < SWD_DMAX; ++k)
                if (k < d) acc = fmaf(xv[k], dp[k], acc);
            u[(int64_t)(p0 + p) * n + i] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------------------ segmented sort
// The kernels are templates on the element K they sort: uint32_t, the mapped key alone (mf_segsort_f32), or uint64_t, the
// composite  mapped key << 32 | position in the segment  (mf_segsort_pairs_f32).  Composites are unique, so their order is the
// mapped-key order with ties by ascending position whatever the network and the merges do; the tail of a segment is padded
// with KEY_LAST << 32 | 0xFFFFFFFF, behind every real NaN (positions stay below 2^31).
template <typename K> struct SortKey;
template <> struct SortKey<uint32_t> {
    static constexpr uint32_t PAD = KEY_LAST;
    static __device__ __forceinline__ uint32_t load(float f, int64_t) { return key_map(f); }
    static __device__ __forceinline__ void store(uint32_t* out, int32_t*, int64_t i, uint32_t k) {
        reinterpret_cast<float*>(out)[i] = key_unmap(k);
    }
};
template <> struct SortKey<uint64_t> {
    static constexpr uint64_t PAD = ((uint64_t)KEY_LAST << 32) | 0xFFFFFFFFu;
    static __device__ __forceinline__ uint64_t load(float f, int64_t pos) { return ((uint64_t)key_map(f) << 32) | (uint32_t)pos; }
    static __device__ __forceinline__ void store(uint64_t* out, int32_t* perm, int64_t i, uint64_t k) {
        reinterpret_cast<float*>(out)[i] = key_unmap((uint32_t)(k >> 32));      // the sorted values and the positions are
        perm[i] = (int32_t)(uint32_t)k;                                         // two fp32-sized arrays, not a K array
    }
};

// LDS index of element i, in elements.
// 4-byte keys: one spare word per 32: a thread that works on 16 (tile sort) or 8 (merge) consecutive keys then shares no
// bank with the other lanes of its 32-lane half (16 t + t / 2 and 8 t + t / 4 are distinct mod 64 for 32 consecutive t).
// 8-byte composites: one spare element per 16.  An element covers two banks, so a ds_read_b64 (64 banks, served per 32-lane
// half) is conflict-free where the 32 element slots are distinct mod 32, and a ds_write_b64 (32 banks, served per 16
// consecutive lanes) where 16 slots are distinct mod 16.  A thread on 16 consecutive elements sits at slot 17 t + r: distinct
// mod 32 over 32 consecutive t (17 is odd) and mod 16 over 16 (17 t = t); one spare per 32 would put lanes t and t + 1 of an
// even t on the same write banks (16 t + t / 2 = t / 2 mod 16).  Lanes on consecutive elements (the coalesced copies, the
// network's passes at strides >= 16) stay within one run of 16 per write group; in a full pass at stride 16 the two runs of a
// 32-lane half lie 256 elements = 272 slots = 16 mod 32 apart: conflict-free reads as well.  What remains: a read of 32
// consecutive elements crosses one spare and meets slot s again at s + 32 (one bank pair two-way), the short passes at stride
// 16 (fewer than 4 substages) put their two runs 2 .. 8 slots apart mod 32, and the merge's 8-element threads (8 t + t / 2)
// are conflict-free on their write-back only; their reads follow the data anyway.
template <typename K> __device__ __forceinline__ int lds_pad(int i) { return i + (i >> (sizeof(K) == 4 ? 5 : 4)); }
template <typename K> constexpr size_t lds_bytes(int count) { return sizeof(K) * (size_t)(count + (count >> (sizeof(K) == 4 ? 5 : 4))); }

// One substage of the bitonic network on the 16 keys a thread holds: pairs (r, r | 1 << sub); idx[r] is the key's position in
// the tile, ascending where the phase bit k of the position is clear.  `sub` is a constant after unrolling: v stays in registers.
template <typename K> __device__ __forceinline__ void bitonic_substage(K (&v)[16], const int (&idx)[16], int k, int sub) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (r & (1 << sub)) continue;
        const int q = r | (1 << sub);
        const K a = v[r], c = v[q];
        const bool swap = (a > c) == ((idx[r] & k) == 0);
        v[r] = swap ? c : a;
        v[q] = swap ? a : c;
    }
}

// The substages of phase k whose strides are the bit positions [b, b + nb) of the key position, nb <= 4, in one LDS round trip:
// the low nb bits of r run over those positions, the rest of r and the thread number the tile's 2^nb-key groups (groups of
// consecutive lanes are consecutive in LDS).
template <typename K> __device__ __forceinline__ void bitonic_pass(K* s, int k, int b, int nb) {
    const int t = threadIdx.x, nt = blockDim.x;
    K v[16];
    int idx[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int e = (r >> nb) * nt + t;
        idx[r] = ((e >> b) << (b + nb)) | ((r & ((1 << nb) - 1)) << b) | (e & ((1 << b) - 1));
        v[r] = s[lds_pad<K>(idx[r])];
    }
#pragma unroll
    for (int sub = 3; sub >= 0; --sub)
        if (sub < nb) bitonic_substage(v, idx, k, sub);
#pragma unroll
    for (int r = 0; r < 16; ++r) s[lds_pad<K>(idx[r])] = v[r];
    __syncthreads();
}

// workgroup b sorts tile b % tiles of segment b / tiles; blockDim.x = T / 16, dynamic LDS: lds_bytes<K>(T).  With `unmap` (a
// single tile is the whole sort) the result goes out as floats, and positions into `perm` for composites, else as elements K.  Every thread holds 16
// keys in registers per LDS round trip: phases 2..16 run on 16 consecutive keys at once, every later phase 2^m takes
// ceil(m / 4) round trips (24 for a 4096-key tile where a key-pair-per-step network takes 78).  `out` may be `keys` (a tile
// is read whole before any of it is written), hence no __restrict__ here.
template <typename K>
__global__ __launch_bounds__(SWD_BLOCK) void segsort_tile_kernel(const float* keys, int64_t n, int tile_log2, int64_t tiles,
                                                                 int unmap, K* out, int32_t* perm) {
    MF_DYN_SMEM(K, s);
    const int T = 1 << tile_log2;
    const int nt = (int)blockDim.x;
    const int64_t seg = (int64_t)blockIdx.x / tiles;
    const int64_t t0 = ((int64_t)blockIdx.x % tiles) * T;
    const int cnt = (int)min((int64_t)T, n - t0);
    const int64_t base = seg * n + t0;
    for (int i = threadIdx.x; i < T; i += nt) s[lds_pad<K>(i)] = i < cnt ? SortKey<K>::load(keys[base + i], t0 + i) : SortKey<K>::PAD;
    __syncthreads();
    {
        K v[16];
        int idx[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            idx[r] = 16 * (int)threadIdx.x + r;
            v[r] = s[lds_pad<K>(idx[r])];
        }
#pragma unroll
        for (int k = 2; k <= 16; k <<= 1) {
#pragma unroll
            for (int sub = 3; sub >= 0; --sub)
                if ((1 << sub) < k) bitonic_substage(v, idx, k, sub);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) s[lds_pad<K>(idx[r])] = v[r];
        __syncthreads();
    }
    for (int m = 5; m <= tile_log2; ++m) {
        const int rem = m & 3;
        if (rem) bitonic_pass(s, 1 << m, m - rem, rem);
        for (int b = m - rem - 4; b >= 0; b -= 4) bitonic_pass(s, 1 << m, b, 4);
    }
    if (unmap) {
        for (int i = threadIdx.x; i < cnt; i += nt) SortKey<K>::store(out, perm, base + i, s[lds_pad<K>(i)]);
    } else {
        for (int i = threadIdx.x; i < cnt; i += nt) out[base + i] = s[lds_pad<K>(i)];
    }
}

// Geometry of output chunk c of a segment in a pass that merges runs of `run` keys: the pair of runs it lies in and its diagonals.
struct MergeChunk {
    int64_t pair0;      // start of the pair's left run in the segment
    int64_t la, lb;     // lengths of the left and right run (the right one may be short or empty)
    int64_t d0, d1;     // the chunk covers merged outputs [d0, d1) of the pair
};

__device__ __forceinline__ MergeChunk merge_chunk(int64_t c, int chunk, int64_t run, int64_t n) {
    MergeChunk m;
    const int64_t o0 = c * chunk;                            // chunk divides 2 * run: a chunk never straddles two pairs
    m.pair0 = o0 / (2 * run) * (2 * run);
    m.la = min(run, n - m.pair0);
    m.lb = min(run, n - m.pair0 - m.la);
    m.d0 = o0 - m.pair0;
    m.d1 = min(m.d0 + (int64_t)chunk, m.la + m.lb);
    return m;
}

// split[seg * chunks + c] = how many of the first d0 merged outputs of chunk c's pair come from the left run (ties: left first)
template <typename K>
__global__ __launch_bounds__(SWD_BLOCK) void segsort_partition_kernel(const K* __restrict__ in, int64_t n, int64_t run,
                                                                      int chunk, int64_t chunks, int64_t total,
                                                                      int32_t* __restrict__ split) {
    const int64_t g = (int64_t)blockIdx.x * SWD_BLOCK + threadIdx.x;
    if (g >= total) return;
    const int64_t seg = g / chunks;
    const MergeChunk m = merge_chunk(g % chunks, chunk, run, n);
    const K* A = in + seg * n + m.pair0;
    const K* B = A + m.la;
    int64_t lo = max(m.d0 - m.lb, (int64_t)0), hi = min(m.d0, m.la);
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (A[mid] <= B[m.d0 - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    split[g] = (int32_t)lo;
}

// blockDim.x = chunk / SORT_MERGE_PER_THREAD; dynamic LDS: lds_bytes<K>(chunk).  The chunk's two input pieces are staged in LDS,
// every thread finds the split of its own diagonal there, merges 8 keys serially into registers (ties: left piece first), and
// the merged chunk goes back through the same LDS words to be stored coalesced.
template <typename K>
__global__ __launch_bounds__(SWD_BLOCK) void segsort_merge_kernel(const K* __restrict__ in, int64_t n, int64_t run, int chunk,
                                                                  int64_t chunks, const int32_t* __restrict__ split, int unmap,
                                                                  K* __restrict__ out, int32_t* __restrict__ perm) {
    MF_DYN_SMEM(K, s);
    const int nt = (int)blockDim.x;
    const int64_t seg = (int64_t)blockIdx.x / chunks;
    const int64_t c = (int64_t)blockIdx.x % chunks;
    const MergeChunk m = merge_chunk(c, chunk, run, n);
    const int64_t a0 = split[blockIdx.x];
    const int64_t a1 = (m.d1 == m.la + m.lb) ? m.la : (int64_t)split[blockIdx.x + 1];   // the next chunk lies in the same pair
    const int64_t b0 = m.d0 - a0;
    const int na = (int)(a1 - a0);
    const int tot = (int)(m.d1 - m.d0);
    const int nb = tot - na;
    const K* A = in + seg * n + m.pair0 + a0;
    const K* B = in + seg * n + m.pair0 + m.la + b0;
    for (int i = threadIdx.x; i < tot; i += nt) s[lds_pad<K>(i)] = i < na ? A[i] : B[i - na];
    __syncthreads();
    const int diag = min((int)threadIdx.x * SORT_MERGE_PER_THREAD, tot);
    int lo = max(diag - nb, 0), hi = min(diag, na);
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[lds_pad<K>(mid)] <= s[lds_pad<K>(na + diag - 1 - mid)]) lo = mid + 1;
        else hi = mid;
    }
    int ai = lo, bi = diag - lo;
    K ka = ai < na ? s[lds_pad<K>(ai)] : K(0);
    K kb = bi < nb ? s[lds_pad<K>(na + bi)] : K(0);
    K r[SORT_MERGE_PER_THREAD];
#pragma unroll
    for (int i = 0; i < SORT_MERGE_PER_THREAD; ++i) {        // beyond the end of both pieces r[i] is filler and is not stored
        const bool left = bi >= nb || (ai < na && ka <= kb);
        r[i] = left ? ka : kb;
        if (left) {
            ++ai;
            ka = ai < na ? s[lds_pad<K>(ai)] : K(0);
        } else {
            ++bi;
            kb = bi < nb ? s[lds_pad<K>(na + bi)] : K(0);
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < SORT_MERGE_PER_THREAD; ++i)
        if (diag + i < tot) s[lds_pad<K>(diag + i)] = r[i];
    __syncthreads();
    const int64_t o = seg * n + m.pair0 + m.d0;
    if (unmap) {
        for (int i = threadIdx.x; i < tot; i += nt) SortKey<K>::store(out, perm, o + i, s[lds_pad<K>(i)]);
    } else {
        for (int i = threadIdx.x; i < tot; i += nt) out[o + i] = s[lds_pad<K>(i)];
    }
}

// ------------------------------------------------------------------------------------------------ quantile cost
__device__ __forceinline__ double cost_term(float a, float b, int pkind, double p) {
    const double t = (double)fabsf(a - b);                   // one fp32 subtraction per term
    return pkind == 1 ? t : (pkind == 2 ? t * t : pow(t, p));
}

// a[P, n], b[P, m] sorted, n >= m.  In units of 1 / (n m), element k of a owns (k m, (k + 1) m], element j of b owns
// (j n, (j + 1) n]: k meets j0 = floor(k m / n) and, when (j0 + 1) n < (k + 1) m, j0 + 1.  Equal sizes: weight 1 each.
__global__ __launch_bounds__(SWD_BLOCK) void swd_cost_kernel(const float* __restrict__ a, int64_t n, const float* __restrict__ b,
                                                             int64_t m, int pkind, double p, int64_t nchunks,
                                                             double* __restrict__ partial) {
    __shared__ double red[SWD_BLOCK];
    const int64_t seg = (int64_t)blockIdx.x / nchunks;
    const int64_t k0 = ((int64_t)blockIdx.x % nchunks) * COST_PER_BLOCK;
    const float* as = a + seg * n;
    const float* bs = b + seg * m;
    double acc = 0.0;
    for (int q = 0; q < COST_PER_BLOCK / SWD_BLOCK; ++q) {
        const int64_t k = k0 + threadIdx.x + (int64_t)q * SWD_BLOCK;
        if (k >= n) break;
        const float ak = as[k];
        if (n == m) {
            acc += cost_term(ak, bs[k], pkind, p);
        } else {
            const int64_t km = k * m;
            const int64_t j0 = km / n;
            const int64_t end0 = (j0 + 1) * n;
            acc += (double)(min(km + m, end0) - km) * cost_term(ak, bs[j0], pkind, p);
            if (end0 < km + m) acc += (double)(km + m - end0) * cost_term(ak, bs[j0 + 1], pkind, p);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = SWD_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// one workgroup: wpp[s] = (sum of the segment's partials in chunk order) / denom, dist = (sum_s wpp[s] / P)^(1/p)
__global__ __launch_bounds__(SWD_BLOCK) void swd_cost_finish_kernel(const double* __restrict__ partial, int P, int64_t nchunks,
                                                                    double denom, int pkind, double p, double* __restrict__ wpp,
                                                                    float* __restrict__ dist) {
    __shared__ double red[SWD_BLOCK];
    double local = 0.0;
    for (int s = threadIdx.x; s < P; s += SWD_BLOCK) {
        double t = 0.0;
        for (int64_t c = 0; c < nchunks; ++c) t += partial[(int64_t)s * nchunks + c];
        t /= denom;
        wpp[s] = t;
        local += t;
    }
    red[threadIdx.x] = local;
    __syncthreads();
    for (int s = SWD_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mean = red[0] / (double)P;
        *dist = (float)(pkind == 1 ? mean : (pkind == 2 ? sqrt(mean) : pow(mean, 1.0 / p)));
    }
}

// ------------------------------------------------------------------------------------------------ adjoint of the quantile cost
// d phi / d t of phi(t) = |t|^p at t = a - b: one fp32 subtraction as in cost_term, then fp64.  A tie gives 0, a NaN gives NaN.
__device__ __forceinline__ double cost_dterm(float a, float b, int pkind, double p) {
    const double t = (double)(a - b);
    if (pkind == 1) return t > 0.0 ? 1.0 : (t < 0.0 ? -1.0 : t);
    if (pkind == 2) return 2.0 * t;
    if (t == 0.0) return 0.0;
    const double r = p * pow(fabs(t), p - 1.0);
    return t < 0.0 ? -r : r;
}

// gdist * d dist / d wpp[s], the same for every s: with M = sum_s wpp[s] / P, gdist (1/p) M^(1/p - 1) / P.  Every workgroup
// repeats the forward's sum (strided shares, the same tree), so M is bitwise the mean the forward took the root of.  M == 0
// gives 0 (identical clouds: every phi' is 0 as well, and 0 * inf is not wanted), M NaN gives NaN.  `red` is free on return.
__device__ __forceinline__ double swd_grad_coef(const double* __restrict__ wpp, int P, int pkind, double p,
                                                const float* __restrict__ gdist, double* red) {
    double local = 0.0;
    for (int s = threadIdx.x; s < P; s += SWD_BLOCK) local += wpp[s];
    red[threadIdx.x] = local;
    __syncthreads();
    for (int s = SWD_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double M = red[0] / (double)P;
    __syncthreads();
    double c;
    if (M != M) c = M;
    else if (M == 0.0) c = 0.0;
    else c = pkind == 1 ? 1.0 : (pkind == 2 ? 0.5 / sqrt(M) : pow(M, 1.0 / p - 1.0) / p);
    return (double)gdist[0] * c / (double)P;
}

// The side with the threads of the forward: a[P, n], b[P, m] sorted, n >= m; element k of a meets j0 and possibly j0 + 1 with
// the weights of swd_cost_kernel.  ga (NULL: skipped) takes the gradient of a.  Equal sizes: gb (NULL: skipped) takes the
// gradient of b, the exact negative, in the same launch.  perm_* != NULL: the value of rank k goes to position perm[seg, k].
__global__ __launch_bounds__(SWD_BLOCK) void swd_cost_bwd_large_kernel(const float* __restrict__ a, int64_t n,
                                                                       const int32_t* __restrict__ perm_a,
                                                                       const float* __restrict__ b, int64_t m,
                                                                       const int32_t* __restrict__ perm_b, int P, int pkind,
                                                                       double p, int64_t nchunks, const double* __restrict__ wpp,
                                                                       const float* __restrict__ gdist, float* __restrict__ ga,
                                                                       float* __restrict__ gb) {
    __shared__ double red[SWD_BLOCK];
    const double coef = swd_grad_coef(wpp, P, pkind, p, gdist, red);
    const double denom = n == m ? (double)n : (double)n * (double)m;
    const int64_t seg = (int64_t)blockIdx.x / nchunks;
    const int64_t k0 = ((int64_t)blockIdx.x % nchunks) * COST_PER_BLOCK;
    const float* as = a + seg * n;
    const float* bs = b + seg * m;
    for (int q = 0; q < COST_PER_BLOCK / SWD_BLOCK; ++q) {
        const int64_t k = k0 + threadIdx.x + (int64_t)q * SWD_BLOCK;
        if (k >= n) break;
        const float ak = as[k];
        double g;
        if (n == m) {
            g = cost_dterm(ak, bs[k], pkind, p);
        } else {
            const int64_t km = k * m;
            const int64_t j0 = km / n;
            const int64_t end0 = (j0 + 1) * n;
            g = (double)(min(km + m, end0) - km) * cost_dterm(ak, bs[j0], pkind, p);
            if (end0 < km + m) g += (double)(km + m - end0) * cost_dterm(ak, bs[j0 + 1], pkind, p);
        }
        const float gf = (float)(coef * g / denom);
        if (ga) ga[seg * n + (perm_a ? (int64_t)perm_a[seg * n + k] : k)] = gf;
        if (n == m && gb) gb[seg * n + (perm_b ? (int64_t)perm_b[seg * n + k] : k)] = -gf;
    }
}

constexpr int COST_BWD_ROUNDS = 16;         // elements of the smaller set each lane group handles, one after the other

// The smaller side, m < n: element j of b owns (j n, (j + 1) n] and meets the elements k = floor(j n / m) .. floor(((j + 1) n
// - 1) / m) of a, each with weight min((k + 1) m, (j + 1) n) - max(k m, j n) > 0: the forward's pieces seen from b.  A group
// of 2^glog2 consecutive lanes strides that range and sums in fp64 through a tree of fixed shape in LDS; the group size is
// chosen by the host from n and m alone (the smallest power of two that holds ceil(n / m) + 1 terms, 256 at most), so the
// order of the sum is a function of the shapes.  d |a_k - b_j|^p / d b_j = -phi'(a_k - b_j).
__global__ __launch_bounds__(SWD_BLOCK) void swd_cost_bwd_small_kernel(const float* __restrict__ a, int64_t n,
                                                                       const float* __restrict__ b, int64_t m,
                                                                       const int32_t* __restrict__ perm_b, int P, int pkind,
                                                                       double p, int glog2, int64_t nchunks,
                                                                       const double* __restrict__ wpp,
                                                                       const float* __restrict__ gdist, float* __restrict__ gb) {
    __shared__ double red[SWD_BLOCK];
    const double coef = swd_grad_coef(wpp, P, pkind, p, gdist, red);
    const double denom = (double)n * (double)m;
    const int G = 1 << glog2, groups = SWD_BLOCK >> glog2;
    const int lane = (int)threadIdx.x & (G - 1), grp = (int)threadIdx.x >> glog2;
    const int64_t seg = (int64_t)blockIdx.x / nchunks;
    const int64_t j0 = ((int64_t)blockIdx.x % nchunks) * groups * COST_BWD_ROUNDS;
    const float* as = a + seg * n;
    const float* bs = b + seg * m;
    for (int q = 0; q < COST_BWD_ROUNDS; ++q) {
        if (j0 + (int64_t)q * groups >= m) break;           // the same for the whole workgroup: barriers below
        const int64_t j = j0 + (int64_t)q * groups + grp;
        double acc = 0.0;
        if (j < m) {
            const float bj = bs[j];
            const int64_t lo = j * n, hi = lo + n;
            const int64_t k_last = (hi - 1) / m;
            for (int64_t k = lo / m + lane; k <= k_last; k += G) {
                const int64_t km = k * m;
                acc += (double)(min(km + m, hi) - max(km, lo)) * cost_dterm(as[k], bj, pkind, p);
            }
        }
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int s = G / 2; s > 0; s >>= 1) {
            if (lane < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (lane == 0 && j < m) gb[seg * m + (perm_b ? (int64_t)perm_b[seg * m + j] : j)] = (float)(-(coef * red[threadIdx.x] / denom));
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ back-projection
// gx[i, k] (+)= sum_p dir[k, p] g[p, i]: one thread per point, the directions staged in LDS in the layout of swd_project_kernel,
// chunk after chunk of SWD_PCHUNK inside the workgroup, so every output is one fmaf chain over ascending p.  g is read
// coalesced for every p.
__global__ __launch_bounds__(SWD_BLOCK) void swd_project_bwd_kernel(const float* __restrict__ g, int64_t n, int d,
                                                                    const float* __restrict__ dir, int P, float* __restrict__ gx,
                                                                    int accumulate) {
    MF_DYN_SMEM(float, sdir);               // [pc][SWD_DMAX], zero beyond d
    const int64_t i = (int64_t)blockIdx.x * SWD_BLOCK + threadIdx.x;
    float acc[SWD_DMAX];
#pragma unroll
    for (int k = 0; k < SWD_DMAX; ++k) acc[k] = 0.0f;
    for (int p0 = 0; p0 < P; p0 += SWD_PCHUNK) {
        const int pc = min(P - p0, SWD_PCHUNK);
        if (p0 > 0) __syncthreads();        // everybody is done with the previous chunk
        for (int e = threadIdx.x; e < pc * SWD_DMAX; e += SWD_BLOCK) {
            const int p = e / SWD_DMAX, k = e % SWD_DMAX;
            sdir[e] = k < d ? dir[(int64_t)k * P + p0 + p] : 0.0f;
        }
        __syncthreads();
        if (i < n) {
#pragma unroll 8
            for (int p = 0; p < pc; ++p) {
                const float gp = g[(int64_t)(p0 + p) * n + i];
                const float* dp = sdir + p * SWD_DMAX;
#pragma unroll
                for (int k = 0; k < SWD_DMAX; ++k)
                    if (k < d) acc[k] = fmaf(dp[k], gp, acc[k]);
            }
        }
    }
    if (i < n) {
#pragma unroll
        for (int k = 0; k < SWD_DMAX; ++k)
            if (k < d) gx[i * d + k] = accumulate ? gx[i * d + k] + acc[k] : acc[k];
    }
}

struct SortPlan {
    int tile_log2;
    int chunk;
    int64_t tiles, chunks;
    int passes;
};

// checks the arguments of the sort; tile_log2 = 0 selects the default tile of the element type
static int sort_plan(int P, int64_t n, int tile_log2, int default_tile_log2, SortPlan* sp) {
    if (P < 1 || n < 1) return fail("segmented sort: needs at least one segment and one key (got %d x %lld)", P, (long long)n);
    if ((int64_t)P * n >= (int64_t)1 << 31) return fail("segmented sort: %d x %lld keys reach 2^31", P, (long long)n);
    if (tile_log2 == 0) tile_log2 = default_tile_log2;
    if (tile_log2 < SORT_TILE_LOG2_MIN || tile_log2 > SORT_TILE_LOG2_MAX)
        return fail("segmented sort: tile_log2 must be 0 (default) or %d..%d (got %d)", SORT_TILE_LOG2_MIN, SORT_TILE_LOG2_MAX,
                    tile_log2);
    const int64_t T = (int64_t)1 << tile_log2;
    sp->tile_log2 = tile_log2;
    sp->chunk = (int)min(T, (int64_t)SORT_MERGE_CHUNK);
    sp->tiles = (n + T - 1) / T;
    sp->chunks = (n + sp->chunk - 1) / sp->chunk;
    sp->passes = 0;
    for (int64_t r = 1; r < sp->tiles; r <<= 1) sp->passes++;
    return 0;
}

}  // namespace mf

using namespace mf;

// ================================================================================================= C ABI
extern "C" int mf_swd_project(const float* x, int64_t n, int d, const float* dir, int P, float* u, void* stream) {
    if (d < 1 || d > SWD_DMAX) return fail("mf_swd_project supports 1 <= ndim <= %d (got %d)", SWD_DMAX, d);
    if (P < 1 || n < 1) return fail("mf_swd_project: needs at least one direction and one point (got %d, %lld)", P, (long long)n);
    if ((int64_t)P * n >= (int64_t)1 << 31) return fail("mf_swd_project: %d x %lld projections reach 2^31", P, (long long)n);
    const int py = (P + SWD_PCHUNK - 1) / SWD_PCHUNK;
    if (py > 65535) return fail("mf_swd_project: too many directions (%d)", P);
    int64_t gx = (n + SWD_BLOCK - 1) / SWD_BLOCK;
    if (gx > NUM_CU * 8) gx = NUM_CU * 8;
    const size_t smem = sizeof(float) * SWD_DMAX * (size_t)(P < SWD_PCHUNK ? P : SWD_PCHUNK);
    MF_LAUNCH(swd_project_kernel, dim3((unsigned)gx, (unsigned)py), SWD_BLOCK, smem, stream, x, n, d, dir, P, u);
    return check_launch("mf_swd_project");
}

// Tile sort, then `passes` merge passes.  Intermediate results hop between bufs[0] and bufs[1] starting at bufs[cur]; the last
// stage (the tile sort itself where one tile holds a segment) writes floats to `final_out` and, for composites, positions to `perm`.
template <typename K>
static int segsort_launch(const char* who, const float* keys, int P, int64_t n, const SortPlan& sp, K* const (&bufs)[2], int cur,
                          int32_t* split, K* final_out, int32_t* perm, void* stream) {
    const int T = 1 << sp.tile_log2;
    MF_LAUNCH(segsort_tile_kernel<K>, dim3((unsigned)(P * sp.tiles)), T / 16, lds_bytes<K>(T), stream, keys, n, sp.tile_log2, sp.tiles,
              (int)(sp.passes == 0), sp.passes == 0 ? final_out : bufs[cur], perm);
    if (check_launch(who)) return 1;
    const int64_t total = (int64_t)P * sp.chunks;
    int64_t run = T;
    for (int pass = 0; pass < sp.passes; ++pass, run <<= 1) {
        const bool last = pass == sp.passes - 1;
        MF_LAUNCH(segsort_partition_kernel<K>, dim3((unsigned)((total + SWD_BLOCK - 1) / SWD_BLOCK)), SWD_BLOCK, 0, stream,
                  (const K*)bufs[cur], n, run, sp.chunk, sp.chunks, total, split);
        if (check_launch(who)) return 1;
        MF_LAUNCH(segsort_merge_kernel<K>, dim3((unsigned)total), sp.chunk / SORT_MERGE_PER_THREAD, lds_bytes<K>(sp.chunk), stream,
                  (const K*)bufs[cur], n, run, sp.chunk, sp.chunks, (const int32_t*)split, (int)last, last ? final_out : bufs[cur ^ 1],
                  perm);
        if (check_launch(who)) return 1;
        cur ^= 1;
    }
    return 0;
}

extern "C" int64_t mf_segsort_workspace_bytes(int P, int64_t n, int tile_log2) {
    SortPlan sp;
    if (sort_plan(P, n, tile_log2, SORT_TILE_LOG2, &sp)) return -1;
    if (sp.passes == 0) return 0;
    return 4 * ((int64_t)P * n + (int64_t)P * sp.chunks);
}

extern "C" int mf_segsort_f32(const float* keys, int P, int64_t n, int tile_log2, float* out, void* ws, void* stream) {
    SortPlan sp;
    if (sort_plan(P, n, tile_log2, SORT_TILE_LOG2, &sp)) return 1;
    if (sp.passes > 0 && ws == nullptr) return fail("mf_segsort_f32: %d merge passes need the workspace", sp.passes);
    uint32_t* const bufs[2] = {reinterpret_cast<uint32_t*>(out), reinterpret_cast<uint32_t*>(ws)};
    int32_t* split = sp.passes > 0 ? reinterpret_cast<int32_t*>(bufs[1] + (int64_t)P * n) : nullptr;
    // the tile sort writes where an even number of hops ends in `out`
    return segsort_launch<uint32_t>("mf_segsort_f32", keys, P, n, sp, bufs, sp.passes & 1, split, bufs[0], nullptr, stream);
}

// workspace of the pair sort: one buffer of composites per hop that does not end in (out, perm), two at most, then the splits
extern "C" int64_t mf_segsort_pairs_workspace_bytes(int P, int64_t n, int tile_log2) {
    SortPlan sp;
    if (sort_plan(P, n, tile_log2, SORT_PAIR_TILE_LOG2, &sp)) return -1;
    if (sp.passes == 0) return 0;
    return 8 * (int64_t)P * n * (sp.passes > 1 ? 2 : 1) + 4 * (int64_t)P * sp.chunks;
}

extern "C" int mf_segsort_pairs_f32(const float* keys, int P, int64_t n, int tile_log2, float* out, int32_t* perm, void* ws,
                                    void* stream) {
    SortPlan sp;
    if (sort_plan(P, n, tile_log2, SORT_PAIR_TILE_LOG2, &sp)) return 1;
    if (out == nullptr || perm == nullptr) return fail("mf_segsort_pairs_f32: out and perm are both required");
    if (sp.passes > 0 && ws == nullptr) return fail("mf_segsort_pairs_f32: %d merge passes need the workspace", sp.passes);
    if (((uintptr_t)ws & 7) != 0) return fail("mf_segsort_pairs_f32: the workspace must be 8-byte aligned");
    uint64_t* const b0 = reinterpret_cast<uint64_t*>(ws);
    uint64_t* const b1 = sp.passes > 1 ? b0 + (int64_t)P * n : nullptr;
    uint64_t* const bufs[2] = {b0, b1};
    int32_t* split = sp.passes > 0 ? reinterpret_cast<int32_t*>(b0 + (int64_t)P * n * (sp.passes > 1 ? 2 : 1)) : nullptr;
    return segsort_launch<uint64_t>("mf_segsort_pairs_f32", keys, P, n, sp, bufs, 0, split, reinterpret_cast<uint64_t*>(out), perm,
                                    stream);
}

extern "C" int64_t mf_swd_cost_ws_doubles(int P, int64_t n1, int64_t n2) {
    const int64_t n = n1 > n2 ? n1 : n2;
    if (P < 1 || n < 1) return 0;
    return (int64_t)P * ((n + COST_PER_BLOCK - 1) / COST_PER_BLOCK);
}

extern "C" int mf_swd_quantile_cost(const float* u, int64_t n1, const float* v, int64_t n2, int P, float p, double* partial,
                                    double* wpp, float* dist, void* stream) {
    if (P < 1 || n1 < 1 || n2 < 1)
        return fail("mf_swd_quantile_cost: needs at least one projection and one point per set (got %d, %lld, %lld)", P,
                    (long long)n1, (long long)n2);
    if (!(p >= 1.0f)) return fail("mf_swd_quantile_cost: the order p must be a real number >= 1 (got %g)", (double)p);
    const bool swap = n2 > n1;               // the larger set gets the threads; the integral is symmetric
    const float* a = swap ? v : u;
    const float* b = swap ? u : v;
    const int64_t n = swap ? n2 : n1, m = swap ? n1 : n2;
    if ((int64_t)P * n >= (int64_t)1 << 31) return fail("mf_swd_quantile_cost: %d x %lld projections reach 2^31", P, (long long)n);
    const int64_t nchunks = (n + COST_PER_BLOCK - 1) / COST_PER_BLOCK;
    const int pkind = p == 1.0f ? 1 : (p == 2.0f ? 2 : 0);
    MF_LAUNCH(swd_cost_kernel, dim3((unsigned)(P * nchunks)), SWD_BLOCK, 0, stream, a, n, b, m, pkind, (double)p, nchunks, partial);
    if (check_launch("mf_swd_quantile_cost")) return 1;
    const double denom = n == m ? (double)n : (double)n * (double)m;
    MF_LAUNCH(swd_cost_finish_kernel, 1, SWD_BLOCK, 0, stream, (const double*)partial, P, nchunks, denom, pkind, (double)p, wpp,
              dist);
    return check_launch("mf_swd_quantile_cost (finish)");
}

extern "C" int mf_swd_quantile_cost_bwd(const float* u, int64_t n1, const int32_t* perm_u, const float* v, int64_t n2,
                                        const int32_t* perm_v, int P, float p, const double* wpp, const float* gdist, float* gu,
                                        float* gv, void* stream) {
    if (P < 1 || n1 < 1 || n2 < 1)
        return fail("mf_swd_quantile_cost_bwd: needs at least one projection and one point per set (got %d, %lld, %lld)", P,
                    (long long)n1, (long long)n2);
    if (!(p >= 1.0f)) return fail("mf_swd_quantile_cost_bwd: the order p must be a real number >= 1 (got %g)", (double)p);
    const bool swap = n2 > n1;               // a: the larger set, as in the forward
    const float* a = swap ? v : u;
    const float* b = swap ? u : v;
    const int32_t* perm_a = swap ? perm_v : perm_u;
    const int32_t* perm_b = swap ? perm_u : perm_v;
    float* ga = swap ? gv : gu;
    float* gb = swap ? gu : gv;
    const int64_t n = swap ? n2 : n1, m = swap ? n1 : n2;
    if ((int64_t)P * n >= (int64_t)1 << 31)
        return fail("mf_swd_quantile_cost_bwd: %d x %lld projections reach 2^31", P, (long long)n);
    const int pkind = p == 1.0f ? 1 : (p == 2.0f ? 2 : 0);
    if (ga != nullptr || (n == m && gb != nullptr)) {
        const int64_t nchunks = (n + COST_PER_BLOCK - 1) / COST_PER_BLOCK;
        MF_LAUNCH(swd_cost_bwd_large_kernel, dim3((unsigned)(P * nchunks)), SWD_BLOCK, 0, stream, a, n, perm_a, b, m, perm_b, P, pkind,
                  (double)p, nchunks, wpp, gdist, ga, gb);
        if (check_launch("mf_swd_quantile_cost_bwd")) return 1;
    }
    if (n != m && gb != nullptr) {
        const int64_t terms = (n + m - 1) / m + 1;          // the most elements of a that one element of b meets
        int glog2 = 1;
        while (glog2 < 8 && ((int64_t)1 << glog2) < terms) ++glog2;
        const int64_t per_block = (int64_t)(SWD_BLOCK >> glog2) * COST_BWD_ROUNDS;
        const int64_t nchunks = (m + per_block - 1) / per_block;
        MF_LAUNCH(swd_cost_bwd_small_kernel, dim3((unsigned)(P * nchunks)), SWD_BLOCK, 0, stream, a, n, b, m, perm_b, P, pkind,
                  (double)p, glog2, nchunks, wpp, gdist, gb);
        if (check_launch("mf_swd_quantile_cost_bwd (smaller set)")) return 1;
    }
    return 0;
}

extern "C" int mf_swd_project_bwd(const float* g, int64_t n, int d, const float* dir, int P, float* gx, int accumulate,
                                  void* stream) {
    if (d < 1 || d > SWD_DMAX) return fail("mf_swd_project_bwd supports 1 <= ndim <= %d (got %d)", SWD_DMAX, d);
    if (P < 1 || n < 1) return fail("mf_swd_project_bwd: needs at least one direction and one point (got %d, %lld)", P, (long long)n);
    if ((int64_t)P * n >= (int64_t)1 << 31) return fail("mf_swd_project_bwd: %d x %lld projections reach 2^31", P, (long long)n);
    const size_t smem = sizeof(float) * SWD_DMAX * (size_t)(P < SWD_PCHUNK ? P : SWD_PCHUNK);
    MF_LAUNCH(swd_project_bwd_kernel, dim3((unsigned)((n + SWD_BLOCK - 1) / SWD_BLOCK)), SWD_BLOCK, smem, stream, g, n, d, dir, P, gx,
              accumulate);
    return check_launch("mf_swd_project_bwd");
}
