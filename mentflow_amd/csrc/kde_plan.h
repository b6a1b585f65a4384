// Launch policy of the four projection + KDE launchers of kde.hip (mf_proj_kde1d_fwd / _bwd, mf_proj_kde2d_fwd / _bwd): from the sizes
// of a call and the MENTFLOW_KDE* tuning variables to the launch shape.  Host-only plain C++ (no HIP types): kde.hip launches what
// kde_plan returns, mf_proj_kde_plan reports it, and tests/emu/sanitize_main.cpp walks it over the knob grid of tools/kde_sweep.py.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

namespace mf {

constexpr int KDE_CUS = 256;                          // NUM_CU of common.h (kde.hip asserts that they agree)
constexpr size_t KDE_LDS_BYTES = 156 * 1024;          // dynamic LDS a workgroup may ask for (of 160 KiB)
constexpr int KDE_MAX_PER_WG = 8192;                  // particles per workgroup: 2^13 * 2^50 < 2^64, no overflow
constexpr int KDE_VS = 8;                             // LDS row stride of the projection vectors (two 16-byte reads)
constexpr int KDE_RMAX2D = 5;

enum KdeKernel { KDE1D_FWD = 0, KDE1D_BWD, KDE2D_FWD, KDE2D_BWD, KDE_KERNELS };
enum KdeKnob { KNOB_BLOCK = 0, KNOB_LDS, KNOB_WAVES, KNOB_NPT, KDE_KNOBS };

// The tuning variable behind each knob of each launcher (nullptr: the launcher has no such knob).  0 = heuristic; waves default to 4.
constexpr const char* KDE_KNOB_ENV[KDE_KERNELS][KDE_KNOBS] = {
    {"MENTFLOW_KDE1D_BLOCK", "MENTFLOW_KDE1D_LDS", "MENTFLOW_KDE1D_WAVES", nullptr},
    {"MENTFLOW_KDE1D_BWD_BLOCK", "MENTFLOW_KDE1D_BWD_LDS", nullptr, nullptr},
    {"MENTFLOW_KDE2D_BLOCK", "MENTFLOW_KDE2D_FWD_LDS", "MENTFLOW_KDE2D_WAVES", nullptr},
    {"MENTFLOW_KDE2D_BWD_BLOCK", "MENTFLOW_KDE2D_BWD_LDS", nullptr, "MENTFLOW_KDE2D_BWD_NPT"}};
struct KdeKnobs {
    int v[KDE_KERNELS][KDE_KNOBS] = {{0, 0, 4, 0}, {0, 0, 4, 0}, {0, 0, 4, 0}, {0, 0, 4, 0}};
};

inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
inline KdeKnobs kde_knobs_from_env() {
    KdeKnobs k;
    for (int i = 0; i < KDE_KERNELS; ++i)
        for (int j = 0; j < KDE_KNOBS; ++j)
            if (KDE_KNOB_ENV[i][j]) k.v[i][j] = env_int(KDE_KNOB_ENV[i][j], k.v[i][j]);
    return k;
}

struct KdePlan {
    int window;        // kernel instance: 4 = factorised radius-4 window, 0 = run-time radius
    int block, Pg;     // threads per workgroup; projections whose images one workgroup holds in LDS
    int groups;        // ceil(P / Pg): grid.y of the forwards, passes over the images of the backwards
    int per_wg;        // particles per workgroup
    int split;         // 1-D backward: CH, lanes per particle; 2-D backward: NPT, particles per thread; forwards: 0
    int shift;         // kde_global_shift(n) of the forwards
    int64_t grid_x;    // workgroups along the particles
    size_t smem;       // dynamic LDS bytes
    char err[160];     // why kde_plan refused
};

// the forwards' global accumulators hold 2^(shift-50) units (fix_flush of kde.hip): exact up to 8192 particles per call
inline int kde_global_shift(int64_t n) {
    int k = 0;
    while (((int64_t)1 << k) < n) ++k;
    return k > 13 ? k - 13 : 0;
}
// particles per forward workgroup: enough workgroups to cover the chip `waves` times over, a multiple of the block
// size, at most KDE_MAX_PER_WG (fixed-point headroom)
inline int kde_per_wg(int64_t n, int ngroups, int block, int waves) {
    int64_t want = (n * ngroups + (int64_t)waves * KDE_CUS - 1) / ((int64_t)waves * KDE_CUS);
    want = ((want + block - 1) / block) * block;
    if (want < block) want = block;
    if (want > KDE_MAX_PER_WG) want = (KDE_MAX_PER_WG / block) * block;
    return (int)want;
}
inline int kde_radius_1d(int radius, int B) { return radius < 0 ? 0 : (radius > B ? B : radius); }

// The launch shape of `kernel` (a KdeKernel) for n particles, P projections and Bx (x By) bins; By and radius_y are ignored in 1-D.
// false, with the reason in p.err, where the launcher refuses the call: bad sizes, an image that does not fit LDS, a bad knob.
inline bool kde_plan(int kernel, int64_t n, int P, int Bx, int By, int radius_x, int radius_y, const KdeKnobs& knobs, KdePlan& p) {
    p = KdePlan{};
    auto refuse = [&p](const char* fmt, auto... a) { return snprintf(p.err, sizeof(p.err), fmt, a...), false; };
    if (kernel < 0 || kernel >= KDE_KERNELS) return refuse("kernel must be 0 .. 3 (got %d)", kernel);
    const bool two_d = kernel >= KDE2D_FWD, fwd = kernel == KDE1D_FWD || kernel == KDE2D_FWD;
    if (!two_d) By = 1;
    if (n < 0 || P < 1 || Bx < 2 || (two_d && By < 2))
        return refuse("need n >= 0, P >= 1 and at least 2 bins (n=%lld, P=%d, bins=%d x %d)", (long long)n, P, Bx, By);
    if (two_d && (radius_x > KDE_RMAX2D || radius_y > KDE_RMAX2D))
        return refuse("2-D KDE kernel supports a truncation radius <= %d bins (bandwidth <= 0.6 bin widths)", KDE_RMAX2D);
    const int* kn = knobs.v[kernel];
    const char* const* env = KDE_KNOB_ENV[kernel];
    if (kn[KNOB_BLOCK] != 0 && kn[KNOB_BLOCK] != 256 && kn[KNOB_BLOCK] != 512 && kn[KNOB_BLOCK] != 1024)
        return refuse("%s=%d: a block is 256, 512 or 1024 threads (0 = heuristic)", env[KNOB_BLOCK], kn[KNOB_BLOCK]);
    if (kn[KNOB_LDS] < 0) return refuse("%s=%d: an LDS budget is a number of bytes (0 = heuristic)", env[KNOB_LDS], kn[KNOB_LDS]);
    if (env[KNOB_WAVES] && kn[KNOB_WAVES] < 1) return refuse("%s=%d: needs at least 1", env[KNOB_WAVES], kn[KNOB_WAVES]);
    if (env[KNOB_NPT] && kn[KNOB_NPT] != 0 && kn[KNOB_NPT] != 1 && kn[KNOB_NPT] != 2 && kn[KNOB_NPT] != 4)
        return refuse("%s=%d: particles per thread are 1, 2 or 4 (0 = heuristic)", env[KNOB_NPT], kn[KNOB_NPT]);
    // LDS of a workgroup: per projection its image (64-bit fixed-point cells forward, the fp32 cells of gS backward) and its one or
    // two projection vectors; once, the bin centres
    const size_t per_proj = (fwd ? sizeof(uint64_t) : sizeof(float)) * (size_t)Bx * By + sizeof(float) * KDE_VS * (two_d ? 2 : 1);
    const size_t fixed = sizeof(float) * ((size_t)Bx + (two_d ? By : 0));
    if (per_proj + fixed > KDE_LDS_BYTES) return refuse("histogram image %d x %d exceeds the LDS budget", Bx, By);

    const bool small = n <= 65536;
    size_t budget = 52 * 1024;
    if (kernel == KDE1D_FWD) {
        // Large batches: all projections that fit one image (C4: 100 x 64 bins = 51 KiB), big workgroups.  Small batches
        // (the reference's 25 000 particles): 256 threads and many small projection groups so that ~4 * NUM_CU
        // workgroups exist.
        // tuned on MI355X at C4 (tools/kde_sweep.py, profiles/r02_kde_sweep_1d.txt): 1024 threads, ~52 KiB images (two
        // workgroups = 32 waves per CU): 1.11-1.13 ms against 1.19-1.51 ms for 256 threads; 4 workgroup waves over the
        // chip (4096 particles per workgroup at C4) rather than 8: 2 % slower, half the flush atomics
        p.block = small ? 256 : 1024;
    } else if (kernel == KDE1D_BWD) {
        p.block = n >= 262144 ? 512 : 256;
    } else if (kernel == KDE2D_FWD) {
        // tuned on MI355X at C5 (tools/kde_sweep.py): one 85 x 85 image (58 KiB) per 1024-thread workgroup, two
        // workgroups per CU: 6.0 ms against 6.7 (512 threads) / 9-16 ms (256 threads, the r01 shape)
        p.block = 1024;
        budget = 60 * 1024;
    } else {
        // tuned on MI355X at C5 (tools/kde_sweep.py): 1024 threads x 4 particles each with four 85 x 85 images (116 KiB)
        // staged per pass — 3.8 ms against 5.3 ms for the r01 shape (256 threads x 4, one image); staging an image costs
        // L2 -> LDS traffic per workgroup, so fat workgroups win once there are enough particles to fill the chip with them.
        // Smaller batches step down to (1024, 2), (1024, 1), (512, 1), (256, 1) until >= 2 workgroups per CU exist.
        static const int shapes[5][2] = {{1024, 4}, {1024, 2}, {1024, 1}, {512, 1}, {256, 1}};
        for (int k = 0; k < 5; ++k) {
            p.block = shapes[k][0];
            p.split = shapes[k][1];
            if (n / ((int64_t)p.block * p.split) >= 2 * KDE_CUS) break;
        }
        if (kn[KNOB_NPT]) p.split = kn[KNOB_NPT];
    }
    if (kn[KNOB_BLOCK]) p.block = kn[KNOB_BLOCK];
    if (kernel == KDE2D_BWD) budget = (size_t)(p.block >= 1024 ? 118 : (p.block >= 512 ? 59 : 30)) * 1024;
    if (kn[KNOB_LDS]) budget = (size_t)kn[KNOB_LDS];
    // budget -> projections per group -> LDS bytes: at least one projection, at most what a workgroup may ask for
    if (budget > KDE_LDS_BYTES) budget = KDE_LDS_BYTES;
    if (budget < per_proj + fixed) budget = per_proj + fixed;
    const size_t fit = (budget - fixed) / per_proj;
    p.Pg = fit < (size_t)P ? (int)fit : P;
    if (kernel == KDE1D_FWD && small) {
        const int64_t wg_particles = n > 0 ? (n + p.block - 1) / p.block : 1;
        const int64_t want_groups = (4 * KDE_CUS + wg_particles - 1) / wg_particles;
        if (want_groups > 1) {
            int pg_small = (int)((P + want_groups - 1) / want_groups);
            if (pg_small < 4) pg_small = P < 4 ? P : 4;
            if (pg_small < p.Pg) p.Pg = pg_small;
        }
    } else if (kernel == KDE1D_FWD) {
        const int ng = (P + p.Pg - 1) / p.Pg;             // equal-sized groups
        p.Pg = (P + ng - 1) / ng;
    }
    p.groups = (P + p.Pg - 1) / p.Pg;
    p.smem = per_proj * p.Pg + fixed;
    if (kernel == KDE1D_BWD) {
        // lanes per particle: enough workgroups to give every SIMD a wave (>= 1024 workgroups of 4 waves), at most 8
        p.split = 1;
        while (p.split < 8 && p.split * 2 <= P && (n * p.split + p.block - 1) / p.block < 4 * KDE_CUS) p.split *= 2;
        p.per_wg = p.block / p.split;
    } else if (kernel == KDE2D_BWD) {
        p.per_wg = p.block * p.split;
    } else {
        p.per_wg = (kernel == KDE1D_FWD && small) ? p.block : kde_per_wg(n, p.groups, p.block, kn[KNOB_WAVES]);
        p.shift = kde_global_shift(n);
    }
    p.grid_x = (n + p.per_wg - 1) / p.per_wg;
    p.window = (two_d ? radius_x == 4 && radius_y == 4 : kde_radius_1d(radius_x, Bx) == 4) ? 4 : 0;
    return true;
}

}  // namespace mf
