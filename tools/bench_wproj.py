"""Time the weighted projection kernels (mentflow_amd/csrc/wproj.hip) beside the unweighted ones, and one sample-mode sub-step
of classical MENT on weighted chains beside the resampling path.  For DESIGN.md section 6k; nothing here is a pass/fail threshold.

Protocol of tools/bench_smc.py.  Each configuration is one process that merges its record into <out>/wproj_bench.json, so that
every GPU step can run under a time limit of its own and a failing step ends the chain:

    timeout -k 10 600 python tools/bench_wproj.py --out profiles --only kernels && \
    timeout -k 10 600 python tools/bench_wproj.py --out profiles --only substep && \
    timeout -k 10 900 python tools/bench_wproj.py --out profiles --only rmse

  * kernels: 2 097 152 x 6 particles (seeded normal), 100 unit projections, 64 bins on [-4, 4] (1-D) and 85 x 85 (2-D),
    bandwidth 0.5 bins, weights exp(randn).  Forward and backward (both gradients from the weighted one) of the unweighted and the
    weighted entry point ALTERNATE inside one process: `--repeats` timings each, a timing being BATCH back-to-back calls between
    two device events, after one untimed round of both.  Milliseconds per call, and the ratio of the medians.  Before timing,
    weights 1 are checked to reproduce the unweighted result bit for bit at this size.
  * substep: bench_mala.py's 6-D problem (100 one-D projections x 64 bins) after its one untimed Gauss-Seidel epoch; then
    MENT.simulate(0, 0), the prediction of one sub-step, with SequentialMonteCarloSampler(65 536 chains, 8 islands, 32
    temperatures): model.weighted = True (the population and its weights, 65 536 rows) against model.weighted = False at n_samples = 1 000 000
    (forced resampling and 16 collection rounds).  Wall time with a device synchronisation on both sides, alternating, after an
    untimed first call of each (the ladder): the timed calls are bridges, as every sub-step after the first is.
  * rmse: the same two predictions from a fresh sampler per seed, 16 seeds, against the same model's integrate-mode
    prediction of view 0 on a `--res`^5 grid over [-3.5, 3.5]^5: root-mean-square error over bins and seeds, for both."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_mala import CHAINS, NDIM, XMAX, make_model, spread  # noqa: E402
from mentflow_amd import ops  # noqa: E402
from mentflow_amd._lib import call, ptr, stream_ptr  # noqa: E402
from mentflow_amd.ment import MENT  # noqa: E402
from mentflow_amd.sample import SequentialMonteCarloSampler  # noqa: E402

N, P, B1, B2, BATCH = 2_097_152, 100, 64, 85, 5
GROUPS, TEMPS, SPT = 8, 32, 2
CONFIGS = ("kernels", "substep", "rmse")
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731


def time_pair(fn_a, fn_b, repeats):
    """Milliseconds per call of fn_a and fn_b, alternating: `repeats` batches of BATCH calls each between two events, after one
    untimed round of both."""
    out = ([], [])
    for i in range(repeats + 1):
        for fn, times in zip((fn_a, fn_b), out):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(BATCH):
                fn()
            t1.record()
            torch.cuda.synchronize()
            if i:
                times.append(t0.elapsed_time(t1) / BATCH)
    return out


def run_kernels(dev, repeats):
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(N, NDIM, device=dev, generator=gen)
    w = torch.exp(torch.randn(N, device=dev, generator=gen))
    ones = torch.ones(N, device=dev)

    def dirs():
        v = torch.randn(P, NDIM, device=dev, generator=gen)
        return (v / v.norm(dim=1, keepdim=True)).contiguous()

    V0, V1 = dirs(), dirs()
    e1, e2 = torch.linspace(-4, 4, B1 + 1, device=dev), torch.linspace(-4, 4, B2 + 1, device=dev)
    c1, c2 = 0.5 * (e1[1:] + e1[:-1]), 0.5 * (e2[1:] + e2[:-1])
    s1, s2, R = 0.5 * float(e1[1] - e1[0]), 0.5 * float(e2[1] - e2[0]), ops.kde_radius(0.5)
    g1 = torch.randn(P, B1, device=dev, generator=gen)
    g2 = torch.randn(P, B2, B2, device=dev, generator=gen)
    gx, gw = torch.empty_like(x), torch.empty_like(w)
    args2 = (V0, V1, c2, c2, s2, s2, R, R)
    # same results first: weights 1 give the unweighted sums bit for bit at the size that is timed
    same_1d = torch.equal(ops.ProjWKde1dFn.apply(x, ones, V0, c1, s1, R), ops.ProjKde1dFn.apply(x, V0, c1, s1, R))
    same_2d = torch.equal(ops.ProjWKde2dFn.apply(x, ones, *args2), ops.ProjKde2dFn.apply(x, *args2))

    def bwd1(weighted):
        if weighted:
            return lambda: call("mf_proj_wkde1d_bwd", ptr(x), ptr(w), N, NDIM, ptr(V0), P, ptr(c1), B1, s1, R, ptr(g1), ptr(gx),
                                ptr(gw), 0, stream_ptr(x))
        return lambda: call("mf_proj_kde1d_bwd", ptr(x), N, NDIM, ptr(V0), P, ptr(c1), B1, s1, R, ptr(g1), ptr(gx), 0, stream_ptr(x))

    def bwd2(weighted):
        if weighted:
            return lambda: call("mf_proj_wkde2d_bwd", ptr(x), ptr(w), N, NDIM, ptr(V0), ptr(V1), P, ptr(c2), B2, s2, R, ptr(c2), B2,
                                s2, R, ptr(g2), ptr(gx), ptr(gw), 0, stream_ptr(x))
        return lambda: call("mf_proj_kde2d_bwd", ptr(x), N, NDIM, ptr(V0), ptr(V1), P, ptr(c2), B2, s2, R, ptr(c2), B2, s2, R,
                            ptr(g2), ptr(gx), 0, stream_ptr(x))

    pairs = {
        "kde1d_fwd": (lambda: ops.ProjKde1dFn.apply(x, V0, c1, s1, R), lambda: ops.ProjWKde1dFn.apply(x, w, V0, c1, s1, R)),
        "kde1d_bwd": (bwd1(False), bwd1(True)),
        "kde2d_fwd": (lambda: ops.ProjKde2dFn.apply(x, *args2), lambda: ops.ProjWKde2dFn.apply(x, w, *args2)),
        "kde2d_bwd": (bwd2(False), bwd2(True)),
        "hist1d": (lambda: ops.proj_hist_counts_1d(x, V0, e1), lambda: ops.proj_whist_sums_1d(x, w, V0, e1)),
    }
    rec = dict(config="kernels", particles=N, ndim=NDIM, projections=P, bins_1d=B1, bins_2d=[B2, B2], bandwidth_bins=0.5,
               calls_per_timing=BATCH, unit_weights_bitwise_equal=dict(kde1d=same_1d, kde2d=same_2d), ms_per_call={})
    for name, (plain, weighted) in pairs.items():
        a, b = time_pair(plain, weighted, repeats)
        rec["ms_per_call"][name] = dict(unweighted=spread(a, 4), weighted=spread(b, 4), weighted_over_unweighted=round(med(b) / med(a), 4))
        print(name, rec["ms_per_call"][name], flush=True)
    return rec


def _models(dev, seed, base_scale):
    """(model with tables after one Gauss-Seidel epoch, resampling MENT, weighted MENT) sharing transforms and tables"""
    model = make_model(dev)
    torch.manual_seed(0)
    model.gauss_seidel_update(lr=0.99)                     # untimed: structured tables
    assert model.fused_args() is not None

    def with_sampler(weighted, sd):
        s = SequentialMonteCarloSampler(NDIM, chains=CHAINS, groups=GROUPS, n_temps=TEMPS, steps_per_temp=SPT,
                                        base_scale=base_scale, seed=sd).to(dev)
        m = MENT(ndim=NDIM, transforms=model.transforms, diagnostics=model.diagnostics, measurements=model.measurements,
                 prior=model.prior, mode="sample", sampler=s, n_samples=1_000_000, device=dev)
        m.weighted = weighted
        m.lagrange_functions = model.lagrange_functions
        return m

    return model, with_sampler


def run_substep(dev, repeats, base_scale, seed):
    model, with_sampler = _models(dev, seed, base_scale)
    plain, weighted = with_sampler(False, seed), with_sampler(True, seed)

    def timed(m):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.simulate(0, 0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    first = dict(resampled_ms=round(timed(plain), 3), weighted_ms=round(timed(weighted), 3))     # the ladder: untimed below
    a, b = [], []
    for _ in range(repeats):
        a.append(timed(plain))
        b.append(timed(weighted))
    return dict(config="substep", ndim=NDIM, slots=100, bins=64, chains=CHAINS, groups=GROUPS, n_temps=TEMPS, steps_per_temp=SPT,
                base_scale=base_scale, n_samples_resampled=1_000_000, first_call_with_ladder=first,
                resampled_substep_ms=spread(a, 3), weighted_substep_ms=spread(b, 3),
                resampled_over_weighted=round(med(a) / med(b), 3))


def run_rmse(dev, base_scale, seeds, res):
    model, with_sampler = _models(dev, 0, base_scale)
    n_int = NDIM - 1
    model.integration_limits = [[[(-XMAX, XMAX)] * n_int] for _ in model.transforms]
    model.integration_shape = [[(res,) * n_int] for _ in model.transforms]
    model.mode = "integrate"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = model.simulate(0, 0).double()
    torch.cuda.synchronize()
    t_ref = time.perf_counter() - t0
    err = {False: [], True: []}
    for sd in range(seeds):
        for weighted in (False, True):
            pred = with_sampler(weighted, 1000 + sd).simulate(0, 0).double()
            err[weighted].append(float(((pred - ref) ** 2).mean()))
    rms = {k: math.sqrt(sum(v) / len(v)) for k, v in err.items()}
    return dict(config="rmse", seeds=seeds, integrate_grid=[res] * n_int, integrate_seconds=round(t_ref, 2),
                largest_reference_density=round(float(ref.max()), 4), rmse_resampled_1M=round(rms[False], 6),
                rmse_weighted_65536=round(rms[True], 6), per_seed_rmse_resampled=[round(math.sqrt(v), 6) for v in err[False]],
                per_seed_rmse_weighted=[round(math.sqrt(v), 6) for v in err[True]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="", help="one of " + ", ".join(CONFIGS) + " (default: all, in one process)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--base-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--seeds", type=int, default=16, help="rmse: fresh samplers")
    ap.add_argument("--res", type=int, default=21, help="rmse: nodes per integrated axis of the integrate-mode reference")
    args = ap.parse_args()
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    names = [args.only] if args.only else list(CONFIGS)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "wproj_bench.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.setdefault("configs", {})
    out["device"] = torch.cuda.get_device_name(0)
    for name in names:
        if name == "kernels":
            rec = run_kernels(dev, args.repeats)
        elif name == "substep":
            rec = run_substep(dev, args.repeats, args.base_scale, args.seed)
        else:
            rec = run_rmse(dev, args.base_scale, args.seeds, args.res)
        print(json.dumps(rec), flush=True)
        out["configs"][name] = rec
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
