"""Time the Langevin kernel (mf_mala_ment_steps) against the random-walk kernel (mf_mcmc_ment_steps) on the C4 measurement set in
6-D (100 one-D projections x 64 bins), and measure what a step is worth: the integrated autocorrelation time of each axis and,
from it, effective samples per millisecond.  For DESIGN.md section 6g; nothing here is a pass/fail threshold.

Protocol of tools/bench_mcmc.py.  Each configuration is one process that merges its record into <out>/mala_bench.json, so that
every GPU step can run under a time limit of its own and a failing step ends the chain:

    timeout -k 10 600 python tools/bench_mala.py --out profiles --only mala && \
    timeout -k 10 600 python tools/bench_mala.py --out profiles --only mh

Every process builds the same problem (seeded) and runs one untimed Gauss-Seidel epoch with the random-walk sampler, which gives
Lagrange tables with structure and 65 536 chains burnt in inside the support; the tables then stay fixed.  Then, with the
samplers' default settings (step 0.25, drift_clip 1):
  * time: `--repeats` device-synchronised wall times of one launch of 64 steps of the 65 536 chains on pre-drawn noise, every
    repeat from the same states (median, min, max), as nanoseconds per step and chain.  The `mala` configuration times both
    kernels in the same process.
  * acceptance: of that launch.
  * autocorrelation: 4 096 of the chains run 500 further steps to forget the other sampler's burn-in, then 2 000 steps with every
    state kept.  Per axis, the autocorrelation function is the mean over the chains of each chain's own (FFT) autocovariance
    divided by the mean variance, and tau = 1 + 2 sum_{k <= M} rho_k with Sokal's window, the first M >= 5 tau(M).  The spread
    is that of four groups of 1 024 chains.  effective samples per ms = 1e6 / (tau_max * ns per step and chain).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import mentflow_amd as mf  # noqa: E402
from mentflow_amd import ops  # noqa: E402
from mentflow_amd.harness import build_problem  # noqa: E402
from mentflow_amd.ment import MENT  # noqa: E402
from mentflow_amd.sample import LangevinSampler, MetropolisHastingsSampler  # noqa: E402

NDIM, XMAX, CHAINS, STEPS = 6, 3.5, 65536, 64
ACF_CHAINS, ACF_BURN, ACF_STEPS = 4096, 500, 2000
CONFIGS = ("mala", "mh")


def make_model(dev):
    p = build_problem(device=dev, seed=2, meas_samples=500_000, hidden_units=64, ndim=NDIM, num=100, bins=64, xmax=XMAX,
                      optics="nd_1d", dist_name="gaussian_mixture", prior_scale=3.0)
    sampler = MetropolisHastingsSampler(NDIM, chains=CHAINS, start_scale=0.5)
    return MENT(ndim=NDIM, transforms=p.transforms, diagnostics=p.diagnostics, measurements=p.measurements,
                prior=mf.prior.Gaussian(ndim=NDIM, scale=3.0), mode="sample", sampler=sampler.to(dev), n_samples=1_000_000,
                device=dev)


def spread(values, digits=4):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], digits), min=round(v[0], digits), max=round(v[-1], digits), n=len(v))


def draw_noise(steps, chains, dev):
    nz = torch.randn(steps, NDIM + 1, chains, device=dev)
    nz[:, NDIM].uniform_()
    return nz


def stepper(kind, args, scale, drift_clip):
    if kind == "mala":
        return lambda x, nz, acc, out=None: ops.mala_ment_steps(x, *args[:3], args[3], nz, scale, acc, drift_clip=drift_clip,
                                                                out=out)
    return lambda x, nz, acc, out=None: ops.mcmc_ment_steps(x, *args[:3], args[3], nz, scale, acc, out=out)


def time_kernel(step_fn, start, noise, repeats):
    times, rate = [], None
    for i in range(repeats + 1):                           # the first launch is untimed
        x = start.clone()
        acc = torch.zeros(x.shape[0], dtype=torch.int32, device=x.device)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step_fn(x, noise, acc)
        torch.cuda.synchronize()
        if i:
            times.append((time.perf_counter() - t0) * 1e9 / (noise.shape[0] * x.shape[0]))
        rate = float(acc.sum()) / (noise.shape[0] * x.shape[0])
    return times, rate


def iact(traj):
    """traj [T, C, d] -> tau [d]: integrated autocorrelation time per axis, Sokal's window with c = 5."""
    T = traj.shape[0]
    x = traj.double() - traj.double().mean(0, keepdim=True)
    f = torch.fft.rfft(x, n=2 * T, dim=0)
    acov = torch.fft.irfft(f * f.conj(), n=2 * T, dim=0)[:T] / torch.arange(T, 0, -1, device=x.device)[:, None, None]
    rho = (acov.mean(1) / acov[0].mean(0)).cpu()           # [T, d]
    tau_m = 1.0 + 2.0 * torch.cumsum(rho[1:], 0)           # tau with the window M = 1, 2, ...
    m = torch.arange(1, T, dtype=torch.float64)[:, None]
    ok = m >= 5.0 * tau_m
    first = torch.where(ok.any(0), ok.to(torch.int8).argmax(0), torch.full((rho.shape[1],), T - 2))
    return tau_m.gather(0, first[None])[0]


def run(name, dev, repeats):
    model = make_model(dev)
    torch.manual_seed(0)
    model.gauss_seidel_update(lr=0.99)                     # untimed: structured tables, chains burnt in inside the support
    args = model.fused_args()
    assert args is not None
    start = model.sampler.state.clone()
    default = LangevinSampler(NDIM, chains=CHAINS) if name == "mala" else model.sampler
    scale = torch.tensor(default.step, dtype=torch.float32, device=dev)
    clip = getattr(default, "drift_clip", None)
    rec = dict(config=name, ndim=NDIM, slots=100, bins=64, chains=CHAINS, steps_per_launch=STEPS, step=default.step,
               drift_clip=clip, acf_chains=ACF_CHAINS, acf_steps=ACF_STEPS)
    noise = draw_noise(STEPS, CHAINS, dev)
    fn = stepper(name, args, scale, clip)
    times, rate = time_kernel(fn, start, noise, repeats)
    rec.update(ns_per_step_and_chain=spread(times), acceptance=round(rate, 4))
    if name == "mala":                                     # the random-walk kernel in the same run, on the same noise and states
        t_mh, r_mh = time_kernel(stepper("mh", args, scale, None), start, noise, repeats)
        rec.update(mh_ns_per_step_and_chain=spread(t_mh), mh_acceptance=round(r_mh, 4),
                   time_ratio_to_mh=round(sorted(times)[len(times) // 2] / sorted(t_mh)[len(t_mh) // 2], 3))
    del noise
    x = start[:ACF_CHAINS].clone().contiguous()
    acc = torch.zeros(ACF_CHAINS, dtype=torch.int32, device=dev)
    fn(x, draw_noise(ACF_BURN, ACF_CHAINS, dev), acc)
    traj = torch.empty(ACF_STEPS, ACF_CHAINS, NDIM, device=dev)
    acc.zero_()
    fn(x, draw_noise(ACF_STEPS, ACF_CHAINS, dev), acc, out=traj)
    tau = iact(traj)
    groups = torch.stack([iact(traj[:, k::4]) for k in range(4)])
    ns = rec["ns_per_step_and_chain"]["median"]
    rec.update(acf_acceptance=round(float(acc.sum()) / (ACF_STEPS * ACF_CHAINS), 4),
               iact_per_axis=[round(float(v), 2) for v in tau],
               iact_per_axis_group_min=[round(float(v), 2) for v in groups.min(0)[0]],
               iact_per_axis_group_max=[round(float(v), 2) for v in groups.max(0)[0]],
               effective_samples_per_ms=round(1e6 / (float(tau.max()) * ns), 1))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="", help="one of " + ", ".join(CONFIGS) + " (default: all, in one process)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    names = [args.only] if args.only else list(CONFIGS)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "mala_bench.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.setdefault("configs", {})
    out["device"] = torch.cuda.get_device_name(0)
    for name in names:
        out["configs"][name] = run(name, dev, args.repeats)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
