"""Time classical MENT in sample mode with the Metropolis-Hastings sampler against GridSampler on the C4 measurement set in 6-D
(100 one-D projections x 64 bins, 1 M samples per sub-step), for DESIGN.md "Metropolis-Hastings sampler".

Protocol of tools/bench_ment.py.  Per configuration: one untimed Gauss-Seidel epoch first (every op has then run once, the
chains are burnt in), then `--repeats` timed sub-steps (simulate of slot (0, 0)) and `--repeats` timed epochs, each a
device-synchronised wall time (median, min, max recorded).  After every epoch a fresh, untimed simulate_all gives the mean KL
discrepancy, so `discrepancy_after_epoch[2]` is the value after three epochs (the warm-up epoch and two timed ones).  For the MH
configurations the acceptance rate of the last timed sub-step and the HIP-event time of the kernel launches per epoch are
recorded too.  Each configuration is one process that merges its record into <out>/mcmc_bench.json, so that every GPU step can
run under a time limit of its own and a failing step ends the chain:

    timeout -k 10 600 python tools/bench_mcmc.py --out profiles --only mh_16384 && \
    timeout -k 10 600 python tools/bench_mcmc.py --out profiles --only mh_65536 && \
    timeout -k 10 600 python tools/bench_mcmc.py --out profiles --only mh_262144 && \
    timeout -k 10 600 python tools/bench_mcmc.py --out profiles --only grid_res25 && \
    timeout -k 10 600 python tools/bench_mcmc.py --out profiles --only grid_res33
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
from mentflow_amd.sample import GridSampler, MetropolisHastingsSampler  # noqa: E402

NDIM, XMAX, N_SAMPLES = 6, 3.5, 1_000_000
MH = dict(step=0.25, burn=200, thin=10, start_scale=0.5)
CONFIGS = {"mh_16384": ("mh", 16384), "mh_65536": ("mh", 65536), "mh_262144": ("mh", 262144), "grid_res25": ("grid", 25),
           "grid_res33": ("grid", 33)}


def make_model(kind, size, dev):
    p = build_problem(device=dev, seed=2, meas_samples=500_000, hidden_units=64, ndim=NDIM, num=100, bins=64, xmax=XMAX,
                      optics="nd_1d", dist_name="gaussian_mixture", prior_scale=3.0)
    sampler = (MetropolisHastingsSampler(NDIM, chains=size, **MH) if kind == "mh" else
               GridSampler(limits=NDIM * [(-XMAX, XMAX)], shape=NDIM * [size]))
    return MENT(ndim=NDIM, transforms=p.transforms, diagnostics=p.diagnostics, measurements=p.measurements,
                prior=mf.prior.Gaussian(ndim=NDIM, scale=3.0), mode="sample", sampler=sampler.to(dev), n_samples=N_SAMPLES,
                device=dev)


def spread(values):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4), n=len(v))


def mean_discrepancy(model):
    return float(torch.stack([d.float() for d in model.discrepancy_vector(model.simulate_all())]).mean())


class KernelEvents:
    """HIP events around ops.mcmc_ment_steps for the duration of a `with` block."""

    def __enter__(self):
        self.events, self.saved = [], ops.mcmc_ment_steps

        def wrapped(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self.saved(*a, **k)
            e1.record()
            self.events.append((e0, e1))
        ops.mcmc_ment_steps = wrapped
        return self

    def __exit__(self, *exc):
        ops.mcmc_ment_steps = self.saved

    def total_ms(self):
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.events)


def run(name, dev, repeats):
    kind, size = CONFIGS[name]
    model = make_model(kind, size, dev)
    torch.manual_seed(0)
    disc = []
    model.gauss_seidel_update(lr=0.99)                     # warm-up epoch, untimed
    disc.append(mean_discrepancy(model))
    torch.cuda.synchronize()
    subs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        model.simulate(0, 0)
        torch.cuda.synchronize()
        subs.append((time.perf_counter() - t0) * 1e3)
    acceptance = float(model.sampler.acceptance) if kind == "mh" else None
    epochs, kernel_ms, launches = [], [], 0
    for _ in range(repeats):
        with KernelEvents() as ke:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.gauss_seidel_update(lr=0.99)
            torch.cuda.synchronize()
            epochs.append(time.perf_counter() - t0)
        kernel_ms.append(ke.total_ms())
        launches = len(ke.events)
        disc.append(mean_discrepancy(model))
    rec = dict(config=name, sampler=kind, chains=size if kind == "mh" else None, res=size if kind == "grid" else None,
               cells=size ** NDIM if kind == "grid" else None, ndim=NDIM, slots=100, bins=64, n_samples=N_SAMPLES,
               substep_ms=spread(subs), epoch_s=spread(epochs), discrepancy_after_epoch=[round(v, 6) for v in disc],
               fully_fused=model.fully_fused())
    if kind == "mh":
        steps = model.sampler.burn_persistent + -(-N_SAMPLES // size) * model.sampler.thin
        rec.update(mh=MH, acceptance=round(acceptance, 4), steps_per_substep=steps,
                   density_evaluations_per_substep=steps * size, mcmc_kernel_ms_per_epoch=spread(kernel_ms),
                   mcmc_launches_per_epoch=launches)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="", help="one of " + ", ".join(CONFIGS) + " (default: all, in one process)")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    names = [args.only] if args.only else list(CONFIGS)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "mcmc_bench.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.setdefault("configs", {})
    out["device"] = torch.cuda.get_device_name(0)
    for name in names:
        out["configs"][name] = run(name, dev, args.repeats)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
