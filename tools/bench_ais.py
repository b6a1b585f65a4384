"""Time the annealed-importance-sampling kernel (mf_ais_ment_steps) beside the Langevin kernel (mf_mala_ment_steps) on the C4
measurement set in 6-D (100 one-D projections x 64 bins), and measure what a ladder is worth: the effective sample size and the
standard error of log Z against the number of temperatures.  For DESIGN.md section 6i; nothing here is a pass/fail threshold.

Protocol of tools/bench_mala.py.  Each configuration is one process that merges its record into <out>/ais_bench.json, so that
every GPU step can run under a time limit of its own and a failing step ends the chain:

    timeout -k 10 600 python tools/bench_ais.py --out profiles --only time && \
    timeout -k 10 600 python tools/bench_ais.py --out profiles --only ladder

Every process builds bench_mala.py's problem (seeded) and runs its one untimed Gauss-Seidel epoch with the random-walk sampler:
Lagrange tables with structure and 65 536 chains burnt in inside the support; the tables then stay fixed.
  * time: `--repeats` device-synchronised wall times of one launch of 32 temperatures x 2 transitions of the 65 536 chains on
    pre-drawn noise (the ladder linspace(0, 1, 33), the samplers' default step 0.25 and drift_clip 1, base N(0, base_scale^2)),
    every repeat from the same burnt-in states (median, min, max), as nanoseconds per chain and transition; then one launch of
    the Langevin kernel with the same 64 rows of noise, the same states and the same step, in the same process.
  * ladder: MENT.log_normalization with 16 384 chains, 2 transitions per temperature and n_temps = 8 .. 256: log_z, log_z_se,
    ess / C and the acceptance rate per ladder, one seed each (the seed is recorded)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_mala import CHAINS, NDIM, draw_noise, make_model, spread, stepper, time_kernel  # noqa: E402
from mentflow_amd import ops  # noqa: E402
from mentflow_amd.sample import AnnealedImportanceSampler  # noqa: E402

TEMPS, SPT = 32, 2
LADDER_CHAINS, LADDERS = 16384, (8, 16, 32, 64, 128, 256)
CONFIGS = ("time", "ladder")


def run_time(model, dev, repeats, base_scale):
    args = model.fused_args()
    start = model.sampler.state.clone()
    default = AnnealedImportanceSampler(NDIM, chains=CHAINS, n_temps=TEMPS, steps_per_temp=SPT)
    scale = torch.tensor(default.step, dtype=torch.float32, device=dev)
    betas = default.betas.to(dev)
    noise = draw_noise(TEMPS * SPT, CHAINS, dev)
    mean, base = [0.0] * NDIM, [base_scale] * NDIM

    def ais(x, nz, acc, out=None):
        logw = torch.zeros(x.shape[0], dtype=torch.float64, device=dev)
        ops.ais_ment_steps(x, *args[:3], args[3], nz, betas, SPT, scale, mean, base, logw, acc, drift_clip=default.drift_clip)

    times, rate = time_kernel(ais, start, noise, repeats)
    t_mala, r_mala = time_kernel(stepper("mala", args, scale, default.drift_clip), start, noise, repeats)
    med = lambda v: sorted(v)[len(v) // 2]
    return dict(config="time", ndim=NDIM, slots=100, bins=64, chains=CHAINS, temps_per_launch=TEMPS, steps_per_temp=SPT,
                step=default.step, drift_clip=default.drift_clip, base_scale=base_scale,
                ns_per_chain_and_transition=spread(times), acceptance=round(rate, 4),
                mala_ns_per_step_and_chain=spread(t_mala), mala_acceptance=round(r_mala, 4),
                time_ratio_to_mala=round(med(times) / med(t_mala), 3))


def run_ladder(model, dev, base_scale, seed):
    rows = []
    for n_temps in LADDERS:
        res = model.log_normalization(chains=LADDER_CHAINS, n_temps=n_temps, steps_per_temp=SPT, base_scale=base_scale, seed=seed)
        rows.append(dict(n_temps=n_temps, log_z=round(float(res["log_z"]), 4), log_z_se=round(float(res["log_z_se"]), 4),
                         ess_over_chains=round(float(res["ess"]) / LADDER_CHAINS, 4), entropy=round(float(res["entropy"]), 4),
                         accept_rate=round(float(res["accept_rate"]), 4)))
        print(json.dumps(rows[-1]), flush=True)
    return dict(config="ladder", ndim=NDIM, slots=100, bins=64, chains=LADDER_CHAINS, steps_per_temp=SPT, base_scale=base_scale,
                seed=seed, ladders=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="", help="one of " + ", ".join(CONFIGS) + " (default: all, in one process)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--base-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    names = [args.only] if args.only else list(CONFIGS)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "ais_bench.json")
    out = json.load(open(path)) if os.path.exists(path) else {}
    out.setdefault("configs", {})
    out["device"] = torch.cuda.get_device_name(0)
    for name in names:
        model = make_model(dev)
        torch.manual_seed(0)
        model.gauss_seidel_update(lr=0.99)                 # untimed: structured tables, chains burnt in inside the support
        assert model.fused_args() is not None
        rec = run_time(model, dev, args.repeats, args.base_scale) if name == "time" else run_ladder(model, dev, args.base_scale,
                                                                                                    args.seed)
        print(json.dumps(rec), flush=True)
        out["configs"][name] = rec
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
