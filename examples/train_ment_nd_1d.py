"""End-to-end classical MENT reconstruction of a 4-D distribution from 1-D projections (the reference's
experiments/rec_nd_1d/train_ment.py setting) on the MI355X: measurements from mentflow_amd.harness, a GridSampler at
res 33, sample mode with 1 M samples per sub-step, MENTTrainer with an mf.Evaluator as its eval hook: per epoch it prints the mean
KL discrepancy of 50 000 model samples and their sliced Wasserstein distance (50 projections, p = 2) to 50 000 fresh
ground-truth samples, as experiments/rec_nd_1d/setup.py::setup_eval does.  `--sampler mh` draws the particles from
Metropolis-Hastings chains (mentflow_amd.sample.MetropolisHastingsSampler) instead of the dense grid, `--sampler mala` from
Metropolis-adjusted Langevin chains (mentflow_amd.sample.LangevinSampler), whose proposals follow the gradient of the log-density,
`--sampler smc` from a sequential Monte Carlo population (mentflow_amd.sample.SequentialMonteCarloSampler): a temperature ladder
with resampling per island at the first sub-step, one reweighting step per later sub-step, and a running estimate of log Z,
`--sampler ais` from annealed importance sampling (mentflow_amd.sample.AnnealedImportanceSampler).  With `--weighted` (ais and smc
only) every sub-step bins the sampler's `--chains` states with their importance weights instead of `--samples` rows resampled
from them (model.weighted = True).

    python examples/train_ment_nd_1d.py [--epochs 5] [--num 50] [--res 33]
    python examples/train_ment_nd_1d.py --sampler mh [--chains 65536] [--step 0.25] [--burn 200] [--thin 10]
    python examples/train_ment_nd_1d.py --sampler mala [--drift-clip 1.0] [--chains 65536] [--step 0.25] [--burn 200] [--thin 10]
    python examples/train_ment_nd_1d.py --sampler smc [--chains 65536] [--step 0.25] [--temps 32] [--groups 8] [--ess-threshold 0.5]
    python examples/train_ment_nd_1d.py --sampler ais|smc --weighted [--chains 65536] [--temps 32]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mentflow_amd as mf  # noqa: E402
from mentflow_amd.distributions import get_distribution  # noqa: E402
from mentflow_amd.harness import build_problem  # noqa: E402
from mentflow_amd.ment import MENT  # noqa: E402
from mentflow_amd.sample import (AnnealedImportanceSampler, GridSampler, LangevinSampler,  # noqa: E402
                                 MetropolisHastingsSampler, SequentialMonteCarloSampler)
from mentflow_amd.train import MENTTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--num", type=int, default=50)
    ap.add_argument("--bins", type=int, default=85)
    ap.add_argument("--res", type=int, default=33)
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--eval-size", type=int, default=50_000)
    ap.add_argument("--sampler", choices=("grid", "mh", "mala", "smc", "ais"), default="grid")
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--step", type=float, default=0.25)
    ap.add_argument("--burn", type=int, default=200)
    ap.add_argument("--thin", type=int, default=10)
    ap.add_argument("--drift-clip", type=float, default=1.0, help="mala: bound of the drift per axis, in proposal standard deviations")
    ap.add_argument("--temps", type=int, default=32, help="smc: temperatures of the ladder")
    ap.add_argument("--groups", type=int, default=8, help="smc: independent islands")
    ap.add_argument("--ess-threshold", type=float, default=0.5, help="smc: an island resamples below this share of its size")
    ap.add_argument("--weighted", action="store_true",
                    help="ais, smc: bin the sampler's weighted states as they are instead of resampling --samples rows from them")
    args = ap.parse_args()
    if args.weighted and args.sampler not in ("ais", "smc"):
        ap.error(f"--weighted needs a sampler that carries weights (--sampler ais or smc), not {args.sampler}")
    dev = torch.device("cuda", 0)
    ndim, xmax = 4, 4.0
    prob = build_problem(ndim=ndim, num=args.num, bins=args.bins, xmax=xmax, seed=2, dist_name="gaussian_mixture",
                         prior_scale=3.0, device=dev, meas_samples=1_000_000)
    if args.sampler == "grid":
        sampler = GridSampler(limits=ndim * [(-xmax, xmax)], shape=ndim * [args.res], noise=1.0)
    elif args.sampler == "mala":
        sampler = LangevinSampler(ndim, chains=args.chains, step=args.step, burn=args.burn, thin=args.thin, start_scale=0.5,
                                  drift_clip=args.drift_clip)
    elif args.sampler == "smc":
        sampler = SequentialMonteCarloSampler(ndim, chains=args.chains, step=args.step, n_temps=args.temps, groups=args.groups,
                                              ess_threshold=args.ess_threshold, drift_clip=args.drift_clip)
    elif args.sampler == "ais":
        sampler = AnnealedImportanceSampler(ndim, chains=args.chains, step=args.step, n_temps=args.temps,
                                            drift_clip=args.drift_clip)
    else:               # chains started inside the support: a chain that starts outside it walks freely and may not return
        sampler = MetropolisHastingsSampler(ndim, chains=args.chains, step=args.step, burn=args.burn, thin=args.thin,
                                            start_scale=0.5)
    model = MENT(ndim=ndim, transforms=prob.transforms, diagnostics=prob.diagnostics, measurements=prob.measurements,
                 prior=mf.prior.Gaussian(ndim=ndim, scale=3.0), mode="sample", sampler=sampler.to(dev),
                 n_samples=args.samples, device=dev)
    model.weighted = args.weighted

    # the ground truth of build_problem (same name, ndim and seed), drawn afresh at every evaluation
    evaluate = mf.Evaluator(args.eval_size, distance=mf.loss.SlicedWassersteinDistance(n_projections=50, p=2, device=dev),
                            distribution=get_distribution("gaussian_mixture", ndim=ndim, seed=2))
    trainer = MENTTrainer(model=model, eval=evaluate)
    trainer.train(epochs=args.epochs, lr=0.99)
    if args.sampler == "smc":
        print("running log Z of the population:", round(float(sampler.log_z), 4))
    print("mean KL discrepancy per epoch:", [f"{v:.3e}" for v in trainer.history["D_norm"]])
    print("time per epoch (s):", [round(b - a, 3) for a, b in zip(trainer.history["time"], trainer.history["time"][1:])])


if __name__ == "__main__":
    main()
