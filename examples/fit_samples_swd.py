#!/usr/bin/env python
"""Fit a generator to samples of a distribution by minimising the sliced Wasserstein distance on one MI355X: the usage
document of `mentflow_amd.loss.SlicedWassersteinLoss` (sample-to-sample, no density needed, so the plain network works as well
as the flow).  Fresh directions and fresh target samples every step; the distance to fresh ground truth before and after is
measured as `mentflow_amd.Evaluator` measures it (same size, same metric class, under no_grad).

    python examples/fit_samples_swd.py --gen nn  --dist swissroll
    python examples/fit_samples_swd.py --gen nsf --dist rings --steps 500
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mentflow_amd as mf                                    # noqa: E402
from mentflow_amd.distributions import get_distribution      # noqa: E402
from mentflow_amd.loss import SlicedWassersteinDistance, SlicedWassersteinLoss   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gen", default="nn", choices=["nn", "nsf"])
    ap.add_argument("--dist", default="swissroll")
    ap.add_argument("--ndim", type=int, default=2)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batch-size", type=int, default=20000)
    ap.add_argument("--projections", type=int, default=50)
    ap.add_argument("--eval-size", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    torch.manual_seed(args.seed)
    truth = get_distribution(args.dist, ndim=args.ndim, seed=args.seed)
    kws = dict(transforms=3, bins=20) if args.gen == "nsf" else {}
    gen = mf.generate.build_generator(args.gen, input_features=args.ndim, output_features=args.ndim, hidden_layers=3,
                                      hidden_units=64, device=dev, **kws)
    loss_fn = SlicedWassersteinLoss(n_projections=args.projections, p=2, device=dev)
    metric = SlicedWassersteinDistance(n_projections=args.projections, p=2, device=dev)

    def distance_to_truth():
        with torch.no_grad():
            return float(metric(gen.sample(args.eval_size), truth.sample(args.eval_size).to(dev)))

    before = distance_to_truth()
    print("dist(x_model, x_true) = {}".format(before))
    opt = torch.optim.Adam(gen.parameters(), lr=1e-3)
    t0 = time.time()
    for step in range(args.steps):
        opt.zero_grad()
        loss = loss_fn(gen.sample(args.batch_size), truth.sample(args.batch_size).to(dev))     # fresh directions inside
        loss.backward()
        opt.step()
        if step % 50 == 0 or step == args.steps - 1:
            print(f"step {step:4d}  SWD {float(loss.detach()):.4f}")
    torch.cuda.synchronize()
    print(f"{args.gen}: {args.steps} steps of {args.batch_size} samples in {time.time() - t0:.1f} s")
    after = distance_to_truth()
    print("dist(x_model, x_true) = {}".format(after))
    return 0 if after < before else 1


if __name__ == "__main__":
    sys.exit(main())
