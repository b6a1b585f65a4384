#!/usr/bin/env python
"""Fit a normalizing flow to a classical MENT solution by reverse KL on one MI355X: the usage document of
`MENT.log_density`, the differentiable log-density of classical MENT (mentflow_amd/csrc/ment_logp.hip).

1. A small 2-D classical MENT reconstruction (swissroll, 7 linear 1-D projections, a GridSampler, a few Gauss-Seidel epochs).
2. An `nsf` generator q is fitted to it by minimising  mean_{x ~ q} [log q(x) - log p_MENT(x)]  through `log_density`: the
   particles are pulled by the gradient of the log-density kernel.  The MENT density is unnormalised, so the estimate printed
   during the fit is the reverse KL up to the constant log Z; with pad > 0 a particle outside the support counts log(pad) and is
   not pulled.  `MENT.log_normalization` (annealed importance sampling, mentflow_amd/csrc/ais.hip) estimates log Z and the
   entropy of the solution before the fit, and the absolute reverse KL is printed after it.
3. The fitted flow is a fast sampler and a density estimate of the MENT solution: its samples are compared with samples that
   Metropolis-Hastings chains draw from the same density (sliced Wasserstein distance, 50 projections).

    python examples/fit_flow_to_ment.py
    python examples/fit_flow_to_ment.py --epochs 5 --steps 600
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mentflow_amd as mf                                    # noqa: E402
from mentflow_amd.harness import build_problem               # noqa: E402
from mentflow_amd.loss import SlicedWassersteinDistance      # noqa: E402
from mentflow_amd.ment import MENT                           # noqa: E402
from mentflow_amd.sample import GridSampler, MetropolisHastingsSampler   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dist", default="swissroll")
    ap.add_argument("--epochs", type=int, default=3, help="Gauss-Seidel epochs of the MENT reconstruction")
    ap.add_argument("--steps", type=int, default=300, help="reverse-KL steps of the flow")
    ap.add_argument("--batch-size", type=int, default=8192)
    ap.add_argument("--pad", type=float, default=1e-12)
    ap.add_argument("--eval-size", type=int, default=50000)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    xmax = 3.5
    prob = build_problem(ndim=2, num=7, bins=64, xmax=xmax, seed=args.seed, dist_name=args.dist, optics="2d_linear",
                         prior_scale=3.0, device=dev, meas_samples=500_000)
    ment = MENT(ndim=2, transforms=prob.transforms, diagnostics=prob.diagnostics, measurements=prob.measurements,
                prior=mf.prior.Gaussian(ndim=2, scale=3.0), mode="sample",
                sampler=GridSampler(limits=2 * [(-xmax, xmax)], shape=(200, 200), noise=1.0).to(dev), n_samples=500_000, device=dev)
    torch.manual_seed(args.seed)
    for epoch in range(args.epochs):
        ment.gauss_seidel_update(lr=0.9)
        D = torch.stack([d.float() for d in ment.discrepancy_vector(ment.simulate_all())]).mean()
        print(f"MENT epoch {epoch}: mean KL discrepancy {float(D):.3e}")
    norm = ment.log_normalization(chains=8192, n_temps=64, steps_per_temp=2, step=0.3, base_scale=1.5)
    print(f"MENT solution: log Z = {float(norm['log_z']):.4f} +- {float(norm['log_z_se']):.4f} (effective chains "
          f"{float(norm['ess']):.0f} of 8192, acceptance {float(norm['accept_rate']):.2f}), entropy {float(norm['entropy']):.4f}")

    gen = mf.generate.build_generator("nsf", input_features=2, output_features=2, hidden_layers=3, hidden_units=64, transforms=3,
                                      bins=20, device=dev)
    opt = torch.optim.Adam(gen.parameters(), lr=1e-3)
    t0 = time.time()
    for step in range(args.steps):
        opt.zero_grad()
        x, log_q = gen.sample_and_log_prob(args.batch_size)
        kl = (log_q - ment.log_density(x, pad=args.pad)).mean()          # reverse KL up to log Z
        kl.backward()
        opt.step()
        if step % 50 == 0 or step == args.steps - 1:
            print(f"step {step:4d}  KL(q || p_MENT) - log Z = {float(kl.detach()):.4f}")
    torch.cuda.synchronize()
    print(f"{args.steps} steps of {args.batch_size} particles in {time.time() - t0:.1f} s")
    with torch.no_grad():
        x, log_q = gen.sample_and_log_prob(args.eval_size)
        kl_abs = (log_q - ment.log_density(x, pad=args.pad, normalized=True)).mean()
    print(f"KL(q || p_MENT / Z) = {float(kl_abs):.4f}   (absolute: log Z subtracted, +- {float(norm['log_z_se']):.4f} from its "
          "estimate)")

    chains = MetropolisHastingsSampler(2, chains=16384, step=0.3, burn=300, thin=10, start_scale=0.5).to(dev)
    with torch.no_grad():
        x_mh = chains(ment.prob, args.eval_size)
        x_flow = gen.sample(args.eval_size)
        swd = SlicedWassersteinDistance(n_projections=50, p=2, device=dev)
        print(f"SWD(flow samples, Metropolis-Hastings samples of the MENT density) = {float(swd(x_flow, x_mh)):.4f}")
        print(f"SWD(two independent flow batches) = {float(swd(x_flow, gen.sample(args.eval_size))):.4f}   (the noise floor)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
