"""The Metropolis-Hastings sampler at C4's scale on the MI355X: the 6-D measurement set of 100 one-D projections x 64 bins,
65 536 chains.  Transitions of a fixed random subset of 256 chains over 64 steps are verified in fp64 (tests/_mcmc_fp64.py: no
disagreement outside the band, at most 0.5 % ambiguous), a rerun is bitwise equal, and one sample-mode Gauss-Seidel sub-step with
the sampler returns only points of non-zero density.  Times are printed, not gated."""
import time

import pytest
import torch

from _mcmc_fp64 import assert_transitions, verify

CHAINS, STEPS = 65536, 64


def c4_model(dev, sampler):
    import mentflow_amd as mf
    from mentflow_amd.harness import build_problem
    from mentflow_amd.ment import MENT
    prob = build_problem(ndim=6, num=100, bins=64, xmax=3.5, seed=2, prior_scale=3.0, device=dev, dist_name="gaussian_mixture",
                         meas_samples=200000)
    return MENT(ndim=6, transforms=prob.transforms, diagnostics=prob.diagnostics, measurements=prob.measurements,
                prior=mf.prior.Gaussian(ndim=6, scale=3.0), mode="sample", sampler=sampler.to(dev), n_samples=1_000_000,
                device=dev)


@pytest.mark.gpu
def test_c4_transitions_rerun_and_substep():
    import mentflow_amd as mf
    from mentflow_amd import _lib
    from mentflow_amd.sample import MetropolisHastingsSampler
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    # start_scale 0.5: every chain starts inside the support (a chain outside it walks freely and, in 6-D, rarely returns)
    model = c4_model(dev, MetropolisHastingsSampler(6, chains=CHAINS, step=0.25, burn=200, thin=10, start_scale=0.5))
    assert model.fully_fused()
    torch.manual_seed(0)
    model.gauss_seidel_update(lr=0.9)                 # tables with structure, not only the 0 / 1 of the first epoch
    sampler = model.sampler
    assert bool((model.prob(sampler.state) > 0).all())

    gen = torch.Generator().manual_seed(4)
    start = sampler.state.clone()
    noise = torch.randn(STEPS, 7, CHAINS, generator=gen)
    noise[:, 6] = torch.rand(STEPS, CHAINS, generator=gen)
    noise = noise.to(dev)
    runs = []
    for _ in range(2):
        sampler.state = start.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        traj = sampler.run(model.prob, STEPS, noise=noise)
        torch.cuda.synchronize()
        runs.append((traj, sampler.state.clone(), float(sampler.acceptance), time.perf_counter() - t0))
    print(f"C4 6-D, {CHAINS} chains x {STEPS} steps x 100 slots: {runs[1][3] * 1e3:.2f} ms, acceptance {runs[1][2]:.3f}")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert traj.shape == (STEPS, CHAINS, 6) and torch.isfinite(traj).all()

    subset = torch.randperm(CHAINS, generator=torch.Generator().manual_seed(5))[:256]
    chain = model._get_plan()[0][0]
    slots = [(chain.rows[k], model.lagrange_functions[i][j].coord_list(), model.lagrange_functions[i][j].values)
             for k, (i, j) in enumerate(chain.slots)]
    stats = verify(start.cpu()[subset], noise.cpu()[:, :, subset], traj.cpu()[:, subset], 0.25, slots, ("gaussian", 3.0))
    print(stats)
    assert_transitions(stats)
    assert stats["accepted"] > 0.05 * stats["total"]

    # one sample-mode sub-step with the sampler: 1 M samples = 16 rounds of the 65 536 chains
    torch.manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pred = model.simulate(0, 0)
    torch.cuda.synchronize()
    print(f"one sample-mode simulate (burn {sampler.burn_persistent} + 16 x {sampler.thin} steps + KDE): "
          f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
    assert torch.isfinite(pred).all()
    x = model.sample(1_000_000)
    assert x.shape == (1_000_000, 6) and bool((model.prob(x) > 0).all())
    model.gauss_seidel_update(lr=0.9)
    assert all(torch.isfinite(lf.values).all() for lf in mf.utils.unravel(model.lagrange_functions))
