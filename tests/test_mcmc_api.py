"""mentflow_amd.sample.MetropolisHastingsSampler through the public interface: as the sampler of a sample-mode MENT on the 2-D
linear problem (6 projections x 85 bins), persistent chains, save / load, the choice between the fused kernel and the generic
torch path, refusals, and a reconstruction compared with GridSampler's.  Emulator here, the MI355X with -m gpu."""
import logging
import math
import os

import pytest
import torch

import mentflow_amd as mf
from _mcmc_fp64 import assert_transitions, verify
from mentflow_amd import _lib, ops
from mentflow_amd.harness import build_problem
from mentflow_amd.ment import MENT
from mentflow_amd.sample import GridSampler, MetropolisHastingsSampler


def linear_2d(device, sampler, n_samples, meas_samples=50000):
    p = build_problem(ndim=2, num=6, bins=85, xmax=4.0, optics="2d_linear", dist_name="rings", prior_scale=3.0, seed=2,
                      device=device, meas_samples=meas_samples)
    return MENT(ndim=2, transforms=p.transforms, diagnostics=p.diagnostics, measurements=p.measurements,
                prior=mf.prior.Gaussian(ndim=2, scale=3.0), mode="sample", sampler=sampler.to(device), n_samples=n_samples,
                device=device)


def mean_discrepancy(model):
    return float(torch.stack([d.float() for d in model.discrepancy_vector(model.simulate_all())]).mean())


def small_sampler(**kw):
    # start_scale 0.5: every chain starts inside the support (the measurements are non-zero for |u| <= 2.7), where the rule
    # keeps it; a chain that starts outside walks freely and need not find the support within the burn-in
    kw = dict(dict(ndim=2, chains=1024, step=0.3, burn=40, thin=5, start_scale=0.5), **kw)
    return MetropolisHastingsSampler(**kw)


def test_ment_runs_with_the_sampler(backend):
    model = linear_2d(backend, small_sampler(), n_samples=5000)          # 5000 is not a multiple of the 1024 chains
    assert model.fully_fused()
    torch.manual_seed(3)
    x = model.sample(5000)
    assert x.shape == (5000, 2) and x.dtype == torch.float32 and x.device.type == backend.type
    assert torch.isfinite(x).all() and bool((model.prob(x) > 0).all())
    assert 0.05 < float(model.sampler.acceptance) < 0.95
    assert model.sample(700).shape == (700, 2)
    pred = model.simulate(1, 0)
    width = float(model.diagnostics[1][0].edges[1] - model.diagnostics[1][0].edges[0])
    assert pred.shape == (85,) and abs(float(pred.sum()) * width - 1.0) < 1e-4
    preds = model.simulate_all()
    assert len(preds) == 6 and all(p[0].shape == (85,) and torch.isfinite(p[0]).all() for p in preds)
    model.gauss_seidel_update(lr=0.9)
    assert model.epoch == 1 and all(torch.isfinite(lf.values).all() for lf in mf.utils.unravel(model.lagrange_functions))
    # torch.manual_seed fixes a run bitwise
    draws = []
    for _ in range(2):
        m = linear_2d(backend, small_sampler(), n_samples=5000)
        torch.manual_seed(11)
        m.gauss_seidel_update(lr=0.9)
        draws.append((m.sample(3000), torch.cat([lf.values for lf in mf.utils.unravel(m.lagrange_functions)])))
    assert torch.equal(draws[0][0], draws[1][0]) and torch.equal(draws[0][1], draws[1][1])


def test_persistent_chains_and_reset(backend, monkeypatch):
    model = linear_2d(backend, small_sampler(), n_samples=5000)
    s = model.sampler
    steps = []
    real = MetropolisHastingsSampler.run
    monkeypatch.setattr(MetropolisHastingsSampler, "run", lambda self, f, n, **k: steps.append((n, k)) or real(self, f, n, **k))
    assert s.state is None
    s(model.prob, 3000)                                   # 3 rounds of 1024: burn 40 + 3 * 5 steps, rows 44, 49, 54 kept
    assert steps[-1] == (55, dict(keep_from=44, keep_every=5))
    first = s.state.clone()
    s(model.prob, 1024)                                   # continues: burn_persistent = thin = 5, then one round
    assert steps[-1] == (10, dict(keep_from=9, keep_every=5))
    assert not torch.equal(s.state, first) and bool((model.prob(s.state) > 0).all())
    s.reset()
    assert s.state is None
    s(model.prob, 10)
    assert steps[-1][0] == 45
    # persistent=False: every call starts from `start` again, so equal noise gives equal draws
    start = 0.3 * torch.randn(1024, 2, generator=torch.Generator().manual_seed(1))
    fresh = small_sampler(start=start, persistent=False, burn_persistent=3).to(backend)
    out = []
    for _ in range(2):
        torch.manual_seed(5)
        out.append(fresh(model.prob, 2000))
        assert steps[-1][0] == 40 + 2 * 5
    assert torch.equal(out[0], out[1])
    cont = small_sampler(start=start, burn_persistent=3).to(backend)
    cont(model.prob, 2000)
    cont(model.prob, 2000)
    assert steps[-1] == (3 + 2 * 5, dict(keep_from=3 + 4, keep_every=5))


def test_save_load_and_to(backend, tmp_path):
    model = linear_2d(backend, small_sampler(step=[0.3, 0.2]), n_samples=4000)
    torch.manual_seed(0)
    model.gauss_seidel_update(lr=0.9)
    path = str(tmp_path / "ment_mh.pt")
    model.save(path)
    other = linear_2d(backend, small_sampler(chains=64), n_samples=4000)
    other.load(path, device=backend)
    s, o = model.sampler, other.sampler
    assert isinstance(o, MetropolisHastingsSampler) and o is not s
    assert (o.ndim, o.chains, o.step, o.burn, o.thin, o.persistent) == (2, 1024, [0.3, 0.2], 40, 5, True)
    assert torch.equal(o.state, s.state) and o.to(backend) is o
    torch.manual_seed(7)
    a = model.sample(2000)
    torch.manual_seed(7)
    b = other.sample(2000)
    assert torch.equal(a, b)


def test_fused_path_for_the_bound_ment_prob_only(backend, monkeypatch, caplog):
    model = linear_2d(backend, small_sampler(), n_samples=4000)
    calls = []
    real = ops.mcmc_ment_steps
    monkeypatch.setattr(ops, "mcmc_ment_steps", lambda *a, **k: calls.append(1) or real(*a, **k))
    with caplog.at_level(logging.INFO, logger="mentflow_amd.sample"):
        s = model.sampler
        s(model.prob, 1000)
        assert calls == [1] and not [r for r in caplog.records if "generic path" in r.getMessage()]
        # a wrapper, and a subclass's override, are densities of their own: the same rule in torch ops, logged once per sampler
        g = small_sampler().to(backend)
        x = g(lambda v: model.prob(v), 1000)
        g(lambda v: model.prob(v), 1000)
        assert calls == [1] and x.shape == (1000, 2)
        assert len([r for r in caplog.records if "generic path" in r.getMessage()]) == 1

        class HalfPlane(MENT):
            def prob(self, x):
                return super().prob(x) * (x[:, 0] > 0).float()

        half = linear_2d(backend, small_sampler(start=torch.rand(1024, 2) * 0.5), n_samples=4000)
        half.__class__ = HalfPlane
        y = half.sample(2000)
        assert calls == [1] and bool((y[:, 0] > 0).all())
        assert len([r for r in caplog.records if "generic path" in r.getMessage()]) == 2


def test_generic_path_is_stationary_on_a_gaussian(backend):
    """The bounds of test_mcmc_kernels.test_stationarity_and_acceptance_rate, for the torch path on a user density."""
    d, C, T, s = 3, 8192, 20, 1.3
    gen = torch.Generator().manual_seed(22)
    start = s * torch.randn(C, d, generator=gen)
    sampler = MetropolisHastingsSampler(d, chains=C, step=2.4 * s / math.sqrt(d), start=start).to(backend)
    torch.manual_seed(1)
    kept = sampler.run(lambda x: torch.exp(-0.5 * (x * x).sum(1) / s ** 2), T, keep_from=T - 1)
    assert kept.shape == (1, C, d) and torch.equal(kept[0], sampler.state)
    final = sampler.state.cpu().double()
    assert float(final.mean(0).abs().max()) <= 5 * s / math.sqrt(C)
    assert float((final.var(0) - s * s).abs().max()) <= 5 * s * s * math.sqrt(2.0 / (C - 1))
    assert 0.1 < float(sampler.acceptance) < 0.6


def test_generic_and_fused_paths_pass_the_verifier_on_the_same_noise(backend):
    model = linear_2d(backend, small_sampler(), n_samples=4000)
    torch.manual_seed(2)
    model.gauss_seidel_update(lr=0.9)
    chain = model._get_plan()[0][0]
    slots = [(chain.rows[k], model.lagrange_functions[i][j].coord_list(), model.lagrange_functions[i][j].values)
             for k, (i, j) in enumerate(chain.slots)]
    gen = torch.Generator().manual_seed(8)
    C, T = 512, 40
    start = 0.8 * torch.randn(C, 2, generator=gen)
    noise = torch.randn(T, 3, C, generator=gen)
    noise[:, 2] = torch.rand(T, C, generator=gen)
    trajs = []
    for prob_func in (model.prob, lambda v: model.prob(v)):
        s = MetropolisHastingsSampler(2, chains=C, step=0.3, start=start).to(backend)
        traj = s.run(prob_func, T, noise=noise.to(backend))
        assert traj.shape == (T, C, 2) and torch.equal(traj[-1], s.state)
        stats = verify(start, noise, traj, 0.3, slots, ("gaussian", 3.0))
        print(stats, float(s.acceptance))
        assert_transitions(stats)
        assert abs(float(s.acceptance) - stats["accepted"] / stats["total"]) < 1e-6
        trajs.append(traj)
    assert float((trajs[0] == trajs[1]).all(2).float().mean()) > 0.95      # the same chains but for those that met an ambiguous transition


def test_bad_arguments_raise(backend):
    with pytest.raises(ValueError, match="ndim"):
        MetropolisHastingsSampler(9)
    with pytest.raises(ValueError, match="step"):
        MetropolisHastingsSampler(3, step=[0.1, 0.2])
    with pytest.raises(ValueError, match="start"):
        MetropolisHastingsSampler(2, chains=16, start=torch.zeros(16, 3))
    model = linear_2d(backend, small_sampler(), n_samples=2000)
    with pytest.raises(ValueError, match="ndim=2"):
        MetropolisHastingsSampler(3, chains=64).to(backend)(model.prob, 100)
    s = small_sampler(chains=64).to(backend)
    with pytest.raises(ValueError, match="noise"):
        s.run(model.prob, 10, noise=torch.zeros(10, 3, 65))
    with pytest.raises(ValueError, match="noise"):
        s.run(model.prob, 10, noise=torch.zeros(9, 3, 64))
    with pytest.raises(ValueError, match="keep_every"):
        s.run(model.prob, 10, keep_every=0)


def test_no_cpu_fallback():
    import __graft_entry__ as g
    if not os.path.exists(g.LIB):
        g.build()
    _lib.use_library(g.LIB)
    s = MetropolisHastingsSampler(2, chains=64, start=torch.zeros(64, 2), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s(lambda x: torch.exp(-(x * x).sum(1)), 100)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mcmc_ment_steps(torch.zeros(64, 2), torch.zeros(0, 24), torch.zeros(0, 4, dtype=torch.int32), torch.zeros(1),
                            (1, 1.0, 0.0), torch.zeros(4, 3, 64), torch.ones(2), torch.zeros(64, dtype=torch.int32))


def test_reconstruction_against_grid_sampler(backend):
    """Three Gauss-Seidel epochs (lr 0.99) of the 2-D linear problem in sample mode, then the mean KL discrepancy of a fresh
    simulate_all.

    On the MI355X: GridSampler on a 250 x 250 grid over [-4, 4]^2 with 1e5 samples per sub-step, torch.manual_seed(0..4), gives
    five values; with spread = (max - min) / mean of the five, the gate is
        MH (32 768 chains, step 0.3, burn 200, thin 20, start_scale 0.5, seed 0)  <=  max of the five * (1 + spread).
    The rule was fixed before the first run.  The test forms the gate from its own five grid runs and prints the five values,
    the spread and the MH value.  No figures are recorded yet: this test has not run on an MI355X.
    On the emulator a cut-down run (20 000 samples, 2 048 chains) only checks that the discrepancy falls from epoch 0 to 2."""
    gpu = backend.type == "cuda"
    n = 100_000 if gpu else 20_000

    def mh():
        return (MetropolisHastingsSampler(2, chains=32768, step=0.3, burn=200, thin=20, start_scale=0.5) if gpu else
                MetropolisHastingsSampler(2, chains=2048, step=0.3, burn=100, thin=5, start_scale=0.5))

    def three_epochs(sampler, seed):
        model = linear_2d(backend, sampler, n_samples=n, meas_samples=1_000_000 if gpu else 50_000)
        torch.manual_seed(seed)
        d = [mean_discrepancy(model)]
        for _ in range(3):
            model.gauss_seidel_update(lr=0.99)
            d.append(mean_discrepancy(model))
        return d

    d_mh = three_epochs(mh(), 0)
    print("MH mean discrepancy after epochs 0..3:", d_mh)
    assert all(math.isfinite(v) for v in d_mh)
    assert d_mh[2] < d_mh[0], d_mh
    if not gpu:
        return
    grid = [three_epochs(GridSampler(limits=[(-4.0, 4.0)] * 2, shape=(250, 250)), seed)[-1] for seed in range(5)]
    spread = (max(grid) - min(grid)) / (sum(grid) / len(grid))
    print("GridSampler res 250, seeds 0..4:", grid, "spread", spread, "gate", max(grid) * (1 + spread), "MH", d_mh[-1])
    assert d_mh[-1] <= max(grid) * (1 + spread), (d_mh[-1], grid, spread)
