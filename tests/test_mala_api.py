"""mentflow_amd.sample.LangevinSampler through the public interface: as the sampler of a sample-mode MENT on the 2-D linear problem
(6 projections x 85 bins), persistent chains, the choice between the fused kernel and the generic torch path (MENT.log_density
or a user log-density, the gradient from autograd), refusals, and a reconstruction compared with GridSampler's.  Emulator here,
the MI355X with -m gpu."""
import logging
import math

import pytest
import torch

import mentflow_amd as mf
from _mala_fp64 import assert_transitions, verify
from mentflow_amd import ops
from mentflow_amd.ment import MENT, UniformPrior
from mentflow_amd.sample import GridSampler, LangevinSampler, MetropolisHastingsSampler
from test_mcmc_api import linear_2d, mean_discrepancy


def small_sampler(**kw):
    # start_scale 0.5: every chain starts inside the support (the measurements are non-zero for |u| <= 2.7)
    kw = dict(dict(ndim=2, chains=1024, step=0.3, burn=40, thin=5, start_scale=0.5), **kw)
    return LangevinSampler(**kw)


def test_constructor_validation():
    with pytest.raises(ValueError, match="ndim"):
        LangevinSampler(9)
    with pytest.raises(ValueError, match="step"):
        LangevinSampler(3, step=[0.1, 0.2])
    with pytest.raises(ValueError, match="step > 0"):
        LangevinSampler(2, step=[0.1, 0.0])
    with pytest.raises(ValueError, match="step > 0"):
        LangevinSampler(2, step=-0.1)
    with pytest.raises(ValueError, match="drift_clip"):
        LangevinSampler(2, drift_clip=-1.0)
    with pytest.raises(ValueError, match="drift_clip"):
        LangevinSampler(2, drift_clip=float("nan"))
    with pytest.raises(ValueError, match="start"):
        LangevinSampler(2, chains=16, start=torch.zeros(16, 3))
    with pytest.raises(ValueError, match="thin"):
        LangevinSampler(2, thin=0)
    s = LangevinSampler(3, chains=8, step=[0.1, 0.2, 0.3], drift_clip=0.0)
    assert (s.step, s.drift_clip, s.log_density, s.burn, s.thin) == ([0.1, 0.2, 0.3], 0.0, None, 200, 10)
    assert LangevinSampler(2).drift_clip == 1.0
    # the shared base must not have moved the random-walk sampler's messages
    with pytest.raises(ValueError, match="MetropolisHastingsSampler: 1 <= ndim <= 8"):
        MetropolisHastingsSampler(9)


def test_ment_runs_a_gauss_seidel_epoch_with_the_sampler(backend):
    model = linear_2d(backend, small_sampler(), n_samples=5000)          # 5000 is not a multiple of the 1024 chains
    assert model.fully_fused()
    torch.manual_seed(3)
    x = model.sample(5000)
    assert x.shape == (5000, 2) and x.dtype == torch.float32 and x.device.type == backend.type
    assert torch.isfinite(x).all() and bool((model.prob(x) > 0).all())
    assert 0.05 < float(model.sampler.acceptance) < 1.0
    preds = model.simulate_all()
    assert len(preds) == 6 and all(p[0].shape == (85,) and torch.isfinite(p[0]).all() for p in preds)
    model.gauss_seidel_update(lr=0.9)
    assert model.epoch == 1 and all(torch.isfinite(lf.values).all() for lf in mf.utils.unravel(model.lagrange_functions))
    draws = []
    for _ in range(2):                                                    # torch.manual_seed fixes a run bitwise
        m = linear_2d(backend, small_sampler(), n_samples=5000)
        torch.manual_seed(11)
        m.gauss_seidel_update(lr=0.9)
        draws.append(m.sample(3000))
    assert torch.equal(draws[0], draws[1])


def test_persistent_chains_reset_and_to(backend, monkeypatch):
    model = linear_2d(backend, small_sampler(), n_samples=5000)
    s = model.sampler
    steps = []
    real = LangevinSampler.run
    monkeypatch.setattr(LangevinSampler, "run", lambda self, f, n, **k: steps.append((n, k)) or real(self, f, n, **k))
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
    assert s.to(backend) is s and s.state.device.type == backend.type
    start = 0.3 * torch.randn(1024, 2, generator=torch.Generator().manual_seed(1))
    fresh = small_sampler(start=start, persistent=False, burn_persistent=3).to(backend)
    out = []
    for _ in range(2):                                    # persistent=False: every call starts from `start` again
        torch.manual_seed(5)
        out.append(fresh(model.prob, 2000))
        assert steps[-1][0] == 40 + 2 * 5
    assert torch.equal(out[0], out[1])
    cont = small_sampler(start=start, burn_persistent=3).to(backend)
    cont(model.prob, 2000)
    cont(model.prob, 2000)
    assert steps[-1] == (3 + 2 * 5, dict(keep_from=3 + 4, keep_every=5))


def test_fused_path_for_the_bound_ment_prob_only(backend, monkeypatch, caplog):
    model = linear_2d(backend, small_sampler(), n_samples=4000)
    calls = []
    real = ops.mala_ment_steps
    monkeypatch.setattr(ops, "mala_ment_steps", lambda *a, **k: calls.append(k["drift_clip"]) or real(*a, **k))
    generic = lambda: [r for r in caplog.records if "generic path" in r.getMessage()]
    with caplog.at_level(logging.INFO, logger="mentflow_amd.sample"):
        s = model.sampler
        s(model.prob, 1000)
        assert calls == [1.0] and not generic()
        # a wrapper is a density of its own: without a log-density there is nothing to differentiate
        g = small_sampler().to(backend)
        with pytest.raises(ValueError, match="differentiable log-density"):
            g(lambda v: model.prob(v), 1000)
        with pytest.raises(ValueError, match="differentiable log-density"):
            g(model.log_prob, 1000)
        # with a user log-density the same rule runs in torch ops, logged once per sampler
        g = small_sampler(log_density=model.log_density).to(backend)
        x = g(lambda v: model.prob(v), 1000)
        g(lambda v: model.prob(v), 1000)
        assert calls == [1.0] and x.shape == (1000, 2) and bool((model.prob(x) > 0).all())
        assert len(generic()) == 1 and "LangevinSampler" in generic()[0].getMessage()

        # a subclass that overrides prob alone: MENT.log_density is not its density
        class HalfPlane(MENT):
            def prob(self, x):
                return super().prob(x) * (x[:, 0] > 0).float()

        half = linear_2d(backend, small_sampler(start=torch.rand(1024, 2) * 0.5), n_samples=4000)
        half.__class__ = HalfPlane
        with pytest.raises(ValueError, match="differentiable log-density"):
            half.sample(2000)

        # ... and one that overrides both runs the generic path on its own log-density
        class HalfPlaneBoth(HalfPlane):
            def log_density(self, x, pad=0.0):
                return super().log_density(x) + torch.log((x[:, 0] > 0).float())

        half.__class__ = HalfPlaneBoth
        y = half.sample(2000)
        assert calls == [1.0] and bool((y[:, 0] > 0).all()) and len(generic()) == 2
    # a log-density that autograd cannot follow is refused
    blind = small_sampler(log_density=lambda v: model.log_density(v.detach())).to(backend)
    with pytest.raises(ValueError, match="differentiable"):
        blind(lambda v: model.prob(v), 100)
    with pytest.raises(ValueError, match="ndim=2"):
        LangevinSampler(3, chains=64).to(backend)(model.prob, 100)
    with pytest.raises(ValueError, match="noise"):
        small_sampler(chains=64).to(backend).run(model.prob, 10, noise=torch.zeros(10, 3, 65))


def test_generic_path_of_a_ment_with_a_torch_slot(backend, monkeypatch, caplog):
    """A 1-D MENT whose only slot sits on the offset grid [997, 1003] (not uniform in fp32: a torch slot, so no fused
    arguments): called with its bound prob the sampler takes MENT.log_density and autograd."""
    B = 30
    diag = mf.diagnostics.Histogram1D(axis=0, edges=torch.linspace(997.0, 1003.0, B + 1)).to(backend)
    sampler = LangevinSampler(1, chains=512, step=0.5, burn=20, thin=2,
                              start=1000.0 + torch.randn(512, 1, generator=torch.Generator().manual_seed(2))).to(backend)
    model = MENT(ndim=1, transforms=[mf.simulate.LinearTransform(torch.eye(1)).to(backend)], diagnostics=[[diag]],
                 measurements=[[torch.ones(B).to(backend)]], prior=UniformPrior(ndim=1, scale=2000.0), mode="sample",
                 sampler=sampler, device=backend)
    lf = model.lagrange_functions[0][0]
    lf.set_values((0.5 + torch.rand(B, generator=torch.Generator().manual_seed(3))).to(backend))
    assert not model.fully_fused() and model.fused_args() is None
    monkeypatch.setattr(ops, "mala_ment_steps", lambda *a, **k: pytest.fail("the fused kernel cannot take a torch slot"))
    torch.manual_seed(4)
    with caplog.at_level(logging.INFO, logger="mentflow_amd.sample"):
        x = model.sample(1500)
    assert len([r for r in caplog.records if "generic path" in r.getMessage()]) == 1
    c = lf.coord_list()[0]
    assert x.reshape(-1).shape == (1500,) and bool(((x >= c[0]) & (x <= c[-1])).all()), "inside the support chains stay inside"
    assert 0.3 < float(sampler.acceptance) < 1.0
    assert float(x.std()) > 0.8, "the chains spread over the 6-wide support"


def test_generic_and_fused_paths_pass_the_verifier_on_the_same_noise(backend):
    """The fused kernel (called with MENT.prob) and the torch rule on MENT.log_density (forced by a wrapper), same start, same
    noise: both trajectories pass the fp64 verifier, and they are the same chains but for those that met an ambiguous transition.
    The Lagrange functions are set uniform in [0.25, 2]: the verifier's band holds away from zeros of the tables only."""
    model = linear_2d(backend, small_sampler(), n_samples=4000)
    gen = torch.Generator().manual_seed(2)
    for lf in mf.utils.unravel(model.lagrange_functions):
        lf.set_values((0.25 + 1.75 * torch.rand(lf.values.shape, generator=gen)).to(backend))
    chain = model._get_plan()[0][0]
    slots = [(chain.rows[k], model.lagrange_functions[i][j].coord_list(), model.lagrange_functions[i][j].values)
             for k, (i, j) in enumerate(chain.slots)]
    args = model.fused_args()
    grad32 = lambda x: ops.ment_logprob(x.to(backend).contiguous(), args[0], args[1], args[2], args[3], want_grad=True)[1].cpu()
    gen = torch.Generator().manual_seed(8)
    C, T = 512, 40
    start = 0.5 * torch.randn(C, 2, generator=gen)
    noise = torch.randn(T, 3, C, generator=gen)
    noise[:, 2] = torch.rand(T, C, generator=gen)
    trajs = []
    for prob_func, log_density in ((model.prob, None), (lambda v: model.prob(v), model.log_density)):
        s = LangevinSampler(2, chains=C, step=0.3, start=start, log_density=log_density).to(backend)
        traj = s.run(prob_func, T, noise=noise.to(backend))
        assert traj.shape == (T, C, 2) and torch.equal(traj[-1], s.state)
        stats = verify(start, noise, traj, 0.3, 1.0, slots, ("gaussian", 3.0), grad32)
        print(stats, float(s.acceptance))
        assert_transitions(stats)
        assert abs(float(s.acceptance) - stats["accepted"] / stats["total"]) < 1e-6
        trajs.append(traj)
    same = (trajs[0] == trajs[1]).all(2)
    print("identical states:", float(same.float().mean()), "chains identical throughout:", float(same.all(0).float().mean()))
    assert float(same.float().mean()) > 0.9


def test_generic_path_with_a_user_log_density_is_stationary(backend):
    """The bounds of test_mala_kernels.test_stationarity for the torch path on a user log-density: N(0, s^2 I) in d = 3, chains
    started from exact draws, so the states after 20 steps are exact draws."""
    d, C, T, s = 3, 4096, 20, 1.3
    gen = torch.Generator().manual_seed(22)
    start = s * torch.randn(C, d, generator=gen)
    sampler = LangevinSampler(d, chains=C, step=0.5 * s, start=start, log_density=lambda x: -0.5 * (x * x).sum(1) / s ** 2)
    sampler.to(backend)
    torch.manual_seed(1)
    kept = sampler.run(lambda x: torch.exp(-0.5 * (x * x).sum(1) / s ** 2), T, keep_from=T - 1)
    assert kept.shape == (1, C, d) and torch.equal(kept[0], sampler.state)
    final = sampler.state.cpu().double()
    assert float(final.mean(0).abs().max()) <= 5 * s / math.sqrt(C)
    assert float((final.var(0) - s * s).abs().max()) <= 5 * s * s * math.sqrt(2.0 / (C - 1))
    assert 0.3 < float(sampler.acceptance) < 1.0


def test_reconstruction_against_grid_sampler(backend):
    """Three Gauss-Seidel epochs (lr 0.99) of the 2-D linear problem in sample mode, then the mean KL discrepancy of a fresh
    simulate_all: the gate of test_mcmc_api.test_reconstruction_against_grid_sampler, built the same way.

    On the MI355X: GridSampler on a 250 x 250 grid over [-4, 4]^2 with 1e5 samples per sub-step, torch.manual_seed(0..4), gives
    five values; with spread = (max - min) / mean of the five, the gate is
        Langevin (32 768 chains, step 0.3, burn 200, thin 20, start_scale 0.5, drift_clip 1, seed 0)  <=  max of the five * (1 + spread).
    The test forms the gate from its own five grid runs and prints the five values, the spread and the Langevin value.
    On the emulator a cut-down run (20 000 samples, 2 048 chains) only checks that the discrepancy falls from epoch 0 to 2."""
    gpu = backend.type == "cuda"
    n = 100_000 if gpu else 20_000

    def mala():
        return (LangevinSampler(2, chains=32768, step=0.3, burn=200, thin=20, start_scale=0.5) if gpu else
                LangevinSampler(2, chains=2048, step=0.3, burn=100, thin=5, start_scale=0.5))

    def three_epochs(sampler, seed):
        model = linear_2d(backend, sampler, n_samples=n, meas_samples=1_000_000 if gpu else 50_000)
        torch.manual_seed(seed)
        d = [mean_discrepancy(model)]
        for _ in range(3):
            model.gauss_seidel_update(lr=0.99)
            d.append(mean_discrepancy(model))
        return d

    d_mala = three_epochs(mala(), 0)
    print("Langevin mean discrepancy after epochs 0..3:", d_mala)
    assert all(math.isfinite(v) for v in d_mala)
    assert d_mala[2] < d_mala[0], d_mala
    if not gpu:
        return
    grid = [three_epochs(GridSampler(limits=[(-4.0, 4.0)] * 2, shape=(250, 250)), seed)[-1] for seed in range(5)]
    spread = (max(grid) - min(grid)) / (sum(grid) / len(grid))
    print("GridSampler res 250, seeds 0..4:", grid, "spread", spread, "gate", max(grid) * (1 + spread), "Langevin", d_mala[-1])
    assert d_mala[-1] <= max(grid) * (1 + spread), (d_mala[-1], grid, spread)
