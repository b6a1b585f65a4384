"""sample.SequentialMonteCarloSampler and MENT.log_normalization with it, through the public interface, against fp64 quadrature
of tests/_ment_logp_fp64.logp64 (the densities, settings and references of tests/test_ais_api.py).  Emulator here, the MI355X with
-m gpu.

Settings: 2 048 chains in 8 islands, 2 transitions per temperature, step 0.5, drift_clip 1, base N(0, 1.5^2).  Ladders of 8
temperatures on case (b), where AnnealedImportanceSampler ends at ess / C = 0.42, and of 32 on case (a).

The fp64 prototype of the sampler (tests/_smc_fp64.py, `python tests/_smc_fp64.py`; five seeds per configuration) gave at worst:

  configuration                    |d log Z|  |d H|   ess / C          accept           island se          |d log Z| / se
  (b),  8 temperatures, thr 0.5     0.047     0.088   0.772 .. 0.963   0.840 .. 0.846   0.0082 .. 0.0231   4.6
  (b),  8 temperatures, thr 1.1     0.046     0.044   0.977 .. 0.980   0.842 .. 0.845   0.0120 .. 0.0256   2.8
  (a), 32 temperatures, thr 1.1     0.016     0.022   0.998 .. 0.999   0.902 .. 0.906   0.0077 .. 0.0134   2.1
  (b),  8 temperatures, thr 0       0.048     0.084   0.415 .. 0.431   (no resampling: AnnealedImportanceSampler)

Gates, at about twice the worst prototype value: |d log Z| <= 0.12, |d H| <= 0.18, accept >= 0.6, 0 < log_z_se <= 0.08, and
ess / C >= 0.8 at threshold 1.1.  At threshold 0.5 the prototype's worst ess / C is 0.772, below the 0.939 the gate of 0.8 was
first derived from: the last decision precedes the last temperature, and an island that stood just above half its size there is
not resampled.  The prototype decides: twice its worst shortfall from 1 gives ess / C >= 1 - 2 (1 - 0.772) = 0.54 there.
|d log Z| / log_z_se reaches 4.6 with 8 islands and is not gated.

The bridge (table 0 of case (b) times exp(sin(1.3 centres)), a factor in [0.37, 2.71]; ten runs): |d log Z| <= 0.026, the mean of
65 536 returned points within 0.029 of 1-D quadrature on every axis, island ess / S >= 0.70 before the resampling.  Gates:
|d log Z| <= 0.14 and 0.11 per axis for the mean."""
import math

import pytest
import torch

import mentflow_amd as mf
from _smc_fp64 import bridge_reference
from mentflow_amd import ops
from mentflow_amd.ment import MENT
from mentflow_amd.sample import AnnealedImportanceSampler, SequentialMonteCarloSampler
from test_ais_api import CENTRES, EDGES, build, reference
from test_ais_api import SETTINGS as AIS_SETTINGS

SETTINGS = dict(chains=2048, groups=8, steps_per_temp=2, step=0.5, drift_clip=1.0, base_scale=1.5)
KEYS = ("x", "logw", "logp", "accepted")


def test_threshold_zero_is_annealed_importance_sampling(backend, monkeypatch):
    model, _ = build("a", backend)
    monkeypatch.setattr(ops, "smc_resample", lambda *a, **k: pytest.fail("threshold 0 known on the host: no resampling launch"))
    ais = AnnealedImportanceSampler(2, seed=5, **AIS_SETTINGS).to(backend).run(model)
    for every in (1, 5):
        smc = SequentialMonteCarloSampler(2, ess_threshold=0, seed=5, resample_every=every, **AIS_SETTINGS).to(backend).run(model)
        assert all(torch.equal(smc[k], ais[k]) for k in KEYS)
        assert float(smc["resampled"]) == 0 and smc["log_z_groups"].shape == (8,) and smc["log_z_groups"].dtype == torch.float64
    monkeypatch.undo()
    smc = SequentialMonteCarloSampler(2, ess_threshold=1.1, seed=5, **AIS_SETTINGS).to(backend).run(model)
    assert float(smc["resampled"]) == 8 * (AIS_SETTINGS["n_temps"] - 1), "every island at every temperature but the last"
    assert not torch.equal(smc["x"], ais["x"])


@pytest.mark.parametrize("case,n_temps,threshold,ess_gate", [("b", 8, 0.5, 0.54), ("b", 8, 1.1, 0.8), ("a", 32, 1.1, 0.8)])
def test_log_z_entropy_and_ess_against_quadrature(backend, case, n_temps, threshold, ess_gate):
    """Gates and the prototype's figures: module docstring.  Measured on the emulator and the MI355X: DESIGN.md 6j."""
    model, _ = build(case, backend)
    ref_log_z, ref_h = reference(case)
    sampler = SequentialMonteCarloSampler(model.ndim, n_temps=n_temps, ess_threshold=threshold, seed=5, **SETTINGS).to(backend)
    res = model.log_normalization(sampler)
    assert all(v.dim() == 0 and v.dtype == torch.float64 and v.device.type == backend.type for v in res.values())
    log_z, se, ess, h, rate = (float(res[k]) for k in ("log_z", "log_z_se", "ess", "entropy", "accept_rate"))
    print(f"case {case}, {n_temps} temperatures, threshold {threshold}: log Z {log_z:.5f} (quadrature {ref_log_z:.5f}, |d| "
          f"{abs(log_z - ref_log_z):.5f}), log_z_se {se:.5f}, ess / C {ess / SETTINGS['chains']:.4f}, H {h:.5f} (quadrature "
          f"{ref_h:.5f}, |d| {abs(h - ref_h):.5f}), accept {rate:.4f}, resampled {float(sampler.last['resampled']):.0f}")
    # the formulas of MENT.log_normalization restated from the islands' estimates
    lzg = sampler.last["log_z_groups"].cpu()
    expect = float(torch.logsumexp(lzg, 0)) - math.log(8)
    assert abs(log_z - expect) <= 1e-12 * (1 + abs(expect))
    expect_se = float(torch.exp(lzg - expect).std(unbiased=True)) / math.sqrt(8)
    assert abs(se - expect_se) <= 1e-12 * (1 + expect_se)
    per = sampler.last["logw"].cpu().view(8, -1)
    assert float((lzg - (torch.logsumexp(per, 1) - math.log(per.shape[1]))).abs().max()) <= 1e-12
    assert abs(log_z - ref_log_z) <= 0.12
    assert abs(h - ref_h) <= 0.18
    assert ess / SETTINGS["chains"] >= ess_gate
    assert rate >= 0.6
    assert 0 < se <= 0.08
    assert model.log_z is res["log_z"] and float(sampler.log_z) == log_z
    assert float(sampler.last["resampled"]) > 0 and sampler.last["ess_groups"].shape == (8,)


def test_one_island_has_no_standard_error(backend):
    model, _ = build("a", backend)
    s = SequentialMonteCarloSampler(2, n_temps=4, seed=1, **dict(SETTINGS, chains=256, groups=1)).to(backend)
    res = model.log_normalization(s)
    assert math.isnan(float(res["log_z_se"])) and math.isfinite(float(res["log_z"]))
    with pytest.raises(TypeError, match="either"):
        model.log_normalization(s, chains=16)


def changed_tables(model, backend):
    """Table 0 of case (b) times exp(sin(1.3 centres)): a factor in [0.37, 2.71]."""
    lf = model.lagrange_functions[0][0]
    lf.set_values(lf.values * torch.exp(torch.sin(1.3 * CENTRES)).to(backend))


def test_bridge_reweights_exactly(backend):
    model, _ = build("b", backend)
    s = SequentialMonteCarloSampler(6, n_temps=8, ess_threshold=0, bridge_steps=0, seed=3, **SETTINGS).to(backend)
    model.sampler = s
    model.sample(1000)                                        # the whole ladder
    pop = {k: v.clone() for k, v in s.population.items()}
    args = model.fused_args()
    lp_old = ops.ment_logprob(pop["x"], args[0], args[1], args[2], args[3])[0]
    assert torch.equal(lp_old.view(torch.int32), pop["logp"].view(torch.int32)), "the population carries ment_logprob's bits"
    assert torch.isfinite(pop["logw"]).all()
    changed_tables(model, backend)
    model.sample(1000)                                        # the bridge: no resampling, no moves before the collection
    args = model.fused_args()
    lp_new = ops.ment_logprob(pop["x"], args[0], args[1], args[2], args[3])[0]
    assert not torch.equal(lp_new, lp_old)
    expect = pop["logw"] + (lp_new.double() - lp_old.double())
    assert torch.equal(s.last["logw"].view(torch.int64), expect.view(torch.int64))
    assert torch.equal(s.last["x"], pop["x"]) and torch.equal(s.last["logp"].view(torch.int32), lp_new.view(torch.int32))
    assert float(s.last["resampled"]) == 0
    # a state without weight, or outside the new support, gets weight 0 and no NaN is formed
    s.population["logw"][:3] = float("-inf")
    s.population["logp"][3:5] = float("-inf")
    s.population["x"][5] = 30.0
    model.sample(10)
    assert torch.isneginf(s.last["logw"][:6]).all() and not torch.isnan(s.last["logw"]).any()
    assert torch.isfinite(s.last["logw"][6:]).all()


def test_bridge_follows_the_tables(backend):
    model, slots = build("b", backend)
    s = SequentialMonteCarloSampler(6, n_temps=8, ess_threshold=0.5, bridge_steps=4, seed=7, **SETTINGS).to(backend)
    model.sampler = s
    model.sample(2048)
    old_log_z = float(s.log_z)
    assert abs(old_log_z - reference("b")[0]) <= 0.12
    changed_tables(model, backend)
    factor = torch.exp(torch.sin(1.3 * CENTRES))
    new_log_z, new_mean = bridge_reference([(slots[0][0], slots[0][1], slots[0][2] * factor)] + slots[1:])
    calls = []
    real = ops.ais_ment_steps
    try:
        ops.ais_ment_steps = lambda *a, **k: calls.append(a[6].cpu().tolist()) or real(*a, **k)
        x = model.sample(65536)
    finally:
        ops.ais_ment_steps = real
    assert all(b == [1.0, 1.0] for b in calls) and len(calls) == 1 + 32, "a bridge call never walks the ladder"
    d_mean = (x.double().mean(0).cpu() - new_mean).abs()
    print(f"bridge: log Z {float(s.log_z):.5f} (quadrature {new_log_z:.5f}, before the change {old_log_z:.5f}), |d mean| per axis "
          f"{[round(float(v), 4) for v in d_mean]}, islands resampled {float(s.last['resampled']):.0f}, ess / S "
          f"{[round(float(v) / 256, 3) for v in s.last['ess_groups']]}")
    assert abs(float(s.log_z) - new_log_z) <= 0.14
    assert abs(new_log_z - old_log_z) > 0.14, "the change moves log Z by more than the gate"
    assert float(d_mean.max()) <= 0.11
    assert x.shape == (65536, 6) and bool((model.prob(x) > 0).all())


def test_sampler_serves_a_ment(backend):
    model, _ = build("a", backend)
    make = lambda: SequentialMonteCarloSampler(2, seed=2, **dict(SETTINGS, chains=1024, n_temps=16)).to(backend)
    model.sampler, model.mode, model.n_samples = make(), "sample", 3000
    s = model.sampler
    first = model.sample(700)
    assert first.shape == (700, 2) and first.dtype == torch.float32 and first.device.type == backend.type
    assert s.population is not None and s.population["x"].shape == (1024, 2) and 0.6 < float(s.acceptance) <= 1.0
    x = model.sample(3000)                                    # more points than chains, from the kept population
    assert x.shape == (3000, 2) and bool((model.prob(x) > 0).all())
    assert torch.unique(x, dim=0).shape[0] > 1024
    model.gauss_seidel_update(lr=0.9)
    assert model.epoch == 1 and all(torch.isfinite(lf.values).all() for lf in mf.utils.unravel(model.lagrange_functions))
    assert math.isfinite(float(s.log_z))
    # reset(): the next call is a full ladder, and a fixed seed gives the first call's bits; so does a new sampler
    model2, _ = build("a", backend)
    for sampler in (s, make()):
        sampler.reset()
        assert sampler.population is None
        assert torch.equal(sampler(model2.prob, 700), first)
    assert torch.equal(s(model2.prob, 500), make()(model2.prob, 500)) is False, "a kept population goes on, it does not restart"
    # persistent=False walks the ladder at every call
    fresh = SequentialMonteCarloSampler(2, seed=2, persistent=False, **dict(SETTINGS, chains=1024, n_temps=16)).to(backend)
    assert torch.equal(fresh(model2.prob, 700), first) and torch.equal(fresh(model2.prob, 700), first)
    assert s.to(backend) is s
    with pytest.raises(NotImplementedError, match="MENT.prob"):
        s(model2.log_prob, 10)


def test_pre_transform_chains_are_refused(backend):
    kick = mf.simulate.CompositeTransform(mf.simulate.MultipoleTransform(order=3, strength=0.5),
                                          mf.simulate.LinearTransform(torch.eye(2)))
    transforms = [mf.simulate.LinearTransform(torch.eye(2)).to(backend), kick.to(backend)]
    diagnostics = [[mf.diagnostics.Histogram1D(axis=0, edges=EDGES.clone()).to(backend)] for _ in transforms]
    meas = [[torch.ones(16).to(backend)] for _ in transforms]
    sampler = SequentialMonteCarloSampler(2, chains=64, n_temps=2).to(backend)
    model = MENT(ndim=2, transforms=transforms, diagnostics=diagnostics, measurements=meas,
                 prior=mf.prior.Gaussian(ndim=2, scale=3.0), sampler=sampler, mode="sample", device=backend)
    assert not model.fully_fused()
    with pytest.raises(NotImplementedError, match="pre-transform"):
        model.sample(10)
    with pytest.raises(NotImplementedError, match="pre-transform"):
        sampler.run(model)
    with pytest.raises(NotImplementedError, match="pre-transform"):
        model.log_normalization(sampler)


def test_constructor_validation():
    with pytest.raises(ValueError, match="ndim"):
        SequentialMonteCarloSampler(9)
    with pytest.raises(ValueError, match="step"):
        SequentialMonteCarloSampler(2, step=0.0)
    with pytest.raises(ValueError, match="betas"):
        SequentialMonteCarloSampler(2, betas=[0.1, 1.0])
    for groups in (0, -1, 3):
        with pytest.raises(ValueError, match="groups"):
            SequentialMonteCarloSampler(2, chains=64, groups=groups)
    for bad in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="ess_threshold"):
            SequentialMonteCarloSampler(2, ess_threshold=bad)
    for kws in (dict(resample_every=0), dict(bridge_steps=-1), dict(thin=0)):
        with pytest.raises(ValueError, match="resample_every"):
            SequentialMonteCarloSampler(2, **kws)
    s = SequentialMonteCarloSampler(3)
    assert (s.groups, s.ess_threshold, s.resample_every, s.persistent, s.bridge_steps, s.thin) == (8, 0.5, 1, True, 4, 2)
    assert (s.chains, s.n_temps, s.steps_per_temp) == (4096, 64, 2) and s.population is None and s.log_z is None
