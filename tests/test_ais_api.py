"""MENT.log_normalization and sample.AnnealedImportanceSampler through the public interface, against fp64 quadrature of
tests/_ment_logp_fp64.logp64 (the fp64 restatement of the density, never the code under test).  Emulator here, the MI355X with
-m gpu.

Two densities, both with 16-bin 1-D views on [-4, 4] (centres -3.75 .. 3.75), tables exp(-u^2 / 2) U[0.5, 1.5] at the centres and
the Gaussian prior of scale 3:
  (a) 2-D, four views at 0, 45, 90 and 135 degrees: Z and H by the 2049^2 trapezoid rule on [-3.75, 3.75]^2, which holds the
      support (the hulls of the 0 and 90 degree views);
  (b) 6-D, one view on each coordinate axis: the density factorises, so log Z and H are sums of six 1-D trapezoid rules
      (65 537 nodes on the hull).
With Z = integral of p and p = exp(logp64): H = log Z - (integral of p log p) / Z.

Settings (both cases): base N(0, 1.5^2), step 0.5, drift_clip 1, 2 048 chains, 32 temperatures, 2 transitions per temperature.
An fp64 prototype of the rule gave, over three seeds, |d log Z| <= 0.016 / 0.009, log_z_se ~ 0.0125 / 0.015, ess / C = 0.75 / 0.68
and |d H| <= 0.034 / 0.083 for (a) / (b), with acceptance 0.83 .. 0.88.  Gates:
  |d log Z| <= 4 log_z_se + 2e-3     (four standard errors of the estimate itself, plus the quadrature's and fp32's share)
  ess / C   >= 0.5                   (keeps a broken sampler from hiding behind a large standard error)
  |d H|     <= 0.15                  (about twice the worst prototype value: Monte-Carlo noise at this size)
  accept    >= 0.6."""
import functools
import math

import pytest
import torch

import mentflow_amd as mf
from _ment_logp_fp64 import logp64
from mentflow_amd.ment import MENT
from mentflow_amd.sample import AnnealedImportanceSampler

EDGES = torch.linspace(-4.0, 4.0, 17)
CENTRES = 0.5 * (EDGES[:-1] + EDGES[1:])
SETTINGS = dict(chains=2048, n_temps=32, steps_per_temp=2, step=0.5, drift_clip=1.0, base_scale=1.5)


def tables(n, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.exp(-0.5 * CENTRES ** 2) * (0.5 + torch.rand(16, generator=gen)) for _ in range(n)]


def rows_of(case):
    if case == "a":
        return [torch.tensor([math.cos(math.radians(t)), math.sin(math.radians(t))], dtype=torch.float32) for t in (0, 45, 90, 135)]
    return [torch.eye(6)[k] for k in range(6)]


def build(case, device):
    """The MENT of case (a) or (b): one LinearTransform per view whose first row is the view's direction."""
    rows = rows_of(case)
    d = rows[0].numel()
    vals = tables(len(rows), 17 if case == "a" else 23)
    transforms = []
    for r in rows:
        m = torch.eye(d)
        if case == "a":
            m = torch.stack([r, torch.stack([-r[1], r[0]])])
        else:
            k = int(r.argmax())
            m[[0, k]] = m[[k, 0]]                       # a permutation: row 0 reads axis k
        transforms.append(mf.simulate.LinearTransform(m).to(device))
    diagnostics = [[mf.diagnostics.Histogram1D(axis=0, edges=EDGES.clone()).to(device)] for _ in rows]
    meas = [[torch.ones(16).to(device)] for _ in rows]
    model = MENT(ndim=d, transforms=transforms, diagnostics=diagnostics, measurements=meas,
                 prior=mf.prior.Gaussian(ndim=d, scale=3.0), device=device)
    for i, v in enumerate(vals):
        model.lagrange_functions[i][0].set_values(v.to(device))
    assert model.fully_fused()
    slots = [([r], [CENTRES], v) for r, v in zip(rows, vals)]
    return model, slots


def _trapezoid_weights(n, h):
    w = torch.full((n,), h, dtype=torch.float64)
    w[0] = w[-1] = 0.5 * h
    return w


@functools.lru_cache(maxsize=None)
def reference(case):
    """(log Z, H) by fp64 quadrature of logp64: module docstring.  Computed once per case and shared."""
    _, slots = build(case, torch.device("cpu"))
    lo, hi = float(CENTRES[0]), float(CENTRES[-1])
    if case == "a":
        n = 2049
        t = torch.linspace(lo, hi, n, dtype=torch.float64)
        w = _trapezoid_weights(n, (hi - lo) / (n - 1))
        z = plp = 0.0
        for i0 in range(0, n, 128):                       # rows of the grid in chunks
            xs = t[i0:i0 + 128]
            pts = torch.stack(torch.meshgrid(xs, t, indexing="ij"), -1).reshape(-1, 2)
            lp = logp64(pts, slots, ("gaussian", 3.0))[0]
            ww = (w[i0:i0 + 128, None] * w[None, :]).reshape(-1)
            p = torch.exp(lp)
            z += float((ww * p).sum())
            plp += float((ww * torch.where(p > 0, p * lp, torch.zeros_like(p))).sum())
        return math.log(z), math.log(z) - plp / z
    n = 65537
    t = torch.linspace(lo, hi, n, dtype=torch.float64)[:, None]
    w = _trapezoid_weights(n, (hi - lo) / (n - 1))
    log_z = h = 0.0
    for rows, coords, values in slots:                    # the factor of one axis: its view times the 1-D prior
        lp = logp64(t, [([torch.ones(1)], coords, values)], ("gaussian", 3.0))[0]
        p = torch.exp(lp)
        z = float((w * p).sum())
        log_z += math.log(z)
        h += math.log(z) - float((w * torch.where(p > 0, p * lp, torch.zeros_like(p))).sum()) / z
    return log_z, h


@pytest.mark.parametrize("case", ["a", "b"])
def test_log_z_and_entropy_against_quadrature(backend, case):
    """Measured (seed 5), |d log Z| / log_z_se / ess / C / |d H| / accept: see DESIGN.md 6i."""
    model, _ = build(case, backend)
    ref_log_z, ref_h = reference(case)
    res = model.log_normalization(seed=5, **SETTINGS)
    assert all(v.dim() == 0 and v.dtype == torch.float64 and v.device.type == backend.type for v in res.values())
    log_z, se, ess, h, rate = (float(res[k]) for k in ("log_z", "log_z_se", "ess", "entropy", "accept_rate"))
    print(f"case {case}: log Z {log_z:.5f} (quadrature {ref_log_z:.5f}, |d| {abs(log_z - ref_log_z):.5f}), log_z_se {se:.5f}, "
          f"ess / C {ess / SETTINGS['chains']:.4f}, H {h:.5f} (quadrature {ref_h:.5f}, |d| {abs(h - ref_h):.5f}), "
          f"accept {rate:.4f}")
    assert abs(log_z - ref_log_z) <= 4 * se + 2e-3
    assert ess / SETTINGS["chains"] >= 0.5
    assert abs(h - ref_h) <= 0.15
    assert rate >= 0.6
    assert model.log_z is res["log_z"]


def test_normalized_log_density(backend):
    model, _ = build("a", backend)
    x = torch.randn(64, 2, generator=torch.Generator().manual_seed(0)).to(backend)
    with pytest.raises(RuntimeError, match="log_normalization"):
        model.log_density(x, normalized=True)
    plain = model.log_density(x)
    res = model.log_normalization(seed=1, **dict(SETTINGS, chains=512, n_temps=8))
    assert torch.equal(model.log_density(x), plain), "the default path is untouched by an estimate"
    assert torch.equal(model.log_density(x, normalized=True), plain - res["log_z"])
    assert model.log_density(x, normalized=True).dtype == torch.float32
    # a sampler of one's own in place of the arguments; both at once is refused
    own = AnnealedImportanceSampler(2, seed=1, **dict(SETTINGS, chains=512, n_temps=8))
    assert torch.equal(model.log_normalization(own)["log_z"], res["log_z"])
    with pytest.raises(TypeError, match="either"):
        model.log_normalization(own, chains=16)


def test_fixed_seed_is_bitwise_reproducible(backend):
    model, _ = build("b", backend)
    kws = dict(SETTINGS, chains=300, n_temps=5)
    a = model.log_normalization(seed=3, **kws)
    b = model.log_normalization(seed=3, **kws)
    c = model.log_normalization(seed=4, **kws)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert not torch.equal(a["log_z"], c["log_z"])
    s = AnnealedImportanceSampler(6, seed=3, **kws).to(backend)
    r1, r2 = s.run(model), s.run(model)
    assert all(torch.equal(r1[k], r2[k]) for k in ("x", "logw", "logp", "accepted"))
    assert r1["logw"].dtype == torch.float64 and r1["x"].shape == (300, 6)
    # the launches are cut by a byte budget; the cut changes no bit
    import mentflow_amd.sample as sample
    budget = sample._AIS_NOISE_BYTES
    try:
        sample._AIS_NOISE_BYTES = 4 * 7 * 300 * 2 * 2          # two temperatures per launch: 2 + 2 + 1
        r3 = s.run(model)
    finally:
        sample._AIS_NOISE_BYTES = budget
    assert all(torch.equal(r1[k], r3[k]) for k in ("x", "logw", "logp", "accepted"))


def test_resampling_sampler_serves_a_ment(backend):
    model, _ = build("a", backend)
    model.sampler = AnnealedImportanceSampler(2, seed=2, **dict(SETTINGS, chains=1024, n_temps=16)).to(backend)
    for size in (700, 3000):                              # fewer and more points than chains
        x = model.sample(size)
        assert x.shape == (size, 2) and x.dtype == torch.float32 and x.device.type == backend.type
        assert bool((model.prob(x) > 0).all()), "a resampled point has weight > 0, so it lies inside the support"
    assert 0.6 < float(model.sampler.acceptance) <= 1.0
    # the resampled cloud has the moments of the weighted chains
    res = model.sampler.last
    w = torch.exp(res["logw"] - torch.logsumexp(res["logw"], 0))
    mean = (w[:, None] * res["x"].double()).sum(0)
    assert float((x.double().mean(0) - mean).abs().max()) < 0.05
    with pytest.raises(NotImplementedError, match="MENT.prob"):
        model.sampler(model.log_prob, 10)


def test_constructor_and_ladder_validation():
    with pytest.raises(ValueError, match="ndim"):
        AnnealedImportanceSampler(9)
    with pytest.raises(ValueError, match="step"):
        AnnealedImportanceSampler(2, step=0.0)
    with pytest.raises(ValueError, match="drift_clip"):
        AnnealedImportanceSampler(2, drift_clip=-1.0)
    with pytest.raises(ValueError, match="base_scale"):
        AnnealedImportanceSampler(2, base_scale=[1.0, 0.0])
    with pytest.raises(ValueError, match="n_temps"):
        AnnealedImportanceSampler(2, n_temps=0)
    for bad in ([0.1, 1.0], [0.0, 0.9], [0.0, 0.6, 0.5, 1.0], [1.0]):
        with pytest.raises(ValueError, match="betas"):
            AnnealedImportanceSampler(2, betas=bad)
    s = AnnealedImportanceSampler(3, betas=[0.0, 0.0, 0.5, 1.0, 1.0])
    assert s.n_temps == 4 and s.drift_clip == mf.sample.LangevinSampler(3).drift_clip and s.steps_per_temp == 2
    assert torch.equal(AnnealedImportanceSampler(2, n_temps=4).betas, torch.linspace(0.0, 1.0, 5))


def test_pre_transform_chains_are_refused(backend):
    kick = mf.simulate.CompositeTransform(mf.simulate.MultipoleTransform(order=3, strength=0.5),
                                          mf.simulate.LinearTransform(torch.eye(2)))
    transforms = [mf.simulate.LinearTransform(torch.eye(2)).to(backend), kick.to(backend)]
    diagnostics = [[mf.diagnostics.Histogram1D(axis=0, edges=EDGES.clone()).to(backend)] for _ in transforms]
    meas = [[torch.ones(16).to(backend)] for _ in transforms]
    model = MENT(ndim=2, transforms=transforms, diagnostics=diagnostics, measurements=meas,
                 prior=mf.prior.Gaussian(ndim=2, scale=3.0), device=backend)
    assert not model.fully_fused()
    with pytest.raises(NotImplementedError, match="pre-transform"):
        model.log_normalization(chains=64, n_temps=2)
    with pytest.raises(NotImplementedError, match="pre-transform"):
        AnnealedImportanceSampler(2, chains=64, n_temps=2).to(backend).run(model)
    assert model.log_z is None
