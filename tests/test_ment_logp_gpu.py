"""The log-density of classical MENT on the MI355X only: the C4 shape (6-D, 100 slots x 64 bins) at 262 144 points against the
fp64 yardstick on a subsample, one graphed MENT-Flow step with a MENT prior, and a flow fitted to a MENT solution by reverse KL.

The reverse-KL fit.  Four views at angles k pi / 4 with the Lagrange functions exp(-u^2 / (2 0.8^2)) and a Gaussian prior of
scale 3 multiply to an isotropic Gaussian in closed form: sum_k (r_k . x)^2 = 2 |x|^2, so the precision is 2 / 0.64 + 1 / 9.  The
yardstick is the same training loop (same seed, same base draws) against that closed form in plain torch; the kernel-trained
run's final reverse-KL estimate (mean of the last 20 steps, plus the analytic log Z) may exceed the yardstick run's by at most
50 % + 0.01 nats, which covers seed-to-seed spread and the interpolation error of the tables (64 centres on [-4, 4])."""
import math

import pytest
import torch

from _ment_logp_fp64 import check_gates, logp64
from test_ment_logp_kernels import make_slots

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev():
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    return torch.device("cuda", 0)


def test_c4_shape_against_fp64_on_a_subsample(dev):
    from mentflow_amd import ops
    d, n, sub = 6, 262144, 4096
    gen = torch.Generator().manual_seed(64)
    slots, desc, meta, tab = make_slots(d, [(1, 64)] * 100, gen)
    x = 1.2 * torch.randn(n, d, generator=gen)
    s = 1.7
    prior = (1, s, -d * (math.log(s) + 0.5 * math.log(2 * math.pi)))
    lp, g = ops.ment_logprob(x.to(dev), desc.to(dev), meta.to(dev), tab.to(dev), prior, want_grad=True)
    lp2, g2 = ops.ment_logprob(x.to(dev), desc.to(dev), meta.to(dev), tab.to(dev), prior, want_grad=True)
    assert torch.equal(lp, lp2) and torch.equal(g, g2)
    idx = torch.randperm(n, generator=gen)[:sub]
    ref, gref, amb = logp64(x[idx], slots, ("gaussian", s))
    check_gates(lp.cpu()[idx], g.cpu()[idx], ref, gref, amb, cap=0.04)


def test_graphed_step_with_a_ment_prior_replays_bitwise(dev):
    import mentflow_amd as mf
    from test_ment_prior import flow_problem
    model = flow_problem(dev).model
    n = 4096
    model.generator.inject_z = (1.5 * torch.randn(n, 2, generator=torch.Generator().manual_seed(8))).to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.0, capturable=True)
    L0 = model.loss(n)[0].detach().clone()
    step = mf.graph.GraphedTrainStep(model, opt, n, warmup=3, guard=True)
    step.step()
    first = step.scalars().clone()
    step.undo_last_step()
    step.step()
    second = step.scalars().clone()
    assert torch.isfinite(first).all() and torch.equal(first, second)
    assert torch.equal(first[0], L0), "the captured step computes what the eager one does"


def test_flow_fitted_to_a_ment_solution_by_reverse_kl(dev):
    import mentflow_amd as mf
    from mentflow_amd.ment import MENT
    sigma_h, scale, B = 0.8, 3.0, 64
    h = 8.0 / (B - 1)
    edges = torch.linspace(-4.0 - 0.5 * h, 4.0 + 0.5 * h, B + 1)               # centres: 64 points on [-4, 4]
    diag = mf.diagnostics.Histogram1D(axis=0, edges=edges).to(dev)
    angles = [math.pi * k / 4 for k in range(4)]
    transforms = [mf.simulate.LinearTransform(mf.simulate.rotation_matrix(a).float()).to(dev) for a in angles]
    ment = MENT(ndim=2, transforms=transforms, diagnostics=[[diag] for _ in transforms],
                measurements=[[torch.ones(B).to(dev)] for _ in transforms], prior=mf.prior.Gaussian(ndim=2, scale=scale),
                mode="sample", device=dev)
    c = mf.utils.coords_from_edges(edges)
    for lf in mf.utils.unravel(ment.lagrange_functions):
        lf.set_values(torch.exp(-c ** 2 / (2 * sigma_h ** 2)).to(dev))
    assert ment.fully_fused()
    lam = 2.0 / sigma_h ** 2 + 1.0 / scale ** 2
    log_norm = ment.prior.log_norm()
    log_z = log_norm + math.log(2 * math.pi / lam)

    def closed_form(x):
        return log_norm - 0.5 * lam * x.square().sum(1)

    def fit(log_density):
        torch.manual_seed(0)
        gen = mf.generate.build_generator("nsf", input_features=2, output_features=2, hidden_layers=3, hidden_units=64,
                                          transforms=2, bins=20, device=dev)
        opt = torch.optim.Adam(gen.parameters(), lr=1e-3)
        losses = []
        for _ in range(300):
            opt.zero_grad(set_to_none=False)
            x, logq = gen.sample_and_log_prob(8192)
            loss = (logq - log_density(x)).mean()
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        return float(torch.stack(losses[-20:]).mean()) + log_z, float(losses[0]) + log_z

    kl_kernel, first_kernel = fit(lambda x: ment.log_density(x, pad=1e-12))
    kl_closed, first_closed = fit(closed_form)
    print(f"reverse KL after 300 steps: kernel-trained {kl_kernel:.5f} nats, closed-form-trained {kl_closed:.5f} nats "
          f"(first step {first_kernel:.4f} / {first_closed:.4f})")
    assert math.isfinite(kl_kernel) and kl_kernel < 0.5 * first_kernel, "the fit must have moved"
    assert kl_kernel <= 1.5 * kl_closed + 0.01
