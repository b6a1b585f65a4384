"""Classical MENT at C4's scale on the MI355X: the 6-D measurement set of 100 one-D projections x 64 bins, GridSampler at
res 33 (1.29e9 cells: beyond the reference, whose points alone would take 31 GB and whose torch.multinomial refuses more than
2^24 categories), one sample-mode Gauss-Seidel sub-step with 1 M samples.  The time is printed, not gated."""
import time

import pytest
import torch


@pytest.mark.gpu
def test_c4_sample_substep():
    import mentflow_amd as mf
    from mentflow_amd import _lib, ops
    from mentflow_amd.harness import build_problem
    from mentflow_amd.ment import MENT
    from mentflow_amd.sample import GridSampler
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    prob = build_problem(ndim=6, num=100, bins=64, xmax=3.5, seed=2, prior_scale=3.0, device=dev, dist_name="gaussian_mixture",
                         meas_samples=200000)
    res = 33
    model = MENT(ndim=6, transforms=prob.transforms, diagnostics=prob.diagnostics, measurements=prob.measurements,
                 prior=mf.prior.Gaussian(ndim=6, scale=3.0), mode="sample",
                 sampler=GridSampler(limits=6 * [(-3.5, 3.5)], shape=6 * [res]).to(dev), n_samples=1_000_000, device=dev)
    assert model.fully_fused()
    torch.manual_seed(0)
    pred = model.simulate(0, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.manual_seed(1)
    pred = model.simulate(0, 0)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"C4 6-D res {res}: one sample-mode simulate (grid prob + 1 M draws + KDE) {dt * 1e3:.1f} ms")
    assert torch.isfinite(pred).all()
    assert abs(float(pred.sum() * (prob.diagnostics[0][0].edges[1] - prob.diagnostics[0][0].edges[0])) - 1.0) < 1e-4
    torch.manual_seed(1)
    again = model.simulate(0, 0)
    assert torch.equal(pred, again)
    # the drawn cells follow K2's prob: marginal along axis 0 of the grid vs the histogram of 1 M draws
    coords = [c.to(dev) for c in model.sampler.coords]
    p, sums = model.prob_on_grid(coords)
    assert torch.isfinite(p).all() and p.numel() == res ** 6
    w = (p.double() + 1e-15).view(res, -1).sum(1)
    w = w / w.sum()
    torch.manual_seed(5)
    x = model.sample(1_000_000)
    e = model.sampler.edges[0]
    idx = torch.clamp(((x[:, 0] - e[0]) / (e[1] - e[0])).floor().long(), 0, res - 1)
    freq = torch.bincount(idx, minlength=res).double() / x.shape[0]
    sigma = torch.sqrt(w * (1 - w) / x.shape[0])
    assert bool(((freq - w).abs() <= 6 * sigma + 1e-9).all())
