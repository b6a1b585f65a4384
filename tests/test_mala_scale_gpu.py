"""The Langevin kernel at C4's shape on the MI355X: 6-D, 100 one-D projections x 64 bins (9 200 floats: the tables-in-LDS instance),
65 536 chains, 20 steps.  Every state is finite, the acceptance rate lies strictly between 0 and 1, 4 096 transitions drawn at
random from the 1.3 M pass the fp64 verifier (tests/_mala_fp64.py: none wrong, none malformed, at most 4 % ambiguous), and the run
cut in two launches is bitwise the run in one.  The tables are uniform in [0.25, 2] (the condition of the verifier's band) under
the Gaussian prior of scale 1.7, the chains start at 0.5 randn, and the step is 0.1: below the tables' bin width of 0.125, since
a proposal is informed by the gradient only within a cell.  The time is printed, not gated."""
import time

import pytest
import torch

from _mala_fp64 import assert_transitions, verify
from test_mcmc_kernels import gaussian_prior, make_noise
from test_ment_logp_kernels import make_slots

CHAINS, STEPS, STEP = 65536, 20, 0.1


@pytest.mark.gpu
def test_c4_shape_transitions_and_split_run():
    from mentflow_amd import _lib, ops
    _lib.use_library(_lib.DEFAULT_PATH)
    dev = torch.device("cuda", 0)
    d = 6
    gen = torch.Generator().manual_seed(77)
    slots, desc, meta, tab = make_slots(d, [(1, 64)] * 100, gen)
    prior, prior64 = gaussian_prior(d)
    start = 0.5 * torch.randn(CHAINS, d, generator=gen)
    noise = make_noise(STEPS, d, CHAINS, gen).to(dev)
    args = [t.to(dev) for t in (desc, meta, tab)]
    scale = torch.full((d,), STEP, device=dev)

    def run(cuts):
        x = start.to(dev).contiguous()
        out = torch.full((STEPS, CHAINS, d), float("nan"), device=dev)
        acc = torch.zeros(CHAINS, dtype=torch.int32, device=dev)
        logp = torch.empty(CHAINS, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a, b in zip(cuts[:-1], cuts[1:]):
            ops.mala_ment_steps(x, *args, prior, noise[a:b], scale, acc, step_offset=a, out=out, logp=logp)
        torch.cuda.synchronize()
        return out, x, acc, logp, time.perf_counter() - t0

    traj, final, acc, logp, _ = run([0, STEPS])
    traj2, final2, acc2, logp2, ms = run([0, STEPS])
    rate = float(acc.sum()) / (CHAINS * STEPS)
    print(f"C4 shape, {CHAINS} chains x {STEPS} steps x 100 slots: {ms * 1e3:.2f} ms, acceptance {rate:.3f}")
    assert torch.isfinite(traj).all() and torch.isfinite(final).all() and torch.isfinite(logp).all()
    assert 0.0 < rate < 1.0
    assert torch.equal(traj, traj2) and torch.equal(final, final2) and torch.equal(acc, acc2) and torch.equal(logp, logp2)
    cut = run([0, 7, STEPS])
    assert torch.equal(traj, cut[0]) and torch.equal(final, cut[1]) and torch.equal(acc, cut[2]) and torch.equal(logp, cut[3])
    assert torch.equal(logp, ops.ment_logprob(final, *args, prior)[0])

    pick = torch.randperm(STEPS * CHAINS, generator=torch.Generator().manual_seed(5))[:4096]
    grad32 = lambda x: ops.ment_logprob(x.to(dev).contiguous(), *args, prior, want_grad=True)[1].cpu()
    stats = verify(start, noise, traj, STEP, 1.0, slots, prior64, grad32, pick=pick)
    print(stats)
    assert stats["total"] == 4096
    assert_transitions(stats)
    assert 0 < stats["accepted"] < stats["total"]
