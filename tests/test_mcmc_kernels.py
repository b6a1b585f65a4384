"""The Metropolis-Hastings kernel (mentflow_amd/csrc/mcmc.hip, ops.mcmc_ment_steps) against the fp64 transition verifier of
tests/_mcmc_fp64.py, on the emulator here and on the MI355X with -m gpu (the `backend` fixture).

Every transition of the full trajectory is classified in fp64 from the kernel's own previous state; none may disagree outside
the band m = 1e-3 (see _mcmc_fp64) and at most 0.5 % may be ambiguous.  The stationarity test needs no band: started exactly
from the target N(0, s^2 I), the states after any number of correct transitions are exact independent draws from it, so the
per-axis mean lies within 5 s / sqrt(C) and the per-axis variance within 5 s^2 sqrt(2 / (C - 1)) (five standard errors)."""
import math

import pytest
import torch

from _mcmc_fp64 import assert_transitions, verify
from _ment_fp64 import prob64
from mentflow_amd import ops
from test_ment_kernels import make_slots

CHAINS, STEPS = 512, 40
# (d, slot specs, proposal step): the shapes whose ambiguous share was measured on the CPU at 0.015 .. 0.054 % of 20 480
SHAPES = {
    "4d_mixed": (4, [(1 if k % 2 == 0 else 2, 9 + k) for k in range(8)], 0.4),
    "6d_24x12": (6, [(1, 12)] * 24, 0.25),
    "2d_5x16": (2, [(1, 16)] * 5, 0.5),
}


def gaussian_prior(d, s=1.7):
    return (1, s, -d * (math.log(s) + 0.5 * math.log(2 * math.pi))), ("gaussian", s)


def make_noise(steps, d, chains, gen):
    nz = torch.randn(steps, d + 1, chains, generator=gen)
    nz[:, d] = torch.rand(steps, chains, generator=gen)
    return nz


def run_kernel(dev, start, noise, step, desc, meta, tab, prior, step_offset=0, keep_from=0, keep_every=1, n_keep=None,
               accepted=None):
    """(kept states, final states, accepted) of one ops.mcmc_ment_steps call."""
    steps, dp1, chains = noise.shape
    d = dp1 - 1
    x = start.clone().to(dev).contiguous()
    if n_keep is None:
        n_keep = 0 if step_offset + steps <= keep_from else (step_offset + steps - 1 - keep_from) // keep_every + 1
    out = torch.full((n_keep, chains, d), float("nan"), device=dev) if n_keep else None
    acc = torch.zeros(chains, dtype=torch.int32, device=dev) if accepted is None else accepted
    scale = torch.full((d,), float(step), device=dev) if not torch.is_tensor(step) else step.to(dev)
    ops.mcmc_ment_steps(x, desc.to(dev), meta.to(dev), tab.to(dev), prior, noise.to(dev).contiguous(), scale, acc,
                        step_offset=step_offset, keep_from=keep_from, keep_every=keep_every, out=out)
    return out, x, acc


def problem(name, with_prior=True, seed=0):
    d, specs, step = SHAPES[name]
    gen = torch.Generator().manual_seed(1000 + seed + 7 * d)
    slots, desc, meta, tab = make_slots(d, specs, gen)
    prior, prior64 = gaussian_prior(d) if with_prior else ((0, 0.0, 0.0), None)
    start = torch.randn(CHAINS, d, generator=gen)
    noise = make_noise(STEPS, d, CHAINS, gen)
    return d, step, slots, desc, meta, tab, prior, prior64, start, noise


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("with_prior", [True, False])
def test_transitions_verified(backend, name, with_prior):
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem(name, with_prior)
    traj, final, acc = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    stats = verify(start, noise, traj, step, slots, prior64)
    print(name, with_prior, stats)
    assert_transitions(stats)
    assert stats["accepted"] > 0.02 * stats["total"], "the chains must move"
    assert torch.equal(final.cpu(), traj[-1].cpu())
    # the acceptance counters are the changed states along each chain's trajectory
    prev = torch.cat([start[None], traj.cpu()[:-1]])
    changed = (traj.cpu() != prev).any(2).sum(0).to(torch.int32)
    assert torch.equal(acc.cpu(), changed)


def test_transitions_tables_beyond_lds(backend):
    """6 x 85^2 2-D tables (43 350 floats): read from global memory, as in test_ment_kernels.py."""
    d, step = 4, 0.4
    gen = torch.Generator().manual_seed(7)
    slots, desc, meta, tab = make_slots(d, [(2, 85)] * 6, gen, zeros=False)
    prior, prior64 = gaussian_prior(d)
    start = torch.randn(256, d, generator=gen)
    noise = make_noise(STEPS, d, 256, gen)
    traj, _, _ = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    stats = verify(start, noise, traj, step, slots, prior64)
    print(stats)
    assert_transitions(stats)
    assert stats["accepted"] > 0.02 * stats["total"]


def test_chains_started_outside_the_support_walk_in_and_stay(backend):
    """Half of the chains start far outside every hull (prob == 0): they random-walk (every finite proposal to another
    zero-density point is accepted) and, once a state has prob > 0, every later state of that chain has prob > 0."""
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("2d_5x16", seed=3)
    start[::2] = start[::2] * 0.3 + torch.tensor([3.4, 0.0])          # just outside the first slot's hull (|x0| <= ~2.8)
    traj, _, acc = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    stats = verify(start, noise, traj, step, slots, prior64)
    print(stats)
    assert_transitions(stats)
    T, C = traj.shape[:2]
    dev_args = [t.to(backend) for t in (desc, meta, tab)]
    p = ops.ment_prob(traj.reshape(T * C, d).contiguous(), *dev_args, prior).reshape(T, C).cpu()
    p0 = ops.ment_prob(start.to(backend).contiguous(), *dev_args, prior).cpu()
    assert int((p0 == 0).sum()) >= C // 4, "the test needs chains that start outside"
    inside = torch.cat([p0[None], p]) > 0
    ever = torch.cummax(inside.to(torch.int8), 0)[0].bool()
    assert torch.equal(inside, ever), "a chain left the support (by the bits mf_ment_prob returns)"
    entered = ~inside[0] & inside[-1]
    assert int(entered.sum()) > 0, "no outside chain found the support"


def test_nan_noise_is_rejected_and_does_not_spread(backend):
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("4d_mixed", seed=5)
    start[:] = start * 0.3
    noise[7, 1, 11] = float("nan")            # a NaN proposal coordinate of chain 11 at step 7
    noise[9, d, 12] = float("nan")            # a NaN uniform of chain 12 at step 9
    noise[3, :, 13] = float("nan")            # a whole NaN row
    traj, final, _ = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    traj = traj.cpu()
    assert torch.isfinite(traj).all() and torch.isfinite(final).all()
    assert torch.equal(traj[7, 11], traj[6, 11]) and torch.equal(traj[9, 12], traj[8, 12]) and torch.equal(traj[3, 13], traj[2, 13])
    stats = verify(start, noise, traj, step, slots, prior64)
    assert_transitions(stats)
    # the other chains are what they are without the NaNs
    clean = noise.clone()
    clean[7, 1, 11] = clean[9, d, 12] = 0.5
    clean[3, :, 13] = 0.5
    ref, _, _ = run_kernel(backend, start, clean, step, desc, meta, tab, prior)
    others = [c for c in range(CHAINS) if c not in (11, 12, 13)]
    assert torch.equal(traj[:, others], ref.cpu()[:, others])


def test_chunk_invariance_rerun_and_keep_selection(backend):
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("6d_24x12", seed=2)
    full, final, acc = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    again, final2, acc2 = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    assert torch.equal(full, again) and torch.equal(final, final2) and torch.equal(acc, acc2)
    # 4 launches of 10 steps, step_offset advanced, into one output buffer
    x = start.clone().to(backend)
    out = torch.full((STEPS, CHAINS, d), float("nan"), device=backend)
    acc4 = torch.zeros(CHAINS, dtype=torch.int32, device=backend)
    scale = torch.full((d,), step, device=backend)
    dev_args = [t.to(backend) for t in (desc, meta, tab)]
    for t0 in range(0, STEPS, 10):
        ops.mcmc_ment_steps(x, *dev_args, prior, noise[t0:t0 + 10].to(backend).contiguous(), scale, acc4, step_offset=t0, out=out)
    assert torch.equal(out, full) and torch.equal(x, final) and torch.equal(acc4, acc)
    # keep_from / keep_every pick rows of the full trajectory, in one launch and across launches
    for keep_from, keep_every in ((0, 1), (3, 1), (5, 7), (9, 10), (39, 3), (0, 40)):
        rows = list(range(keep_from, STEPS, keep_every))
        kept, fin, _ = run_kernel(backend, start, noise, step, desc, meta, tab, prior, keep_from=keep_from, keep_every=keep_every)
        assert kept.shape[0] == len(rows) and torch.equal(kept, full[rows]) and torch.equal(fin, final)
        x = start.clone().to(backend)
        out = torch.full((len(rows), CHAINS, d), float("nan"), device=backend)
        for t0, t1 in ((0, 13), (13, 14), (14, 40)):
            ops.mcmc_ment_steps(x, *dev_args, prior, noise[t0:t1].to(backend).contiguous(), scale, acc4, step_offset=t0,
                                keep_from=keep_from, keep_every=keep_every, out=out)
        assert torch.equal(out, full[rows])
    # nothing kept: out may be None, and a keep_from beyond the run writes nothing
    x = start.clone().to(backend)
    ops.mcmc_ment_steps(x, *dev_args, prior, noise.to(backend), scale, acc4)
    assert torch.equal(x, final)
    none, fin, _ = run_kernel(backend, start, noise, step, desc, meta, tab, prior, keep_from=STEPS, keep_every=3, n_keep=2)
    assert torch.isnan(none).all() and torch.equal(fin, final)


def test_density_is_recomputed_at_entry(backend):
    """The tables change between two calls (a Gauss-Seidel update): the second call's transitions verify against the NEW
    density from the first step on, with no state but x carried over."""
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("2d_5x16", seed=4)
    _, mid, _ = run_kernel(backend, start, noise[:20], step, desc, meta, tab, prior)
    gen = torch.Generator().manual_seed(99)
    tab2 = tab * (0.5 + torch.rand(tab.shape, generator=gen))
    slots2, off = [], 0
    for rows, coords, values in slots:
        slots2.append((rows, coords, tab2[off:off + values.numel()].reshape(values.shape)))
        off += values.numel()
    traj, _, _ = run_kernel(backend, mid.cpu(), noise[20:], step, desc, meta, tab2, prior)
    assert_transitions(verify(mid.cpu(), noise[20:], traj, step, slots2, prior64))


def test_stationarity_and_acceptance_rate(backend):
    """No slots, Gaussian prior of scale s in d = 3: 8192 chains started from exact draws of N(0, s^2 I), 20 steps with the
    proposal scale 2.4 s / sqrt(d).  Mean and variance bounds: module docstring.  The acceptance rate must match an fp64 run of
    the same noise within 0.01, so a kernel that never moves (trivially stationary) fails."""
    d, C, T, s = 3, 8192, 20, 1.3
    gen = torch.Generator().manual_seed(21)
    start = s * torch.randn(C, d, generator=gen)
    noise = make_noise(T, d, C, gen)
    step = 2.4 * s / math.sqrt(d)
    prior, _ = gaussian_prior(d, s)
    desc, meta, tab = torch.zeros(0, 24), torch.zeros(0, 4, dtype=torch.int32), torch.zeros(1)
    _, final, acc = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    final = final.cpu().double()
    assert float(final.mean(0).abs().max()) <= 5 * s / math.sqrt(C), final.mean(0)
    assert float((final.var(0) - s * s).abs().max()) <= 5 * s * s * math.sqrt(2.0 / (C - 1)), final.var(0)
    # fp64 chain on the same noise
    x, n_acc = start.double(), 0
    logp = lambda v: -0.5 * (v * v).sum(1) / s ** 2
    for t in range(T):
        y = x + float(torch.tensor(step, dtype=torch.float32)) * noise[t, :d].T.double()
        a = torch.log(noise[t, d].double()) < logp(y) - logp(x)
        x = torch.where(a[:, None], y, x)
        n_acc += int(a.sum())
    rate = float(acc.sum()) / (C * T)
    print("acceptance", rate, "fp64", n_acc / (C * T))
    assert abs(rate - n_acc / (C * T)) <= 0.01
    assert 0.1 < rate < 0.6


def test_argument_checks(backend):
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("2d_5x16")
    dev = backend
    x = start.to(dev)
    acc = torch.zeros(CHAINS, dtype=torch.int32, device=dev)
    scale = torch.full((d,), step, device=dev)
    a = [t.to(dev) for t in (desc, meta, tab)]
    nz = noise.to(dev)
    with pytest.raises(RuntimeError, match="noise"):
        ops.mcmc_ment_steps(x, *a, prior, nz[:, :d], scale, acc)
    with pytest.raises(RuntimeError, match="float32"):
        ops.mcmc_ment_steps(x.double(), *a, prior, nz, scale, acc)
    with pytest.raises(RuntimeError, match="accepted"):
        ops.mcmc_ment_steps(x, *a, prior, nz, scale, acc.long())
    with pytest.raises(RuntimeError, match="scale"):
        ops.mcmc_ment_steps(x, *a, prior, nz, scale[:1], acc)
    with pytest.raises(RuntimeError, match="out"):
        ops.mcmc_ment_steps(x, *a, prior, nz, scale, acc, out=torch.empty(STEPS - 1, CHAINS, d, device=dev))
    with pytest.raises(RuntimeError, match="keep_every"):
        ops.mcmc_ment_steps(x, *a, prior, nz, scale, acc, keep_every=0)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.mcmc_ment_steps(x, *a, prior, nz.permute(0, 2, 1).contiguous().permute(0, 2, 1), scale, acc)
    assert torch.equal(x.cpu(), start), "a refused call must not touch the state"
