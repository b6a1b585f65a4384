"""The Metropolis-adjusted Langevin kernel (mentflow_amd/csrc/mala.hip, ops.mala_ment_steps) against the fp64 transition verifier
of tests/_mala_fp64.py, on the emulator here and on the MI355X with -m gpu (the `backend` fixture).

Every transition of the full trajectory is classified in fp64 from the kernel's own previous state; none may disagree outside
the band of _mala_fp64 (derived there from the 3e-4 gate of the log-density tests) and at most 4 % may be ambiguous.  Band-verified
cases use tables uniform in [0.25, 2]: near a zero of a table log h amplifies fp32 rounding without bound, so the gate, and the
band with it, holds only away from zeros (the condition tests/test_ment_logp_kernels.py states).  Tables with zeros are tested
for the support conventions instead, by the bits mf_ment_logprob returns.  The stationarity test needs no band: started exactly
from the target N(0, s^2 I), the states after any number of correct transitions are exact independent draws from it, so the
per-axis mean lies within 5 s / sqrt(C) and the per-axis variance within 5 s^2 sqrt(2 / (C - 1)) (five standard errors, the
derivation of tests/test_mcmc_kernels.py)."""
import math

import pytest
import torch

from _mala_fp64 import assert_transitions, verify
from mentflow_amd import _lib, ops
from test_mcmc_kernels import CHAINS, SHAPES, STEPS, gaussian_prior, make_noise
from test_ment_kernels import make_slots
from test_ment_logp_kernels import make_slots as make_logp_slots

NO_PRIOR = ((0, 0.0, 0.0), None)


def run_kernel(dev, start, noise, step, desc, meta, tab, prior, drift_clip=1.0, step_offset=0, keep_from=0, keep_every=1,
               n_keep=None, want_logp=True):
    """(kept states, final states, accepted, logp of the final states) of one ops.mala_ment_steps call."""
    steps, dp1, chains = noise.shape
    d = dp1 - 1
    x = start.clone().to(dev).contiguous()
    if n_keep is None:
        n_keep = 0 if step_offset + steps <= keep_from else (step_offset + steps - 1 - keep_from) // keep_every + 1
    out = torch.full((n_keep, chains, d), float("nan"), device=dev) if n_keep else None
    acc = torch.zeros(chains, dtype=torch.int32, device=dev)
    logp = torch.full((chains,), float("nan"), device=dev) if want_logp else None
    scale = torch.full((d,), float(step), device=dev)
    ops.mala_ment_steps(x, desc.to(dev), meta.to(dev), tab.to(dev), prior, noise.to(dev).contiguous(), scale, acc,
                        drift_clip=drift_clip, step_offset=step_offset, keep_from=keep_from, keep_every=keep_every, out=out,
                        logp=logp)
    return out, x, acc, logp


def grad32(dev, desc, meta, tab, prior):
    """x -> the fp32 gradient of ops.ment_logprob on the backend: what the kernel's proposals are built from."""
    args = [t.to(dev) for t in (desc, meta, tab)]
    return lambda x: ops.ment_logprob(x.to(dev).contiguous(), *args, prior, want_grad=True)[1].cpu()


def logp32(dev, x, desc, meta, tab, prior):
    return ops.ment_logprob(x.to(dev).contiguous(), desc.to(dev), meta.to(dev), tab.to(dev), prior)[0]


def problem(name, with_prior=True, seed=0, zeros=False, chains=CHAINS):
    d, specs, step = SHAPES[name]
    gen = torch.Generator().manual_seed(2000 + seed + 7 * d)
    slots, desc, meta, tab = make_slots(d, specs, gen, zeros=zeros, lo=0.0 if zeros else 0.25)
    prior, prior64 = gaussian_prior(d) if with_prior else NO_PRIOR
    start = 0.5 * torch.randn(chains, d, generator=gen)
    noise = make_noise(STEPS, d, chains, gen)
    return d, step, slots, desc, meta, tab, prior, prior64, start, noise


def check_run(backend, start, noise, step, slots, desc, meta, tab, prior, prior64, drift_clip=1.0):
    traj, final, acc, logp = run_kernel(backend, start, noise, step, desc, meta, tab, prior, drift_clip)
    stats = verify(start, noise, traj, step, drift_clip, slots, prior64, grad32(backend, desc, meta, tab, prior))
    print(stats)
    assert_transitions(stats)
    assert stats["accepted"] > 0.02 * stats["total"], "the chains must move"
    assert torch.equal(final.cpu(), traj[-1].cpu())
    # the acceptance counters are the changed states along each chain's trajectory
    prev = torch.cat([start[None], traj.cpu()[:-1]])
    changed = (traj.cpu() != prev).any(2).sum(0).to(torch.int32)
    assert torch.equal(acc.cpu(), changed)
    # the log-density the chain carries is the one mf_ment_logprob returns for its state
    assert torch.equal(logp.view(torch.int32), logp32(backend, final, desc, meta, tab, prior).view(torch.int32))
    return stats


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("with_prior", [True, False])
def test_transitions_verified(backend, name, with_prior):
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem(name, with_prior)
    check_run(backend, start, noise, step, slots, desc, meta, tab, prior, prior64)


def test_transitions_verified_with_a_wider_clip(backend):
    """drift_clip = 2 at half the step: the drift is clamped on other axes and at other points than with the default."""
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("4d_mixed", seed=1)
    check_run(backend, start, noise, 0.5 * step, slots, desc, meta, tab, prior, prior64, drift_clip=2.0)


def test_driftless_walk(backend):
    """drift_clip = 0: y = x + s z and r = -z, a random walk under the same acceptance rule."""
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("2d_5x16", seed=6)
    check_run(backend, start, noise, step, slots, desc, meta, tab, prior, prior64, drift_clip=0.0)


def test_transitions_tables_beyond_lds(backend):
    """6 x 85^2 2-D tables (43 350 floats): read from global memory, as in test_ment_kernels.py."""
    d, step = 4, 0.4
    gen = torch.Generator().manual_seed(7)
    slots, desc, meta, tab = make_slots(d, [(2, 85)] * 6, gen, zeros=False, lo=0.25)
    prior, prior64 = gaussian_prior(d)
    start = 0.5 * torch.randn(256, d, generator=gen)
    noise = make_noise(STEPS, d, 256, gen)
    check_run(backend, start, noise, step, slots, desc, meta, tab, prior, prior64)


def test_chunk_invariance_rerun_and_keep_selection(backend):
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("6d_24x12", seed=2)
    full, final, acc, logp = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    again, final2, acc2, logp2 = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    assert torch.equal(full, again) and torch.equal(final, final2) and torch.equal(acc, acc2)
    assert torch.equal(logp.view(torch.int32), logp2.view(torch.int32))
    # 4 launches of 10 steps, step_offset advanced, into one output buffer
    x = start.clone().to(backend)
    out = torch.full((STEPS, CHAINS, d), float("nan"), device=backend)
    acc4 = torch.zeros(CHAINS, dtype=torch.int32, device=backend)
    lp4 = torch.empty(CHAINS, device=backend)
    scale = torch.full((d,), step, device=backend)
    dev_args = [t.to(backend) for t in (desc, meta, tab)]
    for t0 in range(0, STEPS, 10):
        ops.mala_ment_steps(x, *dev_args, prior, noise[t0:t0 + 10].to(backend).contiguous(), scale, acc4, step_offset=t0, out=out,
                            logp=lp4)
    assert torch.equal(out, full) and torch.equal(x, final) and torch.equal(acc4, acc)
    assert torch.equal(lp4.view(torch.int32), logp.view(torch.int32))
    # keep_from / keep_every pick rows of the full trajectory, in one launch and across launches
    for keep_from, keep_every in ((0, 1), (3, 1), (5, 7), (9, 10), (39, 3), (0, 40)):
        rows = list(range(keep_from, STEPS, keep_every))
        kept, fin, _, _ = run_kernel(backend, start, noise, step, desc, meta, tab, prior, keep_from=keep_from,
                                     keep_every=keep_every)
        assert kept.shape[0] == len(rows) and torch.equal(kept, full[rows]) and torch.equal(fin, final)
        x = start.clone().to(backend)
        out = torch.full((len(rows), CHAINS, d), float("nan"), device=backend)
        for t0, t1 in ((0, 13), (13, 14), (14, 40)):
            ops.mala_ment_steps(x, *dev_args, prior, noise[t0:t1].to(backend).contiguous(), scale, acc4, step_offset=t0,
                                keep_from=keep_from, keep_every=keep_every, out=out)
        assert torch.equal(out, full[rows])
    # nothing kept: out and logp may be None, and a keep_from beyond the run writes nothing
    x = start.clone().to(backend)
    ops.mala_ment_steps(x, *dev_args, prior, noise.to(backend), scale, acc4)
    assert torch.equal(x, final)
    none, fin, _, _ = run_kernel(backend, start, noise, step, desc, meta, tab, prior, keep_from=STEPS, keep_every=3, n_keep=2,
                                 want_logp=False)
    assert torch.isnan(none).all() and torch.equal(fin, final)


def test_chains_started_outside_the_support_walk_in_and_stay(backend):
    """Tables with zeros; half of the chains start just outside the first slot's hull (logp == -inf, gradient row 0): they
    random-walk and, once a state has logp > -inf, every later state of that chain has.  No band here: next to a zero of a table
    the gate the band rests on does not hold."""
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("2d_5x16", seed=3, zeros=True)
    start[::2] = start[::2] * 0.6 + torch.tensor([3.4, 0.0])          # just outside the first slot's hull (|x0| <= ~2.8)
    traj, final, acc, logp = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    assert torch.isfinite(traj).all() and torch.isfinite(final).all()
    T, C = traj.shape[:2]
    lp = logp32(backend, traj.reshape(T * C, d), desc, meta, tab, prior).reshape(T, C).cpu()
    lp0 = logp32(backend, start, desc, meta, tab, prior).cpu()
    assert not torch.isnan(lp).any() and not torch.isnan(lp0).any()
    assert int(torch.isneginf(lp0).sum()) >= C // 4, "the test needs chains that start outside"
    assert int((lp0 > float("-inf")).sum()) >= C // 4, "and chains that start inside"
    inside = torch.cat([lp0[None], lp]) > float("-inf")
    ever = torch.cummax(inside.to(torch.int8), 0)[0].bool()
    assert torch.equal(inside, ever), "a chain left the support (by the bits mf_ment_logprob returns)"
    entered = ~inside[0] & inside[-1]
    assert int(entered.sum()) > 0, "no outside chain found the support"
    assert torch.equal(logp.cpu().view(torch.int32), lp[-1].view(torch.int32))
    assert int(acc.sum()) > 0.02 * T * C


def test_nan_noise_is_rejected_and_does_not_spread(backend):
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("4d_mixed", seed=5)
    noise[7, 1, 11] = float("nan")            # a NaN proposal coordinate of chain 11 at step 7
    noise[9, d, 12] = float("nan")            # a NaN uniform of chain 12 at step 9
    noise[3, :, 13] = float("nan")            # a whole NaN row
    traj, final, _, logp = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    traj = traj.cpu()
    assert torch.isfinite(traj).all() and torch.isfinite(final).all() and torch.isfinite(logp).all()
    assert torch.equal(traj[7, 11], traj[6, 11]) and torch.equal(traj[9, 12], traj[8, 12]) and torch.equal(traj[3, 13], traj[2, 13])
    assert_transitions(verify(start, noise, traj, step, 1.0, slots, prior64, grad32(backend, desc, meta, tab, prior)))
    # the other chains are what they are without the NaNs
    clean = noise.clone()
    clean[7, 1, 11] = clean[9, d, 12] = 0.5
    clean[3, :, 13] = 0.5
    ref, _, _, _ = run_kernel(backend, start, clean, step, desc, meta, tab, prior)
    others = [c for c in range(CHAINS) if c not in (11, 12, 13)]
    assert torch.equal(traj[:, others], ref.cpu()[:, others])


def test_nan_noise_outside_the_support_is_rejected(backend):
    """A chain outside the support accepts every finite proposal; a NaN proposal or a NaN uniform must still leave it where it
    is.  Zero slots and the uniform prior on [-1, 1]^2: a NaN point is outside (logp == -inf), the branch that accepts."""
    d, C = 2, 256
    gen = torch.Generator().manual_seed(8)
    desc, meta, tab = torch.zeros(0, 24), torch.zeros(0, 4, dtype=torch.int32), torch.zeros(1)
    prior = (2, 1.0, -d * math.log(2.0))
    start = torch.full((C, d), 5.0)
    noise = make_noise(4, d, C, gen)
    noise[1, 0, 3] = float("nan")
    noise[2, d, 4] = float("nan")
    traj, final, acc, _ = run_kernel(backend, start, noise, 0.1, desc, meta, tab, prior)
    traj = traj.cpu()
    assert torch.isfinite(traj).all()
    assert torch.equal(traj[1, 3], traj[0, 3]) and torch.equal(traj[2, 4], traj[1, 4])
    expect = torch.full((C,), 4, dtype=torch.int32)
    expect[3] = expect[4] = 3
    assert torch.equal(acc.cpu(), expect), "outside the support every finite proposal to another outside point is accepted"


def test_density_is_recomputed_at_entry(backend):
    """The tables change between two calls (a Gauss-Seidel update): the second call's transitions verify against the NEW
    log-density and gradient from the first step on, with no state but x carried over."""
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("2d_5x16", seed=4)
    _, mid, _, _ = run_kernel(backend, start, noise[:20], step, desc, meta, tab, prior)
    gen = torch.Generator().manual_seed(99)
    tab2 = tab * (0.5 + torch.rand(tab.shape, generator=gen))
    slots2, off = [], 0
    for rows, coords, values in slots:
        slots2.append((rows, coords, tab2[off:off + values.numel()].reshape(values.shape)))
        off += values.numel()
    traj, _, _, _ = run_kernel(backend, mid.cpu(), noise[20:], step, desc, meta, tab2, prior)
    assert_transitions(verify(mid.cpu(), noise[20:], traj, step, 1.0, slots2, prior64, grad32(backend, desc, meta, tab2, prior)))


def test_stationarity(backend):
    """No slots, Gaussian prior of scale s in d = 3, drift_clip = 1: 4096 chains started from exact draws of N(0, s^2 I), 40
    steps.  Mean and variance bounds: module docstring.  The acceptance rate must lie strictly inside (0.3, 1), so a kernel that
    never moves (trivially stationary) fails: at step s / 2 the Langevin proposal on a Gaussian is accepted far more often than
    not."""
    d, C, T, s = 3, 4096, 40, 1.3
    gen = torch.Generator().manual_seed(21)
    start = s * torch.randn(C, d, generator=gen)
    noise = make_noise(T, d, C, gen)
    prior, _ = gaussian_prior(d, s)
    desc, meta, tab = torch.zeros(0, 24), torch.zeros(0, 4, dtype=torch.int32), torch.zeros(1)
    _, final, acc, _ = run_kernel(backend, start, noise, 0.5 * s, desc, meta, tab, prior)
    final = final.cpu().double()
    assert float(final.mean(0).abs().max()) <= 5 * s / math.sqrt(C), final.mean(0)
    assert float((final.var(0) - s * s).abs().max()) <= 5 * s * s * math.sqrt(2.0 / (C - 1)), final.var(0)
    rate = float(acc.sum()) / (C * T)
    print("acceptance", rate)
    assert 0.3 < rate < 1.0


def test_stays_a_metropolis_chain_where_the_product_leaves_fp32(backend):
    """6-D, 100 one-axis factors of ~1e-3 (the tables of the log-density range test): mf_ment_prob is 0 everywhere, so the
    Metropolis-Hastings kernel sees no support at all and walks freely, while logp is about -690 and finite.  The Langevin chains
    started inside keep a finite logp, and no transition is wrong or malformed by the verifier.  Its band is relative to
    1 + |l| as the gate it is derived from, so with |l| ~ 690 it is b ~ 3e-4 * 1380 = 0.41 wide on either side and holds about a
    quarter of the uniforms: the 4 % cap of the other tests cannot apply to the band's share here.  The rest of the ambiguous
    transitions (bin centres, clamp) is capped apart, and the acceptance rate must lie in the interval the fp64 rule leaves open:
    between its must-accept share and that plus the ambiguous share (implied by "none wrong"; asserted so that the figures print).
    The step is 0.05, 0.4 of the tables' bin width (8 / 64): a hundred piecewise-linear factors change slope at every centre,
    and a proposal is informed by the gradient only within a cell."""
    d, C, step = 6, 256, 0.05
    gen = torch.Generator().manual_seed(5)
    slots, desc, meta, tab = make_logp_slots(d, [(1, 64)] * 100, gen, lo=0.5e-3, hi=2e-3)
    start = 0.8 * torch.randn(C, d, generator=gen)
    noise = make_noise(STEPS, d, C, gen)
    prior, prior64 = NO_PRIOR
    dev_args = [t.to(backend) for t in (desc, meta, tab)]
    assert torch.isfinite(logp32(backend, start, desc, meta, tab, prior)).all(), "the chains are meant to start inside"
    assert (ops.ment_prob(start.to(backend), *dev_args) == 0).all(), "the product is meant to underflow here"
    traj, final, acc, logp = run_kernel(backend, start, noise, step, desc, meta, tab, prior)
    assert (ops.ment_prob(final, *dev_args) == 0).all(), "the density mf_mcmc_ment_steps compares is 0 at every state"
    lp = logp32(backend, traj.reshape(-1, d), desc, meta, tab, prior)
    assert torch.isfinite(lp).all() and float(lp.max()) < -600
    stats = verify(start, noise, traj, step, 1.0, slots, prior64, grad32(backend, desc, meta, tab, prior))
    print(stats)
    assert stats["accept_wrong"] == 0 and stats["reject_wrong"] == 0 and stats["malformed"] == 0, stats
    assert stats["ambiguous"] - stats["in_band"] <= 0.04 * stats["total"], stats
    assert stats["must_accept"] <= stats["accepted"] <= stats["must_accept"] + stats["ambiguous"], stats
    assert 0.02 * stats["total"] < stats["accepted"] < stats["total"]


def test_refusals(backend):
    """The C entry point refuses bad arguments with a non-zero return and mf_last_error set, before any launch."""
    import ctypes as C
    d, step, slots, desc, meta, tab, prior, prior64, start, noise = problem("2d_5x16")
    dev = backend
    lib = _lib.get_lib()
    x = start.to(dev).contiguous()
    nz, scale = noise.to(dev).contiguous(), torch.full((d,), step, device=dev)
    acc = torch.zeros(CHAINS, dtype=torch.int32, device=dev)
    dsc, mt, tb = [t.to(dev) for t in (desc, meta, tab)]
    p = _lib.ptr

    def call(chains=CHAINS, dd=d, nslot=desc.shape[0], steps=STEPS, step_offset=0, clip=1.0, keep_from=0, keep_every=1):
        return lib.mf_mala_ment_steps(p(x), chains, dd, nslot, p(dsc), p(mt), p(tb), tb.numel(), prior[0], prior[1], prior[2],
                                      p(nz), steps, step_offset, p(scale), clip, keep_from, keep_every, None, p(acc), None,
                                      ops.stream_ptr(x))

    for kwargs in (dict(dd=9), dict(dd=0), dict(nslot=513), dict(chains=-1), dict(chains=2 ** 31), dict(steps=-1),
                   dict(step_offset=-1), dict(keep_from=-1), dict(keep_every=0), dict(keep_every=2 ** 50), dict(steps=2 ** 41),
                   dict(clip=-0.5), dict(clip=float("nan"))):
        assert call(**kwargs) != 0, kwargs
        assert lib.mf_last_error().decode(), kwargs
    assert "drift_clip" in lib.mf_last_error().decode()
    assert torch.equal(x.cpu(), start) and int(acc.sum()) == 0, "a refused call must not touch the state"
    assert call(chains=0) == 0
    assert torch.equal(x.cpu(), start)
    # the wrapper's own checks
    with pytest.raises(RuntimeError, match="noise"):
        ops.mala_ment_steps(x, dsc, mt, tb, prior, nz[:, :d], scale, acc)
    with pytest.raises(RuntimeError, match="drift_clip"):
        ops.mala_ment_steps(x, dsc, mt, tb, prior, nz, scale, acc, drift_clip=-1.0)
    with pytest.raises(RuntimeError, match="logp"):
        ops.mala_ment_steps(x, dsc, mt, tb, prior, nz, scale, acc, logp=torch.empty(CHAINS - 1, device=dev))
    with pytest.raises(RuntimeError, match="keep_every"):
        ops.mala_ment_steps(x, dsc, mt, tb, prior, nz, scale, acc, keep_every=0)
    assert torch.equal(x.cpu(), start)
