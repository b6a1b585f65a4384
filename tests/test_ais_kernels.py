"""The annealed-importance-sampling kernel (mentflow_amd/csrc/ais.hip, ops.ais_ment_steps) against the fp64 transition verifier of
tests/_ais_fp64.py, on the emulator here and on the MI355X with -m gpu (the `backend` fixture).

Every transition of the ladder is classified in fp64 from the kernel's own previous state (the `out` rows); none may disagree
outside the band of _ais_fp64 and at most 4 % may be ambiguous.  Band-verified cases use tables uniform in [0.25, 2], for the
reason tests/test_mala_kernels.py gives.  The log-weights are restated from the same trajectory: the increment of temperature k is
the fp32 product (b_k - b_{k-1}) * (lp - lq) at the state the chain had when it reached k, with lp from ops.ment_logprob (the
kernel's own bits) and lq restated in fp32 in the kernel's order, summed in fp64; the restatement differs from the kernel by the
rounding of c0 at most, so it must hold to 1e-6 (1 + |logw|), the bound the importance-sampling identity is given.

The ladder of the verified cases has 8 temperatures with a leading b == 0 (transitions on the base alone, where lp must not
matter), two repeated temperatures (increments of exactly 0) and uneven gaps."""
import ctypes as C
import math

import pytest
import torch

from _ais_fp64 import assert_transitions, base32, verify
from mentflow_amd import _lib, ops
from test_mcmc_kernels import SHAPES, gaussian_prior, make_noise
from test_ment_kernels import make_slots

CHAINS, SPT = 300, 3                                    # two workgroups, the second with 44 lanes
LADDER = torch.tensor([0.0, 0.0, 0.1, 0.25, 0.25, 0.5, 0.8, 1.0, 1.0])
K = LADDER.numel() - 1


def prior_of(kind, d):
    if kind == "none":
        return (0, 0.0, 0.0), None
    if kind == "gaussian":
        return gaussian_prior(d)
    return (2, 2.5, -d * math.log(5.0)), ("uniform", 2.5)


def base_of(d):
    return [0.1 * (-1) ** j for j in range(d)], [1.2 + 0.05 * j for j in range(d)]


def run_kernel(dev, start, noise, betas, spt, step, desc, meta, tab, prior, mean, base, drift_clip=1.0, temp_offset=0, ntemps=None,
               want_out=True, state=None):
    """(out, x, logw, accepted, logp) of one ops.ais_ment_steps call; state = (x, logw, accepted, logp, out) continues a run."""
    chains, d = start.shape
    total = (betas.numel() - 1) * spt
    if state is None:
        state = (start.clone().to(dev).contiguous(), torch.zeros(chains, dtype=torch.float64, device=dev),
                 torch.zeros(chains, dtype=torch.int32, device=dev), torch.full((chains,), float("nan"), device=dev),
                 torch.full((total, chains, d), float("nan"), device=dev) if want_out and total else None)
    x, logw, acc, logp, out = state
    scale = torch.full((d,), float(step), device=dev)
    ops.ais_ment_steps(x, desc.to(dev), meta.to(dev), tab.to(dev), prior, noise.to(dev).contiguous(), betas.to(dev), spt, scale,
                       mean, base, logw, acc, drift_clip=drift_clip, temp_offset=temp_offset, ntemps=ntemps, out=out, logp=logp)
    return out, x, logw, acc, logp


def logp32_on(dev, desc, meta, tab, prior):
    """x -> (lp32, g32) of ops.ment_logprob on the backend: what the kernel's proposals and weights are built from."""
    args = [t.to(dev) for t in (desc, meta, tab)]

    def f(x):
        lp, g = ops.ment_logprob(x.to(dev).contiguous(), *args, prior, want_grad=True)
        return lp.cpu(), g.cpu()
    return f


def logw_restated(start, traj, betas, spt, lpf, mean, base):
    """The log-weights from the trajectory: module docstring."""
    logw = torch.zeros(start.shape[0], dtype=torch.float64)
    for k in range(1, betas.numel()):
        at = start if k == 1 or spt == 0 else traj[(k - 1) * spt - 1]
        if float(betas[k]) == float(betas[k - 1]):
            continue
        lp = lpf(at)[0].float()
        lq = base32(at, mean, base)[0]
        inc = (betas[k] - betas[k - 1]) * (lp - lq)
        logw += torch.where(lp > float("-inf"), inc, torch.full_like(inc, float("-inf"))).double()
    return logw


def assert_logw(logw, expect):
    logw, expect = logw.cpu(), expect.cpu()
    assert not torch.isnan(logw).any()
    assert torch.equal(torch.isneginf(logw), torch.isneginf(expect))
    fin = torch.isfinite(expect)
    assert torch.isfinite(logw[fin]).all()
    assert bool(((logw[fin] - expect[fin]).abs() <= 1e-6 * (1 + expect[fin].abs())).all()), (logw[fin] - expect[fin]).abs().max()


def check_run(backend, d, step, slots, desc, meta, tab, prior, prior64, gen, drift_clip=1.0):
    mean, base = base_of(d)
    start = torch.tensor(mean) + torch.tensor(base) * torch.randn(CHAINS, d, generator=gen)
    noise = make_noise(K * SPT, d, CHAINS, gen)
    traj, final, logw, acc, logp = run_kernel(backend, start, noise, LADDER, SPT, step, desc, meta, tab, prior, mean, base,
                                              drift_clip)
    lpf = logp32_on(backend, desc, meta, tab, prior)
    stats = verify(start, noise, traj, LADDER[1:].repeat_interleave(SPT), step, drift_clip, slots, prior64, lpf, mean, base)
    print(stats)
    assert_transitions(stats)
    assert stats["accepted"] > 0.02 * stats["total"], "the chains must move"
    traj = traj.cpu()
    assert torch.equal(final.cpu(), traj[-1])
    prev = torch.cat([start[None], traj[:-1]])
    assert torch.equal(acc.cpu(), (traj != prev).any(2).sum(0).to(torch.int32))
    assert torch.equal(logp.cpu().view(torch.int32), lpf(final)[0].view(torch.int32))
    assert_logw(logw, logw_restated(start, traj, LADDER, SPT, lpf, mean, base))
    return stats


@pytest.mark.parametrize("name", ["2d_5x16", "6d_24x12", "4d_mixed"])
@pytest.mark.parametrize("prior_kind", ["none", "gaussian", "uniform"])
def test_transitions_verified(backend, name, prior_kind):
    """d = 2, d = 6 and the 8 mixed 1-D / 2-D slots in d = 4, under no prior, the Gaussian and the box (|x| <= 2.5, which
    leaves a few per cent of the starts outside: chains of weight 0 that walk in)."""
    d, specs, step = SHAPES[name]
    gen = torch.Generator().manual_seed(3100 + 7 * d)
    slots, desc, meta, tab = make_slots(d, specs, gen, zeros=False, lo=0.25)
    prior, prior64 = prior_of(prior_kind, d)
    check_run(backend, d, step, slots, desc, meta, tab, prior, prior64, gen)


def test_transitions_tables_beyond_lds(backend):
    """6 x 85^2 2-D tables (43 350 floats): read from global memory, as in test_mala_kernels.py."""
    d, step = 4, 0.4
    gen = torch.Generator().manual_seed(7)
    slots, desc, meta, tab = make_slots(d, [(2, 85)] * 6, gen, zeros=False, lo=0.25)
    prior, prior64 = gaussian_prior(d)
    check_run(backend, d, step, slots, desc, meta, tab, prior, prior64, gen)


def test_driftless_walk(backend):
    """drift_clip = 0: a random walk under the same acceptance rule on the tempered log-density."""
    d, specs, step = SHAPES["2d_5x16"]
    gen = torch.Generator().manual_seed(6)
    slots, desc, meta, tab = make_slots(d, specs, gen, zeros=False, lo=0.25)
    prior, prior64 = gaussian_prior(d)
    check_run(backend, d, step, slots, desc, meta, tab, prior, prior64, gen, drift_clip=0.0)


def problem(name="4d_mixed", seed=0, zeros=False, chains=CHAINS):
    d, specs, step = SHAPES[name]
    gen = torch.Generator().manual_seed(4000 + seed)
    slots, desc, meta, tab = make_slots(d, specs, gen, zeros=zeros, lo=0.0 if zeros else 0.25)
    prior, _ = gaussian_prior(d)
    mean, base = base_of(d)
    start = torch.tensor(mean) + torch.tensor(base) * torch.randn(chains, d, generator=gen)
    return d, step, desc, meta, tab, prior, mean, base, start, gen


def test_importance_sampling_identity(backend):
    """K = 1 and no moves: plain importance sampling.  logw is double(fp32(lp - lq)) and x is untouched."""
    d, step, desc, meta, tab, prior, mean, base, start, gen = problem(zeros=True)
    start[:5] = 30.0                                                 # outside every hull
    noise = torch.zeros(0, d + 1, CHAINS)
    _, x, logw, acc, logp = run_kernel(backend, start, noise, torch.tensor([0.0, 1.0]), 0, step, desc, meta, tab, prior, mean, base)
    assert torch.equal(x.cpu().view(torch.int32), start.view(torch.int32))
    lp = logp32_on(backend, desc, meta, tab, prior)(start)[0]
    expect = (lp - base32(start, mean, base)[0]).double()
    assert int(torch.isneginf(expect).sum()) >= 5 and int(torch.isfinite(expect).sum()) > CHAINS // 2
    assert_logw(logw, expect)
    assert int(acc.sum()) == 0
    assert torch.equal(logp.cpu().view(torch.int32), lp.view(torch.int32))


def test_split_invariance_and_rerun(backend):
    d, step, desc, meta, tab, prior, mean, base, start, gen = problem("6d_24x12", seed=1)
    noise = make_noise(K * SPT, d, CHAINS, gen)
    one = run_kernel(backend, start, noise, LADDER, SPT, step, desc, meta, tab, prior, mean, base)
    again = run_kernel(backend, start, noise, LADDER, SPT, step, desc, meta, tab, prior, mean, base)
    first = run_kernel(backend, start, noise[:3 * SPT], LADDER, SPT, step, desc, meta, tab, prior, mean, base, ntemps=3)
    split = run_kernel(backend, start, noise[3 * SPT:], LADDER, SPT, step, desc, meta, tab, prior, mean, base, temp_offset=3,
                       ntemps=5, state=(first[1], first[2], first[3], first[4], first[0]))
    for other in (again, split):
        out, x, logw, acc, logp = other
        assert torch.equal(out.view(torch.int32), one[0].view(torch.int32))
        assert torch.equal(x.view(torch.int32), one[1].view(torch.int32))
        assert torch.equal(logw.view(torch.int64), one[2].view(torch.int64))
        assert torch.equal(acc, one[3])
        assert torch.equal(logp.view(torch.int32), one[4].view(torch.int32))
    assert int(one[3].sum()) > 0 and torch.isfinite(one[2]).any()
    # out == None and logp == None are taken
    x = start.clone().to(backend)
    logw = torch.zeros(CHAINS, dtype=torch.float64, device=backend)
    acc = torch.zeros(CHAINS, dtype=torch.int32, device=backend)
    ops.ais_ment_steps(x, desc.to(backend), meta.to(backend), tab.to(backend), prior, noise.to(backend), LADDER.to(backend), SPT,
                       torch.full((d,), step, device=backend), mean, base, logw, acc)
    assert torch.equal(x, one[1]) and torch.equal(logw, one[2]) and torch.equal(acc, one[3])


def test_start_outside_every_hull_has_weight_zero(backend):
    """Tables with zeros; a quarter of the chains start outside every hull: logw == -inf exactly, whatever they do later, and no
    NaN anywhere.  A temperature equal to the one before adds exactly 0, also outside the support."""
    d, step, desc, meta, tab, prior, mean, base, start, gen = problem("2d_5x16", seed=2, zeros=True)
    start[::4] = start[::4] * 0.1 + 30.0
    noise = make_noise(K * SPT, d, CHAINS, gen)
    traj, x, logw, acc, logp = run_kernel(backend, start, noise, LADDER, SPT, step, desc, meta, tab, prior, mean, base)
    assert torch.isneginf(logw[::4]).all()
    assert not torch.isnan(logw).any() and torch.isfinite(traj).all() and torch.isfinite(x).all() and not torch.isnan(logp).any()
    assert torch.isfinite(logw).sum() > CHAINS // 2
    # the ladder [0, 0, 0]: two temperatures that add nothing, inside or outside; the moves are those of the base alone
    flat = torch.zeros(3)
    _, x0, logw0, acc0, _ = run_kernel(backend, start, noise[:2 * SPT], flat, SPT, step, desc, meta, tab, prior, mean, base)
    assert torch.equal(logw0.cpu(), torch.zeros(CHAINS, dtype=torch.float64))
    assert int(acc0.sum()) > 0.3 * 2 * SPT * CHAINS, "at b == 0 a chain moves on the base, inside the support or not"
    # [0, 1, 1]: the second temperature adds exactly 0
    once, twice = torch.tensor([0.0, 1.0]), torch.tensor([0.0, 1.0, 1.0])
    _, _, logw1, _, _ = run_kernel(backend, start, noise[:SPT], once, SPT, step, desc, meta, tab, prior, mean, base)
    _, _, logw2, _, _ = run_kernel(backend, start, noise[:2 * SPT], twice, SPT, step, desc, meta, tab, prior, mean, base)
    assert torch.equal(logw1.view(torch.int64), logw2.view(torch.int64))


def test_nan_noise_leaves_the_state_alone(backend):
    d, step, desc, meta, tab, prior, mean, base, start, gen = problem(seed=3)
    start[13] = 30.0                                       # an outside chain accepts every finite proposal, but not a NaN one
    noise = make_noise(K * SPT, d, CHAINS, gen)
    noise[7, 1, 11] = float("nan")
    noise[9, d, 12] = float("nan")
    noise[3, :, 13] = float("nan")
    noise[0, 0, 14] = float("nan")                         # at b == 0
    traj, x, logw, acc, logp = run_kernel(backend, start, noise, LADDER, SPT, step, desc, meta, tab, prior, mean, base)
    traj = traj.cpu()
    assert torch.isfinite(traj).all() and not torch.isnan(logw).any() and not torch.isnan(logp).any()
    assert torch.equal(traj[7, 11], traj[6, 11]) and torch.equal(traj[9, 12], traj[8, 12]) and torch.equal(traj[3, 13], traj[2, 13])
    assert torch.equal(traj[0, 14], start[14])
    clean = noise.clone()
    clean[torch.isnan(clean)] = 0.5
    ref = run_kernel(backend, start, clean, LADDER, SPT, step, desc, meta, tab, prior, mean, base)
    others = [c for c in range(CHAINS) if c not in (11, 12, 13, 14)]
    assert torch.equal(traj[:, others], ref[0].cpu()[:, others]) and torch.equal(logw.cpu()[others], ref[2].cpu()[others])


def test_no_chains_and_no_temperatures_do_nothing(backend):
    d, step, desc, meta, tab, prior, mean, base, start, gen = problem(seed=4)
    empty = run_kernel(backend, start[:0], torch.zeros(K * SPT, d + 1, 0), LADDER, SPT, step, desc, meta, tab, prior, mean, base,
                       want_out=False)
    assert empty[1].shape == (0, d)
    _, x, logw, acc, _ = run_kernel(backend, start, torch.zeros(0, d + 1, CHAINS), LADDER, SPT, step, desc, meta, tab, prior, mean,
                                    base, ntemps=0, want_out=False)
    assert torch.equal(x.cpu(), start) and int(acc.sum()) == 0 and torch.equal(logw.cpu(), torch.zeros(CHAINS, dtype=torch.float64))


def test_refusals(backend):
    """The C entry point refuses bad arguments with a non-zero return and mf_last_error set, before any launch."""
    d, step, desc, meta, tab, prior, mean, base, start, gen = problem(seed=5)
    dev = backend
    lib = _lib.get_lib()
    x = start.to(dev).contiguous()
    nz = make_noise(K * SPT, d, CHAINS, gen).to(dev).contiguous()
    scale, betas = torch.full((d,), step, device=dev), LADDER.to(dev)
    acc = torch.zeros(CHAINS, dtype=torch.int32, device=dev)
    logw = torch.zeros(CHAINS, dtype=torch.float64, device=dev)
    dsc, mt, tb = [t.to(dev) for t in (desc, meta, tab)]
    p = _lib.ptr

    def call(chains=CHAINS, dd=d, spt=SPT, ntemps=K, temp_offset=0, clip=1.0, lw=logw, b=base, m=mean):
        mh, bh = (C.c_float * 9)(*(list(m) + [0.0] * (9 - len(m)))), (C.c_float * 9)(*(list(b) + [1.0] * (9 - len(b))))
        return lib.mf_ais_ment_steps(p(x), chains, dd, desc.shape[0], p(dsc), p(mt), p(tb), tb.numel(), prior[0], prior[1],
                                     prior[2], p(nz), p(betas), betas.numel(), ntemps, temp_offset, spt, p(scale), clip,
                                     C.cast(mh, C.c_void_p), C.cast(bh, C.c_void_p), p(lw), None, p(acc), None,
                                     ops.stream_ptr(x))

    for kwargs, word in ((dict(dd=9), "ndim"), (dict(spt=-1), "steps_per_temp"), (dict(lw=None), "logw"),
                         (dict(b=[1.0, 0.0, 1.0, 1.0]), "base_scale"), (dict(b=[1.0, -2.0, 1.0, 1.0]), "base_scale"),
                         (dict(b=[float("nan")] * 4), "base_scale"), (dict(ntemps=K + 1), "ladder"),
                         (dict(temp_offset=1), "ladder"), (dict(ntemps=-1), "ntemps"), (dict(chains=-1), "chain"),
                         (dict(clip=-0.5), "drift_clip"), (dict(clip=float("nan")), "drift_clip")):
        assert call(**kwargs) != 0, kwargs
        assert word in lib.mf_last_error().decode(), (kwargs, lib.mf_last_error().decode())
    assert torch.equal(x.cpu(), start) and int(acc.sum()) == 0 and float(logw.abs().sum()) == 0, "a refused call touches nothing"
    assert call(chains=0) == 0 and call(ntemps=0) == 0
    assert torch.equal(x.cpu(), start)
    # the wrapper's own checks
    args = (x, dsc, mt, tb, prior, nz, betas, SPT, scale, mean, base, logw, acc)
    with pytest.raises(RuntimeError, match="noise"):
        ops.ais_ment_steps(*args[:5], nz[:-1], *args[6:])
    with pytest.raises(RuntimeError, match="steps_per_temp"):
        ops.ais_ment_steps(*args[:7], -1, *args[8:])
    with pytest.raises(RuntimeError, match="base_scale"):
        ops.ais_ment_steps(*args[:10], [1.0, 1.0, 0.0, 1.0], *args[11:])
    with pytest.raises(RuntimeError, match="logw"):
        ops.ais_ment_steps(*args[:11], logw.float(), acc)
    with pytest.raises(RuntimeError, match="drift_clip"):
        ops.ais_ment_steps(*args, drift_clip=-1.0)
    with pytest.raises(RuntimeError, match="logp"):
        ops.ais_ment_steps(*args, logp=torch.empty(CHAINS - 1, device=dev))
    assert torch.equal(x.cpu(), start)
