"""The resampling kernels of the sequential Monte Carlo sampler (mentflow_amd/csrc/smc.hip, ops.smc_resample) against the fp64
restatement of tests/_smc_fp64.py, on the emulator here and on the MI355X with -m gpu (the `backend` fixture).

Shapes: islands of S = 1, 2, 255, 256, 257, 1000 and 4099 chains (one thread segment, ragged segments, 5 elements per thread of the
1 024-thread workgroup), 1, 3 and 8 islands, d = 1, 6 and 8 (rows copied as floats, float2 and float4).  Log-weight patterns:
3 N(0, 1); the same shifted by -5 000 (every weight underflows without the max subtraction); a quarter of the entries -inf; all
but one -inf; all -inf; one NaN entry; all equal.

The kernel sums in thread segments and the restatement with cumsum, so a position within 1e-11 S1 of a prefix boundary may take
either neighbour (_smc_fp64.resample64's lo and hi); such rows are at most 0.5 % of all rows, and with continuous random weights
there are none.  Everything else is exact or holds to 1e-12."""
import ctypes as C

import numpy as np
import pytest
import torch

from _smc_fp64 import resample64
from mentflow_amd import _lib, ops

SIZES = [1, 2, 255, 256, 257, 1000, 4099]
GROUPS = [1, 3, 8]
DIMS = [1, 6, 8]
PATTERNS = ["normal", "shifted", "quarter_dead", "one_alive", "all_dead", "one_nan", "equal"]
UMAX = 1.0 - 2.0 ** -53


def make_logw(pattern, chains, gen, scale=3.0):
    lw = scale * torch.randn(chains, dtype=torch.float64, generator=gen)
    if pattern == "shifted":
        lw = lw - 5000.0
    elif pattern == "quarter_dead":
        lw[torch.rand(chains, generator=gen) < 0.25] = float("-inf")
    elif pattern == "one_alive":
        keep = int(torch.randint(chains, (1,), generator=gen))
        value = lw[keep].clone()
        lw[:] = float("-inf")
        lw[keep] = value
    elif pattern == "all_dead":
        lw[:] = float("-inf")
    elif pattern == "one_nan":
        lw[int(torch.randint(chains, (1,), generator=gen))] = float("nan")
    elif pattern == "equal":
        lw[:] = 0.7
    return lw


def run(dev, x, logw, u, groups, threshold):
    """(x_out, ancestors, stats, logw afterwards) of one ops.smc_resample call, as CPU tensors; logw itself is not changed."""
    lw = logw.clone().to(dev)
    x_out, anc, stats = ops.smc_resample(x.to(dev).contiguous(), lw, u.to(dev), groups, threshold)
    assert x_out.dtype == torch.float32 and anc.dtype == torch.int32 and stats.dtype == torch.float64
    assert tuple(x_out.shape) == tuple(x.shape) and tuple(anc.shape) == (x.shape[0],) and tuple(stats.shape) == (groups, 4)
    return x_out.cpu(), anc.cpu().long(), stats.cpu(), lw.cpu()


def same_bits(a, b):
    view = torch.int64 if a.dtype == torch.float64 else torch.int32
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def assert_stats(stats, expect):
    stats, expect = stats.numpy(), np.asarray(expect)
    fin = np.isfinite(expect)
    assert np.array_equal(stats[~fin], expect[~fin])
    assert bool((np.abs(stats[fin] - expect[fin]) <= 1e-12 * np.abs(expect[fin])).all()), (stats, expect)


def check_against_restatement(x, logw, u, groups, threshold, got, pattern):
    """Every property of the module docstring for one call; returns the number of ambiguous rows."""
    x_out, anc, stats, lw_after = got
    chains = x.shape[0]
    S = chains // groups
    r = resample64(logw.numpy(), u.numpy(), groups, threshold)
    assert_stats(stats, r["stats"])
    a = anc.numpy()
    assert bool(((a >= r["lo"]) & (a <= r["hi"])).all()), "a parent outside what the restatement allows"
    ambiguous = int((r["lo"] != r["hi"]).sum())
    assert same_bits(x_out, x[anc]), "x_out is x[ancestors], bitwise"
    for g in range(groups):
        sl = slice(g * S, (g + 1) * S)
        if not r["stats"][g, 2]:
            assert np.array_equal(a[sl], np.arange(g * S, (g + 1) * S)), "an island that does not resample keeps its rows"
            assert same_bits(lw_after[sl], logw[sl]), "and its logw, bit for bit"
            continue
        assert bool((np.diff(a[sl]) >= 0).all()), "parents do not decrease within an island"
        assert bool((a[sl] >= g * S).all() and (a[sl] < (g + 1) * S).all())
        w = r["weight"][sl]
        assert bool((w[a[sl] - g * S] > 0).all()), "a state of weight 0 (or NaN) is never a parent"
        counts = np.bincount(a[sl] - g * S, minlength=S)
        assert bool((np.abs(counts - S * w / w.sum()) < 1 + 1e-9).all()), "offspring counts of systematic resampling"
        assert bool((lw_after[sl] == stats[g, 0]).all()), "every logw of the island is its log mean weight"
        before = float(torch.logsumexp(torch.nan_to_num(logw[sl], nan=float("-inf")), 0)) - np.log(S)
        after = float(torch.logsumexp(lw_after[sl], 0)) - np.log(S)
        assert abs(after - before) <= 1e-12 * (1 + abs(before)), (before, after)
    if pattern != "one_nan":
        assert not torch.isnan(stats).any() and not torch.isnan(lw_after).any()
    return ambiguous


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("groups", GROUPS)
@pytest.mark.parametrize("S", SIZES)
def test_resampling_against_restatement(backend, S, groups, d):
    """Every island resamples (threshold 1.1: ess <= S), except those whose weights are all zero."""
    chains = S * groups
    gen = torch.Generator().manual_seed(1000 * S + 10 * groups + d)
    x = torch.randn(chains, d, generator=gen)
    ambiguous = rows = 0
    for pattern in PATTERNS:
        logw = make_logw(pattern, chains, gen)
        u = 0.05 + 0.9 * torch.rand(groups, dtype=torch.float64, generator=gen)
        got = run(backend, x, logw, u, groups, 1.1)
        n = check_against_restatement(x, logw, u, groups, 1.1, got, pattern)
        if pattern == "normal":
            assert n == 0, "continuous random weights: the restatement has no ambiguous row"
        if pattern == "all_dead":
            assert float(got[2][:, 2].sum()) == 0 and same_bits(got[0], x), "nothing to resample from"
        ambiguous, rows = ambiguous + n, rows + chains
    assert ambiguous <= 0.005 * rows, (ambiguous, rows)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("S", SIZES)
def test_equal_weights_give_the_identity(backend, S, d):
    """w = 1, P_i = i + 1, c = 1: the arithmetic is exact, and every u in [0, 1) keeps every row where it is."""
    groups = 3
    chains = S * groups
    x = torch.randn(chains, d, generator=torch.Generator().manual_seed(S + d))
    logw = make_logw("equal", chains, None)
    for u0 in (0.0, 0.5, UMAX):
        u = torch.full((groups,), u0, dtype=torch.float64)
        x_out, anc, stats, lw_after = run(backend, x, logw, u, groups, 1.1)
        assert torch.equal(anc, torch.arange(chains)), u0
        assert same_bits(x_out, x) and same_bits(lw_after, logw)
        assert torch.equal(stats, torch.tensor([[0.7, float(S), 1.0, 0.7]] * groups, dtype=torch.float64))
    # u outside [0, 1) and NaN are clamped into it
    for u0 in (-1.0, 1.0, 7.5, float("nan"), float("inf")):
        _, anc, _, _ = run(backend, x, logw, torch.full((groups,), u0, dtype=torch.float64), groups, 1.1)
        assert torch.equal(anc, torch.arange(chains)), u0


@pytest.mark.parametrize("S", [2, 257, 1000])
def test_decision_per_island(backend, S):
    """Eight islands whose weights spread differently: flat (no resampling at 0.5), 3 N(0, 1) (resampling), all -inf (none)."""
    groups, d = 8, 6
    chains = S * groups
    gen = torch.Generator().manual_seed(77 + S)
    x = torch.randn(chains, d, generator=gen)
    logw = torch.cat([make_logw("all_dead" if g == 2 else "normal", S, gen, scale=(0.3 if g % 2 else 3.0)) for g in range(groups)])
    u = 0.05 + 0.9 * torch.rand(groups, dtype=torch.float64, generator=gen)
    seen = set()
    for threshold in (0.5, 0.9, 0.0, 1.1):
        r = resample64(logw.numpy(), u.numpy(), groups, threshold)
        while not bool((r["margin"] > 1e-6).all()):                   # keep clear of the threshold itself
            threshold += 0.013
            r = resample64(logw.numpy(), u.numpy(), groups, threshold)
        got = run(backend, x, logw, u, groups, threshold)
        assert torch.equal(got[2][:, 2], torch.from_numpy(r["stats"][:, 2])), threshold
        check_against_restatement(x, logw, u, groups, threshold, got, "normal")
        assert not torch.isnan(got[2]).any() and not torch.isnan(got[3]).any()
        assert float(got[2][2, 2]) == 0 and float(got[2][2, 1]) == 0 and torch.isneginf(got[2][2, 0]), "the all -inf island"
        seen.add(int(got[2][:, 2].sum()))
    assert len(seen) >= 3 and 0 in seen, seen
    # a NaN threshold resamples nothing
    got = run(backend, x, logw, u, groups, float("nan"))
    assert float(got[2][:, 2].sum()) == 0 and same_bits(got[0], x) and same_bits(got[3], logw)


@pytest.mark.parametrize("S", [1, 257, 4099])
def test_islands_are_independent_and_calls_reproducible(backend, S):
    groups, d = 3, 6
    chains = S * groups
    gen = torch.Generator().manual_seed(5 + S)
    x = torch.randn(chains, d, generator=gen)
    logw = torch.cat([make_logw(p, S, gen) for p in ("quarter_dead", "normal", "one_nan")])
    u = torch.rand(groups, dtype=torch.float64, generator=gen)
    one = run(backend, x, logw, u, groups, 1.1)
    again = run(backend, x, logw, u, groups, 1.1)
    assert same_bits(one[0], again[0]) and torch.equal(one[1], again[1]) and same_bits(one[2], again[2])
    assert same_bits(one[3], again[3])
    for g in range(groups):
        sl = slice(g * S, (g + 1) * S)
        alone = run(backend, x[sl], logw[sl], u[g:g + 1], 1, 1.1)
        assert same_bits(alone[0], one[0][sl]) and torch.equal(alone[1] + g * S, one[1][sl])
        assert same_bits(alone[2], one[2][g:g + 1]) and same_bits(alone[3], one[3][sl])


def test_refusals(backend):
    """The C entry point refuses bad arguments with a non-zero return and mf_last_error set, before any launch."""
    dev = backend
    lib = _lib.get_lib()
    chains, d, groups = 24, 6, 3
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(chains, d, generator=gen).to(dev)
    x_out = torch.full((chains, d), float("nan"), device=dev)
    logw = torch.randn(chains, dtype=torch.float64, generator=gen).to(dev)
    kept = logw.clone()
    u = torch.rand(groups, dtype=torch.float64, generator=gen).to(dev)
    anc = torch.full((chains,), -1, dtype=torch.int32, device=dev)
    stats = torch.full((groups, 4), float("nan"), dtype=torch.float64, device=dev)
    scratch = torch.empty(chains, dtype=torch.float64, device=dev)
    p = _lib.ptr

    def call(xs=x, xo=x_out, n=chains, dd=d, gr=groups, lw=logw, uu=u, an=anc, st=stats, sc=scratch):
        return lib.mf_smc_resample(p(xs), p(xo), n, dd, gr, p(lw), p(uu), 1.1, p(an), p(st), p(sc), ops.stream_ptr(x))

    for kwargs, word in ((dict(xo=x), "x_out"), (dict(gr=5), "multiple"), (dict(gr=0), "groups"), (dict(gr=-1), "groups"),
                         (dict(dd=9), "ndim"), (dict(dd=0), "ndim"), (dict(n=-3), "chain"), (dict(n=3 << 30), "chain"),
                         (dict(xs=None), "null"), (dict(xo=None), "null"), (dict(lw=None), "null"), (dict(uu=None), "null"),
                         (dict(an=None), "null"), (dict(st=None), "null"), (dict(sc=None), "null")):
        assert call(**kwargs) != 0, kwargs
        assert word in lib.mf_last_error().decode(), (kwargs, lib.mf_last_error().decode())
    assert torch.isnan(x_out).all() and torch.isnan(stats).all() and bool((anc == -1).all()), "a refused call writes nothing"
    assert same_bits(logw.cpu(), kept.cpu())
    assert call(n=0) == 0 and torch.isnan(stats).all(), "no chains: nothing to do"
    assert call() == 0 and not torch.isnan(x_out).any()
    # the wrapper's own checks
    with pytest.raises(RuntimeError, match="groups"):
        ops.smc_resample(x, logw, u[:2].contiguous(), 5, 0.5)
    with pytest.raises(RuntimeError, match="groups"):
        ops.smc_resample(x, logw, u, 0, 0.5)
    with pytest.raises(RuntimeError, match="logw"):
        ops.smc_resample(x, logw.float(), u, groups, 0.5)
    with pytest.raises(RuntimeError, match="logw"):
        ops.smc_resample(x, logw[:-1].contiguous(), u, groups, 0.5)
    with pytest.raises(RuntimeError, match="u must"):
        ops.smc_resample(x, logw, u.float(), groups, 0.5)
    with pytest.raises(RuntimeError, match="float32"):
        ops.smc_resample(x.double(), logw, u, groups, 0.5)
    with pytest.raises(RuntimeError, match="d <= 8"):
        ops.smc_resample(torch.zeros(chains, 9, device=dev), logw, u, groups, 0.5)
