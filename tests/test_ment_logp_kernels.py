"""The log-density kernel of classical MENT (mentflow_amd/csrc/ment_logp.hip, ops.ment_logprob) against the fp64 restatement of
tests/_ment_logp_fp64.py, on the emulator here and on the MI355X with -m gpu (the `backend` fixture).

Gates (tests/_ment_logp_fp64.check_gates).  On points that are not ambiguous (no slot within 1e-4 of a bin centre in grid units,
see _ment_logp_fp64): |l - l64| <= 3e-4 (1 + |l64|) and max_j |g - g64| <= 3e-4 (1 + |g64|_inf).  3e-4 is the gate the project
already holds 100-factor products to (tests/test_ment_kernels.py): one factor carries ~2e-6 relative error from the fp32
projection and interpolation weight, a hundred of them 2e-4 in the sum of logs; the kernel's own arithmetic (one rounding per
factor of the running product, one logf) adds 6e-6.  Tables are uniform in [0.25, 2]: near a zero of a table log h amplifies
the error of the interpolation weight without bound, which is a property of the function, not of the kernel.  Ambiguous points
may hold no NaN and may be at most 1 % of the points with <= 8 slots, 4 % with 100 slots (each slot has B centres, a band of
2e-4 bin widths around each: ~2e-4 per slot and point)."""
import math

import pytest
import torch

from _ment_logp_fp64 import check_gates, logp64
from mentflow_amd import ops
from mentflow_amd.ment import _slot_rows
from mentflow_amd.utils import coords_from_edges

N = 4133


def make_slots(d, specs, gen, lo=0.25, hi=2.0, xmax=4.0):
    """specs: [(ndim, bins)] -> (fp64 slots, desc, meta, tables): random unit rows, centres of `bins` bins on [-xmax, xmax]."""
    slots, desc, meta, tabs, off = [], [], [], [], 0
    for nd, B in specs:
        rows = [torch.randn(d, generator=gen) for _ in range(nd)]
        rows = [r / r.norm() for r in rows]
        coords = [coords_from_edges(torch.linspace(-xmax, xmax, B + 1)) for _ in range(nd)]
        values = lo + torch.rand(*([B] * nd), generator=gen) * (hi - lo)
        dsc, m = _slot_rows(rows, coords, d)
        desc.append(dsc)
        meta.append(m + [off])
        off += values.numel()
        tabs.append(values.reshape(-1))
        slots.append((rows, coords, values))
    return slots, torch.tensor(desc, dtype=torch.float32).reshape(-1, 24), torch.tensor(meta, dtype=torch.int32).reshape(-1, 4), \
        (torch.cat(tabs) if tabs else torch.zeros(1))


def priors(d):
    s, a = 1.7, 2.5
    return {"none": ((0, 0.0, 0.0), None),
            "gaussian": ((1, s, -d * (math.log(s) + 0.5 * math.log(2 * math.pi))), ("gaussian", s)),
            "uniform": ((2, a, -d * math.log(2 * a)), ("uniform", a))}


def run(dev, x, desc, meta, tab, prior=(0, 0.0, 0.0), want_grad=True):
    return ops.ment_logprob(x.to(dev).contiguous(), desc.to(dev), meta.to(dev), tab.to(dev), prior, want_grad)


MIXED8 = [(1 if k % 2 == 0 else 2, 16 + (48 * k) // 7) for k in range(8)]        # B = 16 .. 64, tables fit in LDS
_cache = {}


def problem(name, d):
    """(x, slots, desc, meta, tables) and the fp64 reference per prior, computed once per shape."""
    if (name, d) not in _cache:
        gen = torch.Generator().manual_seed(31 * d + len(name))
        specs = {"mixed8": MIXED8, "hundred": [(1, 64)] * 100, "beyond_lds": [(2, 64)] * 3}[name]
        slots, desc, meta, tab = make_slots(d, specs, gen)
        x = 1.2 * torch.randn(N, d, generator=gen)
        _cache[(name, d)] = (x, slots, desc, meta, tab, {})
    return _cache[(name, d)]


def reference(name, d, prior_name):
    x, slots, desc, meta, tab, refs = problem(name, d)
    if prior_name not in refs:
        refs[prior_name] = logp64(x, slots, priors(d)[prior_name][1])
    return refs[prior_name]


@pytest.mark.parametrize("d", [1, 2, 6, 8])
@pytest.mark.parametrize("prior_name", ["none", "gaussian", "uniform"])
def test_value_and_gradient_vs_fp64(backend, d, prior_name):
    x, slots, desc, meta, tab, _ = problem("mixed8", d)
    assert desc.shape[0] * 28 + tab.numel() <= 10240, "this case is meant for the tables-in-LDS instance"
    ref, gref, amb = reference("mixed8", d, prior_name)
    lp, g = run(backend, x, desc, meta, tab, priors(d)[prior_name][0])
    check_gates(lp, g, ref, gref, amb, cap=0.01)


def test_hundred_slots(backend):
    """6-D, 100 1-D slots of 64 bins (the C4 measurement set): 9 200 floats, the tables-in-LDS instance."""
    d = 6
    x, slots, desc, meta, tab, _ = problem("hundred", d)
    ref, gref, amb = reference("hundred", d, "gaussian")
    lp, g = run(backend, x, desc, meta, tab, priors(d)["gaussian"][0])
    check_gates(lp, g, ref, gref, amb, cap=0.04)


def test_tables_beyond_lds(backend):
    """Three 64 x 64 slots, 12 288 floats: the tables are read from global memory."""
    d = 6
    x, slots, desc, meta, tab, _ = problem("beyond_lds", d)
    assert tab.numel() > 10240
    ref, gref, amb = reference("beyond_lds", d, "none")
    lp, g = run(backend, x, desc, meta, tab)
    check_gates(lp, g, ref, gref, amb, cap=0.01)


def test_stays_finite_where_the_product_leaves_fp32(backend):
    """100 factors of ~1e-3 (and of ~1e3): mf_ment_prob underflows to 0 (overflows to inf), logp is -690 (+690) within the gate."""
    d = 6
    gen = torch.Generator().manual_seed(5)
    for lo, hi in ((0.5e-3, 2e-3), (0.5e3, 2e3)):
        slots, desc, meta, tab = make_slots(d, [(1, 64)] * 100, gen, lo=lo, hi=hi)
        x = 0.8 * torch.randn(512, d, generator=gen)
        ref, gref, amb = logp64(x, slots)
        lp, g = run(backend, x, desc, meta, tab)
        prob = ops.ment_prob(x.to(backend), desc.to(backend), meta.to(backend), tab.to(backend)).cpu()
        inside = torch.isfinite(ref)
        assert inside.sum() > 400
        assert ((prob[inside] == 0) | torch.isinf(prob[inside])).all(), "the product is meant to leave fp32's range here"
        assert float(ref[inside].abs().min()) > 600
        check_gates(lp, g, ref, gref, amb, cap=0.04)


def test_support_pattern_is_that_of_the_product(backend):
    """Tables with whole cells of exact zeros (else >= 0.25): -inf exactly where mf_ment_prob returns 0, exp(logp) the product
    elsewhere, gradient rows of -inf points exactly 0."""
    for d in (2, 6):
        gen = torch.Generator().manual_seed(40 + d)
        slots, desc, meta, tab = make_slots(d, MIXED8, gen)
        tab = tab.clone()
        for nd, Bx, By, off in meta.tolist():           # zero the corners of ~4 % of the cells: whole cells of exact zeros
            t = tab[off:off + Bx * By].reshape(Bx, By)
            hit = torch.rand(Bx - 1, max(By - 1, 1), generator=gen) < 0.04
            for i, k in hit.nonzero().tolist():
                t[i:i + 2, k:k + 2] = 0.0
        x = 1.2 * torch.randn(N, d, generator=gen)
        for prior in (priors(d)["none"][0], priors(d)["uniform"][0]):
            lp, g = run(backend, x, desc, meta, tab, prior)
            prob = ops.ment_prob(x.to(backend), desc.to(backend), meta.to(backend), tab.to(backend), prior)
            dead = prob == 0
            assert 0.05 * N < int(dead.sum()) < 0.95 * N
            assert torch.equal(torch.isneginf(lp), dead)
            rel = (torch.exp(lp[~dead]) - prob[~dead]).abs() / prob[~dead]
            assert float(rel.max()) <= 1e-4
            assert (g[dead] == 0).all() and torch.isfinite(g).all()


def knot_problem(dev):
    """d = 1, row [1.0], centres -3.9375 + 0.125 k (all exactly representable, as is every product below)."""
    B = 64
    c = -3.9375 + 0.125 * torch.arange(B, dtype=torch.float32)
    t = 0.125 * torch.randint(2, 15, (B,), generator=torch.Generator().manual_seed(3)).float()   # multiples of 1/8: exact slopes
    desc, meta = _slot_rows([torch.ones(1)], [c], 1)
    return c, t, torch.tensor([desc]).to(dev), torch.tensor([meta + [0]], dtype=torch.int32).to(dev)


def test_knot_convention_in_exact_arithmetic(backend):
    c, t, desc, meta = knot_problem(backend)
    lp, g = ops.ment_logprob(c[:, None].to(backend).contiguous(), desc, meta, t.to(backend), want_grad=True)
    lp, g = lp.cpu(), g.cpu()[:, 0]
    assert float((lp - torch.log(t)).abs().max()) <= 5e-7, "h is exactly the table value at a centre; 4 ulp for the logarithm"
    slope = torch.empty(64)
    slope[:-1] = (t[1:] - t[:-1]) * 8.0                                    # right slope at interior centres
    slope[-1] = (t[-1] - t[-2]) * 8.0                                      # left slope at the last
    assert float((g - slope / t).abs().max()) <= 1e-6 * float((slope / t).abs().max())
    assert int((slope[:-2] != slope[1:-1]).sum()) > 40, "neighbouring cells must differ in slope for this to tell left from right"
    # one ulp outside either end
    out = torch.stack([torch.nextafter(c[0], torch.tensor(-10.0)), torch.nextafter(c[-1], torch.tensor(10.0))])[:, None]
    lp, g = ops.ment_logprob(out.to(backend).contiguous(), desc, meta, t.to(backend), want_grad=True)
    assert torch.isneginf(lp).all() and (g == 0).all()


def test_upper_clamp(backend):
    c, t, desc, meta = knot_problem(backend)
    t = t.clone()
    t[10:13] = 3.0e10
    x = torch.tensor([[float(c[10])], [float(c[11]) + 0.03], [float(c[12]) + 0.12], [float(c[20]) + 0.03]])
    lp, g = ops.ment_logprob(x.to(backend), desc, meta, t.to(backend), (1, 2.0, 0.0), want_grad=True)
    lp, g = lp.cpu(), g.cpu()
    prior = -0.5 * x[:, 0] ** 2 / 4.0
    assert float((lp[:2] - (math.log(1e10) + prior[:2])).abs().max()) <= 1e-5
    assert float((g[:2, 0] + x[:2, 0] / 4.0).abs().max()) <= 1e-6, "on the clamp only the prior pulls"
    h2 = 3.0e10 * 0.04 + float(t[13]) * 0.96                               # 1.2e9: below the clamp, a steep ordinary cell
    assert abs(float(lp[2]) - (math.log(h2) + float(prior[2]))) <= 1e-4
    assert float(g[2, 0]) < -1.0 and math.isfinite(float(g[3, 0]))


def test_nan_and_inf_rows(backend):
    d = 6
    x, slots, desc, meta, tab, _ = problem("mixed8", d)
    x = x[:600].clone()
    base_lp, base_g = run(backend, x, desc, meta, tab, priors(d)["gaussian"][0])
    y = x.clone()
    y[7, 2] = float("nan")
    y[300, 0] = float("inf")
    y[301, 5] = float("-inf")
    y[599] = float("nan")
    for prior in (priors(d)["gaussian"][0], priors(d)["none"][0]):
        lp, g = run(backend, y, desc, meta, tab, prior)
        prob = ops.ment_prob(y.to(backend), desc.to(backend), meta.to(backend), tab.to(backend), prior)
        assert torch.isnan(lp[7]) and torch.isnan(lp[599]) and torch.isnan(g[7]).all() and torch.isnan(g[599]).all()
        for r in (300, 301):                                                   # exactly as the product dictates
            assert bool(torch.isnan(lp[r])) == bool(torch.isnan(prob[r])) and bool(torch.isneginf(lp[r])) == bool(prob[r] == 0)
            assert torch.isnan(g[r]).all() if torch.isnan(lp[r]) else (g[r] == 0).all()
    lp, g = run(backend, y, desc, meta, tab, priors(d)["gaussian"][0])
    others = [r for r in range(600) if r not in (7, 300, 301, 599)]
    assert torch.equal(lp[others], base_lp[others]) and torch.equal(g[others], base_g[others])


def test_reproducible_splittable_and_grad_optional(backend):
    d = 6
    x, slots, desc, meta, tab, _ = problem("hundred", d)
    prior = priors(d)["gaussian"][0]
    lp, g = run(backend, x, desc, meta, tab, prior)
    lp2, g2 = run(backend, x, desc, meta, tab, prior)
    assert torch.equal(lp, lp2) and torch.equal(g, g2)
    k = 1000
    la, ga = run(backend, x[:k], desc, meta, tab, prior)
    lb, gb = run(backend, x[k:], desc, meta, tab, prior)
    assert torch.equal(torch.cat([la, lb]), lp) and torch.equal(torch.cat([ga, gb]), g)
    lv, none = run(backend, x, desc, meta, tab, prior, want_grad=False)
    assert none is None and torch.equal(lv, lp)
    x8, s8, d8, m8, t8, _ = problem("beyond_lds", d)
    lv, _ = run(backend, x8, d8, m8, t8, prior, want_grad=False)
    assert torch.equal(lv, run(backend, x8, d8, m8, t8, prior)[0])


def test_no_points_and_no_slots(backend):
    d = 3
    desc, meta, tab = torch.zeros(0, 24), torch.zeros(0, 4, dtype=torch.int32), torch.zeros(1)
    a = 1.3
    prior = (1, a, -0.7)
    lp, g = run(backend, torch.zeros(0, d), desc, meta, tab, prior)
    assert lp.shape == (0,) and g.shape == (0, d)
    x = torch.randn(300, d, generator=torch.Generator().manual_seed(1))
    lp, g = run(backend, x, desc, meta, tab, prior)
    ref = -0.7 - 0.5 * (x.double() ** 2).sum(1) / a ** 2
    assert float((lp.cpu().double() - ref).abs().max()) <= 1e-6 * float(1 + ref.abs().max())
    assert float((g.cpu().double() + x.double() / a ** 2).abs().max()) <= 1e-6 * float((x / a ** 2).abs().max())
    lp, g = run(backend, x, desc, meta, tab)
    assert (lp == 0).all() and (g == 0).all()


def test_argument_checks(backend):
    d = 2
    x, slots, desc, meta, tab, _ = problem("mixed8", d)
    dev = backend
    with pytest.raises(RuntimeError, match="float32"):
        ops.ment_logprob(x.double().to(dev), desc.to(dev), meta.to(dev), tab.to(dev))
    with pytest.raises(RuntimeError, match="d <= 8"):
        ops.ment_logprob(torch.zeros(4, 9, device=dev), desc.to(dev), meta.to(dev), tab.to(dev))
    with pytest.raises(RuntimeError, match="meta"):
        ops.ment_logprob(x.to(dev), desc.to(dev), meta.long().to(dev), tab.to(dev))
