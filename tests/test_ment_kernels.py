"""Classical MENT kernels (mentflow_amd/csrc/ment.hip) against the fp64 restatement in tests/_ment_fp64.py, on the emulator
here and on the MI355X with -m gpu (the `backend` fixture).

Gates.  A kernel factor is the fp32 interpolant at u = r . x: u carries ~d ulp of rounding, the weight (u - c_0) / delta a few
more, so one factor is within ~1e-6 relative of fp64 where the table is smooth; at a cell boundary of a table with zeros
the error is |dh/du| * du, still ~1e-6 of the table's range.  A product of <= 12 such factors (values <= 2) stays within 3e-5 of
the largest fp64 product: that is the gate.  Integrals sum fp32 products in fp64, so they meet the same relative gate."""
import math

import pytest
import torch

from _ment_fp64 import interp64, prob64
from mentflow_amd import ops
from mentflow_amd.ment import _slot_rows
from mentflow_amd.utils import coords_from_edges, get_grid_points


def make_slots(d, specs, gen, zeros=True, lo=0.0, hi=2.0):
    """specs: list of (ndim, bins) -> (fp64 slots, desc, meta, tables) with random rows and tables (some zeros)."""
    slots, desc, meta, tabs, off = [], [], [], [], 0
    for k, (nd, B) in enumerate(specs):
        rows = [torch.randn(d, generator=gen) for _ in range(nd)]
        rows = [r / r.norm() for r in rows]
        if k == 0:                                   # axis-aligned first slot: its projections are exact (hull tests)
            rows = [torch.eye(d)[a] for a in range(nd)]
        coords = [coords_from_edges(torch.linspace(-3.0 - 0.1 * k, 3.0 + 0.2 * a, B + 1)) for a in range(nd)]
        shape = [B] * nd
        values = lo + torch.rand(*shape, generator=gen) * (hi - lo)
        if zeros:
            values[torch.rand(*shape, generator=gen) < 0.2] = 0.0
        dsc, m = _slot_rows(rows, coords, d)
        desc.append(dsc)
        meta.append(m + [off])
        off += values.numel()
        tabs.append(values.reshape(-1))
        slots.append((rows, coords, values))
    return slots, torch.tensor(desc, dtype=torch.float32).reshape(-1, 24), torch.tensor(meta, dtype=torch.int32).reshape(-1, 4), \
        (torch.cat(tabs) if tabs else torch.zeros(1))


def special_points(d, slots, n, gen):
    """random points plus points whose first slot's projection sits exactly on c_0 / c_{B-1}, between the outer edge and
    the outer centre, far outside, and NaN rows."""
    x = torch.randn(n, d, generator=gen) * 1.5
    c = slots[0][1][0]
    e0 = float(c[0]) - 0.5 * float(c[1] - c[0])
    extra = torch.randn(4, d, generator=gen) * 0.3
    extra[:, 0] = torch.tensor([float(c[0]), float(c[-1]), 0.5 * (e0 + float(c[0])), 10.0])   # the first slot reads x[:, 0]
    x = torch.cat([x, extra, torch.full((2, d), float("nan"))])
    return x


def to(dev, *ts):
    return [t.to(dev) for t in ts]


PRIORS = [(0, 0.0, 0.0, None), (1, 1.7, -1.0, ("gaussian", 1.7))]


@pytest.mark.parametrize("d", [2, 3, 5, 8])
@pytest.mark.parametrize("kind", ["1d", "2d", "mixed"])
@pytest.mark.parametrize("with_prior", [False, True])
def test_prob_points_vs_fp64(backend, d, kind, with_prior):
    gen = torch.Generator().manual_seed(100 * d + len(kind) + with_prior)
    nslot = {"1d": 7, "2d": 3, "mixed": 5}[kind]
    specs = [(1 if (kind == "1d" or (kind == "mixed" and k % 2 == 0)) else 2, 9 + k) for k in range(nslot)]
    slots, desc, meta, tab = make_slots(d, specs, gen)
    x = special_points(d, slots, 600, gen)
    if with_prior:
        s = 1.7
        prior = (1, s, -d * (math.log(s) + 0.5 * math.log(2 * math.pi)))
        ref = prob64(x, slots, ("gaussian", s))
    else:
        prior = (0, 0.0, 0.0)
        ref = prob64(x, slots)
    xd, desc, meta, tab = to(backend, x, desc, meta, tab)
    got = ops.ment_prob(xd.contiguous(), desc, meta, tab, prior).cpu().double()
    nan = torch.isnan(ref)
    assert torch.equal(nan, torch.isnan(got)), "NaN rows must give NaN, and only they"
    assert nan.sum() == 2
    scale = ref[~nan].abs().max()
    assert float((got[~nan] - ref[~nan]).abs().max()) <= 3e-5 * float(scale) + 1e-30
    # points on c_0 / c_last of the first slot are inside (value kept), between edge and centre / far out give 0
    n0 = x.shape[0] - 6
    h_first = interp64(slots[0][1], slots[0][2], torch.stack([x[n0:n0 + 4] @ r for r in slots[0][0]], 1))
    assert h_first[2] == 0 and h_first[3] == 0
    assert got[n0 + 2] == 0 and got[n0 + 3] == 0


def test_prob_points_tables_beyond_lds_and_multiply(backend):
    """6 x 85^2 2-D tables (43 350 floats, more than the 24 576-float LDS budget): read from global memory.  Multiply mode
    multiplies into the output: prob(x; A) * prob(x; B) = prob(x; A + B)."""
    gen = torch.Generator().manual_seed(7)
    d = 4
    slots, desc, meta, tab = make_slots(d, [(2, 85)] * 6, gen, zeros=False)
    x = special_points(d, slots, 1500, gen)
    ref = prob64(x, slots)
    xd, dd, md, td = to(backend, x, desc, meta, tab)
    got = ops.ment_prob(xd.contiguous(), dd, md, td).cpu().double()
    nan = torch.isnan(ref)
    assert torch.equal(nan, torch.isnan(got))
    assert float((got[~nan] - ref[~nan]).abs().max()) <= 3e-5 * float(ref[~nan].abs().max())
    # split the six slots into two launches
    sa, da, ma, ta = make_slots(d, [(1, 20)] * 3, torch.Generator().manual_seed(8))
    sb, db, mb, tb = make_slots(d, [(2, 12)] * 2, torch.Generator().manual_seed(9))
    y = torch.randn(800, d, generator=gen)
    yd = y.to(backend)
    out = ops.ment_prob(yd, *to(backend, da, ma, ta))
    ops.ment_prob(yd, *to(backend, db, mb, tb), out=out, multiply=True)
    ref = prob64(y, sa + sb)
    assert float((out.cpu().double() - ref).abs().max()) <= 3e-5 * float(ref.abs().max())


def test_prob_points_hundred_slots(backend):
    """P = 100 slots (the C4 measurement set's count), 1-D and 2-D mixed, tables in [0.5, 1.5] so the product stays in range.
    Each factor carries ~2e-6 relative error (module docstring), 100 of them ~2e-4: gated at 3e-4 of the largest value."""
    gen = torch.Generator().manual_seed(100)
    d = 6
    slots, desc, meta, tab = make_slots(d, [(1 if k % 3 else 2, 12) for k in range(100)], gen, zeros=False, lo=0.5, hi=1.5)
    x = torch.randn(2000, d, generator=gen) * 0.4
    ref = prob64(x, slots)
    got = ops.ment_prob(x.to(backend), *to(backend, desc, meta, tab)).cpu().double()
    assert float(ref.max()) > 0
    assert float((got - ref).abs().max()) <= 3e-4 * float(ref.max())


@pytest.mark.parametrize("d", [2, 3, 4])
def test_prob_grid_matches_points(backend, d):
    """K2 (implicit grid) against K1 on the stored grid points; block sums are fp64 sums of prob + 1e-15."""
    gen = torch.Generator().manual_seed(11 + d)
    # d = 4: two 85^2 tables (14 450 floats), beyond the LDS budget: the global-memory instance
    specs = [(2, 85), (1, 10), (2, 85)] if d == 4 else [(1, 10), (2, 8), (1, 6)]
    slots, desc, meta, tab = make_slots(d, specs, gen)
    shape = {2: (37, 29), 3: (13, 11, 17), 4: (9, 8, 7, 6)}[d]
    coords = [coords_from_edges(torch.linspace(-3.2, 3.0, n + 1)) for n in shape]
    pts = get_grid_points(*coords)
    desc, meta, tab = to(backend, desc, meta, tab)
    prior = (1, 2.0, -d * (math.log(2.0) + 0.5 * math.log(2 * math.pi)))
    p1 = ops.ment_prob(pts.to(backend).contiguous(), desc, meta, tab, prior).cpu()
    p2, sums = ops.ment_prob_grid([c.to(backend) for c in coords], desc, meta, tab, prior)
    p2, sums = p2.cpu(), sums.cpu()
    assert torch.allclose(p1, p2, rtol=1e-6, atol=0.0)
    w = (p2 + 1e-15).double()
    nb = (w.numel() + 1023) // 1024
    ref = torch.stack([w[b * 1024:(b + 1) * 1024].sum() for b in range(nb)])
    assert torch.allclose(sums, ref, rtol=1e-12)
    assert float((p2.double() - prob64(pts, slots, ("gaussian", 2.0))).abs().max()) <= 3e-5 * float(p2.max())


@pytest.mark.parametrize("d,nd,res", [(2, 1, 40), (3, 1, 12), (3, 1, 70), (3, 2, 12), (4, 1, 7), (4, 2, 7), (4, 2, 6)])
def test_integrate_vs_fp64(backend, d, nd, res):
    """res 70 in 3-D: 4 900 points per bin, two 4 096-point chunks (the fixed-order pass over chunks); the last case reads
    two 85^2 tables from global memory."""
    gen = torch.Generator().manual_seed(31 * d + nd + res)
    specs = [(2, 85), (1, 9), (2, 85)] if res == 6 else [(1, 9), (2, 7), (1, 11)]
    slots, desc, meta, tab = make_slots(d, specs, gen, zeros=False)
    M = torch.linalg.qr(torch.randn(d, d, generator=gen))[0].float()
    minv = torch.linalg.inv(M)
    meas_axes = (0,) if nd == 1 else (2, 0) if d >= 3 else (0, 1)
    B = 6
    centres = coords_from_edges(torch.linspace(-2.5, 2.5, B + 1))
    axis_coords = [centres if a in meas_axes else torch.linspace(-3.0, 2.8, res) for a in range(d)]
    pred = ops.ment_integrate(minv, [c.to(backend) for c in axis_coords], meas_axes, *to(backend, desc, meta, tab)).cpu()
    int_axes = [a for a in range(d) if a not in meas_axes]
    bins = get_grid_points(*[axis_coords[a] for a in meas_axes])
    ints = get_grid_points(*[axis_coords[a] for a in int_axes])
    u = torch.zeros(bins.shape[0], ints.shape[0], d)
    for k, a in enumerate(meas_axes):
        u[:, :, a] = bins[:, k][:, None]
    for k, a in enumerate(int_axes):
        u[:, :, a] = ints[None, :, k]
    x = u.reshape(-1, d) @ minv.T
    ref = prob64(x, slots).reshape(bins.shape[0], -1).sum(1)
    assert pred.shape == (bins.shape[0],)
    assert float((pred.double() - ref).abs().max()) <= 3e-5 * float(ref.abs().max())


def cell_stats(backend, draws, noise):
    shape = (4, 5, 3)
    gen = torch.Generator().manual_seed(5)
    p = torch.rand(shape, generator=gen)
    p[1, 2, 0] = 0.0
    edges = [torch.linspace(-1.0, 2.0, s + 1) for s in shape]
    torch.manual_seed(0)
    pd = p.to(backend)
    x = ops.ment_sample(pd, list(shape), ops.ment_block_sums(pd), [e.to(backend) for e in edges], draws, noise).cpu()
    return p, edges, x


@pytest.mark.parametrize("noise", [False, True])
def test_sample_cell_frequencies(backend, noise):
    """Inverse-CDF draws on a 4x5x3 grid: every cell's frequency within 5 sigma of p; points inside their cell (noise: within
    half a cell of it)."""
    draws = 4_000_000 if backend.type == "cuda" else 120_000
    p, edges, x = cell_stats(backend, draws, noise)
    w = (p + 1e-15).double().reshape(-1)
    w = w / w.sum()
    assert x.shape == (draws, 3) and torch.isfinite(x).all()
    delta = torch.tensor([float(e[1] - e[0]) for e in edges])
    lo = torch.tensor([float(e[0]) for e in edges])
    if not noise:
        idx = torch.floor((x - lo) / delta).long()
        for a, s in enumerate(p.shape):
            idx[:, a] = idx[:, a].clamp(0, s - 1)
        flat = (idx[:, 0] * 5 + idx[:, 1]) * 3 + idx[:, 2]
        freq = torch.bincount(flat, minlength=60).double() / draws
        sigma = torch.sqrt(w * (1 - w) / draws)
        assert bool(((freq - w).abs() <= 5 * sigma + 1e-12).all())
        assert freq[(1 * 5 + 2) * 3 + 0] == 0
    else:
        hi = torch.tensor([float(e[-1]) for e in edges])
        assert bool((x >= lo - 0.5 * delta).all()) and bool((x <= hi + 0.5 * delta).all())
        # the noise spreads each axis by 0.5 U(-delta, delta): the spread of x - (cell centre) exceeds the cell
        idx = torch.floor((x - lo) / delta)
        assert bool(((idx < 0) | (idx >= torch.tensor(p.shape))).any())


def test_reproducible(backend):
    gen = torch.Generator().manual_seed(3)
    d = 4
    slots, desc, meta, tab = make_slots(d, [(1, 10), (2, 9)], gen)
    desc, meta, tab = to(backend, desc, meta, tab)
    x = torch.randn(3000, d, generator=gen).to(backend)
    assert torch.equal(ops.ment_prob(x, desc, meta, tab), ops.ment_prob(x, desc, meta, tab))
    coords = [coords_from_edges(torch.linspace(-3, 3, 9)).to(backend) for _ in range(d)]
    a, sa = ops.ment_prob_grid(coords, desc, meta, tab)
    b, sb = ops.ment_prob_grid(coords, desc, meta, tab)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    edges = [torch.linspace(-3, 3, 9).to(backend) for _ in range(d)]
    draws = []
    for _ in range(2):
        torch.manual_seed(42)
        draws.append(ops.ment_sample(a, [8] * d, sa, edges, 5000, True))
    assert torch.equal(draws[0], draws[1])
    minv = torch.eye(d)
    axis_coords = [coords[0]] + [torch.linspace(-3, 3, 7).to(backend)] * (d - 1)
    p1 = ops.ment_integrate(minv, axis_coords, (0,), desc, meta, tab)
    p2 = ops.ment_integrate(minv, axis_coords, (0,), desc, meta, tab)
    assert torch.equal(p1, p2)
