"""Classical MENT kernels (mentflow_amd/csrc/ment.hip) against the fp64 restatement in tests/_ment_fp64.py, on the emulator
here and on the MI355X with -m gpu (the `backend` fixture).

Gates.  A kernel factor is the fp32 interpolant at u = r . x: u carries ~d ulp of rounding, the weight (u - c_0) / delta a few
more, so one factor is within ~1e-6 relative of fp64 where the table is smooth; at a cell boundary of a table with zeros
the error is |dh/du| * du, still ~1e-6 of the table's range.  A product of <= 12 such factors (values <= 2) stays within 3e-5 of
the largest fp64 product: that is the gate.  Integrals sum fp32 products in fp64, so they meet the same relative gate."""
import math

import pytest
import torch

from _ment_fp64 import cdf64, interp64, place64, prob64, sample64
from mentflow_amd import ops
from mentflow_amd.ment import _slot_rows
from mentflow_amd.utils import coords_from_edges, get_grid_points


def make_slots(d, specs, gen, zeros=True, lo=0.0, hi=2.0, shift=0.1):
    """specs: list of (ndim, bins) -> (fp64 slots, desc, meta, tables) with random rows and tables (some zeros).  Slot k's
    grids start at -3 - shift * k, so with hundreds of slots the hull [c_0, c_{B-1}] of the later ones leaves the test points
    behind: shift=0 keeps every slot's hull over |u| <= 3 - 3 / B."""
    slots, desc, meta, tabs, off = [], [], [], [], 0
    for k, (nd, B) in enumerate(specs):
        rows = [torch.randn(d, generator=gen) for _ in range(nd)]
        rows = [r / r.norm() for r in rows]
        if k == 0:                                   # axis-aligned first slot: its projections are exact (hull tests)
            rows = [torch.eye(d)[a] for a in range(nd)]
        coords = [coords_from_edges(torch.linspace(-3.0 - shift * k, 3.0 + 0.2 * a, B + 1)) for a in range(nd)]
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


def gaussian_prior(d, s):
    return (1, s, -d * (math.log(s) + 0.5 * math.log(2 * math.pi))), ("gaussian", s)


def uniform_prior(d, a):
    """(kernel triple, prob64's prior) of the uniform density on [-a, a]^d."""
    return (2, a, -d * math.log(2 * a)), ("uniform", a)


def priors(d, s, a):
    return [("none", (0, 0.0, 0.0), None), ("gaussian",) + gaussian_prior(d, s), ("uniform",) + uniform_prior(d, a)]


def report(what, err, gate):
    """every fp64 comparison prints its figure beside its gate (pytest -s shows them)"""
    print(f"[ment fp64] {what}: max error {err:.3e}, gate {gate:.3e}")


def nonzero_share(ref, least):
    """a test must not pass on zeros: at least `least` of the finite reference values are positive"""
    ref = ref[~torch.isnan(ref)]
    share = float((ref > 0).double().mean())
    assert share >= least, f"only {share:.3f} of the reference values are non-zero"
    return share


@pytest.mark.parametrize("d", [2, 3, 5, 8])
@pytest.mark.parametrize("kind", ["1d", "2d", "mixed"])
@pytest.mark.parametrize("with_prior", [False, True, "uniform"])
def test_prob_points_vs_fp64(backend, d, kind, with_prior):
    """with_prior "uniform": the box [-1.5, 1.5]^d through prob_point; the first 2 d points have one coordinate exactly on
    -a or +a (inside: the box is closed), the rest of each such point well inside."""
    gen = torch.Generator().manual_seed(100 * d + len(kind) + (2 if with_prior == "uniform" else int(with_prior)))
    nslot = {"1d": 7, "2d": 3, "mixed": 5}[kind]
    specs = [(1 if (kind == "1d" or (kind == "mixed" and k % 2 == 0)) else 2, 9 + k) for k in range(nslot)]
    slots, desc, meta, tab = make_slots(d, specs, gen)
    x = special_points(d, slots, 600, gen)
    if with_prior == "uniform":
        a = 1.5
        x[:2 * d] = x[:2 * d].clamp(-0.6, 0.6)
        for j in range(d):
            x[2 * j, j], x[2 * j + 1, j] = -a, a
        kprior, prior64 = uniform_prior(d, a)
        ref = prob64(x, slots, prior64)
        on_edge = ref[:2 * d]
        assert int((on_edge > 0).sum()) >= d // 2, "points on the box's faces must count as inside"
        inside = (x[:600].abs() <= a).all(1)
        assert 0.02 < float(inside.float().mean()) < 0.98, "both branches of the box"
    elif with_prior:
        s = 1.7
        kprior = (1, s, -d * (math.log(s) + 0.5 * math.log(2 * math.pi)))
        ref = prob64(x, slots, ("gaussian", s))
    else:
        kprior = (0, 0.0, 0.0)
        ref = prob64(x, slots)
    xd, desc, meta, tab = to(backend, x, desc, meta, tab)
    got = ops.ment_prob(xd.contiguous(), desc, meta, tab, kprior).cpu().double()
    nan = torch.isnan(ref)
    assert torch.equal(nan, torch.isnan(got)), "NaN rows must give NaN, and only they"
    assert nan.sum() == 2
    scale = ref[~nan].abs().max()
    nonzero_share(ref, 0.02)
    report(f"prob_points d={d} {kind} prior={with_prior}", float((got[~nan] - ref[~nan]).abs().max()), 3e-5 * float(scale))
    assert float((got[~nan] - ref[~nan]).abs().max()) <= 3e-5 * float(scale) + 1e-30
    if with_prior == "uniform":
        assert torch.equal(got[:2 * d] > 0, on_edge > 0)
    # points on c_0 / c_last of the first slot are inside (value kept), between edge and centre / far out give 0
    n0 = x.shape[0] - 6
    h_first = interp64(slots[0][1], slots[0][2], torch.stack([x[n0:n0 + 4] @ r for r in slots[0][0]], 1))
    assert h_first[2] == 0 and h_first[3] == 0
    assert got[n0 + 2] == 0 and got[n0 + 3] == 0


def test_prob_points_tables_beyond_lds_and_multiply(backend):
    """6 x 85^2 2-D tables (43 350 floats, more than the 10 240 floats that descriptors and tables may take in LDS together):
    read from global memory.  Multiply mode multiplies into the output: prob(x; A) * prob(x; B) = prob(x; A + B)."""
    gen = torch.Generator().manual_seed(7)
    d = 4
    slots, desc, meta, tab = make_slots(d, [(2, 85)] * 6, gen, zeros=False)
    x = special_points(d, slots, 1500, gen)
    ref = prob64(x, slots)
    xd, dd, md, td = to(backend, x, desc, meta, tab)
    got = ops.ment_prob(xd.contiguous(), dd, md, td).cpu().double()
    nan = torch.isnan(ref)
    assert torch.equal(nan, torch.isnan(got))
    nonzero_share(ref, 0.25)
    assert float((got[~nan] - ref[~nan]).abs().max()) <= 3e-5 * float(ref[~nan].abs().max())
    # split the six slots into two launches
    sa, da, ma, ta = make_slots(d, [(1, 20)] * 3, torch.Generator().manual_seed(8))
    sb, db, mb, tb = make_slots(d, [(2, 12)] * 2, torch.Generator().manual_seed(9))
    y = torch.randn(800, d, generator=gen)
    yd = y.to(backend)
    out = ops.ment_prob(yd, *to(backend, da, ma, ta))
    ops.ment_prob(yd, *to(backend, db, mb, tb), out=out, multiply=True)
    ref = prob64(y, sa + sb)
    nonzero_share(ref, 0.25)
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
    nonzero_share(ref, 0.25)
    assert float((got - ref).abs().max()) <= 3e-4 * float(ref.max())


GRID_SHAPES = {2: (37, 29), 3: (13, 11, 17), 4: (9, 8, 7, 6), 5: (3, 4, 2, 5, 3), 6: (3, 2, 4, 3, 2, 5), 7: (2, 3, 2, 3, 2, 3, 4),
               8: (2, 3, 2, 2, 3, 2, 2, 3), "1x1024x1": (1, 1024, 1), "32x1x32x1": (32, 1, 32, 1), "1x1": (1, 1)}


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7, 8, "1x1024x1", "32x1x32x1", "1x1"])
def test_prob_grid_matches_points(backend, d):
    """K2 (implicit grid) against K1 on the stored grid points and against fp64; block sums are fp64 sums of prob + 1e-15.
    Up to MENT_DMAX = 8 axes, axes of one cell, 1 024 cells = exactly one block, a single cell; each with no prior, the
    Gaussian and the uniform prior (half-width 1.7 inside the grid's [-3.2, 3.0]: cells on either side of the box).  From
    five axes on the grid is coarse and narrower, so that its corners stay in the hulls of the slots."""
    shape, key = GRID_SHAPES[d], d
    d = len(shape)
    gen = torch.Generator().manual_seed(11 + (key if isinstance(key, int) else sum(shape)))
    # d = 4: two 85^2 tables (14 450 floats), beyond the LDS budget: the global-memory instance
    specs = [(2, 85), (1, 10), (2, 85)] if shape == GRID_SHAPES[4] else [(1, 10), (2, 8), (1, 6)]
    slots, desc, meta, tab = make_slots(d, specs, gen)
    lo, hi, a = (-3.2, 3.0, 1.7) if d <= 4 else (-1.6, 1.5, 0.8)
    coords = [coords_from_edges(torch.linspace(lo, hi, n + 1)) for n in shape]
    pts = get_grid_points(*coords)
    desc, meta, tab = to(backend, desc, meta, tab)
    assert nonzero_share(prob64(pts, slots), 0.2 if pts.shape[0] > 1 else 1.0)
    for name, prior, prior64 in priors(d, 2.0, a):
        p1 = ops.ment_prob(pts.to(backend).contiguous(), desc, meta, tab, prior).cpu()
        p2, sums = ops.ment_prob_grid([c.to(backend) for c in coords], desc, meta, tab, prior)
        p2, sums = p2.cpu(), sums.cpu()
        assert torch.allclose(p1, p2, rtol=1e-6, atol=0.0)
        w = (p2 + 1e-15).double()
        nb = (w.numel() + 1023) // 1024
        assert sums.numel() == nb
        ref = torch.stack([w[b * 1024:(b + 1) * 1024].sum() for b in range(nb)])
        assert torch.allclose(sums, ref, rtol=1e-12)
        ref = prob64(pts, slots, prior64)
        if name == "uniform" and pts.shape[0] > 1:
            inside = (pts.abs() <= a).all(1)
            assert inside.any() and not inside.all(), "both branches of the box"
            assert bool((p2[~inside] == 0).all())
        err = float((p2.double() - ref).abs().max())
        report(f"prob_grid {tuple(shape)} prior={name}", err, 3e-5 * float(ref.max()))
        assert float(ref.max()) > 0 and err <= 3e-5 * float(ref.max())


def integrate64(minv, axis_coords, meas_axes, slots, prior64=None):
    """fp64 line / plane integrals: the bins in ij order of meas_axes as given, the other axes ascending -> (ref[nbins], the
    share of non-zero integrand values)."""
    d = len(axis_coords)
    int_axes = [a for a in range(d) if a not in meas_axes]
    bins = get_grid_points(*[axis_coords[a] for a in meas_axes])
    ints = get_grid_points(*[axis_coords[a] for a in int_axes]) if int_axes else torch.zeros(1, 0)
    u = torch.zeros(bins.shape[0], ints.shape[0], d)
    for k, a in enumerate(meas_axes):
        u[:, :, a] = bins[:, k][:, None]
    for k, a in enumerate(int_axes):
        u[:, :, a] = ints[None, :, k]
    x = u.reshape(-1, d) @ minv.T
    p = prob64(x, slots, prior64)
    return p.reshape(bins.shape[0], -1).sum(1), float((p > 0).double().mean())


# beyond four axes: (d, measured axes in the order given, bins per measured axis, points per integrated axis in ascending
# axis order).  The lengths differ from axis to axis, so a swapped stride or a permuted axis changes the sums.
INTEGRATE_WIDE = {
    "5-m3": (5, (3,), (6,), (3, 4, 5, 4)),
    "6-m0": (6, (0,), (6,), (3, 4, 5, 3, 4)),                 # the C4 shape: one measured axis of six
    "6-m52": (6, (5, 2), (6, 4), (3, 4, 5, 3)),               # descending, 6 x 4 bins
    "7-m6": (7, (6,), (6,), (3, 4, 5, 3, 4, 5)),
    "8-m70": (8, (7, 0), (6, 4), (3, 4, 5, 3, 4, 5)),
    "8-m3": (8, (3,), (6,), (3, 4, 3, 5, 3, 3, 3)),           # 4 860 points per bin: two chunks
    "2-m10": (2, (1, 0), (6, 4), ()),                         # no integrated axis: one point per bin
    "1-m0": (1, (0,), (6,), ()),
}


@pytest.mark.parametrize("d,nd,res", [(2, 1, 40), (3, 1, 12), (3, 1, 70), (3, 2, 12), (4, 1, 7), (4, 2, 7), (4, 2, 6)]
                         + [pytest.param(None, k, None, id=k) for k in INTEGRATE_WIDE])
def test_integrate_vs_fp64(backend, d, nd, res):
    """res 70 in 3-D: 4 900 points per bin, two 4 096-point chunks (the fixed-order pass over chunks); (4, 2, 6) reads
    two 85^2 tables from global memory.  The named cases are those of INTEGRATE_WIDE.  Each runs without a prior and with
    the uniform prior, whose box cuts through the points."""
    if d is None:
        d, meas_axes, nbins, lens = INTEGRATE_WIDE[nd]
        gen = torch.Generator().manual_seed(31 * d + 7 * len(meas_axes) + sum(lens))
        lens = list(lens)
        half = a = 3.0 / math.sqrt(d)                         # |x| = |u| <= 3: about the hull of every slot
        axis_coords = [coords_from_edges(torch.linspace(-half, half, nbins[meas_axes.index(ax)] + 1)) if ax in meas_axes
                       else torch.linspace(-half, 0.9 * half, lens.pop(0)) for ax in range(d)]
        specs = [(1, 9), (2, 7), (1, 11)]
    else:
        gen = torch.Generator().manual_seed(31 * d + nd + res)
        specs = [(2, 85), (1, 9), (2, 85)] if res == 6 else [(1, 9), (2, 7), (1, 11)]
        meas_axes = (0,) if nd == 1 else (2, 0) if d >= 3 else (0, 1)
        centres = coords_from_edges(torch.linspace(-2.5, 2.5, 6 + 1))
        axis_coords = [centres if ax in meas_axes else torch.linspace(-3.0, 2.8, res) for ax in range(d)]
        a = 1.9
    slots, desc, meta, tab = make_slots(d, specs, gen, zeros=False)
    M = torch.linalg.qr(torch.randn(d, d, generator=gen))[0].float()
    minv = torch.linalg.inv(M)
    nb = math.prod(axis_coords[ax].numel() for ax in meas_axes)
    for name, prior, prior64 in priors(d, 2.0, a)[::2]:
        pred = ops.ment_integrate(minv, [c.to(backend) for c in axis_coords], meas_axes, *to(backend, desc, meta, tab), prior).cpu()
        ref, share = integrate64(minv, axis_coords, meas_axes, slots, prior64)
        assert share >= 0.05, f"only {share:.3f} of the integrand values are non-zero"
        assert pred.shape == (nb,)
        err = float((pred.double() - ref).abs().max())
        report(f"integrate d={d} measured={tuple(meas_axes)} prior={name}", err, 3e-5 * float(ref.abs().max()))
        assert err <= 3e-5 * float(ref.abs().max())


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


# ------------------------------------------------------------------------------------------------ the sampler, draw by draw
# ops.ment_sample takes its uniforms, so every draw has one right answer.  The kernel sums the fp64 weights in another order
# than a cumulative sum (a tree per 1 024-cell block, then the blocks in sequence): the two CDFs differ by at most
# n * 2^-53 ~ 1.2e-10 of the total for n <= 2^20 cells.  A draw whose target lies within AMBIGUOUS * total of an end of its
# cell's CDF interval is ambiguous: it may fall in a cell whose interval reaches into that band around the target, and in no
# other (between cells wider than the band that is the neighbour; cells of zero weight are 1e-15 wide and a run of them may be
# stepped over).  Every other draw must land in the fp64 cell.  The point is gated at 4 * 2^-24 of the axis's largest |edge|:
# three fp32 roundings, and the GPU build's contraction of lb + (ub - lb) * r into an FMA.
AMBIGUOUS = 1e-10
AMBIGUOUS_SHARE = 1e-3        # a condition on the test's grids, not a measurement: see test_sample_matches_fp64_inverse_cdf


def check_draws(what, p, shape, edges, rnd, noise, x):
    """x[size, d] from the kernel against sample64 -> (cell64, ambiguous mask)."""
    cell, x64, gap, total = sample64(p, shape, edges, rnd, noise)
    assert x.shape == x64.shape and bool(torch.isfinite(x).all())
    gate = torch.tensor([4 * 2.0 ** -24 * float(e.abs().max()) for e in edges], dtype=torch.float64)
    amb = gap <= AMBIGUOUS * total
    share = float(amb.double().mean())
    err = (x.double() - x64.double()).abs() / gate
    sure = err[~amb].max()
    print(f"[ment fp64] {what} noise={noise}: largest |x - x64| = {float(sure):.3f} of its gate 4 * 2^-24 * max|edge|, "
          f"ambiguous draws {int(amb.sum())} of {amb.numel()} = {share:.2e} (cap {AMBIGUOUS_SHARE:.0e})")
    assert share <= AMBIGUOUS_SHARE
    wrong = (~amb & (err > 1).any(1)).nonzero().reshape(-1)
    assert wrong.numel() == 0, f"{wrong.numel()} draws off the fp64 cell, first: draw {int(wrong[0])}, cell {int(cell[wrong[0]])}"
    cdf = cdf64(p)
    for i in amb.nonzero().reshape(-1).tolist():
        target = rnd[i, 0].double() * total
        band = torch.stack([target - AMBIGUOUS * total, target + AMBIGUOUS * total])
        first, last = torch.searchsorted(cdf, band, right=True).clamp(max=cdf.numel() - 1).tolist()   # the cells of the band's ends
        cand = torch.arange(first, last + 1)
        xc = place64(cand, shape, edges, rnd[i:i + 1].expand(cand.numel(), -1), noise)
        hit = ((x[i].double() - xc.double()).abs() <= gate).all(1)
        assert bool(hit.any()), f"ambiguous draw {i} is in none of the cells {first}..{last} around its target"
    return cell, amb


SAMPLE_GRIDS = [(4, 5, 3), (37, 29), (1024,), (1025,), (13, 11, 17, 5), (3, 2, 5, 2, 3, 2, 3, 2), (7, 1, 9, 1, 11), (1100, 1024)]


@pytest.mark.parametrize("shape", SAMPLE_GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_sample_matches_fp64_inverse_cdf(backend, shape):
    """Every one of 20 000 draws against the fp64 inverse CDF, with and without noise: one block, a ragged second block,
    exactly one block and one cell more, 12 blocks, eight axes, axes of one cell with 90 % empty cells, and 1 100 blocks
    (more than the 1 024 scan threads: each owns two) of values over six decades.  30 % of the cells are exactly zero;
    above 4 096 cells so are the whole blocks [1024, 3072), whose prefix entries collide.  Every axis has its own edges, so
    a permuted axis shows.  Draw 0 has rnd = 0 and lands in cell 0 although p[0] = 0 (its weight is 1e-15, not 0: the
    documented behaviour of ops.ment_sample); draw 1 has the largest fp32 uniform, 1 - 2^-24, and lands in a cell with p > 0.
    AMBIGUOUS_SHARE: the planted rnd = 0 draw is always ambiguous (1 / 20 000 = 5e-5); a random one is with probability
    2 * 1e-10 * ncells, 2.3e-4 at the largest grid."""
    n = math.prod(shape)
    gen = torch.Generator().manual_seed(1000 + n)
    p = 10.0 ** (-6.0 * torch.rand(n, generator=gen)) if n > 100_000 else torch.rand(n, generator=gen)
    p[torch.rand(n, generator=gen) < (0.9 if 1 in shape else 0.3)] = 0.0
    if n > 4096:
        p[1024:3072] = 0.0
    p[0] = 0.0
    edges = [torch.linspace(-1.0, 2.0 + ax, s + 1) for ax, s in enumerate(shape)]
    size, d = 20_000, len(shape)
    rnd = torch.rand(size, 1 + 2 * d, generator=gen)
    rnd[0, 0], rnd[1, 0] = 0.0, 1.0 - 2.0 ** -24
    pd = p.to(backend)
    sums = ops.ment_block_sums(pd)
    for noise in (False, True):
        x = ops.ment_sample(pd, list(shape), sums, [e.to(backend) for e in edges], size, noise, rnd=rnd.to(backend)).cpu()
        cell, amb = check_draws("x".join(map(str, shape)), p, shape, edges, rnd, noise, x)
        gate = torch.tensor([4 * 2.0 ** -24 * float(e.abs().max()) for e in edges], dtype=torch.float64)
        x0 = place64(torch.zeros(1, dtype=torch.long), shape, edges, rnd[:1], noise)
        assert bool(((x[0].double() - x0[0].double()).abs() <= gate).all()), "rnd = 0 lands in cell 0"
        assert not bool(amb[1]) and float(p[cell[1]]) > 0.0, "rnd = 1 - 2^-24 lands in a cell with p > 0"
        assert int((p[cell] == 0).sum()) <= 1, "cells of zero weight are drawn with probability ~1e-15 each"


def test_sample_exact_ties(backend):
    """Targets exactly on the ends of the CDF intervals.  Weights 1, 2 or 3 (p + 1e-15 is p in fp32) that sum to 8 192 over
    4 096 cells: every partial sum is a small integer, exact in fp64 in any order, and rnd = cdf / 8192 is exact in fp32, so
    no draw is ambiguous.  A target on the boundary between two cells belongs to the upper one (searchsorted right=True; the
    block search's prefix[b] <= target, the cell scan's target < run), also where the boundary is a block's: draws 1 024,
    2 048 and 3 072."""
    n, total = 4096, 8192
    gen = torch.Generator().manual_seed(79)
    p = torch.randint(1, 4, (n,), generator=gen).float()
    c = 0
    while int(p.sum()) != total:                    # walk the cells, nudging one at a time, until the sum is 2^13
        step = 1.0 if p.sum() < total else -1.0
        if 1.0 <= float(p[c]) + step <= 3.0:
            p[c] += step
        c = (c + 7) % n
    cdf = cdf64(p)
    assert float(cdf[-1]) == total and bool((cdf == cdf.round()).all())
    edges = [torch.linspace(-1.0, 2.0, n + 1)]
    rnd = torch.rand(n, 3, generator=gen)
    rnd[1:, 0] = (cdf[:-1] / total).float()          # the lower end of cell i's interval = the upper end of cell i - 1's
    rnd[0, 0] = 0.0
    assert bool((rnd[:, 0].double() * total == torch.cat([torch.zeros(1, dtype=torch.float64), cdf[:-1]])).all())
    pd = p.to(backend)
    x = ops.ment_sample(pd, [n], ops.ment_block_sums(pd), [edges[0].to(backend)], n, False, rnd=rnd.to(backend)).cpu()
    x64 = place64(torch.arange(n), (n,), edges, rnd, False)
    off = ((x.double() - x64.double()).abs() > 4 * 2.0 ** -24 * 2.0).reshape(-1).nonzero().reshape(-1)
    assert off.numel() == 0, f"{off.numel()} boundary targets off their cell, first: {int(off[0])}"


def test_sample_grid_stride(backend):
    """1 048 576 + 300 draws: more than the 4 096 workgroups x 256 lanes of the launch, so the last 300 come from a second
    trip of the kernel's grid-stride loop.  Every draw against fp64."""
    shape, size = (2000,), 4096 * 256 + 300
    gen = torch.Generator().manual_seed(77)
    p = torch.rand(shape[0], generator=gen)
    p[torch.rand(shape[0], generator=gen) < 0.3] = 0.0
    edges = [torch.linspace(-1.0, 2.0, shape[0] + 1)]
    rnd = torch.rand(size, 3, generator=gen)
    pd = p.to(backend)
    x = ops.ment_sample(pd, list(shape), ops.ment_block_sums(pd), [edges[0].to(backend)], size, True, rnd=rnd.to(backend)).cpu()
    check_draws("grid stride", p, shape, edges, rnd, True, x)


# ------------------------------------------------------------------------------------------------ K1, K2 and K4 on one slot set
def check_three_kernels(backend, what, d, slots, desc, meta, tab, half, gate=3e-5, least=0.25, prior_list=None):
    """K1 on random points, K2 on a small grid and K4 on a small integral, all within [-half, half] per axis, each against
    fp64 at `gate` of the largest reference value and with at least `least` of the reference values non-zero."""
    gen = torch.Generator().manual_seed(5 + d)
    dev = to(backend, desc, meta, tab)
    x = (torch.rand(1500, d, generator=gen) * 2 - 1) * half
    shape = [5, 4, 3, 3, 2, 3, 2, 3][:d]
    coords = [coords_from_edges(torch.linspace(-half, 0.9 * half, n + 1)) for n in shape]
    pts = get_grid_points(*coords)
    M = torch.linalg.qr(torch.randn(d, d, generator=gen))[0].float()
    minv = torch.linalg.inv(M)
    axis_coords = [torch.linspace(-half, 0.9 * half, 5 if ax == d - 1 else 3 + ax % 2) / math.sqrt(d) for ax in range(d)]
    for name, prior, prior64 in (prior_list or priors(d, 2.0, 0.6 * half)[:1]):
        ref = prob64(x, slots, prior64)
        got = ops.ment_prob(x.to(backend), *dev, prior).cpu().double()
        nonzero_share(ref, least)
        report(f"{what} K1 prior={name}", float((got - ref).abs().max()), gate * float(ref.max()))
        assert float((got - ref).abs().max()) <= gate * float(ref.max())
        ref = prob64(pts, slots, prior64)
        got = ops.ment_prob_grid([c.to(backend) for c in coords], *dev, prior)[0].cpu().double()
        nonzero_share(ref, least / 4)
        report(f"{what} K2 prior={name}", float((got - ref).abs().max()), gate * float(ref.max()))
        assert float((got - ref).abs().max()) <= gate * float(ref.max())
        ref, share = integrate64(minv, axis_coords, (d - 1,), slots, prior64)
        got = ops.ment_integrate(minv, [c.to(backend) for c in axis_coords], (d - 1,), *dev, prior).cpu().double()
        assert share >= least / 4
        report(f"{what} K4 prior={name}", float((got - ref).abs().max()), gate * float(ref.max()))
        assert float((got - ref).abs().max()) <= gate * float(ref.max())


@pytest.mark.parametrize("last_bins", [36, 37])
def test_table_placement_boundary(backend, last_bins):
    """Descriptors and tables share LDS while 28 * nslot + table_floats <= 10 240 floats (24 + 4 per slot, ment_slots.h):
    three 58 x 58 tables and one of 36 bins with four slots make exactly 10 240, the last set that runs from LDS; 37 bins
    make 10 241, the first that reads its tables from global memory.  Both against fp64 through K1, K2 and K4.  (Tables of
    ~0.1-wide cells, as elsewhere in this file: the module's gate assumes that an fp32 u moves the weight by ~1e-6.)"""
    gen = torch.Generator().manual_seed(last_bins)
    specs = [(2, 58)] * 3 + [(1, last_bins)]
    slots, desc, meta, tab = make_slots(3, specs, gen)
    assert 28 * len(specs) + tab.numel() == 10240 + (last_bins - 36)
    check_three_kernels(backend, f"placement {28 * len(specs) + tab.numel()}", 3, slots, desc, meta, tab, half=2.0)


def test_slot_count_limits(backend):
    """No slot at all: the density is the prior alone.  MENT_MAX_SLOTS = 512 slots (14 336 descriptor floats, 57 KB of
    dynamic LDS) of 4 bins with tables in [0.97, 1.03]: the module's gate allows 3e-5 for 12 factors, 2.5e-6 per factor, so
    512 factors are gated at 3e-5 * 512 / 12 = 1.28e-3 of the largest value.  513 slots are refused by name."""
    gen = torch.Generator().manual_seed(512)
    d = 6
    slots, desc, meta, tab = make_slots(d, [], gen)
    assert desc.shape == (0, 24) and meta.shape == (0, 4)
    check_three_kernels(backend, "no slot", d, slots, desc, meta, tab, half=1.0, least=0.4, prior_list=priors(d, 0.8, 0.9))
    x = torch.randn(300, d, generator=gen)
    slots, desc, meta, tab = make_slots(d, [(1, 4)] * 512, gen, zeros=False, lo=0.97, hi=1.03, shift=0.0)
    check_three_kernels(backend, "512 slots", d, slots, desc, meta, tab, half=0.8, gate=3e-5 * 512 / 12, least=0.9)
    slots, desc, meta, tab = make_slots(d, [(1, 4)] * 513, gen, zeros=False, shift=0.0)
    with pytest.raises(RuntimeError, match=r"MENT kernels take 0\.\.512 slots per launch \(got 513\)"):
        ops.ment_prob(x.to(backend), *to(backend, desc, meta, tab))


def test_prob_points_grid_stride(backend):
    """1 048 576 + 300 points: more than the 4 096 workgroups x 256 lanes of the launch, so the last 300 come from a second
    trip of K1's grid-stride loop.  The whole output against fp64."""
    gen = torch.Generator().manual_seed(78)
    d, n = 3, 4096 * 256 + 300
    slots, desc, meta, tab = make_slots(d, [(1, 12), (2, 9)], gen)
    x = torch.randn(n, d, generator=gen)
    ref = prob64(x, slots)
    nonzero_share(ref, 0.25)
    assert float(ref[-300:].max()) > 0
    got = ops.ment_prob(x.to(backend), *to(backend, desc, meta, tab)).cpu().double()
    report("prob_points grid stride", float((got - ref).abs().max()), 3e-5 * float(ref.max()))
    assert float((got - ref).abs().max()) <= 3e-5 * float(ref.max())
