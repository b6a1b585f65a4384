"""Kernels of the differentiable sliced Wasserstein distance (mentflow_amd/csrc/swd.hip: pair sort, adjoint of the quantile
cost, back-projection, and ops.SlicedWassersteinFn over them) against torch.sort and the fp64 gradient written out in
tests/_swd_grad_fp64.py: emulator here (64-key tile override, so that a few thousand keys go through six merge passes), the
MI355X with -m gpu (default tile).  Bounds: see each test; none is fitted to what the kernels return."""
import numpy as np
import pytest
import torch

import _swd_fp64 as ref
import _swd_grad_fp64 as gref
from mentflow_amd import ops
from test_swd_kernels import clouds, make_keys, tile_of


# ------------------------------------------------------------------------------------------------ the oracle itself
ORACLE_CASES = [(300, 300, 2.0), (257, 100, 1.0), (100, 457, 3.0), (5, 3, 2.0), (2, 97, 2.0)]


def oracle_inputs(n, m, P=3):
    rng = np.random.default_rng(n * 13 + m)
    return rng.normal(size=(P, n)), 0.4 + 1.3 * rng.normal(size=(P, m))


def torch_dist(u, v, p):
    """The composed formula in torch fp64: sort(stable) + gather over the quantile pieces, mean, root."""
    width, iu, iv, denom = gref.pieces(u.shape[1], v.shape[1])
    us, vs = torch.sort(u, dim=1, stable=True).values, torch.sort(v, dim=1, stable=True).values
    t = us[:, torch.from_numpy(iu)] - vs[:, torch.from_numpy(iv)]
    wpp = (torch.from_numpy(width).double() * t.abs() ** p).sum(dim=1) / denom
    return wpp.mean() ** (1.0 / p)


@pytest.mark.parametrize("n,m,p", ORACLE_CASES)
def test_oracle_agrees_with_torch_fp64_autograd(n, m, p):
    u, v = oracle_inputs(n, m)
    dist, gu, au, gv, av = gref.dist_and_grad(u, v, p)
    want = float(np.mean([ref.wasserstein_1d_pp(a, b, p) for a, b in zip(u, v)]) ** (1.0 / p))
    assert abs(dist - want) <= 1e-15 * want
    tu, tv = torch.from_numpy(u).requires_grad_(), torch.from_numpy(v).requires_grad_()
    torch_dist(tu, tv, p).backward()
    eu, ev = np.abs(gu - tu.grad.numpy()), np.abs(gv - tv.grad.numpy())
    print(f"n={n} m={m} p={p}: max err / abs_sum = {max((eu / au).max(), (ev / av).max()):.2e}")
    assert (eu <= 1e-12 * au).all() and (ev <= 1e-12 * av).all()


@pytest.mark.parametrize("n,m,p", ORACLE_CASES)
def test_oracle_agrees_with_central_differences(n, m, p):
    u, v = oracle_inputs(n, m)
    _, gu, _, gv, _ = gref.dist_and_grad(u, v, p)
    rng = np.random.default_rng(5)
    du, dv = rng.normal(size=u.shape), rng.normal(size=v.shape)
    eps = 1e-7
    fd = (gref.dist_and_grad(u + eps * du, v + eps * dv, p)[0] - gref.dist_and_grad(u - eps * du, v - eps * dv, p)[0]) / (2 * eps)
    an = float((gu * du).sum() + (gv * dv).sum())
    print(f"n={n} m={m} p={p}: directional derivative {an!r}, central difference {fd!r}, rel {abs(an - fd) / abs(an):.2e}")
    assert abs(an - fd) <= 1e-6 * abs(an)


def test_oracle_gives_zero_for_identical_clouds():
    u, _ = oracle_inputs(50, 50)
    dist, gu, au, gv, av = gref.dist_and_grad(u, u.copy(), 2.0)
    assert dist == 0.0 and not gu.any() and not gv.any() and not au.any() and not av.any()


# ------------------------------------------------------------------------------------------------ pair sort
def mapped_keys(k: np.ndarray) -> np.ndarray:
    """The order-preserving unsigned key of swd.hip restated: sign bit set -> all bits flipped, else the sign bit set; NaN last."""
    b = k.view(np.uint32)
    m = np.where(b >> 31 != 0, ~b, b ^ np.uint32(0x80000000))
    return np.where(np.isnan(k), np.uint32(0xFFFFFFFF), m)


def assert_pairs(keys, got, perm, backend, tl):
    plain = ops.segmented_sort(keys.to(backend), _tile_log2=tl)
    assert got.dtype == torch.float32 and perm.dtype == torch.int32 and got.shape == perm.shape == keys.shape
    assert torch.equal(got.view(torch.int32), plain.view(torch.int32)), "values differ from the keys-only sort"
    perm = perm.cpu().numpy()
    want = np.argsort(mapped_keys(keys.numpy()), axis=1, kind="stable")
    assert (perm == want).all(), f"{int((perm != want).sum())} positions differ from the stable argsort of the mapped keys"
    k = keys.numpy()
    if not ((k == 0.0) & np.signbit(k)).any():
        assert (perm == torch.sort(keys, dim=1, stable=True).indices.numpy()).all()


@pytest.mark.parametrize("P", [1, 3, 50])
@pytest.mark.parametrize("kind", ["random", "duplicates", "sorted", "reversed", "special"])
def test_pair_sort_values_and_positions(backend, kind, P):
    tl, T = tile_of(backend)
    gen = torch.Generator().manual_seed(4321 + P)
    for N in (1, 2, T - 1, T, T + 1, 3 * T + 17, 11 * T - 1):
        keys = make_keys(kind, P, N, gen)
        got, perm = ops.segmented_sort_pairs(keys.to(backend), _tile_log2=tl)
        assert_pairs(keys, got, perm, backend, tl)


def test_pair_sort_many_tiles_and_in_place(backend):
    """37 tiles: six merge passes, the last run without a partner in several of them; sorting into the input buffer."""
    tl, T = tile_of(backend)
    gen = torch.Generator().manual_seed(5)
    keys = make_keys("special", 3, 37 * T + 5, gen)
    dev = keys.to(backend)
    got, perm = ops.segmented_sort_pairs(dev, _tile_log2=tl)
    assert_pairs(keys, got, perm, backend, tl)
    _, perm2 = ops.segmented_sort_pairs(dev, out=dev, _tile_log2=tl)
    assert torch.equal(dev.view(torch.int32), got.view(torch.int32)) and torch.equal(perm2, perm)


def test_pair_sort_tile_sizes_agree(backend):
    gen = torch.Generator().manual_seed(6)
    keys = make_keys("duplicates", 2, 3000, gen)
    want = torch.sort(keys, dim=1, stable=True)
    for tl in (4, 5, 6, 7, 8, 9, 10, 11, 12, 0):
        got, perm = ops.segmented_sort_pairs(keys.to(backend), _tile_log2=tl)
        assert torch.equal(got.cpu(), want.values) and torch.equal(perm.cpu().long(), want.indices), tl
    with pytest.raises(RuntimeError, match="tile_log2"):
        ops.segmented_sort_pairs(keys.to(backend), _tile_log2=3)


# ------------------------------------------------------------------------------------------------ adjoint of the cost
def sorted_rows(n1, n2, gen, P=5):
    u = torch.sort(torch.randn(P, n1, generator=gen), dim=1).values
    v = torch.sort(0.4 + 1.3 * torch.randn(P, n2, generator=gen), dim=1).values
    return u, v


@pytest.mark.parametrize("p", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("n1,n2", [(1, 1), (5, 3), (3, 5), (1000, 777), (777, 1000), (4096, 4096), (9000, 4001), (2, 4097),
                                   (4097, 1)])
def test_cost_backward_against_fp64(backend, n1, n2, p):
    """Exactly sorted fp32 rows.  Per entry |got - want| <= 2e-6 abs_sum (abs_sum: the sum of the absolute terms of that entry):
    t = a - b is one fp32 subtraction, 2^-24 relative, times p - 1 through the power; the final rounding to fp32 adds 2^-24;
    coef inherits the 1e-6 that test_quantile_cost_against_fp64 allows on wpp, times |1/p - 1| <= 1:
    1e-6 + (p + 1) 6e-8 < 2e-6 for p <= 3.  Where no term is non-zero the result is exactly 0."""
    gen = torch.Generator().manual_seed(n1 + 3 * n2)
    u, v = sorted_rows(n1, n2, gen)
    du, dv = u.to(backend), v.to(backend)
    wpp, _ = ops.swd_quantile_cost(du, dv, p)
    gu, gv = ops.swd_quantile_cost_bwd(du, dv, wpp, torch.ones((), device=backend), p)
    assert gu.shape == u.shape and gv.shape == v.shape and gu.dtype == gv.dtype == torch.float32
    _, wu, au, wv, av = gref.dist_and_grad(u.numpy(), v.numpy(), p)
    worst = 0.0
    for got, want, a in ((gu, wu, au), (gv, wv, av)):
        got = got.cpu().numpy().astype(np.float64)
        err = np.abs(got - want)
        worst = max(worst, float((err[a > 0] / a[a > 0]).max()))
        assert (err <= 2e-6 * a).all() and (got[a == 0] == 0.0).all()
    print(f"n1={n1} n2={n2} p={p}: max err / abs_sum = {worst:.2e}")
    # the upstream gradient scales the result; one side may be left out
    g3, none = ops.swd_quantile_cost_bwd(du, dv, wpp, torch.full((), -3.0, device=backend), p, need_v=False)
    assert none is None and np.allclose(g3.cpu().numpy(), -3.0 * gu.cpu().numpy(), rtol=1e-6, atol=0.0)
    none, g4 = ops.swd_quantile_cost_bwd(du, dv, wpp, torch.ones((), device=backend), p, need_u=False)
    assert none is None and torch.equal(g4, gv)


@pytest.mark.parametrize("n1,n2", [(300, 300), (300, 211), (2, 700)])
def test_cost_backward_unsort_swap_and_degenerate_inputs(backend, n1, n2):
    gen = torch.Generator().manual_seed(n1 + n2)
    u, v = sorted_rows(n1, n2, gen, P=3)
    du, dv = u.to(backend), v.to(backend)
    one = torch.ones((), device=backend)
    wpp, _ = ops.swd_quantile_cost(du, dv, 2.0)
    gu, gv = ops.swd_quantile_cost_bwd(du, dv, wpp, one, 2.0)
    # with perm the value of rank r lands at position perm[s, r]
    pu = torch.stack([torch.randperm(n1, generator=gen) for _ in range(3)]).to(torch.int32)
    pv = torch.stack([torch.randperm(n2, generator=gen) for _ in range(3)]).to(torch.int32)
    su, sv = ops.swd_quantile_cost_bwd(du, dv, wpp, one, 2.0, perm_u=pu.to(backend), perm_v=pv.to(backend))
    want_u, want_v = torch.empty_like(u), torch.empty_like(v)
    want_u.scatter_(1, pu.long(), gu.cpu())
    want_v.scatter_(1, pv.long(), gv.cpu())
    assert torch.equal(su.cpu(), want_u) and torch.equal(sv.cpu(), want_v)
    # the larger set always gets the threads: swapping the arguments swaps the outputs, bit for bit
    wpp_s, _ = ops.swd_quantile_cost(dv, du, 2.0)
    hv, hu = ops.swd_quantile_cost_bwd(dv, du, wpp_s, one, 2.0)
    assert torch.equal(hu.view(torch.int32), gu.view(torch.int32)) and torch.equal(hv.view(torch.int32), gv.view(torch.int32))
    # a NaN cost makes every gradient NaN
    bad = wpp.clone()
    bad[1] = float("nan")
    for p in (1.0, 2.0):
        nu, nv = ops.swd_quantile_cost_bwd(du, dv, bad, one, p)
        assert bool(torch.isnan(nu).all()) and bool(torch.isnan(nv).all())
    # identical rows: M == 0 and zero gradients, also for p = 2 where the composed formula has 0 * inf
    if n1 == n2:
        for p in (1.0, 2.0):
            w0, d0 = ops.swd_quantile_cost(du, du.clone(), p)
            assert float(d0) == 0.0
            zu, zv = ops.swd_quantile_cost_bwd(du, du.clone(), w0, one, p)
            assert bool((zu == 0).all()) and bool((zv == 0).all())


# ------------------------------------------------------------------------------------------------ back-projection
@pytest.mark.parametrize("P", [1, 50, 1100])
@pytest.mark.parametrize("d", [1, 3, 6, 8])
def test_back_projection_within_the_fma_chain_bound(backend, d, P):
    """gx[i, k] = sum_p dir[k, p] g[p, i] as an fmaf chain of P terms: |err| <= (P + 2) 2^-24 sum_p |dir[k, p] g[p, i]| (the
    form of the forward projection's bound; P = 1100 crosses the 1024 directions one LDS chunk holds).  accumulate: one more
    rounding, of prior + sum, so |prior| joins the sum of absolute terms."""
    gen = torch.Generator().manual_seed(100 * d + P)
    N = 300 if backend.type == "cpu" else 20003
    g = torch.randn(P, N, generator=gen)
    dirs = torch.randn(d, P, generator=gen)
    dirs = dirs / dirs.norm(dim=0, keepdim=True)
    got = ops.swd_project_bwd(g.to(backend), dirs.to(backend))
    assert got.shape == (N, d) and got.dtype == torch.float32
    want = gref.back_project(g.numpy(), dirs.numpy())
    mag = np.abs(g.numpy().astype(np.float64)).T @ np.abs(dirs.numpy().astype(np.float64)).T
    bound = (P + 2) * 2.0 ** -24 * mag
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"d={d} P={P}: max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    prior = torch.randn(N, d, generator=gen)
    buf = prior.clone().to(backend)
    ops.swd_project_bwd(g.to(backend), dirs.to(backend), out=buf, accumulate=True)
    err = np.abs(buf.cpu().numpy().astype(np.float64) - (want + prior.numpy().astype(np.float64)))
    assert (err <= (P + 2) * 2.0 ** -24 * (mag + np.abs(prior.numpy().astype(np.float64)))).all()
    with pytest.raises(RuntimeError, match="ndim"):
        ops.swd_project_bwd(torch.randn(2, 16).to(backend), torch.randn(9, 2).to(backend))


# ------------------------------------------------------------------------------------------------ end to end
def end_to_end_oracle(x1, x2, dirs, p, backend):
    """Gradient and per-entry bound from the fp32 projections the library itself forms, promoted to fp64: the pairing of ranks
    is then the library's (ties go by position in both).  The gradient jumps across rank swaps, so an oracle on exact fp64
    projections would bound nothing.  Bound per entry of gx: (2e-6 + (P + 2) 2^-24) sum_p |dir[k, p]| abs_sum[p, i]: the gate
    of the cost backward and the fma chain of the back-projection."""
    P = dirs.shape[1]
    u1 = ops.swd_project(x1.to(backend), dirs.to(backend)).cpu().numpy()
    u2 = ops.swd_project(x2.to(backend), dirs.to(backend)).cpu().numpy()
    dist, g1, a1, g2, a2 = gref.dist_and_grad(u1, u2, p)
    rel = 2e-6 + (P + 2) * 2.0 ** -24
    absdir = np.abs(dirs.numpy().astype(np.float64))
    return dist, [(gref.back_project(g, dirs.numpy()), rel * (a.T @ absdir.T)) for g, a in ((g1, a1), (g2, a2))]


@pytest.mark.parametrize("p", [1.0, 2.0])
@pytest.mark.parametrize("shape", ["equal", "unequal"])
def test_end_to_end_gradient(backend, shape, p):
    gen = torch.Generator().manual_seed(11)
    d, P = 6, 20
    if backend.type == "cpu":
        n1, n2 = (3000, 3000) if shape == "equal" else (3000, 1801)
    else:
        n1, n2 = (20000, 20000) if shape == "equal" else (20000, 12007)
    x1, x2 = clouds(n1, n2, d, gen)
    dirs = torch.randn(d, P, generator=gen)
    dirs = dirs / dirs.norm(dim=0, keepdim=True)
    tl, _ = tile_of(backend)
    a, b = x1.clone().to(backend).requires_grad_(), x2.clone().to(backend).requires_grad_()
    dist = ops.SlicedWassersteinFn.apply(a, b, dirs.to(backend), p, tl)
    assert dist.dim() == 0 and dist.dtype == torch.float32 and dist.requires_grad
    assert torch.equal(dist.detach(), ops.sliced_wasserstein(x1.to(backend), x2.to(backend), dirs.to(backend), p))
    dist.backward()
    want_dist, sides = end_to_end_oracle(x1, x2, dirs, p, backend)
    assert abs(float(dist.detach()) - want_dist) <= 2e-6 * want_dist
    for name, got, (want, bound) in (("gx1", a.grad, sides[0]), ("gx2", b.grad, sides[1])):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print(f"{shape} p={p} {name}: max err / bound = {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
    # one side only: the other sort carries no positions, the gradient is the same bits
    a1 = x1.clone().to(backend).requires_grad_()
    ops.SlicedWassersteinFn.apply(a1, x2.to(backend), dirs.to(backend), p, tl).backward()
    assert torch.equal(a1.grad, a.grad)


def test_translation_gradient_closed_form(backend):
    """x2 = x1 + c on the 2^-10 grid of test_swd_api.test_translation, p = 2: every projection moves rigidly by s_p = c . dir_p, so
    dist^2 = mean_p s_p^2 and, whatever the ranks, every row of gx1 is  -sum_p s_p dir_p / (n P dist)  and gx2 its negative.
    Gate per entry, derived as test_translation derives its own.  The library pairs sorted fp32 projections, each within delta
    (tests/_swd_fp64.delta) of its exact value, so every difference is -(s_p + e), |e| <= 2 delta.  Its 1 / dist is within
    rho = 1 / sqrt(1 - B / dist^2) - 1 of the exact one, B being test_translation's bound on dist^2.  The cost backward and the
    fma chain add eps = 2e-6 + (P + 2) 2^-24 relative (test_cost_backward_against_fp64, the back-projection test).  Hence
    |got - want| <= sum_p |dir[k, p]| (|s_p| rel + 2 delta (1 + rel)) / (n P dist),   rel = (1 + rho)(1 + eps) - 1."""
    gen = torch.Generator().manual_seed(2)
    d, P, N = 6, 50, 4000
    x1 = torch.round(torch.randn(N, d, generator=gen) * 1024.0) / 1024.0
    c = torch.round(torch.randn(d, generator=gen) * 512.0) / 1024.0
    x2 = x1 + c
    dirs = torch.randn(d, P, generator=gen)
    dirs = dirs / dirs.norm(dim=0, keepdim=True)
    tl, _ = tile_of(backend)
    a, b = x1.clone().to(backend).requires_grad_(), x2.clone().to(backend).requires_grad_()
    ops.SlicedWassersteinFn.apply(a, b, dirs.to(backend), 2.0, tl).backward()
    D = dirs.double().numpy()
    s = c.double().numpy() @ D
    dist_sq = float(np.mean(s**2))
    dist = dist_sq ** 0.5
    want = -(D * s).sum(axis=1) / (N * P * dist)
    dl = ref.delta(x1.numpy(), x2.numpy())
    B = float(np.mean(4.0 * dl * np.abs(s) + 4.0 * dl * dl)) + (2.0 ** -22 + 1e-6) * dist_sq
    rel = (1.0 / np.sqrt(1.0 - B / dist_sq)) * (1.0 + 2e-6 + (P + 2) * 2.0 ** -24) - 1.0
    bound = (np.abs(D) * (np.abs(s) * rel + 2.0 * dl * (1.0 + rel))).sum(axis=1) / (N * P * dist)
    e1 = np.abs(a.grad.cpu().numpy().astype(np.float64) - want[None, :])
    e2 = np.abs(b.grad.cpu().numpy().astype(np.float64) + want[None, :])
    print(f"translation gradient: max err / bound = {float(max((e1 / bound).max(), (e2 / bound).max())):.3f}")
    assert (e1 <= bound[None, :]).all() and (e2 <= bound[None, :]).all()
