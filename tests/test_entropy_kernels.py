"""Kernels of the sample-based entropy estimators (mentflow_amd/csrc/entropy.hip) against the fp64 restatement in
tests/_entropy_fp64.py and the reference's covariance estimator (tests/golden/ref_entropy_cov.npz): emulator here (sizes up to
about 3 000 points, candidate range cut through the private chunk override), the MI355X with -m gpu (also 25 000 and 100 000
points).  Every bound is derived where it is used, from the rounding of the formats; none is fitted to what the kernels return.

u = 2^-24 is the unit roundoff of fp32 throughout."""
import math

import numpy as np
import pytest
import torch

import _entropy_fp64 as ref
from mentflow_amd import ops

U = 2.0 ** -24
FLT_MIN = ref.FLT_MIN


# ------------------------------------------------------------------------------------------------ data
def make_cloud(kind, n, d, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "gaussian":
        x = torch.randn(n, d, generator=g)
    elif kind == "ring":                         # a thin shell of radius 2 in the first two coordinates
        phi = 2 * math.pi * torch.rand(n, generator=g)
        r = 2.0 + 0.05 * torch.randn(n, generator=g)
        x = 0.3 * torch.randn(n, d, generator=g)
        x[:, 0] = r * torch.cos(phi)
        if d > 1:
            x[:, 1] = r * torch.sin(phi)
    elif kind == "clustered":                    # seven tight clusters of very different widths, far from the origin
        centres = 5.0 * torch.randn(7, d, generator=g) + 10.0
        widths = torch.tensor([1.0, 0.3, 0.1, 0.03, 0.01, 0.003, 0.001])
        pick = torch.randint(0, 7, (n,), generator=g)
        x = centres[pick] + widths[pick, None] * torch.randn(n, d, generator=g)
    else:
        raise AssertionError(kind)
    return x.to(torch.float32).contiguous()


def run(x, k, backend, chunks=0, grad=False):
    """(H, idx, rho2, S[, dH/dx]) on the CPU."""
    xd = x.detach().clone().to(backend).requires_grad_(grad)
    H, idx, rho2, S = ops.knn_entropy(xd, k, _chunks=chunks)
    out = [H.detach().cpu(), idx.cpu(), rho2.cpu(), S.cpu()]
    if grad:
        H.backward()
        out.append(xd.grad.cpu())
    return out


def cases(backend):
    """(kind, N, d, k, chunk override): ragged N (no multiple of the 256-query workgroup, the 256-candidate tile or 4)."""
    small = [("gaussian", 1501, 6, 5, 3), ("ring", 2999, 2, 5, 0), ("clustered", 1203, 6, 5, 7), ("gaussian", 777, 1, 1, 2),
             ("gaussian", 1030, 16, 16, 5), ("ring", 517, 3, 1, 1), ("clustered", 2050, 2, 16, 4), ("gaussian", 18, 6, 16, 0),
             ("gaussian", 3, 2, 2, 0)]
    if backend.type == "cpu":
        return small
    return small + [("gaussian", 25000, 6, 5, 0), ("ring", 25000, 6, 5, 0), ("clustered", 25000, 6, 5, 0),
                    ("gaussian", 100000, 6, 5, 0), ("gaussian", 25000, 1, 5, 0), ("gaussian", 25000, 2, 1, 0),
                    ("ring", 25000, 16, 16, 0), ("clustered", 100000, 2, 16, 0)]


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("n,d,k", [(2000, 2, 1), (2000, 6, 5), (3001, 3, 16), (500, 1, 3)])
def test_restatement_distances_equal_ckdtree(n, d, k):
    from scipy.spatial import cKDTree
    x = np.random.default_rng(n + d + k).normal(size=(n, d))
    _, rho2 = ref.kth_neighbours(x, k)
    dist, _ = cKDTree(x).query(x, k=k + 1)                 # the first hit is the point itself
    want = dist[:, k]
    # both form sum_c diff^2 in fp64; the tree takes the root, we square it again: two roundings
    assert np.max(np.abs(np.sqrt(rho2) - want) / want) <= 4 * 2.0 ** -53
    idx_t, rho2_t = ref.kth_neighbours_tree(x, k)
    idx_d, _ = ref.kth_neighbours(x, k)
    assert np.array_equal(idx_t, idx_d) and np.array_equal(rho2_t, rho2)


def test_restatement_by_hand():
    # x = 0, 1, 3 on a line, k = 1: rho = 1, 1, 2 with neighbours 1, 0, 1
    x = np.array([[0.0], [1.0], [3.0]])
    H, idx, rho2 = ref.knn_entropy(x, 1)
    assert idx.tolist() == [1, 0, 1] and rho2.tolist() == [1.0, 1.0, 4.0]
    # psi(3) - psi(1) = 1 + 1/2, c_1 = 2, sum ln rho = ln 2, d / N = 1/3
    assert H == pytest.approx(-(1.5 + math.log(2.0) + math.log(2.0) / 3.0), rel=1e-15)
    # x = 0, 1, 2: point 1 has two neighbours at distance 1
    idx2, rho22 = ref.kth_neighbours(np.array([[0.0], [1.0], [2.0]]), 1)
    assert idx2.tolist() == [1, 0, 1] and rho22.tolist() == [1.0, 1.0, 1.0]          # the lower index wins the tie
    idx3, _ = ref.kth_neighbours(np.array([[0.0], [1.0], [2.0]]), 2)
    assert idx3.tolist() == [2, 2, 0]
    g = ref.knn_entropy_grad(x, 1)               # sum ln rho = ln|x1-x0| + ln|x0-x1| + ln|x2-x1|; dH = -(1/3) d(sum)
    assert np.allclose(g[:, 0], -np.array([-2.0, 2.0 - 0.5, 0.5]) / 3.0, rtol=1e-15)


@pytest.mark.parametrize("d,k", [(2, 1), (6, 5)])
def test_restatement_gradient_equals_autograd(d, k):
    x = torch.randn(300, d, dtype=torch.float64, generator=torch.Generator().manual_seed(d)).requires_grad_(True)
    # direct differences (cdist's default for this size is the Gram form, which loses digits for close pairs)
    dist = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist") + torch.diag(torch.full((300,), float("inf"), dtype=torch.float64))
    rho = torch.topk(dist, k, dim=1, largest=False).values[:, k - 1]
    H = -(ref.constant(300, d, k) + d / 300 * torch.log(rho).sum())
    H.backward()
    assert float(H.detach()) == pytest.approx(ref.knn_entropy(x.detach().numpy(), k)[0], rel=1e-13)
    want = x.grad.numpy()
    got = ref.knn_entropy_grad(x.detach().numpy(), k)
    # both are fp64 chains of about ten operations per term and at most a few dozen terms per row: below 100 * 2^-53 of a
    # row's sum of absolute terms, itself below ten times the largest gradient entry here
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


# ------------------------------------------------------------------------------------------------ neighbours, value, gradient
def test_neighbours_value_and_gradient(backend):
    """For every case, EVERY point (no point is left out):

    Neighbours.  The kernel orders fp32 squared distances r = fl(sum_c fl(x_ic - x_jc)^2): each difference carries one
    rounding (relative u, squared: 2 u), the d fused multiply-adds one each, so r = rho^2 (1 + e), |e| <= (d + 2) u, and the
    root rho (1 + e / 2).  The k-th order statistic of values perturbed by at most that factor lies within the same factor of
    the exact k-th order statistic, and the returned point lies within it once more:
        |rho64(i, j(i)) - rho64_k(i)| <= (d + 2) 2^-23 rho64_k(i),      |rho2[i] - rho64(i, j(i))^2| <= (d + 2) u rho64^2.
    (Stated for rho^2 well above the subnormal range, >= 2^24 FLT_MIN; the clouds here have no closer pairs — asserted.)

    Value.  H = -[C + (d / N) S], S = sum_i 0.5 ln rho2[i].  From the above |0.5 ln(1 + e)| <= 0.5 (d + 2) u (1 + 2^-20) per
    term, hence (d / 2)(d + 2) u (1 + 2^-20) in H.  The logarithm is taken in fp64 (error below 4 ulp of fp64 on
    |ln rho^2| <= 89, the range of fp32): (d / 2) 4 * 89 * 2^-53.  The N terms are added in fp64 in a fixed tree: at most
    N 2^-53 sum |ln rho| <= N^2 45 * 2^-53 on S, d N 45 * 2^-53 on H.  C is formed on the host in fp64 (psi by its asymptotic
    series, error < 1e-14; lgamma): 1e-13.  H is rounded to fp32 once: u |H|.  The fp64 sum S is returned too and is held to
    the bound without the last term.

    Gradient.  Row i of dH/dx is -(d / N) g times the sum of m_i terms w_t (x_i - x_t) (its own neighbour and the points whose
    k-th neighbour it is), compared with the same sum in fp64 over the kernel's own — just verified — indices.  Per term: the
    difference u, w = fl(1 / rho2) (d + 2) u + u, the product u (the later terms are one fma: that rounding is the
    accumulation's); accumulating m_i terms in sequence at most (m_i - 1) u of sum |terms|; the factor fl(fl(d / N) * g) and
    the final product 3 u.  Hence per component, with second-order terms covered by 1 %:
        |err| <= 1.01 (d + 7 + m_i) u (d / N) sum_t |w_t (x_ic - x_tc)|.
    """
    worst = dict(nb=0.0, r2=0.0, H=0.0, S=0.0, g=0.0)
    for kind, n, d, k, chunks in cases(backend):
        x = make_cloud(kind, n, d, 100 + n + d + k)
        H, idx, rho2, S, gx = run(x, k, backend, chunks, grad=True)
        x64 = x.numpy().astype(np.float64)
        idx64, rho2_64 = ref.kth_neighbours(x64, k)
        assert rho2_64.min() >= 2.0 ** 24 * FLT_MIN
        j = idx.numpy().astype(np.int64)
        assert idx.dtype == torch.int32 and j.min() >= 0 and j.max() < n and not np.any(j == np.arange(n))
        diff = x64 - x64[j]
        r2_of_j = np.einsum("nc,nc->n", diff, diff)
        rho_k = np.sqrt(rho2_64)
        e_nb = np.abs(np.sqrt(r2_of_j) - rho_k) / rho_k
        e_r2 = np.abs(rho2.numpy().astype(np.float64) - r2_of_j) / r2_of_j
        differ = int(np.sum(j != idx64))
        assert e_nb.max() <= (d + 2) * 2.0 ** -23, (kind, n, d, k, e_nb.max())
        assert e_r2.max() <= (d + 2) * U, (kind, n, d, k, e_r2.max())

        H64 = ref.entropy_from(rho2_64, d, k)
        S64 = float(np.sum(ref.ln_rho(rho2_64)))
        fp64_part = 0.5 * 4 * 89 * 2.0 ** -53 + n * 45 * 2.0 ** -53
        bound_S = n * (0.5 * (d + 2) * U * (1 + 2.0 ** -20) + fp64_part)
        bound_H = d / n * bound_S + 1e-13 + U * abs(H64)
        err_S, err_H = abs(float(S) - S64), abs(float(H) - H64)
        assert err_S <= bound_S, (kind, n, d, k, err_S, bound_S)
        assert err_H <= bound_H, (kind, n, d, k, err_H, bound_H)

        terms, absg, count = ref.grad_terms(x64, j)
        want = -(d / n) * terms
        bound_g = 1.01 * (d + 7 + count)[:, None] * U * (d / n) * absg
        err_g = np.abs(gx.numpy().astype(np.float64) - want)
        ratio = float(np.max(err_g / np.maximum(bound_g, 1e-300)))
        assert np.all(err_g <= bound_g), (kind, n, d, k, ratio)
        print(f"knn {kind:9s} N={n:6d} d={d:2d} k={k:2d} chunks={chunks}: {differ} indices differ from fp64, "
              f"max rel err rho {e_nb.max():.2e} (bound {(d + 2) * 2.0 ** -23:.2e}), |dH| {err_H:.2e} (bound {bound_H:.2e}), "
              f"|dS| {err_S:.2e} (bound {bound_S:.2e}), gradient error / bound {ratio:.3f}, max in-degree {count.max() - 1}")
        worst = dict(nb=max(worst["nb"], e_nb.max() / ((d + 2) * 2.0 ** -23)), r2=max(worst["r2"], e_r2.max() / ((d + 2) * U)),
                     H=max(worst["H"], err_H / bound_H), S=max(worst["S"], err_S / bound_S), g=max(worst["g"], ratio))
    print("knn worst error / bound:", {k_: f"{v:.3f}" for k_, v in worst.items()})


# ------------------------------------------------------------------------------------------------ exact properties
@pytest.mark.parametrize("kind,n,d,k", [("gaussian", 1501, 6, 5), ("clustered", 900, 2, 1), ("ring", 1100, 16, 16)])
def test_scaling_by_two_and_translation(backend, kind, n, d, k):
    """Scaling by 2 is exact in fp32: every squared distance is multiplied by 4 exactly, the neighbours are identical and
    H(2x) - H(x) = -d ln 2 up to the roundings of the two fp64 sums (N 2^-53 * 45 relative to N, twice) and of the two fp32
    results (u |H| each).  A translation by a power of two that keeps all coordinates on the grid of the originals keeps every
    difference exact: idx and rho2 are unchanged."""
    x = make_cloud(kind, n, d, 7)
    H1, i1, r1, S1 = run(x, k, backend)
    H2, i2, r2, S2 = run(2.0 * x, k, backend)
    assert torch.equal(i1, i2) and torch.equal(4.0 * r1, r2)
    tol = U * (abs(float(H1)) + abs(float(H2))) + 2 * d * n * 45 * 2.0 ** -53 + 1e-13
    assert abs((float(H2) - float(H1)) + d * math.log(2.0)) <= tol
    assert abs((float(S2) - float(S1)) - n * math.log(2.0)) <= 2 * n * n * 45 * 2.0 ** -53 + n * 2.0 ** -52
    # coordinates rounded to multiples of 2^-10 below 64 in magnitude: x + 64 is exact in fp32 (needs 6 + 10 + 1 bits)
    xq = torch.round(x.clamp(-60, 60) * 1024) / 1024
    _, i3, r3, _ = run(xq, k, backend)
    _, i4, r4, _ = run(xq + 64.0, k, backend)
    assert torch.equal(i3, i4) and torch.equal(r3, r4)


# ------------------------------------------------------------------------------------------------ determinism
def test_bitwise_reproducible_and_independent_of_the_chunking(backend):
    n, d, k = (2311, 6, 5) if backend.type == "cpu" else (25000, 6, 5)
    x = make_cloud("ring", n, d, 3)
    a = run(x, k, backend, grad=True)
    b = run(x, k, backend, grad=True)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    for chunks in (1, 2, 9, 64, 300):
        c = run(x, k, backend, chunks)
        assert torch.equal(a[1], c[1]) and torch.equal(a[2], c[2]), chunks
        assert float(c[3]) == float(a[3])                  # same rho2, same fixed-order sum


def test_ties_go_to_the_lower_index_whatever_the_chunking(backend):
    """Points on an integer lattice: most k-th distances are tied between several candidates, which may lie in different
    chunks; distances between small integers are exact in fp32, so the kernel must return the restatement's index."""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 6, (1400, 3), generator=g).float()
    for k in (1, 5, 16):
        idx64, rho2_64 = ref.kth_neighbours(x.numpy(), k)
        for chunks in (0, 1, 3, 50):
            _, idx, rho2, _ = run(x, k, backend, chunks)
            assert np.array_equal(idx.numpy().astype(np.int64), idx64), (k, chunks)
            assert np.array_equal(rho2.numpy().astype(np.float64), rho2_64), (k, chunks)


# ------------------------------------------------------------------------------------------------ edge cases
def test_duplicates_are_floored_with_zero_gradient(backend):
    x = make_cloud("gaussian", 600, 6, 11)
    x[100:200] = x[0:100]                                    # a hundred exact pairs
    H, idx, rho2, S, gx = run(x, 1, backend, grad=True)
    assert math.isfinite(float(H)) and bool(torch.isfinite(gx).all())
    assert bool((rho2[:200] == 0).all()) and torch.equal(idx[:100], torch.arange(100, 200, dtype=torch.int32))
    assert torch.equal(idx[100:200], torch.arange(0, 100, dtype=torch.int32))
    H64 = ref.entropy_from(ref.kth_neighbours(x.numpy(), 1)[1], 6, 1)     # the floor ln sqrt(FLT_MIN) for 200 terms
    assert abs(float(H) - H64) <= 3 * 8 * U * (1 + 2.0 ** -20) + U * abs(H64) + 1e-9
    terms, absg, count = ref.grad_terms(x.numpy().astype(np.float64), idx.numpy().astype(np.int64))
    assert np.all(np.abs(gx.numpy() - (-(6 / 600) * terms)) <= 1.01 * (13 + count)[:, None] * U * (6 / 600) * absg)
    assert bool((gx[:200][torch.from_numpy(count[:200] == 2)] == 0).all())   # a pair that nobody else points at: no gradient at all


def test_all_identical_points(backend):
    for k in (1, 5, 16):
        x = torch.full((k + 1, 4), 1.25)
        H, idx, rho2, S, gx = run(x, k, backend, grad=True)
        assert bool((rho2 == 0).all()) and bool((gx == 0).all())
        assert float(H) == pytest.approx(-(ref.constant(k + 1, 4, k) + 4 * 0.5 * math.log(FLT_MIN)), rel=1e-6)
        want = [k if i < k else k - 1 for i in range(k + 1)]      # the k-th other index in ascending order
        assert idx.tolist() == want


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_non_finite_row(backend, bad):
    x = make_cloud("gaussian", 700, 6, 13)
    x[345, 2] = bad
    H, idx, rho2, S, gx = run(x, 5, backend, chunks=3, grad=True)
    assert not math.isfinite(float(H))
    assert int(idx.min()) >= 0 and int(idx.max()) < 700
    assert int(idx[345]) == 345 and float(rho2[345]) == float("inf")
    others = torch.arange(700) != 345
    assert bool((idx[others] != 345).all()) and bool(torch.isfinite(rho2[others]).all())


def test_limits_raise_by_name(backend):
    dev = backend
    with pytest.raises(RuntimeError, match="N > k"):
        ops.knn_entropy(torch.randn(5, 2).to(dev), 5)
    with pytest.raises(RuntimeError, match="N > k"):
        ops.knn_entropy(torch.randn(3, 2).to(dev), 7)
    with pytest.raises(RuntimeError, match="1 <= k <= 16"):
        ops.knn_entropy(torch.randn(50, 2).to(dev), 17)
    with pytest.raises(RuntimeError, match="1 <= k <= 16"):
        ops.knn_entropy(torch.randn(50, 2).to(dev), 0)
    with pytest.raises(RuntimeError, match="1 <= ndim <= 16"):
        ops.knn_entropy(torch.randn(50, 17).to(dev), 5)
    with pytest.raises(RuntimeError, match="chunk override"):
        ops.knn_entropy(torch.randn(50, 2).to(dev), 5, _chunks=-1)
    with pytest.raises(RuntimeError, match="float32"):
        ops.knn_entropy(torch.randn(50, 2, dtype=torch.float64).to(dev), 5)
    with pytest.raises(RuntimeError, match="1 <= ndim <= 16"):
        ops.cov_entropy(torch.randn(50, 17).to(dev))
    with pytest.raises(RuntimeError, match="at least two points"):
        ops.cov_entropy(torch.randn(1, 3).to(dev))
    import mentflow_amd as mf
    for cls in (mf.entropy.KNNEntropyEstimator, mf.entropy.CovarianceEntropyEstimator):
        with pytest.raises(ValueError, match=r"This class cannot estimate relative entropy \(prior != None\)\."):
            cls(prior=mf.prior.Gaussian(ndim=2, scale=1.0))


# ------------------------------------------------------------------------------------------------ covariance estimator
def cov_fp64(x, pad=1e-12):
    """The reference's formula and its closed-form gradient in fp64 (numpy): (H, dH/dx, cond(C))."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    mu = x.mean(0)
    C = np.atleast_2d(np.cov(x.T))
    eps = math.sqrt(np.linalg.det(C))
    H = -3.0 * math.log(2 * math.pi * math.e) - math.log(eps + pad)
    g = -eps / (eps + pad) * np.linalg.solve(C, (x - mu).T).T / (n - 1)
    return H, g, np.linalg.cond(C)


def test_covariance_against_the_reference(backend, golden):
    """The inputs are fp32 and exact in fp64; products of two fp32 values are exact in fp64, so the moments carry only the fp64
    accumulation, at most N 2^-53 relative to sum |x_a x_b|.  Forming C = (M - N mu mu^T) / (N - 1) cancels: relative to C the
    error is at most (N + 4) 2^-53 (1 + |mu|^2 / var) =: e_C per entry, elimination in fp64 amplifies it by at most
    cond(C) * d, so ln det carries d * cond * e_C and H half of it; H is rounded to fp32 once:
        |dH| <= u |H| + 0.5 d cond e_C + 1e-15.
    The gradient A (x_n - mu) is evaluated in fp64 (A and mu within d cond e_C relatively, the d-term dot product within d 2^-53
    of sum |A_ab (x_b - mu_b)|) and rounded to fp32 once, and the upstream factor 1.0 is exact:
        |err_na| <= (u + 2 d cond e_C + d 2^-53) sum_b |A_ab (x_nb - mu_b)|."""
    f = golden("ref_entropy_cov")
    for d in (2, 6):
        x = f[f"x_{d}"].float()
        n = x.shape[0]
        H64, g64, cond = cov_fp64(x.numpy())
        assert H64 == pytest.approx(float(f[f"H_{d}"]), rel=1e-12)                # the restatement is the reference's
        assert np.max(np.abs(g64 - f[f"dH_{d}"].numpy())) <= 1e-10 * np.max(np.abs(g64))
        xd = x.detach().clone().to(backend).requires_grad_(True)
        H = ops.cov_entropy(xd)
        H.backward()
        x64 = x.numpy().astype(np.float64)
        mu, var = x64.mean(0), x64.var(0)
        e_C = (n + 4) * 2.0 ** -53 * (1 + float(np.max(mu ** 2 / var)))
        bound_H = U * abs(H64) + 0.5 * d * cond * e_C + 1e-15
        err_H = abs(float(H.detach()) - float(f[f"H_{d}"]))
        C = np.atleast_2d(np.cov(x64.T))
        eps = math.sqrt(np.linalg.det(C))
        A = -eps / (eps + 1e-12) * np.linalg.inv(C) / (n - 1)
        absg = np.abs(x64 - mu) @ np.abs(A).T
        bound_g = (U + 2 * d * cond * e_C + d * 2.0 ** -53) * absg
        err_g = np.abs(xd.grad.cpu().numpy().astype(np.float64) - f[f"dH_{d}"].numpy())
        print(f"cov d={d}: H {float(H.detach()):.7f} reference {float(f[f'H_{d}']):.7f} |dH| {err_H:.2e} (bound {bound_H:.2e}); "
              f"gradient error / bound {float(np.max(err_g / bound_g)):.3f}")
        assert err_H <= bound_H
        assert np.all(err_g <= bound_g)


@pytest.mark.parametrize("n,d", [(2, 1), (3, 2), (1001, 6), (2777, 16), (5000, 3)])
def test_covariance_ragged_sizes_and_determinism(backend, n, d):
    """N not a multiple of the 256-row workgroup or of the 1024 rows a workgroup takes per pass; bounds as in
    test_covariance_against_the_reference against the same formula in fp64."""
    g = torch.Generator().manual_seed(n)
    x = (torch.randn(n, d, generator=g) @ (torch.eye(d) + 0.2 * torch.randn(d, d, generator=g)) + 0.5).float().contiguous()
    H64, g64, cond = cov_fp64(x.numpy())
    outs = []
    for _ in range(2):
        xd = x.detach().clone().to(backend).requires_grad_(True)
        H = ops.cov_entropy(xd)
        (3.0 * H).backward()                                 # the upstream gradient reaches the kernel as a device scalar
        outs.append((H.detach().cpu(), xd.grad.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    x64 = x.numpy().astype(np.float64)
    mu, var = x64.mean(0), x64.var(0)
    e_C = (n + 4) * 2.0 ** -53 * (1 + float(np.max(mu ** 2 / var)))
    assert abs(float(outs[0][0]) - H64) <= U * abs(H64) + 0.5 * d * cond * e_C + 1e-15
    C = np.atleast_2d(np.cov(x64.T))
    eps = math.sqrt(np.linalg.det(C))
    A = -eps / (eps + 1e-12) * np.linalg.inv(C) / (n - 1)
    absg = 3.0 * np.abs(x64 - mu) @ np.abs(A).T
    assert np.all(np.abs(outs[0][1].numpy() - 3.0 * g64) <= (U + 2 * d * cond * e_C + d * 2.0 ** -53) * absg + 1e-300)


def test_covariance_of_a_degenerate_cloud(backend):
    """All points on the line x = y: det C = 0, so eps = 0 up to rounding and H = -3 ln(2 pi e) - ln(eps + pad) stays finite.
    The three second moments are sums of the same products; should a reduction ever give them in different roundings, C differs
    from rank one by at most e_C = (N + 4) 2^-53 (1 + mu^2 / var) per entry relatively, det by 2 e_C var^2 and eps by its root:
    H lies between the exact-zero value -3 ln(2 pi e) - ln(pad) and that with eps = var sqrt(2 e_C), or is NaN for a determinant
    rounded below zero (the reference's behaviour too).  The gradient is either exactly zero (det <= 0) or finite."""
    t = torch.linspace(-1, 1, 500)
    x = torch.stack([t, t], dim=1).contiguous()
    xd = x.detach().clone().to(backend).requires_grad_(True)
    H = ops.cov_entropy(xd)
    H.backward()
    var = float(t.double().var())
    e_C = 504 * 2.0 ** -53
    hi = -3.0 * math.log(2 * math.pi * math.e) - math.log(1e-12)
    lo = -3.0 * math.log(2 * math.pi * math.e) - math.log(var * math.sqrt(2 * e_C) + 1e-12)
    h = float(H.detach())
    assert math.isnan(h) or lo - U * abs(lo) <= h <= hi + U * abs(hi)
    assert bool(torch.isfinite(xd.grad).all())
    if math.isnan(h) or h == pytest.approx(hi, rel=1e-6):
        assert bool((xd.grad == 0).all())
