"""Kernels of the sliced Wasserstein distance (mentflow_amd/csrc/swd.hip) against torch.sort and the fp64 restatement in
tests/_swd_fp64.py: emulator here (small tile override, so that a few thousand keys go through several merge passes), the
MI355X with -m gpu (default tile).  Bounds: see each test; none is fitted to what the kernels return."""
import numpy as np
import pytest
import torch

import _swd_fp64 as ref
from mentflow_amd import ops


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("n,m", [(1000, 1000), (1000, 777), (50000, 30011), (5, 3), (3, 5), (1, 1), (7, 1)])
def test_restatement_agrees_with_scipy_for_p1(n, m):
    from scipy.stats import wasserstein_distance
    rng = np.random.default_rng(n * 7 + m)
    u = rng.normal(size=n).astype(np.float32)
    v = (0.3 + 1.2 * rng.normal(size=m)).astype(np.float32)
    got, want = ref.wasserstein_1d_pp(u, v, 1.0), wasserstein_distance(u.astype(np.float64), v.astype(np.float64))
    print(f"restatement {got!r} scipy {want!r} rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-12 * want


def test_restatement_by_hand():
    # u = {0, 1, 2}, v = {0, 3}: quantile pieces (0,1/3] 0|0, (1/3,1/2] 1|0, (1/2,2/3] 1|3, (2/3,1] 2|3
    assert ref.wasserstein_1d_pp([2, 0, 1], [3, 0], 1.0) == pytest.approx(1 / 6 + 2 / 6 + 1 / 3, rel=1e-15)
    assert ref.wasserstein_1d_pp([2, 0, 1], [3, 0], 2.0) == pytest.approx(1 / 6 + 4 / 6 + 1 / 3, rel=1e-15)


# ------------------------------------------------------------------------------------------------ sort
def tile_of(backend):
    """(private tile override, tile size): a 64-key tile on the emulator, the built-in 4096 on the GPU."""
    return (6, 64) if backend.type == "cpu" else (0, 4096)


def make_keys(kind, P, N, gen):
    if kind == "random":
        k = torch.randn(P, N, generator=gen)
    elif kind == "duplicates":
        k = torch.randint(0, 5, (P, N), generator=gen).float() - 2.0
    elif kind == "sorted":
        k = torch.sort(torch.randn(P, N, generator=gen), dim=1).values
    elif kind == "reversed":
        k = torch.sort(torch.randn(P, N, generator=gen), dim=1, descending=True).values
    elif kind == "special":
        k = torch.randn(P, N, generator=gen)
        pool = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 1e-45, -1e-45, 1.1754942e-38, -3e-42, float("nan"),
                             -float("nan"), 3.4028235e38, -3.4028235e38])
        pick = torch.randint(0, 3 * pool.numel(), (P, N), generator=gen)          # a third of the keys are special values
        k = torch.where(pick < pool.numel(), pool[pick.clamp(max=pool.numel() - 1)], k)
    else:
        raise AssertionError(kind)
    return k


def assert_sorted_like_torch(got, keys):
    want = torch.sort(keys, dim=1).values
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaNs are not in the same trailing positions"
    fin = ~torch.isnan(want)
    assert bool((got[fin] == want[fin]).all()), f"{int((got[fin] != want[fin]).sum())} keys differ from torch.sort"


@pytest.mark.parametrize("P", [1, 3, 50])
@pytest.mark.parametrize("kind", ["random", "duplicates", "sorted", "reversed", "special"])
def test_segmented_sort_equals_torch_sort(backend, kind, P):
    tl, T = tile_of(backend)
    gen = torch.Generator().manual_seed(1234 + P)
    for N in (1, 2, T - 1, T, T + 1, 3 * T + 17, 5 * T + 3, 11 * T - 1):
        keys = make_keys(kind, P, N, gen)
        got = ops.segmented_sort(keys.to(backend), _tile_log2=tl)
        assert_sorted_like_torch(got, keys)


def test_segmented_sort_many_tiles_and_in_place(backend):
    """37 tiles: six merge passes, the last run without a partner in several of them; sorting into the input buffer."""
    tl, T = tile_of(backend)
    gen = torch.Generator().manual_seed(5)
    keys = make_keys("special", 3, 37 * T + 5, gen)
    dev = keys.to(backend)
    got = ops.segmented_sort(dev, _tile_log2=tl)
    assert_sorted_like_torch(got, keys)
    again = ops.segmented_sort(dev, _tile_log2=tl)
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))            # bitwise, NaN payloads included
    ops.segmented_sort(dev, out=dev, _tile_log2=tl)
    assert torch.equal(dev.view(torch.int32), got.view(torch.int32))


def test_segmented_sort_tile_sizes_agree(backend):
    gen = torch.Generator().manual_seed(6)
    keys = make_keys("random", 2, 3000, gen)
    for tl in (4, 5, 6, 7, 8, 9, 10, 11, 12, 0):
        assert_sorted_like_torch(ops.segmented_sort(keys.to(backend), _tile_log2=tl), keys)
    with pytest.raises(RuntimeError, match="tile_log2"):
        ops.segmented_sort(keys.to(backend), _tile_log2=3)


# ------------------------------------------------------------------------------------------------ projection
@pytest.mark.parametrize("d", [2, 3, 6, 8])
def test_projection_within_the_dot_product_rounding_bound(backend, d):
    """|u - exact| <= (d + 2) 2^-24 |x_n|_2 for unit directions: the rounding bound of a d-term fp32 dot product,
    gamma_d sum_k |x_k dir_k| <= d 2^-24 (1 + O(d 2^-24)) |x|_2 |dir|_2, with the +2 covering the second-order term and a
    direction normalised in fp32 (|dir|_2 within 2^-23 of 1).  The exact value uses the same fp32 directions in fp64."""
    gen = torch.Generator().manual_seed(d)
    N, P = (3001, 50) if backend.type == "cpu" else (200003, 50)
    x = torch.randn(N, d, generator=gen) * torch.linspace(0.1, 30.0, d)
    dirs = torch.randn(d, P, generator=gen)
    dirs = dirs / dirs.norm(dim=0, keepdim=True)
    u = ops.swd_project(x.to(backend), dirs.to(backend)).cpu()
    assert u.shape == (P, N)
    want = ref.project(x.numpy(), dirs.numpy())
    err = np.abs(u.numpy().astype(np.float64) - want)
    bound = (d + 2) * 2.0 ** -24 * np.linalg.norm(x.numpy().astype(np.float64), axis=1)
    print(f"d={d}: max err / bound = {float((err / bound[None, :]).max()):.3f}")
    assert (err <= bound[None, :]).all()


def test_projection_many_directions(backend):
    """More directions than one workgroup stages (1024): the second chunk of directions."""
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(130, 3, generator=gen)
    dirs = torch.randn(3, 1100, generator=gen)
    dirs = dirs / dirs.norm(dim=0, keepdim=True)
    u = ops.swd_project(x.to(backend), dirs.to(backend)).cpu().numpy().astype(np.float64)
    bound = 5 * 2.0 ** -24 * np.linalg.norm(x.numpy().astype(np.float64), axis=1)
    assert (np.abs(u - ref.project(x.numpy(), dirs.numpy())) <= bound[None, :]).all()


# ------------------------------------------------------------------------------------------------ cost
@pytest.mark.parametrize("p", [1.0, 2.0, 3.0])
@pytest.mark.parametrize("n1,n2", [(4096, 4096), (1, 1), (5, 3), (1000, 777), (777, 1000), (9000, 4001), (4099, 12500),
                                   (2, 4097)])
def test_quantile_cost_against_fp64(backend, n1, n2, p):
    """Exactly sorted fp32 inputs: the kernel adds one fp32 subtraction per term (2^-24 relative, times p through the power)
    and fp64 summation error to the restatement: 1e-6 relative is the gate the issue sets."""
    gen = torch.Generator().manual_seed(n1 + 3 * n2)
    P = 5
    u = torch.sort(torch.randn(P, n1, generator=gen), dim=1).values
    v = torch.sort(0.4 + 1.3 * torch.randn(P, n2, generator=gen), dim=1).values
    wpp, dist = ops.swd_quantile_cost(u.to(backend), v.to(backend), p)
    assert wpp.dtype == torch.float64 and dist.dtype == torch.float32 and dist.dim() == 0
    want = np.array([ref.wasserstein_1d_pp(a, b, p) for a, b in zip(u.numpy(), v.numpy())])
    rel = np.abs(wpp.cpu().numpy() - want) / want
    print(f"n1={n1} n2={n2} p={p}: max rel err {rel.max():.2e}")
    assert (rel <= 1e-6).all()
    want_dist = float(np.mean(want) ** (1.0 / p))
    assert abs(float(dist) - want_dist) <= 2e-6 * want_dist          # the same 1e-6, one root and one rounding to fp32 later


def test_quantile_cost_nan_and_symmetry(backend):
    gen = torch.Generator().manual_seed(2)
    u = torch.sort(torch.randn(3, 300, generator=gen), dim=1).values
    v = torch.sort(torch.randn(3, 211, generator=gen), dim=1).values
    a, da = ops.swd_quantile_cost(u.to(backend), v.to(backend), 2.0)
    b, db = ops.swd_quantile_cost(v.to(backend), u.to(backend), 2.0)
    assert torch.equal(a, b) and torch.equal(da, db)                  # the larger set always gets the threads
    u[1, -1] = float("nan")                                           # a sorted row with a NaN carries it last
    w, dist = ops.swd_quantile_cost(u.to(backend), v.to(backend), 2.0)
    w = w.cpu()
    assert torch.isnan(w[1]) and torch.isfinite(w[0]) and torch.isfinite(w[2]) and torch.isnan(dist.cpu())


# ------------------------------------------------------------------------------------------------ end to end
def clouds(n1, n2, d, gen):
    x1 = torch.randn(n1, d, generator=gen)
    x2 = 0.15 + 1.05 * torch.randn(n2, d, generator=gen)               # nearby Gaussians
    return x1, x2


@pytest.mark.parametrize("shape", ["equal", "unequal"])
def test_end_to_end_within_the_projection_bound(backend, shape):
    """p = 2, per projection: |wpp - exact| <= 4 delta W_1 + 4 delta^2 (tests/_swd_fp64.wpp_bound_p2) plus the cost kernel's own
    1e-6 relative (previous test).  One misplaced key moves wpp by about 1e-5 at these sizes."""
    gen = torch.Generator().manual_seed(11)
    d, P = 6, 50
    if backend.type == "cpu":
        n1, n2 = (3000, 3000) if shape == "equal" else (3000, 1801)
    else:
        n1, n2 = (50000, 50000) if shape == "equal" else (50000, 30011)
    x1, x2 = clouds(n1, n2, d, gen)
    dirs = torch.randn(d, P, generator=gen)
    dirs = dirs / dirs.norm(dim=0, keepdim=True)
    tl, _ = tile_of(backend)
    u1 = ops.segmented_sort(ops.swd_project(x1.to(backend), dirs.to(backend)), _tile_log2=tl)
    u2 = ops.segmented_sort(ops.swd_project(x2.to(backend), dirs.to(backend)), _tile_log2=tl)
    wpp, dist = ops.swd_quantile_cost(u1, u2, 2.0)
    want = ref.swd_wpp(x1.numpy(), x2.numpy(), dirs.numpy(), 2.0)
    bound = ref.wpp_bound_p2(x1.numpy(), x2.numpy(), dirs.numpy()) + 1e-6 * want
    err = np.abs(wpp.cpu().numpy() - want)
    print(f"{shape}: max err / bound = {float((err / bound).max()):.2e}")
    assert (err <= bound).all()
    # the composed op: same kernels (default tile), same value as its parts up to the tile-independent sort, and reproducible
    a = ops.sliced_wasserstein(x1.to(backend), x2.to(backend), dirs.to(backend), 2.0)
    b = ops.sliced_wasserstein(x1.to(backend), x2.to(backend), dirs.to(backend), 2.0)
    assert a.dim() == 0 and a.dtype == torch.float32 and a.device.type == backend.type
    assert torch.equal(a, b) and torch.equal(a, dist)
    assert abs(float(a) ** 2 - float(np.mean(want))) <= float(np.mean(bound)) + 2.0 ** -22 * float(np.mean(want))
