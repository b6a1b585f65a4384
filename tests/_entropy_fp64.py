"""fp64 restatement of the Kozachenko-Leonenko k-nearest-neighbour entropy estimate (test infrastructure).  The reference
declares the estimator without a forward, so this file is the normative definition the kernels are tested against:

    H = -[psi(N) - psi(k) + ln c_d + (d / N) sum_i ln rho_k(i)],   c_d = pi^(d/2) / Gamma(d/2 + 1),
    rho_k(i) = Euclidean distance of x_i to its k-th nearest OTHER point, neighbours ordered by (rho^2, index),
    ln rho = 0.5 ln max(rho^2, FLT_MIN)  (a floored term has zero gradient),

with squared distances formed from direct differences in fp64.  tests/test_entropy_kernels.py pins it to
scipy.spatial.cKDTree, to a case done by hand and to torch autograd through cdist / topk."""
import numpy as np
from scipy.special import digamma, gammaln

FLT_MIN = float(np.finfo(np.float32).tiny)


def sqdist_rows(x, rows):
    """[len(rows), N] squared distances from direct differences (fp64)."""
    x = np.asarray(x, dtype=np.float64)
    diff = x[rows][:, None, :] - x[None, :, :]
    return np.einsum("inc,inc->in", diff, diff)


def kth_neighbours_tree(x, k, extra=8):
    """kth_neighbours for large N: a k-d tree proposes the k + extra nearest other points, whose squared distances are then
    formed anew from direct differences and ordered by (rho^2, index).  Equal to the dense search unless more than `extra`
    further points tie with the k-th distance (asserted)."""
    from scipy.spatial import cKDTree
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    m = min(n, k + extra + 1)
    _, cand = cKDTree(x).query(x, k=m, workers=-1)
    cand = cand.reshape(n, m)
    diff = x[:, None, :] - x[cand]
    d2 = np.einsum("nmc,nmc->nm", diff, diff)
    d2[cand == np.arange(n)[:, None]] = np.inf
    order = np.lexsort((cand, d2), axis=1)
    rows = np.arange(n)
    idx = cand[rows, order[:, k - 1]]
    rho2 = d2[rows, order[:, k - 1]]
    if m < n:
        assert np.all(d2[rows, order[:, m - 2]] > rho2), "more ties with the k-th distance than candidates were proposed"
    return idx.astype(np.int64), rho2


def kth_neighbours(x, k, block=None):
    """(idx[N], rho2[N]): the k-th nearest other point under the (rho^2, index) order and its squared distance.  Dense search
    over all pairs up to 8192 points, the k-d tree variant beyond."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    assert n > k >= 1
    if n > 8192:
        return kth_neighbours_tree(x, k)
    block = block or max(1, int(2e7) // (n * x.shape[1]))
    idx = np.empty(n, dtype=np.int64)
    rho2 = np.empty(n, dtype=np.float64)
    for a in range(0, n, block):
        rows = np.arange(a, min(n, a + block))
        d2 = sqdist_rows(x, rows)
        d2[np.arange(rows.size), rows] = np.inf                       # not its own neighbour
        order = np.lexsort((np.broadcast_to(np.arange(n), d2.shape), d2), axis=1)   # by rho^2, then by index
        idx[rows] = order[:, k - 1]
        rho2[rows] = d2[np.arange(rows.size), idx[rows]]
    return idx, rho2


def constant(n, d, k):
    """psi(N) - psi(k) + ln c_d"""
    return float(digamma(n) - digamma(k) + 0.5 * d * np.log(np.pi) - gammaln(0.5 * d + 1.0))


def ln_rho(rho2):
    return 0.5 * np.log(np.maximum(np.asarray(rho2, dtype=np.float64), FLT_MIN))


def entropy_from(rho2, d, k):
    n = len(rho2)
    return -(constant(n, d, k) + d / n * float(np.sum(ln_rho(rho2))))


def knn_entropy(x, k):
    """(H, idx, rho2) in fp64."""
    x = np.asarray(x, dtype=np.float64)
    idx, rho2 = kth_neighbours(x, k)
    return entropy_from(rho2, x.shape[1], k), idx, rho2


def grad_terms(x, idx):
    """Closed-form d(sum_i ln rho_i)/dx for GIVEN k-th neighbours idx: (grad[N, d], absgrad[N, d], count[N]) with absgrad the sum
    of the absolute values of a row's terms and count their number.  Term of pair (i, j = idx[i]): (x_i - x_j) / rho^2 on row
    i, its negative on row j; zero where rho^2 <= FLT_MIN."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    diff = x - x[idx]
    r2 = np.einsum("nc,nc->n", diff, diff)
    w = np.where(r2 > FLT_MIN, 1.0 / np.where(r2 > FLT_MIN, r2, 1.0), 0.0)
    t = diff * w[:, None]
    grad = t.copy()
    absg = np.abs(t)
    count = np.ones(n, dtype=np.int64)
    np.add.at(grad, idx, -t)
    np.add.at(absg, idx, np.abs(t))
    np.add.at(count, idx, 1)
    return grad, absg, count


def knn_entropy_grad(x, k):
    """dH/dx in fp64 with the restatement's own neighbours."""
    x = np.asarray(x, dtype=np.float64)
    idx, _ = kth_neighbours(x, k)
    return -(x.shape[1] / x.shape[0]) * grad_terms(x, idx)[0]
