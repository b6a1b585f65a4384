"""The table-gradient kernel of classical MENT (mentflow_amd/csrc/ment_tabgrad.hip, ops.ment_logprob_table_grad) against the fp64
closed form of tests/_ment_tabgrad_fp64.py, on the emulator here and on the MI355X with -m gpu (the `backend` fixture).

Gate.  |L - L64|[e] <= 3e-4 (A[e] + max |weight|), A[e] = sum |weight_n| over the live points whose cell has e as a node, and
the same for grad_tab relative to tables[e].  Derivation: the fp32 grid position carries <= 1e-5 (docstring of
_ment_logp_fp64); rho = a (1 - w) / h has |d rho / dw| = a b / h^2 <= max / min of the cell's nodes, <= 8 for tables in
[0.25, 2]; so a point's responsibility is off by <= 8e-5 per unit weight, and 3e-4 is the gate the project already holds these
kernels to.  The fixed-point quantum (2^-50 of max |weight| per contribution) is far below that.  Rows within the band of
_ment_logp_fp64.ambiguous around a HULL END get weight 0 in the input (there fp32 and fp64 may disagree on whether the point is
inside at all); interior centres need no exclusion because rho is continuous across them.  Live rows come from the kernel's own
logp.  The measured maxima are printed."""
import pytest
import torch

from _ment_logp_fp64 import ambiguous
from _ment_tabgrad_fp64 import autograd64, closed_form64
from mentflow_amd import ops
from test_ment_logp_kernels import N, knot_problem, make_slots, problem, reference

TOL = 3.0e-4


def near_hull_end(x, slots):
    """Rows that _ment_logp_fp64.ambiguous puts within its band of the first or the last centre of some axis of some slot."""
    out = torch.zeros(x.shape[0], dtype=torch.bool)
    xd = x.double()
    for rows, coords, _ in slots:
        for r, c in zip(rows, coords):
            u = (xd @ r.double())[:, None]
            c = c.double()
            s = torch.round((u[:, 0] - c[0]) / ((c[-1] - c[0]) / (c.numel() - 1)))
            out |= ambiguous([c], u) & ((s == 0) | (s == c.numel() - 1))
    return out


def make_weight(x, slots, seed, positive=False):
    w = torch.randn(x.shape[0], generator=torch.Generator().manual_seed(seed))
    if positive:
        w = w.abs() + 0.01
    end = near_hull_end(x, slots)
    assert float(end.double().mean()) <= 0.01
    w[end] = 0.0
    return w


def run(dev, x, desc, meta, tab, weight, logp=None):
    x, desc, meta, tab = x.to(dev).contiguous(), desc.to(dev), meta.to(dev), tab.to(dev)
    if logp is None:
        logp = ops.ment_logprob(x, desc, meta, tab)[0]
    gl, gt = ops.ment_logprob_table_grad(x, desc, meta, tab, logp.to(dev), weight.to(dev))
    return logp.cpu(), gl.cpu(), gt.cpu()


def check_gate(gl, gt, x, slots, tab, logp, weight, what):
    live = torch.isfinite(logp) & (weight != 0)
    assert int(live.sum()) > 0.5 * x.shape[0]
    L64, A = closed_form64(x, slots, live, weight)
    bound = TOL * (A + float(weight[live].abs().max()))
    err = (gl.double() - L64).abs()
    pos = tab > 0
    err_tab = (gt.double()[pos] * tab.double()[pos] - L64[pos]).abs()
    print(what, {"grad_log": float((err / bound).max()), "grad_tab": float((err_tab / bound[pos]).max()),
                 "abs": float(err.max()), "largest": float(L64.abs().max())})
    assert torch.isfinite(gl).all() and torch.isfinite(gt).all()
    assert (err <= bound).all(), float((err / bound).max())
    assert (err_tab <= bound[pos]).all(), float((err_tab / bound[pos]).max())
    assert (gt[~pos] == 0).all()
    return L64


def test_closed_form_is_fp64_autograd():
    """The yardstick itself: the closed form equals fp64 autograd with the tables as leaves (expected ~1e-13; gate 1e-10), and
    the restated sum is that of _ment_logp_fp64.logp64."""
    for name, d in (("mixed8", 6), ("mixed8", 1), ("hundred", 6)):
        x, slots, desc, meta, tab, _ = problem(name, d)
        ref = reference(name, d, "none")[0]
        live = torch.isfinite(ref)
        w = torch.randn(N, generator=torch.Generator().manual_seed(d))
        L64, _ = closed_form64(x, slots, live, w)
        g, value = autograd64(x, slots, live, w)
        assert torch.equal(torch.isneginf(value), torch.isneginf(ref))
        assert float((value[live] - ref[live]).abs().max()) <= 1e-12
        err = float((g * tab.double() - L64).abs().max())
        print(name, d, err)
        assert err <= 1e-10


@pytest.mark.parametrize("d", [1, 2, 6, 8])
def test_mixed_slots_vs_fp64(backend, d):
    """Eight slots, 1-D and 2-D alternating, 16 .. 64 bins: the LDS instance; weights of both signs."""
    x, slots, desc, meta, tab, _ = problem("mixed8", d)
    assert desc.shape[0] * 28 + tab.numel() <= 10240, "this case is meant for the LDS instance"
    w = make_weight(x, slots, 100 + d)
    assert (w < 0).any() and (w > 0).any()
    logp, gl, gt = run(backend, x, desc, meta, tab, w)
    check_gate(gl, gt, x, slots, tab, logp, w, f"mixed8 d={d}")


def test_positive_weights(backend):
    d = 6
    x, slots, desc, meta, tab, _ = problem("mixed8", d)
    w = make_weight(x, slots, 7, positive=True)
    logp, gl, gt = run(backend, x, desc, meta, tab, w)
    check_gate(gl, gt, x, slots, tab, logp, w, "positive")
    assert (gl >= 0).all()
    # per 1-D slot the responsibilities of a point sum to 1: the slot's total is the total live weight
    live = torch.isfinite(logp)
    for nd, Bx, By, off in meta.tolist():
        total = float(gl[off:off + Bx * By].double().sum())
        assert abs(total - float(w[live].double().sum())) <= 1e-5 * float(w[live].sum())


def test_hundred_slots_takes_the_lds_instance(backend):
    """6-D, 100 1-D slots of 64 bins (the C4 measurement set): 9 200 floats, within the rule of the LDS instance."""
    d = 6
    x, slots, desc, meta, tab, _ = problem("hundred", d)
    assert desc.shape[0] * 28 + tab.numel() <= 10240         # the size rule of slot_geometry, which the launcher follows
    w = make_weight(x, slots, 11)
    logp, gl, gt = run(backend, x, desc, meta, tab, w)
    check_gate(gl, gt, x, slots, tab, logp, w, "hundred")


def test_tables_beyond_lds_take_the_global_instance(backend):
    """Three 64 x 64 slots, 12 288 floats: tables from global memory, integer atomics straight into the accumulator."""
    d = 6
    x, slots, desc, meta, tab, _ = problem("beyond_lds", d)
    assert desc.shape[0] * 28 + tab.numel() > 10240
    w = make_weight(x, slots, 12)
    logp, gl, gt = run(backend, x, desc, meta, tab, w)
    check_gate(gl, gt, x, slots, tab, logp, w, "beyond_lds")


def test_zero_weights_give_exact_zeros(backend):
    for name in ("mixed8", "beyond_lds"):
        x, slots, desc, meta, tab, _ = problem(name, 6)
        logp, gl, gt = run(backend, x, desc, meta, tab, torch.zeros(N))
        assert (gl == 0).all() and (gt == 0).all()


def test_tables_with_zero_entries(backend):
    """Eight 1-D slots with ~10 % of single entries zeroed.  grad_tab is 0 there and the rest stays within the gate: next to a
    zero node the other node's responsibility is exactly 1, so the bound on d rho / dw holds.  (In a 2-D cell with a zero node h
    tends to 0 towards that corner and the responsibilities of the other three vary without bound: a property of the function.)"""
    d = 6
    gen = torch.Generator().manual_seed(77)
    slots, desc, meta, tab = make_slots(d, [(1, 16 + 6 * k) for k in range(8)], gen)
    tab = tab.clone()
    zero = torch.rand(tab.numel(), generator=gen) < 0.10
    tab[zero] = 0.0
    slots = [(rows, coords, tab[off:off + Bx]) for (rows, coords, _), (nd, Bx, By, off) in zip(slots, meta.tolist())]
    x = 1.2 * torch.randn(N, d, generator=gen)
    w = make_weight(x, slots, 13)
    logp, gl, gt = run(backend, x, desc, meta, tab, w)
    assert 0.01 * N < int(torch.isneginf(logp).sum()) < 0.6 * N, "cells between two zeros put some rows outside the support"
    check_gate(gl, gt, x, slots, tab, logp, w, "zeros")
    assert int(zero.sum()) > 10 and (gt[zero] == 0).all() and (gl[zero] == 0).all()


def test_factor_on_the_upper_clamp_contributes_nothing(backend):
    c, t, desc, meta = knot_problem(backend)
    t = t.clone()
    t[10:13] = 3.0e10
    x = torch.tensor([[float(c[10])], [float(c[11]) + 0.03], [float(c[20]) + 0.03]])
    w = torch.tensor([1.5, -0.75, 2.0])
    logp, gl, gt = run(backend, x, desc.cpu(), meta.cpu(), t, w)
    assert torch.isfinite(logp).all()
    assert (gl[10:13] == 0).all() and (gt[10:13] == 0).all(), "h >= 1e10 is a constant"
    others = torch.ones(64, dtype=torch.bool)
    others[20:22] = False
    assert abs(float(gl[20] + gl[21]) - 2.0) <= 1e-6 and (gl[others] == 0).all()
    x2 = torch.tensor([[float(c[12]) + 0.12]])                    # h = 1.2e9: below the clamp, an ordinary cell
    logp, gl, gt = run(backend, x2, desc.cpu(), meta.cpu(), t, torch.ones(1))
    assert abs(float(gl[12] + gl[13]) - 1.0) <= 1e-6 and float(gl[12]) > 0.99


def test_rows_outside_the_support_are_ignored_whatever_their_weight(backend):
    d = 6
    x, slots, desc, meta, tab, _ = problem("mixed8", d)
    x = x[:900].clone()
    x[[3, 450, 899]] = 25.0
    w = make_weight(x, slots, 14)
    w[[3, 450, 899]] = 0.0
    base = run(backend, x, desc, meta, tab, w)
    assert torch.isneginf(base[0][[3, 450, 899]]).all()
    w2 = w.clone()
    w2[3], w2[450], w2[899] = float("nan"), 1.0e30, float("-inf")
    got = run(backend, x, desc, meta, tab, w2)
    assert torch.equal(got[1], base[1]) and torch.equal(got[2], base[2]) and torch.isfinite(got[1]).all()


def test_poison(backend):
    """A NaN logp with a non-zero weight, or a non-finite weight on a live row: all NaN through ops; a NaN row with weight 0 is
    masked by the caller and harmless."""
    d = 6
    x, slots, desc, meta, tab, _ = problem("mixed8", d)
    x = x[:700].clone()
    w = make_weight(x, slots, 15)
    base = run(backend, x, desc, meta, tab, w)
    y = x.clone()
    y[333, 2] = float("nan")
    logp, gl, gt = run(backend, y, desc, meta, tab, w)
    assert torch.isnan(logp[333]) and w[333] != 0
    assert torch.isnan(gl).all() and torch.isnan(gt).all()
    w0 = w.clone()
    w0[333] = 0.0
    logp, gl, gt = run(backend, y, desc, meta, tab, w0)
    assert torch.isfinite(gl).all() and torch.isfinite(gt).all()
    live = int(torch.isfinite(base[0]).nonzero()[5])
    for bad in (float("inf"), float("-inf"), float("nan")):
        wb = w.clone()
        wb[live] = bad
        logp, gl, gt = run(backend, x, desc, meta, tab, wb)
        assert torch.isnan(gl).all() and torch.isnan(gt).all(), bad
    logp, gl, gt = run(backend, x, desc, meta, tab, w)          # the status word is cleared by every call
    assert torch.equal(gl, base[1]) and torch.equal(gt, base[2])


def test_bitwise_reproducible_and_independent_of_row_order(backend):
    for name in ("hundred", "beyond_lds"):
        x, slots, desc, meta, tab, _ = problem(name, 6)
        w = make_weight(x, slots, 16)
        a = run(backend, x, desc, meta, tab, w)
        b = run(backend, x, desc, meta, tab, w)
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        perm = torch.randperm(N, generator=torch.Generator().manual_seed(17))
        c = run(backend, x[perm], desc, meta, tab, w[perm])
        assert torch.equal(c[0], a[0][perm])
        assert torch.equal(c[1], a[1]) and torch.equal(c[2], a[2])
        # a weight scale that is no power of two changes P and every contribution, not the gate
        check_gate(*run(backend, x, desc, meta, tab, 3.7e-9 * w)[1:], x, slots, tab, a[0], 3.7e-9 * w, name + " tiny weights")


def test_no_points_and_no_slots(backend):
    d = 3
    x, slots, desc, meta, tab, _ = problem("mixed8", 2)
    logp, gl, gt = run(backend, torch.zeros(0, 2), desc, meta, tab, torch.zeros(0))
    assert gl.shape == tab.shape and (gl == 0).all() and (gt == 0).all()
    desc0, meta0, tab0 = torch.zeros(0, 24), torch.zeros(0, 4, dtype=torch.int32), torch.zeros(1)
    x = torch.randn(300, d, generator=torch.Generator().manual_seed(1))
    logp, gl, gt = run(backend, x, desc0, meta0, tab0, torch.ones(300))
    assert (gl == 0).all() and (gt == 0).all()


def test_argument_checks(backend):
    d = 2
    x, slots, desc, meta, tab, _ = problem("mixed8", d)
    dev = backend
    x, desc, meta, tab = x.to(dev), desc.to(dev), meta.to(dev), tab.to(dev)
    lp, w = torch.zeros(N, device=dev), torch.ones(N, device=dev)
    with pytest.raises(RuntimeError, match="float32"):
        ops.ment_logprob_table_grad(x.double(), desc, meta, tab, lp, w)
    with pytest.raises(RuntimeError, match="float32"):
        ops.ment_logprob_table_grad(x, desc, meta, tab, lp, w.double())
    with pytest.raises(RuntimeError, match="d <= 8"):
        ops.ment_logprob_table_grad(torch.zeros(4, 9, device=dev), desc, meta, tab, lp[:4], w[:4])
    with pytest.raises(RuntimeError, match="meta"):
        ops.ment_logprob_table_grad(x, desc, meta.long(), tab, lp, w)
    with pytest.raises(RuntimeError, match="weight"):
        ops.ment_logprob_table_grad(x, desc, meta, tab, lp, w[:-1])
    with pytest.raises(RuntimeError, match="slots"):              # the library's own refusal: more than 512 slots
        ops.ment_logprob_table_grad(x, torch.zeros(513, 24, device=dev), torch.zeros(513, 4, dtype=torch.int32, device=dev), tab,
                                    lp, w)
