"""The table gradient of classical MENT on the MI355X only: a forward + backward into the tables captured in a graph (a linear
stream, no parallel branches) that replays bit for bit, which shows that the path has no host synchronisation; and one launch of
the C4 shape (6-D, 100 slots x 64 bins, 2 097 152 points) against the fp64 closed form on a 262 144-point subset: rows outside
the subset get weight 0, so the kernel runs the full shape and the reference only the subset.  Gate and hull-end rule:
tests/test_ment_tabgrad_kernels.py."""
import pytest
import torch

from test_ment_logp_kernels import MIXED8, make_slots
from test_ment_tabgrad_kernels import check_gate, near_hull_end

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev():
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    return torch.device("cuda", 0)


def test_graphed_forward_and_table_backward_replays_bitwise(dev):
    from mentflow_amd import ops
    d, n = 6, 20000
    gen = torch.Generator().manual_seed(21)
    slots, desc, meta, tab = make_slots(d, MIXED8, gen)
    desc, meta = desc.to(dev), meta.to(dev)
    x = (1.2 * torch.randn(n, d, generator=gen)).to(dev)
    w = torch.randn(n, generator=gen).to(dev)
    tables = tab.to(dev).requires_grad_(True)
    prior = (1, 2.0, 0.0)

    def step():
        lp = ops.MentLogProbFn.apply(x, desc, meta, tables, prior)
        (g,) = torch.autograd.grad((torch.where(torch.isfinite(lp), lp, torch.zeros_like(lp)) * w).sum(), tables)
        return g

    eager = step().clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    first = out.clone()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(first).all() and float(first.abs().max()) > 0
    assert torch.equal(first, out) and torch.equal(first, eager)
    # new inputs in the captured buffers: the replay follows them, poison included
    row = int(torch.isfinite(ops.ment_logprob(x, desc, meta, tab.to(dev), prior)[0]).nonzero()[0])
    with torch.no_grad():
        w[row] = float("inf")
    graph.replay()
    assert torch.isnan(out).all()


def test_c4_shape_against_fp64_on_a_subset(dev):
    from mentflow_amd import ops
    d, n, sub = 6, 2097152, 262144
    gen = torch.Generator().manual_seed(64)
    slots, desc, meta, tab = make_slots(d, [(1, 64)] * 100, gen)
    x = 1.2 * torch.randn(n, d, generator=gen)
    idx = torch.randperm(n, generator=gen)[:sub]
    ws = torch.randn(sub, generator=gen)
    end = near_hull_end(x[idx], slots)
    assert float(end.double().mean()) <= 0.01
    ws[end] = 0.0
    w = torch.zeros(n)
    w[idx] = ws
    xd, dd, md, td = x.to(dev), desc.to(dev), meta.to(dev), tab.to(dev)
    logp = ops.ment_logprob(xd, dd, md, td)[0]
    gl, gt = ops.ment_logprob_table_grad(xd, dd, md, td, logp, w.to(dev))
    gl2, gt2 = ops.ment_logprob_table_grad(xd, dd, md, td, logp, w.to(dev))
    assert torch.equal(gl, gl2) and torch.equal(gt, gt2)
    check_gate(gl.cpu(), gt.cpu(), x[idx], slots, tab, logp.cpu()[idx], ws, "c4")
