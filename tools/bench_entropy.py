"""Time the sample-based entropy estimators (mentflow_amd.ops.knn_entropy / cov_entropy) on the GPU for the shapes of
DESIGN.md §6d: d = 6, k = 5, N = 25 000 (the reference's training batch) and 100 000 (its epoch-end evaluation).

Per shape: `--warmup` untimed calls (code objects loaded, allocator warm), then `--repeats` calls timed with HIP events on the
current stream (median, min, max) of: the k-NN estimator forward and forward + backward, the covariance estimator forward and
forward + backward, and the k-NN estimate composed from torch ops on the same GPU — torch.cdist (its default, matrix-product
form, the faster one) + topk(k + 1, smallest) over row chunks of 4096 so that the N x N distances never exist at once, forward
and forward + backward through autograd (one backward per chunk).  A last record times one training step (loss + backward +
AdamW) of the `examples/train_rec_2d_nonlinear.py --gen nn` problem at 25 000 particles with and without `--entropy knn`;
the difference is the estimator's share of the step.  Each record runs in a child process of its own under a time limit; a child that fails or
runs out of time ends the run (nothing else is started on the GPU).  Writes <out>/knn_entropy_bench.json.

    python tools/bench_entropy.py --out profiles [--only 25000] [--repeats 20]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mentflow_amd import ops  # noqa: E402

# name: (N, d, k, time limit of the child in seconds)
SHAPES = {
    "batch_25000": (25_000, 6, 5, 240),
    "eval_100000": (100_000, 6, 5, 420),
    "train_step_nn_25000": (25_000, 2, 5, 300),
}
TORCH_ROWS = 4096


def spread(values):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4), n=len(v))


def timed(fn, warmup, repeats):
    """HIP-event time of each of `repeats` calls, in ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in pairs]


def torch_sum_ln_rho(x, k):
    """sum_i ln rho_k(i) from torch ops, row chunks of TORCH_ROWS.  Timed for comparison; its value is a sanity figure, not a
    check: under cdist's matrix-product form the distance of a point to itself is not exactly 0, so a very close neighbour can
    sort ahead of it and entry k of topk(k + 1) is then not the k-th other point."""
    total = x.new_zeros(())
    for a in range(0, x.shape[0], TORCH_ROWS):
        dist = torch.cdist(x[a:a + TORCH_ROWS], x)
        rho = torch.topk(dist, k + 1, dim=1, largest=False).values[:, k]        # the nearest is the point itself
        total = total + torch.log(rho).sum()
    return total


def torch_fwd_bwd(x, k):
    """The same with the gradient, one backward per row chunk so that only one chunk of distances is alive at a time."""
    x.grad = None
    for a in range(0, x.shape[0], TORCH_ROWS):
        dist = torch.cdist(x[a:a + TORCH_ROWS], x)
        rho = torch.topk(dist, k + 1, dim=1, largest=False).values[:, k]
        torch.log(rho).sum().backward()


def with_backward(fn, x):
    def step():
        x.grad = None
        fn(x).backward()
    return step


def run_shape(name, warmup, repeats):
    n, d, k, _ = SHAPES[name]
    dev = torch.device("cuda", 0)
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(0)).to(dev)
    xg = x.clone().requires_grad_(True)
    rec = dict(shape=name, n=n, d=d, k=k)
    H = ops.knn_entropy(x, k)
    S_torch = torch_sum_ln_rho(x, k)
    rec["sum_ln_rho_library"] = float(H[3])
    rec["sum_ln_rho_torch"] = float(S_torch)
    rec["knn_fwd_ms"] = spread(timed(lambda: ops.knn_entropy(x, k), warmup, repeats))
    rec["knn_fwd_bwd_ms"] = spread(timed(with_backward(lambda t: ops.knn_entropy(t, k)[0], xg), warmup, repeats))
    rec["cov_fwd_ms"] = spread(timed(lambda: ops.cov_entropy(x), warmup, repeats))
    rec["cov_fwd_bwd_ms"] = spread(timed(with_backward(ops.cov_entropy, xg), warmup, repeats))
    t_rep = max(3, repeats // 4)                             # the torch composition takes tens of milliseconds per call
    rec["torch_fwd_ms"] = spread(timed(lambda: torch_sum_ln_rho(x, k), 2, t_rep))
    rec["torch_fwd_bwd_ms"] = spread(timed(lambda: torch_fwd_bwd(xg, k), 2, t_rep))
    rec["torch_chunk_bytes"] = 4 * TORCH_ROWS * n
    rec["library_workspace_bytes"] = int(ops._lib.get_lib().mf_knn_entropy_ws_bytes(n, d, k, 0))
    rec["knn_over_torch_fwd"] = round(rec["knn_fwd_ms"]["median"] / rec["torch_fwd_ms"]["median"], 4)
    rec["knn_over_torch_fwd_bwd"] = round(rec["knn_fwd_bwd_ms"]["median"] / rec["torch_fwd_bwd_ms"]["median"], 4)
    return rec


def run_train_step(name, warmup, repeats):
    from mentflow_amd.harness import build_problem
    n = SHAPES[name][0]
    dev = torch.device("cuda", 0)
    rec = dict(shape=name, n=n, d=2, k=5)
    for est in ("none", "knn"):
        prob = build_problem(ndim=2, num=4, bins=85, xmax=4.5, seed=21, device=dev, dist_name="rings", meas_samples=1_000_000,
                             optics="2d_nonlinear", gen_name="nn", hidden_layers=3, hidden_units=50, discrepancy="mae",
                             entropy_estimator=est)
        model = prob.model
        model.penalty_parameter = 500.0
        opt = torch.optim.AdamW(model.parameters(), lr=1e-2, weight_decay=0.0)

        def step():
            opt.zero_grad()
            L, _, _ = model.loss(n)
            L.backward()
            opt.step()
        rec[f"step_{est}_ms"] = spread(timed(step, warmup, repeats))
    rec["knn_share_of_step"] = round(1.0 - rec["step_none_ms"]["median"] / rec["step_knn_ms"]["median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--shape", default="", help="(internal) run this one shape in this process and print its record")
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be at least 3")
    if args.shape:
        from mentflow_amd import _lib
        _lib.use_library(_lib.DEFAULT_PATH)
        fn = run_train_step if args.shape.startswith("train_step") else run_shape
        print(json.dumps(fn(args.shape, args.warmup, args.repeats)), flush=True)
        return 0
    recs = []
    for name, shape in SHAPES.items():
        if args.only and args.only not in name:
            continue
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--repeats", str(args.repeats),
                                    "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=shape[-1])
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {shape[-1]} s; stopping", file=sys.stderr)
            return 1
        if child.returncode != 0:
            print(f"{name}: exit status {child.returncode}; stopping\n{child.stderr[-2000:]}", file=sys.stderr)
            return 1
        line = child.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        recs.append(json.loads(line))
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "knn_entropy_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), warmup=args.warmup, repeats=args.repeats, shapes=recs), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
