"""Time forward + backward of the differentiable sliced Wasserstein distance (mentflow_amd.ops.SlicedWassersteinFn) on the GPU
for the shapes of DESIGN.md §6c, in the manner of tools/bench_swd.py.

Per shape and per mode (gradient to x1 only, gradient to both clouds): one untimed call first, then `--repeats` timed calls of
forward + backward (device-synchronised wall time; median, min, max), the HIP-event time of every stage (median over the timed
calls), and the same computation composed from torch ops with autograd on the same GPU (matmul, torch.sort, gather, mean,
.backward()) timed the same way.  The quantile breakpoints of the unequal shape are built once, outside the timed region, in
the composition's favour.  The pair sort is also timed alone for the tiles 2^10 .. 2^12.  Each shape runs in a child process
of its own under a time limit; a child that fails or runs out of time ends the run (nothing else is started on the GPU).
Writes <out>/swd_grad_bench.json and prints one line per shape.

    python tools/bench_swd_grad.py --out profiles [--only equal] [--repeats 5]
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
from tools.bench_swd import spread, timed  # noqa: E402

STAGES = ("swd_project", "segmented_sort", "segmented_sort_pairs", "swd_quantile_cost", "swd_quantile_cost_bwd", "swd_project_bwd")
# name: (N1, N2, d, P, time limit of the child in seconds)
SHAPES = {
    "equal_50k_50k": (50_000, 50_000, 6, 50, 180),
    "unequal_50k_30011": (50_000, 30_011, 6, 50, 180),
}


class StageTimer:
    """Wraps the ops entry points named in STAGES with HIP events for the duration of a `with` block (the autograd function
    looks them up in the module at call time)."""

    def __init__(self):
        self.events = {k: [] for k in STAGES}
        self.saved = {}

    def __enter__(self):
        for name in STAGES:
            fn = getattr(ops, name)
            self.saved[name] = fn

            def wrapped(*a, _fn=fn, _name=name, **k):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = _fn(*a, **k)
                e1.record()
                self.events[_name].append((e0, e1))
                return out
            setattr(ops, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(ops, name, fn)

    def report(self):
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.events.items()}


def torch_pieces(n, m, dev):
    """(weights, rank of x1's projection, rank of x2's projection) of the quantile pieces; None for equal sizes."""
    if n == m:
        return None
    bu = torch.arange(1, n + 1, device=dev, dtype=torch.int64) * m
    bv = torch.arange(1, m + 1, device=dev, dtype=torch.int64) * n
    b = torch.unique(torch.cat([bu, bv]))
    w = (torch.diff(b, prepend=b.new_zeros(1)).double() / (float(n) * float(m))).float()
    return w, (b - 1) // m, (b - 1) // n


def torch_swd(x1, x2, dirs, pieces):
    """The same distance (p = 2) from torch ops in fp32, with a graph."""
    s1 = torch.sort(torch.matmul(x1, dirs), dim=0).values
    s2 = torch.sort(torch.matmul(x2, dirs), dim=0).values
    if pieces is None:
        wpp = torch.mean(torch.square(s1 - s2), dim=0)
    else:
        w, i1, i2 = pieces
        wpp = torch.sum(w[:, None] * torch.square(s1[i1] - s2[i2]), dim=0)
    return torch.sqrt(torch.mean(wpp))


def step(fn, x1, x2, both):
    a = x1.detach().requires_grad_()
    b = x2.detach().requires_grad_() if both else x2
    value = fn(a, b)
    value.backward()
    return value.detach(), a.grad, (b.grad if both else None)


def run(name, repeats):
    from mentflow_amd import _lib
    _lib.use_library(_lib.DEFAULT_PATH)
    n1, n2, d, P, _ = SHAPES[name]
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    x1 = torch.randn(n1, d, generator=gen).to(dev)
    x2 = (0.15 + 1.05 * torch.randn(n2, d, generator=gen)).to(dev)
    dirs = torch.randn(d, P, generator=gen)
    dirs = (dirs / dirs.norm(dim=0, keepdim=True)).to(dev)
    pieces = torch_pieces(n1, n2, dev)
    lib = lambda a, b: ops.SlicedWassersteinFn.apply(a, b, dirs, 2.0)          # noqa: E731
    comp = lambda a, b: torch_swd(a, b, dirs, pieces)                          # noqa: E731
    rec = dict(shape=name, n1=n1, n2=n2, d=d, projections=P, p=2, modes={})
    for mode, both in (("grad_x1", False), ("grad_both", True)):
        lv, lg, _ = step(lib, x1, x2, both)                    # untimed first calls
        tv, tg, _ = step(comp, x1, x2, both)
        lib_ms = timed(lambda: step(lib, x1, x2, both), repeats)
        torch_ms = timed(lambda: step(comp, x1, x2, both), repeats)
        stages = {k: [] for k in STAGES}
        for _ in range(repeats):
            with StageTimer() as st:
                step(lib, x1, x2, both)
            for k, v in st.report().items():
                stages[k].append(v)
        rec["modes"][mode] = dict(
            library_ms=spread(lib_ms), torch_ms=spread(torch_ms), stages_ms={k: spread(v) for k, v in stages.items()},
            library_value=float(lv), torch_value=float(tv),
            max_grad_difference_over_max_grad=float((lg - tg).abs().max() / tg.abs().max()),
            library_over_torch=round(spread(lib_ms)["median"] / spread(torch_ms)["median"], 3))
    # the pair sort alone, per tile: all 2P rows of the equal shape / the P rows of the larger cloud
    rows = 2 * P if n1 == n2 else P
    keys = torch.randn(rows, n1, generator=gen).to(dev)
    sweep = {}
    for tl in (10, 11, 12):
        ops.segmented_sort_pairs(keys, _tile_log2=tl)
        sweep[f"2^{tl}"] = spread(timed(lambda: ops.segmented_sort_pairs(keys, _tile_log2=tl), repeats))
    ops.segmented_sort(keys)
    sweep["keys_only_2^12"] = spread(timed(lambda: ops.segmented_sort(keys), repeats))
    rec["pair_sort_ms_by_tile"] = dict(rows=rows, n=n1, **sweep)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles")
    ap.add_argument("--only", default="")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", default="", help="(internal) run this one shape in this process and print its record")
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats must be at least 3")
    if args.shape:
        run(args.shape, args.repeats)
        return 0
    recs = []
    for name, shape in SHAPES.items():
        if args.only and args.only not in name:
            continue
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name, "--repeats", str(args.repeats)],
                                   capture_output=True, text=True, timeout=shape[-1])
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
    with open(os.path.join(args.out, "swd_grad_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), shapes=recs), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
