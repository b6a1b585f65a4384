"""Time the sliced Wasserstein distance (mentflow_amd.ops.sliced_wasserstein) on the GPU for the shapes of DESIGN.md §6c.

Per shape: one untimed call first (code objects loaded, allocator warm), then `--repeats` timed calls (device-synchronised wall
time; median, min, max), the HIP-event time of each of the three stages (projection, segmented sort, quantile cost; median over
the timed calls), and the same computation composed from torch ops on the same GPU (matmul, torch.sort(dim=0), elementwise,
mean) timed the same way.  Each shape runs in a child process of its own under a time limit; a child that fails or runs out of
time ends the run (nothing else is started on the GPU).  Writes <out>/swd_bench.json and prints one line per shape.

    python tools/bench_swd.py --out profiles [--only eval] [--repeats 5]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mentflow_amd import ops  # noqa: E402

STAGES = ("swd_project", "segmented_sort", "swd_quantile_cost")
# name: (N1, N2, d, P, time limit of the child in seconds)
SHAPES = {
    "eval_50k_50k": (50_000, 50_000, 6, 50, 120),           # experiments/*/setup.py::setup_eval
    "truth_1M_1M": (1_000_000, 1_000_000, 6, 50, 180),      # the size of the reference's ground-truth sets
    "unequal_50k_30011": (50_000, 30_011, 6, 50, 120),
}


class StageTimer:
    """Wraps the ops.swd_* entry points with HIP events for the duration of a `with` block."""

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


def torch_swd(x1, x2, dirs):
    """The same distance (p = 2) from torch ops in fp32."""
    s1 = torch.sort(torch.matmul(x1, dirs), dim=0).values
    s2 = torch.sort(torch.matmul(x2, dirs), dim=0).values
    n, m = s1.shape[0], s2.shape[0]
    if n == m:
        wpp = torch.mean(torch.square(s1 - s2), dim=0)
    else:                                                     # merged quantile breakpoints in units of 1 / (n m)
        bu = torch.arange(1, n + 1, device=x1.device, dtype=torch.int64) * m
        bv = torch.arange(1, m + 1, device=x1.device, dtype=torch.int64) * n
        b = torch.unique(torch.cat([bu, bv]))
        w = (torch.diff(b, prepend=b.new_zeros(1)).double() / (float(n) * float(m))).float()
        wpp = torch.sum(w[:, None] * torch.square(s1[(b - 1) // m] - s2[(b - 1) // n]), dim=0)
    return torch.sqrt(torch.mean(wpp))


def spread(values):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4), n=len(v))


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


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
    lib_value = float(ops.sliced_wasserstein(x1, x2, dirs, 2.0))          # untimed first calls
    torch_value = float(torch_swd(x1, x2, dirs))
    lib_ms = timed(lambda: ops.sliced_wasserstein(x1, x2, dirs, 2.0), repeats)
    torch_ms = timed(lambda: torch_swd(x1, x2, dirs), repeats)
    stages = {k: [] for k in STAGES}
    for _ in range(repeats):
        with StageTimer() as st:
            ops.sliced_wasserstein(x1, x2, dirs, 2.0)
        for k, v in st.report().items():
            stages[k].append(v)
    rec = dict(shape=name, n1=n1, n2=n2, d=d, projections=P, p=2, library_ms=spread(lib_ms), torch_ms=spread(torch_ms),
               stages_ms={k: spread(v) for k, v in stages.items()}, library_value=lib_value, torch_value=torch_value,
               library_over_torch=round(spread(lib_ms)["median"] / spread(torch_ms)["median"], 3))
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
    with open(os.path.join(args.out, "swd_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), shapes=recs), f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
