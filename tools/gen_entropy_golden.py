"""Writes tests/golden/ref_entropy_cov.npz from the reference's own CovarianceEntropyEstimator (mentflow/entropy.py, loaded by
path: the module needs numpy and torch only).

Needs the reference checkout (REF, as for oracle/gen_golden.py); it is not part of any test run.  The fixture holds inputs and
outputs only: per dimension d in (2, 6) a cloud x_d[2048, d] in fp32 (a sheared, shifted Gaussian), and H_d, dH_d[2048, d] =
the reference's forward and its autograd gradient evaluated in fp64 on exactly those fp32 values, plus the recorded
inspect.signature strings of the reference's estimator constructors.

    python tools/gen_entropy_golden.py
"""
import importlib.util
import inspect
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.gen_golden import REF  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_entropy_cov.npz")


def main():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_entropy", os.path.join(REF, "mentflow", "entropy.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    g = torch.Generator().manual_seed(20261017)
    arrays = {}
    for d in (2, 6):
        shear = torch.eye(d) + 0.35 * torch.randn(d, d, generator=g)
        shift = torch.randn(d, generator=g)
        x = (torch.randn(2048, d, generator=g) @ shear.T * 0.8 + shift).to(torch.float32)
        x64 = x.double().requires_grad_(True)
        H = ref.CovarianceEntropyEstimator()(x64)
        (dH,) = torch.autograd.grad(H, x64)
        arrays[f"x_{d}"] = x.numpy()
        arrays[f"H_{d}"] = H.detach().numpy()
        arrays[f"dH_{d}"] = dH.numpy()
    signatures = "\n".join(f"{name}{inspect.signature(getattr(ref, name).__init__)}"
                           for name in ("CovarianceEntropyEstimator", "KNNEntropyEstimator"))
    arrays["signatures"] = np.frombuffer(signatures.encode(), dtype=np.uint8)      # utf-8 bytes, one constructor per line
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT}  ({os.path.getsize(OUT) / 1024:.1f} KiB)")
    print(signatures)


if __name__ == "__main__":
    main()
