"""Model evaluator — the body of the reference's per-experiment ``setup_eval`` (experiments/rec_nd_1d/setup.py:118-159; its
mentflow/train/eval.py is empty) as one callable for ``Trainer(eval=...)`` and ``MENTTrainer(eval=...)``."""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import simulate
from .loss import kl_divergence
from .utils import unravel


class Evaluator:
    """``Evaluator(size, ...)(model) -> {"discrepancy": float, "distance": float | None}``.

    Draws ``size`` samples from the model (a ``MENTFlow`` or a ``MENT``: anything with ``sample``, ``transforms``,
    ``diagnostics`` and ``measurements``), simulates the measurements and averages ``discrepancy(prediction, measurement)`` over
    them (setup.py:122-134); with a ``distance`` (e.g. ``loss.SlicedWassersteinDistance``) and a ground-truth
    ``distribution`` it also returns the distance between the samples and ``distribution.sample(size)`` (setup.py:136-148).
    ``verbose`` prints both numbers as the reference does."""

    def __init__(self, size: int, discrepancy: Callable = kl_divergence, distance: Optional[Callable] = None,
                 distribution=None) -> None:
        if distance is not None and distribution is None:
            raise ValueError("a distance needs the ground-truth distribution to draw from")
        self.size = int(size)
        self.discrepancy = discrepancy
        self.distance = distance
        self.distribution = distribution
        self.verbose = True

    def __call__(self, model) -> dict:
        with torch.no_grad():
            x_pred = model.sample(self.size).type(torch.float32)
            predictions = simulate.forward(x_pred, model.transforms, model.diagnostics)
            values = [self.discrepancy(y_pred, y_meas).float()
                      for y_pred, y_meas in zip(unravel(predictions), unravel(model.measurements))]
            discrepancy = float(torch.stack(values).mean())
            distance = None
            if self.distance is not None:
                x_true = self.distribution.sample(self.size).type(torch.float32).to(x_pred.device)
                distance = float(self.distance(x_pred[:self.size, :], x_true[:self.size, :]))
        if self.verbose:
            print("disc(y_model, y_true) = {}".format(discrepancy))
            if distance is not None:
                print("dist(x_model, x_true) = {}".format(distance))
        return {"discrepancy": discrepancy, "distance": distance}
