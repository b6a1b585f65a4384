"""mentflow_amd — MI355X (gfx950) implementation of the MENT-Flow training-step hot path.

Same public names as the reference package ``mentflow`` for the hot path:
``MENTFlow``, ``generate``, ``simulate``, ``diagnostics``, ``entropy``, ``prior``, ``loss``, ``train``, ``utils``, and the
classical MENT solver: ``ment``, ``sample`` (``train.MENTTrainer``); ``evaluate.Evaluator`` is the reference's per-experiment
``setup_eval`` as one class.
Compute = hand-written HIP kernels behind the C ABI in include/mentflow_hip.h; no CPU fallback.
"""
from .core import MENTFlow
from . import diagnostics
from . import dist
from . import entropy
from . import evaluate
from . import generate
from . import graph
from . import loss
from . import ment
from . import ops
from . import prior
from . import sample
from . import simulate
from . import train
from . import utils
from .evaluate import Evaluator
from .utils import unravel
