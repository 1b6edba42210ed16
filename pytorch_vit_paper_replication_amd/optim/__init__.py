"""Optimizers and schedules (reference recipe: MAIN.ipynb:2792-2960)."""
from .adam import FusedAdam
from .ema import ModelEma
from .lamb import FusedLamb
from .schedule import param_groups_weight_decay, warmup_cosine_decay, warmup_decay_steps, warmup_linear_decay
from .sgd import FusedSGD

__all__ = ["FusedAdam", "FusedLamb", "FusedSGD", "ModelEma", "param_groups_weight_decay", "warmup_cosine_decay", "warmup_decay_steps",
           "warmup_linear_decay"]
