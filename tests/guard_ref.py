"""A torch restatement of ubpl_grad_guard (include/ubpl_hip.h), shared by the
guard tests: squares and their sum in float64, the coefficient of
torch.nn.utils.clip_grad_norm_ in float64 rounded once to float32."""
import math

import numpy as np
import torch


def guard_ref(g, max_norm):
    """g: float32 tensor -> (c float32, norm float32, skip bool)."""
    total = float((g.detach().double().cpu() ** 2).sum())
    skip = not math.isfinite(total)
    norm = math.sqrt(total) if total == total and total >= 0 else float("nan")
    c = 1.0
    if not skip and max_norm > 0:
        c = min(1.0, max_norm / (norm + 1e-6))
    return np.float32(c), np.float32(norm), skip
