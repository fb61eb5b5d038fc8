"""Optimizer kernels (E1): EMA, AdamW and its device-step, EMA-fused and guarded forms, the
gradient guard.  The *_dev_ steps check nothing: they are host work per launch in the eager step."""
import torch

from .. import _lib
from . import _check


def ema_update_(ema, p, alpha):
    _check._chk(ema, "ema")
    _check._chk(p, "param")
    assert ema.numel() == p.numel()
    _lib.call("ubpl_ema_update", ema, p, ema.numel(), float(alpha))


def adamw_step_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _check._chk(t, n)
    _lib.call("ubpl_adamw_step", p, g, m, v, p.numel(), float(lr), float(beta1), float(beta2), float(eps),
              float(weight_decay), int(step))


def adamw_step_dev_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step_t, coef):
    """AdamW with the step count in device memory (int64 scalar, incremented);
    replayable inside a captured HIP graph.  coef: 4-float scratch."""
    _lib.call("ubpl_adamw_step_dev", p, g, m, v, p.numel(), float(lr), float(beta1), float(beta2), float(eps),
              float(weight_decay), step_t, coef)


def adamw_ema_step_dev_(p, g, m, v, nlive, lr, beta1, beta2, eps, weight_decay, step_t, coef, ema, alpha):
    """adamw_step_dev_ on p[:nlive] and ema_update_(ema, p, alpha) over all of p, one pass."""
    if ema.numel() != p.numel() or nlive > p.numel():
        raise ValueError("adamw_ema_step_dev_: ema / p / nlive sizes disagree")
    _lib.call("ubpl_adamw_ema_step_dev", p, g, m, v, int(nlive), float(lr), float(beta1), float(beta2), float(eps),
              float(weight_decay), step_t, coef, ema, p.numel(), float(alpha))


def scale_(x, s):
    _check._chk(x, "x")
    _lib.call("ubpl_scale_", x, x.numel(), float(s))


def grad_guard_scratch(n, device):
    """The f64 scratch grad_guard_ needs for a gradient of n floats."""
    return torch.zeros(int(_lib.lib().ubpl_grad_guard_scratch(int(n))), dtype=torch.float64, device=device)


def grad_guard_(g, max_norm, part, guard):
    """guard[4] = {clip coefficient, L2 norm, skip, 0} of the flat gradient g (numel a
    multiple of 4, 16-B aligned): clip_grad_norm_'s coefficient for max_norm (<= 0: no
    clipping), skip = 1.0 iff some element is inf or NaN.  part: grad_guard_scratch."""
    _check._chk(g, "g")
    _lib.call("ubpl_grad_guard", g, g.numel(), float(max_norm), part, guard)


def adamw_step_guarded_dev_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step_t, coef, guard, skipped):
    """adamw_step_dev_ on g * guard[0]; a no-op but for skipped[2] (int64: total,
    consecutive) when guard[2] is set."""
    _lib.call("ubpl_adamw_step_guarded_dev", p, g, m, v, p.numel(), float(lr), float(beta1), float(beta2),
              float(eps), float(weight_decay), step_t, coef, guard, skipped)


def adamw_ema_step_guarded_dev_(p, g, m, v, nlive, lr, beta1, beta2, eps, weight_decay, step_t, coef, ema, alpha,
                                guard, skipped):
    """adamw_ema_step_dev_ under a guard: on a skipped step only the EMA half runs."""
    if ema.numel() != p.numel() or nlive > p.numel():
        raise ValueError("adamw_ema_step_guarded_dev_: ema / p / nlive sizes disagree")
    _lib.call("ubpl_adamw_ema_step_guarded_dev", p, g, m, v, int(nlive), float(lr), float(beta1), float(beta2),
              float(eps), float(weight_decay), step_t, coef, ema, p.numel(), float(alpha), guard, skipped)


def restore_if_(dst, saved, guard):
    """dst = saved when guard[2] is set; otherwise nothing."""
    _check._chk(dst, "dst")
    _check._chk(saved, "saved")
    if dst.numel() != saved.numel():
        raise ValueError("restore_if_: dst and saved sizes disagree")
    _lib.call("ubpl_restore_if", dst, saved, dst.numel(), guard)
