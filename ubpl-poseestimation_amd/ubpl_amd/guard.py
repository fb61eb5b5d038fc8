"""Guarded step: args.maxGradNorm (0 / absent: off), args.skipNonFinite (absent:
False), args.maxSkippedSteps (default 10) — DESIGN.md §4.  A step starts with
_save_stats and takes the guard right before its optimizer step (_guard_and_restore,
from train._step_and_ema); the epoch drivers watch the skip counts (_SkipWatch)."""
import contextlib

import torch

from . import kernels as Kn
from .step_graph import _LaggedRecords


# Order within a step: backward, the gradient all-reduce (every rank then holds
# the same summed gradients and takes the same decision), the guard, the guarded
# step.  With skipNonFinite each network's BatchNorm running statistics are
# copied to a shadow buffer at the start of the step and put back after the
# guard when the step is skipped: student i and teacher i by student i's guard
# (a NaN teacher output reaches student i's consistency loss).  Everything goes
# through device memory, inside the captured region.
def _guard_opts(args):
    return (float(getattr(args, "maxGradNorm", 0) or 0), bool(getattr(args, "skipNonFinite", False)),
            int(getattr(args, "maxSkippedSteps", 10)))


def _guard_nets(models, models_ema):
    """Per optimizer, the networks whose BatchNorm statistics its guard covers."""
    return [[m] + ([models_ema[i]] if i < len(models_ema) else []) for i, m in enumerate(models)]


def _bn_shadows(o, nets):
    sh = getattr(o, "_bn_shadow", None)
    if sh is None or [s.shape for s in sh] != [n.flat_stats.shape for n in nets]:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ubpl_amd.train: the BatchNorm shadow buffers must exist before the step is captured")
        sh = o._bn_shadow = [torch.empty_like(n.flat_stats) for n in nets]
    return sh


def _configure_guard(optims, nets, args):
    """Apply args' guard options to the optimizers (an optimizer built with its own
    options keeps them when args sets none) and allocate the shadow buffers."""
    mgn, snf, _ = _guard_opts(args)
    for o, ns in zip(optims, nets):
        if mgn > 0 or snf:
            if not hasattr(o, "configure_guard"):
                raise TypeError("ubpl_amd.train: maxGradNorm / skipNonFinite need FlatAdamW optimizers, got %s "
                                "(torch's AdamW is not covered)" % type(o).__name__)
            if (o.max_grad_norm, o.skip_nonfinite) != (mgn, snf):
                o.configure_guard(mgn, snf)
        if getattr(o, "skip_nonfinite", False):
            _bn_shadows(o, ns)


def _save_stats(optims, nets):
    """Start of a step: shadow copies of the BatchNorm running statistics."""
    for o, ns in zip(optims, nets):
        if getattr(o, "skip_nonfinite", False):
            for s, n in zip(_bn_shadows(o, ns), ns):
                s.copy_(n.flat_stats)


def _guard_and_restore(optims, nets):
    """After the gradients are final: each guarded optimizer's guard, then the
    statistics of a skipped step back from their shadows."""
    for o, ns in zip(optims, nets):
        if not getattr(o, "guarded", False):
            continue
        g = o.guard()
        if o.skip_nonfinite:
            for s, n in zip(_bn_shadows(o, ns), ns):
                Kn.restore_if_(n.flat_stats, s, g)


def _gd(o):
    return {"guard_done": True} if getattr(o, "guarded", False) else {}


class _SkipWatch:
    """The consecutive-skip counts reach the host as the records do, one step late
    (a second small lagged copy: no new host synchronisation per step); at
    maxSkippedSteps in a row the run stops with FloatingPointError."""

    def __init__(self, optims, args):
        self.optims = [o for o in optims if getattr(o, "guarded", False)]
        self.limit = _guard_opts(args)[2]
        self.lag = _LaggedRecords()

    def push(self, bat):
        if self.optims and self.limit > 0:
            self.lag.push(torch.stack([o._skipped for o in self.optims]), lambda host, bat=bat: self._check(host, bat))

    def _check(self, host, bat):
        worst = max(int(c) for c in host[1::2])
        if worst >= self.limit:
            raise FloatingPointError(
                "ubpl_amd.train: %d consecutive optimizer steps skipped for a non-finite gradient (batch %d; "
                "totals per student: %s).  The default 2xfp16 conv path holds its operands in fp16 after "
                "power-of-two scaling: |activation| <= 2047 and |w| <= 65504 / fp16_wscale(K) (K = Cin * taps; "
                "|w| <= 4 for a 64-channel 3x3); beyond that range the forward overflows to inf and the "
                "gradients to NaN.  Check the inputs for inf / NaN, lower the learning rate or set maxGradNorm, "
                "or run with UBPL_CONV_PRECISION=6xbf16, which has f32's range."
                % (worst, bat + 1, [int(c) for c in host[0::2]]))

    @contextlib.contextmanager
    def flushing(self):
        with self.lag.flushing():
            yield self
