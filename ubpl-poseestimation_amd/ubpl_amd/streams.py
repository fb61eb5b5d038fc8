"""Per-network HIP streams of a multi-network training step and the rule their
phases keep: between fork and join no PyTorch arithmetic kernel is enqueued.
A step's forwards run between _ModelStreams.make and join, its backwards between
_backward_all's fork and _join_merge; _OnMain sits between outputs and losses."""
import os

import torch


# Invariant of the networks' phases (fork -> join): no PyTorch arithmetic kernel
# is enqueued — PyTorch's elementwise kernels carry packed-FP32 instructions,
# which this hardware mis-executed beside concurrent matrix work (DESIGN.md §6;
# the library itself is built without them, csrc/Makefile NOPK).  With
# UBPL_STREAM_CHECK=1 every phase runs under _PhaseCheck, which records each
# aten op on a floating-point device tensor that is not a view, an allocation
# or a copy, and join() raises naming them (tests/test_gpu_race.py runs the
# step so).
_STREAM_CHECK = os.environ.get("UBPL_STREAM_CHECK") == "1"
# data movement and metadata: no arithmetic
_PHASE_OK = {"empty", "empty_strided", "empty_like", "zeros", "zeros_like", "zero_", "fill_", "copy_", "clone",
             "_to_copy", "to", "cat", "stack", "detach", "alias", "view", "_unsafe_view", "reshape", "as_strided",
             "expand", "select", "slice", "unsqueeze", "squeeze", "permute", "t", "transpose", "unbind", "split",
             "contiguous", "record_stream", "set_", "resize_", "lift_fresh", "new_empty", "new_zeros",
             "new_empty_strided", "split_with_sizes", "narrow", "view_as", "_reshape_alias", "unfold", "flatten",
             "is_same_size"}


def _phase_violation(func, args, kwargs, on_device):
    """The aten op's name if it is arithmetic on a floating-point device tensor."""
    if func.namespace != "aten":
        return None
    name = func.__name__.split(".")[0]
    if name in _PHASE_OK:
        return None
    ts = [a for a in list(args) + list((kwargs or {}).values()) if torch.is_tensor(a)]
    ts += [x for a in args if isinstance(a, (list, tuple)) for x in a if torch.is_tensor(x)]
    if any(on_device(t) and t.is_floating_point() for t in ts):
        return name
    return None


class _PhaseCheck:
    """Records the aten arithmetic ops enqueued while the networks' streams are
    forked (see _STREAM_CHECK).  on_device: which tensors count (the tests use
    CPU tensors to check the classifier itself)."""

    def __init__(self, on_device=lambda t: t.is_cuda):
        from torch.utils._python_dispatch import TorchDispatchMode
        seen = self.seen = []

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                v = _phase_violation(func, args, kwargs, on_device)
                if v is not None:
                    seen.append(v)
                return func(*args, **(kwargs or {}))
        self.mode = Mode()

    def __enter__(self):
        self.mode.__enter__()
        return self

    def __exit__(self, *a):
        return self.mode.__exit__(*a)


class _ModelStreams:
    """One HIP stream per network (students 0..M-1, then their teachers).  The
    networks are independent until the losses, and their small hourglass
    levels (<= 16x16: a few dozen workgroups per launch) leave most of the
    chip idle, so several networks in flight fill it.  Autograd runs each
    network's backward on its forward's stream (PyTorch stream semantics of
    backward), so the backward overlaps the same way.  UBPL_MODEL_STREAMS=0
    runs everything on the current stream."""
    _cache = {}

    def __init__(self, M, dev):
        self.main = torch.cuda.current_stream(dev)
        key = (M, dev.index)
        if key not in self._cache:
            self._cache[key] = [torch.cuda.Stream(device=dev) for _ in range(2 * M)]
        self.side = self._cache[key]
        self.M = M
        self._check = None
        self.fork()

    @staticmethod
    def make(M, dev):
        if M < 2 or os.environ.get("UBPL_MODEL_STREAMS", "1") == "0":
            return None
        return _ModelStreams(M, dev)

    # diagnostic: UBPL_ONE_SIDE=1 runs every network on ONE side stream (still not main)
    _one = os.environ.get("UBPL_ONE_SIDE") == "1"

    def on(self, mi):
        return torch.cuda.stream(self.side[0 if self._one else mi])

    def on_teacher(self, mi):
        return torch.cuda.stream(self.side[0 if self._one else self.M + mi])

    def fork(self):
        """Every network stream waits for main: the start of a networks' phase
        (in a segment captured on its own it also brings the streams into the
        capture)."""
        for s in self.side:
            s.wait_stream(self.main)
        if _STREAM_CHECK and self._check is None:
            self._check = _PhaseCheck().__enter__()
            _OPEN_CHECKS.append(self)

    def end_check(self):
        """Leave the phase's _PhaseCheck mode (if one is on); returns what it saw."""
        if self._check is None:
            return ()
        chk, self._check = self._check, None
        chk.__exit__(None, None, None)
        if self in _OPEN_CHECKS:
            _OPEN_CHECKS.remove(self)
        return chk.seen

    def join(self, tensors=()):
        seen = self.end_check()
        for s in self.side:
            self.main.wait_stream(s)
        if seen:                          # (main has joined every network stream first)
            raise RuntimeError("ubpl_amd: PyTorch arithmetic enqueued while the network streams run "
                               "(UBPL_STREAM_CHECK): %s" % sorted(set(seen)))
        if torch.cuda.is_current_stream_capturing():
            return                        # the graph's own dependencies order them
        for t in tensors:                 # produced on a side stream, used on main
            if t is not None and t.is_cuda:
                t.record_stream(self.main)


# phases whose _PhaseCheck mode is on (UBPL_STREAM_CHECK): a step that raised between a
# fork and its join leaves its mode on the dispatch stack; the step drivers close them
_OPEN_CHECKS = []


def _close_phase_checks():
    while _OPEN_CHECKS:
        _OPEN_CHECKS[-1].end_check()


# The students' gradient all-reduce runs after the network streams have joined,
# with nothing else on the device beside it.  torch's RCCL gfx950 reduce kernels
# carry packed-FP32 adds (runTreeUpDown<float, FuncSum>, ReduceScatter PAT f32:
# tools/rccl_pk_check.py, profiles/r05_rccl_packed_fp32.txt), the instruction this
# hardware mis-executed beside concurrent matrix work, so round 3's
# overlap of student i's all-reduce with the other networks' backward (worth < 1 %
# of the step) is gone.
def _join_merge(mstreams, models):
    """Join the network streams and merge every student's second-view gradients
    (projects/MT_UBPL.py:334-336 accumulate both views into .grad)."""
    if mstreams:
        mstreams.join()
    for m in models:
        m.merge_alt_grads()


class _OnMain(torch.autograd.Function):
    """Identity applied on the main stream to a network output produced on a
    side stream.  Autograd sums the several loss gradients of a tensor on the
    stream of the node that consumes them; without this node that is the
    network's stream, reading summands the loss backward allocated on main,
    which the caching allocator hands back to main once autograd drops them —
    while the side stream may still be reading them (a race that only shows
    when main is not the legacy null stream, i.e. in the captured step and
    its warm-up).  With it, the sum happens on main and the network's backward
    receives one tensor that lives until its node has run."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g


def _backward_all(totals, outputs=None, mstreams=None):
    """The reference runs total_i.backward(retain_graph=True) once per student
    (projects/MT_UBPL.py:334-336): the shared FDL term makes every call reach
    every student, so each network's backward would run M times with gradients
    that are then summed into .grad.  Backward is linear, so one traversal of
    sum_i total_i accumulates the same gradients with each network's backward
    run once (its upstream gradients summed first).

    outputs (the networks' outputs the losses read): two phases — first every
    loss gradient w.r.t. those outputs, on the main stream, then the networks'
    backwards from them, on their own streams — so no PyTorch elementwise
    kernel (autograd's gradient sums, the loss backward) runs beside the
    networks' matrix work: PyTorch's kernels use packed-FP32 instructions,
    which this hardware mis-executed beside concurrent matrix work (csrc/Makefile
    NOPK)."""
    if outputs is None:
        torch.autograd.backward(totals)
        return
    outs = [t for t in outputs if t is not None and t.requires_grad]
    grads = torch.autograd.grad(totals, outs, allow_unused=True)
    pairs = [(t, g) for t, g in zip(outs, grads) if g is not None]
    if mstreams is not None:
        mstreams.fork()                   # the networks' phase (a captured segment's streams join here)
    torch.autograd.backward([t for t, _ in pairs], [g for _, g in pairs])
