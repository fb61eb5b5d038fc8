"""Who runs a step generator (train.py's *_core), for train.py's epoch drivers:
_drive performs its yielded collectives at once, _StepGraph captures the device
work around them as HIP graphs and replays it, and _LaggedRecords brings each
step's one device->host copy to the host a step late."""
import contextlib
import os

import torch

from . import dist as D
from .streams import _close_phase_checks


# The MT_UBPL and DualPose steps (_mt_ubpl_core, _dualpose_core) are generators: it YIELDS its two exchanges —
# ("sum", t): SUM all-reduce of the packed loss sums and counts in place (dist.py
# exchange 1), ("grads", models): the students' gradient all-reduce (exchange 2)
# — and whoever drives them performs them.  Eagerly they run at once (_drive); the
# captured step under torch.distributed captures the device work between them as
# graph segments and runs the collectives between the segments' replays
# (_StepGraph), so the exchanges are never inside a captured graph.
def _collective(req):
    kind, obj = req
    if kind == "sum":
        D.allreduce_(obj)
    elif kind == "grads":
        D.allreduce_grads(obj)
    else:
        raise ValueError("unknown collective %r" % (kind,))


def _drive(gen):
    """Run a step generator eagerly: each yielded collective is performed at once."""
    try:
        req = gen.send(None)
        while True:
            _collective(req)
            req = gen.send(None)
    except StopIteration as e:
        return e.value
    finally:
        _close_phase_checks()


def _flatten(obj, leaves):
    """Tiny pytree flatten of a batch: tensors become leaves; lists, tuples and
    dicts recurse; anything else is a constant kept in the spec."""
    if torch.is_tensor(obj):
        leaves.append(obj)
        return ("T", len(leaves) - 1, tuple(obj.shape), str(obj.dtype))
    if isinstance(obj, (list, tuple)):
        return (type(obj).__name__, tuple(_flatten(v, leaves) for v in obj))
    if isinstance(obj, dict):
        return ("dict", tuple((k, _flatten(v, leaves)) for k, v in obj.items()))
    return ("C", repr(obj), obj)


def _spec_key(spec):
    if spec[0] == "C":
        return ("C", spec[1])
    if spec[0] == "T":
        return spec
    if spec[0] == "dict":
        return ("dict", tuple((k, _spec_key(v)) for k, v in spec[1]))
    return (spec[0], tuple(_spec_key(v) for v in spec[1]))


def _unflatten(spec, leaves):
    kind = spec[0]
    if kind == "T":
        return leaves[spec[1]]
    if kind == "C":
        return spec[2]
    if kind == "dict":
        return {k: _unflatten(v, leaves) for k, v in spec[1]}
    vals = [_unflatten(v, leaves) for v in spec[1]]
    return tuple(vals) if kind == "tuple" else vals


class _KeepAll:
    """Diagnostic (UBPL_GRAPH_KEEPALL=1): keeps every tensor any torch op
    allocates during the capture alive until the graph is released, so no
    memory block is reused inside the captured step."""

    def __enter__(self):
        from torch.utils._python_dispatch import TorchDispatchMode
        kept = self.kept = []

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                out = func(*args, **(kwargs or {}))
                kept.append(out)
                return out
        self.mode = Mode()
        self.mode.__enter__()
        return self

    def __exit__(self, *a):
        return self.mode.__exit__(*a)


class _StepGraph:
    """Runs a device-only step function (a *_core below) and, once the batch
    shapes repeat, replays it from a captured HIP graph: ~6k kernel launches
    per MT_UBPL step become one graph launch, so the host no longer paces the
    GPU.  The first WARM steps run eagerly on a side stream (graph warm-up
    rule); the next step is captured (capture records, it does not execute)
    and then replayed for that batch and every later one, its tensors copied
    into the graph's static inputs first.  Everything the step reads from the
    host — args, learning rates — is part of the cache key, so a change
    re-captures; per-step state (AdamW step counts, BN counters) lives on the
    device.  Under torch.distributed the step is captured as segments — the
    device work before, between and after its two collectives, in one memory
    pool, replayed in capture order — and the collectives run eagerly between
    the replays (no collective inside a graph).  Verified bit-identical to the
    eager step on gloo (two ranks, tests/test_gpu_dist.py) and on RCCL with one
    rank on the GPU (UBPL_DIST_WORLD1: both collectives through RCCL between the
    replays, test_rccl_segmented_graph_matches_eager); RCCL with more than one rank
    needs a multi-GPU box and is the driver's scaling run.  UBPL_STEP_GRAPH=0
    disables."""
    WARM = 2
    _cache = {}

    def __init__(self, core, models, models_ema, optims, args):
        self.core, self.models, self.emas, self.optims, self.args = core, models, models_ema, optims, args
        # default: captured, with or without per-network streams (rounds 1-3 kept
        # it off with streams for a divergence whose cause — packed-FP32
        # instructions beside concurrent matrix work — round 4 removed: DESIGN.md
        # §6); UBPL_STEP_GRAPH=0 disables it.
        self.enabled = os.environ.get("UBPL_STEP_GRAPH") != "0" and all(hasattr(o, "_step_t") for o in optims)
        self.n_eager = 0
        self.graph = None                  # the captured segments (one without torch.distributed)
        self.reqs = []                     # the collective after each segment but the last
        self.hkey = self.key = self.static = self.out = self.side = None

    _force_eager = False

    @classmethod
    @contextlib.contextmanager
    def eager(cls):
        """Context: run steps eagerly (e.g. to time individual kernels with host
        events, which a captured graph cannot record)."""
        old = cls._force_eager
        cls._force_eager = True
        try:
            yield
        finally:
            cls._force_eager = old

    @classmethod
    def get(cls, core, models, models_ema, optims, args):
        """One runner per (step function, networks, optimisers).  The host
        constants the captured step bakes in (args: loss weights, epoch ->
        EMA alpha; the learning rates) change every epoch: then the old graph
        and its memory pool are released and the next step re-captures."""
        key = (core.__name__, tuple(map(id, models)), tuple(map(id, models_ema)), tuple(map(id, optims)))
        hkey = (repr(sorted(vars(args).items())) if hasattr(args, "__dict__") else repr(args),
                repr([(o.param_groups, getattr(o, "max_grad_norm", None), getattr(o, "skip_nonfinite", None))
                      for o in optims]))
        r = cls._cache.get(key)
        if r is None:
            cls.clear()                      # one runner: an old one would pin its networks and pool
            r = cls._cache[key] = cls(core, models, models_ema, optims, args)
            r.hkey = hkey
        if r.hkey != hkey:
            r.release()
            r.args, r.hkey = args, hkey
        return r

    @classmethod
    def clear(cls):
        for r in cls._cache.values():
            r.release()
        cls._cache.clear()

    def release(self):
        """Drop the captured graph, its static inputs and outputs (its private
        memory pool goes with them)."""
        if self.graph is not None:
            for g in self.graph:
                g.reset()
            self.graph, self.reqs, self.key, self.static, self.out = None, [], None, None, None
            torch.cuda.empty_cache()

    def _eager(self, batch):
        return _drive(self.core(self.models, self.emas, self.optims, self.args, *batch))

    def _replay(self):
        for i, g in enumerate(self.graph):
            g.replay()
            if i < len(self.reqs):
                _collective(self.reqs[i])

    def _capture(self, sbatch):
        """Capture the step: one graph, or under torch.distributed one graph per
        stretch between collectives (shared pool, replayed in this order)."""
        gen = self.core(self.models, self.emas, self.optims, self.args, *sbatch)
        keep = _KeepAll() if os.environ.get("UBPL_GRAPH_KEEPALL") == "1" else contextlib.nullcontext()
        if not D.is_dist():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g), keep:
                self.out = _drive(gen)
            self._kept = getattr(keep, "kept", None)
            self.graph, self.reqs = [g], []
            return
        pool = torch.cuda.graph_pool_handle()
        graphs, reqs, done = [], [], False
        try:
            while not done:
                g = torch.cuda.CUDAGraph()
                # thread_local: the process group's own threads may query HIP while a segment captures
                with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
                    try:
                        req = gen.send(None)
                    except StopIteration as e:
                        self.out, done = e.value, True
                graphs.append(g)
                if not done:
                    reqs.append(req)
        finally:
            _close_phase_checks()
        self.graph, self.reqs = graphs, reqs

    def run(self, batch, dev):
        if not self.enabled or self._force_eager:
            return self._eager(batch)
        leaves = []
        spec = _flatten(batch, leaves)
        key = _spec_key(spec)
        if self.graph is not None and key == self.key:
            for dst, src in zip(self.static, leaves):
                dst.copy_(src, non_blocking=True)
            self._replay()
            return self.out
        if self.n_eager < self.WARM or self.graph is not None:
            # warm-up (or a batch of another shape): eager, on a side stream
            if self.side is None:
                self.side = torch.cuda.Stream(device=dev)
            main = torch.cuda.current_stream(dev)
            self.side.wait_stream(main)
            with torch.cuda.stream(self.side):
                out = self._eager(batch)
            main.wait_stream(self.side)
            self.n_eager += 1
            return out
        self.static = [l.to(dev).clone() for l in leaves]
        sbatch = _unflatten(spec, self.static)
        torch.cuda.synchronize(dev)
        self._capture(sbatch)
        self.key = key
        self._replay()
        return self.out


class _LaggedRecords:
    """A step's records reach the host one step late: the device->host copy of
    step k goes into pinned memory asynchronously right behind step k's work,
    and the host reads it (waiting on its event) only after step k+1 has been
    enqueued — so the GPU never idles while the host enqueues the next step
    (a blocking .cpu() per step drained the queue every step: the next step's
    ~5k launches then started from an empty queue).  The records, their order
    and every printed line are those of the blocking form; `consume` runs in
    step order.  UBPL_LAG_RECORDS=0: consume each step's records at once."""
    _on = os.environ.get("UBPL_LAG_RECORDS", "1") != "0"

    def __init__(self):
        self.pending = None

    def push(self, packed, consume):
        dev_t = packed.detach().reshape(-1)
        host = torch.empty(dev_t.shape, dtype=dev_t.dtype, pin_memory=True)
        host.copy_(dev_t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev_t.device))    # the stream the copy went on
        prev, self.pending = self.pending, (host, ev, consume)
        if prev is not None:
            self._run(prev)
        if not self._on:
            self.flush()

    def flush(self):
        prev, self.pending = self.pending, None
        if prev is not None:
            self._run(prev)

    @contextlib.contextmanager
    def flushing(self):
        """Flush on exit — also when the loader raised mid-epoch (the last
        step's records); then an error the flush itself raises (a wait on a
        step a GPU error left half-done) does not replace the one already
        propagating."""
        try:
            yield self
        except BaseException:
            try:
                self.flush()
            except Exception:
                pass
            raise
        self.flush()

    @staticmethod
    def _run(item):
        host, ev, consume = item
        ev.synchronize()
        consume(host.tolist())
