"""FlatAdamW — torch.optim.AdamW semantics over a model's flat parameter
buffer, one fused HIP kernel per step (optim.hip).

The reference builds `AdamW(model.parameters(), lr=args.lr,
weight_decay=args.wd)` per student (projects/MT_UBPL.py:48).  Here the
moments are two flat buffers the size of the grad-carrying prefix; the
never-trained skip_layer parameters (which torch skips because their grad
stays None) are outside that prefix and are never touched, exactly as in the
reference.

Guarded step (max_grad_norm / skip_nonfinite, both off by default): one pass
over the flat gradient (ubpl_grad_guard) leaves the clip_grad_norm_
coefficient, the norm and a skip flag on the device, and the guarded entries
take g * c in registers and leave the weights, the moments and the step count
alone when the gradient holds an inf or a NaN.
"""
import torch

from . import kernels as Kn
from .hourglass import StackedHourglass


class FlatAdamW:
    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
                 skip_nonfinite=False):
        if not isinstance(model, StackedHourglass):
            raise TypeError("FlatAdamW needs a ubpl_amd StackedHourglass")
        self.model = model
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        n = model.n_live
        self.exp_avg = torch.zeros(n, device=model.flat_params.device)
        self.exp_avg_sq = torch.zeros(n, device=model.flat_params.device)
        # the step count lives on the device so a captured step graph replays
        # it (ubpl_adamw_step_dev increments it); host reads sync lazily
        self._step_t = torch.zeros((), dtype=torch.int64, device=model.flat_params.device)
        self._coef = torch.zeros(4, device=model.flat_params.device)
        self.param_groups = [{"lr": lr, "betas": betas, "eps": eps, "weight_decay": weight_decay}]
        self.guarded = False
        self.configure_guard(max_grad_norm, skip_nonfinite)

    def configure_guard(self, max_grad_norm=None, skip_nonfinite=False):
        """Set the guard's options (the training steps do, from args.maxGradNorm /
        skipNonFinite).  With max_grad_norm alone a non-finite norm still skips (a NaN
        never reaches p); skip_nonfinite alone skips without clipping.  The device
        buffers are allocated once and keep their addresses and counts."""
        mgn = float(max_grad_norm) if max_grad_norm else 0.0
        if mgn < 0:
            raise ValueError("FlatAdamW: max_grad_norm must be positive (None or 0: off)")
        self.max_grad_norm, self.skip_nonfinite = mgn, bool(skip_nonfinite)
        self.guarded = mgn > 0 or self.skip_nonfinite
        if self.guarded and not hasattr(self, "_guard"):
            dev = self.model.flat_params.device
            self._guard_part = Kn.grad_guard_scratch(self.model.n_live, dev)
            self._guard = torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev)
            self._skipped = torch.zeros(2, dtype=torch.int64, device=dev)

    @property
    def step_count(self):
        return int(self._step_t.item())

    # the guard's counters and last norm live on the device; like step_count these
    # reads synchronise, so call them between steps, not inside one
    def _need_guard(self):
        if not self.guarded:
            raise RuntimeError("FlatAdamW: built without max_grad_norm / skip_nonfinite, there is no guard")

    @property
    def skipped_steps(self):
        """Steps skipped for a non-finite gradient since construction (not persisted)."""
        self._need_guard()
        return int(self._skipped[0].item())

    @property
    def consecutive_skipped(self):
        self._need_guard()
        return int(self._skipped[1].item())

    @property
    def last_grad_norm(self):
        """The global L2 norm the last guard() saw, before clipping (inf / NaN on a skipped step)."""
        self._need_guard()
        return float(self._guard[1].item())

    @property
    def last_clip_coef(self):
        self._need_guard()
        return float(self._guard[0].item())

    def guard(self):
        """Read the live gradients once and leave {clip coefficient, norm, skip, 0} in
        self._guard for the guarded step (step() / step_and_ema() call it themselves;
        the training steps call it first to restore BatchNorm statistics from it)."""
        self._need_guard()
        Kn.grad_guard_(self.model.live_grads(), self.max_grad_norm, self._guard_part, self._guard)
        return self._guard

    def zero_grad(self, set_to_none=True):
        self.model.flat_grads.zero_()
        self.model.attach_grad_views()

    def step(self, guard_done=False):
        g = self.param_groups[0]
        if self.guarded:
            if not guard_done:
                self.guard()
            Kn.adamw_step_guarded_dev_(self.model.live_params(), self.model.live_grads(), self.exp_avg,
                                       self.exp_avg_sq, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                                       g["weight_decay"], self._step_t, self._coef, self._guard, self._skipped)
            return
        Kn.adamw_step_dev_(self.model.live_params(), self.model.live_grads(), self.exp_avg, self.exp_avg_sq,
                           g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], self._step_t,
                           self._coef)

    def step_and_ema(self, ema_model, alpha, guard_done=False):
        """step() then update_ema_variables(model, ema_model) with this alpha, in
        one pass over the flat buffers (bit-identical to the two calls).  On a
        skipped step the teacher still moves toward the unchanged student."""
        if not isinstance(ema_model, StackedHourglass) or ema_model.n_total != self.model.n_total:
            raise ValueError("step_and_ema: the teacher must be a StackedHourglass of the same architecture")
        g = self.param_groups[0]
        if self.guarded:
            if not guard_done:
                self.guard()
            Kn.adamw_ema_step_guarded_dev_(self.model.flat_params, self.model.flat_grads, self.exp_avg,
                                           self.exp_avg_sq, self.model.n_live, g["lr"], g["betas"][0],
                                           g["betas"][1], g["eps"], g["weight_decay"], self._step_t, self._coef,
                                           ema_model.flat_params, alpha, self._guard, self._skipped)
            return
        Kn.adamw_ema_step_dev_(self.model.flat_params, self.model.flat_grads, self.exp_avg, self.exp_avg_sq,
                               self.model.n_live, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                               g["weight_decay"], self._step_t, self._coef, ema_model.flat_params, alpha)

    # -- checkpoints: torch.optim.AdamW's state_dict layout -----------------
    # projects/MT_UBPL.py:97-103 stores optims[b].state_dict() in the
    # checkpoint next to the models' state_dicts (utils/base/comm.py:92-103
    # torch.save).  The state is laid out exactly as torch.optim.AdamW lays it
    # out over model.parameters() (reference order, 454 tensors for HG2): one
    # entry per parameter that has been stepped (the live ones; the dead
    # skip_layer parameters never get a gradient, so torch keeps no state for
    # them either), 'step' a CPU float tensor, group keys from torch itself.
    # Checkpoints interchange both ways with the reference's optimizers.
    # The guard's options and counters (skipped_steps, consecutive_skipped) are
    # not part of that layout and are NOT persisted: a resumed run counts from 0.
    def _group_template(self):
        g = self.param_groups[0]
        probe = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=g["lr"], betas=g["betas"], eps=g["eps"],
                                  weight_decay=g["weight_decay"])
        grp = dict(probe.state_dict()["param_groups"][0])
        grp.update({k: v for k, v in g.items()})
        return grp

    def _live_slices(self):
        m = self.model
        for i, (name, _) in enumerate(m.named_parameters()):
            s, n, shp = m._offs[name]
            yield i, s, n, shp, s < m.n_live

    def state_dict(self):
        """torch.optim.AdamW's layout; the guard's skip counters are not persisted."""
        names = list(self.model.named_parameters())
        grp = self._group_template()
        grp["params"] = list(range(len(names)))
        state = {}
        step = self.step_count
        if step > 0:
            for i, s, n, shp, live in self._live_slices():
                if live:
                    state[i] = {"step": torch.tensor(float(step)),
                                "exp_avg": self.exp_avg[s:s + n].view(shp).clone(),
                                "exp_avg_sq": self.exp_avg_sq[s:s + n].view(shp).clone()}
        return {"state": state, "param_groups": [grp]}

    def load_state_dict(self, sd):
        """Accepts torch.optim.AdamW's layout over model.parameters() (a
        reference checkpoint's optim<b>_state, or this class's state_dict)."""
        groups = sd["param_groups"]
        if len(groups) != 1:
            raise ValueError("FlatAdamW holds one parameter group, the state has %d" % len(groups))
        nparams = sum(1 for _ in self.model.parameters())
        if len(groups[0]["params"]) != nparams:
            raise ValueError("loaded state dict has a group of %d parameters, the model has %d"
                             % (len(groups[0]["params"]), nparams))
        pos = {pid: i for i, pid in enumerate(groups[0]["params"])}
        st = {pos[k]: v for k, v in sd["state"].items()}
        steps = set()
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for i, s, n, shp, live in self._live_slices():
            e = st.get(i)
            if e is None:
                continue
            if not live:
                raise ValueError("state for parameter %d, which never receives a gradient here" % i)
            if tuple(e["exp_avg"].shape) != tuple(shp):
                raise ValueError("state shape %s for parameter %d of shape %s" % (tuple(e["exp_avg"].shape), i,
                                                                                  tuple(shp)))
            self.exp_avg[s:s + n].copy_(e["exp_avg"].reshape(-1))
            self.exp_avg_sq[s:s + n].copy_(e["exp_avg_sq"].reshape(-1))
            steps.add(int(float(e["step"])))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ (%s): one flat step count cannot hold them"
                             % sorted(steps))
        self._step_t.fill_(steps.pop() if steps else 0)
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("FlatAdamW runs plain AdamW (amsgrad / maximize unsupported)")
        self.lr, self.betas, self.eps, self.weight_decay = g["lr"], tuple(g["betas"]), g["eps"], g["weight_decay"]
        self.param_groups[0].update(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"])
