"""utils.losses drop-in: heatmap losses on the HIP kernels (L1-L4, L6).

Same class names, constructor arguments, call signatures and return tuples as
utils/losses.py (JointMSELoss :8, JointDistLoss :32, JointFeatureDistLoss :56,
JointPseudoLoss3 :169, JointDistLoss_mt2 :246, AvgCounter(s) :357-396).  Rows
follow the reference's reshape semantics exactly: with nStack == 1 a row is
(sample, preds.size(1)) — for a [B,1,K,R,R] model output that is one row per
sample over K*R*R pixels, as `preds.reshape((bs, k, -1))` makes it.

Counts are returned as Python ints, as the reference returns them; that costs
one device->host copy per call (the reference pays one per element).  The
fused training step (ubpl_amd.train) keeps counts on device instead.
"""
import torch
from torch import nn

from . import _lib
from . import kernels as Kn


NO_RULE = ("none", 0.0)


class _RowLoss(torch.autograd.Function):
    """Every heatmap row loss: sum over rows of w_row * mean_px((a - target)^2).
    rows: a Kn.RowSpec (where each row's target lies).  kind: what the row mask tests —
    0 nothing, 1 the target's score, 2 both inputs' scores, 3 both and gate > 0 as a row mask
    (ubpl_loss_finalize's kinds).  rule: what a score is and what it is held to —
      ("none", 0.0)   kind 0;
      ("max", v)      the per-map maximum at the constant v;
      ("softmax", v)  the softmax score (softmax across the keypoint axis at every pixel, then the
                      per-map maximum: utils/losses.py:137-138) at the constant v;
      ("rank", r)     the softmax score at, per stack, the r-th smallest of the batch's B*K scores
                      (folded into the finalize launch, ubpl_loss_finalize_rank).
    The softmax rules serve kinds 1 and 2; a target that is one map per row for all stacks is
    scored once.
    forward: (sum, cnt[4] int32, score[K], thr[2*S]: rateThr1[S] then rateThr2[S]) on the device,
    no host sync; score is empty for kind 0 (and for kind 1 under a softmax rule), thr for the
    rules "none" and "max".  backward: d preds (and d targets for a one-member target that
    requires grad); the mask carries no gradient."""

    @staticmethod
    def forward(ctx, a, t, rows, kind, rule, use_gate, use_sw, gate, sw):
        B, S, K, HW = rows[:4]
        how, val = rule
        thr = None
        if how in ("none", "max"):
            sq, am, tm = Kn.row_stats(a, t, rows, want_amax=(kind in (2, 3)), want_tmax=(kind != 0))
            s, cnt, score, w = Kn.loss_finalize(kind, sq, am, tm, gate, sw, use_gate, use_sw, B, S, K, val)
        else:
            sq, _, _ = Kn.row_stats(a, t, rows)
            St = rows.t_stacks
            tsc = Kn.softmax_peak_scores(rows.target(t), rows.t_sb, rows.t_ss, rows.t_sm, rows.M, B, St, K, HW)
            asc = Kn.softmax_peak_scores(a, rows.a_sb, rows.a_ss, 0, 1, B, S, K, HW) if kind == 2 else None
            if how == "rank":
                s, cnt, score, w, thr = Kn.loss_finalize_rank(kind, sq, asc, tsc, St, val, gate, sw, use_gate, use_sw,
                                                              B, S, K, want_score=(kind == 2))
            else:
                thr = torch.full((2 * S,), float(val), device=a.device, dtype=torch.float32)
                if St != S:                                      # the one target score per (b,k) serves every stack
                    tsc = tsc.view(B, 1, K).expand(B, S, K).contiguous().view(-1)
                s, cnt, score, w = Kn.loss_finalize_ranked(kind, sq, asc, tsc, thr[:S] if kind == 2 else None, thr[S:],
                                                           gate, sw, use_gate, use_sw, B, S, K, want_score=(kind == 2))
        ctx.save_for_backward(a, t, w)
        ctx.rows = rows
        ctx.t_grad = t.requires_grad and rows.M == 1 and rows.t_sm == 0
        outs = (s.view(()), cnt, score if score is not None else s.new_empty(0),
                thr if thr is not None else s.new_empty(0))
        ctx.mark_non_differentiable(*outs[1:])
        return outs

    @staticmethod
    def backward(ctx, gs, *_):
        a, t, w = ctx.saved_tensors
        da = torch.empty_like(a)
        Kn.row_grad(a, t, ctx.rows, w, gs.reshape(1).contiguous().float(), 2.0 / ctx.rows.HW, da)
        dt = -da if ctx.t_grad else None
        return (da, dt) + (None,) * 7


def _f32c(t):
    return None if t is None else t.detach().float().contiguous()


def _gate_rows(kpsGate, B, K, S):
    """Gate per loss row.  With nStack == 1 and [B,1,...] predictions the
    reference's rows are per sample (K == 1) while the gate is [B,Kg]:
    `loss.mul(kpsGate)` broadcasts [B,1] x [B,Kg] (utils/losses.py:25), i.e.
    each sample's loss is weighted by the SUM of its gates, and the count is
    still #{gate > 0} over the full gate (:18-19).  Returns (gate rows, count
    override or None)."""
    gate = _f32c(kpsGate)
    if gate is None or gate.shape[-1] == K:
        return gate, None
    if K != 1:
        raise RuntimeError("kpsGate %s does not broadcast against %d rows per sample" % (tuple(gate.shape), K))
    count = S * int((gate > 0).sum().item())
    return gate.reshape(B, -1).sum(1, keepdim=True).contiguous(), count


def _sw_vec(sw):
    return None if sw is None else sw.detach().float().reshape(-1).contiguous()


def _gated_sum(mod, a, t, rows, kpsGate, sampleWeight):
    """The unmasked losses' common end -> (sum, nStack*#{gate>0})."""
    gate, count = _gate_rows(kpsGate, rows.B, rows.K, rows.S)
    sw = _sw_vec(sampleWeight) if mod.useSampleWeight else None
    s, cnt, _, _ = _RowLoss.apply(a, t, rows, 0, NO_RULE, bool(mod.useKPsGate and gate is not None), sw is not None,
                                  gate, sw)
    return s, count if count is not None else int(cnt[0].item())


class JointMSELoss(nn.Module):
    """utils/losses.py:8-29 -> (sum over stacks/rows of the per-map pixel mean, nStack*#{gate>0})."""

    def __init__(self, nStack=1, useKPsGate=False, useSampleWeight=False):
        super().__init__()
        self.nStack, self.useKPsGate, self.useSampleWeight = nStack, useKPsGate, useSampleWeight

    def forward(self, preds, gts, kpsGate=None, sampleWeight=None):
        _lib.require_gpu(preds)
        a = preds.contiguous()
        rows = Kn.RowSpec.ground_truth(*Kn.pred_rows(a, self.nStack))
        t = gts.detach().contiguous()
        if t.numel() != rows.B * rows.K * rows.HW:
            raise RuntimeError("gts do not match preds rows")
        return _gated_sum(self, a, t, rows, kpsGate, sampleWeight)


class JointDistLoss(nn.Module):
    """utils/losses.py:32-53 (Mean-Teacher consistency)."""

    def __init__(self, nStack=1, useKPsGate=False, useSampleWeight=False):
        super().__init__()
        self.nStack, self.useKPsGate, self.useSampleWeight = nStack, useKPsGate, useSampleWeight

    def forward(self, preds1, preds2, kpsGate=None, sampleWeight=None):
        _lib.require_gpu(preds1)
        a = preds1.contiguous()
        rows = Kn.RowSpec.same(*Kn.pred_rows(a, self.nStack))
        t = preds2.contiguous()
        return _gated_sum(self, a, t, rows, kpsGate, sampleWeight)


def _some_rows(cnt):
    """cnt[4] on the host; no row with sampleWeight > 0 raises as the reference's torch.stack of an
    empty list does (utils/losses.py:107,157,201,279)."""
    c = cnt.tolist()
    if c[3] == 0:
        raise RuntimeError("stack expects a non-empty TensorList")
    return c


class JointDistLoss_mt2(nn.Module):
    """utils/losses.py:246-286: consistency kept where the second input's
    (teacher's) per-map max >= scoreThr.  Returns (sum, nStack*#gate,
    n_pseudo, n_sel, score[K])."""

    def __init__(self, nStack=1, useKPsGate=False, useSampleWeight=False, scoreThr=0.5):
        super().__init__()
        self.nStack, self.useKPsGate, self.useSampleWeight, self.scoreThr = nStack, useKPsGate, useSampleWeight, scoreThr

    def forward(self, preds1, preds2, kpsGate=None, sampleWeight=None):
        _lib.require_gpu(preds1)
        a = preds1.contiguous()
        rows = Kn.RowSpec.same(*Kn.pred_rows(a, self.nStack))
        t = preds2.contiguous()
        gate = _f32c(kpsGate)
        sw = _sw_vec(sampleWeight)
        # rows feeding the score are those with sampleWeight > 0 (utils/losses.py:276), weighted or not
        s, cnt, score, _ = _RowLoss.apply(a, t, rows, 1, ("max", float(self.scoreThr)),
                                          bool(self.useKPsGate and gate is not None),
                                          bool(self.useSampleWeight and sw is not None), gate, sw)
        c = _some_rows(cnt)
        return s, c[0], c[1], c[2], score


def _pseudo_rows(mod, preds, targets, sampleWeight, rule):
    """The ensemble pseudo-label losses' common body: targets [M,B,St,K,R,R] ([M,B,K,R,R] with
    nStack == 1), the member mean of the last stack against every stack of preds, both inputs'
    scores under `rule` -> (sum, n_pseudo, n_sel, score[K], rateThr1[S], rateThr2[S]; empty
    under the "max" rule)."""
    _lib.require_gpu(preds)
    a = preds.contiguous()
    B, S, K, HW = Kn.pred_rows(a, mod.nStack)
    t = targets.detach().contiguous()
    rows = Kn.RowSpec.ensemble(B, S, K, HW, t.shape[0], 1 if mod.nStack == 1 else t.shape[2])
    s, cnt, score, thr = _RowLoss.apply(a, t, rows, 2, rule, False, True, None, _sw_vec(sampleWeight))
    c = _some_rows(cnt)
    return s, c[1], c[2], score, thr[:S], thr[S:]


class JointPseudoLoss3(nn.Module):
    """utils/losses.py:169-210 — the UBPL ensemble pseudo-label loss with the
    per-(sample, keypoint) confidence mask."""

    def __init__(self, nStack=1, scoreThr=0.5):
        super().__init__()
        self.nStack, self.scoreThr = nStack, scoreThr

    def forward(self, preds, targets, sampleWeight):
        out = _pseudo_rows(self, preds, targets, sampleWeight, ("max", float(self.scoreThr)))
        return out[:4] + (self.scoreThr, self.scoreThr)


def sel_rank(n, selRate):
    """The reference's index into the sorted scores, in its own Python-float arithmetic
    (utils/losses.py:139): not exact — int(10 * (1 - 0.9)) is 0."""
    return int(n * (1 - selRate))


def _batch_rank(preds, nstack, selRate):
    """sel_rank over the batch's B*K scores, out of range as the reference's indexing raises it."""
    B, _, K, _ = Kn.pred_rows(preds, nstack)
    rank = sel_rank(B * K, selRate)
    if not 0 <= rank < B * K:
        raise IndexError("index %d is out of bounds for dimension 0 with size %d" % (rank, B * K))
    return rank


class JointPseudoLoss(nn.Module):
    """utils/losses.py:73-115: JointPseudoLoss3's mask on the softmax scores (softmax across the
    keypoint axis at every pixel, then the per-map maximum) at the constant scoreThr.  Returns
    (sum, n_pseudo, n_sel, score[K]).  For maps in [0,1] and K = 16 a softmax score cannot exceed
    e/(e+15) = 0.153: the default 0.8 selects nothing, as in the reference."""

    def __init__(self, nStack=1, scoreThr=0.8):
        super().__init__()
        self.nStack, self.scoreThr = nStack, scoreThr

    def forward(self, preds, targets, sampleWeight):
        return _pseudo_rows(self, preds, targets, sampleWeight, ("softmax", float(self.scoreThr)))[:4]


class JointPseudoLoss2(nn.Module):
    """utils/losses.py:118-166: the pseudo-label loss that keeps a fixed SHARE of the joints.  Per
    stack, the threshold of each input is the int(B*K*(1 - selRate))-th smallest of its B*K softmax
    scores (sel_rank: the reference's float expression), and a row counts where both inputs'
    scores reach their thresholds.  The ranking is over every row of the batch, labeled rows
    (sampleWeight 0) included, as the reference ranks them.  Ties at the threshold are all kept.
    Returns (sum, n_pseudo, n_sel, score[K], rateThr1[S], rateThr2[S]); the thresholds are device
    tensors.  selRate <= 0 raises IndexError as the reference's indexing does; no row with
    sampleWeight > 0 raises RuntimeError."""

    def __init__(self, nStack=1, selRate=0.5):
        super().__init__()
        self.nStack, self.selRate = nStack, selRate

    def forward(self, preds, targets, sampleWeight):
        rank = _batch_rank(preds, self.nStack, self.selRate)
        return _pseudo_rows(self, preds, targets, sampleWeight, ("rank", rank))


class JointDistLoss_mt(nn.Module):
    """utils/losses.py:213-243: consistency kept where the second input's per-stack softmax score
    reaches the int(B*K*(1 - selRate))-th smallest of its batch.  Returns (sum, nStack*#gate)."""

    def __init__(self, nStack=1, useKPsGate=False, useSampleWeight=False, selRate=0.5):
        super().__init__()
        self.nStack, self.useKPsGate, self.useSampleWeight, self.selRate = nStack, useKPsGate, useSampleWeight, selRate

    def forward(self, preds1, preds2, kpsGate=None, sampleWeight=None):
        _lib.require_gpu(preds1)
        a = preds1.contiguous()
        rank = _batch_rank(a, self.nStack, self.selRate)
        rows = Kn.RowSpec.same(*Kn.pred_rows(a, self.nStack))
        t = preds2.contiguous()
        gate = _f32c(kpsGate)
        sw = _sw_vec(sampleWeight)
        s, cnt, _, _ = _RowLoss.apply(a, t, rows, 1, ("rank", rank),
                                      bool(self.useKPsGate and gate is not None),
                                      bool(self.useSampleWeight and sw is not None), gate, sw)
        return s, int(cnt[0].item())


class JointFeatureDistLoss(nn.Module):
    """utils/losses.py:56-70 (FDL_type 'distance')."""

    def forward(self, inp1, inp2):
        _lib.require_gpu(inp1)
        bs, n, c = inp1.shape[:3]
        a = inp1.contiguous()
        t = inp2.contiguous()
        rows = Kn.RowSpec.flat(bs, n * c, a.numel() // (bs * n * c))
        s, _, _, _ = _RowLoss.apply(a, t, rows, 0, NO_RULE, False, False, None, None)
        return s, bs * n


class _FeaturesCov(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, rowmask):
        val, cnt, saved = Kn.fdl_cov_forward(f1, f2, rowmask)
        ctx.save_for_backward(f1, f2, cnt, *saved)
        ctx.rowmask = rowmask
        ctx.mark_non_differentiable(cnt)
        return val.view(()), cnt

    @staticmethod
    def backward(ctx, gv, _gc):
        f1, f2, cnt, cov, mu1, mu2 = ctx.saved_tensors
        d1 = torch.empty_like(f1) if ctx.needs_input_grad[0] else None
        d2 = torch.empty_like(f2) if ctx.needs_input_grad[1] else None
        Kn.fdl_cov_backward(f1, f2, ctx.rowmask, (cov, mu1, mu2), cnt, gv.reshape(1).contiguous().float(), d1, d2)
        return d1, d2, None


def features_cov(inp1, inp2, rowmask=None):
    """ProcessUtils.features_cov (utils/process.py:18-31) on device.  With a
    rowmask [B] (>0 = selected) the selection of projects/MT_UBPL.py:309-320 is
    fused in; the count is returned as a device int32[1]."""
    _lib.require_gpu(inp1)
    return _FeaturesCov.apply(inp1.contiguous(), inp2.contiguous(), _f32c(rowmask))


class AvgCounter(object):
    """utils/losses.py:357-371 (host-side running mean)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = 0
        self.avg = 0
        self.sum = 0
        self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = 0. if self.count == 0 else self.sum / self.count


class AvgCounters(object):
    """utils/losses.py:374-396."""

    def __init__(self, num=1):
        self.counters = [AvgCounter() for _ in range(num)]
        self.reset()

    def reset(self):
        for c in self.counters:
            c.reset()

    def update(self, idx, val, n=1):
        self.check_idx(idx)
        self.counters[idx].update(val, n)

    def avg(self):
        return [c.avg for c in self.counters]

    def sum(self):
        return [c.sum for c in self.counters]

    def check_idx(self, idx):
        while len(self.counters) < idx + 1:
            self.counters.append(AvgCounter())
