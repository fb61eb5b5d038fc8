"""Heatmap rendering (R1) and the loss kernels (L1-L5): row statistics, the selection rules'
finalizes, row gradients and the feature covariance loss."""
from typing import NamedTuple

import torch

from .. import _lib
from . import _check
from ._check import F32


# ------------------------------------------------------------------ R1
def render_heatmaps(kps, img_hw, inp_res, out_res, kernel_size=3.0, sigma=1.0, cutoff=0.01, kps_out=None):
    """kps [N,K,3] -> (hm [N,K,Rh,Rw], kps_out [N,K,3] with vis applied)."""
    _check._chk(kps, "kps")
    N, K, _ = kps.shape
    stride = inp_res / out_res
    rh, rw = int(img_hw[0] / stride), int(img_hw[1] / stride)
    hm = torch.empty((N, K, rh, rw), device=kps.device, dtype=F32)
    if kps_out is None:
        kps_out = torch.empty_like(kps)
    _lib.call("ubpl_render_heatmaps", kps, hm, kps_out, N, K, int(img_hw[0]), int(img_hw[1]), int(inp_res),
              int(out_res), float(kernel_size), float(sigma), float(cutoff))
    return hm, kps_out


# ------------------------------------------------------------------ L1-L4
class RowSpec(NamedTuple):
    """Rows of a (pred, target) pair for the heatmap loss kernels, in elements.  The predictions
    are contiguous [B,S,K,HW]: row (b,s,k) at (b*S + s)*K*HW + k*HW.  Its target is the mean over
    m < M of the maps at base + m*t_sm + b*t_sb + s*t_ss + k*HW of the flat target tensor.  The
    constructors below are the layouts that exist, and the only place a target stride is
    multiplied out: a wrong one reads valid memory of the wrong map, which nothing downstream
    can notice."""
    B: int
    S: int
    K: int
    HW: int
    t_sb: int
    t_ss: int
    t_sm: int
    M: int
    base: int

    @classmethod
    def ground_truth(cls, B, S, K, HW):
        """t [B,K,HW]: one map per (b,k), broadcast over the stacks."""
        return cls(B, S, K, HW, K * HW, 0, 0, 1, 0)

    @classmethod
    def same(cls, B, S, K, HW):
        """t [B,S,K,HW]: the predictions' own layout, stack by stack."""
        return cls(B, S, K, HW, S * K * HW, K * HW, 0, 1, 0)

    @classmethod
    def ensemble(cls, B, S, K, HW, M, St=1):
        """t [M,B,St,K,HW] (or [M,B,K,HW], St = 1): the member mean of the LAST stack, for every
        stack of the predictions."""
        return cls(B, S, K, HW, St * K * HW, 0, B * St * K * HW, M, (St - 1) * K * HW)

    @classmethod
    def flat(cls, B, C, HW):
        """a and t [B,C,HW] (the feature-distance loss): row (b,c) against row (b,c)."""
        return cls(B, 1, C, HW, C * HW, 0, 0, 1, 0)

    @property
    def a_sb(self):
        return self.S * self.K * self.HW

    @property
    def a_ss(self):
        return self.K * self.HW

    @property
    def t_stacks(self):
        """Stacks of distinct target rows: S, or 1 when one map per (b,k) serves every stack."""
        return 1 if self.t_ss == 0 else self.S

    def target(self, t):
        """The flat view of t at the base element: what the kernels take as the target pointer."""
        return t.reshape(-1)[self.base:]


def pred_rows(preds, nstack):
    """(B, S, K, HW) of the reference's reshape((bs, k, -1)) per stack (utils/losses.py:20-23):
    with nStack == 1 a row is (sample, preds.size(1)) — for a [B,1,K,R,R] model output that is
    ONE row per sample over K*R*R pixels."""
    B = preds.shape[0]
    if nstack == 1:
        K = preds.shape[1]
        return B, 1, K, preds.numel() // (B * K)
    K = preds.shape[2]
    return B, nstack, K, preds.numel() // (B * nstack * K)


def row_stats(a, t, rows, want_amax=False, want_tmax=False):
    """Per row of a against its target (rows: a RowSpec): the pixel mean of the squared
    difference, and where wanted the maxima of the row and of its target."""
    _check._chk(a, "preds")
    _check._chk(t, "targets")
    B, S, K, HW, t_sb, t_ss, t_sm, M, _ = rows
    n = B * S * K
    sq = torch.empty(n, device=a.device, dtype=F32)
    am = torch.empty(n, device=a.device, dtype=F32) if want_amax else None
    tm = torch.empty(n, device=a.device, dtype=F32) if want_tmax else None
    _lib.call("ubpl_heatmap_row_stats", a, rows.a_sb, rows.a_ss, rows.target(t), t_sb, t_ss, t_sm, M, B, S, K, HW,
              sq, am, tm)
    return sq, am, tm


def loss_finalize(kind, sq, amax, tmax, gate, sw, use_gate, use_sw, B, S, K, thr):
    dev = sq.device
    if kind == 3:                                               # the pseudo mask with a given selection
        _check._chk(gate, "gate")
        if gate is None or gate.numel() != B * K:
            raise ValueError("ubpl_amd: loss_finalize kind 3 takes a gate of [B,K] = %d x %d entries" % (B, K))
    out_sum = torch.empty(1, device=dev, dtype=F32)
    out_cnt = torch.empty(4, device=dev, dtype=torch.int32)
    score = torch.empty(K, device=dev, dtype=F32) if kind != 0 else None
    w = torch.empty(B * S * K, device=dev, dtype=F32)
    _lib.call("ubpl_loss_finalize", int(kind), sq, amax, tmax, gate, sw, int(use_gate), int(use_sw), B, S, K,
              float(thr), out_sum, out_cnt, score, w)
    return out_sum, out_cnt, score, w


def row_grad(a, t, rows, w, gscale, extra, da):
    """da = w[row] * gscale[0] * extra * (a - target) per row of rows (a RowSpec)."""
    B, S, K, HW, t_sb, t_ss, t_sm, M, _ = rows
    _lib.call("ubpl_heatmap_row_grad", a, rows.a_sb, rows.a_ss, rows.target(t), t_sb, t_ss, t_sm, M, B, S, K, HW, w,
              gscale, float(extra), da, 0)
    return da


# ------------------------------------------------------------------ L2b-L2d (rank / softmax-score selection)
MAX_SCORE_MAPS = 32        # ubpl_softmax_peak_scores: K maps of a pixel in registers
MAX_SCORE_MEMBERS = 8
MAX_RANK_GROUP = 8192      # ubpl_rank_threshold: one group in LDS


def softmax_peak_scores(x, x_sb, x_ss, x_sm, M, B, S, K, HW, out=None):
    """score [B*S*K] of the maps (b,s,k) = mean over m < M of x + m*x_sm + b*x_sb + s*x_ss + k*HW
    (x: a flat view at the base element): softmax across the K maps at every pixel, then the
    per-map maximum (utils/losses.py:137-138)."""
    _check._chk(x, "x")
    if not 1 <= K <= MAX_SCORE_MAPS or not 1 <= M <= MAX_SCORE_MEMBERS:
        raise ValueError("ubpl_amd: softmax_peak_scores takes 1..%d maps and 1..%d members, got %d and %d"
                         % (MAX_SCORE_MAPS, MAX_SCORE_MEMBERS, K, M))
    score = torch.empty(B * S * K, device=x.device, dtype=F32) if out is None else out
    _lib.call("ubpl_softmax_peak_scores", x, int(x_sb), int(x_ss), int(x_sm), M, B, S, K, HW, score)
    return score


def rank_threshold(scores, G, N, rank):
    """thr [G]: the rank-th smallest (0-based) of each group of N in scores [G*N], on the device."""
    _check._chk(scores, "scores")
    if not 1 <= N <= MAX_RANK_GROUP:
        raise ValueError("ubpl_amd: rank_threshold takes groups of 1..%d scores, got %d" % (MAX_RANK_GROUP, N))
    if not 0 <= rank < N:
        raise IndexError("ubpl_amd: rank %d is out of range for a group of %d scores" % (rank, N))
    thr = torch.empty(G, device=scores.device, dtype=F32)
    _lib.call("ubpl_rank_threshold", scores, G, N, int(rank), thr)
    return thr


def loss_finalize_ranked(kind, sq, ascore, tscore, athr, tthr, gate, sw, use_gate, use_sw, B, S, K, want_score=True):
    """loss_finalize for kinds 1 and 2 with given scores and per-stack device thresholds
    -> (sum [1], cnt [4] int32, score [K] or None, w [B*S*K])."""
    dev = sq.device
    if kind not in (1, 2):
        raise ValueError("ubpl_amd: loss_finalize_ranked is kind 1 or 2, got %r" % (kind,))
    if tscore is None or tthr is None or (kind == 2 and (ascore is None or athr is None)):
        raise ValueError("ubpl_amd: loss_finalize_ranked kind %d needs its scores and thresholds" % kind)
    out_sum = torch.empty(1, device=dev, dtype=F32)
    out_cnt = torch.empty(4, device=dev, dtype=torch.int32)
    score = torch.empty(K, device=dev, dtype=F32) if want_score else None
    w = torch.empty(B * S * K, device=dev, dtype=F32)
    _lib.call("ubpl_loss_finalize_ranked", int(kind), sq, ascore, tscore, athr, tthr, gate, sw, int(use_gate),
              int(use_sw), B, S, K, out_sum, out_cnt, score, w)
    return out_sum, out_cnt, score, w


def loss_finalize_rank(kind, sq, ascore, tscore, t_stacks, rank, gate, sw, use_gate, use_sw, B, S, K, want_score=True):
    """rank_threshold of every stack of both score sets and loss_finalize_ranked in one launch (the
    training step's form).  tscore [B,t_stacks,K] with t_stacks S, or 1: one target score per (b,k)
    for every stack -> (sum [1], cnt [4] int32, score [K] or None, w [B*S*K], thr [2*S]: rateThr1
    [S] (NaN for kind 1), then rateThr2 [S])."""
    dev = sq.device
    if kind not in (1, 2):
        raise ValueError("ubpl_amd: loss_finalize_rank is kind 1 or 2, got %r" % (kind,))
    if not 1 <= B * K <= MAX_RANK_GROUP:
        raise ValueError("ubpl_amd: loss_finalize_rank ranks 1..%d scores per stack, got %d" % (MAX_RANK_GROUP, B * K))
    if not 0 <= rank < B * K:
        raise IndexError("ubpl_amd: rank %d is out of range for %d scores" % (rank, B * K))
    out_sum = torch.empty(1, device=dev, dtype=F32)
    out_cnt = torch.empty(4, device=dev, dtype=torch.int32)
    score = torch.empty(K, device=dev, dtype=F32) if want_score else None
    w = torch.empty(B * S * K, device=dev, dtype=F32)
    thr = torch.empty(2 * S, device=dev, dtype=F32)
    _lib.call("ubpl_loss_finalize_rank", int(kind), sq, ascore, tscore, int(t_stacks), int(rank), gate, sw,
              int(use_gate), int(use_sw), B, S, K, thr, out_sum, out_cnt, score, w)
    return out_sum, out_cnt, score, w, thr


# ------------------------------------------------------------------ L5
def fdl_cov_forward(f1, f2, rowmask=None):
    _check._chk(f1, "f1")
    _check._chk(f2, "f2")
    B, S, C = f1.shape[:3]
    HW = f1[0, 0, 0].numel()
    dev = f1.device
    cov = torch.empty(B * S * C, device=dev, dtype=F32)
    mu1, mu2 = torch.empty_like(cov), torch.empty_like(cov)
    val = torch.empty(1, device=dev, dtype=F32)
    cnt = torch.empty(1, device=dev, dtype=torch.int32)
    _lib.call("ubpl_fdl_cov_forward", f1, f2, rowmask, B, S, C, HW, cov, mu1, mu2, val, cnt)
    return val, cnt, (cov, mu1, mu2)


def fdl_cov_backward(f1, f2, rowmask, saved, cnt, gscale, d1=None, d2=None, accumulate=False):
    B, S, C = f1.shape[:3]
    HW = f1[0, 0, 0].numel()
    cov, mu1, mu2 = saved
    _lib.call("ubpl_fdl_cov_backward", f1, f2, rowmask, cov, mu1, mu2, cnt, gscale, B, S, C, HW, d1, d2,
              int(accumulate))
    return d1, d2
