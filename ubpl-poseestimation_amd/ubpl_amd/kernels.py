"""Tensor-level wrappers over the C-ABI (no autograd here).

Each wrapper validates device / dtype / contiguity, allocates outputs with
the torch caching allocator on the input's device and enqueues on torch's
current stream.  Nothing here computes on the host.
"""
import math
import os

import torch

from . import _lib
from ._lib import call

F32 = torch.float32


def _chk(t, name, dtype=F32):
    if t is None:
        return
    _lib.require_gpu(t)
    if t.dtype != dtype:
        raise TypeError("ubpl_amd: %s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("ubpl_amd: %s must be contiguous" % name)


# ------------------------------------------------------------------ R1
def render_heatmaps(kps, img_hw, inp_res, out_res, kernel_size=3.0, sigma=1.0, cutoff=0.01, kps_out=None):
    """kps [N,K,3] -> (hm [N,K,Rh,Rw], kps_out [N,K,3] with vis applied)."""
    _chk(kps, "kps")
    N, K, _ = kps.shape
    stride = inp_res / out_res
    rh, rw = int(img_hw[0] / stride), int(img_hw[1] / stride)
    hm = torch.empty((N, K, rh, rw), device=kps.device, dtype=F32)
    if kps_out is None:
        kps_out = torch.empty_like(kps)
    call("ubpl_render_heatmaps", kps, hm, kps_out, N, K, int(img_hw[0]), int(img_hw[1]), int(inp_res), int(out_res),
         float(kernel_size), float(sigma), float(cutoff))
    return hm, kps_out


# ------------------------------------------------------------------ L1-L4
class RowGeom:
    """Row geometry of a (pred, target) pair for the heatmap loss kernels.
    a rows (b,s,k): a + b*a_sb + s*a_ss + k*HW; target rows: mean over m of
    t + m*t_sm + b*t_sb + s*t_ss + k*HW (strides in elements)."""

    def __init__(self, a, a_sb, a_ss, t, t_sb, t_ss, t_sm, M, B, S, K, HW):
        self.a, self.t = a, t
        self.a_off = 0
        self.args = (a_sb, a_ss, t_sb, t_ss, t_sm, M, B, S, K, HW)
        self.B, self.S, self.K, self.HW = B, S, K, HW
        self.a_ptr = a          # row base pointers as tensors (views at an element offset)
        self.t_ptr = t


def geom_stack(a, t, S, t_mode):
    """a: [B,S,K,R,R] (or [B,K,R,R] with S==1), contiguous.
    t_mode 'gt'    t [B,K,R,R] broadcast over stacks;
           'same'  t has a's layout;
           'ens'   t [M,B,St,K,R,R] (or [M,B,K,R,R]): mean over M of the LAST stack."""
    _chk(a, "preds")
    _chk(t, "targets")
    B = a.shape[0]
    K = a.shape[-3]
    HW = a.shape[-1] * a.shape[-2]
    a_sb, a_ss = S * K * HW, K * HW
    if t_mode == "gt":
        return RowGeom(a, a_sb, a_ss, t, K * HW, 0, 0, 1, B, S, K, HW)
    if t_mode == "same":
        return RowGeom(a, a_sb, a_ss, t, a_sb, a_ss, 0, 1, B, S, K, HW)
    M = t.shape[0]
    St = t.shape[2] if t.dim() == 6 else 1
    g = RowGeom(a, a_sb, a_ss, t, St * K * HW, 0, B * St * K * HW, M, B, S, K, HW)
    g.t_ptr = t.reshape(-1)[(St - 1) * K * HW:]
    return g


def geom_rows(a, a_base_elems, a_sb, t, t_base_elems, t_sb, B, K, HW, t_sm=0, M=1):
    """Single-stack rows with explicit base offsets/strides (e.g. last-stack slices)."""
    g = RowGeom(a, a_sb, 0, t, t_sb, 0, t_sm, M, B, 1, K, HW)
    g.a_ptr = a.reshape(-1)[a_base_elems:]
    g.t_ptr = t.reshape(-1)[t_base_elems:]
    return g


def row_stats(g, want_amax=False, want_tmax=False):
    dev = g.a.device
    rows = g.B * g.S * g.K
    sq = torch.empty(rows, device=dev, dtype=F32)
    am = torch.empty(rows, device=dev, dtype=F32) if want_amax else None
    tm = torch.empty(rows, device=dev, dtype=F32) if want_tmax else None
    a_sb, a_ss, t_sb, t_ss, t_sm, M, B, S, K, HW = g.args
    call("ubpl_heatmap_row_stats", g.a_ptr, a_sb, a_ss, g.t_ptr, t_sb, t_ss, t_sm, M, B, S, K, HW, sq, am, tm)
    return sq, am, tm


def loss_finalize(kind, sq, amax, tmax, gate, sw, use_gate, use_sw, B, S, K, thr):
    dev = sq.device
    if kind == 3:                                               # the pseudo mask with a given selection
        _chk(gate, "gate")
        if gate is None or gate.numel() != B * K:
            raise ValueError("ubpl_amd: loss_finalize kind 3 takes a gate of [B,K] = %d x %d entries" % (B, K))
    out_sum = torch.empty(1, device=dev, dtype=F32)
    out_cnt = torch.empty(4, device=dev, dtype=torch.int32)
    score = torch.empty(K, device=dev, dtype=F32) if kind != 0 else None
    w = torch.empty(B * S * K, device=dev, dtype=F32)
    call("ubpl_loss_finalize", int(kind), sq, amax, tmax, gate, sw, int(use_gate), int(use_sw), B, S, K, float(thr),
         out_sum, out_cnt, score, w)
    return out_sum, out_cnt, score, w


def row_grad(g, w, gscale, extra, da, accumulate=False):
    a_sb, a_ss, t_sb, t_ss, t_sm, M, B, S, K, HW = g.args
    call("ubpl_heatmap_row_grad", g.a_ptr, a_sb, a_ss, g.t_ptr, t_sb, t_ss, t_sm, M, B, S, K, HW, w, gscale,
         float(extra), da, int(accumulate))
    return da


# ------------------------------------------------------------------ L2b-L2d (rank / softmax-score selection)
MAX_SCORE_MAPS = 32        # ubpl_softmax_peak_scores: K maps of a pixel in registers
MAX_SCORE_MEMBERS = 8
MAX_RANK_GROUP = 8192      # ubpl_rank_threshold: one group in LDS


def softmax_peak_scores(x, x_sb, x_ss, x_sm, M, B, S, K, HW, out=None):
    """score [B*S*K] of the maps (b,s,k) = mean over m < M of x + m*x_sm + b*x_sb + s*x_ss + k*HW
    (x: a flat view at the base element): softmax across the K maps at every pixel, then the
    per-map maximum (utils/losses.py:137-138)."""
    _chk(x, "x")
    if not 1 <= K <= MAX_SCORE_MAPS or not 1 <= M <= MAX_SCORE_MEMBERS:
        raise ValueError("ubpl_amd: softmax_peak_scores takes 1..%d maps and 1..%d members, got %d and %d"
                         % (MAX_SCORE_MAPS, MAX_SCORE_MEMBERS, K, M))
    score = torch.empty(B * S * K, device=x.device, dtype=F32) if out is None else out
    call("ubpl_softmax_peak_scores", x, int(x_sb), int(x_ss), int(x_sm), M, B, S, K, HW, score)
    return score


def rank_threshold(scores, G, N, rank, out=None):
    """thr [G]: the rank-th smallest (0-based) of each group of N in scores [G*N], on the device."""
    _chk(scores, "scores")
    if not 1 <= N <= MAX_RANK_GROUP:
        raise ValueError("ubpl_amd: rank_threshold takes groups of 1..%d scores, got %d" % (MAX_RANK_GROUP, N))
    if not 0 <= rank < N:
        raise IndexError("ubpl_amd: rank %d is out of range for a group of %d scores" % (rank, N))
    thr = torch.empty(G, device=scores.device, dtype=F32) if out is None else out
    call("ubpl_rank_threshold", scores, G, N, int(rank), thr)
    return thr


def loss_finalize_ranked(kind, sq, ascore, tscore, athr, tthr, gate, sw, use_gate, use_sw, B, S, K,
                         want_score=True, out=None):
    """loss_finalize for kinds 1 and 2 with given scores and per-stack device thresholds
    -> (sum [1], cnt [4] int32, score [K] or None, w [B*S*K])."""
    dev = sq.device
    if kind not in (1, 2):
        raise ValueError("ubpl_amd: loss_finalize_ranked is kind 1 or 2, got %r" % (kind,))
    if tscore is None or tthr is None or (kind == 2 and (ascore is None or athr is None)):
        raise ValueError("ubpl_amd: loss_finalize_ranked kind %d needs its scores and thresholds" % kind)
    out_sum, out_cnt, score, w = out if out is not None else (None,) * 4
    out_sum = torch.empty(1, device=dev, dtype=F32) if out_sum is None else out_sum
    out_cnt = torch.empty(4, device=dev, dtype=torch.int32) if out_cnt is None else out_cnt
    if score is None and want_score:
        score = torch.empty(K, device=dev, dtype=F32)
    w = torch.empty(B * S * K, device=dev, dtype=F32) if w is None else w
    call("ubpl_loss_finalize_ranked", int(kind), sq, ascore, tscore, athr, tthr, gate, sw, int(use_gate), int(use_sw),
         B, S, K, out_sum, out_cnt, score, w)
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
    call("ubpl_loss_finalize_rank", int(kind), sq, ascore, tscore, int(t_stacks), int(rank), gate, sw, int(use_gate),
         int(use_sw), B, S, K, thr, out_sum, out_cnt, score, w)
    return out_sum, out_cnt, score, w, thr


# ------------------------------------------------------------------ L5
def fdl_cov_forward(f1, f2, rowmask=None):
    _chk(f1, "f1")
    _chk(f2, "f2")
    B, S, C = f1.shape[:3]
    HW = f1[0, 0, 0].numel()
    dev = f1.device
    cov = torch.empty(B * S * C, device=dev, dtype=F32)
    mu1, mu2 = torch.empty_like(cov), torch.empty_like(cov)
    val = torch.empty(1, device=dev, dtype=F32)
    cnt = torch.empty(1, device=dev, dtype=torch.int32)
    call("ubpl_fdl_cov_forward", f1, f2, rowmask, B, S, C, HW, cov, mu1, mu2, val, cnt)
    return val, cnt, (cov, mu1, mu2)


def fdl_cov_backward(f1, f2, rowmask, saved, cnt, gscale, d1=None, d2=None, accumulate=False):
    B, S, C = f1.shape[:3]
    HW = f1[0, 0, 0].numel()
    cov, mu1, mu2 = saved
    call("ubpl_fdl_cov_backward", f1, f2, rowmask, cov, mu1, mu2, cnt, gscale, B, S, C, HW, d1, d2, int(accumulate))
    return d1, d2


# ------------------------------------------------------------------ D1-D4
def decode_heatmaps(hm, tinv=None):
    """hm [N,K,H,W] -> (raw [N,K,2], preds [N,K,2] or None, scores [N,K])."""
    _chk(hm, "heatmap")
    N, K, H, W = hm.shape
    dev = hm.device
    raw = torch.empty((N, K, 2), device=dev, dtype=F32)
    preds = torch.empty((N, K, 2), device=dev, dtype=F32) if tinv is not None else None
    scores = torch.empty((N, K), device=dev, dtype=F32)
    if tinv is not None:
        _chk(tinv, "tinv", torch.float64)
    call("ubpl_decode_heatmaps", hm, N, K, H, W, tinv, raw, preds, scores)
    return raw, preds, scores


def flip_perm(K, pairs):
    """Host int32 [K] joint permutation of the flip test's left/right swap
    (utils/udaap/transforms.py:20-57 flip_back): perm[a] = b, perm[b] = a for
    every pair, identity elsewhere.  Indices in [0, K), each joint in at most
    one pair (ValueError otherwise)."""
    perm = list(range(K))
    seen = set()
    for pr in pairs:
        if len(pr) != 2:
            raise ValueError("ubpl_amd: a flip pair is two joint indices, got %r" % (pr,))
        a, b = int(pr[0]), int(pr[1])
        for j in (a, b):
            if not 0 <= j < K:
                raise ValueError("ubpl_amd: flip pair %r names joint %d of %d" % (tuple(pr), j, K))
        if a == b or a in seen or b in seen:
            raise ValueError("ubpl_amd: flip pair %r repeats a joint" % (tuple(pr),))
        seen.update((a, b))
        perm[a], perm[b] = b, a
    return torch.tensor(perm, dtype=torch.int32)


def _chk_maps(t, name, counts, strides, plane, signed=True):
    """t (None: nothing to check) holds strided maps: counts[i] steps of strides[i] floats, then
    one block of `plane` floats.  signed=False: a negative stride is refused as well."""
    if t is None:
        return
    _chk(t, name)
    need = sum((n - 1) * st for n, st in zip(counts, strides)) + plane
    if t.numel() < need or not (signed or min(strides) >= 0):
        if len(counts) == 1:
            raise ValueError("ubpl_amd: %s holds %d floats, %d maps of stride %d need %d"
                             % (name, t.numel(), counts[0], strides[0], need))
        if len(counts) > 2:
            raise ValueError("ubpl_amd: %s holds %d floats, %s maps of strides %s need %d"
                             % (name, t.numel(), " x ".join(map(str, counts)), ", ".join(map(str, strides)), need))
        raise ValueError("ubpl_amd: %s holds %d floats, %d x %d maps of strides %d, %d need %d"
                         % (name, t.numel(), *counts, *strides, need))


def _chk_entries(perm, K, tinv, swap=None, V=None, N=None):
    """perm int32 [K], swap int32 [V] and tinv float64 ([N,6] where N is given), each or None."""
    _chk(swap, "swap", torch.int32)
    _chk(perm, "perm", torch.int32)
    _chk(tinv, "tinv", torch.float64)
    if swap is not None and swap.numel() != V:
        raise ValueError("ubpl_amd: swap has %d entries for %d views" % (swap.numel(), V))
    if perm is not None and perm.numel() != K:
        raise ValueError("ubpl_amd: perm has %d entries for %d joints" % (perm.numel(), K))
    if N is not None and tinv is not None and tinv.numel() != N * 6:
        raise ValueError("ubpl_amd: tinv has %d entries for %d samples" % (tinv.numel(), N))


def _outs(out, dev, *rows):
    """The outputs of a wrapper: `out` as given, or per (shape, wanted) row a fresh float32 tensor
    or None."""
    if out is not None:
        return tuple(out)
    return tuple(torch.empty(shape, device=dev, dtype=F32) if wanted else None for shape, wanted in rows)


def decode_heatmaps_flip(hm, hm_flip, sb, N, K, H, W, perm=None, tinv=None, want_merged=False, out=None):
    """Flip-test decode (ubpl_decode_heatmaps_flip): hm / hm_flip are tensors whose
    first element is map (0, 0) — views at an element offset, e.g. the last stack of
    a [B,S,K,H,W] output — with batch stride sb floats; hm_flip None: a plain
    strided decode.  perm: device int32 [K] (flip_perm(...).to(device)) or None.
    -> (raw [N,K,2], preds [N,K,2] or None, scores [N,K], merged [N,K,H,W] or None);
    out = (raw, preds, scores, merged): write into these instead of allocating."""
    _chk_maps(hm, "hm", (N,), (sb,), K * H * W)
    _chk_maps(hm_flip, "hm_flip", (N,), (sb,), K * H * W)
    _chk_entries(perm, K, tinv)
    raw, preds, scores, merged = _outs(out, hm.device, ((N, K, 2), True), ((N, K, 2), tinv is not None),
                                       ((N, K), True), ((N, K, H, W), want_merged))
    call("ubpl_decode_heatmaps_flip", hm, hm_flip, int(sb), N, K, H, W, perm, tinv, merged, raw, preds, scores)
    return raw, preds, scores, merged


def ensemble_pseudo(hm, sm, sb, M, N, K, H, W, thr, tinv=None, want_mean=False, out=None):
    """UBPL ensemble pseudo-labels (ubpl_ensemble_pseudo; JointPseudoLoss3's target and
    mask, utils/losses.py:176-210): hm is a tensor whose first element is member 0's map
    (0, 0), member stride sm and batch stride sb floats — a [M,N,K,H,W] buffer, or the last
    stacks of [M,B,S,K,H,W] through a view at an element offset.  1 <= M <= 8.  thr: device
    float32 [1] (read by the kernel).
    -> (ens_raw [N,K,2], ens_preds [N,K,2] or None, ens_score [N,K], member_score [M,N,K],
        disagree [M,N,K], select [M,N,K] 0/1, mean_hm [N,K,H,W] or None);
    out = the same tuple: write into these instead of allocating (select is required)."""
    if not 1 <= M <= 8:
        raise ValueError("ubpl_amd: ensemble_pseudo takes 1 to 8 members, got %d" % M)
    _chk_maps(hm, "hm", (M, N), (sm, sb), K * H * W)
    _chk(thr, "thr")
    _chk(tinv, "tinv", torch.float64)
    if thr is None or thr.numel() != 1:
        raise ValueError("ubpl_amd: thr is a device float32 tensor of one element")
    ens_raw, ens_preds, ens_score, member_score, disagree, select, mean_hm = _outs(
        out, hm.device, ((N, K, 2), True), ((N, K, 2), tinv is not None), ((N, K), True), ((M, N, K), True),
        ((M, N, K), True), ((M, N, K), True), ((N, K, H, W), want_mean))
    if select is None:
        raise ValueError("ubpl_amd: ensemble_pseudo always writes select")
    call("ubpl_ensemble_pseudo", hm, int(sm), int(sb), M, N, K, H, W, tinv, thr, mean_hm, ens_raw, ens_preds, ens_score,
         member_score, disagree, select)
    return ens_raw, ens_preds, ens_score, member_score, disagree, select, mean_hm


REFINE_MODES = {"quarter": 1, "taylor": 2}
MAX_BLUR_RADIUS = 5


def blur_taps(sigma):
    """Host float32 [radius + 1]: the half w[0..radius] of the Gaussian blur kernel of
    ubpl_refine_peaks' Taylor mode.  sigma <= 0: [1.0] (no blur).  Otherwise radius =
    ceil(2.5 sigma), w[j] = exp(-j^2 / (2 sigma^2)) normalised so that the full
    2 radius + 1 kernel sums to 1, in float64 rounded to float32.  ValueError above
    radius 5 (sigma > 2.0)."""
    sigma = float(sigma)
    if not sigma > 0:
        return torch.ones(1, dtype=F32)
    radius = int(math.ceil(2.5 * sigma))
    if radius > MAX_BLUR_RADIUS:
        raise ValueError("ubpl_amd: blur sigma %g needs radius %d, at most %d (sigma <= 2.0)"
                         % (sigma, radius, MAX_BLUR_RADIUS))
    w = [math.exp(-j * j / (2.0 * sigma * sigma)) for j in range(radius + 1)]
    total = w[0] + 2.0 * sum(w[1:])
    return torch.tensor([v / total for v in w], dtype=torch.float64).to(F32)


def refine_peaks(hm, hm_flip, sb, N, K, H, W, perm, raw, mode, taps, tinv=None, out=None):
    """Sub-pixel refinement of decoded peaks (ubpl_refine_peaks): hm / hm_flip / sb / perm
    exactly as given to decode_heatmaps_flip, raw [N,K,2] the peaks it wrote.  mode
    "quarter" or "taylor" (or 1 / 2); taps: device float32 [radius + 1]
    (blur_taps(sigma).to(device); read in Taylor mode).
    -> (raw_sub [N,K,2], preds_sub [N,K,2] or None, how [N,K] = the rule taken, 0 / 1 / 2);
    out = the same tuple: write into these instead of allocating."""
    mode = REFINE_MODES.get(mode, mode)
    if mode not in (1, 2):
        raise ValueError("ubpl_amd: refine mode is one of %s, got %r" % (", ".join(REFINE_MODES), mode))
    _chk_maps(hm, "hm", (N,), (sb,), K * H * W)
    _chk_maps(hm_flip, "hm_flip", (N,), (sb,), K * H * W)
    _chk(raw, "raw")
    _chk(taps, "taps")
    _chk_entries(perm, K, tinv)
    if raw is None or raw.numel() != N * K * 2:
        raise ValueError("ubpl_amd: raw is the decode's [N,K,2] peaks")
    if taps is None or not 1 <= taps.numel() <= MAX_BLUR_RADIUS + 1:
        raise ValueError("ubpl_amd: taps holds 1 to %d floats (blur_taps)" % (MAX_BLUR_RADIUS + 1))
    raw_sub, preds_sub, how = _outs(out, hm.device, ((N, K, 2), True), ((N, K, 2), tinv is not None), ((N, K), True))
    call("ubpl_refine_peaks", hm, hm_flip, int(sb), N, K, H, W, perm, raw, mode, taps, taps.numel() - 1, tinv,
         raw_sub, preds_sub, how)
    return raw_sub, preds_sub, how


# ---- multi-view test-time augmentation (csrc/decode_warp.hip; the convention: DESIGN.md §4)
MAX_VIEWS = 16
F64 = torch.float64


def _mat6(m):
    return torch.as_tensor(m, dtype=F64).reshape(-1, 6)


def compose_pixels(a, b):
    """Pixel matrices [...,6] (output pixel -> source pixel) -> a o b: b first, then a, in float64."""
    a, b = _mat6(a), _mat6(b)
    out = torch.empty(torch.broadcast_shapes(a.shape, b.shape), dtype=F64)
    for r in (0, 3):
        out[:, r + 0] = a[:, r] * b[:, 0] + a[:, r + 1] * b[:, 3]
        out[:, r + 1] = a[:, r] * b[:, 1] + a[:, r + 1] * b[:, 4]
        out[:, r + 2] = a[:, r] * b[:, 2] + a[:, r + 1] * b[:, 5] + a[:, r + 2]
    return out


def mirror_pixels(W):
    """m(x, y) = (W - 1 - x, y) as a pixel matrix [1,6] (float64)."""
    return torch.tensor([[-1.0, 0.0, W - 1.0, 0.0, 1.0, 0.0]], dtype=F64)


def affine_theta_to_pixels(theta, H, W):
    """theta [V,2,3] (or [2,3]) of F.affine_grid(..., align_corners=True) on [H,W] planes — the
    reference's affine_back2 convention, utils/augment.py:36-47: normalised output position ->
    normalised source position, -1 and 1 the centres of the first and last pixel — -> the pixel
    matrices [V,6] float64 (output pixel -> source pixel) that sample the same positions."""
    if H < 2 or W < 2:
        raise ValueError("ubpl_amd: align_corners=True normalises over H - 1 and W - 1; %dx%d has none" % (H, W))
    t = torch.as_tensor(theta, dtype=F64).reshape(-1, 2, 3)
    hx, hy = (W - 1) / 2.0, (H - 1) / 2.0
    m = torch.empty((t.shape[0], 6), dtype=F64)
    m[:, 0] = t[:, 0, 0]
    m[:, 1] = t[:, 0, 1] * (hx / hy)
    m[:, 2] = hx * (t[:, 0, 2] + 1.0 - t[:, 0, 0] - t[:, 0, 1])
    m[:, 3] = t[:, 1, 0] * (hy / hx)
    m[:, 4] = t[:, 1, 1]
    m[:, 5] = hy * (t[:, 1, 2] + 1.0 - t[:, 1, 0] - t[:, 1, 1])
    return m


def affine_pixels_to_theta(mat, H, W):
    """The inverse of affine_theta_to_pixels: pixel matrices [V,6] -> theta [V,2,3] float64."""
    if H < 2 or W < 2:
        raise ValueError("ubpl_amd: align_corners=True normalises over H - 1 and W - 1; %dx%d has none" % (H, W))
    m = _mat6(mat)
    hx, hy = (W - 1) / 2.0, (H - 1) / 2.0
    t = torch.empty((m.shape[0], 2, 3), dtype=F64)
    t[:, 0, 0] = m[:, 0]
    t[:, 0, 1] = m[:, 1] * (hy / hx)
    t[:, 0, 2] = m[:, 2] / hx - 1.0 + t[:, 0, 0] + t[:, 0, 1]
    t[:, 1, 0] = m[:, 3] * (hx / hy)
    t[:, 1, 1] = m[:, 4]
    t[:, 1, 2] = m[:, 5] / hy - 1.0 + t[:, 1, 0] + t[:, 1, 1]
    return t


def _about_centre(a, S):
    """q -> c + a (q - c), c = ((S-1)/2, (S-1)/2), a a 2x2 nested list -> one matrix row [6]."""
    c = (S - 1) / 2.0
    return [a[0][0], a[0][1], c - a[0][0] * c - a[0][1] * c, a[1][0], a[1][1], c - a[1][0] * c - a[1][1] * c]


def view_matrices(views, flip, R, H):
    """The matrices of test-time-augmentation views on square planes ("Multi-view
    decode").  views: [(angle_deg, zoom), ...]; A = R(angle) / zoom, R(a) = [[cos a, -sin a],
    [sin a, cos a]], y down, so zoom > 1 magnifies.  The view image is view(q) = img(c + A (q - c));
    the original frame's heatmap at p samples the view's at q = c_h + A^-1 (p - c_h).  flip: every
    view once more mirrored, after the plain ones — view_f(q) = view(m(q)), its heatmap sampled at
    m(q), m(x, y) = (S - 1 - x, y) — with swap = 1 (the joint permutation is not geometry).
    -> host (img_mat [V,6] on [R,R] planes, hm_mat [V,6] on [H,H] planes, both output pixel ->
    source pixel, float64 rounded to float32; swap [V] int32)."""
    img, hm = [], []
    for angle, zoom in views:
        a = math.radians(float(angle))
        co, si, z = math.cos(a), math.sin(a), float(zoom)
        img.append(_about_centre([[co / z, -si / z], [si / z, co / z]], R))
        hm.append(_about_centre([[co * z, si * z], [-si * z, co * z]], H))
    img, hm = _mat6(img), _mat6(hm)
    swap = [0] * len(img)
    if flip:
        # view_f(q) = img(M m(q)): M o m on the image; the heatmap is read at m(q(p)): m o M
        img = torch.cat([img, compose_pixels(img, mirror_pixels(R))])
        hm = torch.cat([hm, compose_pixels(mirror_pixels(H), hm)])
        swap = swap + [1] * len(swap)
    return img.to(F32), hm.to(F32), torch.tensor(swap, dtype=torch.int32)


def warp_views(src, mat, out=None):
    """Views of a batch (ubpl_warp_views): src [N,C,H,W], mat device float32 [V,6] pixel matrices
    (output pixel -> source pixel) -> out [V,N,C,H,W] (or any contiguous tensor of that many
    floats, e.g. rows of a [V*N,C,H,W] batch), bilinear, zero outside; an identity view copies."""
    _chk(src, "src")
    _chk(mat, "mat")
    if src.dim() != 4 or mat.dim() != 2 or mat.shape[1] != 6:
        raise ValueError("ubpl_amd: warp_views takes src [N,C,H,W] and mat [V,6]")
    N, C, H, W = src.shape
    V = mat.shape[0]
    out, = _outs(None if out is None else (out,), src.device, ((V, N, C, H, W), True))
    _chk(out, "out")
    if out.numel() != V * src.numel():
        raise ValueError("ubpl_amd: out holds %d floats, %d views of %d need %d"
                         % (out.numel(), V, src.numel(), V * src.numel()))
    if V * src.numel():
        lo, hi = src.data_ptr(), src.data_ptr() + src.numel() * 4
        if out.data_ptr() < hi and lo < out.data_ptr() + out.numel() * 4:
            raise ValueError("ubpl_amd: warp_views writes a tensor that does not overlap its input")
    call("ubpl_warp_views", src, N, C, H, W, mat, V, out)
    return out


def decode_heatmaps_views(hm, sv, sb, V, N, K, H, W, mat, swap=None, perm=None, tinv=None, want_merged=False,
                          out=None):
    """Multi-view decode (ubpl_decode_heatmaps_views): hm is a tensor whose first element is view
    0's map (0, 0), view stride sv and batch stride sb floats — a [V,N,K,H,W] buffer, or the last
    stacks of a view-major [V*N,S,K,H,W] output through a view at an element offset.  mat: device
    float32 [V,6] (view_matrices' hm_mat); swap: device int32 [V] or None; perm: device int32 [K]
    or None.  1 <= V <= 16.
    -> (raw [N,K,2], preds [N,K,2] or None, scores [N,K], merged [N,K,H,W] or None);
    out = (raw, preds, scores, merged): write into these instead of allocating."""
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError("ubpl_amd: decode_heatmaps_views takes 1 to %d views, got %d" % (MAX_VIEWS, V))
    _chk_maps(hm, "hm", (V, N), (sv, sb), K * H * W, signed=False)
    _chk(mat, "mat")
    if mat is None or mat.numel() != V * 6:
        raise ValueError("ubpl_amd: mat is [V,6], one pixel matrix per view")
    _chk_entries(perm, K, tinv, swap, V)
    raw, preds, scores, merged = _outs(out, hm.device, ((N, K, 2), True), ((N, K, 2), tinv is not None),
                                       ((N, K), True), ((N, K, H, W), want_merged))
    call("ubpl_decode_heatmaps_views", hm, int(sv), int(sb), V, N, K, H, W, mat, swap, perm, tinv, merged, raw, preds,
         scores)
    return raw, preds, scores, merged


# ---- view-consistency uncertainty (csrc/uncertainty.hip; the rule: include/ubpl_hip.h)
def view_back_matrices(hm_mat):
    """view_matrices' hm_mat [V,6] (original-frame heatmap pixel -> view heatmap pixel) -> host
    float32 [V,6], view heatmap pixel -> original-frame heatmap pixel: the inverse of each (float32)
    matrix taken in float64 and rounded once.  ValueError on a singular matrix."""
    m = _mat6(hm_mat.detach().cpu() if torch.is_tensor(hm_mat) else hm_mat)
    det = m[:, 0] * m[:, 4] - m[:, 1] * m[:, 3]
    if not bool(((det != 0) & torch.isfinite(det)).all()):
        raise ValueError("ubpl_amd: view_back_matrices takes invertible pixel matrices")
    out = torch.empty_like(m)
    out[:, 0], out[:, 1] = m[:, 4] / det, -m[:, 1] / det
    out[:, 3], out[:, 4] = -m[:, 3] / det, m[:, 0] / det
    out[:, 2] = -(out[:, 0] * m[:, 2] + out[:, 1] * m[:, 5])
    out[:, 5] = -(out[:, 3] * m[:, 2] + out[:, 4] * m[:, 5])
    return out.to(F32)


UNC_OUTPUTS = ("pts", "legal", "int_dist", "aug_coord", "ext_dist", "aext_dist", "ext_views", "mix_dist", "unc",
               "select")


def view_uncertainty(raw, sm, M, V, N, K, back, dist_thr, swap=None, perm=None, tinv=None, out=None):
    """View-consistency uncertainty (ubpl_view_uncertainty; utils/business.py pseudo_cal_unc /
    assess_pseudo_unc2): raw is a tensor whose first element is member 0's point of view 0, sample
    0, joint 0 — per member a view-major [V*N,K,2] block of 1-based view-frame peaks, member stride
    sm floats.  back: device float32 [V,6] (view_back_matrices(hm_mat).to(device)); dist_thr: device
    float32 [1] (read by the kernel); swap: device int32 [V] or None; perm: device int32 [K] or
    None; tinv: device float64 [N,6] or None (points in heatmap cells).  1 <= M <= 8, 2 <= V <= 16.
    -> (pts [M,V,N,K,2], legal [M,N,K], int_dist [M,N,K], aug_coord [M,N,K,2], ext_dist [N,K],
        aext_dist [N,K], ext_views [N,K], mix_dist [M,N,K], unc [M,N,K], select [M,N,K] 0/1);
    out = the same tuple: write into these instead of allocating (select is required)."""
    if not 1 <= M <= 8:
        raise ValueError("ubpl_amd: view_uncertainty takes 1 to 8 members, got %d" % M)
    if not 2 <= V <= MAX_VIEWS:
        raise ValueError("ubpl_amd: view_uncertainty takes 2 to %d views, got %d" % (MAX_VIEWS, V))
    _chk(raw, "raw")
    need = (M - 1) * sm + V * N * K * 2
    if raw is None or sm < 0 or (M > 1 and sm < V * N * K * 2) or raw.numel() < need:
        raise ValueError("ubpl_amd: raw holds %d floats, %d members of stride %d with %d x %d x %d points need %d"
                         % (0 if raw is None else raw.numel(), M, sm, V, N, K, need))
    _chk(back, "back")
    _chk(dist_thr, "dist_thr")
    if back is None or back.numel() != V * 6:
        raise ValueError("ubpl_amd: back is [V,6], one pixel matrix per view")
    if dist_thr is None or dist_thr.numel() != 1:
        raise ValueError("ubpl_amd: dist_thr is a device float32 tensor of one element")
    _chk_entries(perm, K, tinv, swap, V, N)
    mnk, nk = (M, N, K), (N, K)                                 # (in UNC_OUTPUTS' order)
    outs = _outs(out, raw.device, *((shape, True) for shape in ((M, V, N, K, 2), mnk, mnk, (M, N, K, 2), nk, nk, nk,
                                                                mnk, mnk, mnk)))
    if len(outs) != len(UNC_OUTPUTS):
        raise ValueError("ubpl_amd: view_uncertainty writes %d outputs, got %d" % (len(UNC_OUTPUTS), len(outs)))
    if outs[-1] is None:
        raise ValueError("ubpl_amd: view_uncertainty always writes select")
    call("ubpl_view_uncertainty", raw, int(sm), M, V, N, K, back, swap, perm, tinv, dist_thr, *outs)
    return outs


def view_uncertainty_samples(raw, sm, sv, M, V, N, K, back, dist_thr, out=None):
    """view_uncertainty where every (view, sample) has its own matrix (ubpl_view_uncertainty_samples;
    the training step's augmented views): member m's point of view v, sample n, joint k is the pair
    at raw[m*sm + v*sv + (n*K + k)*2] — a [V,M,N,K,2] buffer has sm = N*K*2, sv = M*N*K*2 — and
    back: device float32 [V,N,6] (train_back_matrices).  No swap / perm / tinv: the points come out
    in the frame back maps to.  dist_thr: device float32 [1].  1 <= M <= 8, 2 <= V <= 16.
    -> view_uncertainty's ten outputs and gate [N,K] = 1 where every member is selected;
    out = the same eleven: write into these instead of allocating (None: not wanted; select is
    required)."""
    if not 1 <= M <= 8:
        raise ValueError("ubpl_amd: view_uncertainty_samples takes 1 to 8 members, got %d" % M)
    if not 2 <= V <= MAX_VIEWS:
        raise ValueError("ubpl_amd: view_uncertainty_samples takes 2 to %d views, got %d" % (MAX_VIEWS, V))
    _chk(raw, "raw")
    blk = N * K * 2
    need = (M - 1) * sm + (V - 1) * sv + blk
    nested = M == 1 or sm >= (V - 1) * sv + blk or sv >= (M - 1) * sm + blk
    if raw is None or sm < 0 or sv < blk or (M > 1 and sm < blk) or not nested or raw.numel() < need:
        raise ValueError("ubpl_amd: raw holds %d floats, %d members of stride %d and %d views of stride %d with "
                         "%d x %d points need %d" % (0 if raw is None else raw.numel(), M, sm, V, sv, N, K, need))
    _chk(back, "back")
    _chk(dist_thr, "dist_thr")
    if back is None or back.numel() != V * N * 6:
        raise ValueError("ubpl_amd: back is [V,N,6], one pixel matrix per view and sample")
    if dist_thr is None or dist_thr.numel() != 1:
        raise ValueError("ubpl_amd: dist_thr is a device float32 tensor of one element")
    _chk_entries(None, K, None)
    mnk, nk = (M, N, K), (N, K)                                 # (UNC_OUTPUTS' order, then gate)
    outs = _outs(out, raw.device, *((shape, True) for shape in ((M, V, N, K, 2), mnk, mnk, (M, N, K, 2), nk, nk, nk,
                                                                mnk, mnk, mnk, nk)))
    if len(outs) != len(UNC_OUTPUTS) + 1:
        raise ValueError("ubpl_amd: view_uncertainty_samples writes %d outputs, got %d"
                         % (len(UNC_OUTPUTS) + 1, len(outs)))
    if outs[-2] is None:
        raise ValueError("ubpl_amd: view_uncertainty_samples always writes select")
    call("ubpl_view_uncertainty_samples", raw, int(sm), int(sv), M, V, N, K, back, dist_thr, *outs)
    return outs


def train_back_matrices(viewmat, R, H):
    """The back matrices of the training step's views for view_uncertainty_samples.
    viewmat: [V,N,6] (or a list of V [N,6]) float32, DeviceAugment.views(with_mats=True)'s matrices
    (warp_matrix: 0-based view input pixel -> 0-based source-image pixel), on any device; R the
    views' input side, H the heatmaps'.  -> float32 [V,N,6] on viewmat's device: 0-based heatmap
    cell -> source-image pixel, back = viewmat o C.

    The cell convention C is the renderer's, inverted.  render_batch centres the Gaussian of a
    keypoint at view pixel x on the 0-based cell x / (R/H) (csrc/render.hip: cx = trunc(x) /
    stride), so C(c) = (R/H) c on both axes, and a decoded 1-based peak raw enters the kernel as
    c = raw - 1.  The keypoint coordinates the loader hands the renderer are taken as the view's
    pixel coordinates, as the renderer takes them; the reference's keypoint path (transform_point:
    p - 1, the float64 product truncated, + 1; kps_fliplr: W - x) lands within a pixel of where
    warp_matrix puts the same source pixel (DESIGN.md §4 has the measured offsets).
    Composed in float64 and rounded once to float32, as compose_pixels does, with tensor ops only:
    on the device it needs no host synchronisation and can be captured."""
    m = torch.stack(list(viewmat)) if isinstance(viewmat, (list, tuple)) else viewmat
    if m.dim() != 3 or m.shape[-1] != 6:
        raise ValueError("ubpl_amd: viewmat is [V,N,6], one pixel matrix per view and sample")
    m = m.to(F64)
    s = float(R) / float(H)
    out = m * s                                                 # the linear part: a cell is R/H pixels
    out[..., 2::3] = m[..., 2::3]                               # C has no offset: the translation stays
    return out.to(F32).contiguous()


# ---- cross-view pseudo-label targets (csrc/view_merge.hip)
def train_pair_matrices(viewmat, R, H):
    """The pair matrices of the training step's views for merge_views_samples.  viewmat, R, H as
    train_back_matrices takes them (view v's matrix Mv: 0-based view input pixel -> 0-based
    source-image pixel).  -> float32 [V,V,N,6] on viewmat's device: P[a][v][n] maps a 0-based
    heatmap cell of view a to the 0-based heatmap cell of view v that shows the same source pixel,

        P[a][v] = C^-1 o inv(Mv) o Ma o C,    C(c) = (R/H) c

    — train_back_matrices' cell convention, so the gate and the targets agree.  In float64, in this
    order: inv(Mv) by view_back_matrices' formula; L = inv(Mv) o Ma by compose_pixels' formula;
    the linear part of P is L's, its translation L's divided by R/H; rounded once to float32.  The
    diagonal a == v is written as exactly (1,0,0,0,1,0).  A singular Mv gives non-finite entries,
    which the kernel's sampling rule counts as outside.  Tensor ops only: on the device it needs no
    host synchronisation and can be captured."""
    m = torch.stack(list(viewmat)) if isinstance(viewmat, (list, tuple)) else viewmat
    if m.dim() != 3 or m.shape[-1] != 6:
        raise ValueError("ubpl_amd: viewmat is [V,N,6], one pixel matrix per view and sample")
    m = m.to(F64)
    V = m.shape[0]
    s = float(R) / float(H)
    det = m[..., 0] * m[..., 4] - m[..., 1] * m[..., 3]
    i0, i1, i3, i4 = m[..., 4] / det, -m[..., 1] / det, -m[..., 3] / det, m[..., 0] / det
    i2 = -(i0 * m[..., 2] + i1 * m[..., 5])
    i5 = -(i3 * m[..., 2] + i4 * m[..., 5])
    inv = torch.stack([i0, i1, i2, i3, i4, i5], -1)         # [V,N,6]
    a, b = inv.unsqueeze(0), m.unsqueeze(1)                  # a o b at [target a][source v]: inv(Mv) o Ma
    rows = []
    for r in (0, 3):
        rows += [a[..., r] * b[..., 0] + a[..., r + 1] * b[..., 3],
                 a[..., r] * b[..., 1] + a[..., r + 1] * b[..., 4],
                 (a[..., r] * b[..., 2] + a[..., r + 1] * b[..., 5] + a[..., r + 2]) / s]
    out = torch.stack(rows, -1).to(F32)                      # [V,V,N,6]
    eye = (torch.arange(6, device=out.device) % 4 == 0).to(F32)   # (1,0,0,0,1,0) without a host -> device copy
    diag = torch.eye(V, dtype=torch.bool, device=out.device).reshape(V, V, 1, 1)
    return torch.where(diag, eye, out).contiguous()


def merge_views_samples(hm, sv, sm, sb, V, M, N, K, H, W, mat, include_self=True, want_cover=False, out=None):
    """Per-sample cross-view merge (ubpl_merge_views_samples): hm is a tensor whose first element
    is view 0's, member 0's map (0, 0), with view, member and batch strides sv, sm, sb floats — a
    [V,M,N,K,H,W] buffer, or the last stacks of [.., S, K, H, W] outputs through a view at an
    element offset.  mat: device float32 [V,V,N,6] (train_pair_matrices).  include_self: a view's
    own maps count in its target ("merged") or not ("other", V >= 2).  1 <= V <= 16, 1 <= M <= 8.
    -> (out [V,M,N,K,H,W]: every view's maps as the mean of the views that cover each cell, warped
        into its frame; cover [V,N,H,W] or None: the covering views' weight per cell);
    out = (out, cover): write into these instead of allocating (cover None: not wanted)."""
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError("ubpl_amd: merge_views_samples takes 1 to %d views, got %d" % (MAX_VIEWS, V))
    if not 1 <= M <= 8:
        raise ValueError("ubpl_amd: merge_views_samples takes 1 to 8 members, got %d" % M)
    if not include_self and V < 2:
        raise ValueError("ubpl_amd: merge_views_samples without a view's own maps needs at least 2 views")
    plane = K * H * W
    _chk_maps(hm, "hm", (V, M, N), (sv, sm, sb), plane, signed=False)
    if hm is None or any(n > 1 and st < plane for n, st in ((V, sv), (M, sm), (N, sb))):
        raise ValueError("ubpl_amd: hm's strides %d, %d, %d are at least one block of %d floats"
                         % (sv, sm, sb, plane))
    _chk(mat, "mat")
    if mat is None or mat.numel() != V * V * N * 6:
        raise ValueError("ubpl_amd: mat is [V,V,N,6], one pixel matrix per view pair and sample")
    res, cover = _outs(out, hm.device, ((V, M, N, K, H, W), True), ((V, N, H, W), want_cover))
    _chk(res, "out")
    _chk(cover, "cover")
    if res is None or res.numel() != V * M * N * plane:
        raise ValueError("ubpl_amd: out holds %d floats, [V,M,N,K,H,W] needs %d"
                         % (0 if res is None else res.numel(), V * M * N * plane))
    if cover is not None and cover.numel() != V * N * H * W:
        raise ValueError("ubpl_amd: cover holds %d floats, [V,N,H,W] needs %d" % (cover.numel(), V * N * H * W))
    lo, hi = hm.data_ptr(), hm.data_ptr() + ((V - 1) * sv + (M - 1) * sm + (N - 1) * sb + plane) * 4
    for t in (res, cover):
        if t is not None and t.numel() and t.data_ptr() < hi and lo < t.data_ptr() + t.numel() * 4:
            raise ValueError("ubpl_amd: merge_views_samples writes tensors that do not overlap its input")
    call("ubpl_merge_views_samples", hm, int(sv), int(sm), int(sb), V, M, N, K, H, W, mat, int(bool(include_self)),
         res, cover)
    return res, cover


def fliplr(x, out=None):
    """ProcessUtils.image_fliplr on device planes: x [..., H, W] -> x mirrored along W
    (out: a different tensor of x's size)."""
    _chk(x, "x")
    y = torch.empty_like(x) if out is None else out
    _chk(y, "out")
    if y.numel() != x.numel() or y.data_ptr() == x.data_ptr():
        raise ValueError("ubpl_amd: fliplr writes a different tensor of the input's size")
    H, W = x.shape[-2], x.shape[-1]
    call("ubpl_fliplr", x, x.numel() // max(H * W, 1), H, W, y)
    return y


def pck(preds, gts, ref, thr):
    _chk(preds, "preds")
    _chk(gts, "gts")
    N, K, _ = preds.shape
    dev = preds.device
    errs = torch.empty(K + 1, device=dev, dtype=F32)
    accs = torch.empty(K + 1, device=dev, dtype=F32)
    hits = torch.empty(K, device=dev, dtype=torch.int32)
    valid = torch.empty(K, device=dev, dtype=torch.int32)
    call("ubpl_pck", preds, gts, N, K, int(ref[0]), int(ref[1]), float(thr), errs, accs, hits, valid)
    return errs, accs, hits, valid


# ------------------------------------------------------------------ E1
def ema_update_(ema, p, alpha):
    _chk(ema, "ema")
    _chk(p, "param")
    assert ema.numel() == p.numel()
    call("ubpl_ema_update", ema, p, ema.numel(), float(alpha))


def adamw_step_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step):
    for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, n)
    call("ubpl_adamw_step", p, g, m, v, p.numel(), float(lr), float(beta1), float(beta2), float(eps),
         float(weight_decay), int(step))



def adamw_step_dev_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step_t, coef):
    """AdamW with the step count in device memory (int64 scalar, incremented);
    replayable inside a captured HIP graph.  coef: 4-float scratch."""
    call("ubpl_adamw_step_dev", p, g, m, v, p.numel(), float(lr), float(beta1), float(beta2), float(eps),
         float(weight_decay), step_t, coef)

def adamw_ema_step_dev_(p, g, m, v, nlive, lr, beta1, beta2, eps, weight_decay, step_t, coef, ema, alpha):
    """adamw_step_dev_ on p[:nlive] and ema_update_(ema, p, alpha) over all of p, one pass."""
    if ema.numel() != p.numel() or nlive > p.numel():
        raise ValueError("adamw_ema_step_dev_: ema / p / nlive sizes disagree")
    call("ubpl_adamw_ema_step_dev", p, g, m, v, int(nlive), float(lr), float(beta1), float(beta2), float(eps),
         float(weight_decay), step_t, coef, ema, p.numel(), float(alpha))


def scale_(x, s):
    _chk(x, "x")
    call("ubpl_scale_", x, x.numel(), float(s))


def grad_guard_scratch(n, device):
    """The f64 scratch grad_guard_ needs for a gradient of n floats."""
    return torch.zeros(int(_lib.lib().ubpl_grad_guard_scratch(int(n))), dtype=torch.float64, device=device)


def grad_guard_(g, max_norm, part, guard):
    """guard[4] = {clip coefficient, L2 norm, skip, 0} of the flat gradient g (numel a
    multiple of 4, 16-B aligned): clip_grad_norm_'s coefficient for max_norm (<= 0: no
    clipping), skip = 1.0 iff some element is inf or NaN.  part: grad_guard_scratch."""
    _chk(g, "g")
    call("ubpl_grad_guard", g, g.numel(), float(max_norm), part, guard)


def adamw_step_guarded_dev_(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step_t, coef, guard, skipped):
    """adamw_step_dev_ on g * guard[0]; a no-op but for skipped[2] (int64: total,
    consecutive) when guard[2] is set."""
    call("ubpl_adamw_step_guarded_dev", p, g, m, v, p.numel(), float(lr), float(beta1), float(beta2), float(eps),
         float(weight_decay), step_t, coef, guard, skipped)


def adamw_ema_step_guarded_dev_(p, g, m, v, nlive, lr, beta1, beta2, eps, weight_decay, step_t, coef, ema, alpha,
                                guard, skipped):
    """adamw_ema_step_dev_ under a guard: on a skipped step only the EMA half runs."""
    if ema.numel() != p.numel() or nlive > p.numel():
        raise ValueError("adamw_ema_step_guarded_dev_: ema / p / nlive sizes disagree")
    call("ubpl_adamw_ema_step_guarded_dev", p, g, m, v, int(nlive), float(lr), float(beta1), float(beta2),
         float(eps), float(weight_decay), step_t, coef, ema, p.numel(), float(alpha), guard, skipped)


def restore_if_(dst, saved, guard):
    """dst = saved when guard[2] is set; otherwise nothing."""
    _chk(dst, "dst")
    _chk(saved, "saved")
    if dst.numel() != saved.numel():
        raise ValueError("restore_if_: dst and saved sizes disagree")
    call("ubpl_restore_if", dst, saved, dst.numel(), guard)


# ------------------------------------------------------------------ BN
def bn_part(B, C, device):
    """Zeroed BN scratch (partial sums + self-resetting arrival counters)."""
    return torch.zeros(int(_lib.lib().ubpl_bn_part_doubles(B, C)), dtype=torch.float64, device=device)


def bn_forward_stats(x, gamma, beta, eps, momentum, rmean, rvar, part, mean, invstd, scale, shift):
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    call("ubpl_bn_forward_stats", x, B, C, HW, gamma, beta, float(eps), float(momentum), rmean, rvar, part, mean,
         invstd, scale, shift)


def bn_eval_coeffs(gamma, beta, rmean, rvar, eps, scale, shift):
    call("ubpl_bn_eval_coeffs", gamma, beta, rmean, rvar, float(eps), gamma.numel(), scale, shift)


def bn_coeff_table(rows, n_params, n_stats, n_coef):
    """Host int64 [nbn,6] table of ubpl_bn_eval_coeffs_table from rows (gamma_off,
    beta_off, rmean_off, rvar_off, coef_off, C), every offset checked against the
    buffers' sizes (the kernel trusts the table)."""
    t = torch.tensor(rows, dtype=torch.int64).reshape(-1, 6)
    for g, b, rm, rv, co, c in t.tolist():
        if c < 1 or min(g, b, rm, rv, co) < 0 or max(g, b) + c > n_params or max(rm, rv) + c > n_stats \
                or co + 2 * c > n_coef:
            raise ValueError("ubpl_amd: BatchNorm table row %r reaches outside params[%d] / stats[%d] / coef[%d]"
                             % ((g, b, rm, rv, co, c), n_params, n_stats, n_coef))
    return t


def bn_eval_coeffs_table(params, stats, table, eps, coef):
    """scale | shift of every BatchNorm of `table` (bn_coeff_table(...).to(device)) in one launch."""
    call("ubpl_bn_eval_coeffs_table", params, stats, table, int(table.shape[0]), float(eps), coef)


def bn_apply(x, scale, shift, relu, out=None):
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    y = torch.empty_like(x) if out is None else out
    call("ubpl_bn_apply", x, B, C, HW, scale, shift, int(relu), y)
    return y


def bn_partial_buffer(C, N, device):
    return torch.empty(int(_lib.lib().ubpl_bn_partial_floats(C, N)), device=device, dtype=F32)


def bn_partials(y, part):
    B, C = y.shape[:2]
    call("ubpl_bn_partials", y, B, C, y[0, 0].numel(), part)
    return part


def bn_stats_from_partials(part, C, N, gamma, beta, eps, momentum, rmean, rvar, mean, invstd, scale, shift_out):
    call("ubpl_bn_stats_from_partials", part, C, int(N), gamma, beta, float(eps), float(momentum), rmean, rvar, mean,
         invstd, scale, shift_out)


def bn_backward_split(dz, x, gamma, mean, invstd, scale, shift, relu, scratch, coef, dgamma, dbeta, npieces, pad,
                      part=None):
    """bn_backward with dx delivered as a SplitAct (PSA planes) only.  npieces 2
    (2xfp16): the pieces of dx times the power of two its bound asks for, kept on
    the device at coef[3C] — the SplitAct's `scale`, read by its consumers (so coef
    must not be reused before they are enqueued: stream order)."""
    B, C, H, W = x.shape
    plane = B * C * (H + 2 * pad) * (W + 2 * pad)
    out = torch.empty(npieces * plane, device=x.device, dtype=torch.int16)
    call("ubpl_bn_backward_split", dz, x, B, C, H, W, gamma, mean, invstd, scale, shift, int(relu), scratch, part, coef,
         dgamma, dbeta, int(pad), int(npieces), out, int(plane))
    return SplitAct(out, plane, B, C, H, W, pad, npieces, coef[3 * C:3 * C + 1] if npieces == 2 else None)


def bn_backward(dz, x, gamma, mean, invstd, scale, shift, relu, scratch, coef, dgamma, dbeta, add1=None, add2=None,
                out=None, part=None):
    """BatchNorm(+ReLU) backward.  scratch: bn_part(B, C) (zeroed double
    scratch of the one-launch statistics); part: the backward partials dz's
    producer wrote (bn_bwd_partials layout) — then only the finalize runs."""
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    dx = dz if out is None else out
    call("ubpl_bn_backward", dz, x, B, C, HW, gamma, mean, invstd, scale, shift, int(relu), scratch, part, coef, dgamma,
         dbeta, add1, add2, dx)
    return dx


def bn_bwd_partials(dz, x, scale, shift, mean, relu):
    """Backward statistics partials (S1, S2) per (channel, 64-pixel slice)."""
    B, C = x.shape[:2]
    HW = x[0, 0].numel()
    part = bn_partial_buffer(C, B * HW, x.device)
    call("ubpl_bn_backward_partials", dz, x, B, C, HW, scale, shift, mean, int(relu), part)
    return part


# ------------------------------------------------------------------ conv
def _workspace(query, *sizes):
    """Floats of workspace the C-ABI size query `query` (a ubpl_*_workspace entry) asks for."""
    return int(getattr(_lib.lib(), query)(*sizes))


def _slab(query, device, *sizes, or_none=False):
    """The f32 workspace slab of _workspace(query, *sizes) floats (or_none: None when it asks for none)."""
    n = _workspace(query, *sizes)
    return None if or_none and n <= 0 else torch.empty(n, device=device, dtype=F32)


def conv_out_hw(H, W, KS, stride):
    pad = (KS - 1) // 2
    return (H + 2 * pad - KS) // stride + 1, (W + 2 * pad - KS) // stride + 1


def conv_weight_tapmajor(w):
    Cout, Cin, KS, _ = w.shape
    wt = torch.empty((Cout, KS * KS, Cin), device=w.device, dtype=F32)
    call("ubpl_conv_weight_tapmajor", w, Cout, Cin, KS, wt)
    return wt


def conv2d_forward(x, w, bias, stride=1, pscale=None, pshift=None, res=None, out=None, w_tap=None):
    """w: reference layout [Cout,Cin,KS,KS] (re-laid out here for KS > 1) — or
    pass w_tap, an already re-laid-out copy viewed as [Cout,KS*KS,Cin] (its
    element order is ubpl_conv_weight_tapmajor's grouped tap-major layout)."""
    B, Cin, H, W = x.shape
    if w_tap is not None:
        Cout, T, wc = w_tap.shape
        KS = int(round(T ** 0.5))
        wk = w_tap
    else:
        Cout, wc, KS, _ = w.shape
        wk = w if KS == 1 else conv_weight_tapmajor(w)
    if wc != Cin:
        raise AssertionError("{} {}".format(Cin, wc))  # models/base/layers.py:44
    Ho, Wo = conv_out_hw(H, W, KS, stride)
    y = torch.empty((B, Cout, Ho, Wo), device=x.device, dtype=F32) if out is None else out
    slab = _slab("ubpl_conv2d_forward_workspace", x.device, B, Cin, Cout, KS, Ho, Wo, or_none=True)
    call("ubpl_conv2d_forward", x, B, Cin, H, W, wk, bias, Cout, KS, stride, pscale, pshift, res, y, Ho, Wo, slab)
    return y


def conv1x1_kmajor_ok(x, cout):
    """Shapes / alignment the LDS-DMA 1x1 kernel takes (x: its B operand)."""
    return (x.shape[1] % 16 == 0 and cout % 4 == 0 and (x.shape[2] * x.shape[3]) % 4 == 0
            and x.data_ptr() % 16 == 0)


def conv1x1_forward_kmajor(x, wk, bias, pscale=None, pshift=None, res=None, out=None, stat_part=None):
    """1x1 stride-1 conv with k-major weights wk (Cin*Cout floats, [Cin][Cout]):
    y = conv(relu(x*pscale + pshift) or x) + bias (+ res; res may alias out);
    stat_part: BatchNorm partials of y (bn_partial_buffer)."""
    B, Cin, H, W = x.shape
    Cout = wk.numel() // Cin
    y = torch.empty((B, Cout, H, W), device=x.device, dtype=F32) if out is None else out
    slab = _slab("ubpl_conv1x1_kmajor_workspace", x.device, B, Cin, Cout, H * W, or_none=True)
    call("ubpl_conv1x1_forward_kmajor", x, B, Cin, H * W, wk, bias, Cout, pscale, pshift, res, y, slab, stat_part)
    return y


def conv2d_wgrad(dy, x, KS, stride, dw, db, pscale=None, pshift=None, accumulate=True):
    B, Cin, H, W = x.shape
    Cout, Ho, Wo = dy.shape[1], dy.shape[2], dy.shape[3]
    slab = _slab("ubpl_conv2d_wgrad_workspace", x.device, B, Cin, Cout, KS, Ho, Wo)
    call("ubpl_conv2d_wgrad", dy, x, B, Cin, H, W, Cout, KS, stride, pscale, pshift, Ho, Wo, slab, dw, db,
         int(accumulate))


def wgrad1x1_split_load_ok(dy, x):
    B, Cin, H, W = x.shape
    return (dy.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
            and _workspace("ubpl_wgrad1x1_split_load_workspace", B, Cin, dy.shape[1], H * W) > 0)


def conv2d_wgrad1x1_split_load(dy, x, dw, db, pscale=None, pshift=None, accumulate=True, npieces=3):
    """1x1 weight (+ bias) gradient on the split path (npieces 3: 6xbf16; 1: bf16
    operands, f32 accumulation), f32 operands split on load (v = relu(x*pscale +
    pshift) when pscale is given)."""
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    slab = _slab("ubpl_wgrad1x1_split_load_workspace", x.device, B, Cin, Cout, H * W)
    call("ubpl_wgrad1x1_split_load", dy, x, B, Cin, Cout, H * W, pscale, pshift, slab, dw, db, int(accumulate),
         int(npieces))


def conv_weight_flip(w):
    """Data-gradient weights (stride 1), viewed as [Cin, KS*KS, Cout]."""
    Cout, Cin, KS, _ = w.shape
    wt = torch.empty((Cin, KS * KS, Cout), device=w.device, dtype=F32)
    call("ubpl_conv_weight_flip", w, Cout, Cin, KS, wt)
    return wt


def conv_weights_relayout(src, dst, table, mode):
    """table: int64 [nseg,5] device tensor (src_off, dst_off, Cout, Cin, T)."""
    call("ubpl_conv_weights_relayout", src, dst, table, int(table.shape[0]), int(mode))


# Conv arithmetic: "f32" = exact-f32 MFMA (v_mfma_f32_32x32x2_f32); "6xbf16" =
# split-bf16 MFMA with 3 bf16 pieces per f32 operand (6 piece products, f32
# accumulation: exact operands); "2xfp16" = the forward convs (students' and
# teachers') with 2 fp16 pieces per operand of the power-of-two-scaled value (3
# piece products on the fp16 MFMA, operands to 2^-22: split_common.h / common.h
# split2), the backward (data and weight gradients, whose operands have no
# known range) on 6xbf16; "bf16" = one piece, i.e. both operands rounded to bf16
# (RNE) with f32 accumulation — the throughput precision of BASELINE config 5
# (8 stacks, 384x384), not parity-grade.  Value = the forward's pieces (0 for f32).
CONV_PRECISIONS = {"f32": 0, "bf16": 1, "2xfp16": 2, "6xbf16": 3}
# (round 6: 2xfp16 the default — every network-level parity test green on it, the step 17 % faster)
DEFAULT_CONV_PRECISION = "2xfp16"


def backward_pieces(pieces):
    """Pieces of the data / weight gradients' split operands for a precision's
    forward pieces (2xfp16: the backward runs on 6xbf16)."""
    return 3 if pieces == 2 else pieces


def conv_precision_name(name=None):
    return name or os.environ.get("UBPL_CONV_PRECISION", DEFAULT_CONV_PRECISION)


def conv_precision_pieces(name=None):
    """Pieces for a precision name (default: $UBPL_CONV_PRECISION or DEFAULT_CONV_PRECISION)."""
    name = conv_precision_name(name)
    if name not in CONV_PRECISIONS:
        raise ValueError("conv precision %r not in %s" % (name, sorted(CONV_PRECISIONS)))
    return CONV_PRECISIONS[name]


class SplitWeights:
    """One conv's weights as `npieces` bf16 planes (conv_weights_split.hip): a view into
    a shared buffer `buf` (int16, planes `plane` elements apart) at element
    offset `off`; shape = (rows, KS*KS, cols) of the GEMM A operand."""

    __slots__ = ("buf", "plane", "off", "shape", "npieces")

    def __init__(self, buf, plane, off, shape, npieces):
        self.buf, self.plane, self.off, self.shape, self.npieces = buf, plane, off, shape, npieces

    def ptr(self):
        """The planes' base as a tensor view at element offset `off`."""
        return self.buf[self.off:]


def conv_weights_split(src, dst, plane, table, mode, npieces):
    """Batched split re-layout (table as conv_weights_relayout, dst int16)."""
    call("ubpl_conv_weights_split", src, dst, int(plane), table, int(table.shape[0]), int(mode), int(npieces))


def conv_weight_split(w, mode, npieces):
    """Single conv: SplitWeights for the forward (mode 0) or data gradient (mode 1)."""
    Cout, Cin, KS, _ = w.shape
    n = w.numel()
    plane = (n + 7) // 8 * 8
    buf = torch.empty(npieces * plane, device=w.device, dtype=torch.int16)
    tbl = torch.tensor([[0, 0, Cout, Cin, KS * KS]], dtype=torch.int64).to(w.device)
    conv_weights_split(w.contiguous(), buf, plane, tbl, mode, npieces)
    shape = (Cout, KS * KS, Cin) if mode == 0 else (Cin, KS * KS, Cout)
    return SplitWeights(buf, plane, 0, shape, npieces)


def conv2d_forward_split(x, ws, bias, pscale=None, pshift=None, res=None, out=None):
    """Split-bf16 MFMA conv (stride 1, KS in {1, 3}, Cin % 16 == 0); ws: SplitWeights."""
    B, Cin, H, W = x.shape
    Cout, T, wc = ws.shape
    KS = int(round(T ** 0.5))
    if wc != Cin:
        raise AssertionError("{} {}".format(Cin, wc))
    Ho, Wo = conv_out_hw(H, W, KS, 1)
    y = torch.empty((B, Cout, Ho, Wo), device=x.device, dtype=F32) if out is None else out
    slab = _slab("ubpl_conv2d_forward_split_workspace", x.device, B, Cin, Cout, KS, Ho, Wo, ws.npieces, or_none=True)
    call("ubpl_conv2d_forward_split", x, B, Cin, H, W, ws.ptr(), int(ws.plane), bias, Cout, KS, 1, pscale, pshift, res,
         y, Ho, Wo, slab, int(ws.npieces))
    return y


class SplitAct:
    """Pre-split activations (conv_psa.hip PSA layout): `npieces` 16-bit planes of
    [B][C/16][H+2pad][W+2pad][16] in an int16 buffer, planes `plane` elements apart
    (3: bf16 pieces; 2: fp16 pieces of v * 32, the 2xfp16 path; 1: bf16(v))."""

    __slots__ = ("buf", "plane", "B", "C", "H", "W", "pad", "npieces", "scale")

    def __init__(self, buf, plane, B, C, H, W, pad, npieces, scale=None):
        self.buf, self.plane, self.B, self.C, self.H, self.W = buf, plane, B, C, H, W
        self.pad, self.npieces = pad, npieces
        # 2xfp16 images whose power-of-two scale lives on the device (a data gradient's: a
        # one-float tensor); None: the fixed activation scale (32) or no scale
        self.scale = scale


def split_activation(x, npieces, pad, pscale=None, pshift=None, out=None, with3=False):
    """x [B,C,H,W] f32 -> SplitAct of relu(x*pscale + pshift) (or x), zero border `pad`.
    with3 (npieces 2): (the 2xfp16 image, the 3-piece 6xbf16 image) from one read — the
    2xfp16 forward's conv input and the 6xbf16 weight gradient's operand."""
    B, C, H, W = x.shape
    plane = B * C * (H + 2 * pad) * (W + 2 * pad)
    if out is None:
        out = torch.empty(npieces * plane, device=x.device, dtype=torch.int16)
    out3 = None
    if with3:
        if npieces != 2:
            raise ValueError("with3: the 2xfp16 split only")
        out3 = torch.empty(3 * plane, device=x.device, dtype=torch.int16)
    call("ubpl_split_activation", x, B, C, H, W, pscale, pshift, int(pad), int(npieces), out, int(plane), out3,
         int(plane))
    xs = SplitAct(out, plane, B, C, H, W, pad, npieces)
    return (xs, SplitAct(out3, plane, B, C, H, W, pad, 3)) if with3 else xs


def conv2d_forward_psa(xs, ws, bias, res=None, out=None, stat_part=None, bwd=None):
    """Stride-1 conv of pre-split activations xs (SplitAct) with SplitWeights ws;
    stat_part: BatchNorm partials of the output (bn_partial_buffer); bwd =
    (x, coef, relu, part): the output is dz of a BN with input x — its backward
    statistics partials into part."""
    Cout, T, wc = ws.shape
    KS = int(round(T ** 0.5))
    if wc != xs.C or ws.npieces != xs.npieces:
        raise AssertionError("{} {} / pieces {} {}".format(xs.C, wc, xs.npieces, ws.npieces))
    B, H, W = xs.B, xs.H, xs.W
    y = torch.empty((B, Cout, H, W), device=xs.buf.device, dtype=F32) if out is None else out
    slab = _slab("ubpl_conv2d_forward_psa_workspace", xs.buf.device, B, xs.C, Cout, KS, H, W, ws.npieces, or_none=True)
    call("ubpl_conv2d_forward_psa", xs.buf, int(xs.plane), B, xs.C, H, W, int(xs.pad), ws.ptr(), int(ws.plane), bias,
         Cout, KS, res, y, slab, int(ws.npieces), stat_part, *_bnb(bwd), xs.scale)
    return y


def stem_s2d_ok(x):
    B, C, H, W = x.shape
    return C <= 4 and H % 2 == 0 and W % 2 == 0 and (B * (H // 2) * (W // 2)) % 256 == 0


def stem_s2d_split(x, pad=2, npieces=3):
    """7x7/s2 stem input as the 16-channel PSA image of its 4 phase images
    (space-to-depth; channels c*4 + 2ph + pw, the rest zero), border `pad`;
    npieces 3 (6xbf16) or 1 (bf16)."""
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    plane = B * (Ho + 2 * pad) * (Wo + 2 * pad) * 16
    buf = torch.empty(npieces * plane, device=x.device, dtype=torch.int16)
    call("ubpl_stem_s2d_split", x, B, C, H, W, int(pad), int(npieces), buf, int(plane))
    return SplitAct(buf, plane, B, 16, Ho, Wo, pad, npieces)


def stem_weight_s2d_split(w, npieces=3, out=None):
    """The stem's 7x7 weights as the split 4x4 weights of its space-to-depth conv
    (out: an earlier result of the same shape, rewritten in place)."""
    Cout, C, KS, _ = w.shape
    plane = Cout * 16 * 16
    if out is not None:
        if (out.plane, out.shape, out.npieces, out.off) != (plane, (Cout, 16, 16), npieces, 0):
            raise ValueError("ubpl_amd: stem split buffer of another shape")
        buf = out.buf
    else:
        buf = torch.empty(npieces * plane, device=w.device, dtype=torch.int16)
    call("ubpl_stem_weight_s2d_split", w.contiguous(), Cout, C, KS, int(npieces), buf, int(plane))
    return SplitWeights(buf, plane, 0, (Cout, 16, 16), npieces) if out is None else out


_NO_SOL = os.environ.get("UBPL_NO_SOL") == "1"      # diagnostic: every 1x1 on the exact-f32 kernels


# small=True (a model on the 2xfp16 precision): the split-load 1x1 also on grids below the chip's
# CU count, down to this many workgroups — the smaller planes' 1x1 convs were on the exact-f32
# kernel at 1/16 of the bf16 MFMA rate (-1 % step, profiles/r06_v8_sol_small_ab.txt); 0, and the
# other precisions: only grids that fill the chip (ubpl_conv1x1_split_load_preferred)
_SOL_MINWG = int(os.environ.get("UBPL_SOL_MINWG", "32"))


def conv1x1_split_load_ok(x, ws, small=False):
    """The split-on-load 1x1 kernel (6xbf16, 2xfp16 or bf16) takes this shape and fills the chip
    (small: on grids of >= _SOL_MINWG workgroups)."""
    B, Cin, H, W = x.shape
    ok = (not _NO_SOL and ws is not None and ws.npieces in (1, 2, 3) and ws.shape[1] == 1 and ws.shape[2] == Cin
          and x.data_ptr() % 16 == 0)
    if not ok:
        return False
    if small and _SOL_MINWG > 0 and ws.npieces in (2, 3):
        return bool(_lib.lib().ubpl_conv1x1_split_load_preferred_min(B, Cin, ws.shape[0], H * W, _SOL_MINWG))
    return bool(_lib.lib().ubpl_conv1x1_split_load_preferred(B, Cin, ws.shape[0], H * W))


def _bnb(bwd):
    """bwd = (x, coef, relu, part): backward BN partials from the epilogue (see
    ubpl_conv2d_forward_psa); coef = scale|shift|mean (3*C contiguous floats)."""
    if bwd is None:
        return None, None, 0, None
    x, coef, relu, part = bwd
    return x, coef, int(relu), part


def conv1x1_forward_split_load(x, ws, bias, pscale=None, pshift=None, res=None, out=None, stat_part=None,
                               bwd=None):
    """1x1 stride-1 conv on the split path (ws.npieces 3: 6xbf16; 2: 2xfp16; 1: bf16 operands)
    with x (NCHW f32) split while it is staged: y = conv(relu(x*pscale + pshift) or x, ws) + bias (+ res; res may
    alias out); ws = SplitWeights (rows, 1, Cin) — a forward (mode 0) or a data
    gradient (mode 1, x = dy) table; stat_part: BatchNorm partials of y."""
    B, Cin, H, W = x.shape
    Cout, T, wc = ws.shape
    if T != 1 or wc != Cin or ws.npieces not in (1, 2, 3) or (ws.npieces != 3 and (stat_part is not None or
                                                                               bwd is not None)):
        raise AssertionError("split-load 1x1: weights {} / pieces {} for {} input channels".format(
            ws.shape, ws.npieces, Cin))
    y = torch.empty((B, Cout, H, W), device=x.device, dtype=F32) if out is None else out
    call("ubpl_conv1x1_forward_split_load", x, B, Cin, H * W, ws.ptr(), int(ws.plane), bias, Cout, pscale, pshift, res,
         y, stat_part, *_bnb(bwd), int(ws.npieces))
    return y


def wgrad3_psa_ok(ys, xs):
    return (ys.npieces in (1, 2, 3) and xs.npieces == ys.npieces and (ys.npieces != 2 or ys.scale is not None) and ys.pad == 1 and xs.pad == 1 and xs.C % 64 == 0
            and ys.C % 64 == 0 and xs.W % 16 == 0 and (ys.B, ys.H, ys.W) == (xs.B, xs.H, xs.W))


def conv2d_wgrad3_psa(ys, xs, dw, db, accumulate=True):
    """3x3 weight (+ bias) gradient from PSA operands: ys = split(dy), xs = split(conv input), pad 1."""
    slab = _slab("ubpl_wgrad3_psa_workspace", xs.buf.device, xs.B, xs.C, ys.C, xs.H, xs.W)
    call("ubpl_wgrad3_psa", ys.buf, int(ys.plane), xs.buf, int(xs.plane), xs.B, xs.C, ys.C, xs.H, xs.W, slab, dw, db,
         int(accumulate), int(xs.npieces), ys.scale)


def wgrad_stem_psa_ok(ys, xs, w):
    Cout, C, KS = w.shape[0], w.shape[1], w.shape[2]
    return (ys.npieces in (1, 3) and xs.npieces == ys.npieces and ys.pad == 1 and xs.pad == 2 and xs.C == 16 and KS == 7
            and C <= 4 and Cout % 64 == 0 and ys.C == Cout and ys.W % 16 == 0
            and (ys.B, ys.H, ys.W) == (xs.B, xs.H, xs.W))


def conv2d_wgrad_stem_psa(ys, xs, dw, db, accumulate=True):
    """The 7x7/s2 stem's weight (+ bias) gradient from PSA operands: ys = split(dy) (pad 1),
    xs = the forward's space-to-depth phase image (stem_s2d_split, pad 2)."""
    Cout, C, KS = dw.shape[0], dw.shape[1], dw.shape[2]
    slab = _slab("ubpl_wgrad_stem_psa_workspace", ys.buf.device, ys.B, Cout, ys.H, ys.W)
    call("ubpl_wgrad_stem_psa", ys.buf, int(ys.plane), xs.buf, int(xs.plane), ys.B, C, Cout, ys.H, ys.W, KS, slab, dw,
         db, int(accumulate), int(ys.npieces))


def conv2d_dgrad(dy, w, res=None, out=None, wt=None):
    """dx of a stride-1 conv = conv(dy, flip(w)^T); res/out allow accumulation."""
    if wt is None:
        wt = conv_weight_flip(w)
    return conv2d_forward(dy, None, None, 1, res=res, out=out, w_tap=wt)


# ------------------------------------------------------------------ pool / upsample
def maxpool2x2(x, out=None, stat_part=None):
    """stat_part: BatchNorm partials of the output (bn_partial_buffer; needs
    (H/2)*(W/2) % 64 == 0, see stats_ok)."""
    B, C, H, W = x.shape
    y = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=F32) if out is None else out
    if stat_part is not None:
        call("ubpl_maxpool2x2_forward_stats", x, B, C, H, W, y, stat_part)
    else:
        call("ubpl_maxpool2x2_forward", x, B * C, H, W, y)
    return y


def stats_ok(H, W):
    """Elementwise producers (max-pool, upsample-add) emit BatchNorm partials for planes of 64k pixels."""
    return (H * W) % 64 == 0


def maxpool2x2_backward(x, dy, dx, accumulate):
    B, C, H, W = x.shape
    call("ubpl_maxpool2x2_backward", x, dy, B * C, H, W, dx, int(accumulate))
    return dx


def avgpool2x2(x, out=None):
    B, C, H, W = x.shape
    y = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=F32) if out is None else out
    call("ubpl_avgpool2x2_forward", x, B * C, H, W, y)
    return y


def avgpool2x2_backward(dy, dx, accumulate):
    B, C, H, W = dx.shape
    call("ubpl_avgpool2x2_backward", dy, B * C, H, W, dx, int(accumulate))
    return dx


def upsample2x_add(up, low, out=None, stat_part=None):
    """stat_part: BatchNorm partials of the output (H*W % 64 == 0)."""
    B, C, H, W = up.shape
    y = torch.empty_like(up) if out is None else out
    if stat_part is not None:
        call("ubpl_upsample2x_add_forward_stats", up, low, B, C, H, W, y, stat_part)
    else:
        call("ubpl_upsample2x_add_forward", up, low, B * C, H, W, y)
    return y


def upsample2x_add_backward(dout, dlow, accumulate):
    B, C, H, W = dout.shape
    call("ubpl_upsample2x_add_backward", dout, B * C, H, W, dlow, int(accumulate))
    return dlow


def add(a, b, out=None):
    y = torch.empty_like(a) if out is None else out
    call("ubpl_add", a, b, a.numel(), y)
    return y


# ------------------------------------------------------------------ pool / upsample folded into BatchNorm
def pool_fuse_ok(H, W, C=1, *tensors):
    """Planes the fused resampling + BatchNorm kernels take (bn.h pool_geom): H and W
    even, W/4 a power of two <= 32 (the 2x2 windows' other row sits in lane ^ (W/4) of the
    same wave), H a power of two (planes divide, or are a power-of-two multiple of, a
    256-thread block's float4s), C <= 512 (the statistics scratch's tickets) and every
    tensor given 16-byte aligned."""
    if H < 2 or W < 4 or H & (H - 1) or W & 3:
        return False
    w4 = W >> 2
    if w4 & (w4 - 1) or w4 > 32 or not 1 <= C <= 512:
        return False
    return all(t is None or t.data_ptr() % 16 == 0 for t in tensors)


def _same_shape(name, t, shape):
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("ubpl_amd: %s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))


def _fuse_geometry(name, x):
    if x.dim() != 4:
        raise ValueError("ubpl_amd: %s takes a [B,C,H,W] tensor, got shape %s" % (name, tuple(x.shape)))
    B, C, H, W = x.shape
    if B < 1 or not pool_fuse_ok(H, W, C):
        raise ValueError("ubpl_amd: %s does not take planes of %dx%d with %d channels (pool_fuse_ok)" % (name, H, W, C))
    return B, C, H, W


def bn_forward_stats_maxpool(x, xbn, pbn, eps, momentum, part, out=None):
    """One launch: bn_forward_stats(x) for the BatchNorm xbn (None: x has none),
    y = maxpool2x2(x), and the statistics of y for the BatchNorm pbn (None: not taken; a new
    summation order, unlike everything else here).  xbn / pbn:
    (gamma, beta, rmean, rvar, mean, invstd, scale, shift), rmean / rvar nullable."""
    B, C, H, W = _fuse_geometry("bn_forward_stats_maxpool", x)
    for nm, bn in (("xbn", xbn), ("pbn", pbn)):
        if bn is None:
            continue
        if len(bn) != 8:
            raise ValueError("ubpl_amd: %s is (gamma, beta, rmean, rvar, mean, invstd, scale, shift)" % nm)
        for i, t in enumerate(bn):
            _same_shape("%s[%d]" % (nm, i), t, (C,))
    _same_shape("out", out, (B, C, H // 2, W // 2))
    _chk(x, "x")
    y = torch.empty((B, C, H // 2, W // 2), device=x.device, dtype=F32) if out is None else out
    call("ubpl_bn_forward_stats_maxpool", x, B, C, H, W, y, *(xbn if xbn is not None else (None,) * 8),
         *(pbn if pbn is not None else (None,) * 8),
         float(eps), float(momentum), part)
    return y


def upsample2x_add_bnstats(up, low, bn, eps, momentum, part, out=None):
    """One launch: out = upsample2x_add(up, low) (out=up: in place) and bn_forward_stats(out)
    for the BatchNorm bn = (gamma, beta, rmean, rvar, mean, invstd, scale, shift)."""
    B, C, H, W = _fuse_geometry("upsample2x_add_bnstats", up)
    _same_shape("low", low, (B, C, H // 2, W // 2))
    _same_shape("out", out, up.shape)
    if bn is None or len(bn) != 8:
        raise ValueError("ubpl_amd: bn is (gamma, beta, rmean, rvar, mean, invstd, scale, shift)")
    for i, t in enumerate(bn):
        _same_shape("bn[%d]" % i, t, (C,))
    _chk(up, "up")
    _chk(low, "low")
    y = torch.empty_like(up) if out is None else out
    gamma, beta, rmean, rvar, mean, invstd, scale, shift = bn
    call("ubpl_upsample2x_add_forward_bnstats", up, low, B, C, H, W, y, gamma, beta, float(eps), float(momentum),
         rmean, rvar, part, mean, invstd, scale, shift)
    return y


def bn_backward_pool(dz, x, gamma, mean, invstd, scale, shift, relu, scratch, coef, dgamma, dbeta, add1=None,
                     pool_dy=None, add2=None, out=None, part=None):
    """bn_backward with the gradient of maxpool2x2(x) folded into the apply:
    dx = ((dL/dx + add1) + maxpool2x2_backward(x, pool_dy)) + add2, bit-identical to
    bn_backward(add1), maxpool2x2_backward(accumulate=True) and add in turn."""
    if pool_dy is None:
        return bn_backward(dz, x, gamma, mean, invstd, scale, shift, relu, scratch, coef, dgamma, dbeta, add1=add1,
                           add2=add2, out=out, part=part)
    B, C, H, W = _fuse_geometry("bn_backward_pool", x)
    for nm, t in (("dz", dz), ("add1", add1), ("add2", add2), ("out", out)):
        _same_shape(nm, t, x.shape)
    _same_shape("pool_dy", pool_dy, (B, C, H // 2, W // 2))
    _chk(x, "x")
    _chk(dz, "dz")
    _chk(pool_dy, "pool_dy")
    dx = dz if out is None else out
    call("ubpl_bn_backward_pool", dz, x, B, C, H, W, gamma, mean, invstd, scale, shift, int(relu), scratch, part, coef,
         dgamma, dbeta, add1, pool_dy, add2, dx)
    return dx


# ------------------------------------------------------------------ f1
def image_mean_u8(imgs):
    """imgs uint8 [N,H,W,3] -> per-image mean / 255 (noisy_mean's mu), float32 [N]."""
    _chk(imgs, "imgs", torch.uint8)
    out = torch.empty(imgs.shape[0], device=imgs.device, dtype=F32)
    call("ubpl_image_mean_u8", imgs, imgs.shape[0], imgs[0].numel(), out)
    return out


def augment_warp(imgs, src_idx, mat, noise, img_mean, chan_mean, out):
    """One launch for V augmented views (see augment.hip): out [V,3,Ho,Wo]."""
    _chk(imgs, "imgs", torch.uint8)
    _chk(src_idx, "src_idx", torch.int32)
    for t, n in ((mat, "mat"), (noise, "noise"), (img_mean, "img_mean"), (chan_mean, "chan_mean"), (out, "out")):
        _chk(t, n)
    V, _, Ho, Wo = out.shape
    if mat.numel() != 6 * V or noise.numel() != 3 * V or src_idx.numel() != V:
        raise ValueError("augment_warp: per-view tables do not match %d views" % V)
    call("ubpl_augment_warp", imgs, imgs.shape[1], imgs.shape[2], src_idx, mat, noise, img_mean, chan_mean, V, Ho, Wo,
         out)
    return out


def augment_chain(imgs, geo, cs, noise, img_mean, chan_mean, Hm, Wm, out):
    """The reference's two resamplings per view (see augment.hip
    ubpl_augment_chain): geo int32 [V,8] (src, flip, ul_x, ul_y, Hp, Wp, Hc, Wc),
    cs float32 [V,2] (cos, sin); out [V,3,Ho,Wo].  Stage-1 scratch [V,3,Hm,Wm]."""
    _chk(imgs, "imgs", torch.uint8)
    _chk(geo, "geo", torch.int32)
    for t, n in ((cs, "cs"), (noise, "noise"), (img_mean, "img_mean"), (chan_mean, "chan_mean"), (out, "out")):
        _chk(t, n)
    V, _, Ho, Wo = out.shape
    if geo.numel() != 8 * V or cs.numel() != 2 * V or noise.numel() != 3 * V:
        raise ValueError("augment_chain: per-view tables do not match %d views" % V)
    g = geo.reshape(V, 8).cpu() if geo.is_cuda else geo.reshape(V, 8)
    if (g[:, 6] > Hm).any() or (g[:, 7] > Wm).any() or (g[:, 6] < 1).any() or (g[:, 7] < 1).any() or \
            (g[:, 0] < 0).any() or (g[:, 0] >= imgs.shape[0]).any():
        raise ValueError("augment_chain: a view's stripped crop exceeds %dx%d or its source index is out of range"
                         % (Hm, Wm))
    # skimage.transform.resize anti-aliases a downscale with a Gaussian of sigma = (s - 1) / 2
    # (s = crop / output); the device resize omits it, which is exact to f32 only while its
    # off-centre weight exp(-1 / (2 sigma^2)) stays below f32 rounding: s <= 1.3 (2e-10 there;
    # the loaders' defaults draw s <= 1.25).  A larger crop would silently leave the reference.
    s = max(float((g[:, 6].double() / Ho).max()), float((g[:, 7].double() / Wo).max()))
    if s > 1.3:
        raise ValueError("augment_chain: a crop %.3fx the output size needs skimage's anti-aliasing blur "
                         "(sigma %.3f px), which the device resize does not run; crops up to 1.3x are exact"
                         % (s, (s - 1) / 2))
    inter = torch.empty((V, 3, Hm, Wm), device=out.device, dtype=F32)
    call("ubpl_augment_chain", imgs, imgs.shape[1], imgs.shape[2], geo, cs, noise, img_mean, chan_mean, V, int(Hm),
         int(Wm), inter, Ho, Wo, out)
    return out


def _occlude_check(V, H, W, nbank, off, hw, pastes, view_first):
    """Every index occlude_kernel derives from a paste row stays inside its
    buffer (host copies of the small tables; occlusion is opt-in)."""
    if not pastes.numel():
        return
    noff = off.numel()
    pr = pastes.reshape(-1, 9).cpu().numpy().astype("int64")
    vf = view_first.cpu().numpy().astype("int64")
    hwh = hw.reshape(-1, 2).cpu().numpy().astype("int64")
    if vf[0] != 0 or (vf[1:] < vf[:-1]).any() or vf[-1] != len(pr):
        raise ValueError("occlude: view_first is not a running count of %d paste rows" % len(pr))
    v, oc, w1, h1, x0, y0, x1, y1 = (pr[:, i] for i in range(8))
    sx0, sy0 = pr[:, 8] & 0xFFFF, pr[:, 8] >> 16
    bad = ((v < 0) | (v >= V) | (oc < 0) | (oc >= min(noff, len(hwh))) | (w1 <= 0) | (h1 <= 0)
           | (x0 < 0) | (y0 < 0) | (x1 > W) | (y1 > H) | (x1 < x0) | (y1 < y0)
           | (sx0 + (x1 - x0) > w1) | (sy0 + (y1 - y0) > h1))
    if bad.any():
        raise ValueError("occlude: paste row %d is out of range for %dx%d views / %d occluders" % (
            int(bad.nonzero()[0][0]), H, W, noff))
    h, w = hwh[oc, 0], hwh[oc, 1]
    if (h <= 0).any() or (w <= 0).any():
        raise ValueError("occlude: an occluder of the bank has an empty size")
    offh = off.cpu().numpy().astype("int64")[oc]
    if (offh < 0).any() or (offh + h * w * 4 > nbank).any():
        raise ValueError("occlude: an occluder reaches past the end of the bank")


def occlude(out, bank, off, hw, pastes, view_first, chan_mean):
    """Random occlusion pastes onto augmented views in place (see augment.hip
    occlude_kernel): out [V,3,H,W]; bank / off / hw: the occluder bank;
    pastes int32 [P,9] sorted by view; view_first int32 [V+1]."""
    _chk(out, "out")
    _chk(bank, "bank")
    _chk(off, "off", torch.int64)
    _chk(hw, "hw", torch.int32)
    _chk(pastes, "pastes", torch.int32)
    _chk(view_first, "view_first", torch.int32)
    _chk(chan_mean, "chan_mean")
    V, _, H, W = out.shape
    if view_first.numel() != V + 1 or (pastes.numel() and pastes.shape[-1] != 9):
        raise ValueError("occlude: paste table does not match %d views" % V)
    _occlude_check(V, H, W, bank.numel(), off, hw, pastes, view_first)
    call("ubpl_occlude", out, V, H, W, bank, off, hw, pastes, view_first, chan_mean)
    return out
