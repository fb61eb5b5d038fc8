"""Heatmap decode (D1-D4): argmax, flip-test decode, the ensemble pseudo-labels, sub-pixel
refinement, the plane mirror and PCK — and the two small host tables they take."""
import math

import torch

from .. import _lib
from . import _check
from ._check import F32, _chk_entries, _chk_maps, _members, _one_float, _outs


def decode_heatmaps(hm, tinv=None):
    """hm [N,K,H,W] -> (raw [N,K,2], preds [N,K,2] or None, scores [N,K])."""
    _check._chk(hm, "heatmap")
    N, K, H, W = hm.shape
    dev = hm.device
    raw = torch.empty((N, K, 2), device=dev, dtype=F32)
    preds = torch.empty((N, K, 2), device=dev, dtype=F32) if tinv is not None else None
    scores = torch.empty((N, K), device=dev, dtype=F32)
    if tinv is not None:
        _check._chk(tinv, "tinv", torch.float64)
    _lib.call("ubpl_decode_heatmaps", hm, N, K, H, W, tinv, raw, preds, scores)
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
    _lib.call("ubpl_decode_heatmaps_flip", hm, hm_flip, int(sb), N, K, H, W, perm, tinv, merged, raw, preds, scores)
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
    _members("ensemble_pseudo", M)
    _chk_maps(hm, "hm", (M, N), (sm, sb), K * H * W)
    _check._chk(thr, "thr")
    _check._chk(tinv, "tinv", torch.float64)
    _one_float(thr, "thr")
    ens_raw, ens_preds, ens_score, member_score, disagree, select, mean_hm = _outs(
        out, hm.device, ((N, K, 2), True), ((N, K, 2), tinv is not None), ((N, K), True), ((M, N, K), True),
        ((M, N, K), True), ((M, N, K), True), ((N, K, H, W), want_mean))
    if select is None:
        raise ValueError("ubpl_amd: ensemble_pseudo always writes select")
    _lib.call("ubpl_ensemble_pseudo", hm, int(sm), int(sb), M, N, K, H, W, tinv, thr, mean_hm, ens_raw, ens_preds,
              ens_score, member_score, disagree, select)
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
    _check._chk(raw, "raw")
    _check._chk(taps, "taps")
    _chk_entries(perm, K, tinv)
    if raw is None or raw.numel() != N * K * 2:
        raise ValueError("ubpl_amd: raw is the decode's [N,K,2] peaks")
    if taps is None or not 1 <= taps.numel() <= MAX_BLUR_RADIUS + 1:
        raise ValueError("ubpl_amd: taps holds 1 to %d floats (blur_taps)" % (MAX_BLUR_RADIUS + 1))
    raw_sub, preds_sub, how = _outs(out, hm.device, ((N, K, 2), True), ((N, K, 2), tinv is not None), ((N, K), True))
    _lib.call("ubpl_refine_peaks", hm, hm_flip, int(sb), N, K, H, W, perm, raw, mode, taps, taps.numel() - 1, tinv,
              raw_sub, preds_sub, how)
    return raw_sub, preds_sub, how


def fliplr(x, out=None):
    """ProcessUtils.image_fliplr on device planes: x [..., H, W] -> x mirrored along W
    (out: a different tensor of x's size)."""
    _check._chk(x, "x")
    y = torch.empty_like(x) if out is None else out
    _check._chk(y, "out")
    if y.numel() != x.numel() or y.data_ptr() == x.data_ptr():
        raise ValueError("ubpl_amd: fliplr writes a different tensor of the input's size")
    H, W = x.shape[-2], x.shape[-1]
    _lib.call("ubpl_fliplr", x, x.numel() // max(H * W, 1), H, W, y)
    return y


def pck(preds, gts, ref, thr):
    _check._chk(preds, "preds")
    _check._chk(gts, "gts")
    N, K, _ = preds.shape
    dev = preds.device
    errs = torch.empty(K + 1, device=dev, dtype=F32)
    accs = torch.empty(K + 1, device=dev, dtype=F32)
    hits = torch.empty(K, device=dev, dtype=torch.int32)
    valid = torch.empty(K, device=dev, dtype=torch.int32)
    _lib.call("ubpl_pck", preds, gts, N, K, int(ref[0]), int(ref[1]), float(thr), errs, accs, hits, valid)
    return errs, accs, hits, valid
