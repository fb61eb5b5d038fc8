"""Multi-view kernels: the view warp and multi-view decode (csrc/decode_warp.hip), the
view-consistency uncertainty (csrc/uncertainty.hip) and the per-sample cross-view merge
(csrc/view_merge.hip).  Their matrices come from view_geometry; the convention: DESIGN.md §4."""
from .. import _lib
from . import _check
from ._check import _chk_entries, _chk_maps, _members, _no_overlap, _one_float, _outs, _views


def warp_views(src, mat, out=None):
    """Views of a batch (ubpl_warp_views): src [N,C,H,W], mat device float32 [V,6] pixel matrices
    (output pixel -> source pixel) -> out [V,N,C,H,W] (or any contiguous tensor of that many
    floats, e.g. rows of a [V*N,C,H,W] batch), bilinear, zero outside; an identity view copies."""
    _check._chk(src, "src")
    _check._chk(mat, "mat")
    if src.dim() != 4 or mat.dim() != 2 or mat.shape[1] != 6:
        raise ValueError("ubpl_amd: warp_views takes src [N,C,H,W] and mat [V,6]")
    N, C, H, W = src.shape
    V = mat.shape[0]
    out, = _outs(None if out is None else (out,), src.device, ((V, N, C, H, W), True))
    _check._chk(out, "out")
    if out.numel() != V * src.numel():
        raise ValueError("ubpl_amd: out holds %d floats, %d views of %d need %d"
                         % (out.numel(), V, src.numel(), V * src.numel()))
    _no_overlap("warp_views", src.data_ptr(), src.data_ptr() + src.numel() * 4, out)
    _lib.call("ubpl_warp_views", src, N, C, H, W, mat, V, out)
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
    _views("decode_heatmaps_views", V, 1)
    _chk_maps(hm, "hm", (V, N), (sv, sb), K * H * W, signed=False)
    _check._chk(mat, "mat")
    if mat is None or mat.numel() != V * 6:
        raise ValueError("ubpl_amd: mat is [V,6], one pixel matrix per view")
    _chk_entries(perm, K, tinv, swap, V)
    raw, preds, scores, merged = _outs(out, hm.device, ((N, K, 2), True), ((N, K, 2), tinv is not None),
                                       ((N, K), True), ((N, K, H, W), want_merged))
    _lib.call("ubpl_decode_heatmaps_views", hm, int(sv), int(sb), V, N, K, H, W, mat, swap, perm, tinv, merged, raw,
              preds, scores)
    return raw, preds, scores, merged


UNC_OUTPUTS = ("pts", "legal", "int_dist", "aug_coord", "ext_dist", "aext_dist", "ext_views", "mix_dist", "unc",
               "select")


def _unc_outs(name, raw, bad, layout, need, M, V, N, K, back, dist_thr, out, per_sample, swap=None, perm=None,
              tinv=None):
    """What view_uncertainty and view_uncertainty_samples share: the M / V ranges, raw against its
    layout (bad: the caller's stride test; layout, need: the message's), back ([V,6], per_sample:
    [V,N,6]), dist_thr, the entry tables and the outputs — UNC_OUTPUTS' order, per_sample: then gate."""
    _members(name, M)
    _views(name, V, 2)
    _check._chk(raw, "raw")
    if raw is None or bad or raw.numel() < need:
        raise ValueError("ubpl_amd: raw holds %d floats, %s need %d"
                         % (0 if raw is None else raw.numel(), layout[0] % layout[1:], need))
    _check._chk(back, "back")
    _check._chk(dist_thr, "dist_thr")
    if back is None or back.numel() != V * (N if per_sample else 1) * 6:
        raise ValueError("ubpl_amd: back is [V,N,6], one pixel matrix per view and sample" if per_sample else
                         "ubpl_amd: back is [V,6], one pixel matrix per view")
    _one_float(dist_thr, "dist_thr")
    _chk_entries(perm, K, tinv, swap, V, N)
    mnk, nk = (M, N, K), (N, K)
    shapes = ((M, V, N, K, 2), mnk, mnk, (M, N, K, 2), nk, nk, nk, mnk, mnk, mnk) + ((nk,) if per_sample else ())
    outs = _outs(out, raw.device, *((shape, True) for shape in shapes))
    if len(outs) != len(shapes):
        raise ValueError("ubpl_amd: %s writes %d outputs, got %d" % (name, len(shapes), len(outs)))
    if outs[len(UNC_OUTPUTS) - 1] is None:
        raise ValueError("ubpl_amd: %s always writes select" % name)
    return outs


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
    blk = V * N * K * 2
    outs = _unc_outs("view_uncertainty", raw, sm < 0 or (M > 1 and sm < blk),
                     ("%d members of stride %d with %d x %d x %d points", M, sm, V, N, K), (M - 1) * sm + blk,
                     M, V, N, K, back, dist_thr, out, False, swap, perm, tinv)
    _lib.call("ubpl_view_uncertainty", raw, int(sm), M, V, N, K, back, swap, perm, tinv, dist_thr, *outs)
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
    blk = N * K * 2
    nested = M == 1 or sm >= (V - 1) * sv + blk or sv >= (M - 1) * sm + blk
    outs = _unc_outs("view_uncertainty_samples", raw, sm < 0 or sv < blk or (M > 1 and sm < blk) or not nested,
                     ("%d members of stride %d and %d views of stride %d with %d x %d points", M, sm, V, sv, N, K),
                     (M - 1) * sm + (V - 1) * sv + blk, M, V, N, K, back, dist_thr, out, True)
    _lib.call("ubpl_view_uncertainty_samples", raw, int(sm), int(sv), M, V, N, K, back, dist_thr, *outs)
    return outs


def merge_views_samples(hm, sv, sm, sb, V, M, N, K, H, W, mat, include_self=True, want_cover=False, out=None):
    """Per-sample cross-view merge (ubpl_merge_views_samples): hm is a tensor whose first element
    is view 0's, member 0's map (0, 0), with view, member and batch strides sv, sm, sb floats — a
    [V,M,N,K,H,W] buffer, or the last stacks of [.., S, K, H, W] outputs through a view at an
    element offset.  mat: device float32 [V,V,N,6] (train_pair_matrices).  include_self: a view's
    own maps count in its target ("merged") or not ("other", V >= 2).  1 <= V <= 16, 1 <= M <= 8.
    -> (out [V,M,N,K,H,W]: every view's maps as the mean of the views that cover each cell, warped
        into its frame; cover [V,N,H,W] or None: the covering views' weight per cell);
    out = (out, cover): write into these instead of allocating (cover None: not wanted)."""
    _views("merge_views_samples", V, 1)
    _members("merge_views_samples", M)
    if not include_self and V < 2:
        raise ValueError("ubpl_amd: merge_views_samples without a view's own maps needs at least 2 views")
    plane = K * H * W
    _chk_maps(hm, "hm", (V, M, N), (sv, sm, sb), plane, signed=False)
    if hm is None or any(n > 1 and st < plane for n, st in ((V, sv), (M, sm), (N, sb))):
        raise ValueError("ubpl_amd: hm's strides %d, %d, %d are at least one block of %d floats"
                         % (sv, sm, sb, plane))
    _check._chk(mat, "mat")
    if mat is None or mat.numel() != V * V * N * 6:
        raise ValueError("ubpl_amd: mat is [V,V,N,6], one pixel matrix per view pair and sample")
    res, cover = _outs(out, hm.device, ((V, M, N, K, H, W), True), ((V, N, H, W), want_cover))
    _check._chk(res, "out")
    _check._chk(cover, "cover")
    if res is None or res.numel() != V * M * N * plane:
        raise ValueError("ubpl_amd: out holds %d floats, [V,M,N,K,H,W] needs %d"
                         % (0 if res is None else res.numel(), V * M * N * plane))
    if cover is not None and cover.numel() != V * N * H * W:
        raise ValueError("ubpl_amd: cover holds %d floats, [V,N,H,W] needs %d" % (cover.numel(), V * N * H * W))
    _no_overlap("merge_views_samples", hm.data_ptr(),
                hm.data_ptr() + ((V - 1) * sv + (M - 1) * sm + (N - 1) * sb + plane) * 4, res, cover)
    _lib.call("ubpl_merge_views_samples", hm, int(sv), int(sm), int(sb), V, M, N, K, H, W, mat,
              int(bool(include_self)), res, cover)
    return res, cover
