"""Inference with trained networks: images -> keypoints.

`Predictor` is what a user of a trained teacher runs.  It follows the
reference's validation (projects/MT_UBPL.py:355-408: per-network argmax decode
+ inverse transform, and the coordinate mean of the networks, :387) and adds
the stacked-hourglass flip test the reference carries the pieces of without
wiring them in (utils/augment.py:239-252 fliplr_back / fliplr_back_tensor,
utils/udaap/transforms.py:20-57 flip_back).

Three things make it cheap at small batches:

* frozen weights — a private snapshot per network (StackedHourglass.freeze):
  the split / re-laid-out conv weights, the stem's space-to-depth weights and
  the eval coefficients of every BatchNorm (one ubpl_bn_eval_coeffs_table
  launch) are made by refresh() and only read by predict();
* the flip test in two kernels — ubpl_fliplr writes the mirrored half of one
  [2N] batch, ubpl_decode_heatmaps_flip flips back, swaps the pairs, averages
  and decodes the last stack of the network's output in place;
* graph replay — per batch size, the frozen forwards, the flip, the decode and
  the mean are captured in one HIP graph on ONE stream (several networks run
  one after another: no fork inside the capture) and replayed.

`Predictor.pseudo_label` asks the method's own question of unlabeled images:
which joints do the networks agree on confidently enough to use as labels
(JointPseudoLoss3's target and mask, utils/losses.py:176-210)?  It is the
same replay with one more launch, ubpl_ensemble_pseudo, over the networks'
merged heatmaps; `label_pool` runs it over a loader.

`Predictor(refine="quarter" | "taylor")` adds sub-pixel coordinates beside the integer
ones: after each network's decode one ubpl_refine_peaks launch on the same heatmap views
(the quarter-offset step the reference carries commented out, utils/udaap/evaluation.py:
218-228, or the distribution-aware Taylor step), inside the same graph.  The default
"none" launches and returns exactly what it did without the option.

`Predictor(tta=[(angle_deg, zoom), ...])` is multi-view test-time augmentation: the reference
computes a warp matrix per augmented view and can warp heatmaps back (utils/augment.py:158-164
affine_getWarpmat, :36-47 affine_back2) but only draws with it (projects/MT_UBPL.py:186-205).
Here ubpl_warp_views fills one view-major batch, each network runs once on it, and
ubpl_decode_heatmaps_views warps the views' last stacks back, averages them over the views that
cover each pixel and decodes the merged maps, which refine and pseudo_label then read (the
convention: DESIGN.md §4 "Multi-view decode").  The default None launches and returns exactly
what it did without the option.

`Predictor(uncertainty=True)` (with tta) keeps what the merge throws away: every network's peak
on every view (the strided plain decode of the same view-major output, refined when refine is
on), and one ubpl_view_uncertainty launch inside the same graph folds them into the reference's
geometric uncertainty (utils/business.py pseudo_cal_unc / assess_pseudo_unc2: how far one
network's views lie apart, how far the networks lie from one another, unc = 1 - exp(-mixDist/5));
`pseudo_label(rule="uncertainty", dist_thr=...)` selects on it (DESIGN.md §4 "View-consistency
uncertainty").  The default False launches and returns exactly what it did without the option.

There is no CPU fallback.
"""
import math
import os
from collections import OrderedDict

import torch

from . import _lib
from . import kernels as Kn


class _Slot:
    """Static buffers of one (batch size, resolution, heatmaps wanted) and, once
    captured, the graph that maps its inputs to its outputs."""

    def __init__(self, M, N, K, R, flip, want_hm, dev, refine=False, views=None, unc=None):
        H = W = R // 4
        f32 = dict(device=dev, dtype=torch.float32)
        self.N, self.H, self.W = N, H, W
        # (views: the view count of Predictor(tta=...), mirrored ones included; view-major rows)
        self.batch = torch.zeros(((2 * N if flip else N) if views is None else views * N, 3, R, R), **f32)
        self.imgs = self.batch[:N]
        self.tinv = torch.zeros((N, 6), device=dev, dtype=torch.float64)
        self.raw = torch.zeros((M, N, K, 2), **f32)
        self.preds = torch.zeros((M, N, K, 2), **f32)
        self.scores = torch.zeros((M, N, K), **f32)
        self.mean = torch.zeros((N, K, 2), **f32)
        self.heatmaps = torch.zeros((M, N, K, H, W), **f32) if want_hm else None
        self.refine = refine
        if refine:                                  # the sub-pixel decode's outputs (Predictor(refine=...))
            self.raw_sub = torch.zeros((M, N, K, 2), **f32)
            self.preds_sub = torch.zeros((M, N, K, 2), **f32)
            self.rule = torch.zeros((M, N, K), **f32)
            self.mean_sub = torch.zeros((N, K, 2), **f32)
        self.unc = unc is not None
        if self.unc:                                # the per-view peaks and their fold (Predictor(uncertainty=True))
            V = views
            self.have_tinv = bool(unc)              # (the kernel's tinv is null or not: part of the slot's key)
            self.raw_views = torch.zeros((M, V * N, K, 2), **f32)
            self.scores_views = torch.zeros((M, V * N, K), **f32)
            if refine:
                self.raw_views_sub = torch.zeros((M, V * N, K, 2), **f32)
            self.dist_thr = torch.zeros(1, **f32)
            self.view_preds = torch.zeros((M, V, N, K, 2), **f32)
            self.aug_coord = torch.zeros((M, N, K, 2), **f32)
            for name in ("view_legal", "int_dist", "mix_dist", "unc_value", "unc_select"):
                setattr(self, name, torch.zeros((M, N, K), **f32))
            for name in ("ext_dist", "aext_dist", "ext_views"):
                setattr(self, name, torch.zeros((N, K), **f32))
        self.graph = None

    def release(self):
        if self.graph is not None:
            self.graph.reset()
            self.graph = None


class _PseudoSlot(_Slot):
    """A slot of pseudo_label: predict's buffers with the merged heatmaps always kept
    (the ensemble kernel reads them in place), the ensemble outputs and the threshold.
    One slot serves calls with and without return_heatmaps."""

    def __init__(self, M, N, K, R, flip, dev, refine=False, views=None, unc=None):
        super().__init__(M, N, K, R, flip, True, dev, refine, views, unc)
        f32 = dict(device=dev, dtype=torch.float32)
        self.thr = torch.zeros(1, **f32)
        self.ens_raw = torch.zeros((N, K, 2), **f32)
        self.ens_preds = torch.zeros((N, K, 2), **f32)
        self.ens_score = torch.zeros((N, K), **f32)
        self.disagree = torch.zeros((M, N, K), **f32)
        self.select = torch.zeros((M, N, K), **f32)
        self.spread = torch.zeros((N, K), **f32)
        self.mean_hm = torch.zeros((N, K, self.H, self.W), **f32)
        if refine:
            self.ens_raw_sub = torch.zeros((N, K, 2), **f32)
            self.ens_preds_sub = torch.zeros((N, K, 2), **f32)
            self.ens_rule = torch.zeros((N, K), **f32)


DEFAULT_BLUR_SIGMA = 1.0
RULES = ("unanimous", "ensemble", "uncertainty")
REFINES = ("none", "quarter", "taylor")


def check_rule(rule):
    if rule not in RULES:
        raise ValueError("ubpl_amd: rule is one of %s, got %r" % (", ".join(RULES), rule))
    return rule


def check_refine(refine, blur_sigma):
    """The refine / blur_sigma arguments -> (refine, the host taps table or None for "none").
    The blur belongs to "taylor"; "quarter" reads unblurred values."""
    if refine not in REFINES:
        raise ValueError("ubpl_amd: refine is one of %s, got %r" % (", ".join(REFINES), refine))
    if refine == "none":
        return refine, None
    return refine, Kn.blur_taps(blur_sigma if refine == "taylor" else 0.0)


def check_tta(tta, flip_test):
    """The tta / flip_test arguments -> None, or the views as a list of (angle_deg, zoom) floats.
    The first view is the image itself; with the flip test every view is run mirrored as well."""
    if tta is None:
        return None
    try:
        views = [(float(a), float(z)) for a, z in tta]
    except (TypeError, ValueError):
        raise ValueError("ubpl_amd: tta is a list of (angle_deg, zoom) pairs, got %r" % (tta,))
    if not views or views[0] != (0.0, 1.0):
        raise ValueError("ubpl_amd: the first tta view is the image itself, (0, 1)")
    for a, z in views:
        if not (math.isfinite(a) and math.isfinite(z)):
            raise ValueError("ubpl_amd: a tta view is a finite (angle_deg, zoom), got (%r, %r)" % (a, z))
        if not 0.5 <= z <= 2.0:
            raise ValueError("ubpl_amd: a tta zoom lies in [0.5, 2], got %r" % z)
    V = len(views) * (2 if flip_test else 1)
    if V > Kn.MAX_VIEWS:
        raise ValueError("ubpl_amd: %d tta views%s make %d, at most %d"
                         % (len(views), " with their mirrors" if flip_test else "", V, Kn.MAX_VIEWS))
    return views


def check_uncertainty(uncertainty, views, flip_test):
    """The uncertainty argument against the checked tta views -> bool.  View consistency needs
    views to compare: tta with at least 2 in all (mirrored ones included)."""
    if not uncertainty:
        return False
    V = 0 if views is None else len(views) * (2 if flip_test else 1)
    if V < 2:
        raise ValueError("ubpl_amd: uncertainty=True compares the views of tta: at least 2 in all, got %s"
                         % ("tta=None" if views is None else "%d" % V))
    return True


def check_dist_thr(rule, dist_thr, uncertainty):
    """pseudo_label's rule / dist_thr against Predictor(uncertainty=...) -> dist_thr as a float, or
    None.  The rule "uncertainty" needs both; the reference ships no default threshold
    (args.distThrMax), and none is invented here."""
    if rule == "uncertainty" and not uncertainty:
        raise ValueError('ubpl_amd: rule "uncertainty" needs Predictor(uncertainty=True)')
    if dist_thr is None:
        if rule == "uncertainty":
            raise ValueError('ubpl_amd: rule "uncertainty" needs dist_thr, a distance in the coordinates of the result')
        return None
    if not uncertainty:
        raise ValueError("ubpl_amd: dist_thr needs Predictor(uncertainty=True)")
    dist_thr = float(dist_thr)
    if not dist_thr >= 0:
        raise ValueError("ubpl_amd: dist_thr is a distance >= 0, got %r" % dist_thr)
    return dist_thr


def assemble_kps(ens_preds, selected):
    """[N,K,2] image coordinates + [N,K] bool -> [N,K,3] (x, y, selected as 0/1), the
    meta["kpsMap"] layout."""
    return torch.cat([ens_preds, selected.to(ens_preds.dtype).unsqueeze(-1)], -1)


class Predictor:
    """Predictor(models, flip_test=False, flip_pairs=None, max_batch=32, max_graphs=4, graph=None,
              refine="none", blur_sigma=DEFAULT_BLUR_SIGMA, tta=None, uncertainty=False)

    models      one StackedHourglass or a list (the teachers), same k, one device;
    flip_test   average each heatmap with the flipped-back heatmap of the mirrored image;
    flip_pairs  [(left, right), ...] joints swapped when flipping back (the caller's
                dataset convention; None = none, the reference's kps_fliplr convention,
                utils/process.py:239-242);
    max_batch   larger inputs run in chunks of this size;
    max_graphs  captured graphs kept (one per exact batch size, least recently used out);
    graph       None: on unless UBPL_PREDICT_GRAPH=0; False: the same path eagerly;
    refine      "none": integer peaks only, no further launch or result key.  "quarter" /
                "taylor": one ubpl_refine_peaks launch after each network's decode (inside the
                graph) adds sub-pixel coordinates under the keys raw_sub, preds_sub,
                preds_mean_sub and refine_rule (pseudo_label: also ens_raw_sub, ens_preds_sub,
                ens_refine_rule, kps_sub); raw, preds and preds_mean keep their integer meaning;
    blur_sigma  "taylor" only: sigma in heatmap cells of the Gaussian blur of the window around
                the peak (0: none; at most 2.0);
    tta         None: one view (two with the flip test), as ever.  A list of (angle_deg, zoom)
                whose first entry is (0, 1): test-time augmentation — every network runs on all
                the views in one batch (ubpl_warp_views makes them; with flip_test each also
                mirrored, at most 16 in all), and ubpl_decode_heatmaps_views warps their heatmaps
                back, averages them over the views that cover each pixel and decodes the merged
                maps, which `heatmaps`, refine and pseudo_label then read.  Chunks shrink so that
                the forward batch stays within 2 max_batch.
    uncertainty False: nothing more.  True (needs tta with at least 2 views in all): every network's
                peak on every view is kept as well — one strided ubpl_decode_heatmaps_flip launch
                per network on the view-major output, and with refine on one ubpl_refine_peaks —
                and one ubpl_view_uncertainty launch over all networks, inside the graph, folds
                them into the reference's view-consistency uncertainty (utils/business.py
                pseudo_cal_unc).  Results gain view_preds [M,V,N,K,2], view_scores [M,V,N,K] (both in
                the output joint order), view_legal [M,N,K] bool, int_dist [M,N,K], aug_coord
                [M,N,K,2], ext_dist, aext_dist, ext_views [N,K], mix_dist and unc [M,N,K]; points
                and distances in image coordinates when center and scale are given, else in
                heatmap cells (1-based, as raw).  A slot then also belongs to one of the two.

    Snapshot semantics: construction and refresh() copy the networks' parameters and
    running statistics into private frozen weight sets; training steps, EMA updates or
    load_state_dict on the networks change nothing here until the next refresh().  The
    networks' training flag, statistics, counters, parameters and own weight buffers are
    never touched."""

    def __init__(self, models, flip_test=False, flip_pairs=None, max_batch=32, max_graphs=4, graph=None,
                 refine="none", blur_sigma=DEFAULT_BLUR_SIGMA, tta=None, uncertainty=False):
        self.refine, taps = check_refine(refine, blur_sigma)
        self.tta = check_tta(tta, flip_test)
        self.uncertainty = check_uncertainty(uncertainty, self.tta, flip_test)
        self.blur_sigma = float(blur_sigma) if refine == "taylor" else None
        _lib.require_gpu()
        from .hourglass import StackedHourglass
        self.models = [models] if isinstance(models, StackedHourglass) else list(models)
        if not self.models or not all(isinstance(m, StackedHourglass) for m in self.models):
            raise TypeError("ubpl_amd: Predictor takes a StackedHourglass or a list of them")
        self.k = self.models[0].k
        self.device = self.models[0].flat_params.device
        if any(m.k != self.k or m.flat_params.device != self.device for m in self.models):
            raise ValueError("ubpl_amd: the networks of a Predictor share k and the device")
        if max_batch < 1 or max_graphs < 1:
            raise ValueError("ubpl_amd: max_batch and max_graphs are at least 1")
        self.flip_test = bool(flip_test)
        self.perm = None
        if flip_pairs:
            self.perm = Kn.flip_perm(self.k, flip_pairs).to(self.device)
        self.taps = None if taps is None else taps.to(self.device)
        self.max_batch, self.max_graphs = int(max_batch), int(max_graphs)
        self.views = None
        if self.tta is not None:
            self.views = len(self.tta) * (2 if self.flip_test else 1)
            self.max_batch = min(self.max_batch, max(1, 2 * self.max_batch // self.views))
            self._view_mats = {}                    # resolution -> device (img_mat, hm_mat, swap)
        if self.uncertainty:
            self._back_mats = {}                    # resolution -> device back [V,6] (view cell -> original cell)
        self.use_graph = os.environ.get("UBPL_PREDICT_GRAPH", "1") != "0" if graph is None else bool(graph)
        self._slots = OrderedDict()
        self._sets = None
        self.refresh()

    # -- weights ----------------------------------------------------------
    def refresh(self):
        """Take the networks' current parameters and running statistics.  The frozen
        buffers are rewritten in place, so captured graphs stay; a network whose conv
        precision changed gets a new frozen set and the graphs are dropped."""
        with torch.cuda.device(self.device), torch.no_grad():
            if self._sets is not None and all(ws.pieces == m.conv_pieces for ws, m in zip(self._sets, self.models)):
                for ws in self._sets:
                    ws.refresh()
                return
            self.release()
            self._sets = [m.freeze() for m in self.models]

    def release(self):
        """Drop every captured graph and its static buffers (their pools go with them)."""
        for s in self._slots.values():
            s.release()
        if self._slots:
            self._slots.clear()
            torch.cuda.empty_cache()

    # -- one batch --------------------------------------------------------
    def _run(self, s):
        """The device work of one batch, on the current stream: static inputs of slot s
        -> its static outputs."""
        if self.tta is not None:
            return self._run_views(s)
        N, K = s.N, self.k
        if self.flip_test:
            Kn.fliplr(s.imgs, out=s.batch[N:])
        for mi, (m, ws) in enumerate(zip(self.models, self._sets)):
            o = m.forward_frozen(s.batch, ws)                       # [N or 2N, S, K, H, W]
            S, H, W = o.shape[1], o.shape[3], o.shape[4]
            if (H, W) != (s.H, s.W):
                raise RuntimeError("ubpl_amd: heatmaps %dx%d, expected %dx%d" % (H, W, s.H, s.W))
            sb, last = S * K * H * W, (S - 1) * K * H * W
            flat = o.reshape(-1)
            # the last stack of rows 0..N and N..2N, in place: row stride + base offset
            hm = flat[last:]
            hm_flip = flat[N * sb + last:] if self.flip_test else None
            Kn.decode_heatmaps_flip(hm, hm_flip, sb, N, K, H, W, self.perm, s.tinv,
                                    out=(s.raw[mi], s.preds[mi], s.scores[mi],
                                         s.heatmaps[mi] if s.heatmaps is not None else None))
            if s.refine:
                Kn.refine_peaks(hm, hm_flip, sb, N, K, H, W, self.perm, s.raw[mi], self.refine, self.taps, s.tinv,
                                out=(s.raw_sub[mi], s.preds_sub[mi], s.rule[mi]))
        s.mean.copy_(torch.stack(list(s.preds), -1).mean(-1))       # projects/MT_UBPL.py:387
        if s.refine:
            s.mean_sub.copy_(torch.stack(list(s.preds_sub), -1).mean(-1))

    def _run_views(self, s):
        """_run with test-time augmentation: the views of s.imgs fill the rest of the view-major
        batch, every network runs once on all of them, and the multi-view decode merges the last
        stacks into s.heatmaps[mi], which the refinement then reads as plain maps."""
        N, K, V = s.N, self.k, self.views
        R = s.batch.shape[2]
        if R not in self._view_mats:
            img_mat, hm_mat, swap = Kn.view_matrices(self.tta, self.flip_test, R, R // 4)
            self._view_mats[R] = (img_mat.to(self.device), hm_mat.to(self.device),
                                  swap.to(self.device) if self.flip_test else None)
        img_mat, hm_mat, swap = self._view_mats[R]
        if V > 1:
            Kn.warp_views(s.imgs, img_mat[1:], out=s.batch[N:])
        for mi, (m, ws) in enumerate(zip(self.models, self._sets)):
            o = m.forward_frozen(s.batch, ws)                       # [V*N, S, K, H, W]
            S, H, W = o.shape[1], o.shape[3], o.shape[4]
            if (H, W) != (s.H, s.W):
                raise RuntimeError("ubpl_amd: heatmaps %dx%d, expected %dx%d" % (H, W, s.H, s.W))
            sb, last = S * K * H * W, (S - 1) * K * H * W
            Kn.decode_heatmaps_views(o.reshape(-1)[last:], N * sb, sb, V, N, K, H, W, hm_mat, swap, self.perm, s.tinv,
                                     out=(s.raw[mi], s.preds[mi], s.scores[mi], s.heatmaps[mi]))
            if s.refine:
                Kn.refine_peaks(s.heatmaps[mi], None, K * H * W, N, K, H, W, None, s.raw[mi], self.refine, self.taps,
                                s.tinv, out=(s.raw_sub[mi], s.preds_sub[mi], s.rule[mi]))
            if s.unc:
                # every view's own peak: the view-major rows share one batch stride, so the last
                # stacks are a strided plain decode of V*N samples (each view's frame and joint order)
                hm_views = o.reshape(-1)[last:]
                Kn.decode_heatmaps_flip(hm_views, None, sb, V * N, K, H, W, None, None,
                                        out=(s.raw_views[mi], None, s.scores_views[mi], None))
                if s.refine:
                    Kn.refine_peaks(hm_views, None, sb, V * N, K, H, W, None, s.raw_views[mi], self.refine, self.taps,
                                    None, out=(s.raw_views_sub[mi], None, None))
        s.mean.copy_(torch.stack(list(s.preds), -1).mean(-1))       # projects/MT_UBPL.py:387
        if s.refine:
            s.mean_sub.copy_(torch.stack(list(s.preds_sub), -1).mean(-1))
        if s.unc:
            if R not in self._back_mats:
                self._back_mats[R] = Kn.view_back_matrices(hm_mat).to(self.device)
            Kn.view_uncertainty(s.raw_views_sub if s.refine else s.raw_views, V * N * K * 2, len(self.models), V, N, K,
                                self._back_mats[R], s.dist_thr, swap, self.perm, s.tinv if s.have_tinv else None,
                                out=(s.view_preds, s.view_legal, s.int_dist, s.aug_coord, s.ext_dist, s.aext_dist,
                                     s.ext_views, s.mix_dist, s.unc_value, s.unc_select))

    def _slot(self, N, R, want_hm, pseudo=False, have_tinv=False):
        # (pseudo_label's slots carry a key of their own: predict's graphs and buffers stay its own)
        want_hm = want_hm or self.tta is not None                   # (the merged maps are the decode's output)
        key = ("pseudo", N, R) if pseudo else (N, R, want_hm)
        if self.uncertainty:                                        # (heatmap cells or image coordinates)
            key = key + (bool(have_tinv),)
        s = self._slots.get(key)
        if s is not None:
            self._slots.move_to_end(key)
            return s, False
        while len(self._slots) >= self.max_graphs:
            _, old = self._slots.popitem(last=False)
            old.release()
            del old
            torch.cuda.empty_cache()
        a = (len(self.models), N, self.k, R, self.flip_test)
        on = self.refine != "none"
        unc = bool(have_tinv) if self.uncertainty else None
        s = self._slots[key] = (_PseudoSlot(*a, self.device, on, self.views, unc) if pseudo else
                                _Slot(*a, want_hm, self.device, on, self.views, unc))
        return s, True

    def _launch(self, s, new, run):
        """run(s) eagerly, or captured once per slot and replayed."""
        if not self.use_graph:
            run(s)
            return
        if new:
            # warm-up: the networks' per-batch-size scratch is allocated here, outside the
            # graph's pool; then the capture (which records, it does not execute)
            run(s)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run(s)
            s.graph = g
        s.graph.replay()

    def _sub_keys(self, s, have):
        """The sub-pixel entries of a predict / pseudo_label result (refine on)."""
        return {"raw_sub": s.raw_sub.clone(), "preds_sub": s.preds_sub.clone() if have else None,
                "preds_mean_sub": s.mean_sub.clone() if have else None, "refine_rule": s.rule.clone()}

    def _unc_keys(self, s):
        """The view-consistency entries of a predict / pseudo_label result (uncertainty on)."""
        M, V = len(self.models), self.views
        scores = s.scores_views.reshape(M, V, s.N, self.k).clone()
        if self.flip_test and self.perm is not None:                # the mirrored views, in the output joint order
            scores[:, V // 2:] = scores[:, V // 2:][..., self.perm.long()]
        return {"view_preds": s.view_preds.clone(), "view_scores": scores, "view_legal": s.view_legal > 0,
                "int_dist": s.int_dist.clone(), "aug_coord": s.aug_coord.clone(), "ext_dist": s.ext_dist.clone(),
                "aext_dist": s.aext_dist.clone(), "ext_views": s.ext_views.clone(), "mix_dist": s.mix_dist.clone(),
                "unc": s.unc_value.clone()}

    def _predict_chunk(self, imgs, tinv, want_hm):
        N, R = imgs.shape[0], imgs.shape[2]
        s, new = self._slot(N, R, want_hm, have_tinv=tinv is not None)
        s.imgs.copy_(imgs, non_blocking=True)
        if tinv is not None:
            s.tinv.copy_(tinv, non_blocking=True)
        self._launch(s, new, self._run)
        out = {"raw": s.raw.clone(), "scores": s.scores.clone(),
               "preds": s.preds.clone() if tinv is not None else None,
               "preds_mean": s.mean.clone() if tinv is not None else None}
        if s.refine:
            out.update(self._sub_keys(s, tinv is not None))
        if s.unc:
            out.update(self._unc_keys(s))
        if want_hm:
            out["heatmaps"] = s.heatmaps.clone()
        return out

    def _inputs(self, what, imgs, center, scale, out_res):
        """The argument checks of predict / pseudo_label -> (contiguous images, tinv or None)."""
        if not torch.is_tensor(imgs) or imgs.dtype != torch.float32 or imgs.dim() != 4 or imgs.shape[1] != 3 \
                or imgs.shape[2] != imgs.shape[3] or imgs.shape[0] < 1:
            raise TypeError("ubpl_amd: %s takes float32 images [N,3,R,R], N >= 1" % what)
        if (center is None) != (scale is None):
            raise ValueError("ubpl_amd: center and scale come together")
        N, R = imgs.shape[0], imgs.shape[2]
        tinv = None
        if center is not None:
            from .process import inverse_transforms
            res = [R // 4, R // 4] if out_res is None else [out_res, out_res]
            tinv = inverse_transforms(center, scale, res)
            if tinv.shape[0] != N:
                raise ValueError("ubpl_amd: %d centers for %d images" % (tinv.shape[0], N))
        return imgs.contiguous(), tinv

    def predict(self, imgs, center=None, scale=None, return_heatmaps=False, out_res=None):
        """imgs float32 [N,3,R,R] (host or device) -> dict of device tensors, the caller's own:
        raw [M,N,K,2] 1-based heatmap coordinates, scores [M,N,K], preds [M,N,K,2] and
        preds_mean [N,K,2] in image coordinates (None without center / scale), and with
        return_heatmaps heatmaps [M,N,K,H,W], the (flip- or view-merged) last-stack maps; M networks.
        out_res: the resolution of the inverse transform (default: the heatmaps')."""
        imgs, tinv = self._inputs("predict", imgs, center, scale, out_res)
        N = imgs.shape[0]
        outs = []
        with torch.cuda.device(self.device), torch.no_grad():
            for a in range(0, N, self.max_batch):
                b = min(N, a + self.max_batch)
                outs.append(self._predict_chunk(imgs[a:b], None if tinv is None else tinv[a:b], bool(return_heatmaps)))
        if len(outs) == 1:
            return outs[0]
        per_sample = ("preds_mean", "preds_mean_sub") + self._PER_SAMPLE_UNC
        return {k: None if outs[0][k] is None else torch.cat([o[k] for o in outs], self._cat_axis(k, per_sample))
                for k in outs[0]}

    # -- ensemble pseudo-labels --------------------------------------------
    def _run_pseudo(self, s):
        """_run, then the ensemble kernel on the merged heatmaps it left in s.heatmaps
        (the members' peaks are s.scores already: not written again) and the members'
        spread around the ensemble peak."""
        self._run(s)
        M, N, K, H, W = len(self.models), s.N, self.k, s.H, s.W
        Kn.ensemble_pseudo(s.heatmaps, N * K * H * W, K * H * W, M, N, K, H, W, s.thr, s.tinv,
                           out=(s.ens_raw, s.ens_preds, s.ens_score, None, s.disagree, s.select,
                                s.mean_hm))
        d = s.raw - s.ens_raw
        s.spread.copy_((d * d).sum(-1).sqrt().amax(0))
        if s.refine:                                                # the ensemble peak, on T itself
            Kn.refine_peaks(s.mean_hm, None, K * H * W, N, K, H, W, None, s.ens_raw, self.refine, self.taps, s.tinv,
                            out=(s.ens_raw_sub, s.ens_preds_sub, s.ens_rule))

    def _pseudo_chunk(self, imgs, tinv, thr, rule, want_hm, dist_thr=None):
        N, R = imgs.shape[0], imgs.shape[2]
        s, new = self._slot(N, R, True, pseudo=True, have_tinv=tinv is not None)
        s.imgs.copy_(imgs, non_blocking=True)
        if tinv is not None:
            s.tinv.copy_(tinv, non_blocking=True)
        s.thr.fill_(thr)                                            # read by the kernel at replay
        if s.unc:
            s.dist_thr.fill_(0.0 if dist_thr is None else dist_thr)  # likewise
        self._launch(s, new, self._run_pseudo)
        have = tinv is not None
        select = s.select > 0
        if rule == "uncertainty":
            selected = (s.unc_select > 0).all(0)
        else:
            selected = select.all(0) if rule == "unanimous" else s.ens_score >= s.thr
        out = {"raw": s.raw.clone(), "scores": s.scores.clone(),
               "preds": s.preds.clone() if have else None,
               "preds_mean": s.mean.clone() if have else None,
               "ens_raw": s.ens_raw.clone(), "ens_preds": s.ens_preds.clone() if have else None,
               "ens_score": s.ens_score.clone(), "member_select": select, "disagree": s.disagree.clone(),
               "selected": selected, "spread": s.spread.clone(),
               "kps": assemble_kps(s.ens_preds, selected) if have else None}
        if s.refine:
            out.update(self._sub_keys(s, have))
            out.update({"ens_raw_sub": s.ens_raw_sub.clone(), "ens_preds_sub": s.ens_preds_sub.clone() if have else None,
                        "ens_refine_rule": s.ens_rule.clone(),
                        "kps_sub": assemble_kps(s.ens_preds_sub, selected) if have else None})
        if s.unc:
            out.update(self._unc_keys(s))
            if dist_thr is not None:
                out["unc_select"] = s.unc_select > 0
        if want_hm:
            out["heatmaps"] = s.heatmaps.clone()
            out["mean_heatmap"] = s.mean_hm.clone()
        return out

    _PER_MEMBER = ("raw", "scores", "preds", "member_select", "disagree", "heatmaps", "raw_sub", "preds_sub",
                   "refine_rule", "view_legal", "int_dist", "aug_coord", "mix_dist", "unc", "unc_select")
    _PER_SAMPLE_UNC = ("ext_dist", "aext_dist", "ext_views")
    _PER_VIEW = ("view_preds", "view_scores")                       # [M,V,N,...]

    def _cat_axis(self, key, per_sample):
        """The sample axis of a result key: chunks are concatenated along it."""
        return 2 if key in self._PER_VIEW else 0 if key in per_sample else 1

    def pseudo_label(self, imgs, center=None, scale=None, thr=0.95, rule="unanimous", return_heatmaps=False,
                     out_res=None, dist_thr=None):
        """The UBPL ensemble pseudo-labels of imgs (JointPseudoLoss3's target and mask,
        utils/losses.py:176-210, with every network in the student's place in turn): which
        joints do the networks agree on confidently enough to use as labels?  Same inputs,
        forwards, flip test and chunking as predict.  -> dict of device tensors, the caller's
        own: everything predict returns, and
          ens_raw [N,K,2], ens_score [N,K]   the decode of T, the per-pixel mean of the M
                                             networks' heatmaps (:179);
          ens_preds [N,K,2]                  ens_raw in image coordinates (None without center / scale);
          member_select [M,N,K] bool         max_px p_m >= thr and ens_score >= thr (:187-193);
          disagree [M,N,K]                   mean_px (p_m - T)^2 (:184);
          selected [N,K] bool                rule "unanimous": every member selects;
                                             rule "ensemble": ens_score >= thr alone;
                                             rule "uncertainty": unc_select of every member;
          spread [N,K]                       max over m of |raw[m] - ens_raw|, heatmap pixels;
          kps [N,K,3]                        (ens_preds x, y, selected as 0/1), the meta["kpsMap"]
                                             layout (None without center / scale);
        with refine on, predict's sub-pixel keys and ens_raw_sub [N,K,2], ens_preds_sub [N,K,2],
        ens_refine_rule [N,K] (the refinement of the ensemble peak on T) and kps_sub [N,K,3]
        (ens_preds_sub x, y, selected); spread stays on the integer peaks;
        with return_heatmaps, heatmaps [M,N,K,H,W] and mean_heatmap [N,K,H,W] (T);
        with uncertainty on, predict's view-consistency keys, and with dist_thr given (required
        by rule "uncertainty": the reference's args.distThrMax has no default) unc_select [M,N,K]
        bool: the member is legal, int_dist, ext_dist and aext_dist are each <= dist_thr and
        mix_dist <= 3 dist_thr (utils/business.py:331-345, :242-247), dist_thr in the units of the
        distances (image pixels with center / scale, else heatmap cells).
        thr defaults to the reference's pseudoScoreThr; one captured graph serves every thr and
        every dist_thr."""
        check_rule(rule)
        dist_thr = check_dist_thr(rule, dist_thr, self.uncertainty)
        if len(self.models) > 8:
            raise ValueError("ubpl_amd: pseudo_label takes up to 8 networks, got %d" % len(self.models))
        imgs, tinv = self._inputs("pseudo_label", imgs, center, scale, out_res)
        N = imgs.shape[0]
        outs = []
        with torch.cuda.device(self.device), torch.no_grad():
            for a in range(0, N, self.max_batch):
                b = min(N, a + self.max_batch)
                outs.append(self._pseudo_chunk(imgs[a:b], None if tinv is None else tinv[a:b], float(thr), rule,
                                               bool(return_heatmaps), dist_thr))
        if len(outs) == 1:
            return outs[0]
        per_sample = [k for k in outs[0] if k not in self._PER_MEMBER]
        return {k: None if outs[0][k] is None else torch.cat([o[k] for o in outs], self._cat_axis(k, per_sample))
                for k in outs[0]}

    def label_pool(self, loader, args=None, thr=0.95, rule="unanimous", dist_thr=None):
        """pseudo_label over a loader of (imgMap, _, meta) batches with meta["center"] /
        meta["scale"] (the shape validate takes; args.outRes, when given, is the resolution of
        the inverse transform).  -> a host dict of plain lists, sample-major: predsArraies
        (the reference's key, projects/MT_UBPL.py:120: [x, y] per joint from ens_preds; with
        refine on from ens_preds_sub, and the dict records "refine" and "blur_sigma"; with tta
        set it records "tta", the views),
        selected, ens_score, spread [N][K], disagree [N][M][K], thr, rule and
        selected_fraction [K].  With uncertainty on it also records int_dist, unc [N][M][K],
        ext_dist, aext_dist [N][K] and dist_thr (None when not given), in image pixels.  Single
        process only, as validate."""
        from . import dist as D
        if D.is_dist():
            raise NotImplementedError("ubpl_amd: Predictor.label_pool runs in one process")
        check_rule(rule)
        dist_thr = check_dist_thr(rule, dist_thr, self.uncertainty)
        on = self.refine != "none"
        keys = ("ens_preds_sub" if on else "ens_preds", "selected", "ens_score", "spread", "disagree")
        if self.uncertainty:
            keys += ("int_dist", "unc", "ext_dist", "aext_dist")
        cols = {k: [] for k in keys}
        for imgMap, _, meta in loader:
            out = self.pseudo_label(imgMap.float(), meta["center"], meta["scale"], thr=thr, rule=rule,
                                    out_res=None if args is None else args.outRes, dist_thr=dist_thr)
            for k in ("disagree",) + (("int_dist", "unc") if self.uncertainty else ()):   # [M,N,K] -> sample-major
                out[k] = out[k].transpose(0, 1)
            for k in keys:
                cols[k].append(out[k].cpu())
        cat = {k: torch.cat(v) if v else torch.zeros(0) for k, v in cols.items()}
        sel = cat["selected"]
        d = {"predsArraies": cat[keys[0]].tolist(), "selected": sel.tolist(),
             "ens_score": cat["ens_score"].tolist(), "spread": cat["spread"].tolist(),
             "disagree": cat["disagree"].tolist(), "thr": float(thr), "rule": rule,
             "selected_fraction": sel.float().mean(0).tolist() if sel.numel() else []}
        if on:
            d.update({"refine": self.refine, "blur_sigma": self.blur_sigma})
        if self.tta is not None:
            d["tta"] = [list(v) for v in self.tta]
        if self.uncertainty:
            d.update({k: cat[k].tolist() for k in ("int_dist", "unc", "ext_dist", "aext_dist")})
            d["dist_thr"] = dist_thr
        return d

    def validate(self, loader, args):
        """train.validate(loader, models, args) from the frozen snapshot: the same triple
        (predsArray, accs_records, errs_records), folded by the same code.  Single process
        only: under torch.distributed this raises NotImplementedError (train.validate shards
        and gathers the batches).  With refine on, the sub-pixel predictions are scored."""
        from . import dist as D
        from . import train as T
        if D.is_dist():
            raise NotImplementedError("ubpl_amd: Predictor.validate runs in one process; use train.validate "
                                      "under torch.distributed")
        rows = []
        for imgMap, _, meta in loader:
            out = self.predict(imgMap.float(), meta["center"], meta["scale"], out_res=args.outRes)
            sub = "_sub" if self.refine != "none" else ""
            pm = list(out["preds" + sub]) + [out["preds_mean" + sub]]
            rows.append(T.valid_batch_row(pm, meta, self.device, args))
        return T.fold_valid_rows(rows, len(self.models) + 1)
