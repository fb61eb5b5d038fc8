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
import os
from functools import partial

import torch

from . import _lib
from . import kernels as Kn
from . import predict_slots as PS
from .predict_args import (DEFAULT_BLUR_SIGMA, REFINES, RULES, assemble_kps, check_dist_thr,  # noqa: F401
                           check_refine, check_rule, check_tta, check_uncertainty, view_count)


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
        self.perm = Kn.flip_perm(self.k, flip_pairs).to(self.device) if flip_pairs else None
        self.taps = None if taps is None else taps.to(self.device)
        self.max_batch, self.max_graphs = int(max_batch), int(max_graphs)
        self.views = view_count(self.tta, self.flip_test) or None
        if self.tta is not None:
            self.max_batch = min(self.max_batch, max(1, 2 * self.max_batch // self.views))
            self._view_mats = {}                    # resolution -> device (img_mat, hm_mat, swap)
        if self.uncertainty:
            self._back_mats = {}                    # resolution -> device back [V,6] (view cell -> original cell)
        self.use_graph = os.environ.get("UBPL_PREDICT_GRAPH", "1") != "0" if graph is None else bool(graph)
        self._slots = PS.SlotCache()
        self._spec = partial(PS.SlotSpec, len(self.models), self.k, self.flip_test, self.views, self.refine != "none",
                             self.uncertainty)               # + (pseudo, N, R, want_hm, have_tinv) of a call
        self._sets = None
        self.refresh()

    @property
    def passes(self):
        """Forward passes per image and network: the views, else 2 with the flip test, else 1."""
        return self.views or (2 if self.flip_test else 1)

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
    def _last_stacks(self, s):
        """Every network's frozen forward of s.batch in turn -> (mi, the flat output from row 0's
        last stack on — a view, so the rows' last stacks lie sb floats apart in it —, sb)."""
        K = self.k
        for mi, (m, ws) in enumerate(zip(self.models, self._sets)):
            o = m.forward_frozen(s.batch, ws)                       # [rows, S, K, H, W]
            S, H, W = o.shape[1], o.shape[3], o.shape[4]
            if (H, W) != (s.H, s.W):
                raise RuntimeError("ubpl_amd: heatmaps %dx%d, expected %dx%d" % (H, W, s.H, s.W))
            yield mi, o.reshape(-1)[(S - 1) * K * H * W:], S * K * H * W

    def _means(self, s):
        s.mean.copy_(torch.stack(list(s.preds), -1).mean(-1))       # projects/MT_UBPL.py:387
        if s.refine:
            s.mean_sub.copy_(torch.stack(list(s.preds_sub), -1).mean(-1))

    def _run(self, s):
        """The device work of one batch, on the current stream: static inputs of slot s
        -> its static outputs."""
        if self.tta is not None:
            return self._run_views(s)
        N, K, H, W = s.N, self.k, s.H, s.W
        if self.flip_test:
            Kn.fliplr(s.imgs, out=s.batch[N:])
        for mi, hm, sb in self._last_stacks(s):
            hm_flip = hm[N * sb:] if self.flip_test else None       # rows N..2N, in place
            Kn.decode_heatmaps_flip(hm, hm_flip, sb, N, K, H, W, self.perm, s.tinv,
                                    out=(s.raw[mi], s.preds[mi], s.scores[mi],
                                         s.heatmaps[mi] if s.spec.want_hm else None))
            if s.refine:
                Kn.refine_peaks(hm, hm_flip, sb, N, K, H, W, self.perm, s.raw[mi], self.refine, self.taps, s.tinv,
                                out=(s.raw_sub[mi], s.preds_sub[mi], s.rule[mi]))
        self._means(s)

    def _run_views(self, s):
        """_run with test-time augmentation: the views of s.imgs fill the rest of the view-major
        batch, every network runs once on all of them, and the multi-view decode merges the last
        stacks into s.heatmaps[mi], which the refinement then reads as plain maps."""
        N, K, V, H, W = s.N, self.k, self.views, s.H, s.W
        R = s.batch.shape[2]
        if R not in self._view_mats:
            img_mat, hm_mat, swap = Kn.view_matrices(self.tta, self.flip_test, R, R // 4)
            self._view_mats[R] = (img_mat.to(self.device), hm_mat.to(self.device),
                                  swap.to(self.device) if self.flip_test else None)
        img_mat, hm_mat, swap = self._view_mats[R]
        if V > 1:
            Kn.warp_views(s.imgs, img_mat[1:], out=s.batch[N:])
        for mi, hm_views, sb in self._last_stacks(s):
            Kn.decode_heatmaps_views(hm_views, N * sb, sb, V, N, K, H, W, hm_mat, swap, self.perm, s.tinv,
                                     out=(s.raw[mi], s.preds[mi], s.scores[mi], s.heatmaps[mi]))
            if s.refine:
                Kn.refine_peaks(s.heatmaps[mi], None, K * H * W, N, K, H, W, None, s.raw[mi], self.refine, self.taps,
                                s.tinv, out=(s.raw_sub[mi], s.preds_sub[mi], s.rule[mi]))
            if s.unc:
                # every view's own peak: the view-major rows share one batch stride, so the last
                # stacks are a strided plain decode of V*N samples (each view's frame and joint order)
                Kn.decode_heatmaps_flip(hm_views, None, sb, V * N, K, H, W, None, None,
                                        out=(s.raw_views[mi], None, s.scores_views[mi], None))
                if s.refine:
                    Kn.refine_peaks(hm_views, None, sb, V * N, K, H, W, None, s.raw_views[mi], self.refine, self.taps,
                                    None, out=(s.raw_views_sub[mi], None, None))
        self._means(s)
        if s.unc:
            if R not in self._back_mats:
                self._back_mats[R] = Kn.view_back_matrices(hm_mat).to(self.device)
            Kn.view_uncertainty(s.raw_views_sub if s.refine else s.raw_views, V * N * K * 2, len(self.models), V, N, K,
                                self._back_mats[R], s.dist_thr, swap, self.perm, s.tinv if s.spec.have_tinv else None,
                                out=(s.view_preds, s.view_legal, s.int_dist, s.aug_coord, s.ext_dist, s.aext_dist,
                                     s.ext_views, s.mix_dist, s.unc_value, s.unc_select))

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

    # -- one call ---------------------------------------------------------
    def _chunk(self, imgs, tinv, pseudo, want_hm, thr=None, dist_thr=None, rule=None):
        """One chunk through its slot: static inputs filled, launched, the result cloned out.
        (pseudo_label's slots are their own: predict's graphs and buffers stay its own.)"""
        spec = self._spec(pseudo, imgs.shape[0], imgs.shape[2], want_hm, tinv is not None)
        s, new = self._slots.fetch(spec, self.max_graphs, self.device)
        s.imgs.copy_(imgs, non_blocking=True)
        if tinv is not None:
            s.tinv.copy_(tinv, non_blocking=True)
        if pseudo:                                                  # read by the kernels at replay
            s.thr.fill_(thr)
            if s.unc:
                s.dist_thr.fill_(0.0 if dist_thr is None else dist_thr)
        PS.launch(s, new, self._run_pseudo if pseudo else self._run, self.use_graph)
        return PS.result(s, PS.Ask(tinv is not None, want_hm, dist_thr, rule, self.perm))

    def _chunked(self, what, imgs, center, scale, out_res, **chunk_kw):
        """The argument checks of predict / pseudo_label, then _chunk over at most max_batch images
        at a time, and the chunks' results as one."""
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
        imgs, B = imgs.contiguous(), self.max_batch
        with torch.cuda.device(self.device), torch.no_grad():
            return PS.concat([self._chunk(imgs[a:a + B], None if tinv is None else tinv[a:a + B], **chunk_kw)
                              for a in range(0, N, B)])

    def predict(self, imgs, center=None, scale=None, return_heatmaps=False, out_res=None):
        """imgs float32 [N,3,R,R] (host or device) -> dict of device tensors, the caller's own:
        raw [M,N,K,2] 1-based heatmap coordinates, scores [M,N,K], preds [M,N,K,2] and
        preds_mean [N,K,2] in image coordinates (None without center / scale), and with
        return_heatmaps heatmaps [M,N,K,H,W], the (flip- or view-merged) last-stack maps; M networks.
        out_res: the resolution of the inverse transform (default: the heatmaps')."""
        return self._chunked("predict", imgs, center, scale, out_res, pseudo=False, want_hm=bool(return_heatmaps))

    # -- from raw frames ---------------------------------------------------
    def _crop(self, bank, center, scale, frame, res):
        """The boxes of a frames.FrameBank as network inputs [n,3,res,res]: the
        reference's evaluation crop (ubpl_crop_frames), run eagerly on the current stream ahead
        of the replay — frame sizes vary, so it is no part of a captured graph."""
        if bank.bank.device != self.device:
            raise ValueError("ubpl_amd: the FrameBank lives on %s, the networks on %s"
                             % (bank.bank.device, self.device))
        with torch.cuda.device(self.device), torch.no_grad():
            return bank.crop(frame, center, scale, res)

    def predict_frames(self, bank, center, scale, res, frame=None, **predict_kwargs):
        """predict on boxes of raw frames: bank a frames.FrameBank (uint8 BGR frames of any
        sizes), box i = (frame[i], center[i] = (x, y), scale[i]) with frame None meaning box i
        of frame i, res the side of the networks' input (required: a Predictor serves any input
        size, so there is none to default to).  The result is predict's on
        bank.crop(frame, center, scale, res) with the same center / scale, bit for bit."""
        return self.predict(self._crop(bank, center, scale, frame, res), center, scale, **predict_kwargs)

    def pseudo_label_frames(self, bank, center, scale, res, frame=None, **pseudo_kwargs):
        """pseudo_label on boxes of raw frames (see predict_frames)."""
        return self.pseudo_label(self._crop(bank, center, scale, frame, res), center, scale, **pseudo_kwargs)

    # -- ensemble pseudo-labels --------------------------------------------
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
        return self._chunked("pseudo_label", imgs, center, scale, out_res, pseudo=True,
                             want_hm=bool(return_heatmaps), thr=float(thr), dist_thr=dist_thr, rule=rule)

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
        unc_keys = ("int_dist", "unc", "ext_dist", "aext_dist") if self.uncertainty else ()
        keys = ("ens_preds_sub" if on else "ens_preds", "selected", "ens_score", "spread", "disagree") + unc_keys
        cols = {k: [] for k in keys}
        for imgMap, _, meta in loader:
            out = self.pseudo_label(imgMap.float(), meta["center"], meta["scale"], thr=thr, rule=rule,
                                    out_res=None if args is None else args.outRes, dist_thr=dist_thr)
            for k in keys:                                          # ([M,N,K] -> sample-major)
                cols[k].append((out[k].transpose(0, 1) if PS.AXIS[k] == 1 else out[k]).cpu())
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
            d.update({k: cat[k].tolist() for k in unc_keys})
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
