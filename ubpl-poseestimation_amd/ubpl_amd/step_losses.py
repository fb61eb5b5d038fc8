"""Device-count loss helpers of the training steps (same row semantics as
ubpl_amd.losses): every loss sum and every count stays a device tensor.  The loss
section of each train.py step (between the networks' forwards and the backward)
builds its sums, counts and FDL views from these; _RecordLayout says where they go."""
import torch

from . import kernels as Kn
from .losses import NO_RULE, _RowLoss, features_cov
from .process import render_batch


def _stacked(preds, S):
    """(B, S, K, HW) of [B,S,K,R,R] predictions: a row per (sample, stack, keypoint)."""
    return preds.shape[0], S, preds.shape[2], preds.shape[-1] * preds.shape[-2]


def _mse(preds, gts, S, gate, sw):
    """JointMSELoss(nStack=S, useKPsGate=True, useSampleWeight=True): (sum, cnt[4])."""
    rows = Kn.RowSpec.ground_truth(*_stacked(preds, S))
    return _RowLoss.apply(preds, gts, rows, 0, NO_RULE, gate is not None, sw is not None, gate, sw)[:2]


def _mse_plain(preds, gts, S):
    """JointMSELoss(nStack=S) without gate/weights (projects/supervised.py:138);
    nStack == 1 keeps the reference's per-sample rows (Kn.pred_rows)."""
    rows = Kn.RowSpec.ground_truth(*Kn.pred_rows(preds, S))
    return _RowLoss.apply(preds, gts, rows, 0, NO_RULE, False, False, None, None)[:2]


def _last_pair(preds, tpreds):
    """The last stacks of both, contiguous, and their same-layout rows."""
    a = preds[:, -1].contiguous()
    t = tpreds[:, -1].contiguous()
    return a, t, Kn.RowSpec.same(a.shape[0], 1, a.shape[1], a.shape[-1] * a.shape[-2])


def _dist_last(preds, tpreds):
    """JointDistLoss() on the last stack of both (projects/MT_UBPL.py:250)."""
    a, t, rows = _last_pair(preds, tpreds)
    return _RowLoss.apply(a, t, rows, 0, NO_RULE, False, False, None, None)[:2]


def _dist_mt2_last(preds, tpreds, sw, thr):
    """JointDistLoss_mt2(useSampleWeight=True, scoreThr) on the last stacks
    (projects/DualPose_UBPL.py:163,203)."""
    a, t, rows = _last_pair(preds, tpreds)
    return _RowLoss.apply(a, t, rows, 1, ("max", float(thr)), False, True, None, sw)[:3]


def _ens_rows(preds, targets, S):
    """Rows of preds [B,S,K,R,R] against the ensemble targets [M,B,St,K,R,R]."""
    return Kn.RowSpec.ensemble(*_stacked(preds, S), targets.shape[0], targets.shape[2])


def _pseudo(preds, targets, sw, S, thr):
    """JointPseudoLoss3(nStack=S, scoreThr) with targets [M,B,S,K,R,R]."""
    return _RowLoss.apply(preds, targets, _ens_rows(preds, targets, S), 2, ("max", float(thr)), False, True, None,
                          sw)[:3]


def _pseudo_gated(preds, targets, sw, S, thr, gate):
    """_pseudo with a given selection (ubpl_loss_finalize kind 3): gate [B,K] device float32, > 0 =
    the joint's pseudo label is kept; the row mask is gate * the two score tests at thr
    (thr = -inf: the gate alone; a NaN score still never selects)."""
    rows = _ens_rows(preds, targets, S)
    if gate is None or gate.numel() != rows.B * rows.K:
        raise ValueError("ubpl_amd: _pseudo_gated takes a gate of [B,K] = %d x %d entries" % (rows.B, rows.K))
    return _RowLoss.apply(preds, targets, rows, 3, ("max", float(thr)), False, True, gate, sw)[:3]


def _pseudo_ranked(preds, targets, sw, S, rank):
    """JointPseudoLoss2(nStack=S) with targets [M,B,S,K,R,R] in _pseudo's place: the row mask is
    each input's softmax score >= the rank-th smallest of the batch's B*K (rank a host integer,
    losses.sel_rank) -> (sum, cnt[4], score[K], thr[2*S]: rateThr1[S] then rateThr2[S]), all on the
    device; the rank selections run inside the finalize launch (ubpl_loss_finalize_rank)."""
    return _RowLoss.apply(preds, targets, _ens_rows(preds, targets, S), 2, ("rank", int(rank)), False, True, None, sw)


def _norm(s, n):
    """(s / n) if n > 0 else s — with n a device tensor."""
    n = n.float()
    return torch.where(n > 0, s / n.clamp(min=1.0), s)


def _fdl_view(fa, fb, rowmask, args):
    """One view of the multi-view feature decorrelation term (projects/MT_UBPL.py:
    301-330, DualPose_UBPL.py:246-270) over the selected rows (rowmask > 0):
    returns (kind, value, n_loc) with n_loc a device float[1].

    'covariance' (FDL_type default): value = ProcessUtils.features_cov of the
    selected rows = their MEAN |cov| (0 when no row of this rank is selected),
    n_loc = rows * S * C.  Any other FDL_type: the reference's else branch,
    JointFeatureDistLoss (utils/losses.py:56-70): value = SUM over the selected
    (sample, stack, channel) rows of the pixel-mean squared distance, n_loc =
    rows * S.  The value of a covariance view is a mean, so under data
    parallelism _fdl_total rescales it by n_loc / N_glob before summing."""
    if args.FDL_type == "covariance":
        v, c = features_cov(fa, fb, rowmask)
        n = c.float()
        return "cov", torch.where(n[0] > 0, v, torch.zeros_like(v)), n
    B, S, C = fa.shape[:3]
    rows = Kn.RowSpec.flat(B, S * C, fa[0, 0, 0].numel())
    s = _RowLoss.apply(fa.contiguous(), fb.contiguous(), rows, 0, NO_RULE, False, True, None,
                       rowmask.reshape(-1).contiguous())[0]
    return "dist", s, ((rowmask > 0).sum() * S).float().reshape(1)


def _fdl_total(views, gcounts_v, W, weight):
    """fdc = FDLWeight * (sum_a value_a) / (sum_a N_a) with global counts N_a
    (MT_UBPL.py:329).  A covariance view is a mean over this rank's rows;
    value_a * n_loc_a / N_a is its share of the global-batch mean (exactly
    value_a on one rank), so the SUM all-reduce of the gradients gives the
    single-device gradient."""
    terms = []
    for (kind, v, n_loc), N_a in zip(views, gcounts_v):
        if kind == "cov" and W > 1:
            v = v * (n_loc[0] / N_a.clamp(min=1.0))
        terms.append(v)
    return weight * _norm(sum(terms), sum(gcounts_v))


def _fdl_record_sums(views):
    """What each rank contributes to the all-reduced FDL record: the local
    SUM (covariance: mean * rows)."""
    return [v.detach() * n[0] if kind == "cov" else v.detach() for kind, v, n in views]


def _fdl_record(views, gsums_v, gcounts_v, W, weight):
    if W == 1:
        vals = [v.detach() for _, v, _ in views]
    else:
        vals = [s / N.clamp(min=1.0) if kind == "cov" else s
                for (kind, _, _), s, N in zip(views, gsums_v, gcounts_v)]
    return weight * _norm(sum(vals), sum(gcounts_v))


def _fdl_rows(sw, args):
    if args.FDL_label == "labeled":
        return (sw > 0).float()
    if args.FDL_label == "unlabeled":
        return (sw == 0).float()
    return torch.ones_like(sw)


def _islabeled(meta_isl, dev):
    return meta_isl.to(dev, non_blocking=True).reshape(-1)


def _w(isl, lab, unlab):
    one = torch.ones(isl.shape[0], device=isl.device)
    return torch.where(isl > 0, lab * one, unlab * one).contiguous()


def _targets(imgs, hms, meta, A, dev, args):
    """Heatmaps and gates per view: either given (reference batch format) or
    rendered on the device from meta['kps'] (list of [B,K,3] per view)."""
    if hms is not None:
        hs = [h[0].to(dev, non_blocking=True).float().contiguous() for h in hms]
        gs = [kw[0].to(dev, non_blocking=True).float().contiguous() for kw in meta["kpsWeights"]]
        return hs, gs
    hs, gs = [], []
    inp = imgs[0].shape[-1]
    for a in range(A):
        hm, kk = render_batch(meta["kps"][a].to(dev).float(), (imgs[a].shape[-2], imgs[a].shape[-1]), inp,
                              args.outRes if hasattr(args, "outRes") else inp // 4)
        hs.append(hm)
        gs.append(kk[:, :, 2].contiguous())
    return hs, gs


class _RecordLayout:
    """Where everything sits in a generator step's three vectors — the only
    place that knows offsets; the cores pack by it, the decoders read by it.
      sums (local / all-reduced): per model SUMS, then one per FDL view
      counts:                     per model `counts`, then one per FDL view
      packed (the one device->host copy): [3M+1 records: per model RECS, then fdc | counts | `blocks` x K scores]
                                          and, only with rate_thr (the "rate" pseudo rule): [| per model rateThr1, rateThr2]
    A plain host object (no tensors): built when the step is captured and reused at every replay."""
    SUMS = ("mtc", "pec", "epc")
    RECS = ("pec", "mtc", "epc")

    def __init__(self, M, counts, nfd, K, blocks=1, rate_thr=False):
        self.M, self.counts, self.nfd, self.K = M, tuple(counts), nfd, K
        nc = len(self.counts) * M
        self.nrec, self.ncn = 3 * M + 1, nc + nfd
        self.size = self.nrec + self.ncn + blocks * K
        self.rate_thr = slice(self.size, self.size + 2 * M) if rate_thr else None     # in packed
        self.size = self.rate_thr.stop if rate_thr else self.size
        self.fdc = 3 * M                                              # in packed: the FDL record
        self.fdl_sums = slice(3 * M, 3 * M + nfd)                     # in sums: the FDL views
        self.fdl_counts = slice(nc, nc + nfd)                         # in counts
        self.fdl_n = slice(self.nrec + nc, self.nrec + nc + nfd)      # in packed

    def s(self, name, mi):                    # in sums: model mi's sum `name`
        return 3 * mi + self.SUMS.index(name)

    def c(self, name, mi):                    # in counts: model mi's count `name`
        return len(self.counts) * mi + self.counts.index(name)

    def r(self, name, mi):                    # in packed: model mi's record `name`
        return 3 * mi + self.RECS.index(name)

    def n(self, name, mi):                    # in packed: model mi's count `name`
        return self.nrec + self.c(name, mi)

    def total(self, host, name):              # of packed.tolist(): the count `name` summed over the models
        return int(sum(host[self.n(name, mi)] for mi in range(self.M)))

    def scores(self, block=0):                # in packed: score block `block`
        return slice(self.nrec + self.ncn + block * self.K, self.nrec + self.ncn + (block + 1) * self.K)
