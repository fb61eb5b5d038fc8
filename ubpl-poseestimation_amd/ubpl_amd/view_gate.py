"""The view-consistency pseudo-label rule of the MT_UBPL training step ("View-consistency
rule in the training step"): its options, its device constants and the gate itself.

The step runs every sample as A augmented views through both teachers.  With args.pseudoRule
"uncertainty" or "score+uncertainty" the teachers' last-stack peaks of every view are decoded
(and refined), mapped back into source-image pixels through each (view, sample)'s own matrix and
folded by ubpl_view_uncertainty_samples — the reference's pseudo_cal_unc (utils/business.py:
220-234), which it wrote for training and wired into no project — into gate [B,K]: 1 where every
teacher's peaks agree across the views and with the other teachers within args.distThrMax pixels.
The gate then masks the ensemble-pseudo loss (step_losses._pseudo_gated).

RULES is the one list of the step's pseudo-label rules, so the "rate" rule (rank-based selection,
step_losses._pseudo_ranked) has its option check here too; it needs no gate and no constants.

VIEWS is the list of args.pseudoViews, where the pseudo loss of view a takes its targets from
("Cross-view pseudo-label targets"): "own" — the teachers' maps of view a, the step
as the reference has it; "merged" — the mean of every view's maps warped into view a's frame;
"other" — the same without view a's own.  It combines with every rule: the rule says which joints
are kept, the views what they are pulled towards."""
import torch

from . import kernels as Kn
from . import predict_args as PA

RULES = ("score", "uncertainty", "score+uncertainty", "rate")
VIEWS = ("own", "merged", "other")


def check_sel_rate(rule, value):
    """args.pseudoSelRate of the "rate" rule ("Rank-based pseudo-label selection"): the
    share of the batch's joints the ensemble-pseudo term keeps, a float in (0, 1]; required, no default."""
    if value is None:
        raise ValueError("ubpl_amd: pseudoRule %r needs pseudoSelRate, the share of joints kept, in (0, 1]" % rule)
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not 0.0 < value <= 1.0:
        raise ValueError("ubpl_amd: pseudoSelRate is a float in (0, 1], got %r" % (value,))
    return float(value)


class GateOptions:
    """The rule's options read from a step's args, checked on the host: every existing namespace
    (none of the attributes) is the score rule on each view's own targets, `on` and `cross` False.
    `on` is the view-consistency gate; the "rate" rule (sel_rate not None) selects by rank instead
    and is not combined with it; `cross` is cross-view targets (views "merged" or "other")."""

    def __init__(self, args):
        self.rule = getattr(args, "pseudoRule", "score")
        if self.rule not in RULES:
            raise ValueError("ubpl_amd: pseudoRule is one of %s, got %r" % (", ".join(RULES), self.rule))
        self.views = getattr(args, "pseudoViews", "own")
        if self.views not in VIEWS:
            raise ValueError("ubpl_amd: pseudoViews is one of %s, got %r" % (", ".join(VIEWS), self.views))
        self.cross = self.views != "own"
        self.sel_rate = None                                 # the "rate" rule's share of joints kept
        if self.rule == "rate":
            self.sel_rate = check_sel_rate(self.rule, getattr(args, "pseudoSelRate", None))
        self.on = self.rule not in ("score", "rate")
        if not self.on:
            return
        # the reference's name, and like the reference no default (predict_args.check_dist_thr)
        if getattr(args, "distThrMax", None) is None:
            raise ValueError("ubpl_amd: pseudoRule %r needs distThrMax, a distance >= 0 in source-image pixels"
                             % self.rule)
        self.dist_thr = PA.check_dist_thr("uncertainty", args.distThrMax, True)
        self.refine, self.taps = PA.check_refine(getattr(args, "pseudoRefine", "taylor"),
                                                 getattr(args, "pseudoBlurSigma", PA.DEFAULT_BLUR_SIGMA))
        # the score tests stay beside the gate only in "score+uncertainty"
        self.thr = float(args.pseudoScoreThr) if self.rule == "score+uncertainty" else float("-inf")
        self._consts = {}                                    # device -> (dist_thr, taps), see constants()


_OPTIONS = {}


def options(args):
    """GateOptions(args), built once per distinct set of option values: the step and its record
    line ask every batch, and the checks (blur_taps, a host tensor) need not run again.
    Entries are never evicted.  That is what keeps a captured step valid: its graph bakes in the
    addresses of the device constants an entry owns (constants()), and nothing but this table
    keeps them alive.  An entry is a few floats, one per option set a process ever trains with."""
    key = (getattr(args, "pseudoRule", "score"), getattr(args, "distThrMax", None),
           getattr(args, "pseudoRefine", None), getattr(args, "pseudoBlurSigma", None),
           getattr(args, "pseudoScoreThr", None), getattr(args, "pseudoSelRate", None),
           getattr(args, "pseudoViews", "own"))
    try:
        opts = _OPTIONS.get(key)
    except TypeError:                                        # an unhashable value: let the checks name it
        return GateOptions(args)
    if opts is None:
        opts = _OPTIONS[key] = GateOptions(args)
    return opts


def refuse(args, where):
    """The steps the rule and the cross-view targets are not wired into say so instead of ignoring
    the option."""
    opts = options(args)
    if opts.cross:
        raise ValueError("ubpl_amd: pseudoViews %r is built into train_mt_ubpl only, not %s" % (opts.views, where))
    if opts.on or opts.sel_rate is not None:
        raise ValueError("ubpl_amd: pseudoRule %r is built into train_mt_ubpl only, not %s"
                         % (args.pseudoRule, where))


def check_batch(opts, meta, A, M):
    """The rule and the cross-view targets against a batch, before any launch: each needs the views'
    matrices and two views."""
    for on, what, does in ((opts.on, "pseudoRule %r" % opts.rule, "compares"),
                           (opts.cross, "pseudoViews %r" % opts.views, "merges")):
        if not on:
            continue
        if A < 2:
            raise ValueError("ubpl_amd: %s %s a sample's augmented views: at least 2, got %d" % (what, does, A))
        if A > Kn.MAX_VIEWS or not 1 <= M <= 8:
            raise ValueError("ubpl_amd: %s takes at most %d views and 8 teachers, got %d and %d"
                             % (what, Kn.MAX_VIEWS, A, M))
        vm = meta.get("viewmat") if isinstance(meta, dict) else None
        if vm is None or len(vm) != A:
            raise ValueError('ubpl_amd: %s needs meta["viewmat"]: one [B,6] float32 matrix table per view '
                             "(DeviceAugment.views(with_mats=True))" % what)


def constants(opts, dev):
    """(dist_thr float32 [1], taps float32 [radius + 1] or None) on the device, made once per
    options object and device and owned by it: host -> device copies cannot be captured, so
    train_mt_ubpl asks for them before its first step and the captured step finds them here.  The
    graph reads them at these addresses at every replay, so they live as long as `opts` does —
    for options(args)' entries, as long as the process (see there)."""
    key = str(dev)
    if key not in opts._consts:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ubpl_amd: the view-gate constants are made before the step is captured")
        opts._consts[key] = (torch.tensor([opts.dist_thr], dtype=torch.float32, device=dev),
                             None if opts.taps is None else opts.taps.to(dev))
    return opts._consts[key]


def view_gate(opts, tgs, viewmat, R):
    """gate [B,K] float32 of one step.  tgs: per view the stacked teacher outputs [M,B,S,K,H,W]
    (contiguous); viewmat: per view a device float32 [B,6]; R: the views' input side.
    Two launches per view (the strided plain decode of all teachers' last stacks, M*B samples of
    batch stride S*K*H*W, and its refinement) and one ubpl_view_uncertainty_samples; the back
    matrices are a handful of elementwise tensor ops.  No host synchronisation."""
    A = len(tgs)
    M, B, S, K, H, W = tgs[0].shape
    dev = tgs[0].device
    dist_thr, taps = constants(opts, dev)
    back = Kn.train_back_matrices([v.to(dev, non_blocking=True).float().reshape(B, 6) for v in viewmat], R, H)
    peaks = torch.empty((A, M, B, K, 2), device=dev, dtype=torch.float32)
    sub = torch.empty_like(peaks) if opts.refine != "none" else peaks
    sb = S * K * H * W
    for a in range(A):
        hm = tgs[a].reshape(-1)[(S - 1) * K * H * W:]           # the last stacks, in place
        Kn.decode_heatmaps_flip(hm, None, sb, M * B, K, H, W, out=(peaks[a].view(M * B, K, 2), None, None, None))
        if opts.refine != "none":
            Kn.refine_peaks(hm, None, sb, M * B, K, H, W, None, peaks[a].view(M * B, K, 2), opts.refine, taps,
                            out=(sub[a].view(M * B, K, 2), None, None))
    select = torch.empty((M, B, K), device=dev, dtype=torch.float32)
    gate = torch.empty((B, K), device=dev, dtype=torch.float32)
    Kn.view_uncertainty_samples(sub.view(-1), B * K * 2, M * B * K * 2, M, A, B, K, back, dist_thr,
                                out=(None,) * 9 + (select, gate))
    return gate


def cross_view_targets(opts, last, viewmat, R):
    """The pseudo loss' targets of every view under args.pseudoViews "merged" / "other".  last: the
    teachers' last stacks of every view, [A,M,B,K,H,W] contiguous; viewmat: per view a device float32
    [B,6]; R: the views' input side.  -> xt [A,M,B,K,H,W]: xt[a] is every teacher's maps of all views
    (without view a's own under "other") warped into view a's frame and averaged over the views that
    cover each cell.  One ubpl_merge_views_samples launch; the pair matrices are a handful of
    elementwise tensor ops.  No host synchronisation."""
    A, M, B, K, H, W = last.shape
    dev = last.device
    pair = Kn.train_pair_matrices([v.to(dev, non_blocking=True).float().reshape(B, 6) for v in viewmat], R, H)
    blk = K * H * W
    xt, _ = Kn.merge_views_samples(last.view(-1), M * B * blk, B * blk, blk, A, M, B, K, H, W, pair,
                                   include_self=opts.views == "merged")
    return xt
