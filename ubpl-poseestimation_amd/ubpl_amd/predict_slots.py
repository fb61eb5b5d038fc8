"""The Predictor's static side (ubpl_amd/predict.py): what one captured graph is made for (the slot
spec), its static buffers (one table), the least-recently-used cache of slots, capture-or-replay,
and what a result is made of (one table: key, source, sample axis, conditions).

A new result key is one row of SCHEMA — and, when it is read from a buffer of its own, one entry of
BUFFERS; its sample axis is declared in that row, and chunk concatenation and label_pool read it
from there."""
from collections import OrderedDict, namedtuple

import torch

from .predict_args import assemble_kps


class SlotSpec(namedtuple("SlotSpec", "M K flip views refine unc pseudo N R want_hm have_tinv")):
    """What a slot is built for, and its key in the cache: the Predictor's constants (M networks,
    K joints, flip test, views = the view count of tta or None, refine on, uncertainty on) and the
    call's (pseudo_label or predict, N images of R x R, heatmaps kept, tinv given).  Normalised, so
    that equal specs share a slot: pseudo_label and tta always keep the (merged) heatmaps, and
    have_tinv (heatmap cells or image coordinates) is None unless uncertainty is on."""
    __slots__ = ()

    def __new__(cls, M, K, flip, views, refine, unc, pseudo, N, R, want_hm, have_tinv):
        return super().__new__(cls, M, K, flip, views, refine, unc, pseudo, N, R,
                               bool(want_hm or pseudo or views is not None), bool(have_tinv) if unc else None)

    def on(self, fields):
        """An option group is on: every field it names is set (none: always)."""
        return all(getattr(self, f) for f in fields)


# option group -> buffer -> shape, one letter per axis: the spec's M N K R V (= views), H = W = R // 4,
# B = the forward batch's rows, a digit = itself.  float32 but for tinv.  No other buffer exists.
BUFFERS = (
    ((), dict(batch="B3RR", tinv="N6", raw="MNK2", preds="MNK2", scores="MNK", mean="NK2")),
    (("want_hm",), dict(heatmaps="MNKHW")),
    (("refine",), dict(raw_sub="MNK2", preds_sub="MNK2", rule="MNK", mean_sub="NK2")),
    # every view's own peaks (view-major, as the batch) and their fold
    (("unc",), dict(raw_views="MBK2", scores_views="MBK", dist_thr="1", view_preds="MVNK2", aug_coord="MNK2",
                    view_legal="MNK", int_dist="MNK", mix_dist="MNK", unc_value="MNK", unc_select="MNK",
                    ext_dist="NK", aext_dist="NK", ext_views="NK")),
    (("unc", "refine"), dict(raw_views_sub="MBK2")),
    # the ensemble kernel's outputs and its threshold
    (("pseudo",), dict(thr="1", ens_raw="NK2", ens_preds="NK2", ens_score="NK", disagree="MNK", select="MNK",
                       spread="NK", mean_hm="NKHW")),
    (("pseudo", "refine"), dict(ens_raw_sub="NK2", ens_preds_sub="NK2", ens_rule="NK")),
)


class Slot:
    """The static buffers of one spec and, once captured, the graph that maps its inputs (imgs,
    tinv, thr, dist_thr) to its outputs."""

    def __init__(self, spec, dev):
        self.spec, self.N, self.H, self.W = spec, spec.N, spec.R // 4, spec.R // 4
        self.refine, self.unc = spec.refine, spec.unc
        rows = spec.N * (spec.views if spec.views is not None else 2 if spec.flip else 1)     # view-major with tta
        dim = dict(M=spec.M, N=spec.N, K=spec.K, R=spec.R, V=spec.views, H=self.H, W=self.W, B=rows)
        for fields, table in BUFFERS:
            if spec.on(fields):
                for name, shape in table.items():
                    setattr(self, name, torch.zeros([int(a) if a.isdigit() else dim[a] for a in shape], device=dev,
                                                    dtype=torch.float64 if name == "tinv" else torch.float32))
        self.imgs = self.batch[:spec.N]
        self.schema = tuple(row for row in SCHEMA if spec.on(row.group))
        self.graph = None

    def release(self):
        if self.graph is not None:
            self.graph.reset()
            self.graph = None


class SlotCache(OrderedDict):
    """spec -> Slot, least recently used first."""

    def fetch(self, spec, limit, dev):
        """-> (the slot of spec, whether it is new); at most `limit` are kept."""
        s = self.get(spec)
        if s is not None:
            self.move_to_end(spec)
            return s, False
        while len(self) >= limit:
            _, old = self.popitem(last=False)
            old.release()
            del old
            torch.cuda.empty_cache()
        s = self[spec] = Slot(spec, dev)
        return s, True


def launch(s, new, run, use_graph):
    """run(s) eagerly, or captured once per slot and replayed."""
    if not use_graph:
        run(s)
        return
    if new:
        # warm-up: the networks' per-batch-size scratch is allocated here, outside the
        # graph's pool; then the capture (which records, it does not execute)
        run(s)
        torch.cuda.synchronize(s.batch.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            run(s)
        s.graph = g
    s.graph.replay()


# ---- the result ------------------------------------------------------------
# What a call asked for: center / scale given, return_heatmaps, pseudo_label's dist_thr and rule, and
# the Predictor's joint permutation (device int32 [K] or None).
Ask = namedtuple("Ask", "have want_hm dist_thr rule perm", defaults=(None, None, None))


def _positive(name):
    return lambda s, ask, out: getattr(s, name) > 0                 # a 0/1 float buffer -> bool


def _view_scores(s, ask, out):
    c = s.spec
    scores = s.scores_views.reshape(c.M, c.views, c.N, c.K).clone()
    if c.flip and ask.perm is not None:                             # the mirrored views, in the output joint order
        scores[:, c.views // 2:] = scores[:, c.views // 2:][..., ask.perm.long()]
    return scores


def _selected(s, ask, out):
    if ask.rule == "uncertainty":
        return (s.unc_select > 0).all(0)
    return out["member_select"].all(0) if ask.rule == "unanimous" else s.ens_score >= s.thr


def _kps(name):
    return lambda s, ask, out: assemble_kps(getattr(s, name), out["selected"])


TINV, HM, DT = 1, 2, 4      # None without center / scale; only with return_heatmaps; only with dist_thr
Row = namedtuple("Row", "key source axis group flags")
_P, _R, _PR, _U = ("pseudo",), ("refine",), ("pseudo", "refine"), ("unc",)
# In the result's key order.  source: the slot buffer to clone, or f(slot, ask, the result so far);
# axis: the sample axis ([N,...], [M,N,...] or [M,V,N,...]); group: as in BUFFERS.
SCHEMA = tuple(Row(*r) for r in (
    ("raw", "raw", 1, (), 0), ("scores", "scores", 1, (), 0), ("preds", "preds", 1, (), TINV),
    ("preds_mean", "mean", 0, (), TINV),
    ("ens_raw", "ens_raw", 0, _P, 0), ("ens_preds", "ens_preds", 0, _P, TINV), ("ens_score", "ens_score", 0, _P, 0),
    ("member_select", _positive("select"), 1, _P, 0), ("disagree", "disagree", 1, _P, 0),
    ("selected", _selected, 0, _P, 0), ("spread", "spread", 0, _P, 0), ("kps", _kps("ens_preds"), 0, _P, TINV),
    ("raw_sub", "raw_sub", 1, _R, 0), ("preds_sub", "preds_sub", 1, _R, TINV),
    ("preds_mean_sub", "mean_sub", 0, _R, TINV), ("refine_rule", "rule", 1, _R, 0),
    ("ens_raw_sub", "ens_raw_sub", 0, _PR, 0), ("ens_preds_sub", "ens_preds_sub", 0, _PR, TINV),
    ("ens_refine_rule", "ens_rule", 0, _PR, 0), ("kps_sub", _kps("ens_preds_sub"), 0, _PR, TINV),
    ("view_preds", "view_preds", 2, _U, 0), ("view_scores", _view_scores, 2, _U, 0),
    ("view_legal", _positive("view_legal"), 1, _U, 0), ("int_dist", "int_dist", 1, _U, 0),
    ("aug_coord", "aug_coord", 1, _U, 0), ("ext_dist", "ext_dist", 0, _U, 0), ("aext_dist", "aext_dist", 0, _U, 0),
    ("ext_views", "ext_views", 0, _U, 0), ("mix_dist", "mix_dist", 1, _U, 0), ("unc", "unc_value", 1, _U, 0),
    ("unc_select", _positive("unc_select"), 1, ("unc", "pseudo"), DT),
    ("heatmaps", "heatmaps", 1, ("want_hm",), HM), ("mean_heatmap", "mean_hm", 0, _P, HM)))
AXIS = {row.key: row.axis for row in SCHEMA}


def result(s, ask):
    """The result dict of one chunk, the caller's own: the slot's schema rows that `ask` admits."""
    out = {}
    for key, source, _, _, flags in s.schema:
        if (flags & HM and not ask.want_hm) or (flags & DT and ask.dist_thr is None):
            continue
        none = flags & TINV and not ask.have
        out[key] = None if none else getattr(s, source).clone() if isinstance(source, str) else source(s, ask, out)
    return out


def concat(outs):
    """The chunks' results as one: every key along its sample axis."""
    if len(outs) == 1:
        return outs[0]
    return {k: None if v is None else torch.cat([o[k] for o in outs], AXIS[k]) for k, v in outs[0].items()}
