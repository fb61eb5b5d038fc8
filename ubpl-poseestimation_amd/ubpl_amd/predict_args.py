"""The Predictor's argument checks (ubpl_amd/predict.py): host only, nothing here touches a device."""
import math

import torch

from . import kernels as Kn

DEFAULT_BLUR_SIGMA = 1.0
RULES = ("unanimous", "ensemble", "uncertainty")
REFINES = ("none", "quarter", "taylor")


def view_count(views, flip_test):
    """The views of one forward batch, mirrored ones included; 0 for tta=None."""
    return 0 if views is None else len(views) * (2 if flip_test else 1)


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
    V = view_count(views, flip_test)
    if V > Kn.MAX_VIEWS:
        raise ValueError("ubpl_amd: %d tta views%s make %d, at most %d"
                         % (len(views), " with their mirrors" if flip_test else "", V, Kn.MAX_VIEWS))
    return views


def check_uncertainty(uncertainty, views, flip_test):
    """The uncertainty argument against the checked tta views -> bool.  View consistency needs
    views to compare: tta with at least 2 in all (mirrored ones included)."""
    if not uncertainty:
        return False
    V = view_count(views, flip_test)
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
