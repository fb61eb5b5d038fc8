"""Host-side checks of the Predictor's layout (no GPU): the slot spec as the cache key, the slot's
buffers and the result schema against literal tables — transcribed from the _Slot / _PseudoSlot /
_predict_chunk / _pseudo_chunk that ubpl_amd/predict_slots.py replaced — and view_count.
Everything at M = 2 networks, N = 2 images, K = 3 joints, R = 16 (4 x 4 heatmaps), V = 3 views."""
import itertools

import pytest
import torch

from ubpl_amd import predict as P
from ubpl_amd import predict_args as A
from ubpl_amd import predict_slots as PS

M, N, K, R, V = 2, 2, 3, 16, 3


def _spec(pseudo=False, want_hm=False, tta=False, unc=False, have_tinv=False, refine=False, flip=False):
    return PS.SlotSpec(M, K, flip, V if tta else None, refine, unc, pseudo, N, R, want_hm, have_tinv)


def _old_key(pseudo, want_hm, tta, unc, have_tinv):
    """The key Predictor._slot() assembled before the spec."""
    key = ("pseudo", N, R) if pseudo else (N, R, want_hm or tta)
    return key + (bool(have_tinv),) if unc else key


# -- spec as key --------------------------------------------------------------
def test_equal_specs_are_the_equal_keys_of_before():
    for tta, unc in ((False, False), (True, False), (True, True)):      # one Predictor's constants
        calls = list(itertools.product((False, True), repeat=3))         # pseudo, want_hm, have_tinv
        for a, b in itertools.product(calls, repeat=2):
            sa, sb = (_spec(c[0], c[1], tta, unc, c[2]) for c in (a, b))
            ka, kb = (_old_key(c[0], c[1], tta, unc, c[2]) for c in (a, b))
            assert (sa == sb) == (ka == kb) and (hash(sa) == hash(sb) or sa != sb), (tta, unc, a, b)
    # pseudo ignores want_hm
    assert _spec(pseudo=True, want_hm=False) == _spec(pseudo=True, want_hm=True)
    assert _spec(pseudo=True, want_hm=False).want_hm is True
    # predict's slots are not pseudo_label's
    assert _spec(pseudo=False, want_hm=True) != _spec(pseudo=True, want_hm=True)
    # without tta predict keeps heatmaps only when asked; tta forces them
    assert _spec(want_hm=False) != _spec(want_hm=True) and _spec(want_hm=False).want_hm is False
    assert _spec(want_hm=False, tta=True) == _spec(want_hm=True, tta=True)
    # have_tinv splits only under uncertainty
    assert _spec(have_tinv=False) == _spec(have_tinv=True) and _spec(have_tinv=True).have_tinv is None
    assert _spec(tta=True, have_tinv=False) == _spec(tta=True, have_tinv=True)
    assert _spec(tta=True, unc=True, have_tinv=False) != _spec(tta=True, unc=True, have_tinv=True)
    assert _spec(tta=True, unc=True, have_tinv=1).have_tinv is True
    assert _spec(pseudo=True, tta=True, unc=True, have_tinv=False) != _spec(pseudo=True, tta=True, unc=True, have_tinv=True)
    every = {_spec(p, h, tta, unc, t) for tta, unc in ((False, False), (True, False), (True, True))
             for p, h, t in itertools.product((False, True), repeat=3)}
    assert len(every) == 3 + 2 + 4


def test_cache_keeps_the_most_recent_and_releases_the_rest():
    class Graph:
        resets = 0

        def reset(self):
            Graph.resets += 1

    cache = PS.SlotCache()
    a, b, c = _spec(), _spec(want_hm=True), _spec(pseudo=True)
    sa, new = cache.fetch(a, 2, "cpu")
    assert new and cache.fetch(a, 2, "cpu") == (sa, False) and sa.graph is None
    sa.graph = Graph()
    cache.fetch(b, 2, "cpu")
    cache.fetch(a, 2, "cpu")                                             # a is the most recent again
    cache.fetch(c, 2, "cpu")
    assert list(cache) == [a, c] and Graph.resets == 0
    cache.fetch(b, 2, "cpu")
    assert list(cache) == [c, b] and Graph.resets == 1 and sa.graph is None


# -- buffers --------------------------------------------------------------------
MNK, NK = (2, 2, 3), (2, 3)
BASE = {"imgs": (2, 3, 16, 16), "tinv": (2, 6), "raw": (2, 2, 3, 2), "preds": (2, 2, 3, 2), "scores": MNK, "mean": (2, 3, 2)}
HEATMAPS = {"heatmaps": (2, 2, 3, 4, 4)}
REFINE = {"raw_sub": (2, 2, 3, 2), "preds_sub": (2, 2, 3, 2), "rule": MNK, "mean_sub": (2, 3, 2)}
UNC = {"raw_views": (2, 6, 3, 2), "scores_views": (2, 6, 3), "dist_thr": (1,), "view_preds": (2, 3, 2, 3, 2),
       "aug_coord": (2, 2, 3, 2), "view_legal": MNK, "int_dist": MNK, "mix_dist": MNK, "unc_value": MNK,
       "unc_select": MNK, "ext_dist": NK, "aext_dist": NK, "ext_views": NK}
UNC_REFINE = {"raw_views_sub": (2, 6, 3, 2)}
PSEUDO = {"thr": (1,), "ens_raw": (2, 3, 2), "ens_preds": (2, 3, 2), "ens_score": NK, "disagree": MNK, "select": MNK,
          "spread": NK, "mean_hm": (2, 3, 4, 4)}
PSEUDO_REFINE = {"ens_raw_sub": (2, 3, 2), "ens_preds_sub": (2, 3, 2), "ens_rule": NK}

# refine, views (None / flip test / tta), uncertainty (None: off; else have_tinv), pseudo, want_hm
COMBOS = [(refine, views, unc, pseudo, want_hm)
          for refine in (False, True) for views, uncs in (("none", (None,)), ("flip", (None,)), ("tta", (None, False, True)))
          for unc in uncs for pseudo in (False, True) for want_hm in (False, True)]


def _combo_spec(refine, views, unc, pseudo, want_hm):
    return _spec(pseudo, want_hm, views == "tta", unc is not None, bool(unc), refine, flip=views == "flip")


@pytest.mark.parametrize("refine,views,unc,pseudo,want_hm", COMBOS)
def test_slot_buffers(refine, views, unc, pseudo, want_hm):
    s = PS.Slot(_combo_spec(refine, views, unc, pseudo, want_hm), "cpu")
    want = dict(BASE, batch=({"none": 2, "flip": 4, "tta": 6}[views], 3, 16, 16))       # N, 2N, V*N rows
    for on, table in ((want_hm or pseudo or views == "tta", HEATMAPS), (refine, REFINE), (unc is not None, UNC),
                      (unc is not None and refine, UNC_REFINE), (pseudo, PSEUDO), (pseudo and refine, PSEUDO_REFINE)):
        if on:
            want.update(table)
    got = {name: tuple(t.shape) for name, t in vars(s).items() if torch.is_tensor(t)}
    assert got == want
    assert all(t.dtype == (torch.float64 if name == "tinv" else torch.float32)
               for name, t in vars(s).items() if torch.is_tensor(t))
    assert s.imgs.data_ptr() == s.batch.data_ptr() and not any(bool(t.any()) for t in vars(s).values() if torch.is_tensor(t))
    assert (s.N, s.H, s.W, s.refine, s.unc, s.graph) == (2, 4, 4, refine, unc is not None, None)
    if unc is None:
        assert not hasattr(s, "raw_views") and not hasattr(s, "dist_thr")
    assert hasattr(s, "raw_views_sub") == (unc is not None and refine)
    s.release()


# -- schema -----------------------------------------------------------------------
K_BASE = ["raw", "scores", "preds", "preds_mean"]
K_ENS = ["ens_raw", "ens_preds", "ens_score", "member_select", "disagree", "selected", "spread", "kps"]
K_SUB = ["raw_sub", "preds_sub", "preds_mean_sub", "refine_rule"]
K_ENS_SUB = ["ens_raw_sub", "ens_preds_sub", "ens_refine_rule", "kps_sub"]
K_UNC = ["view_preds", "view_scores", "view_legal", "int_dist", "aug_coord", "ext_dist", "aext_dist", "ext_views",
         "mix_dist", "unc"]
NONE_WITHOUT_TINV = {"preds", "preds_mean", "ens_preds", "kps", "preds_sub", "preds_mean_sub", "ens_preds_sub", "kps_sub"}
SHAPES = {"raw": (2, 2, 3, 2), "scores": MNK, "preds": (2, 2, 3, 2), "preds_mean": (2, 3, 2), "ens_raw": (2, 3, 2),
          "ens_preds": (2, 3, 2), "ens_score": NK, "member_select": MNK, "disagree": MNK, "selected": NK, "spread": NK,
          "kps": (2, 3, 3), "raw_sub": (2, 2, 3, 2), "preds_sub": (2, 2, 3, 2), "preds_mean_sub": (2, 3, 2),
          "refine_rule": MNK, "ens_raw_sub": (2, 3, 2), "ens_preds_sub": (2, 3, 2), "ens_refine_rule": NK,
          "kps_sub": (2, 3, 3), "view_preds": (2, 3, 2, 3, 2), "view_scores": (2, 3, 2, 3), "view_legal": MNK,
          "int_dist": MNK, "aug_coord": (2, 2, 3, 2), "ext_dist": NK, "aext_dist": NK, "ext_views": NK, "mix_dist": MNK,
          "unc": MNK, "unc_select": MNK, "heatmaps": (2, 2, 3, 4, 4), "mean_heatmap": (2, 3, 4, 4)}
BOOL = {"member_select", "selected", "view_legal", "unc_select"}


@pytest.mark.parametrize("refine,views,unc,pseudo,want_hm", COMBOS)
def test_result_keys_in_order(refine, views, unc, pseudo, want_hm):
    s = PS.Slot(_combo_spec(refine, views, unc, pseudo, want_hm), "cpu")
    perm = torch.tensor([1, 0, 2], dtype=torch.int32)
    haves = (False, True) if unc is None else (bool(unc),)          # (under uncertainty the slot belongs to one)
    for have, dist_thr in itertools.product(haves, (None, 2.0) if pseudo and unc is not None else (None,)):
        want = K_BASE + (K_ENS if pseudo else [])
        if refine:
            want += K_SUB + (K_ENS_SUB if pseudo else [])
        if unc is not None:
            want += K_UNC + (["unc_select"] if dist_thr is not None else [])
        if want_hm:
            want += ["heatmaps"] + (["mean_heatmap"] if pseudo else [])
        for rule in ("unanimous", "ensemble", "uncertainty") if pseudo else (None,):
            if rule == "uncertainty" and dist_thr is None:
                continue
            out = PS.result(s, PS.Ask(have, want_hm, dist_thr, rule, perm))
            assert list(out) == want
            for key, t in out.items():
                if key in NONE_WITHOUT_TINV and not have:
                    assert t is None, key
                    continue
                assert tuple(t.shape) == SHAPES[key] and t.dtype == (torch.bool if key in BOOL else torch.float32), key
                assert all(t.data_ptr() != b.data_ptr() for b in vars(s).values() if torch.is_tensor(b)), key


AXES = {"view_preds": 2, "view_scores": 2,
        "preds_mean": 0, "preds_mean_sub": 0, "ext_dist": 0, "aext_dist": 0, "ext_views": 0,
        "ens_raw": 0, "ens_preds": 0, "ens_score": 0, "ens_raw_sub": 0, "ens_preds_sub": 0, "ens_refine_rule": 0,
        "selected": 0, "spread": 0, "kps": 0, "kps_sub": 0, "mean_heatmap": 0,
        "raw": 1, "scores": 1, "preds": 1, "member_select": 1, "disagree": 1, "heatmaps": 1, "raw_sub": 1, "preds_sub": 1,
        "refine_rule": 1, "view_legal": 1, "int_dist": 1, "aug_coord": 1, "mix_dist": 1, "unc": 1, "unc_select": 1}


def test_every_key_has_its_sample_axis():
    assert PS.AXIS == AXES and [row.key for row in PS.SCHEMA] == list(PS.AXIS) and set(AXES) == set(SHAPES)
    for key, axis in AXES.items():                                   # the axis is the one of length N
        assert SHAPES[key][axis] == N and SHAPES[key][:axis] == ((M, V)[:axis])
    a = {"preds": None, "scores": torch.zeros(2, 2, 3), "ext_dist": torch.zeros(2, 3), "view_scores": torch.zeros(2, 3, 2, 3)}
    b = {"preds": None, "scores": torch.ones(2, 1, 3), "ext_dist": torch.ones(1, 3), "view_scores": torch.ones(2, 3, 1, 3)}
    both = PS.concat([a, b])
    assert list(both) == list(a) and both["preds"] is None and PS.concat([a]) is a
    assert both["scores"].shape == (2, 3, 3) and both["ext_dist"].shape == (3, 3) and both["view_scores"].shape == (2, 3, 3, 3)
    assert bool(both["scores"][:, 2].all()) and bool(both["ext_dist"][2].all()) and bool(both["view_scores"][:, :, 2].all())


def test_view_scores_come_in_the_output_joint_order():
    s = PS.Slot(PS.SlotSpec(M, K, True, 2, False, True, False, N, R, False, False), "cpu")      # the image and its mirror
    s.scores_views.copy_(torch.arange(M * 2 * N * K).reshape(M, 2 * N, K))
    perm = torch.tensor([1, 0, 2], dtype=torch.int32)
    plain = s.scores_views.reshape(M, 2, N, K)
    got = PS.result(s, PS.Ask(False, False, perm=perm))["view_scores"]
    assert torch.equal(got[:, 0], plain[:, 0]) and torch.equal(got[:, 1], plain[:, 1][..., [1, 0, 2]])
    assert torch.equal(PS.result(s, PS.Ask(False, False))["view_scores"], plain)


# -- view_count and the one import ----------------------------------------------------
def test_view_count_and_the_checks_from_both_modules():
    three = [(0, 1), (0, 1.25), (20, 0.8)]
    assert A.view_count(None, False) == 0 and A.view_count(None, True) == 0
    assert A.view_count([(0, 1)], False) == 1 and A.view_count([(0, 1)], True) == 2
    assert A.view_count(three, False) == 3 and A.view_count(three, True) == 6
    for name in ("check_rule", "check_refine", "check_tta", "check_uncertainty", "check_dist_thr", "assemble_kps",
                 "RULES", "REFINES", "DEFAULT_BLUR_SIGMA"):
        assert getattr(P, name) is getattr(A, name), name
    assert P.Predictor.__module__ == "ubpl_amd.predict" and isinstance(P.Predictor.passes, property)
    for mod in (A, P):
        assert mod.check_rule("ensemble") == "ensemble" and mod.check_refine("none", 1.0) == ("none", None)
        assert mod.check_tta(three, True) == [(0.0, 1.0), (0.0, 1.25), (20.0, 0.8)]
        with pytest.raises(ValueError, match="make 18, at most 16"):
            mod.check_tta([(0, 1)] * 9, True)
        assert mod.check_uncertainty(True, [(0.0, 1.0)], True) is True
        with pytest.raises(ValueError, match="at least 2 in all, got 1"):
            mod.check_uncertainty(True, [(0.0, 1.0)], False)
        with pytest.raises(ValueError, match="got tta=None"):
            mod.check_uncertainty(True, None, True)
        assert mod.check_dist_thr("uncertainty", 3, True) == 3.0
