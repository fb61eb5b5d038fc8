"""CPU-only checks of the view-consistency uncertainty: the numpy restatement of
ubpl_view_uncertainty (tests/unc_ref.py) against the reference's own pseudo_cal_unc,
coord_avgDistance, pseudo_filter_mixUnc and assess_pseudo_unc2 (tests/golden/unc.npz, made by
tests/golden/gen_unc_golden.py), the back matrices, the argument and rule checks and the ABI entry."""
import os

import numpy as np
import pytest
import torch

import unc_ref as UR

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unc.npz")
U = 2.0 ** -24                                                       # float32's unit roundoff


def _fixture():
    return dict(np.load(FIXTURE))


def _sets(fx, planted=False):
    return sorted(k.split("/")[0] for k in fx if k.endswith("/pts") and k.startswith("3neg") == planted)


def test_float64_restatement_is_the_reference():
    """Same operations on the same float32 points in the same order: 1e-12 relative (the
    reference's x ** 0.5 and math.exp against numpy's sqrt and exp is all the room needed)."""
    fx = _fixture()
    assert os.path.getsize(FIXTURE) < 64 * 1024
    assert _sets(fx) == ["2", "3", "4", "5"]
    close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=0)
    for name in _sets(fx):
        pts = fx[name + "/pts"]
        assert pts.dtype == np.float32 and pts.shape == (2, int(name), 3, 4, 2)
        assert pts.min() >= 0 and pts.max() < 512
        ok = np.ones(pts.shape[:-1], bool)
        thr = float(fx[name + "/thr"])
        out = UR.fold(pts.astype(np.float64), ok, thr, np.float64)
        assert close(out["int_dist"], fx[name + "/avg"]) and close(out["int_dist"], fx[name + "/intDist"])
        assert close(out["int_dist"][0], fx[name + "/intDist1"]) and close(out["int_dist"][1], fx[name + "/intDist2"])
        assert close(out["aug_coord"], fx[name + "/coord_aug"])
        for ours, theirs in (("ext_dist", "extDist"), ("aext_dist", "aExtDist")):
            assert close(out[ours], fx[name + "/" + theirs][0]) and close(out[ours], fx[name + "/" + theirs][1])
        assert close(out["ext_views"], fx[name + "/extViews"])
        assert close(out["mix_dist"], fx[name + "/mixDist"]) and close(out["unc"], fx[name + "/unc"])
        # the filter: decided on the distance here, on unc there
        assert np.array_equal(out["select"], fx[name + "/enable"])
        assert 0 < fx[name + "/enable"].sum() < fx[name + "/enable"].size, name
        assert out["legal"].all()


def test_legality_is_the_reference_rule():
    """Two planted negative coordinates: a member with one illegal view and a member whose
    view-0 point is illegal make the joint's pair illegal (extDist 999, intDist 999)."""
    fx = _fixture()
    pts = fx["3neg/pts"]
    ok = (pts >= 0).all(-1)
    out = UR.fold(pts.astype(np.float64), ok, 1.0, np.float64)
    pair = out["legal"].all(0) > 0
    assert pair.sum() == pair.size - 2
    assert np.array_equal(fx["3neg/extViews"] == 999, ~pair)
    assert np.allclose(np.where(pair, out["ext_views"], 999), fx["3neg/extViews"], rtol=1e-12, atol=0)
    for m, key in enumerate(("intDist1", "intDist2")):
        assert np.allclose(np.where(pair, out["int_dist"][m], 999), fx["3neg/" + key], rtol=1e-12, atol=0)
    # here a member stands for itself: the one without a planted point keeps its own distance
    assert (out["int_dist"] == 999).sum() == 2 and (out["ext_dist"] == 999).sum() == 2
    assert np.array_equal(out["aug_coord"][out["legal"] == 0], [[-1.0, -1.0]] * 2)
    assert (out["unc"][out["legal"] == 0] == 999).all() and not out["select"][out["legal"] == 0].any()


def test_float32_restatement_within_its_rounding():
    """Every float32 distance lies within 16 u C of the float64 one, u = 2^-24, C = max |coord|.
    Points are float32 in both, so with |dx|, |dy| <= C and d <= sqrt(2) C:
      d = sqrt(dx dx + dy dy): the difference (u), the squares (u each, on top), the sum (u), halved
        by the root, and the root (u): 3 u relative, 3 sqrt(2) u C < 4.3 u C;
      the mean of P = V (V - 1) / 2 <= 10 of them: a sequential sum's additions round by u times a
        partial sum <= j sqrt(2) C, together u sqrt(2) C P (P + 1) / 2, divided by P: 5.5 sqrt(2) u C
        < 7.8 u C; the division: u d < 1.5 u C.  int_dist, ext_views: < 13.6 u C;
      aug_coord: additions round by u j C, j = 2..V <= 5, together 14 u C, divided by V: 2.8 u C, the
        division u C: 3.8 u C per coordinate; a distance of two such points moves by at most
        sqrt(2) 2 3.8 u C < 10.8 u C, plus its own 4.3 u C: aext_dist < 15.1 u C; ext_dist < 4.3 u C.
    mix_dist sums two of these terms and is held to the same bar."""
    fx = _fixture()
    worst = 0.0
    for name in _sets(fx):
        pts = fx[name + "/pts"]
        ok = np.ones(pts.shape[:-1], bool)
        a, b = UR.fold(pts, ok, 1.0, np.float32), UR.fold(pts.astype(np.float64), ok, 1.0, np.float64)
        bar = 16 * U * float(np.abs(pts).max())
        for key in ("int_dist", "ext_dist", "aext_dist", "ext_views", "mix_dist"):
            assert a[key].dtype == np.float32
            err = float(np.abs(a[key].astype(np.float64) - b[key]).max())
            worst = max(worst, err / bar)
            assert err <= bar, (name, key, err, bar)
        assert np.abs(a["unc"].astype(np.float64) - b["unc"]).max() <= 4 * U
    print("worst distance error / bar: %.3f" % worst)


def test_restatement_edges():
    back = np.array([[1, 0, 0, 0, 1, 0], [-1, 0, 7, 0, 1, 0]], np.float32)       # identity, mirror of W = 8
    raw = np.zeros((1, 2, 1, 3, 2), np.float32)
    raw[0, 0, 0] = [[3, 4], [5, 6], [2, 2]]
    raw[0, 1, 0] = [[4, 4], [6, 5], [0, 0]]                       # the mirror's own joint order; joint 2: no peak
    out = UR.view_uncertainty(raw, back, 2.5, swap=[0, 1], perm=[1, 0, 2])
    # joint 0 reads the mirror's joint 1: (6, 5) -> x = 7 - 5 + 1 = 3: distance |(3,4) - (3,5)| = 1
    assert out["pts"][0, 1, 0].tolist() == [[3.0, 5.0], [5.0, 4.0], [9.0, 0.0]]
    assert out["legal"][0, 0].tolist() == [1.0, 1.0, 0.0]
    assert out["int_dist"][0, 0].tolist() == [1.0, 2.0, 999.0] and out["unc"][0, 0, 2] == 999
    assert out["aug_coord"][0, 0].tolist() == [[3.0, 4.5], [5.0, 5.0], [-1.0, -1.0]]
    # one member: no pair, the three pair distances are 0 and mix_dist is int_dist
    assert not out["ext_dist"].any() and not out["aext_dist"].any() and not out["ext_views"].any()
    assert out["mix_dist"][0, 0].tolist() == [1.0, 2.0, 999.0] and out["select"][0, 0].tolist() == [1.0, 1.0, 0.0]
    assert UR.view_uncertainty(raw, back, 1.5, swap=[0, 1], perm=[1, 0, 2])["select"][0, 0].tolist() == [1.0, 0.0, 0.0]
    assert abs(out["unc"][0, 0, 0] - (1 - np.exp(-0.2))) < 1e-7
    # a NaN peak and, with a transform, a negative image coordinate are illegal
    raw[0, 0, 0, 0, 0] = np.nan
    tinv = np.array([[1.0, 0, -4.5, 0, 1.0, 0]])
    out = UR.view_uncertainty(raw, back, 2.5, swap=[0, 1], perm=[1, 0, 2], tinv=tinv)
    assert out["legal"][0, 0].tolist() == [0.0, 1.0, 0.0]
    assert out["pts"][0, 0, 0, 1].tolist() == [0.5, 6.0]          # 1 * 4 + 0 * 5 - 4.5 + 1
    tinv[0, 2] = -5.5
    assert UR.view_uncertainty(raw, back, 2.5, swap=[0, 1], perm=[1, 0, 2], tinv=tinv)["legal"].sum() == 0
    # two members, one of them illegal: no legal pair, the sentinels
    two = np.concatenate([raw, raw], 0)
    two[1, 0, 0, 0, 0] = 3
    out = UR.view_uncertainty(two, back, 10.0, swap=[0, 1], perm=[1, 0, 2])
    assert out["legal"][:, 0].tolist() == [[0.0, 1.0, 0.0], [1.0, 1.0, 0.0]]
    assert out["ext_dist"][0].tolist() == [999.0, 0.0, 999.0] and out["ext_views"][0].tolist() == [999.0, 0.0, 999.0]
    assert out["mix_dist"][1, 0, 0] == 1.0 + 999.0 and out["select"][:, 0].tolist() == [[0.0, 1.0, 0.0], [0.0, 1.0, 0.0]]


@pytest.mark.parametrize("flip", [False, True])
def test_back_matrices_invert_the_heatmap_matrices(flip):
    """back = float32(inverse of hm_mat in float64): every entry is off by at most u times
    itself, so back o hm_mat is off the identity by at most u (|back| o |hm_mat|), entry by entry."""
    from ubpl_amd import kernels as Kn
    views = [(0, 1), (0, 1.25), (20, 0.8), (-35, 2.0), (90, 0.5)]
    _, hm_mat, swap = Kn.view_matrices(views, flip, 256, 64)
    back = Kn.view_back_matrices(hm_mat)
    V = len(views) * (2 if flip else 1)
    assert back.dtype == torch.float32 and back.shape == (V, 6) and back[0].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    got = Kn.compose_pixels(back, hm_mat).numpy()
    room = Kn.compose_pixels(back.abs(), hm_mat.abs()).numpy()
    ident = np.array([1.0, 0, 0, 0, 1.0, 0])
    assert (np.abs(got - ident) <= 1.01 * U * room).all()
    assert np.abs(got - ident).max() > 0                          # (rounded once: not exact)
    if flip:
        assert back[len(views)].tolist() == [-1.0, 0.0, 63.0, 0.0, 1.0, 0.0]
    assert np.array_equal(Kn.view_back_matrices(hm_mat.numpy()).numpy(), back.numpy())
    with pytest.raises(ValueError, match="invertible"):
        Kn.view_back_matrices(torch.tensor([[1.0, 2.0, 0.0, 2.0, 4.0, 0.0]]))


def test_argument_and_rule_checks_raise_without_a_gpu():
    from ubpl_amd import Predictor
    from ubpl_amd import kernels as Kn
    from ubpl_amd import predict as P
    assert P.check_rule("uncertainty") == "uncertainty" and "uncertainty" in P.RULES
    assert P.check_rule("unanimous") == "unanimous" and P.check_rule("ensemble") == "ensemble"
    for bad in ("any", "Uncertainty", None):
        with pytest.raises(ValueError, match="rule is one of"):
            P.check_rule(bad)
    # uncertainty needs views to compare
    for kw in ({}, {"tta": None}, {"tta": [(0, 1)]}):
        with pytest.raises(ValueError, match="at least 2 in all"):
            Predictor(None, uncertainty=True, **kw)
    assert P.check_uncertainty(True, [(0.0, 1.0)], True) is True                   # the image and its mirror
    assert P.check_uncertainty(True, [(0.0, 1.0), (10.0, 1.0)], False) is True
    assert P.check_uncertainty(False, None, False) is False
    # the rule needs the option and a threshold; the threshold needs the option
    with pytest.raises(ValueError, match="needs Predictor\\(uncertainty=True\\)"):
        P.check_dist_thr("uncertainty", 3.0, False)
    with pytest.raises(ValueError, match="needs dist_thr"):
        P.check_dist_thr("uncertainty", None, True)
    with pytest.raises(ValueError, match="dist_thr needs"):
        P.check_dist_thr("unanimous", 3.0, False)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="distance >= 0"):
            P.check_dist_thr("uncertainty", bad, True)
    assert P.check_dist_thr("uncertainty", 3, True) == 3.0 and P.check_dist_thr("ensemble", None, True) is None
    assert P.check_dist_thr("ensemble", 2.5, True) == 2.5 and P.check_dist_thr("unanimous", None, False) is None
    # the wrapper's member and view counts, before anything touches a device
    z = torch.zeros(8)
    for M in (0, 9):
        with pytest.raises(ValueError, match="1 to 8 members"):
            Kn.view_uncertainty(z, 0, M, 2, 1, 1, z, z)
    for V in (1, 17):
        with pytest.raises(ValueError, match="2 to 16 views"):
            Kn.view_uncertainty(z, 0, 1, V, 1, 1, z, z)


def test_header_declares_view_uncertainty():
    from ubpl_amd import _abi, _lib
    decls = {name: (params, ann) for _, name, params, ann in _abi.parse(open(_lib.HEADER_PATH).read())}
    params, ann = decls["ubpl_view_uncertainty"]
    assert [p for _, p in params] == ["raw", "sm", "M", "V", "N", "K", "back", "swap", "perm", "tinv", "dist_thr",
                                      "pts", "legal", "int_dist", "aug_coord", "ext_dist", "aext_dist", "ext_views",
                                      "mix_dist", "unc", "select", "stream"]
    assert ann["raw"] == ("f32", "(M-1)*sm+(int64_t)V*N*K*2") and ann["back"] == ("f32", "V*6")
    assert ann["swap"] == ("i32", "V") and ann["perm"] == ("i32", "K") and ann["tinv"] == ("f64", "N*6")
    assert ann["dist_thr"] == ("f32", "1") and ann["pts"] == ("f32", "(int64_t)M*V*N*K*2")
    assert ann["ext_dist"] == ann["aext_dist"] == ann["ext_views"] == ("f32", "N*K")
    assert ann["select"] == ann["unc"] == ann["legal"] == ("f32", "(int64_t)M*N*K")
    assert "ubpl_view_uncertainty" in _lib.signatures()
