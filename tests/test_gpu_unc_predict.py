"""Predictor(uncertainty=True): the per-view peaks are those of a plain Predictor run on the warped
views, mapped back on the host; the fold is the restatement's (tests/unc_ref.py); graph and eager
agree; one graph serves every dist_thr; chunks concatenate; one network works; and
uncertainty=False is the Predictor of before.  The networks, images and helpers of
tests/test_gpu_tta_predict.py (k = 9, one stack, 128^2)."""
import numpy as np
import pytest
import torch

import unc_ref as UR
from test_gpu_tta_predict import DEV, K, PAIRS, RES, VIEWS3, _cs, _eq, _imgs, _models, _same

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
UNC_KEYS = ("view_preds", "view_scores", "view_legal", "int_dist", "aug_coord", "ext_dist", "aext_dist", "ext_views",
            "mix_dist", "unc")


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _geometry(flip):
    from ubpl_amd import kernels as Kn
    img_mat, hm_mat, swap = Kn.view_matrices(VIEWS3, flip, RES, RES // 4)
    perm = Kn.flip_perm(K, PAIRS).numpy() if flip else None
    return img_mat, hm_mat, swap.numpy() if flip else None, perm


def _map_back64(raw, hm_mat, swap, perm, tinv):
    """raw [M,V,N,K,2] (each view's own frame and joint order) -> the points in the original
    frame, output joint order, all in float64 with the exact inverse of each (float32) hm_mat."""
    M, V, N, _, _ = raw.shape
    out = np.empty(raw.shape, np.float64)
    for v in range(V):
        fwd = np.vstack([hm_mat[v].double().numpy().reshape(2, 3), [0.0, 0.0, 1.0]])
        inv = np.linalg.inv(fwd)[:2]
        r = raw[:, v].astype(np.float64)
        if swap is not None and swap[v] and perm is not None:
            r = r[:, :, perm]
        o = (r - 1.0) @ inv[:, :2].T + inv[:, 2]
        if tinv is None:
            out[:, v] = o + 1.0
        else:
            t = tinv.reshape(N, 2, 3)
            out[:, v] = np.einsum("nij,mnkj->mnki", t[:, :, :2], o) + t[None, :, None, :, 2] + 1.0
    return out


def _view_scores(scores, swap, perm):
    s = scores.copy()
    for v in range(s.shape[1]):
        if swap is not None and swap[v] and perm is not None:
            s[:, v] = s[:, v][..., perm]
    return s


def _plain_views(models, x, flip, refine):
    """The warped views through a plain Predictor (no tta, no flip test), as one batch of V*N images
    (the batch size of the views' own forward) -> host (raw or raw_sub [M,V,N,K,2], scores [M,V,N,K])."""
    from ubpl_amd import Predictor, kernels as Kn
    img_mat = _geometry(flip)[0]
    V, N, M = len(img_mat), x.shape[0], len(models)
    views = Kn.warp_views(x, img_mat.to(DEV)).reshape(V * N, 3, RES, RES)
    plain = Predictor(models, refine=refine, max_batch=V * N)
    out = plain.predict(views)
    plain.release()
    raw = out["raw" if refine == "none" else "raw_sub"].cpu().numpy().reshape(M, V, N, K, 2)
    return raw, out["scores"].cpu().numpy().reshape(M, V, N, K)


def _check_fold(out, raw, hm_mat, swap, perm, tinv, dist_thr=1.0):
    """The result's uncertainty keys against the float32 restatement fed the plain per-view peaks:
    equal bits, unc within 2^-22.  -> the restatement's outputs."""
    from ubpl_amd import kernels as Kn
    want = UR.view_uncertainty(raw, Kn.view_back_matrices(hm_mat).numpy(), dist_thr, swap, perm, tinv)
    names = {"view_preds": "pts", "view_legal": "legal", "unc_select": "select"}
    for key in UNC_KEYS + (("unc_select",) if "unc_select" in out else ()):
        if key in ("unc", "view_scores"):
            continue
        got = out[key].float().cpu().numpy()
        assert np.array_equal(got, want[names.get(key, key)], equal_nan=True), key
    assert np.abs(out["unc"].cpu().numpy().astype(np.float64) - want["unc"]).max() <= 2.0 ** -22
    return want


@pytest.mark.parametrize("refine", ["none", "taylor"])
@pytest.mark.parametrize("flip", [False, True])
def test_view_preds_are_the_plain_predictions_of_the_views(flip, refine):
    from ubpl_amd import Predictor
    from ubpl_amd.process import inverse_transforms
    models = _models()
    kw = dict(tta=VIEWS3, flip_test=flip, flip_pairs=PAIRS if flip else None, refine=refine, uncertainty=True)
    Pg, Pe = Predictor(models, graph=True, **kw), Predictor(models, graph=False, **kw)
    _, hm_mat, swap, perm = _geometry(flip)
    M, V, N = 2, len(hm_mat), 2
    x = _imgs(N, torch.Generator().manual_seed(61))
    center, scale = _cs(N)
    raw, scores = _plain_views(models, x, flip, refine)
    if refine == "taylor":
        assert (raw != np.round(raw)).any()                          # sub-pixel peaks went in
    tinv = inverse_transforms(center, scale, [RES // 4, RES // 4]).numpy()
    for c, s, t in ((center, scale, tinv), (None, None, None)):     # image coordinates; heatmap cells
        g = Pg.predict(x, c, s)
        _same(g, Pe.predict(x, c, s))                               # graph and eager: equal bits
        assert [k for k in g if k in UNC_KEYS] == list(UNC_KEYS) and "unc_select" not in g
        assert g["view_preds"].shape == (M, V, N, K, 2) and g["view_scores"].shape == (M, V, N, K)
        assert g["view_legal"].dtype == torch.bool and g["view_legal"].shape == g["unc"].shape == (M, N, K)
        assert g["aug_coord"].shape == (M, N, K, 2) and g["ext_views"].shape == g["ext_dist"].shape == (N, K)
        want64 = _map_back64(raw, hm_mat, swap, perm, t)
        bar = 16 * U * np.abs(want64).max()
        err = np.abs(g["view_preds"].cpu().numpy() - want64).max()
        print("flip", flip, refine, "image" if t is not None else "cells", "err %.3g bar %.3g" % (err, bar))
        assert err <= bar
        assert np.array_equal(g["view_scores"].cpu().numpy(), _view_scores(scores, swap, perm))
        want = _check_fold(g, raw, hm_mat, swap, perm, t)
        assert want["legal"].any()
        # view 0 is the image itself: its point is the view's own peak, moved by nothing
        if t is None:
            assert np.array_equal(g["view_preds"][:, 0].cpu().numpy(), raw[:, 0])
    assert len(Pg._slots) == 2                                      # one per coordinate system
    Pg.release()
    Pe.release()


def test_one_graph_serves_every_dist_thr():
    from ubpl_amd import Predictor
    from ubpl_amd.predict import assemble_kps
    from ubpl_amd.process import inverse_transforms
    models = _models()
    P = Predictor(models, tta=VIEWS3, uncertainty=True)
    _, hm_mat, swap, perm = _geometry(False)
    x = _imgs(3, torch.Generator().manual_seed(62))
    center, scale = _cs(3)
    raw, _ = _plain_views(models, x, False, "none")
    tinv = inverse_transforms(center, scale, [RES // 4, RES // 4]).numpy()
    first = P.pseudo_label(x, center, scale, thr=0.1)
    assert "unc_select" not in first and len(P._slots) == 1
    base = _check_fold(first, raw, hm_mat, swap, perm, tinv)
    thrs = UR.thresholds_between(base)
    kept = []
    for t in thrs:
        out = P.pseudo_label(x, center, scale, thr=0.1, rule="uncertainty", dist_thr=t)
        want = _check_fold(out, raw, hm_mat, swap, perm, tinv, t)
        assert out["unc_select"].dtype == torch.bool
        assert np.array_equal(out["selected"].cpu().numpy(), want["select"].all(0))
        assert _eq(out["kps"], assemble_kps(out["ens_preds"], out["selected"]))
        for key in first:                                           # nothing else moves with the threshold
            if key not in ("selected", "kps"):
                assert _eq(out[key], first[key]), key
        kept.append(int(want["select"].all(0).sum()))
    print("dist_thr", thrs, "kept", kept)
    assert kept[0] < kept[-1] and len(P._slots) == 1 and next(iter(P._slots.values())).graph is not None
    # the other rules still answer, and may ask for unc_select beside theirs
    both = P.pseudo_label(x, center, scale, thr=0.1, rule="unanimous", dist_thr=thrs[-1])
    assert _eq(both["selected"], first["selected"]) and _eq(both["unc_select"], out["unc_select"])
    with pytest.raises(ValueError, match="needs dist_thr"):
        P.pseudo_label(x, center, scale, rule="uncertainty")
    with pytest.raises(ValueError, match="uncertainty=True"):
        Predictor(models, tta=VIEWS3).pseudo_label(x, center, scale, rule="uncertainty", dist_thr=3.0)
    P.release()


def test_chunks_concatenate_on_the_right_axes():
    """As tests/test_gpu_tta_predict.py: chunked equals the unchunked calls on pieces of equal size."""
    from ubpl_amd import Predictor
    models = _models()
    x = _imgs(5, torch.Generator().manual_seed(63))
    center, scale = _cs(5)
    kw = dict(tta=VIEWS3, refine="quarter", uncertainty=True)
    whole, chunked = Predictor(models, **kw), Predictor(models, max_batch=3, **kw)     # 2 * 3 // 3 = 2 per chunk
    assert chunked.max_batch == 2
    axis = {"view_preds": 2, "view_scores": 2, "preds_mean": 0, "preds_mean_sub": 0, "ext_dist": 0, "aext_dist": 0,
            "ext_views": 0}
    for name, kwargs in (("predict", {}), ("pseudo_label", {"rule": "uncertainty", "dist_thr": 6.0, "thr": 0.1})):
        out = getattr(chunked, name)(x, center, scale, **kwargs)
        parts = [getattr(whole, name)(x[a:b], center[a:b], scale[a:b], **kwargs) for a, b in ((0, 2), (2, 4), (4, 5))]
        per_member = ("raw", "scores", "preds", "member_select", "disagree", "heatmaps", "raw_sub", "preds_sub",
                      "refine_rule", "view_legal", "int_dist", "aug_coord", "mix_dist", "unc", "unc_select")
        for key in out:
            ax = axis.get(key, 1 if key in per_member else 0)
            assert _eq(out[key], torch.cat([p[key] for p in parts], ax)), (name, key)
        assert out["view_preds"].shape == (2, 3, 5, K, 2) and out["int_dist"].shape == (2, 5, K)
        assert out["ext_dist"].shape == (5, K)
    whole.release()
    chunked.release()


def test_uncertainty_off_is_the_predictor_of_before(monkeypatch):
    from ubpl_amd import Predictor, _lib
    x = _imgs(2, torch.Generator().manual_seed(64))
    center, scale = _cs(2)
    kw = dict(tta=VIEWS3, flip_test=True, flip_pairs=PAIRS, refine="taylor")
    old, off, on = Predictor(_models(), **kw), Predictor(_models(), uncertainty=False, **kw), \
        Predictor(_models(), uncertainty=True, **kw)
    for call in (lambda P: P.predict(x, center, scale, return_heatmaps=True), lambda P: P.predict(x),
                 lambda P: P.pseudo_label(x, center, scale, thr=0.1, return_heatmaps=True)):
        a, b, c = call(old), call(off), call(on)
        _same(a, b)
        assert [k for k in c if k not in UNC_KEYS] == list(a)       # the option only adds
        for key in a:
            assert _eq(a[key], c[key]), key
    assert list(off._slots) == list(old._slots) and not hasattr(off, "_back_mats")
    assert not any(hasattr(s, "raw_views") or s.unc for s in off._slots.values())
    for P in (old, off, on):
        P.release()
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    Predictor(_models(), graph=False, **kw).predict(x)
    before = list(names)
    names.clear()
    Predictor(_models(), graph=False, uncertainty=False, **kw).predict(x)
    assert names == before and "ubpl_view_uncertainty" not in names and "ubpl_decode_heatmaps_flip" not in names
    names.clear()
    Predictor(_models(), graph=False, uncertainty=True, **kw).predict(x)
    extra = list(names)
    for n in before:
        extra.remove(n)
    assert sorted(extra) == ["ubpl_decode_heatmaps_flip"] * 2 + ["ubpl_refine_peaks"] * 2 + ["ubpl_view_uncertainty"]


def test_one_network_and_label_pool():
    from ubpl_amd import Predictor
    models = _models()
    gen = torch.Generator().manual_seed(65)
    center, scale = _cs(2)
    x = torch.rand(2, 3, RES, RES, generator=gen) - 0.5
    P = Predictor(models[0], tta=[(0, 1)], flip_test=True, flip_pairs=PAIRS, uncertainty=True)     # the image and its mirror
    out = P.pseudo_label(x, center, scale, thr=0.1, rule="uncertainty", dist_thr=8.0)
    assert out["view_preds"].shape == (1, 2, 2, K, 2) and out["unc_select"].shape == (1, 2, K)
    for key in ("ext_dist", "aext_dist", "ext_views"):
        assert not out[key].any()                                   # one member: no pair
    legal = out["view_legal"]
    assert legal.any() and _eq(out["mix_dist"][legal], out["int_dist"][legal])
    assert _eq(out["selected"], (legal & (out["int_dist"] <= 8.0))[0])
    P.release()
    loader = [(x, None, {"center": center, "scale": scale})]
    P = Predictor(models, tta=VIEWS3, uncertainty=True)
    d = P.label_pool(loader, thr=0.1, rule="uncertainty", dist_thr=8.0)
    out = P.pseudo_label(x, center, scale, thr=0.1, rule="uncertainty", dist_thr=8.0)
    assert d["rule"] == "uncertainty" and d["dist_thr"] == 8.0 and d["selected"] == out["selected"].cpu().tolist()
    assert d["int_dist"] == out["int_dist"].transpose(0, 1).cpu().tolist()
    assert d["unc"] == out["unc"].transpose(0, 1).cpu().tolist()
    assert d["ext_dist"] == out["ext_dist"].cpu().tolist() and d["aext_dist"] == out["aext_dist"].cpu().tolist()
    assert P.label_pool(loader, thr=0.1)["dist_thr"] is None
    assert "dist_thr" not in Predictor(models, tta=VIEWS3).label_pool(loader, thr=0.1)
    P.release()
