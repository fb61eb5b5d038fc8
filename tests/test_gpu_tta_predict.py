"""Predictor(tta=...): the result is ubpl_warp_views -> the eval forward -> ubpl_decode_heatmaps_views
composed by hand, bit for bit, graph and eager, chunked or not; refine and pseudo_label read the
merged maps; and tta=None is the Predictor of before.  Small networks as in
tests/test_gpu_predict.py (k = 9, one stack, 128^2)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, RES = 9, 128
PAIRS = [(0, 1), (2, 5), (7, 8)]
VIEWS3 = [(0, 1), (0, 1.25), (20, 0.8)]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


_MODELS = {}


def _imgs(n, gen):
    return (torch.rand(n, 3, RES, RES, generator=gen) - 0.5).to(DEV)


def _model(seed):
    """As tests/test_gpu_predict.py builds its networks: statistics and BN affine parameters
    off their initial values.  Built once per seed."""
    from ubpl_amd.hourglass import StackedHourglass
    if seed not in _MODELS:
        torch.manual_seed(seed)
        m = StackedHourglass(K, 1, "AvgPool")
        m.set_conv_precision("2xfp16")
        gen = torch.Generator().manual_seed(100 + seed)
        with torch.no_grad():
            for _ in range(2):
                m(_imgs(2, gen))
            for b in m._bn_names:
                for suffix in (".weight", ".bias"):
                    p = m.P(b + suffix)
                    p.add_((torch.randn(p.shape, generator=gen) * 0.1).to(DEV))
        _MODELS[seed] = m
    return _MODELS[seed]


def _models():
    return [_model(0), _model(1)]


def _eager(m, x):
    """Last-stack heatmaps of the eval forward; the training flag is put back."""
    was = m.training
    with torch.no_grad():
        o = m.eval()(x)[0][:, -1].contiguous()
    m.train(was)
    return o


def _cs(n):
    rs = np.random.RandomState(n + RES)
    center = torch.from_numpy(rs.uniform(0.4, 0.6, (n, 2)) * RES).float()
    scale = torch.from_numpy(rs.uniform(0.9, 1.3, n) * RES / 200.0).float()
    return center, scale


def _eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def _same(a, b):
    assert list(a) == list(b)
    for key in a:
        assert _eq(a[key], b[key]), key


CALLS = (lambda P, x, c, s: P.predict(x, c, s, return_heatmaps=True), lambda P, x, c, s: P.predict(x),
         lambda P, x, c, s: P.pseudo_label(x, c, s, thr=0.1, return_heatmaps=True))


@pytest.mark.parametrize("flip", [False, True])
def test_tta_none_and_the_identity_view_are_the_predictor_of_before(flip, monkeypatch):
    from ubpl_amd import Predictor, _lib
    x = _imgs(3, torch.Generator().manual_seed(41))
    center, scale = _cs(3)
    kw = dict(flip_test=flip, flip_pairs=PAIRS if flip else None, refine="taylor")
    old, none, one = Predictor(_models(), **kw), Predictor(_models(), tta=None, **kw), Predictor(_models(), tta=[(0, 1)], **kw)
    for call in CALLS:
        a = call(old, x, center, scale)
        _same(a, call(none, x, center, scale))
        _same(a, call(one, x, center, scale))
    assert none.tta is None and none.views is None and not hasattr(none, "_view_mats")
    assert list(none._slots) == list(old._slots)
    for P in (old, none, one):
        P.release()
    # tta=None launches what it launched; the views launch their two kernels instead
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    Predictor(_models(), tta=None, graph=False, flip_test=flip).predict(x)
    assert names.count("ubpl_decode_heatmaps_flip") == 2 and names.count("ubpl_fliplr") == int(flip)
    assert "ubpl_warp_views" not in names and "ubpl_decode_heatmaps_views" not in names
    names.clear()
    Predictor(_models(), tta=VIEWS3, graph=False, flip_test=flip).predict(x)
    assert names.count("ubpl_decode_heatmaps_views") == 2 and names.count("ubpl_warp_views") == 1
    assert "ubpl_decode_heatmaps_flip" not in names and "ubpl_fliplr" not in names


@pytest.mark.parametrize("flip", [False, True])
def test_three_views_are_the_manual_composition(flip):
    from ubpl_amd import Predictor, kernels as Kn
    from ubpl_amd.process import inverse_transforms
    models = _models()
    kw = dict(tta=VIEWS3, flip_test=flip, flip_pairs=PAIRS if flip else None)
    Pg, Pe = Predictor(models, graph=True, **kw), Predictor(models, graph=False, **kw)
    V = 6 if flip else 3
    assert Pg.views == V
    img_mat, hm_mat, swap = Kn.view_matrices(VIEWS3, flip, RES, RES // 4)
    perm = Kn.flip_perm(K, PAIRS).to(DEV) if flip else None
    gen = torch.Generator().manual_seed(42)
    for N in (1, 2, 2):                  # the second 2: another input through the same graph
        x = _imgs(N, gen)
        center, scale = _cs(N)
        g = Pg.predict(x, center, scale, return_heatmaps=True)
        e = Pe.predict(x, center, scale, return_heatmaps=True)
        _same(g, e)
        assert set(g) == {"raw", "scores", "preds", "preds_mean", "heatmaps"}
        views = Kn.warp_views(x, img_mat.to(DEV))
        assert _eq(views[0], x)
        tinv = inverse_transforms(center, scale, [RES // 4, RES // 4]).to(DEV)
        H = W = RES // 4
        for mi, m in enumerate(models):
            hm = _eager(m, views.reshape(V * N, 3, RES, RES))
            raw, preds, scores, merged = Kn.decode_heatmaps_views(
                hm.reshape(-1), N * K * H * W, K * H * W, V, N, K, H, W, hm_mat.to(DEV),
                swap.to(DEV) if flip else None, perm, tinv, want_merged=True)
            assert _eq(g["heatmaps"][mi], merged) and _eq(g["raw"][mi], raw)
            assert _eq(g["preds"][mi], preds) and _eq(g["scores"][mi], scores)
            assert not _eq(merged, hm[:N])                           # the other views weigh in
        assert _eq(g["preds_mean"], torch.stack(list(g["preds"]), -1).mean(-1))
        bare = Pg.predict(x)
        assert "heatmaps" not in bare and bare["preds"] is None and _eq(bare["raw"], g["raw"])
    assert len(Pg._slots) == 2 and all(s.graph is not None for s in Pg._slots.values())
    assert all(s.batch.shape[0] == V * s.N for s in Pg._slots.values())
    Pg.release()
    Pe.release()


def test_chunks_shrink_with_the_views_and_concatenate():
    """Chunked equals the unchunked calls on the same pieces (the forward's conv plans may differ
    between batch sizes, so pieces are compared at equal sizes, as tests/test_gpu_predict.py does)."""
    from ubpl_amd import Predictor
    models = _models()
    x = _imgs(5, torch.Generator().manual_seed(43))
    center, scale = _cs(5)
    whole = Predictor(models, tta=VIEWS3, refine="quarter")
    chunked = Predictor(models, tta=VIEWS3, refine="quarter", max_batch=3)       # 2 * 3 // 3 = 2 per chunk
    assert whole.max_batch == 21 and chunked.max_batch == 2
    assert Predictor(models, tta=[(0, 1)] * 16, max_batch=4).max_batch == 1
    per_member = ("raw", "scores", "preds", "heatmaps", "member_select", "disagree", "raw_sub", "preds_sub",
                  "refine_rule")
    for name in ("predict", "pseudo_label"):
        out = getattr(chunked, name)(x, center, scale, return_heatmaps=True)
        parts = [getattr(whole, name)(x[a:b], center[a:b], scale[a:b], return_heatmaps=True)
                 for a, b in ((0, 2), (2, 4), (4, 5))]
        for key in out:
            assert _eq(out[key], torch.cat([p[key] for p in parts], 1 if key in per_member else 0)), (name, key)
    assert sorted(s.batch.shape[0] for s in chunked._slots.values()) == [3, 3, 6, 6]     # three chunks: 2, 2, 1
    whole.release()
    chunked.release()


@pytest.mark.parametrize("graph", [True, False])
def test_refine_and_pseudo_label_read_the_merged_maps(graph):
    from ubpl_amd import Predictor, kernels as Kn
    from ubpl_amd.predict import DEFAULT_BLUR_SIGMA, assemble_kps
    from ubpl_amd.process import inverse_transforms
    models = _models()
    P = Predictor(models, tta=VIEWS3, flip_test=True, flip_pairs=PAIRS, refine="taylor", graph=graph)
    x = _imgs(3, torch.Generator().manual_seed(44))
    center, scale = _cs(3)
    H = W = RES // 4
    tinv = inverse_transforms(center, scale, [H, W]).to(DEV)
    taps = Kn.blur_taps(DEFAULT_BLUR_SIGMA).to(DEV)
    refine = lambda hm, raw: Kn.refine_peaks(hm.contiguous(), None, K * H * W, 3, K, H, W, None, raw.contiguous(),
                                             "taylor", taps, tinv)
    out = P.predict(x, center, scale, return_heatmaps=True)
    for mi in range(2):
        raw_sub, preds_sub, how = refine(out["heatmaps"][mi], out["raw"][mi])
        assert _eq(out["raw_sub"][mi], raw_sub) and _eq(out["preds_sub"][mi], preds_sub)
        assert _eq(out["refine_rule"][mi], how)
    assert 2.0 in set(out["refine_rule"].reshape(-1).tolist())
    ps = P.pseudo_label(x, center, scale, thr=0.1, return_heatmaps=True)
    for key in out:
        assert _eq(ps[key], out[key]), key
    thr = torch.full((1,), 0.1, device=DEV)
    ens_raw, ens_preds, ens_score, _, disagree, select, mean_hm = Kn.ensemble_pseudo(
        ps["heatmaps"].contiguous(), 3 * K * H * W, K * H * W, 2, 3, K, H, W, thr, tinv, want_mean=True)
    assert _eq(ps["ens_raw"], ens_raw) and _eq(ps["ens_preds"], ens_preds) and _eq(ps["ens_score"], ens_score)
    assert _eq(ps["disagree"], disagree) and _eq(ps["member_select"], select > 0) and _eq(ps["mean_heatmap"], mean_hm)
    assert _eq(ps["selected"], (select > 0).all(0)) and _eq(ps["kps"], assemble_kps(ens_preds, ps["selected"]))
    raw_sub, preds_sub, how = refine(mean_hm, ens_raw)
    assert _eq(ps["ens_raw_sub"], raw_sub) and _eq(ps["ens_preds_sub"], preds_sub) and _eq(ps["ens_refine_rule"], how)
    P.release()


def test_label_pool_records_the_views():
    from ubpl_amd import Predictor
    gen = torch.Generator().manual_seed(45)
    center, scale = _cs(2)
    loader = [(torch.rand(2, 3, RES, RES, generator=gen) - 0.5, None, {"center": center, "scale": scale})]
    P = Predictor(_models(), tta=VIEWS3)
    d = P.label_pool(loader, thr=0.1)
    assert d["tta"] == [[0.0, 1.0], [0.0, 1.25], [20.0, 0.8]]
    out = P.pseudo_label(loader[0][0], center, scale, thr=0.1)
    assert d["predsArraies"] == out["ens_preds"].cpu().tolist() and d["selected"] == out["selected"].cpu().tolist()
    assert "tta" not in Predictor(_models()).label_pool(loader, thr=0.1)
    P.release()
