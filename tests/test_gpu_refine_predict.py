"""Predictor(refine=...): the sub-pixel keys are ubpl_refine_peaks applied to the merged
heatmaps the Predictor returns — bit for bit, graph and eager — and refine="none" is the
Predictor of before.  Small networks as in tests/test_gpu_predict.py (k = 9, one stack, 128^2)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, RES = 9, 128
PAIRS = [(0, 1), (2, 5), (7, 8)]
SUB_KEYS = {"raw_sub", "preds_sub", "preds_mean_sub", "refine_rule"}
ENS_SUB_KEYS = {"ens_raw_sub", "ens_preds_sub", "ens_refine_rule", "kps_sub"}


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


def _cs(n):
    rs = np.random.RandomState(n + RES)
    center = torch.from_numpy(rs.uniform(0.4, 0.6, (n, 2)) * RES).float()
    scale = torch.from_numpy(rs.uniform(0.9, 1.3, n) * RES / 200.0).float()
    return center, scale


def _eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)


def _by_hand(hm, raw, refine, sigma, center, scale):
    """Kn.refine_peaks on merged heatmaps hm [N,K,H,W] and their peaks raw."""
    from ubpl_amd import kernels as Kn
    from ubpl_amd.process import inverse_transforms
    N, k, H, W = hm.shape
    tinv = inverse_transforms(center, scale, [H, W]).to(DEV)
    taps = Kn.blur_taps(sigma if refine == "taylor" else 0.0).to(DEV)
    return Kn.refine_peaks(hm.contiguous(), None, k * H * W, N, k, H, W, None, raw.contiguous(), refine, taps, tinv)


def test_refine_none_is_the_predictor_of_before(monkeypatch):
    from ubpl_amd import Predictor, _lib
    x = _imgs(3, torch.Generator().manual_seed(31))
    center, scale = _cs(3)
    old = Predictor(_models(), flip_test=True, flip_pairs=PAIRS)
    new = Predictor(_models(), flip_test=True, flip_pairs=PAIRS, refine="none", blur_sigma=1.5)
    for call in (lambda P: P.predict(x, center, scale, return_heatmaps=True), lambda P: P.predict(x),
                 lambda P: P.pseudo_label(x, center, scale, thr=0.1, return_heatmaps=True)):
        a, b = call(old), call(new)
        assert list(a) == list(b) and not (set(b) & (SUB_KEYS | ENS_SUB_KEYS))
        for key in a:
            assert _eq(a[key], b[key]), key
    # and nothing new is launched
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    Predictor(_models(), refine="none", graph=False).pseudo_label(x, center, scale)
    assert "ubpl_refine_peaks" not in names and names.count("ubpl_decode_heatmaps_flip") == 2
    names.clear()
    Predictor(_models(), refine="taylor", graph=False).pseudo_label(x, center, scale)
    assert names.count("ubpl_refine_peaks") == 3 and names.count("ubpl_decode_heatmaps_flip") == 2


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("refine,sigma", [("quarter", 1.0), ("taylor", 0.0), ("taylor", 1.0)])
def test_refine_is_the_kernel_on_the_returned_heatmaps(refine, sigma, flip):
    from ubpl_amd import Predictor
    models = _models()
    kw = dict(flip_test=flip, flip_pairs=PAIRS if flip else None)
    plain = Predictor(models, **kw)
    Pg = Predictor(models, refine=refine, blur_sigma=sigma, graph=True, **kw)
    Pe = Predictor(models, refine=refine, blur_sigma=sigma, graph=False, **kw)
    gen = torch.Generator().manual_seed(32)
    rules = set()
    for N in (1, 3, 3):                  # the second 3: another input through the same graph
        x = _imgs(N, gen)
        center, scale = _cs(N)
        ref = plain.predict(x, center, scale, return_heatmaps=True)
        g = Pg.predict(x, center, scale, return_heatmaps=True)
        e = Pe.predict(x, center, scale, return_heatmaps=True)
        assert set(g) == set(ref) | SUB_KEYS and list(g) == list(e)
        for key in g:
            assert _eq(g[key], e[key]), key
        for key in ref:                  # raw, preds, preds_mean, scores, heatmaps: untouched by refine
            assert _eq(g[key], ref[key]), key
        assert g["raw_sub"].shape == (2, N, K, 2) and g["preds_sub"].shape == (2, N, K, 2)
        assert g["refine_rule"].shape == (2, N, K) and g["preds_mean_sub"].shape == (N, K, 2)
        for mi in range(2):
            raw_sub, preds_sub, how = _by_hand(g["heatmaps"][mi], g["raw"][mi], refine, sigma, center, scale)
            assert _eq(g["raw_sub"][mi], raw_sub) and _eq(g["preds_sub"][mi], preds_sub)
            assert _eq(g["refine_rule"][mi], how)
        assert float((g["raw_sub"] - g["raw"]).abs().max()) <= 1.0
        assert float((g["raw_sub"] - g["raw"]).abs().max()) > 0.0
        assert _eq(g["preds_mean_sub"], torch.stack([g["preds_sub"][0], g["preds_sub"][1]], -1).mean(-1))
        rules |= set(g["refine_rule"].reshape(-1).tolist())
    assert rules <= {0.0, 1.0, 2.0} and (2.0 if refine == "taylor" else 1.0) in rules
    bare = Pg.predict(x)
    assert bare["preds_sub"] is None and bare["preds_mean_sub"] is None
    assert _eq(bare["raw_sub"], g["raw_sub"]) and _eq(bare["refine_rule"], g["refine_rule"])
    for P in (plain, Pg, Pe):
        P.release()


@pytest.mark.parametrize("refine", ["quarter", "taylor"])
def test_pseudo_label_refines_the_ensemble_peak(refine):
    from ubpl_amd import Predictor
    from ubpl_amd.predict import DEFAULT_BLUR_SIGMA, assemble_kps
    models = _models()
    plain = Predictor(models, flip_test=True, flip_pairs=PAIRS)
    x = _imgs(3, torch.Generator().manual_seed(33))
    center, scale = _cs(3)
    ref = plain.pseudo_label(x, center, scale, thr=0.1, return_heatmaps=True)
    for graph in (True, False):
        P = Predictor(models, flip_test=True, flip_pairs=PAIRS, refine=refine, graph=graph)
        out = P.pseudo_label(x, center, scale, thr=0.1, return_heatmaps=True)
        assert set(out) == set(ref) | SUB_KEYS | ENS_SUB_KEYS
        for key in ref:                  # spread included: it stays on the integer peaks
            assert _eq(out[key], ref[key]), key
        raw_sub, preds_sub, how = _by_hand(out["mean_heatmap"], out["ens_raw"], refine, DEFAULT_BLUR_SIGMA, center, scale)
        assert _eq(out["ens_raw_sub"], raw_sub) and _eq(out["ens_preds_sub"], preds_sub)
        assert _eq(out["ens_refine_rule"], how) and out["ens_refine_rule"].shape == (3, K)
        assert _eq(out["kps_sub"], assemble_kps(preds_sub, out["selected"])) and out["kps_sub"].shape == (3, K, 3)
        for mi in range(2):
            got = _by_hand(out["heatmaps"][mi], out["raw"][mi], refine, DEFAULT_BLUR_SIGMA, center, scale)
            assert _eq(out["raw_sub"][mi], got[0]) and _eq(out["preds_sub"][mi], got[1])
        bare = P.pseudo_label(x, thr=0.1)
        assert bare["ens_preds_sub"] is None and bare["kps_sub"] is None and _eq(bare["ens_raw_sub"], raw_sub)
        P.release()


def _loader(gen):
    loader = []
    for bs in (3, 2):
        center, scale = _cs(bs)
        kps = torch.rand(bs, K, 3, generator=gen) * RES
        kps[..., 2] = 1
        kps[0, 4, :2] = 0                                           # an unlabeled joint
        loader.append((torch.rand(bs, 3, RES, RES, generator=gen) - 0.5, None,
                       {"center": center, "scale": scale, "kpsMap": kps}))
    return loader


@pytest.mark.parametrize("refine,sigma", [("quarter", 1.0), ("taylor", 0.5)])
def test_label_pool_and_validate_take_the_sub_pixel_coordinates(refine, sigma):
    from ubpl_amd import Predictor, train as T
    loader = _loader(torch.Generator().manual_seed(34))
    P = Predictor(_models(), refine=refine, blur_sigma=sigma)
    args = types.SimpleNamespace(outRes=32, pck_ref=[0, 1], pck_thr=0.5)
    d = P.label_pool(loader, args, thr=0.1, rule="ensemble")
    outs = [P.pseudo_label(x, m["center"], m["scale"], thr=0.1, rule="ensemble", out_res=32) for x, _, m in loader]
    sub = torch.cat([o["ens_preds_sub"] for o in outs]).cpu()
    assert d["predsArraies"] == sub.tolist() and len(d["predsArraies"]) == 5
    assert d["predsArraies"] != torch.cat([o["ens_preds"] for o in outs]).cpu().tolist()
    assert d["refine"] == refine and d["blur_sigma"] == (sigma if refine == "taylor" else None)
    assert d["selected"] == torch.cat([o["selected"] for o in outs]).cpu().tolist()
    plain = Predictor(_models()).label_pool(loader, args, thr=0.1, rule="ensemble")
    assert "refine" not in plain and "blur_sigma" not in plain
    assert plain["predsArraies"] == torch.cat([o["ens_preds"] for o in outs]).cpu().tolist()
    # validate: the rows of the sub-pixel predictions, folded by the same code
    got = P.validate(loader, args)
    rows = []
    for x, _, m in loader:
        o = P.predict(x, m["center"], m["scale"], out_res=32)
        rows.append(T.valid_batch_row(list(o["preds_sub"]) + [o["preds_mean_sub"]], m, torch.device(DEV), args))
    assert got == T.fold_valid_rows(rows, 3)
    assert got != Predictor(_models()).validate(loader, args)
    assert got[0][0] == torch.cat([P.predict(x, m["center"], m["scale"], out_res=32)["preds_sub"][0]
                                   for x, _, m in loader]).cpu().tolist()


def test_kps_from_heatmap_takes_refine():
    from ubpl_amd import Predictor
    from ubpl_amd.predict import DEFAULT_BLUR_SIGMA
    from ubpl_amd.process import ProcessUtils
    x = _imgs(3, torch.Generator().manual_seed(36))
    center, scale = _cs(3)
    out = Predictor(_model(0)).predict(x, center, scale, return_heatmaps=True)
    hm, res = out["heatmaps"][0], [RES // 4, RES // 4]
    preds, scores = ProcessUtils.kps_fromHeatmap(hm, center, scale, res)
    assert _eq(preds, out["preds"][0]) and _eq(scores, out["scores"][0])      # the default path, untouched
    for refine, sigma in (("quarter", None), ("taylor", None), ("taylor", 0.0)):
        sub, sc = ProcessUtils.kps_fromHeatmap(hm.cpu(), center, scale, res, refine=refine, blur_sigma=sigma)
        want = _by_hand(hm, out["raw"][0], refine, DEFAULT_BLUR_SIGMA if sigma is None else sigma, center, scale)[1]
        assert sub.device.type == "cpu" and _eq(sub, want) and _eq(sc, scores)
        assert not _eq(sub, preds)
    one = ProcessUtils.kps_fromHeatmap(hm[1], center[1], scale[1], res, mode="single", refine="quarter")
    assert _eq(one, _by_hand(hm, out["raw"][0], "quarter", 0.0, center, scale)[1][1])
    with pytest.raises(ValueError, match="refine is one of"):
        ProcessUtils.kps_fromHeatmap(hm, center, scale, res, refine="dark")


def test_chunks_concatenate_the_new_keys():
    from ubpl_amd import Predictor
    models = _models()
    x = _imgs(3, torch.Generator().manual_seed(35))
    center, scale = _cs(3)
    whole = Predictor(models, refine="taylor")
    chunked = Predictor(models, refine="taylor", max_batch=2)
    for name in ("predict", "pseudo_label"):
        out = getattr(chunked, name)(x, center, scale, return_heatmaps=True)
        parts = [getattr(whole, name)(x[a:b], center[a:b], scale[a:b], return_heatmaps=True) for a, b in ((0, 2), (2, 3))]
        assert out["raw_sub"].shape == (2, 3, K, 2) and out["preds_sub"].shape == (2, 3, K, 2)
        assert out["refine_rule"].shape == (2, 3, K) and out["preds_mean_sub"].shape == (3, K, 2)
        per_member = ("raw", "scores", "preds", "heatmaps", "member_select", "disagree", "raw_sub", "preds_sub",
                      "refine_rule")
        assert set(out) == set(parts[0])
        for key in out:
            assert _eq(out[key], torch.cat([p[key] for p in parts], 1 if key in per_member else 0)), (name, key)
    assert out["ens_raw_sub"].shape == (3, K, 2) and out["ens_refine_rule"].shape == (3, K)
    assert out["kps_sub"].shape == (3, K, 3)
