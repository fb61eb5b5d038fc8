"""Predictor.pseudo_label / label_pool: the restatement of tests/test_pseudo_host.py applied
to the heatmaps predict() returns — bit for bit, except disagree (a float32 sum, held to the
project's fp32-loss bar of 1e-4 relative) and spread (the square root of an exact integer,
held to one unit in the last place of float32 around the correctly rounded value)."""
import numpy as np
import pytest
import torch

from test_pseudo_host import restate_pseudo

pytestmark = pytest.mark.gpu
DEV = "cuda"
K, RES = 9, 128


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


_MODELS = {}


def _imgs(n, res, gen):
    return (torch.rand(n, 3, res, res, generator=gen) - 0.5).to(DEV)


def _model(seed):
    """A 1-stack k=9 network whose running statistics and BN affine parameters are not the
    initial ones (as tests/test_gpu_predict.py builds its networks).  Built once per seed."""
    from ubpl_amd.hourglass import StackedHourglass
    if seed not in _MODELS:
        torch.manual_seed(seed)
        m = StackedHourglass(K, 1, "AvgPool")
        m.set_conv_precision("2xfp16")
        gen = torch.Generator().manual_seed(100 + seed)
        with torch.no_grad():
            for _ in range(2):
                m(_imgs(2, RES, gen))
            for b in m._bn_names:
                for suffix in (".weight", ".bias"):
                    p = m.P(b + suffix)
                    p.add_((torch.randn(p.shape, generator=gen) * 0.1).to(DEV))
        _MODELS[seed] = m
    return _MODELS[seed]


def _models(M):
    return [_model(s) for s in range(M)]


def _cs(n, res):
    rs = np.random.RandomState(n + res)
    center = torch.from_numpy(rs.uniform(0.4, 0.6, (n, 2)) * res).float()
    scale = torch.from_numpy(rs.uniform(0.9, 1.3, n) * res / 200.0).float()
    return center, scale


def _eq(a, b):
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def _median_thr(P, x, center, scale):
    """Seeded networks score low: a threshold at the median ensemble score, placed between two
    neighbouring scores so that >= has a margin on both sides."""
    s = P.pseudo_label(x, center, scale, thr=0.0)["ens_score"].reshape(-1).sort().values.cpu()
    mid = s.numel() // 2
    assert s[mid - 1] < s[mid]
    return float((s[mid - 1].double() + s[mid].double()) / 2)


def _check(out, ref, thr, rule, center, scale):
    """out (a pseudo_label result with heatmaps) against predict's result ref and the
    restatement of ref's heatmaps."""
    for key in ("raw", "preds", "scores", "preds_mean", "heatmaps"):
        assert _eq(out[key], ref[key]), key
    want = restate_pseudo(ref["heatmaps"].cpu(), thr, center, scale)
    assert _eq(out["mean_heatmap"], want["mean_hm"])
    for key in ("ens_raw", "ens_preds", "ens_score"):
        assert _eq(out[key], want[key]), key
    assert out["member_select"].dtype == torch.bool and _eq(out["member_select"], want["select"] > 0)
    g, w = out["disagree"].double().cpu().numpy(), want["disagree"].numpy()
    assert (np.abs(g - w) <= 1e-4 * np.abs(w)).all(), float(np.max(np.abs(g - w) / np.abs(w)))
    t32 = torch.tensor(thr, dtype=torch.float32)
    sel = (want["select"] > 0).all(0) if rule == "unanimous" else want["ens_score"] >= t32
    assert out["selected"].dtype == torch.bool and _eq(out["selected"], sel)
    d = ref["raw"].cpu() - want["ens_raw"]
    spread = (d * d).sum(-1).double().sqrt().amax(0)
    assert out["spread"].shape == spread.shape
    assert np.allclose(out["spread"].double().cpu().numpy(), spread.numpy(), rtol=2.0 ** -22, atol=0)
    assert _eq(out["kps"], torch.cat([want["ens_preds"], sel.float()[..., None]], -1))
    return sel


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("M,N,max_batch", [(2, 1, 32), (2, 3, 32), (3, 3, 32), (2, 3, 2)])
def test_pseudo_label_is_the_restatement_of_predicts_heatmaps(M, N, max_batch, flip, graph):
    from ubpl_amd import Predictor
    P = Predictor(_models(M), flip_test=flip, flip_pairs=[(0, 1), (2, 5)] if flip else None, max_batch=max_batch,
                  graph=graph)
    x = _imgs(N, RES, torch.Generator().manual_seed(21 + N))
    center, scale = _cs(N, RES)
    thr = _median_thr(P, x, center, scale)
    ref = P.predict(x, center, scale, return_heatmaps=True)
    sels = {}
    for rule in ("unanimous", "ensemble"):
        out = P.pseudo_label(x, center, scale, thr=thr, rule=rule, return_heatmaps=True)
        assert out["heatmaps"].shape == (M, N, K, RES // 4, RES // 4)
        sels[rule] = _check(out, ref, thr, rule, center, scale)
    if N * K >= 6:
        assert sels["ensemble"].any() and not sels["ensemble"].all()          # both classes occur
    assert not (sels["unanimous"] & ~sels["ensemble"]).any()                  # a subset
    plain = P.pseudo_label(x, thr=thr)
    assert plain["preds"] is None and plain["ens_preds"] is None and plain["kps"] is None
    assert "heatmaps" not in plain and "mean_heatmap" not in plain
    assert _eq(plain["ens_raw"], out["ens_raw"]) and _eq(plain["selected"], sels["unanimous"])
    P.release()


def test_pseudo_label_leaves_predict_alone():
    from ubpl_amd import Predictor
    P = Predictor(_models(2), flip_test=True)
    x = _imgs(3, RES, torch.Generator().manual_seed(22))
    center, scale = _cs(3, RES)
    first = P.predict(x, center, scale, return_heatmaps=True)
    slot = next(iter(P._slots.values()))
    graph = slot.graph
    P.pseudo_label(_imgs(3, RES, torch.Generator().manual_seed(23)), center, scale, thr=0.1)
    second = P.predict(x, center, scale, return_heatmaps=True)
    assert len(P._slots) == 2 and any(s is slot for s in P._slots.values())   # predict's slot and graph stayed
    assert graph is not None and slot.graph is graph
    for key in first:
        assert _eq(first[key], second[key]), key
    P.release()


def test_thresholds_share_one_graph():
    from ubpl_amd import Predictor
    P = Predictor(_models(2), max_graphs=1)
    x = _imgs(3, RES, torch.Generator().manual_seed(24))
    center, scale = _cs(3, RES)
    thr = _median_thr(P, x, center, scale)
    slot = next(iter(P._slots.values()))
    outs = [P.pseudo_label(x, center, scale, thr=t, rule="ensemble") for t in (thr, 1e9, thr)]
    assert len(P._slots) == 1 and next(iter(P._slots.values())) is slot and slot.graph is not None
    assert outs[0]["selected"].any() and not outs[0]["selected"].all()
    assert not outs[1]["selected"].any() and not outs[1]["member_select"].any()
    for key in ("ens_raw", "ens_score", "disagree", "spread"):
        assert _eq(outs[0][key], outs[1][key]), key
    assert _eq(outs[0]["selected"], outs[2]["selected"]) and _eq(outs[0]["member_select"], outs[2]["member_select"])
    with pytest.raises(ValueError, match="rule is one of"):
        P.pseudo_label(x, center, scale, rule="majority")
    P.release()


def test_label_pool_is_pseudo_label_per_batch(tmp_path):
    import types
    from ubpl_amd import Predictor, checkpoint as C
    P = Predictor(_models(2))
    gen = torch.Generator().manual_seed(25)
    loader = []
    for bs in (3, 3, 1):
        center, scale = _cs(bs, RES + len(loader))
        loader.append((torch.rand(bs, 3, RES, RES, generator=gen) - 0.5, None, {"center": center, "scale": scale}))
    thr = _median_thr(P, loader[0][0], loader[0][2]["center"], loader[0][2]["scale"])
    args = types.SimpleNamespace(outRes=32)
    d = P.label_pool(loader, args, thr=thr, rule="ensemble")
    outs = [P.pseudo_label(x, m["center"], m["scale"], thr=thr, rule="ensemble", out_res=32) for x, _, m in loader]
    cat = lambda key, dim=0: torch.cat([o[key] for o in outs], dim).cpu()
    assert d["predsArraies"] == cat("ens_preds").tolist() and len(d["predsArraies"]) == 7
    assert len(d["predsArraies"][0]) == K and len(d["predsArraies"][0][0]) == 2
    assert d["selected"] == cat("selected").tolist()
    assert d["ens_score"] == cat("ens_score").tolist() and d["spread"] == cat("spread").tolist()
    assert d["disagree"] == cat("disagree", 1).transpose(0, 1).tolist()
    assert d["thr"] == thr and d["rule"] == "ensemble"
    frac = cat("selected").float().mean(0).tolist()
    assert d["selected_fraction"] == frac and 0.0 < sum(frac) < K
    path = C.save_pseudo_data(d, str(tmp_path / "pseudo.json"))
    assert C.load_pseudo_data(path) == d
    P.release()
