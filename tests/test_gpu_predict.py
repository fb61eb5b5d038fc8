"""Predictor: frozen, graph-replayed inference against the eager eval forward of the
same networks — bit for bit (the forward has no float atomics: equal inputs through
equal kernels give equal bits)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRECISIONS = ["2xfp16", "f32"]
CONFIGS = [(9, 1), (16, 2)]
FROZEN_CALLS = ("ubpl_conv_weights_split", "ubpl_conv_weights_relayout", "ubpl_stem_weight_s2d_split",
                "ubpl_bn_eval_coeffs", "ubpl_bn_eval_coeffs_table")


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


_MODELS = {}


def _model(k, nstack, prec, seed=0):
    """A network whose running statistics and BN affine parameters are not the initial
    ones: two train-mode forwards, seeded noise on every gamma and beta.  Built once."""
    from ubpl_amd.hourglass import StackedHourglass
    key = (k, nstack, prec, seed)
    if key not in _MODELS:
        torch.manual_seed(seed)
        m = StackedHourglass(k, nstack, "AvgPool")
        m.set_conv_precision(prec)
        gen = torch.Generator().manual_seed(100 + seed)
        with torch.no_grad():
            for _ in range(2):
                m(_imgs(2, 128, gen))
            for b in m._bn_names:
                for suffix in (".weight", ".bias"):
                    p = m.P(b + suffix)
                    p.add_((torch.randn(p.shape, generator=gen) * 0.1).to(DEV))
        _MODELS[key] = m
    return _MODELS[key]


def _imgs(n, res, gen):
    return (torch.rand(n, 3, res, res, generator=gen) - 0.5).to(DEV)


def _eager(m, x):
    """Last-stack heatmaps of the eval forward; the training flag is put back."""
    was = m.training
    with torch.no_grad():
        o = m.eval()(x)[0][:, -1].contiguous()
    m.train(was)
    return o


def _cs(n, res):
    rs = np.random.RandomState(n + res)
    center = torch.from_numpy(rs.uniform(0.4, 0.6, (n, 2)) * res).float()
    scale = torch.from_numpy(rs.uniform(0.9, 1.3, n) * res / 200.0).float()
    return center, scale


def _eq(a, b):
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def _check_against(out, hm, center, scale, mi=0):
    """out (a predict result) decodes the heatmaps hm [N,K,H,W] as Kn.decode_heatmaps does."""
    from ubpl_amd import kernels as Kn
    from ubpl_amd.process import inverse_transforms
    tinv = inverse_transforms(center, scale, list(hm.shape[2:])).to(DEV)
    raw, preds, scores = Kn.decode_heatmaps(hm.contiguous(), tinv)
    assert _eq(out["heatmaps"][mi], hm)
    assert _eq(out["raw"][mi], raw) and _eq(out["preds"][mi], preds) and _eq(out["scores"][mi], scores)


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("case", [(9, 1, 128, 1), (9, 1, 128, 3), (16, 2, 128, 1), (16, 2, 128, 3), (16, 2, 256, 2)])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_predict_is_the_eager_eval_forward(prec, case, graph):
    from ubpl_amd import Predictor
    k, nstack, res, B = case
    m = _model(k, nstack, prec)
    P = Predictor(m, graph=graph)
    gen = torch.Generator().manual_seed(B * 7 + res)
    center, scale = _cs(B, res)
    for rep in range(2):             # the second: another input of the same size through the same graph
        x = _imgs(B, res, gen)
        out = P.predict(x if rep else x.cpu(), center, scale, return_heatmaps=True)
        assert out["heatmaps"].shape == (1, B, k, res // 4, res // 4)
        _check_against(out, _eager(m, x), center, scale)
        assert _eq(out["preds_mean"], out["preds"][0])
    assert len(P._slots) == 1 and (next(iter(P._slots.values())).graph is not None) == graph
    plain = P.predict(x)
    assert plain["preds"] is None and plain["preds_mean"] is None and "heatmaps" not in plain
    assert _eq(plain["raw"], out["raw"]) and _eq(plain["scores"], out["scores"])
    P.release()


@pytest.mark.parametrize("pairs", [None, [(0, 1), (2, 5), (7, 8)]])
@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_flip_test_matches_the_restatement(prec, cfg, pairs):
    from ubpl_amd import Predictor, kernels as Kn
    k, nstack = cfg
    m = _model(k, nstack, prec)
    B, res = 3, 128
    x = _imgs(B, res, torch.Generator().manual_seed(11))
    o = _eager(m, torch.cat([x, x.flip(-1)])).cpu()
    back = o[B:].flip(-1)
    if pairs:
        back = back[:, Kn.flip_perm(k, pairs).long()]
    merged = ((o[:B] + back) * 0.5).to(DEV)
    center, scale = _cs(B, res)
    for graph in (True, False):
        P = Predictor(m, flip_test=True, flip_pairs=pairs, graph=graph)
        _check_against(P.predict(x, center, scale, return_heatmaps=True), merged, center, scale)
        P.release()


@pytest.mark.parametrize("prec", PRECISIONS)
def test_flip_test_of_a_symmetric_image_is_mirror_consistent(prec):
    from ubpl_amd import Predictor
    m = _model(9, 1, prec)
    res = 128
    x = _imgs(2, res, torch.Generator().manual_seed(12))
    x[..., res // 2:] = x[..., :res // 2].flip(-1)
    assert _eq(x, x.flip(-1))
    out = Predictor(m, flip_test=True).predict(x, return_heatmaps=True)
    hm, raw, W = out["heatmaps"][0], out["raw"][0].cpu(), res // 4
    assert _eq(hm, hm.flip(-1))                      # (a + b) / 2 of a map and its own mirror
    seen = 0
    for n in range(2):
        for j in range(9):
            cx, cy = int(raw[n, j, 0]), int(raw[n, j, 1])
            if cx == 0:
                continue
            seen += 1
            # the mirrored pixel holds the same maximum; the smaller flat index was taken
            assert hm[n, j, cy - 1, W - cx] == out["scores"][0, n, j]
            assert cx - 1 <= W - cx
    assert seen > 0


@pytest.mark.parametrize("prec", PRECISIONS)
def test_frozen_means_frozen(prec, monkeypatch):
    from ubpl_amd import Predictor, _lib
    models = [_model(9, 1, prec), _model(9, 1, prec, seed=1)]
    P = Predictor(models, flip_test=True, graph=False)
    counts = {}
    real = _lib.call

    def counting(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", counting)
    x = _imgs(2, 128, torch.Generator().manual_seed(13))
    P.predict(x, *_cs(2, 128))
    assert counts.get("ubpl_decode_heatmaps_flip") == 2 and counts.get("ubpl_fliplr") == 1
    assert [counts.get(n, 0) for n in FROZEN_CALLS] == [0] * len(FROZEN_CALLS), counts
    counts.clear()
    P.refresh()
    assert counts.get("ubpl_bn_eval_coeffs_table") == len(models)
    assert counts.get("ubpl_bn_eval_coeffs", 0) == 0
    assert set(counts) <= set(FROZEN_CALLS), counts


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_snapshot_until_refresh(prec, graph):
    from ubpl_amd import Predictor
    from ubpl_amd.hourglass import StackedHourglass
    from ubpl_amd.losses import JointMSELoss
    torch.manual_seed(5)
    m = StackedHourglass(9, 1, "AvgPool")                      # its own: this test changes it
    m.set_conv_precision(prec)
    gen = torch.Generator().manual_seed(14)
    m(_imgs(2, 128, gen))
    flag, nbt = m.training, m._nbt.clone()
    x = _imgs(3, 128, gen)
    center, scale = _cs(3, 128)
    P = Predictor(m, graph=graph)
    old = P.predict(x, center, scale, return_heatmaps=True)
    _check_against(old, _eager(m, x), center, scale)
    assert m.training == flag and _eq(m._nbt, nbt)
    with torch.no_grad():                                      # a training step's worth of change, in place
        m.flat_params.mul_(1.0 + 0.05 * torch.rand(m.flat_params.shape, generator=gen).to(DEV))
        m.flat_stats.add_(0.05 * torch.rand(m.flat_stats.shape, generator=gen).to(DEV))
    again = P.predict(x, center, scale, return_heatmaps=True)
    for key in old:
        assert _eq(again[key], old[key]), key
    # the network still trains
    preds, _ = m(_imgs(2, 128, gen))
    loss, _ = JointMSELoss(nStack=1)(preds, torch.rand(2, 9, 32, 32, generator=gen).to(DEV))
    loss.backward()
    assert torch.isfinite(m.flat_grads).all() and float(m.flat_grads.abs().sum()) > 0
    again = P.predict(x, center, scale, return_heatmaps=True)
    for key in old:
        assert _eq(again[key], old[key]), key
    flag, nbt = m.training, m._nbt.clone()
    P.refresh()
    new = P.predict(x, center, scale, return_heatmaps=True)
    assert m.training == flag and _eq(m._nbt, nbt)
    _check_against(new, _eager(m, x), center, scale)
    assert not _eq(new["heatmaps"], old["heatmaps"])
    P.release()


@pytest.mark.parametrize("prec", PRECISIONS)
def test_two_teachers_and_their_mean(prec):
    from ubpl_amd import Predictor
    models = [_model(9, 1, prec), _model(9, 1, prec, seed=1)]
    x = _imgs(3, 128, torch.Generator().manual_seed(15))
    center, scale = _cs(3, 128)
    out = Predictor(models).predict(x, center, scale, return_heatmaps=True)
    for mi, m in enumerate(models):
        _check_against(out, _eager(m, x), center, scale, mi)
    assert not _eq(out["preds"][0], out["preds"][1])
    assert _eq(out["preds_mean"], torch.stack([out["preds"][0], out["preds"][1]], -1).mean(-1))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_validate_equals_train_validate(prec):
    from ubpl_amd import Predictor, train as T
    models = [_model(9, 1, prec), _model(9, 1, prec, seed=1)]
    gen = torch.Generator().manual_seed(16)
    loader = []
    for bs in (3, 3, 1):
        center, scale = _cs(bs, 128 + len(loader))
        kps = torch.rand(bs, 9, 3, generator=gen) * 128
        kps[..., 2] = 1
        kps[0, 4, :2] = 0                                       # an unlabeled joint
        loader.append((torch.rand(bs, 3, 128, 128, generator=gen) - 0.5, None,
                       {"center": center, "scale": scale, "kpsMap": kps}))
    args = types.SimpleNamespace(outRes=32, pck_ref=[0, 1], pck_thr=0.5)
    want = T.validate(loader, models, args)
    P = Predictor(models)
    got = P.validate(loader, args)
    assert len(P._slots) == 2                                   # two batch sizes, two graphs
    assert got == want
    assert len(got[0]) == 3 and len(got[0][0]) == 7


def test_one_graph_kept_and_chunks():
    from ubpl_amd import Predictor
    m = _model(9, 1, "2xfp16")
    gen = torch.Generator().manual_seed(17)
    P = Predictor(m, max_graphs=1)
    for n in (1, 3, 1, 3):
        x = _imgs(n, 128, gen)
        out = P.predict(x, *_cs(n, 128), return_heatmaps=True)
        _check_against(out, _eager(m, x), *_cs(n, 128))
        assert len(P._slots) == 1
    x = _imgs(5, 128, gen)
    center, scale = _cs(5, 128)
    out = Predictor(m, max_batch=2).predict(x, center, scale, return_heatmaps=True)
    assert out["raw"].shape == (1, 5, 9, 2) and out["preds_mean"].shape == (5, 9, 2)
    hm = torch.cat([_eager(m, x[a:a + 2]) for a in (0, 2, 4)])
    _check_against(out, hm, center, scale)
