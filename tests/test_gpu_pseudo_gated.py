"""ubpl_loss_finalize kind 3 through step_losses._pseudo_gated: the UBPL pseudo mask with a given
selection.  B = 4, S = 2, K = 3, 16x16 maps, M = 2 teachers."""
import numpy as np
import pytest
import torch

import seeds

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S, K, R, M = 4, 2, 3, 16, 2
THR = 0.95
INF = float("inf")


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


_IN = {}


def _inputs():
    """Seeded blobs whose maxima straddle THR (seeds._blobs), made once and never changed."""
    if not _IN:
        g = torch.Generator().manual_seed(733)
        _IN["preds"] = seeds._blobs(g, (B, S, K), R, 0.6, 1.25)
        t0 = seeds._blobs(g, (B, S, K), R, 0.85, 1.35)
        _IN["teachers"] = torch.stack([t0, t0 + 0.02 * torch.randn(t0.shape, generator=g)]).contiguous()
        _IN["sw"] = torch.tensor([1.0, 0.5, 0.0, 1.0])                 # one labelled row (weight 0)
        _IN["gate"] = torch.tensor([[1, 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 0]], dtype=torch.float32)
    return _IN


def _ref(preds, teachers, sw, thr, gate):
    """JointPseudoLoss3 (utils/losses.py:176-210) in float64, the mask multiplied by the gate
    -> (sum, n_pseudo, n_sel, score [K], d sum / d preds)."""
    p = preds.double().clone().requires_grad_(True)
    T = teachers.double()[:, :, -1].mean(0).reshape(B, 1, K, -1)
    rows = p.reshape(B, S, K, -1)
    loss = ((rows - T) ** 2).mean(-1) * sw.double().reshape(B, 1, 1)
    s1 = rows.max(-1).values
    s2 = T.max(-1).values.expand(B, S, K)
    mask = (s1 >= thr).double() * (s2 >= thr).double() * (gate.double() > 0).double().reshape(B, 1, K)
    total = (loss * mask).sum()
    total.backward()
    on = sw > 0
    score = ((s1[on].mean(0) + s2[on].mean(0)) / 2).mean(0)
    return total.detach(), int((loss > 0).sum()), int((mask > 0).sum()), score.detach(), p.grad


def _run(fn, preds, *a):
    p = preds.clone().to(DEV).requires_grad_(True)
    s, cnt, score = fn(p, *a)
    s.backward()
    torch.cuda.synchronize()
    return s.detach().cpu(), cnt.cpu(), score.cpu(), p.grad.cpu()


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("thr", [THR, 0.15])
def test_gate_of_ones_is_kind_2(thr):
    from ubpl_amd import step_losses as SL
    d = _inputs()
    t, sw = _dev(d["teachers"], d["sw"])
    ones = torch.ones(B, K, device=DEV)
    old = _run(SL._pseudo, d["preds"], t, sw, S, thr)
    new = _run(SL._pseudo_gated, d["preds"], t, sw, S, thr, ones)
    assert 0 < int(old[1][2]) and int(old[1][1]) > 0
    for name, a, b in zip(("sum", "cnt", "score", "grad"), old, new):
        assert _bits_equal(a, b) if a.dtype.is_floating_point else torch.equal(a, b), name
    # out_w as well: the backward's row weights
    from ubpl_amd import kernels as Kn
    rows = Kn.RowSpec.ensemble(B, S, K, R * R, M, t.shape[2])
    sq, am, tm = Kn.row_stats(d["preds"].to(DEV), t, rows, want_amax=True, want_tmax=True)
    w2 = Kn.loss_finalize(2, sq, am, tm, None, sw, False, True, B, S, K, thr)[3]
    w3 = Kn.loss_finalize(3, sq, am, tm, ones, sw, False, True, B, S, K, thr)[3]
    assert _bits_equal(w2, w3) and float(w2.sum()) > 0


def test_gate_of_zeros_selects_nothing():
    from ubpl_amd import step_losses as SL
    d = _inputs()
    t, sw = _dev(d["teachers"], d["sw"])
    old = _run(SL._pseudo, d["preds"], t, sw, S, THR)
    s, cnt, score, grad = _run(SL._pseudo_gated, d["preds"], t, sw, S, THR, torch.zeros(B, K, device=DEV))
    assert float(s) == 0.0 and int(cnt[2]) == 0 and float(grad.abs().max()) == 0.0
    assert int(cnt[1]) == int(old[1][1]) > 0 and int(cnt[0]) == int(old[1][0]) and int(cnt[3]) == int(old[1][3])
    assert _bits_equal(score, old[2])


@pytest.mark.parametrize("thr", [THR, -INF])
def test_mixed_gate_against_float64(thr):
    """Value and gradient against the float64 restatement, at test_losses_vs_golden's kind-2
    tolerances; the counts exactly.  No score of the inputs lies within 1e-4 of THR, so float32 and
    float64 take the same side of every comparison."""
    from ubpl_amd import step_losses as SL
    d = _inputs()
    rs, n_ps, n_sel, rscore, rgrad = _ref(d["preds"], d["teachers"], d["sw"], thr, d["gate"])
    s1 = d["preds"].reshape(B, S, K, -1).max(-1).values
    s2 = d["teachers"][:, :, -1].mean(0).reshape(B, K, -1).max(-1).values
    assert float((s1 - THR).abs().min()) > 1e-4 and float((s2 - THR).abs().min()) > 1e-4
    t, sw, gate = _dev(d["teachers"], d["sw"], d["gate"])
    s, cnt, score, grad = _run(SL._pseudo_gated, d["preds"], t, sw, S, thr, gate)
    print("thr", thr, "sum", float(s), "ref", float(rs), "n_pseudo", n_ps, "n_sel", n_sel)
    assert 0 < n_sel < B * S * K
    if thr == -INF:
        assert n_sel == S * int(d["gate"].sum())                      # the gate alone decides
    else:
        assert n_sel < S * int(d["gate"].sum())                       # the scores bite as well
    assert cnt.tolist() == [S * B * K, n_ps, n_sel, 3]
    np.testing.assert_allclose(float(s), float(rs), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(score.numpy(), rscore.numpy(), rtol=1e-5)
    np.testing.assert_allclose(grad.numpy(), rgrad.numpy(), rtol=1e-4, atol=1e-8)
    gate_rows = (d["gate"] > 0).reshape(B, 1, K, 1, 1).expand(B, S, K, R, R)
    assert float(grad[~gate_rows].abs().max()) == 0.0                 # a closed gate passes no gradient


def test_nan_score_never_selects():
    """A NaN maximum fails both score tests at every thr, -inf included, whatever the gate."""
    from ubpl_amd import kernels as Kn
    d = _inputs()
    sw = d["sw"].to(DEV)
    ones = torch.ones(B, K, device=DEV)
    rows = B * S * K
    sq = torch.full((rows,), 0.25, device=DEV)
    am = torch.ones(rows, device=DEV)
    tm = torch.ones(rows, device=DEV)
    am[1] = float("nan")
    tm[2] = float("nan")
    for thr in (-INF, 0.5):
        _, cnt, _, w = Kn.loss_finalize(3, sq, am, tm, ones, sw, False, True, B, S, K, thr)
        w = w.cpu()
        assert int(cnt[2]) == rows - 2 and w[1] == 0 and w[2] == 0 and w[0] == 1.0
