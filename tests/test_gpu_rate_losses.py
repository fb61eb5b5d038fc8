"""JointPseudoLoss, JointPseudoLoss2 and JointDistLoss_mt on the device against the reference's own
outputs (tests/golden/rate_losses.npz) and, for the gradient, float64 autograd of tests/rate_ref.py.
The fixture's cases meet the separation condition (test_rate_host.py asserts it on the CPU), so counts
compare exactly."""
import os
import sys

import numpy as np
import pytest
import torch

import rate_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "rate_losses.npz")
TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def _close(got, want):
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return got.shape == want.shape and bool((np.abs(got - want) <= TOL * np.abs(want)).all())


def _sw(name):
    return torch.tensor(RR.SW[name], device=DEV).reshape(-1, 1)


def _grad_check(loss, leaf, ref_loss, ref_leaf):
    loss.backward()
    ref_loss.backward()
    g, r = leaf.grad.cpu().double(), ref_leaf.grad
    assert float(r.abs().max()) > 0
    assert float((g - r).abs().max()) <= TOL * float(r.abs().max())


@pytest.mark.parametrize("name", list(RR.CASES))
def test_pseudo_losses_against_the_reference(gold, name):
    from ubpl_amd.losses import JointPseudoLoss, JointPseudoLoss2
    S = RR.CASES[name][2]
    preds, targets, _ = RR.make_case(name)
    p, t = torch.from_numpy(preds).to(DEV), torch.from_numpy(targets).to(DEV)
    for sw in ("half", "unlabeled"):
        for rate in RR.SEL_RATES:
            key = "%s/%s/r%s" % (name, sw, rate)
            s, n_ps, n_sel, score, t1, t2 = JointPseudoLoss2(S, rate)(p, t, _sw(sw))
            assert (n_ps, n_sel) == (int(gold[key + "/n_pseudo"]), int(gold[key + "/n_sel"])), key
            assert isinstance(n_ps, int) and t1.is_cuda and t1.shape == (S,) and t2.shape == (S,)
            assert _close(s.item(), gold[key + "/sum"]) and _close(score.cpu(), gold[key + "/score"]), key
            assert _close(t1.cpu(), gold[key + "/thr1"]) and _close(t2.cpu(), gold[key + "/thr2"]), key
        key = "%s/%s/thr" % (name, sw)
        s, n_ps, n_sel, score = JointPseudoLoss(S, RR.SCORE_THR)(p, t, _sw(sw))
        assert (n_ps, n_sel) == (int(gold[key + "/n_pseudo"]), int(gold[key + "/n_sel"])), key
        assert _close(s.item(), gold[key + "/sum"]) and _close(score.cpu(), gold[key + "/score"]), key
    # the default threshold of JointPseudoLoss is above every softmax score of maps in [0,1]
    assert JointPseudoLoss(S)(p, t, _sw("half"))[2] == 0
    # d preds against float64 autograd of the restatement
    for cls, arg, sel in ((JointPseudoLoss2, 0.5, ("rate", 0.5)), (JointPseudoLoss, RR.SCORE_THR, ("thr", RR.SCORE_THR))):
        leaf = p.clone().requires_grad_(True)
        ref_leaf = torch.from_numpy(preds).double().requires_grad_(True)
        ref = RR.pseudo_loss(ref_leaf, targets, RR.SW["half"], S, sel)
        assert ref["n_sel"] > 0
        _grad_check(cls(S, arg)(leaf, t, _sw("half"))[0], leaf, ref["sum"], ref_leaf)


def test_tie_keeps_both_tied_rows(gold):
    from ubpl_amd.losses import JointPseudoLoss2
    name = RR.TIE_CASE
    B, M, S, K = RR.CASES[name][:4]
    rate, rank = float(gold["tie/rate"]), int(gold["tie/rank"])
    preds, targets, _ = RR.make_case(name, tie=True)
    p, t = torch.from_numpy(preds).to(DEV), torch.from_numpy(targets).to(DEV)
    s, n_ps, n_sel, score, t1, t2 = JointPseudoLoss2(S, rate)(p, t, _sw("unlabeled"))
    assert (n_ps, n_sel) == (int(gold["tie/n_pseudo"]), int(gold["tie/n_sel"]))
    assert _close(s.item(), gold["tie/sum"]) and _close(t2.cpu(), gold["tie/thr2"])
    # the threshold is the tied value itself: both copies' target scores equal it bit for bit
    from ubpl_amd import kernels as Kn
    HW = preds.shape[-1] * preds.shape[-2]
    last = t.reshape(-1)[(S - 1) * K * HW:]
    tsc = Kn.softmax_peak_scores(last, S * K * HW, 0, B * S * K * HW, M, B, 1, K, HW).view(B, K)
    tied = (tsc == t2[0]).nonzero().tolist()
    assert len(tied) == 2 and {b for b, _ in tied} == {1, 3}
    assert int((tsc >= t2[0]).sum()) == B * K - rank + 1               # one more than the nominal share


@pytest.mark.parametrize("name", list(RR.CASES))
def test_dist_loss_mt_against_the_reference(gold, name):
    from ubpl_amd.losses import JointDistLoss_mt
    B, M, S, K = RR.CASES[name][:4]
    preds, _, preds2 = RR.make_case(name)
    gate = (np.random.RandomState(7).uniform(size=(B, K)) > 0.25).astype(np.float32)
    sw = torch.tensor(RR.SW["half"]).reshape(-1, 1) + 0.5
    p1, p2, g = (torch.from_numpy(a).to(DEV) for a in (preds, preds2, gate))
    for rate in RR.SEL_RATES:
        key = "%s/mt/r%s" % (name, rate)
        s, n = JointDistLoss_mt(S, True, True, rate)(p1, p2, g, sw.to(DEV))
        assert n == int(gold[key + "/count"]) and _close(s.item(), gold[key + "/sum"]), key
    a, b = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    ra, rb = (torch.from_numpy(x).double().requires_grad_(True) for x in (preds, preds2))
    ref = RR.dist_loss_mt(ra, rb, gate, sw, S, True, True, 0.5)
    _grad_check(JointDistLoss_mt(S, True, True, 0.5)(a, b, g, sw.to(DEV))[0], a, ref["sum"], ra)
    assert float((b.grad.cpu().double() - rb.grad).abs().max()) <= TOL * float(rb.grad.abs().max())
    # without gate and weights: the count is nStack * B * K
    s, n = JointDistLoss_mt(S, selRate=0.5)(p1, p2)
    ref = RR.dist_loss_mt(preds, preds2, None, None, S, False, False, 0.5)
    assert n == S * B * K and _close(s.item(), float(ref["sum"]))


def test_raises():
    from ubpl_amd.losses import JointDistLoss_mt, JointPseudoLoss, JointPseudoLoss2
    name = "s2k17_12"
    S = RR.CASES[name][2]
    preds, targets, preds2 = RR.make_case(name)
    p, t, p2 = (torch.from_numpy(a).to(DEV) for a in (preds, targets, preds2))
    for mod in (JointPseudoLoss2(S, 0.5), JointPseudoLoss(S, RR.SCORE_THR)):
        with pytest.raises(RuntimeError, match="non-empty TensorList"):
            mod(p, t, _sw("labeled"))
    for rate in (0, 0.0, -0.5):
        with pytest.raises(IndexError):
            JointPseudoLoss2(S, rate)(p, t, _sw("half"))
        with pytest.raises(IndexError):
            JointDistLoss_mt(S, selRate=rate)(p, p2)


def test_drop_in_import(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(HERE), "ubpl-poseestimation_amd", "dropin"))
    for m in [m for m in sys.modules if m.split(".")[0] == "utils"]:
        monkeypatch.delitem(sys.modules, m)
    try:
        from utils.losses import JointDistLoss_mt, JointPseudoLoss, JointPseudoLoss2
        name = "s2k17_12"
        S = RR.CASES[name][2]
        preds, targets, preds2 = RR.make_case(name)
        p, t, p2 = (torch.from_numpy(a).to(DEV) for a in (preds, targets, preds2))
        assert len(JointPseudoLoss(S, RR.SCORE_THR)(p, t, _sw("half"))) == 4
        assert len(JointPseudoLoss2(S, 0.5)(p, t, _sw("half"))) == 6
        assert len(JointDistLoss_mt(S)(p, p2)) == 2
    finally:
        for m in [m for m in sys.modules if m.split(".")[0] == "utils"]:
            sys.modules.pop(m, None)
