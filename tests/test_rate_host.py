"""The rate-based and softmax-score pseudo-label losses, host side: the float64 restatement
(tests/rate_ref.py) against the reference's own outputs (tests/golden/rate_losses.npz), the
separation condition of every fixture case, the "rate" rule's options, the host rank expression, the
record layout and the header.  Nothing here touches a device."""
import os
import types

import numpy as np
import pytest
import torch

import rate_ref as RR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rate_losses.npz")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def _check_pseudo(gold, key, res, S):
    assert (res["n_pseudo"], res["n_sel"]) == (int(gold[key + "/n_pseudo"]), int(gold[key + "/n_sel"])), key
    assert np.array_equal((res["mask1"] * res["mask2"]).numpy(), gold[key + "/mask"]), key
    want = float(gold[key + "/sum"])
    assert abs(float(res["sum"]) - want) <= 1e-6 * abs(want), key
    assert np.allclose(res["score"].numpy(), gold[key + "/score"], rtol=1e-6, atol=0), key
    if key + "/thr1" in gold:
        assert np.allclose(res["thr1"].numpy(), gold[key + "/thr1"].reshape(S), rtol=1e-6, atol=0), key
        assert np.allclose(res["thr2"].numpy(), gold[key + "/thr2"].reshape(S), rtol=1e-6, atol=0), key


@pytest.mark.parametrize("name", list(RR.CASES))
def test_restatement_reproduces_the_reference(gold, name):
    B, M, S, K = RR.CASES[name][:4]
    preds, targets, preds2 = RR.make_case(name)
    for sw in ("half", "unlabeled"):
        for sel in [("rate", r) for r in RR.SEL_RATES] + [("thr", RR.SCORE_THR)]:
            res = RR.pseudo_loss(preds, targets, RR.SW[sw], S, sel)
            RR.assert_separated(res)                                   # masks and counts compare exactly
            key = "%s/%s/%s" % (name, sw, "thr" if sel[0] == "thr" else "r%s" % sel[1])
            _check_pseudo(gold, key, res, S)
            if sel == ("rate", 1.0):                                   # rank 0: every row reaches the minimum
                assert res["n_sel"] == S * B * K
    for sel in (("rate", 0.5), ("thr", RR.SCORE_THR)):
        with pytest.raises(RuntimeError, match="non-empty TensorList"):
            RR.pseudo_loss(preds, targets, RR.SW["labeled"], S, sel)
    with pytest.raises(IndexError):
        RR.pseudo_loss(preds, targets, RR.SW["half"], S, ("rate", 0.0))
    gate = (np.random.RandomState(7).uniform(size=(B, K)) > 0.25).astype(np.float32)
    sw = torch.tensor(RR.SW["half"]).reshape(-1, 1) + 0.5
    for rate in RR.SEL_RATES:
        res = RR.dist_loss_mt(preds, preds2, gate, sw, S, True, True, rate)
        RR.assert_separated(res, (("score2", "thr2"),))
        key = "%s/mt/r%s" % (name, rate)
        want = float(gold[key + "/sum"])
        assert res["count"] == int(gold[key + "/count"]) == S * int(gate.sum())
        assert abs(float(res["sum"]) - want) <= 1e-6 * abs(want), key


def test_tie_selects_both_tied_rows(gold):
    name = RR.TIE_CASE
    B, M, S, K = RR.CASES[name][:4]
    rate, rank = RR.tie_rate(name)
    assert (rate, rank) == (float(gold["tie/rate"]), int(gold["tie/rank"]))
    preds, targets, _ = RR.make_case(name, tie=True)
    res = RR.pseudo_loss(preds, targets, RR.SW["unlabeled"], S, ("rate", rate))
    RR.assert_separated(res)
    _check_pseudo(gold, "tie", res, S)
    s2, t2 = res["score2"][0], res["thr2"][0]
    tied = (s2 == t2).nonzero().tolist()
    assert len(tied) == 2 and {b for b, _ in tied} == {1, 3} and tied[0][1] == tied[1][1]   # the two copies
    assert all(res["mask2"][0][b, k] == 1 for b, k in tied)
    nominal = B * K - rank
    assert int(res["mask2"][0].sum()) == nominal + 1                   # one row more than the share


def test_host_rank_expression():
    from ubpl_amd.losses import sel_rank
    assert int(10 * (1 - 0.9)) == 0                                    # Python floats: 0.0999..., not 1
    for n, r in ((10, 0.9), (64, 0.5), (64, 0.3), (68, 0.9), (512, 0.5), (64, 1.0), (64, 0.0), (7, 1e-9)):
        assert sel_rank(n, r) == int(n * (1 - r)) == RR.rank_of(n, r)
    assert sel_rank(10, 0.9) == 0 and sel_rank(64, 1.0) == 0 and sel_rank(64, 0.0) == 64


def _args(**kw):
    return types.SimpleNamespace(pseudoScoreThr=0.9, **kw)


def test_rate_rule_options():
    from ubpl_amd import view_gate as VG
    assert "rate" in VG.RULES
    o = VG.GateOptions(_args(pseudoRule="rate", pseudoSelRate=0.5))
    assert o.sel_rate == 0.5 and not o.on                              # not the view gate
    assert VG.GateOptions(_args(pseudoRule="rate", pseudoSelRate=1)).sel_rate == 1.0
    assert VG.GateOptions(_args()).sel_rate is None
    assert VG.GateOptions(_args(pseudoRule="score", pseudoSelRate=0.5)).sel_rate is None
    assert VG.GateOptions(_args(pseudoRule="uncertainty", distThrMax=4)).sel_rate is None
    with pytest.raises(ValueError, match="needs pseudoSelRate"):
        VG.GateOptions(_args(pseudoRule="rate"))
    for bad in (0, 0.0, 1.5, -0.5, "0.5", float("nan"), True, [0.5]):
        with pytest.raises(ValueError, match="float in \\(0, 1\\]"):
            VG.options(_args(pseudoRule="rate", pseudoSelRate=bad))
    a1, a2 = _args(pseudoRule="rate", pseudoSelRate=0.5), _args(pseudoRule="rate", pseudoSelRate=0.5)
    assert VG.options(a1) is VG.options(a2)
    assert VG.options(a1) is not VG.options(_args(pseudoRule="rate", pseudoSelRate=0.25))
    for where in ("train_dualpose_ubpl", "train_mt", "train_supervised"):
        with pytest.raises(ValueError, match="train_mt_ubpl only"):
            VG.refuse(a1, where)
    VG.refuse(_args(), "train_mt")


def test_steps_refuse_the_rule_before_touching_their_arguments():
    from ubpl_amd import train as T
    args = _args(pseudoRule="rate", pseudoSelRate=0.5)
    with pytest.raises(ValueError, match="train_mt_ubpl only"):
        T.train_supervised([], None, None, args)
    with pytest.raises(ValueError, match="train_mt_ubpl only"):
        T.train_mt([], None, None, None, args)


def test_record_layout_gains_a_block_only_with_the_rule():
    from ubpl_amd.step_losses import _RecordLayout
    counts = ("pec_n", "epc_n", "n_sel")
    off, on = _RecordLayout(2, counts, 2, 16), _RecordLayout(2, counts, 2, 16, rate_thr=True)
    assert off.rate_thr is None and off.size == 7 + 8 + 16
    assert on.size == off.size + 4 and on.rate_thr == slice(off.size, off.size + 4)
    assert on.scores() == off.scores() and on.fdl_n == off.fdl_n and on.n("n_sel", 1) == off.n("n_sel", 1)


def test_header_declares_the_entries():
    from ubpl_amd import _abi, _lib
    decls = {name: (params, ann) for _, name, params, ann in _abi.parse(open(_lib.HEADER_PATH).read())}
    for name, ptrs in (("ubpl_softmax_peak_scores", {"x", "score"}), ("ubpl_rank_threshold", {"scores", "thr"}),
                       ("ubpl_loss_finalize_ranked", {"sq_mean", "ascore", "tscore", "athr", "tthr", "gate", "sw",
                                                      "out_sum", "out_cnt", "out_score", "out_w"}),
                       ("ubpl_loss_finalize_rank", {"sq_mean", "ascore", "tscore", "gate", "sw", "thr", "out_sum",
                                                    "out_cnt", "out_score", "out_w"})):
        params, ann = decls[name]
        assert set(ann) == ptrs and params[-1] == ("void*", "stream")
    assert decls["ubpl_loss_finalize_ranked"][1]["athr"] == ("f32", "S")


def test_drop_in_exports_the_classes(monkeypatch):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.syspath_prepend(os.path.join(root, "ubpl-poseestimation_amd", "dropin"))
    for name in [m for m in sys.modules if m.split(".")[0] == "utils"]:
        monkeypatch.delitem(sys.modules, name)
    try:
        from utils.losses import JointDistLoss_mt, JointPseudoLoss, JointPseudoLoss2
        from ubpl_amd import losses as L
        assert (JointPseudoLoss, JointPseudoLoss2, JointDistLoss_mt) == (L.JointPseudoLoss, L.JointPseudoLoss2,
                                                                        L.JointDistLoss_mt)
        assert (JointPseudoLoss().scoreThr, JointPseudoLoss2().selRate, JointDistLoss_mt().selRate) == (0.8, 0.5, 0.5)
        assert (JointPseudoLoss2(2, 0.3).nStack, JointDistLoss_mt(2, True, True, 0.3).useKPsGate) == (2, True)
    finally:
        for name in [m for m in sys.modules if m.split(".")[0] == "utils"]:
            sys.modules.pop(name, None)
