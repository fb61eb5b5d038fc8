"""Generate tests/golden/rate_losses.npz by running the REFERENCE's own JointPseudoLoss,
JointPseudoLoss2 and JointDistLoss_mt (utils/losses.py:73-166, 213-243).

TEST INFRASTRUCTURE ONLY, as gen_golden.py (whose import recipe this uses): it runs where the
reference tree is present and writes a fixture; the tests read the fixture alone.  Outputs only are
stored: the tests regenerate the inputs from rate_ref.make_case's seeds.

Per case of rate_ref.CASES and sample-weight pattern ("half", "unlabeled"; "labeled" must raise):
  JointPseudoLoss2 at every rate_ref.SEL_RATES -> <case>/<sw>/r<rate>/{sum,n_pseudo,n_sel,score,thr1,thr2,mask}
  JointPseudoLoss at rate_ref.SCORE_THR        -> <case>/<sw>/thr/{sum,n_pseudo,n_sel,score,mask}
  JointDistLoss_mt (gate and sample weight on) -> <case>/mt/r<rate>/{sum,count}
and the tie variant of rate_ref.TIE_CASE at rate_ref.tie_rate               -> tie/{...,rate,rank}.
mask [S,B,K] is score1 >= thr1 and score2 >= thr2 with the class's own float32 expressions and the
thresholds it returned.  The separation condition (rate_ref.SEP) is asserted on the float64
restatement of every case: a seed that fails it is replaced in rate_ref.CASES, not excluded.

Usage:  python tests/golden/gen_rate_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden  # noqa: E402


def _mask(RR, preds, targets, n_stack, thr1, thr2):
    p, t = torch.from_numpy(preds), torch.from_numpy(targets)
    tmean = (t if n_stack == 1 else t[:, :, -1]).mean(0)
    out = []
    for i in range(n_stack):
        v1 = RR._rows(p, n_stack, i)
        v2 = tmean.reshape(v1.shape[0], v1.shape[1], -1)
        out.append((RR.scores_of(v1).ge(thr1[i]).float() * RR.scores_of(v2).ge(thr2[i]).float()).numpy())
    return np.stack(out)


def _gate(B, K, seed):
    return (np.random.RandomState(seed).uniform(size=(B, K)) > 0.25).astype(np.float32)


def main():
    R = gen_golden.import_reference()
    L = R["L"]
    import rate_ref as RR
    out, worst = {}, {"sep": np.inf, "f32": 0.0}

    def pseudo(key, preds, targets, S, sw, sel):
        swt = torch.tensor(RR.SW[sw]).reshape(-1, 1)
        ref64 = RR.pseudo_loss(preds, targets, RR.SW[sw], S, sel)
        RR.assert_separated(ref64)
        worst["sep"] = min(worst["sep"], *(RR.separation(ref64[s][i].numpy(), ref64[t][i])
                                           for s, t in (("score1", "thr1"), ("score2", "thr2")) for i in range(S)))
        p, t = torch.from_numpy(preds), torch.from_numpy(targets)
        if sel[0] == "rate":
            s, n_ps, n_sel, score, t1, t2 = L.JointPseudoLoss2(S, sel[1])(p, t, swt)
            out[key + "/thr1"], out[key + "/thr2"] = t1.numpy(), t2.numpy()
        else:
            s, n_ps, n_sel, score = L.JointPseudoLoss(S, sel[1])(p, t, swt)
            t1 = t2 = torch.full((S,), sel[1])
        out[key + "/sum"], out[key + "/score"] = s.numpy(), score.numpy()
        out[key + "/n_pseudo"], out[key + "/n_sel"] = np.int64(n_ps), np.int64(n_sel)
        out[key + "/mask"] = _mask(RR, preds, targets, S, t1, t2)
        # the reference's own float32 against the float64 statement
        assert (n_ps, n_sel) == (ref64["n_pseudo"], ref64["n_sel"]), key
        assert np.array_equal(out[key + "/mask"], (ref64["mask1"] * ref64["mask2"]).numpy()), key
        assert abs(float(s) - float(ref64["sum"])) <= 1e-6 * abs(float(ref64["sum"])), key
        worst["f32"] = max(worst["f32"], float(((score.double() - ref64["score"]).abs() / ref64["score"]).max()))

    for name, (B, M, S, K, H, W, _) in RR.CASES.items():
        preds, targets, preds2 = RR.make_case(name)
        for sw in ("half", "unlabeled"):
            for rate in RR.SEL_RATES:
                pseudo("%s/%s/r%s" % (name, sw, rate), preds, targets, S, sw, ("rate", rate))
            pseudo("%s/%s/thr" % (name, sw), preds, targets, S, sw, ("thr", RR.SCORE_THR))
        for cls, arg in ((L.JointPseudoLoss2, 0.5), (L.JointPseudoLoss, RR.SCORE_THR)):
            try:
                cls(S, arg)(torch.from_numpy(preds), torch.from_numpy(targets),
                            torch.tensor(RR.SW["labeled"]).reshape(-1, 1))
                raise AssertionError("no labeled-only raise")
            except RuntimeError:
                pass
        gate, swt = _gate(B, K, 7), torch.tensor(RR.SW["half"]).reshape(-1, 1) + 0.5
        for rate in RR.SEL_RATES:
            s, n = L.JointDistLoss_mt(S, True, True, rate)(torch.from_numpy(preds), torch.from_numpy(preds2),
                                                            torch.from_numpy(gate), swt)
            ref64 = RR.dist_loss_mt(preds, preds2, gate, swt, S, True, True, rate)
            RR.assert_separated(ref64, (("score2", "thr2"),))
            assert n == ref64["count"] and abs(float(s) - float(ref64["sum"])) <= 1e-6 * abs(float(ref64["sum"]))
            key = "%s/mt/r%s" % (name, rate)
            out[key + "/sum"], out[key + "/count"] = s.numpy(), np.int64(n)
    rate, rank = RR.tie_rate(RR.TIE_CASE)
    preds, targets, _ = RR.make_case(RR.TIE_CASE, tie=True)
    pseudo("tie", preds, targets, RR.CASES[RR.TIE_CASE][2], "unlabeled", ("rate", rate))
    out["tie/rate"], out["tie/rank"] = np.float64(rate), np.int64(rank)
    print("closest score to a threshold: %.3g relative; reference f32 scores vs float64: %.3g relative"
          % (worst["sep"], worst["f32"]))
    path = os.path.join(HERE, "rate_losses.npz")
    np.savez_compressed(path, **out)
    print("%s: %d keys, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
