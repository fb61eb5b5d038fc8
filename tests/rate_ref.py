"""A float64 restatement of the reference's softmax-score pseudo-label losses, written from
utils/losses.py: JointPseudoLoss (:73-115), JointPseudoLoss2 (:118-166), JointDistLoss_mt (:213-243).
It returns the masks and scores beside the reference's tuple, and takes torch tensors so that
autograd gives the gradient.  Also here: the seeded inputs the fixture (tests/golden/rate_losses.npz,
written by gen_rate_golden.py from the reference's own classes) and the tests share, and the
separation condition under which masks and counts are compared exactly."""
import numpy as np
import torch

SEP = 1e-5                      # no score within this (relative) of its threshold, planted ties aside
SEL_RATES = (0.3, 0.5, 0.9, 1.0)
SCORE_THR = 0.11                # JointPseudoLoss: between the scores of the planted heights
# name -> (B, M, S, K, H, W, seed)
CASES = {
    "s1k16": (4, 2, 1, 16, 64, 64, 11),
    "s2k16": (4, 2, 2, 16, 64, 64, 12),
    "s1k17": (4, 2, 1, 17, 64, 64, 13),
    "s2k17": (4, 2, 2, 17, 64, 64, 14),
    "s2k17_12": (4, 2, 2, 17, 12, 12, 15),
}
TIE_CASE = "s2k16"              # its tie variant: sample 3 duplicates sample 1
SW = {"half": [0.0, 0.0, 1.0, 1.0], "unlabeled": [1.0, 1.0, 1.0, 1.0], "labeled": [0.0, 0.0, 0.0, 0.0]}


def rank_of(n, sel_rate):
    """The reference's index (:139), in Python floats: int(10 * (1 - 0.9)) is 0."""
    return int(n * (1 - sel_rate))


def _peaks(rs, heights, H, W):
    """[len(heights), H, W] float64: one Gaussian peak (sigma 1.5 px) of each height at a random cell."""
    n = len(heights)
    cy, cx = rs.randint(2, H - 2, n), rs.randint(2, W - 2, n)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = (yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2
    return heights[:, None, None] * np.exp(-d2 / (2 * 1.5 ** 2))


def make_case(name, tie=False):
    """-> (preds [B,S,K,H,W] (S == 1: [B,K,H,W]), targets [M,B,S,K,H,W] ([M,B,K,H,W]), preds2 like
    preds) float32 numpy.  Every map is a peak of a planted height, the B*K heights of an input
    distinct and 0.01 apart, plus N(0, 0.01^2) noise.  tie: sample 3 is a copy of sample 1 in every
    input, so its K scores tie bit for bit."""
    B, M, S, K, H, W, seed = CASES[name]
    rs = np.random.RandomState(seed)
    n = B * K

    def maps():
        h = 0.30 + 0.01 * rs.permutation(n)
        return _peaks(rs, h, H, W).reshape(B, K, H, W)

    preds = np.stack([maps() + rs.normal(0, 0.01, (B, K, H, W)) for _ in range(S)], 1)
    preds2 = np.stack([maps() + rs.normal(0, 0.01, (B, K, H, W)) for _ in range(S)], 1)
    last = maps()
    targets = np.stack([np.stack([(maps() if s < S - 1 else last) + rs.normal(0, 0.01, (B, K, H, W))
                                  for s in range(S)], 1) for _ in range(M)])
    if tie:
        preds[3], preds2[3], targets[:, 3] = preds[1], preds2[1], targets[:, 1]
    if S == 1:
        preds, preds2, targets = preds[:, 0], preds2[:, 0], targets[:, :, 0]
    return preds.astype(np.float32), targets.astype(np.float32), preds2.astype(np.float32)


def scores_of(v):
    """v [B,K,P] -> [B,K]: softmax across the keypoint axis at every pixel, then the per-map maximum."""
    return torch.softmax(v, dim=-2).max(dim=-1)[0]


def _rows(x, n_stack, i):
    bs = x.shape[0]
    k = x.shape[1] if n_stack == 1 else x.shape[2]
    return (x if n_stack == 1 else x[:, i]).reshape(bs, k, -1)


def _threshold(score, sel):
    if sel[0] == "thr":
        return torch.tensor(sel[1], dtype=score.dtype)
    flat = score.reshape(-1)
    return torch.sort(flat, dim=0)[0][rank_of(len(flat), sel[1])]       # IndexError for selRate <= 0


def pseudo_loss(preds, targets, sw, n_stack, sel, dtype=torch.float64):
    """JointPseudoLoss (sel = ("thr", scoreThr)) / JointPseudoLoss2 (sel = ("rate", selRate)).
    -> dict: sum, n_pseudo, n_sel, score [K], thr1 [S], thr2 [S], and per stack [S,B,K]: score1,
    score2, mask1, mask2.  preds may require grad; targets are detached."""
    preds = torch.as_tensor(preds).to(dtype)
    targets = torch.as_tensor(targets).to(dtype).detach()
    sw = torch.as_tensor(sw).to(dtype).reshape(-1, 1)
    tmean = (targets if n_stack == 1 else targets[:, :, -1]).mean(0)
    out = {k: [] for k in ("score1", "score2", "mask1", "mask2", "thr1", "thr2")}
    total, n_pseudo, n_sel, joint = 0.0, 0, 0, []
    for i in range(n_stack):
        v1 = _rows(preds, n_stack, i)
        v2 = tmean.reshape(v1.shape[0], v1.shape[1], -1)
        loss = ((v1 - v2) ** 2).mean(-1) * sw
        s1, s2 = scores_of(v1.detach()), scores_of(v2)
        t1, t2 = _threshold(s1, sel), _threshold(s2, sel)
        m1, m2 = (s1 >= t1).to(dtype), (s2 >= t2).to(dtype)
        n_pseudo += int((loss > 0).sum())
        n_sel += int((m1 * m2 > 0).sum())
        rows = sw.reshape(-1) > 0
        if not rows.any():
            raise RuntimeError("stack expects a non-empty TensorList")
        joint.append((s1[rows].mean(0) + s2[rows].mean(0)) / 2)
        total = total + (loss * m1 * m2).sum()
        for k, v in zip(("score1", "score2", "mask1", "mask2", "thr1", "thr2"), (s1, s2, m1, m2, t1, t2)):
            out[k].append(v)
    out = {k: torch.stack(v) for k, v in out.items()}
    out.update(sum=total, n_pseudo=n_pseudo, n_sel=n_sel, score=torch.stack(joint).mean(0))
    return out


def dist_loss_mt(preds1, preds2, gate, sw, n_stack, use_gate, use_sw, sel_rate, dtype=torch.float64):
    """JointDistLoss_mt -> dict: sum, count, and per stack [S,B,K]: score2, mask2, thr2 [S]."""
    p1, p2 = torch.as_tensor(preds1).to(dtype), torch.as_tensor(preds2).to(dtype)
    bs = p1.shape[0]
    k = p1.shape[1] if n_stack == 1 else p1.shape[2]
    g = torch.ones(bs, k, dtype=dtype) if gate is None else torch.as_tensor(gate).to(dtype)
    out = {k_: [] for k_ in ("score2", "mask2", "thr2")}
    total = 0.0
    for i in range(n_stack):
        v1, v2 = _rows(p1, n_stack, i), _rows(p2, n_stack, i)
        loss = ((v1 - v2) ** 2).mean(-1)
        if use_gate:
            loss = loss * g
        if use_sw and sw is not None:
            loss = loss * torch.as_tensor(sw).to(dtype).reshape(-1, 1)
        s2 = scores_of(v2.detach())
        t2 = _threshold(s2, ("rate", sel_rate))
        m2 = (s2 >= t2).to(dtype)
        total = total + (loss * m2).sum()
        for k_, v in zip(("score2", "mask2", "thr2"), (s2, m2, t2)):
            out[k_].append(v)
    out = {k_: torch.stack(v) for k_, v in out.items()}
    out.update(sum=total, count=n_stack * int((g > 0).sum()))
    return out


def separation(score, thr):
    """The smallest relative distance |s - thr| / thr over the scores of one stack that differ from
    thr (a score equal to it is the threshold itself or a planted duplicate of it)."""
    s = np.asarray(score, np.float64).reshape(-1)
    t = float(thr)
    d = np.abs(s[s != t] - t) / abs(t)
    return float(d.min()) if d.size else float("inf")


def assert_separated(res, keys=(("score1", "thr1"), ("score2", "thr2"))):
    """The separation condition on a pseudo_loss / dist_loss_mt result (float64)."""
    for sk, tk in keys:
        for i in range(res[sk].shape[0]):
            sep = separation(res[sk][i].numpy(), res[tk][i])
            assert sep >= SEP, "%s stack %d: a score lies %.3g relative from its threshold" % (sk, i, sep)


def tie_rate(name):
    """For the tie variant of case `name`: a selRate whose rank lands on the second of two equal
    target scores, so the threshold is a tied value and one row more than the nominal share
    reaches it -> (selRate, rank)."""
    B, M, S, K = CASES[name][:4]
    preds, targets, _ = make_case(name, tie=True)
    res = pseudo_loss(preds, targets, SW["unlabeled"], S, ("rate", 1.0))
    flat = torch.sort(res["score2"][0].reshape(-1))[0]
    n = len(flat)
    for r in range(n // 4, n):
        if flat[r] == flat[r - 1]:
            rate = 1.0 - (r + 0.5) / n
            assert rank_of(n, rate) == r
            return rate, r
    raise AssertionError("no tied pair in the upper three quarters of the scores")
