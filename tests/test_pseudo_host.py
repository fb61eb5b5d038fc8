"""CPU-only checks of the ensemble pseudo-label layer: the torch restatement the GPU
tests compare the kernel with (pinned here to the reference-derived
oracle.losses.joint_pseudo3), the JSON round trip, the rule names and the kps layout."""
import math
import os

import pytest
import torch

from oracle import decode as OD
from oracle import losses as OL

HOST_SHAPES = [(2, 3, 9, 32, 32), (1, 1, 1, 4, 4), (3, 2, 17, 5, 7), (8, 1, 2, 8, 8), (2, 2, 16, 64, 64)]


def restate_pseudo(p, thr, center=None, scale=None, res=None):
    """JointPseudoLoss3's target and mask (utils/losses.py:176-210) from the members'
    heatmaps p [M,N,K,H,W] (float32, host), every member in the student's place in turn.
    T is the sequential float32 sum in member order over float32 M; disagree is float64
    from that float32 T."""
    M, N, K, H, W = p.shape
    T = p[0].clone()
    for m in range(1, M):
        T = T + p[m]
    T = T / torch.tensor(float(M), dtype=torch.float32)               # targets.mean(0) (:179)
    t32 = torch.tensor(thr, dtype=torch.float32)
    out = {"mean_hm": T, "ens_raw": OD.get_preds(T), "ens_preds": None,
           "ens_score": T.reshape(N, K, -1).max(-1).values,
           "member_score": p.reshape(M, N, K, -1).max(-1).values}     # s1 of :187
    if center is not None:
        out["ens_preds"] = OD.kps_from_heatmap(T, center, scale, [H, W] if res is None else res)[0]
    out["disagree"] = ((p.double() - T.double()[None]) ** 2).reshape(M, N, K, -1).mean(-1)   # :184
    out["select"] = (out["member_score"] >= t32).float() * (out["ens_score"] >= t32).float()[None]  # :187-193
    return out


def member_maps(M, N, K, H, W, seed=0):
    """M members' heatmaps of N*K joints: per joint one shared peak location over a low
    background, per member its own noise, and per map its own amplitude from [0.3, 1.2], so
    that the maps' peaks straddle a threshold between."""
    gen = torch.Generator().manual_seed(1000 * seed + 97 * M + 13 * N + 7 * K + W)
    base = torch.rand(N, K, H * W, generator=gen) * 0.5
    peak = torch.randint(0, H * W, (N, K, 1), generator=gen)
    base.scatter_(2, peak, 1.0)
    noise = (torch.rand(M, N, K, H * W, generator=gen) - 0.5) * 0.1
    amp = 0.3 + 0.9 * torch.rand(M, N, K, 1, generator=gen)
    return ((base[None] + noise) * amp).reshape(M, N, K, H, W).contiguous()


@pytest.mark.parametrize("thr", [0.5, 0.75])
def test_restatement_is_joint_pseudo3(thr):
    """Member m as the student: n_sel and the masked loss sum of the reference-pinned
    joint_pseudo3 are the restatement's select[m] and disagree[m].  A case of one or two
    joints can fall on one side of the threshold as a whole; over the cases, and within
    every case of six joints or more, both classes occur."""
    seen = set()
    for M, B, K, H, W in HOST_SHAPES:
        p = member_maps(M, B, K, H, W)
        r = restate_pseudo(p, thr)
        assert torch.equal(r["mean_hm"], p.mean(0)), (M, B, K, H, W)
        scores = torch.cat([r["member_score"].reshape(-1), r["ens_score"].reshape(-1)])
        assert float((scores - thr).abs().min()) > 1e-5           # the oracle's rounding flips no mask
        classes = set(r["select"].reshape(-1).tolist())
        assert classes <= {0.0, 1.0}
        if B * K >= 6:
            assert classes == {0.0, 1.0}, (M, B, K, H, W)
        seen |= classes
        for m in range(M):
            loss_sum, _, n_sel, _, _, _ = OL.joint_pseudo3(p[m], p, torch.ones(B, 1), 1, thr)
            assert n_sel == int(r["select"][m].sum()), (M, B, K, H, W, m)
            want = float((r["disagree"][m] * r["select"][m]).sum())
            assert abs(float(loss_sum) - want) <= 1e-4 * abs(want), (M, B, K, H, W, m, float(loss_sum), want)
    assert seen == {0.0, 1.0}


def test_restatement_edges():
    """>= selects at the threshold itself, a NaN score never does, and one member is its own mean."""
    p = torch.zeros(2, 1, 3, 4, 4)
    p[:, 0, 0, 1, 2] = 0.5                                         # every peak == thr
    p[0, 0, 1, 0, 0] = 0.9
    p[1, 0, 1, 0, 0] = 0.1 - 1e-3                                  # T's peak just under thr
    p[:, 0, 2, 3, 3] = 0.9
    p[1, 0, 2, 0, 1] = float("nan")
    r = restate_pseudo(p, 0.5)
    assert r["select"][:, 0, 0].tolist() == [1.0, 1.0] and r["ens_raw"][0, 0].tolist() == [3.0, 2.0]
    assert r["select"][:, 0, 1].tolist() == [0.0, 0.0]
    assert math.isnan(float(r["ens_score"][0, 2])) and r["select"][:, 0, 2].tolist() == [0.0, 0.0]
    one = member_maps(1, 2, 3, 5, 7)
    r = restate_pseudo(one, 0.5)
    assert torch.equal(r["mean_hm"], one[0]) and float(r["disagree"].abs().max()) == 0.0


def test_pseudo_data_round_trip(tmp_path):
    from ubpl_amd import checkpoint as C
    d = {"predsArraies": [[[12.0, 7.0], [3.0, 4.0]], [[1.0, 1.0], [90.0, 64.0]]],
         "selected": [[True, False], [False, False]], "ens_score": [[0.97, 0.25], [0.5, 0.125]],
         "spread": [[0.0, math.sqrt(2.0)], [1.0, 5.0]],
         "disagree": [[[1e-4, 2e-3], [1e-4, 2e-3]], [[0.5, 0.25], [0.5, 0.25]]],
         "thr": 0.95, "rule": "unanimous", "selected_fraction": [0.5, 0.0]}
    path = C.save_pseudo_data(d, str(tmp_path / "sub" / "pseudo.json"))
    assert os.path.exists(path)
    assert C.load_pseudo_data(path) == d
    with pytest.raises(ValueError, match="predsArraies"):
        C.save_pseudo_data({"selected": []}, str(tmp_path / "bad.json"))
    (tmp_path / "other.json").write_text('{"selected": []}')
    with pytest.raises(ValueError, match="predsArraies"):
        C.load_pseudo_data(str(tmp_path / "other.json"))


def test_rule_names_and_kps_layout():
    from ubpl_amd import predict as P
    assert P.check_rule("unanimous") == "unanimous" and P.check_rule("ensemble") == "ensemble"
    for bad in ("any", "", None, "Unanimous"):
        with pytest.raises(ValueError, match="rule is one of"):
            P.check_rule(bad)
    preds = torch.tensor([[[10.0, 20.0], [30.0, 40.0]]])
    kps = P.assemble_kps(preds, torch.tensor([[True, False]]))
    assert kps.dtype == torch.float32 and kps.tolist() == [[[10.0, 20.0, 1.0], [30.0, 40.0, 0.0]]]


def test_ensemble_pseudo_op_checks_arguments_before_the_call():
    from ubpl_amd import _lib
    if not os.path.exists(_lib.OPS_PATH):
        pytest.skip("libubpl_ops.so not built (run __graft_entry__.build())")
    ops = _lib.load_ops()
    M, N, K, H, W = 3, 2, 3, 4, 5
    S = 2
    sb, last = S * K * H * W, (S - 1) * K * H * W
    sm = N * sb
    hm = torch.zeros(M * sm)[last:]
    assert hm.numel() == (M - 1) * sm + (N - 1) * sb + K * H * W   # exactly what the strided maps need
    a = {"hm": hm, "sm": sm, "sb": sb, "M": M, "N": N, "K": K, "H": H, "W": W,
         "tinv": torch.zeros(N * 6, dtype=torch.float64), "thr": torch.zeros(1),
         "mean_hm": torch.zeros(N * K * H * W), "ens_raw": torch.zeros(N * K * 2), "ens_preds": torch.zeros(N * K * 2),
         "ens_score": torch.zeros(N * K), "member_score": torch.zeros(M * N * K), "disagree": torch.zeros(M * N * K),
         "select": torch.zeros(M * N * K)}
    call = lambda **kw: ops.ensemble_pseudo(*[kw.get(n, v) for n, v in a.items()])
    with pytest.raises(RuntimeError, match="hm holds %d elements" % (hm.numel() - 1)):
        call(hm=hm[1:])
    with pytest.raises(RuntimeError, match="thr holds 0 elements"):
        call(thr=torch.zeros(0))
    with pytest.raises(RuntimeError, match="tinv must be f64"):
        call(tinv=a["tinv"].float())
    with pytest.raises(RuntimeError, match="mean_hm holds"):
        call(mean_hm=a["mean_hm"][1:])
    for name in ("member_score", "disagree", "select"):
        with pytest.raises(RuntimeError, match="%s holds %d elements" % (name, M * N * K - 1)):
            call(**{name: a[name][1:]})
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        call()                                                     # every check passes: refused on CPU
