"""ubpl_softmax_peak_scores, ubpl_rank_threshold and ubpl_loss_finalize_ranked on the device,
against float64 (tests/rate_ref.py), torch.sort of the same device tensor, and a numpy statement of
the finalize."""
import numpy as np
import pytest
import torch

import rate_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCORE_CASES = ("s1k16", "s2k17", "s2k17_12")              # both plane sizes, both K


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _stacked(name):
    """preds [B,S,K,H,W], targets [M,B,S,K,H,W] of a case (a stack axis also where S == 1)."""
    S = RR.CASES[name][2]
    preds, targets, _ = RR.make_case(name)
    return (preds[:, None], targets[:, :, None]) if S == 1 else (preds, targets)


def _ref64(maps):
    """maps [..., K, H, W] float -> float64 scores [..., K]."""
    v = torch.from_numpy(np.asarray(maps)).double()
    return RR.scores_of(v.reshape(v.shape[:-2] + (-1,))).numpy()


def _f32(maps):
    v = torch.from_numpy(np.asarray(maps, np.float32))
    return torch.softmax(v.reshape(v.shape[:-2] + (-1,)), dim=-2).max(dim=-1)[0].double().numpy()


_BAR = {}


def _bar():
    """4 x the maximum relative error of torch's own float32 softmax-then-max on the CPU against
    float64, over the inputs of every case here (the member mean adds one rounding, and the device's
    expf may differ from the CPU's by an ulp or two)."""
    if not _BAR:
        worst = 0.0
        for name in SCORE_CASES:
            preds, targets = _stacked(name)
            tmean32 = torch.from_numpy(targets).mean(0).numpy()
            for m32, m64 in ((preds, preds), (tmean32, targets.astype(np.float64).mean(0))):
                ref = _ref64(m64)
                worst = max(worst, float((np.abs(_f32(m32) - ref) / ref).max()))
        _BAR["cpu"] = worst
        print("torch float32 on the CPU vs float64: max relative error %.3e -> bar %.3e" % (worst, 4 * worst))
    return 4 * _BAR["cpu"]


@pytest.mark.parametrize("name", SCORE_CASES)
def test_scores_against_float64(name):
    from ubpl_amd import kernels as Kn
    B, M, S, K, H, W, _ = RR.CASES[name]
    HW = H * W
    preds, targets = _stacked(name)
    bar = _bar()
    p, t = torch.from_numpy(preds).to(DEV), torch.from_numpy(targets).to(DEV)
    # M = 1: every stack of the predictions
    got = Kn.softmax_peak_scores(p, S * K * HW, K * HW, 0, 1, B, S, K, HW).cpu().double().numpy().reshape(B, S, K)
    ref = _ref64(preds)
    err1 = float((np.abs(got - ref) / ref).max())
    # M = 2: the member mean of the LAST stack of [M,B,S,K,H,W], addressed in place
    last = t.reshape(-1)[(S - 1) * K * HW:]
    got = Kn.softmax_peak_scores(last, S * K * HW, 0, B * S * K * HW, M, B, 1, K, HW).cpu().double().numpy()
    ref = _ref64(targets.astype(np.float64).mean(0)[:, -1])
    err2 = float((np.abs(got.reshape(B, K) - ref) / ref).max())
    # M = 1 on one member's last stack in place, into a preallocated output
    out = torch.full((B * K,), 7.0, device=DEV)
    assert Kn.softmax_peak_scores(last, S * K * HW, 0, 0, 1, B, 1, K, HW, out=out) is out
    ref = _ref64(targets[0][:, -1])
    err3 = float((np.abs(out.cpu().double().numpy().reshape(B, K) - ref) / ref).max())
    print("%s: kernel vs float64 max relative error M=1 %.3e, M=2 in place %.3e, M=1 in place %.3e (bar %.3e)"
          % (name, err1, err2, err3, bar))
    assert max(err1, err2, err3) <= bar


def test_scores_limits_and_nan():
    from ubpl_amd import kernels as Kn
    x = torch.rand(9 * 2 * 33 * 16, device=DEV)
    out = torch.zeros(2 * 33, device=DEV)
    Kn.call("ubpl_softmax_peak_scores", x, 32 * 16, 0, 0, 1, 2, 1, 32, 16, out)            # K = 32: the limit
    Kn.call("ubpl_softmax_peak_scores", x, 16, 0, 2 * 16, 8, 2, 1, 1, 16, out)             # M = 8, K = 1
    assert torch.equal(out[:2], torch.ones(2, device=DEV))                                 # one map: softmax is 1
    for K, M in ((33, 1), (0, 1), (1, 9), (1, 0)):
        with pytest.raises(RuntimeError, match="failed with hipError 1"):
            Kn.call("ubpl_softmax_peak_scores", x, K * 16, 0, 2 * K * 16, M, 2, 1, K, 16, out)
    with pytest.raises(ValueError, match="1..32 maps"):
        Kn.softmax_peak_scores(x, 33 * 16, 0, 0, 1, 2, 1, 33, 16)
    # a NaN at one pixel: the scores of its (b,s) are NaN, the other (b,s) untouched
    x = torch.rand(2, 1, 4, 300, device=DEV)
    clean = Kn.softmax_peak_scores(x, 4 * 300, 4 * 300, 0, 1, 2, 1, 4, 300).clone()
    x[1, 0, 2, 299] = float("nan")
    got = Kn.softmax_peak_scores(x, 4 * 300, 4 * 300, 0, 1, 2, 1, 4, 300)
    assert torch.equal(got[:4], clean[:4]) and torch.isnan(got[4:]).all()


def _rank_inputs(G, N, kind, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "dup7":                                      # heavy duplication: 7 distinct floats
        vals = torch.tensor([0.0625, 0.07, 0.1, 0.1000001, 0.125, 0.15, 0.9])
        return vals[torch.randint(0, 7, (G, N), generator=g)]
    x = torch.rand(G, N, generator=g)
    if kind == "inf" and N >= 2:
        x[:, 0] = float("inf")
        x[:, N // 2] = float("-inf")
        x[:, N - 1] = float("inf")
    return x


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 512, 544, 4096])
def test_thresholds_equal_torch_sort(N):
    from ubpl_amd import kernels as Kn
    for G in (1, 2):
        for kind in ("rand", "dup7", "inf"):
            x = _rank_inputs(G, N, kind, 100 + N).to(DEV)
            srt = torch.sort(x, dim=1)[0]
            for rank in sorted({0, N // 2, N - 1}):
                got = Kn.rank_threshold(x.reshape(-1), G, N, rank)
                want = srt[:, rank].contiguous()
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (G, kind, rank, got, want)


def test_threshold_nans_order_last_and_limits():
    from ubpl_amd import kernels as Kn
    x = torch.tensor([0.3, float("nan"), 0.1, 0.2, float("nan")], device=DEV)
    assert [float(Kn.rank_threshold(x, 1, 5, r)) for r in range(3)] == [float(np.float32(v)) for v in (0.1, 0.2, 0.3)]
    assert torch.isnan(Kn.rank_threshold(x, 1, 5, 3)) and torch.isnan(Kn.rank_threshold(x, 1, 5, 4))
    out = torch.zeros(1, device=DEV)
    big = torch.rand(8193, device=DEV)
    Kn.call("ubpl_rank_threshold", big, 1, 8192, 8191, out)                               # the limits themselves
    assert float(out) == float(big[:8192].max())
    for N, rank in ((8193, 0), (16, 16), (16, -1), (0, 0)):
        with pytest.raises(RuntimeError, match="failed with hipError 1"):
            Kn.call("ubpl_rank_threshold", big, 1, N, rank, out)
    with pytest.raises(IndexError):
        Kn.rank_threshold(big, 1, 16, 16)
    with pytest.raises(ValueError, match="groups of"):
        Kn.rank_threshold(big, 1, 8193, 0)


def _finalize_statement(kind, sq, asc, tsc, athr, tthr, gate, sw, use_gate, use_sw, B, S, K):
    """The finalize entries in numpy, per row in float32 as the kernel, the sum in float64: kinds 1
    and 2 as ubpl_loss_finalize_ranked takes them (per-stack thresholds), and with athr = tthr = one
    constant repeated, kinds 0 to 3 of ubpl_loss_finalize (asc = amax, tsc = tmax).  Kind 3 is kind 2
    with [gate > 0] in the mask and the gate out of cnt[0]."""
    sq, tsc = sq.reshape(B, S, K), tsc.reshape(B, S, K)
    g = np.ones((B, 1, K), np.float32) if gate is None else gate.reshape(B, 1, K)
    w = np.ones((B, 1, 1), np.float32) if sw is None else sw.reshape(B, 1, 1)
    m = np.ones((B, S, K), np.float32) if kind == 0 else (tsc >= tthr.reshape(1, S, 1)).astype(np.float32)
    if kind >= 2:
        l = sq * w
        m = m * (asc.reshape(B, S, K) >= athr.reshape(1, S, 1)).astype(np.float32)
        if kind == 3:
            m = m * (g > 0).astype(np.float32)
        wv = m * w
    else:
        l, wv = sq, m
        if use_gate:
            l, wv = l * g, wv * g
        if use_sw and sw is not None:
            l, wv = l * w, wv * w
    rows = (w.reshape(B) > 0)
    n_rows = int(rows.sum())
    st = tsc[rows].sum(0) / max(n_rows, 1)
    score = ((asc.reshape(B, S, K)[rows].sum(0) / max(n_rows, 1) + st) / 2 if kind >= 2 else st).mean(0)
    n_gate = B * K if kind == 3 else int((g > 0).sum())
    cnt = [S * n_gate, int((l > 0).sum()), int((m > 0).sum()), n_rows]
    return float((l * m).astype(np.float64).sum()), cnt, score, np.broadcast_to(wv, (B, S, K)).reshape(-1)


def _finalize_inputs(seed):
    """B = 5, S = 3, K = 17 (odd against the 256-thread row loop, K > 16): sq_mean with zero rows,
    two score sets with a NaN, gate with zeros, sw with zeros."""
    B, S, K = 5, 3, 17
    rs = np.random.RandomState(seed)
    sq = rs.uniform(0.0, 1.0, B * S * K).astype(np.float32)
    sq[::11] = 0.0
    asc, tsc = (rs.uniform(0.05, 0.15, B * S * K).astype(np.float32) for _ in range(2))
    tsc[7] = np.nan                                                     # a NaN score never selects
    gate = (rs.uniform(size=(B, K)) > 0.3).astype(np.float32) * 1.5
    sw = np.array([0.0, 1.0, 0.5, 0.0, 2.0], np.float32)
    return B, S, K, rs, sq, asc, tsc, gate, sw


def _dv(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


# (gate, sw, use_gate, use_sw) by name: what test_finalize_against_the_statement lists per kind
_COMBOS_GATED = (("gate", "sw", 1, 1), ("gate", "sw", 0, 0), (None, None, 1, 1), ("gate", "sw", 1, 0))
_COMBOS_PSEUDO = ((None, "sw", 0, 1),)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_finalize_constant_threshold_against_the_statement(kind):
    """ubpl_loss_finalize, all four kinds, against the numpy statement: counts and out_w exact, sum
    and score to the file's 1e-4 relative bar."""
    from ubpl_amd import kernels as Kn
    B, S, K, _, sq, amax, tmax, gate, sw = _finalize_inputs(11 + kind)
    thr = float(tmax[K + 3])                                            # a threshold that is a score: >= keeps it
    thrs = np.full(S, thr, np.float32)
    combos = _COMBOS_GATED if kind < 2 else (_COMBOS_PSEUDO if kind == 2 else (("gate", "sw", 0, 1),))
    for gn, wn, ug, us in combos:
        g, w = (gate if gn else None), (sw if wn else None)
        want = _finalize_statement(kind, sq, amax, tmax, thrs, thrs, g, w, ug, us, B, S, K)
        s, cnt, score, wv = Kn.loss_finalize(kind, _dv(sq), _dv(amax) if kind >= 2 else None,
                                             _dv(tmax) if kind else None, _dv(g), _dv(w), ug, us, B, S, K, thr)
        print("kind %d gate %s sw %s use %d %d: cnt %s want %s, sum %.9g want %.9g"
              % (kind, gn, wn, ug, us, cnt.tolist(), want[1], float(s), want[0]))
        assert cnt.tolist() == want[1]
        assert np.array_equal(wv.cpu().numpy(), want[3])
        assert abs(float(s) - want[0]) <= 1e-4 * abs(want[0])
        if kind == 0:
            assert score is None
        else:
            assert np.allclose(score.cpu().numpy(), want[2], rtol=1e-4, atol=0, equal_nan=True)
            assert np.isnan(want[2]).sum() == (1 if w is None else 0)
        assert 0 < want[1][2] and (kind == 0 or want[1][2] < B * S * K)      # the mask is neither empty nor full


@pytest.mark.parametrize("kind", [1, 2])
def test_finalize_and_finalize_ranked_give_the_same_bits(kind):
    """One finalize body serves both entries: ubpl_loss_finalize on (amax, tmax, thr) and
    ubpl_loss_finalize_ranked on the same arrays as scores with thr repeated per stack agree in
    every output bit."""
    from ubpl_amd import kernels as Kn
    B, S, K, _, sq, amax, tmax, gate, sw = _finalize_inputs(21 + kind)
    thr = float(tmax[K + 3])
    thrs = _dv(np.full(S, thr, np.float32))
    for gn, wn, ug, us in (_COMBOS_GATED if kind == 1 else _COMBOS_PSEUDO):
        g, w = _dv(gate if gn else None), _dv(sw if wn else None)
        a_in = _dv(amax) if kind == 2 else None
        one = Kn.loss_finalize(kind, _dv(sq), a_in, _dv(tmax), g, w, ug, us, B, S, K, thr)
        two = Kn.loss_finalize_ranked(kind, _dv(sq), a_in, _dv(tmax), thrs if kind == 2 else None, thrs, g, w, ug, us,
                                      B, S, K)
        assert int(one[1][2]) > 0
        for name, a, b in zip(("sum", "cnt", "score", "w"), one, two):
            assert a.dtype == b.dtype and a.shape == b.shape, name
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (name, a, b)


@pytest.mark.parametrize("kind", [1, 2])
def test_finalize_against_the_statement(kind):
    from ubpl_amd import kernels as Kn
    B, S, K = 5, 3, 17
    rs = np.random.RandomState(3 + kind)
    sq = rs.uniform(0.0, 1.0, B * S * K).astype(np.float32)
    sq[::11] = 0.0
    asc, tsc = (rs.uniform(0.05, 0.15, B * S * K).astype(np.float32) for _ in range(2))
    tsc[7] = np.nan                                                     # a NaN score never selects
    athr, tthr = (rs.uniform(0.08, 0.12, S).astype(np.float32) for _ in range(2))
    tthr[1] = tsc[K + 3]                                                # a threshold that is a score: >= keeps it
    gate = (rs.uniform(size=(B, K)) > 0.3).astype(np.float32) * 1.5
    sw = np.array([0.0, 1.0, 0.5, 0.0, 2.0], np.float32)
    dv = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    combos = [(None, sw, 0, 1)]
    if kind == 1:
        combos = [(gate, sw, 1, 1), (gate, sw, 0, 0), (None, None, 1, 1), (gate, sw, 1, 0)]
    for g, w, ug, us in combos:
        want = _finalize_statement(kind, sq, asc, tsc, athr, tthr, g, w, ug, us, B, S, K)
        a_in = (dv(asc), dv(athr)) if kind == 2 else (None, None)
        s, cnt, score, wv = Kn.loss_finalize_ranked(kind, dv(sq), a_in[0], dv(tsc), a_in[1], dv(tthr), dv(g), dv(w),
                                                    ug, us, B, S, K)
        assert cnt.tolist() == want[1]
        assert np.array_equal(wv.cpu().numpy(), want[3])
        assert abs(float(s) - want[0]) <= 1e-4 * abs(want[0])
        # (the NaN score is in a row with sw = 0: it reaches out_score only where every row counts)
        assert np.allclose(score.cpu().numpy(), want[2], rtol=1e-4, atol=0, equal_nan=True)
        assert np.isnan(want[2]).sum() == (1 if w is None else 0)
    # the step's form, the rank selections folded into the launch: the bits of the two entries composed
    rank = (B * K) // 3
    for ts in (S, 1):
        t_in = dv(tsc) if ts == S else dv(np.ascontiguousarray(tsc.reshape(B, S, K)[:, 0]).reshape(-1))
        g, w, ug, us = combos[0]
        s, cnt, score, wv, thr = Kn.loss_finalize_rank(kind, dv(sq), dv(asc) if kind == 2 else None, t_in, ts, rank,
                                                       dv(g), dv(w), ug, us, B, S, K)
        major = lambda x, n: x.view(B, n, K).transpose(0, 1).contiguous().view(-1)
        t2 = Kn.rank_threshold(major(t_in, ts), ts, B * K, rank).expand(S).contiguous()
        t1 = Kn.rank_threshold(major(dv(asc), S), S, B * K, rank) if kind == 2 else None
        full = t_in if ts == S else t_in.view(B, 1, K).expand(B, S, K).contiguous().view(-1)
        want = Kn.loss_finalize_ranked(kind, dv(sq), dv(asc) if kind == 2 else None, full, t1, t2, dv(g), dv(w),
                                       ug, us, B, S, K)
        assert torch.equal(thr[S:].view(torch.int32), t2.view(torch.int32))
        assert torch.equal(thr[:S].view(torch.int32), t1.view(torch.int32)) if kind == 2 else torch.isnan(thr[:S]).all()
        for a, b in zip((s, cnt, score, wv), want):
            assert torch.equal(a, b) or (a.dtype.is_floating_point and
                                         torch.equal(a.view(torch.int32), b.view(torch.int32)))
    for bad in (dict(rank=B * K), dict(rank=-1), dict(ts=2), dict(S=17)):
        a = dict(dict(rank=rank, ts=S, S=S), **bad)
        with pytest.raises(RuntimeError, match="failed with hipError 1"):
            Kn.call("ubpl_loss_finalize_rank", kind, torch.zeros(B * 17 * K, device=DEV),
                    torch.zeros(B * 17 * K, device=DEV), torch.zeros(B * 17 * K, device=DEV), a["ts"], a["rank"],
                    None, dv(sw), 0, 1, B, a["S"], K, torch.empty(34, device=DEV), torch.empty(1, device=DEV),
                    torch.empty(4, device=DEV, dtype=torch.int32), None, torch.empty(B * 17 * K, device=DEV))
    with pytest.raises(RuntimeError, match="failed with hipError 1"):
        Kn.call("ubpl_loss_finalize_ranked", 2, dv(sq), None, dv(tsc), None, dv(tthr), None, dv(sw), 0, 1, B, S, K,
                torch.empty(1, device=DEV), torch.empty(4, device=DEV, dtype=torch.int32), None,
                torch.empty(B * S * K, device=DEV))
    with pytest.raises(RuntimeError, match="failed with hipError 1"):
        Kn.call("ubpl_loss_finalize_ranked", 0, dv(sq), dv(asc), dv(tsc), dv(athr), dv(tthr), None, dv(sw), 0, 1, B,
                S, K, torch.empty(1, device=DEV), torch.empty(4, device=DEV, dtype=torch.int32), None,
                torch.empty(B * S * K, device=DEV))
