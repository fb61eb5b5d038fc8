"""args.pseudoRule = "rate" inside train_mt_ubpl: one step at B = 4, two 2-stack hourglasses and their
teachers at 256x256, against a CPU statement assembled here from the oracle's step (oracle/step.py,
with its ensemble-pseudo loss swapped for tests/rate_ref.py's JointPseudoLoss2 in float32); the
captured step against the eager one; the record with the rule off; the refusals."""
import contextlib
import io

import numpy as np
import pytest
import torch

import rate_ref as RR
import seeds
from oracle import hourglass as OH
from oracle import losses as OL
from oracle import render as OR
from oracle import step as OS

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEL_RATE = 0.5
# the batch seed: one whose CPU scores meet the separation condition (asserted below, on the CPU)
CFG = dict(seeds.step_cases()["mt_ubpl"], seed=601)
TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _factory(k, s, mode):
    from ubpl_amd.hourglass import StackedHourglass
    return StackedHourglass(k, s, mode)


def _checksums(nets):
    """Per network (sum |p|, sum p^2) in float64.  The signed sum is not used: it cancels to near
    zero for a symmetric initialisation, so its relative error says nothing."""
    out = []
    for m in nets:
        ps = [p.detach().double().cpu() for p in m.parameters()]
        out.append((float(sum(p.abs().sum() for p in ps)), float(sum((p * p).sum() for p in ps))))
    return np.array(out)


_CPU = {}


def _cpu_statement():
    """The oracle's MT_UBPL step with joint_pseudo3 replaced by the restatement of JointPseudoLoss2
    (same targets, same sample weights, same normaliser) -> dict: rec, counts, sep (the closest
    score to its threshold, relative), thr [M,2] (per model the mean rateThr1, rateThr2), sums."""
    if _CPU:
        return _CPU
    seps, thrs = [], []

    def pseudo2(preds, targets, sw, nstack=1, thr=None):
        res = RR.pseudo_loss(preds, targets, sw, nstack, ("rate", SEL_RATE), dtype=torch.float32)
        for sk, tk in (("score1", "thr1"), ("score2", "thr2")):
            seps.extend(RR.separation(res[sk][i].numpy(), res[tk][i]) for i in range(nstack))
        thrs.append([float(res["thr1"].mean()), float(res["thr2"].mean())])
        return res["sum"], res["n_pseudo"], res["n_sel"], res["score"], res["thr1"], res["thr2"]

    torch.set_num_threads(16)
    models, emas, optims = seeds.step_models(OH.oracle_factory, CFG)
    loader, args = seeds.step_batch(CFG, OR.kps_heatmap_torch)
    real = OL.joint_pseudo3
    OL.joint_pseudo3 = pseudo2
    try:
        rec, counts = OS.train_mt_ubpl(loader, models, emas, optims, args)
    finally:
        OL.joint_pseudo3 = real
    M, A = CFG["brNum"], CFG["A"]
    _CPU.update(rec=rec, counts=counts[0], sep=min(seps), thr=np.array(thrs).reshape(M, A, 2).mean(1),
                sums=_checksums(models + emas))
    return _CPU


def _args(**opts):
    _, args = seeds.step_batch(dict(CFG, B=2, res=32, out=8), OR.kps_heatmap_torch)      # (the namespace only)
    for k, v in opts.items():
        setattr(args, k, v)
    return args


_BATCH = []


def _batch():
    if not _BATCH:
        _BATCH.append(seeds.step_batch(CFG, OR.kps_heatmap_torch)[0][0])
    return _BATCH[0]


def _setup(**opts):
    from ubpl_amd.optim import FlatAdamW
    models, emas, _ = seeds.step_models(_factory, CFG, device=DEV)
    optims = [FlatAdamW(m, lr=CFG["lr"], weight_decay=0) for m in models]
    return models, emas, optims, _args(**opts)


def _one_step(models, emas, optims, args):
    from ubpl_amd import train as T
    for m in [*models, *emas]:
        m.train()
    packed, L, *_ = T._drive(T._mt_ubpl_core(models, emas, optims, args, *_batch()))
    torch.cuda.synchronize()
    return packed.cpu(), L


@pytest.fixture
def eager(monkeypatch):
    from ubpl_amd import train as T
    monkeypatch.setenv("UBPL_STEP_GRAPH", "0")
    T._StepGraph.clear()
    yield
    T._StepGraph.clear()


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.abs(want)).max())


def test_eager_step_against_the_cpu_statement(eager):
    ref = _cpu_statement()
    print("closest CPU score to its threshold: %.3e relative" % ref["sep"])
    assert ref["sep"] >= RR.SEP, "this batch does not meet the separation condition: choose another CFG seed"
    models, emas, optims, args = _setup(pseudoRule="rate", pseudoSelRate=SEL_RATE)
    packed, L = _one_step(models, emas, optims, args)
    host = packed.tolist()
    M = L.M
    assert len(host) == L.size and L.rate_thr == slice(L.size - 2 * M, L.size)
    # selection counts: exact
    assert (L.total(host, "n_sel"), L.total(host, "epc_n")) == tuple(ref["counts"])
    assert 0 < L.total(host, "n_sel") < L.total(host, "epc_n")
    pec, mtc, epc, fdc = ref["rec"]
    got = [[host[L.r(n, mi)] for mi in range(M)] for n in ("pec", "mtc", "epc")] + [host[L.fdc]]
    errs = [_rel(got[0], pec), _rel(got[1], mtc), _rel(got[2], epc), _rel(got[3], fdc)]
    thr_err = _rel(np.array(host[L.rate_thr]).reshape(M, 2), ref["thr"])
    sum_err = _rel(_checksums(models + emas), ref["sums"])
    print("relative errors: pec %.2e mtc %.2e epc %.2e fdc %.2e, thresholds %.2e, parameter checksums %.2e"
          % (*errs, thr_err, sum_err))
    assert max(errs) <= TOL and thr_err <= TOL and sum_err <= TOL


def _state(models, emas, optims):
    st = {}
    for i, m in enumerate(models + emas):
        st["params%d" % i] = m.flat_params.detach().clone()
        st["stats%d" % i] = m.flat_stats.detach().clone()
    for i, o in enumerate(optims):
        st["m%d" % i], st["v%d" % i] = o.exp_avg.clone(), o.exp_avg_sq.clone()
    return st


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype.is_floating_point else torch.equal(a, b)


def test_captured_step_matches_eager(monkeypatch):
    """Four steps on the same inputs (two eager warm-ups, the capture with its first replay, one more
    replay): records, printed lines and every buffer bit-equal to four eager steps — the bar of
    test_gpu_view_gate_train's captured case."""
    from ubpl_amd import train as T
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("UBPL_MODEL_STREAMS", "1")
        monkeypatch.setenv("UBPL_STEP_GRAPH", mode)
        T._StepGraph.clear()
        models, emas, optims, args = _setup(pseudoRule="rate", pseudoSelRate=SEL_RATE)
        counts = {}
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            rec = T.train_mt_ubpl([_batch()] * 4, models, emas, optims, args, pseudo_counts=counts)
        torch.cuda.synchronize()
        if mode == "1":
            runner = T._StepGraph.get(T._mt_ubpl_core, models, emas, optims, args)
            assert runner.graph is not None and runner.n_eager == T._StepGraph.WARM
        runs[mode] = (rec, buf.getvalue(), counts, _state(models, emas, optims))
        T._StepGraph.clear()
    e, g = runs["0"], runs["1"]
    assert e[0] == g[0] and e[1] == g[1] and e[2] == g[2], (e[:3], g[:3])
    for k in e[3]:
        assert _bits_equal(e[3][k], g[3][k]), k
    lines = e[1].strip().splitlines()
    assert len(lines) == 4 and all("selRate:0.50" in ln and "rateThr: [" in ln for ln in lines)
    assert e[2]["steps"] == 4 and 0 < e[2]["rate_thr1"] and 0 < e[2]["rate_thr2"] and e[2]["n_sel"] > 0


def test_record_without_the_rule_is_unchanged(eager, monkeypatch):
    from ubpl_amd import _lib
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    plain, L = _one_step(*_setup())                                     # a namespace without the new attributes
    new = ("ubpl_softmax_peak_scores", "ubpl_rank_threshold", "ubpl_loss_finalize_ranked", "ubpl_loss_finalize_rank")
    assert not any(n in new for n in calls)
    before = sorted(calls)
    M, K = L.M, CFG["K"]
    assert L.rate_thr is None and len(plain) == L.size == (3 * M + 1) + (3 * M + L.nfd) + K
    spelled, L2 = _one_step(*_setup(pseudoRule="score", pseudoSelRate=SEL_RATE))
    assert L2.size == L.size and _bits_equal(plain, spelled)
    calls.clear()
    ranked, L3 = _one_step(*_setup(pseudoRule="rate", pseudoSelRate=SEL_RATE))
    assert L3.size == L.size + 2 * M
    for mi in range(M):                                                 # pec and mtc do not depend on the rule
        assert ranked[L.r("pec", mi)] == plain[L.r("pec", mi)] and ranked[L.r("mtc", mi)] == plain[L.r("mtc", mi)]
    extra = list(calls)
    for name in before:
        if name in extra:
            extra.remove(name)
    # per pseudo-loss call: the two score reads, and one launch for the thresholds and the reduction
    calls_per_loss = {"ubpl_softmax_peak_scores": 2, "ubpl_loss_finalize_rank": 1}
    n_loss = M * CFG["A"]
    assert sorted(extra) == sorted(k for k, c in calls_per_loss.items() for _ in range(c * n_loss))
    assert calls.count("ubpl_loss_finalize") == before.count("ubpl_loss_finalize") - n_loss


def test_refusals_before_any_launch(eager, monkeypatch):
    from ubpl_amd import _lib
    from ubpl_amd import train as T
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    models, emas, optims, args = _setup(pseudoRule="rate", pseudoSelRate=SEL_RATE)
    imgs, hms, meta = _batch()
    with pytest.raises(ValueError, match="train_mt_ubpl only"):
        T.train_dualpose_ubpl([(imgs[0], hms[0][0], imgs[1], {"kpsWeight": meta["kpsWeights"][0][0],
                                                              "islabeled": meta["islabeled"][0]})],
                              models, emas, optims, args)
    with pytest.raises(ValueError, match="train_mt_ubpl only"):
        T.train_mt([_batch()], models[0], emas[0], optims[0], args)
    with pytest.raises(ValueError, match="train_mt_ubpl only"):
        T.train_supervised([(imgs[0], hms[0][0], {"islabeled": meta["islabeled"][0]})], models[0], optims[0], args)
    for bad in (None, 0, 1.5, "0.5"):
        a = _args(pseudoRule="rate")
        if bad is not None:
            a.pseudoSelRate = bad
        with pytest.raises(ValueError, match="pseudoSelRate"):
            with contextlib.redirect_stdout(io.StringIO()):
                T.train_mt_ubpl([_batch()], models, emas, optims, a)
    assert calls == []                                                  # nothing was launched
