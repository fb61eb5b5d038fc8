"""Cross-view pseudo-label targets inside train_mt_ubpl (args.pseudoViews) on the smallest MT_UBPL
step the step tests use — test_gpu_view_gate_train.py's setup: two 1-stack hourglasses and their
teachers at 128x128, B = 4 (2 unlabeled + 2 labeled rows), 4 keypoints, DeviceAugment's views of the
first shard of the Mouse fixture images with their matrices."""
import collections
import contextlib
import copy
import io
import os
import random

import numpy as np
import pytest
import torch

import cross_view_ref as CR
import seeds

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(seeds.step_cases()["mt_ubpl"], S=1, K=4, res=128, out=32, seed=611)
PACK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mouse_100_500_0.3")
ROWS = [1, 2, 0, 3]                    # of the first shard: two unlabeled images, then two labeled
MERGE = "ubpl_merge_views_samples"


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _factory(k, s, mode):
    from ubpl_amd.hourglass import StackedHourglass
    return StackedHourglass(k, s, mode)


_DATA = {}


def _mouse():
    """-> (uint8 BGR images [20,256,256,3], keypoints [20,9,3], labelled flags [20], means)."""
    if not _DATA:
        with np.load(os.path.join(PACK, "meta.npz")) as z:
            kps, isl, means = z["train_kps"][:20], z["train_islabeled"][:20].astype(bool), z["means"].tolist()
        with np.load(os.path.join(PACK, "train_imgs_00.npz")) as z:
            imgs = np.ascontiguousarray(np.repeat(z["grey"][..., None], 3, axis=3))
        assert list(isl[ROWS]) == [False, False, True, True]
        _DATA["v"] = (imgs, kps, isl, means)
    return _DATA["v"]


_BATCHES = {}


def _batches(n=2):
    """n seeded batches (views, None, meta) with meta["viewmat"], made once; handed out as copies."""
    if n not in _BATCHES:
        from ubpl_amd.augment import DeviceAugment
        imgs, kps, isl, means = _mouse()
        aug = DeviceAugment(imgs, means, inp_res=CFG["res"], device=DEV)
        random.seed(CFG["seed"])
        torch.manual_seed(CFG["seed"])
        out = []
        for _ in range(n):
            views, ks, mats = [], [], []
            for _ in range(CFG["A"]):
                x, k, m = aug.views(ROWS, kps[ROWS][:, :CFG["K"]], with_mats=True)
                views.append(x)
                ks.append(k)
                mats.append(m)
            out.append((views, None, {"kps": ks, "islabeled": [torch.tensor(isl[ROWS], device=DEV)],
                                      "viewmat": mats}))
        _BATCHES[n] = out
    return copy.deepcopy(_BATCHES[n])


def _args(**opts):
    _, args = seeds.step_batch(dict(CFG, B=2, res=32, out=8), lambda k, shape, res, out: (
        torch.zeros(k.shape[0], out, out), k))                         # (the namespace only)
    args.outRes = CFG["out"]
    for k, v in opts.items():
        setattr(args, k, v)
    return args


def _setup(head_bias=0.0, **opts):
    """head_bias: added to the bias of every teacher's output convolution, so that every map of an
    untrained teacher has a positive maximum (a peak, hence a legal point for the gate)."""
    from ubpl_amd.optim import FlatAdamW
    models, emas, _ = seeds.step_models(_factory, CFG, device=DEV)
    if head_bias:
        with torch.no_grad():
            for e in emas:
                start, n, _ = e._offs["preds.0.conv.bias"]
                e.flat_params[start:start + n] += head_bias
    optims = [FlatAdamW(m, lr=CFG["lr"], weight_decay=0) for m in models]
    return models, emas, optims, _args(**opts)


def _train(loader, models, emas, optims, args):
    from ubpl_amd import train as T
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        rec = T.train_mt_ubpl(loader, models, emas, optims, args)
    torch.cuda.synchronize()
    return rec, buf.getvalue()


def _one_step(models, emas, optims, args, batch):
    """One eager step through the core itself -> (packed records, their layout)."""
    from ubpl_amd import train as T
    for m in [*models, *emas]:
        m.train()
    packed, L, *_ = T._drive(T._mt_ubpl_core(models, emas, optims, args, *batch))
    torch.cuda.synchronize()
    return packed.cpu(), L


def _state(models, emas, optims):
    st = {}
    for i, m in enumerate(models + emas):
        st["params%d" % i] = m.flat_params.detach().clone()
        st["stats%d" % i] = m.flat_stats.detach().clone()
    for i, o in enumerate(optims):
        st["m%d" % i], st["v%d" % i] = o.exp_avg.clone(), o.exp_avg_sq.clone()
    return st


def _eq(a, b):
    if a.dtype.is_floating_point:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    return torch.equal(a, b)


@pytest.fixture
def eager(monkeypatch):
    from ubpl_amd import train as T
    monkeypatch.setenv("UBPL_STEP_GRAPH", "0")
    T._StepGraph.clear()
    yield
    T._StepGraph.clear()


_REF = {}


def _forwards(head_bias=0.0):
    """The reference for batch 0: the networks (as step_models seeds them) called in train mode —
    their outputs depend on the batch statistics only -> (students' outputs [M][A] of [B,S,K,H,W]
    on the device, the teachers' last stacks [A,M,B,K,H,W] numpy, the product's pair matrices
    [A,A,B,6] numpy)."""
    if head_bias not in _REF:
        from ubpl_amd import kernels as Kn
        models, emas, _, _ = _setup(head_bias)
        views, _, meta = _batches()[0]
        with torch.no_grad():
            for m in [*models, *emas]:
                m.train()
            stu = [[m(x)[0].clone() for x in views] for m in models]
            last = torch.stack([torch.stack([e(x)[0][:, -1] for e in emas]) for x in views])
        P = Kn.train_pair_matrices([m.float().reshape(-1, 6) for m in meta["viewmat"]], CFG["res"], CFG["out"])
        _REF[head_bias] = (stu, last.cpu().numpy(), P.cpu().numpy())
    return _REF[head_bias]


def _restated_targets(views, head_bias=0.0):
    """-> targets per view a, [M,B,1,K,H,W] CPU tensors: the numpy restatement's merge of the teachers'
    maps under the product's matrices ("own": the teachers' maps themselves)."""
    if (views, head_bias) not in _REF:
        _, last, P = _forwards(head_bias)
        xt = last if views == "own" else CR.merge_views_samples(last, P, include_self=views == "merged")[0]
        _REF[views, head_bias] = [torch.from_numpy(np.ascontiguousarray(xt[a])).unsqueeze(2)
                                  for a in range(xt.shape[0])]
    return _REF[views, head_bias]


def _nega():
    _, _, isl, _ = _mouse()
    return torch.tensor(np.where(isl[ROWS], 0.0, CFG["pseudoWeight"]), dtype=torch.float32)


def _oracle_records(views, thr):
    """oracle.losses.joint_pseudo3 of every (student, view) on the restated targets
    -> (epc record per student, n_pseudo, n_sel)."""
    from oracle import losses as OL
    stu, _, _ = _forwards()
    tg = _restated_targets(views)
    epc, n_ps, n_sel = [], 0, 0
    for mi in range(len(stu)):
        s_m, c_m = 0.0, 0
        for a in range(CFG["A"]):
            s, c, sel, *_ = OL.joint_pseudo3(stu[mi][a][:, 0].cpu().double(), tg[a][:, :, 0].double(),
                                             _nega().double(), CFG["S"], thr)
            s_m, c_m, n_sel = s_m + float(s), c_m + c, n_sel + sel
        epc.append(CFG["ensemblePseudoWeight"] * (s_m / c_m if c_m > 0 else s_m))
        n_ps += c_m
    return epc, n_ps, n_sel


def _threshold(views):
    """The midpoint of the widest gap between the sorted restated scores (the students' peaks and the
    merged targets' peaks) that leaves 0 < n_sel < n_pseudo; None if there is none."""
    stu, _, _ = _forwards()
    tg = _restated_targets(views)
    scores = [t.mean(0).flatten(-2).max(-1).values.reshape(-1) for t in tg]
    scores += [o.cpu().flatten(-2).max(-1).values.reshape(-1) for ms in stu for o in ms]
    s = np.unique(torch.cat(scores).numpy().astype(np.float64))
    for i in np.argsort(-(s[1:] - s[:-1])):
        thr = float((s[i] + s[i + 1]) / 2)
        _, n_ps, n_sel = _oracle_records(views, thr)
        if 0 < n_sel < n_ps:
            return thr
    return None


@pytest.mark.parametrize("views", ["merged", "other"])
def test_records_match_the_oracle_on_the_restated_targets(eager, views):
    thr = _threshold(views)
    assert thr is not None, "no threshold leaves the selection mixed"
    epc_ref, n_ps_ref, n_sel_ref = _oracle_records(views, thr)
    host, L = _one_step(*_setup(pseudoViews=views, pseudoScoreThr=thr), _batches()[0])
    h = host.tolist()
    n_ps, n_sel = L.total(h, "epc_n"), L.total(h, "n_sel")
    epc = [h[L.r("epc", mi)] for mi in range(L.M)]
    print("%s: pseudoScoreThr %.6f, n_pseudo %d (oracle %d), n_sel %d (oracle %d), epc %s (oracle %s)"
          % (views, thr, n_ps, n_ps_ref, n_sel, n_sel_ref, epc, epc_ref))
    assert (n_ps, n_sel) == (n_ps_ref, n_sel_ref) and 0 < n_sel < n_ps
    for got, want in zip(epc, epc_ref):
        assert abs(got - want) <= 1e-4 * abs(want), (got, want)
    # the own-view run at the same threshold gives other records: the targets did change
    own, _ = _one_step(*_setup(pseudoScoreThr=thr), _batches()[0])
    assert not _eq(own, host)
    assert [own.tolist()[L.r("epc", mi)] for mi in range(L.M)] != epc


def test_captured_step_matches_eager(monkeypatch):
    """Four steps over two alternating batches (two eager warm-ups, the capture with its first
    replay, one more replay: the matrices change between replays): records and every parameter,
    statistic and optimizer buffer bit-equal to the eager run."""
    from ubpl_amd import train as T
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("UBPL_MODEL_STREAMS", "1")
        monkeypatch.setenv("UBPL_STEP_GRAPH", mode)
        T._StepGraph.clear()
        models, emas, optims, args = _setup(pseudoViews="merged", pseudoScoreThr=1e-3)
        b = _batches()
        rec, _ = _train([b[i % 2] for i in range(4)], models, emas, optims, args)
        if mode == "1":
            runner = T._StepGraph.get(T._mt_ubpl_core, models, emas, optims, args)
            assert runner.graph is not None and runner.n_eager == T._StepGraph.WARM
        runs[mode] = (rec, _state(models, emas, optims))
        T._StepGraph.clear()
    e, g = runs["0"], runs["1"]
    assert e[0] == g[0], (e[0], g[0])
    for k in e[1]:
        assert _eq(e[1][k], g[1][k]), k


def _calls_of(monkeypatch, **opts):
    """One eager step of batch 0 -> (Counter of _lib.call names, records, state)."""
    from ubpl_amd import _lib
    calls = []
    real = _lib.call
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
        setup = _setup(**opts)
        host, L = _one_step(*setup, _batches()[0])
    return collections.Counter(calls), host, _state(*setup[:3]), L


def test_default_step_makes_no_new_call(eager, monkeypatch):
    absent, host_a, state_a, _ = _calls_of(monkeypatch)
    assert absent["ubpl_loss_finalize"] > 0 and MERGE not in absent
    own, host_o, state_o, _ = _calls_of(monkeypatch, pseudoViews="own")
    assert own == absent and _eq(host_a, host_o)
    for k in state_a:
        assert _eq(state_a[k], state_o[k]), k
    for views in ("merged", "other"):
        on, host_m, _, _ = _calls_of(monkeypatch, pseudoViews=views)
        assert on - absent == collections.Counter([MERGE]) and not absent - on    # one launch more, nothing else
        assert not _eq(host_m, host_a)


@pytest.mark.parametrize("rule", [dict(pseudoRule="uncertainty", distThrMax=1e9),
                                  dict(pseudoRule="rate", pseudoSelRate=0.5)], ids=["uncertainty", "rate"])
def test_with_the_other_rules(eager, monkeypatch, rule):
    """The rule says which joints are kept, the views what they are pulled towards: the calls are
    the union of the two features', and epc is the product's loss of that rule on the restated
    targets."""
    from ubpl_amd import train as T
    from ubpl_amd import view_gate as VG
    from ubpl_amd.losses import sel_rank
    bias = 1.0                                                         # (every teacher map has a peak: a legal point)
    base, _, _, _ = _calls_of(monkeypatch, head_bias=bias)
    alone, _, _, _ = _calls_of(monkeypatch, head_bias=bias, **rule)
    both, host, _, L = _calls_of(monkeypatch, head_bias=bias, pseudoViews="merged", **rule)
    assert both - alone == collections.Counter([MERGE]) and not alone - both
    assert (both - base) == (alone - base) + collections.Counter([MERGE])
    # the product's loss of the rule on the restated targets
    stu, last, _ = _forwards(bias)
    tg = [t.to(DEV) for t in _restated_targets("merged", bias)]
    nega = _nega().to(DEV)
    B, K, S, A = CFG["B"], CFG["K"], CFG["S"], CFG["A"]
    views, _, meta = _batches()[0]
    if rule["pseudoRule"] == "rate":
        loss = lambda o, t: T._pseudo_ranked(o, t, nega, S, sel_rank(B * K, rule["pseudoSelRate"]))[:2]
    else:
        opts = VG.options(_args(**rule))
        own = [torch.from_numpy(np.ascontiguousarray(last[a])).to(DEV).unsqueeze(2) for a in range(A)]
        gate = VG.view_gate(opts, own, meta["viewmat"], CFG["res"])
        loss = lambda o, t: T._pseudo_gated(o, t, nega, S, opts.thr, gate)[:2]
    h = host.tolist()
    for mi in range(L.M):
        parts = [loss(stu[mi][a], tg[a]) for a in range(A)]
        s, c = sum(float(p[0]) for p in parts), sum(int(p[1][1]) for p in parts)
        want = CFG["ensemblePseudoWeight"] * (s / c if c > 0 else s)
        print("%s model %d: epc %.8g, on the restated targets %.8g (n_pseudo %d)"
              % (rule["pseudoRule"], mi, h[L.r("epc", mi)], want, c))
        assert c > 0 and want > 0
        assert abs(h[L.r("epc", mi)] - want) <= 1e-4 * abs(want)


def test_pseudo_losses_read_a_last_stack_alone_as_they_read_it_in_place():
    """The guard for St = 1: the three pseudo losses on targets [M,B,St,K,H,W] and on their last
    stacks alone, [M,B,1,K,H,W], give equal bits."""
    from ubpl_amd import train as T
    M, B, S, K, H = 2, 3, 2, 4, 16
    g = torch.Generator().manual_seed(3)
    preds = torch.rand(B, S, K, H, H, generator=g).to(DEV)
    tg = torch.rand(M, B, S, K, H, H, generator=g).to(DEV)
    sw = torch.tensor([1.0, 0.0, 1.0], device=DEV)
    gate = (torch.rand(B, K, generator=g) > 0.4).float().to(DEV)
    lastonly = tg[:, :, -1:].contiguous()
    assert lastonly.shape == (M, B, 1, K, H, H)
    for f in (lambda t: T._pseudo(preds, t, sw, S, 0.9), lambda t: T._pseudo_gated(preds, t, sw, S, 0.9, gate),
              lambda t: T._pseudo_ranked(preds, t, sw, S, 5)):
        for x, y in zip(f(tg), f(lastonly)):
            assert _eq(x, y)


def test_errors_before_any_launch(eager, monkeypatch):
    from ubpl_amd import _lib
    from ubpl_amd import train as T
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    views, _, meta = _batches()[0]
    with pytest.raises(ValueError, match="pseudoViews is one of own, merged, other"):
        _train([(views, None, meta)], *_setup(pseudoViews="all"))
    no_mats = {k: v for k, v in meta.items() if k != "viewmat"}
    with pytest.raises(ValueError, match='pseudoViews \'merged\' needs meta\\["viewmat"\\]'):
        _train([(views, None, no_mats)], *_setup(pseudoViews="merged"))
    one = {"kps": meta["kps"][:1], "islabeled": meta["islabeled"], "viewmat": meta["viewmat"][:1]}
    with pytest.raises(ValueError, match="at least 2"):
        _train([(views[:1], None, one)], *_setup(pseudoViews="other"))
    models, emas, optims, args = _setup(pseudoViews="merged")
    with pytest.raises(ValueError, match="pseudoViews 'merged' is built into train_mt_ubpl only"):
        with contextlib.redirect_stdout(io.StringIO()):
            T.train_dualpose_ubpl([(views[0], None, views[1], {"kps": meta["kps"][0],
                                                               "islabeled": meta["islabeled"][0]})],
                                  models, emas, optims, args)
    with pytest.raises(ValueError, match="train_mt_ubpl only, not train_mt"):
        T.train_mt([(views, None, meta)], models[0], emas[0], optims[0], args)
    with pytest.raises(ValueError, match="train_mt_ubpl only, not train_supervised"):
        T.train_supervised([(views[0], None, meta)], models[0], optims[0], args)
    assert calls == []                                                 # nothing was launched


def test_batch_line_shows_the_views(eager):
    _, out = _train(_batches()[:1], *_setup(pseudoViews="merged", pseudoScoreThr=1e-3))
    assert "(scoreThr:0.00 views:merged)" in out
    _, out = _train(_batches()[:1], *_setup(pseudoViews="other", pseudoScoreThr=1e-3, pseudoRule="uncertainty",
                                            distThrMax=4.0))
    assert "(scoreThr:0.00 distThr:4.00 views:other)" in out
    for off in (dict(), dict(pseudoViews="own")):
        _, out = _train(_batches()[:1], *_setup(pseudoScoreThr=1e-3, **off))
        assert "views" not in out and "(scoreThr:0.00)" in out
