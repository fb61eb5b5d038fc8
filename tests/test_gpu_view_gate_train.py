"""The view-consistency pseudo-label rule inside train_mt_ubpl (args.pseudoRule / distThrMax /
pseudoRefine / pseudoBlurSigma) on the smallest MT_UBPL step the step tests use: two 1-stack
hourglasses and their teachers at 128x128, B = 4 (2 unlabeled + 2 labeled rows), 4 keypoints.  The
views are DeviceAugment's, of the first shard of the Mouse fixture images, with their matrices."""
import contextlib
import copy
import io
import os
import random

import numpy as np
import pytest
import torch

import seeds
import view_gate_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = dict(seeds.step_cases()["mt_ubpl"], S=1, K=4, res=128, out=32, seed=611)
PACK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mouse_100_500_0.3")
ROWS = [1, 2, 0, 3]                    # of the first shard: two unlabeled images, then two labeled


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
    untrained teacher has a positive maximum (a peak, hence a legal point)."""
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
    """One eager step through the core itself -> (packed records as a list, their layout)."""
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


@pytest.fixture
def graphed(monkeypatch):
    from ubpl_amd import train as T
    monkeypatch.setenv("UBPL_MODEL_STREAMS", "1")
    monkeypatch.setenv("UBPL_STEP_GRAPH", "1")
    T._StepGraph.clear()
    yield
    T._StepGraph.clear()


_REF = {}


def _teacher_peaks(refine="taylor", head_bias=0.0):
    """The reference for batch 0: the teachers (as step_models seeds them) called in train mode —
    their outputs depend on the batch statistics only — decoded and refined per view
    -> (raw [M,V,B,K,2] numpy, back [V,B,6] numpy, scores [M,V,B,K] numpy)."""
    key = (refine, head_bias)
    if key not in _REF:
        from ubpl_amd import kernels as Kn
        _, emas, _, _ = _setup(head_bias)
        batch = _batches()[0]
        B, K, H = CFG["B"], CFG["K"], CFG["out"]
        taps = Kn.blur_taps(1.0 if refine == "taylor" else 0.0).to(DEV)
        raw, scores = [], []
        with torch.no_grad():
            for e in emas:
                e.train()
                per = []
                for x in batch[0]:
                    hm = e(x)[0][:, -1].contiguous()
                    r, _, sc = Kn.decode_heatmaps(hm)
                    if refine != "none":
                        r, _, _ = Kn.refine_peaks(hm, None, K * H * H, B, K, H, H, None, r, refine, taps)
                    per.append((r.cpu().numpy(), sc.cpu().numpy()))
                raw.append(np.stack([p[0] for p in per]))
                scores.append(np.stack([p[1] for p in per]))
        back = VR.train_back(np.stack([m.cpu().numpy() for m in batch[2]["viewmat"]]), CFG["res"], H)
        _REF[key] = (np.stack(raw), back, np.stack(scores))
    return _REF[key]


def _threshold_with_both(raw, back):
    """The lowest threshold between the restatement's distances at which the gate has zeros and
    ones (None if there is none)."""
    for t in VR.gaps_between(VR.view_gate(raw, back, 1.0)):
        g = VR.view_gate(raw, back, t)["gate"]
        if 0 < g.sum() < g.size:
            return t
    return None


def test_uncertainty_rule_selects_what_the_restatement_selects(eager):
    from ubpl_amd import kernels as Kn
    raw, back, _ = _teacher_peaks()
    thr = _threshold_with_both(raw, back)
    assert thr is not None, "no threshold leaves the gate mixed"
    gate_ref = VR.view_gate(raw, back, thr)["gate"]
    print("distThrMax %.4f: gate_ref %d of %d" % (thr, gate_ref.sum(), gate_ref.size))
    assert 0 < gate_ref.sum() < gate_ref.size
    models, emas, optims, args = _setup(pseudoRule="uncertainty", distThrMax=thr)
    batch = _batches()[0]
    # the wrapper on the same peaks gives the restatement's gate (the step's launch, alone)
    M, V, B, K = raw.shape[:4]
    dev_raw = torch.from_numpy(np.ascontiguousarray(raw.transpose(1, 0, 2, 3, 4))).to(DEV).reshape(-1)
    got = Kn.view_uncertainty_samples(dev_raw, B * K * 2, M * B * K * 2, M, V, B, K, torch.from_numpy(back).to(DEV),
                                      torch.full((1,), thr, device=DEV))[-1]
    assert np.array_equal(got.cpu().numpy(), gate_ref)
    host, L = _one_step(models, emas, optims, args, batch)
    host = host.tolist()
    n_sel, n_ps = L.total(host, "n_sel"), L.total(host, "epc_n")
    print("n_sel %d n_pseudo %d" % (n_sel, n_ps))
    assert n_sel == len(models) * CFG["A"] * CFG["S"] * int(gate_ref.sum())
    assert n_ps > 0


def test_score_and_uncertainty_with_a_huge_threshold_is_the_score_rule(eager):
    bias = 1.0
    raw, back, scores = _teacher_peaks(head_bias=bias)
    ref = VR.view_gate(raw, back, 1e9)
    assert ref["legal"].all() and ref["gate"].all()                   # every member legal: the gate is all ones
    low = 1e-3                                                         # a low score threshold: some rows pass
    assert (scores >= low).all()
    a = _setup(bias, pseudoScoreThr=low)
    host_a, L = _one_step(*a, _batches()[0])
    assert L.total(host_a.tolist(), "n_sel") > 0
    b = _setup(bias, pseudoScoreThr=low, pseudoRule="score+uncertainty", distThrMax=1e9)
    host_b, _ = _one_step(*b, _batches()[0])
    assert _eq(host_a, host_b)
    sa, sb = _state(*a[:3]), _state(*b[:3])
    for k in sa:
        assert _eq(sa[k], sb[k]), k


def test_captured_step_matches_eager(monkeypatch):
    """Four steps over two alternating batches (two eager warm-ups, the capture with its first
    replay, one more replay with other matrices), then two more at a second distThrMax (a
    re-capture): records and every buffer bit-equal to the eager run."""
    from ubpl_amd import train as T
    raw, back, _ = _teacher_peaks()
    thr = _threshold_with_both(raw, back)
    assert thr is not None
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("UBPL_MODEL_STREAMS", "1")
        monkeypatch.setenv("UBPL_STEP_GRAPH", mode)
        T._StepGraph.clear()
        models, emas, optims, args = _setup(pseudoRule="uncertainty", distThrMax=thr)
        b = _batches()
        rec1, _ = _train([b[i % 2] for i in range(4)], models, emas, optims, args)
        if mode == "1":
            runner = T._StepGraph.get(T._mt_ubpl_core, models, emas, optims, args)
            assert runner.graph is not None and runner.n_eager == T._StepGraph.WARM
        mid = _state(models, emas, optims)
        args.distThrMax = 2.5 * thr
        rec2, _ = _train([b[0], b[1]], models, emas, optims, args)
        if mode == "1":
            runner = T._StepGraph.get(T._mt_ubpl_core, models, emas, optims, args)
            assert runner.graph is not None and runner.n_eager == T._StepGraph.WARM
        runs[mode] = (rec1, rec2, mid, _state(models, emas, optims))
        T._StepGraph.clear()
    e, g = runs["0"], runs["1"]
    assert e[0] == g[0] and e[1] == g[1], (e[:2], g[:2])
    for k in e[2]:
        assert _eq(e[2][k], g[2][k]), k
        assert _eq(e[3][k], g[3][k]), k


def test_default_step_makes_no_new_call(eager, monkeypatch):
    from ubpl_amd import _lib
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a[0] if a else None)), real(name, *a))[1])
    _one_step(*_setup(), _batches()[0])                                # no new args, viewmat in the batch or not
    names = [n for n, _ in calls]
    assert "ubpl_loss_finalize" in names
    assert not any(n in ("ubpl_view_uncertainty_samples", "ubpl_view_uncertainty", "ubpl_decode_heatmaps_flip",
                         "ubpl_refine_peaks") for n in names)
    assert not any(n == "ubpl_loss_finalize" and kind == 3 for n, kind in calls)
    before = sorted(names)
    calls.clear()
    _one_step(*_setup(pseudoRule="uncertainty", distThrMax=4.0), _batches()[0])
    names = [n for n, _ in calls]
    extra = list(names)
    for n in before:
        extra.remove(n)
    A = CFG["A"]
    assert sorted(extra) == ["ubpl_decode_heatmaps_flip"] * A + ["ubpl_refine_peaks"] * A + \
        ["ubpl_view_uncertainty_samples"]                               # 2A + 1 launches more
    kinds = [kind for n, kind in calls if n == "ubpl_loss_finalize"]
    assert kinds.count(3) == 2 * A and 2 not in kinds


def test_batch_line_shows_the_threshold(eager):
    models, emas, optims, args = _setup(pseudoRule="score+uncertainty", distThrMax=4.0, pseudoScoreThr=1e-3)
    _, out = _train(_batches()[:1], models, emas, optims, args)
    assert "(scoreThr:0.00 distThr:4.00)" in out
    _, out = _train(_batches()[:1], *_setup(pseudoScoreThr=1e-3))
    assert "distThr" not in out and "(scoreThr:0.00)" in out


def test_errors_before_any_launch(eager, monkeypatch):
    from ubpl_amd import _lib
    from ubpl_amd import train as T
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    views, _, meta = _batches()[0]
    on = dict(pseudoRule="uncertainty", distThrMax=4.0)
    no_mats = {k: v for k, v in meta.items() if k != "viewmat"}
    with pytest.raises(ValueError, match='needs meta\\["viewmat"\\]'):
        _train([(views, None, no_mats)], *_setup(**on))
    one = {"kps": meta["kps"][:1], "islabeled": meta["islabeled"], "viewmat": meta["viewmat"][:1]}
    with pytest.raises(ValueError, match="at least 2"):
        _train([(views[:1], None, one)], *_setup(**on))
    with pytest.raises(ValueError, match="needs distThrMax"):
        _train([(views, None, meta)], *_setup(pseudoRule="uncertainty"))
    with pytest.raises(ValueError, match="pseudoRule is one of"):
        _train([(views, None, meta)], *_setup(pseudoRule="views", distThrMax=1.0))
    models, emas, optims, args = _setup(**on)
    with pytest.raises(ValueError, match="train_mt_ubpl only"):
        with contextlib.redirect_stdout(io.StringIO()):
            T.train_dualpose_ubpl([(views[0], None, views[1], {"kps": meta["kps"][0],
                                                               "islabeled": meta["islabeled"][0]})],
                                  models, emas, optims, args)
    with pytest.raises(ValueError, match="train_mt_ubpl only"):
        T.train_mt([(views, None, meta)], models[0], emas[0], optims[0], args)
    assert calls == []                                                 # nothing was launched


def test_back_map_of_rendered_targets():
    """Both views' transformed keypoints rendered (render_batch), decoded, refined and mapped back:
    the two views of a visible in-frame joint land within one heatmap cell of each other in source
    pixels, and Taylor's sub-pixel peaks closer on average than the integer ones.

    One cell in source pixels is (R/H) * sqrt(|det viewmat|) of a view; the bound is the smaller
    of the two views' cells.  Every joint the renderer calls visible in both views counts, those
    near the border where the refinement falls back from Taylor to the quarter offset included."""
    from ubpl_amd import kernels as Kn
    from ubpl_amd.augment import DeviceAugment
    from ubpl_amd.process import render_batch
    imgs, kps, isl, means = _mouse()
    rows = [i for i in range(20) if isl[i]]
    R, H, K = 256, 64, 9
    aug = DeviceAugment(imgs, means, inp_res=R, device=DEV)
    random.seed(5)
    torch.manual_seed(5)
    raws, subs, mats, vis = [], [], [], []
    taps = Kn.blur_taps(1.0).to(DEV)
    for _ in range(2):
        _, k, m = aug.views(rows, kps[rows], with_mats=True)
        hm, kk = render_batch(k, (R, R), R, H)
        r, _, _ = Kn.decode_heatmaps(hm)
        s, _, how = Kn.refine_peaks(hm, None, K * H * H, len(rows), K, H, H, None, r, "taylor", taps)
        raws.append(r)
        subs.append(s)
        mats.append(m)
        vis.append(kk[:, :, 2] > 0)                                  # visible and in frame (the renderer's test)
        print("view: %d visible joints, %d of them refined by Taylor" % (int(vis[-1].sum()),
                                                                         int((vis[-1] & (how == 2)).sum())))
    N = len(rows)
    back = Kn.train_back_matrices(mats, R, H)
    thr = torch.full((1,), 1e9, device=DEV)
    ok = (vis[0] & vis[1]).cpu().numpy()
    det = torch.stack(mats).cpu().double()
    cell = (R / H) * (det[..., 0] * det[..., 4] - det[..., 1] * det[..., 3]).abs().sqrt()     # [2,N]
    bound = cell.min(0).values.numpy()[:, None]
    dist = {}
    for name, pk in (("integer", raws), ("taylor", subs)):
        out = Kn.view_uncertainty_samples(torch.stack(pk).reshape(-1), N * K * 2, N * K * 2, 1, 2, N, K, back, thr)
        legal, int_dist = out[1][0].cpu().numpy(), out[2][0].cpu().numpy()
        assert (legal[ok] > 0).all()
        dist[name] = int_dist
        print(name, "int_dist mean %.3f max %.3f px over %d joints; cell %.2f to %.2f px; worst ratio %.3f"
              % (int_dist[ok].mean(), int_dist[ok].max(), ok.sum(), bound.min(), bound.max(),
                 (int_dist / bound)[ok].max()))
    assert ok.sum() >= 10
    assert (dist["taylor"][ok] < np.broadcast_to(bound, ok.shape)[ok]).all()
    assert dist["taylor"][ok].mean() < dist["integer"][ok].mean()
