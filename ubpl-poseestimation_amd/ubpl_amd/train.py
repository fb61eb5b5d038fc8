"""T1 — the training step of each project on the HIP path.

Same signatures, batch formats and returned records as the reference
train() functions (projects/MT_UBPL.py:157-352, projects/DualPose_UBPL.py:
156-295, projects/MT.py:161-268, projects/supervised.py:135-175), so a
project's epoch loop can call these instead.  What changes is where the work
happens:

* every loss sum AND every count stays on the device (the reference syncs
  per element, ~8k host round trips per MT_UBPL step at B=32); the step makes
  ONE device->host copy, at its end, for the records / the per-batch line;
* heatmap targets can be rendered on the device inside the step (meta["kps"]
  instead of rendered heatmaps), as the benchmark does;
* the optimiser step and the EMA teacher update are single kernels over the
  flat parameter buffers (FlatAdamW, update_ema_variables);
* under torch.distributed every normaliser is global (one tiny all-reduce of
  sums+counts after the forward) and the student gradients are SUM-reduced
  once after the backward (ubpl_amd.dist).

Reference semantics that look like bugs are kept: teachers run in train mode
and keep their own BN statistics; EMA alpha is keyed on the epoch; the FDL
term is added to both students' totals (its gradient applied twice); the
pseudo-loss normaliser counts rows with a positive weighted loss.

The pieces around the steps (step_losses, streams, step_graph, guard,
validation) are re-exported here: this module is the one import.
"""
import contextlib
import os

import torch

from . import dist as D
from . import view_gate as VG
from .guard import _configure_guard, _gd, _guard_and_restore, _guard_nets, _save_stats, _SkipWatch
from .losses import AvgCounter, sel_rank
from .parameters import ema_alpha, update_ema_variables
from .process import render_batch
from .step_graph import _collective, _drive, _LaggedRecords, _StepGraph  # noqa: F401
from .step_losses import (_dist_last, _dist_mt2_last, _fdl_record, _fdl_record_sums, _fdl_rows,  # noqa: F401
                          _fdl_total, _fdl_view, _islabeled, _mse, _mse_plain, _norm, _pseudo, _pseudo_gated,
                          _pseudo_ranked, _RecordLayout, _targets, _w)
from .streams import _backward_all, _join_merge, _ModelStreams, _OnMain, _PhaseCheck  # noqa: F401
from .validation import fold_valid_rows, gather_valid_rows, valid_batch_row, validate  # noqa: F401

# a student's second-view backward on its teacher's stream (UBPL_SPLIT_BWD=0: one stream per student)
_SPLIT_BWD = os.environ.get("UBPL_SPLIT_BWD", "1") != "0"
# teachers' forwards on their own streams (UBPL_TEACHER_STREAMS=0: on their students' streams)
_TEACHER_STREAMS = os.environ.get("UBPL_TEACHER_STREAMS", "1") != "0"
# AdamW + the EMA teacher update in one pass per model (FlatAdamW.step_and_ema);
# UBPL_FUSED_EMA=0 runs the optimizer step and update_ema_variables separately.
_FUSED_EMA = os.environ.get("UBPL_FUSED_EMA", "1") != "0"


def _sync_stats(local_sums, counts):
    """One small all-reduce: returns (global counts, global sums) — identity
    on one rank."""
    if not D.is_dist():
        return counts, local_sums
    pack = torch.cat([counts.float(), local_sums.detach().float()])
    D.allreduce_(pack)
    n = counts.numel()
    return pack[:n], pack[n:]


def _step_and_ema(models, models_ema, optims, args):
    """optims[i].step() for every student, then update_ema_variables(student,
    teacher) (projects/MT_UBPL.py:338-344, DualPose_UBPL.py:281-287); the
    teacher of model i depends only on student i's updated weights, so the
    per-model fused pass gives the same bits.  Guarded optimizers first take
    their guard and restore a skipped step's BatchNorm statistics."""
    _guard_and_restore(optims, _guard_nets(models, models_ema))
    if _FUSED_EMA and all(hasattr(o, "step_and_ema") and o.model is m for o, m in zip(optims, models)):
        a = ema_alpha(args.epo, args.ema_decay)
        for o, e in zip(optims, models_ema):
            o.step_and_ema(e, a, **_gd(o))
        return
    for o in optims:
        o.step(**_gd(o))
    for mi, m in enumerate(models):
        update_ema_variables(m, models_ema[mi], args)


# ---------------------------------------------------------------------------
# the generator steps (MT_UBPL, DualPose_UBPL): shared scaffolding
# ---------------------------------------------------------------------------
_MT_UBPL_COUNTS = ("pec_n", "epc_n", "n_sel")
_DUALPOSE_COUNTS = ("mtc_n", "pec_n", "epc_n", "c_ps", "c_sel", "e_sel")


def _exchange_sums(counts, local):
    """Exchange 1 of a generator step (`yield from`) -> (global counts, global sums): under
    torch.distributed it yields the packed SUM all-reduce, on one rank it is _sync_stats."""
    if D.is_dist():
        pack = torch.cat([counts, local.detach()])
        yield ("sum", pack)                                  # exchange 1: global sums / counts
        return pack[:counts.numel()], pack[counts.numel():]
    return _sync_stats(local, counts)


def _backward_and_step(totals, outputs, mstreams, models, models_ema, optims, args):
    """The tail of a generator step (`yield from`): backward, join, exchange 2, optimizer step + EMA."""
    _backward_all(totals, outputs if mstreams else None, mstreams)
    _join_merge(mstreams, models)
    if D.is_dist():
        yield ("grads", models)                              # exchange 2: SUM of the students' gradients
    _step_and_ema(models, models_ema, optims, args)


def _train_steps(core, decode, trainLoader, models, models_ema, optims, args, verbose):
    """One epoch of a generator step: each batch runs `core` through _StepGraph and
    `decode` folds its records, one step late, into the counters
    -> (pec_records, mtc_records, epc_records, fdc_record)."""
    M = len(models)
    pec_c, mtc_c, epc_c = ([AvgCounter() for _ in range(M)] for _ in range(3))
    fdc_c = AvgCounter()
    dev = models[0].flat_params.device
    for m in [*models, *models_ema]:
        m.train()
    _configure_guard(optims, _guard_nets(models, models_ema), args)
    runner = _StepGraph.get(core, models, models_ema, optims, args)
    lag, watch = _LaggedRecords(), _SkipWatch(optims, args)
    with lag.flushing(), watch.flushing():
        for bat, batch in enumerate(trainLoader):
            packed, *meta_h = runner.run(tuple(batch), dev)
            watch.push(bat)
            # the step's one device->host copy, read after the next step is enqueued
            lag.push(packed, lambda host, bat=bat, meta_h=meta_h: decode(
                host, bat, *meta_h, (pec_c, mtc_c, epc_c, fdc_c), args, verbose, bool(watch.optims)))
    return ([c.avg for c in pec_c], [c.avg for c in mtc_c], [c.avg for c in epc_c], fdc_c.avg)


def _pseudo_rate(n_sel, n_ps, guarded=False):
    """n_sel / n_ps as the reference's batch line computes it: Python ints, so a step
    without pseudo labels raises ZeroDivisionError (projects/MT_UBPL.py:292-293,
    DualPose_UBPL.py:212-213,238-239).  guarded (the optimizers run under the
    non-finite guard): nan instead — a poisoned batch counts no pseudo label, and its
    step is skipped and counted rather than ending the run here."""
    if guarded and int(n_ps) == 0:
        return float("nan")
    return int(n_sel) / int(n_ps)


def _pseudo_line(bat, kind, args, rate, n_sel, n_ps, scores, dist_thr=None, sel_rate=None, rate_thr=(), views=None):
    """dist_thr: the view-consistency rule's threshold, shown only when that rule is on.
    sel_rate, rate_thr: the "rate" rule's share and the step's thresholds (per model rateThr1,
    rateThr2), shown only when that rule is on.  views: "merged" / "other", shown only with
    cross-view targets."""
    thr = format(args.pseudoScoreThr, ".2f") + ("" if dist_thr is None else " distThr:" + format(dist_thr, ".2f"))
    thr += "" if sel_rate is None else " selRate:" + format(sel_rate, ".2f")
    thr += "" if views is None else " views:" + views
    tail = "" if sel_rate is None else ", rateThr: [{}]".format(", ".join(format(v, ".4f") for v in rate_thr))
    print("batch.{}{} (scoreThr:{}): {} ({}/{}), pseudo-score: [{}]{}".format(
        format(bat + 1, "5d"), kind, thr, format(rate, ".2f"),
        format(n_sel, "5d"), format(n_ps, "5d"), ", ".join(format(v, ".3f") for v in scores), tail))


# ---------------------------------------------------------------------------
# MT_UBPL
# ---------------------------------------------------------------------------
def _mt_ubpl_core(models, models_ema, optims, args, augs_imgMap, augs_heatmaps, meta):
    """One MT_UBPL step (projects/MT_UBPL.py:188-336) on the device with no
    host synchronisation, as a generator: under torch.distributed it yields
    its two exchanges (see _collective), and it returns the packed records
    [3M+1 losses | counts | pseudo scores] as ONE device tensor, their
    _RecordLayout and the host-side constants the layout cannot carry.  Run it
    with _drive (eager) or _StepGraph (captured: one graph on one rank, one
    graph segment per collective-free stretch under torch.distributed)."""
    M = len(models)
    dev = models[0].flat_params.device
    S = args.nStack
    A = len(augs_imgMap)
    use_ep = getattr(args, "useEnsemblePseudo", True)        # :271 (False: epc = 0, no print)
    rule = VG.options(args)                              # the view-consistency rule (off: the score rule)
    gated = rule.on and use_ep
    ranked = rule.sel_rate is not None and use_ep        # the "rate" rule: JointPseudoLoss2 for JointPseudoLoss3
    cross = rule.cross and use_ep                        # pseudoViews "merged" / "other": cross-view targets
    if gated or cross:
        VG.check_batch(rule, meta, A, M)                     # ValueError before any launch
    for o in optims:
        o.zero_grad()
    _save_stats(optims, _guard_nets(models, models_ema))
    imgs = [x.to(dev, non_blocking=True).float().contiguous() for x in augs_imgMap]
    hms, gates = _targets(imgs, augs_heatmaps, meta, A, dev, args)
    isl = _islabeled(meta["islabeled"][0], dev)
    sw = _w(isl, 1.0, 0.0)                                   # getSampleWeight
    nega = _w(isl, 0.0, args.pseudoWeight)                   # getSampleWeight_nega
    B = imgs[0].shape[0]
    outs, feats, outs_ema = [], [], []
    mstreams = _ModelStreams.make(M, dev)
    split_bwd = mstreams is not None and _SPLIT_BWD
    for mi in range(M):                                      # :228-243
        oa, fa, ea = [], [], []
        with (mstreams.on(mi) if mstreams else contextlib.nullcontext()):
            for a in range(A):
                # views >= 1: their backward runs on the teacher's stream (idle by
                # then) into the alternate gradient buffer, beside view 0's
                models[mi]._bwd_stream = mstreams.side[M + mi] if split_bwd and a >= 1 else None
                o, f = models[mi](imgs[a])
                models[mi]._bwd_stream = None
                oa.append(o)
                fa.append(f)
        with (mstreams.on_teacher(mi) if mstreams and _TEACHER_STREAMS else
              mstreams.on(mi) if mstreams else contextlib.nullcontext()):
            for a in range(A):
                with torch.no_grad():
                    ea.append(models_ema[mi](imgs[a])[0])
        outs.append(oa)
        feats.append(fa)
        outs_ema.append(ea)
    if mstreams:
        mstreams.join([t for grp in (outs, feats, outs_ema) for ts in grp for t in ts])
        # the losses' gradients for each student output are summed on main
        outs = [[_OnMain.apply(t) for t in ts] for ts in outs]
        feats = [[None if t is None else _OnMain.apply(t) for t in ts] for ts in feats]
    K = outs[0][0].shape[2]
    zero = torch.zeros((), device=dev)
    zcnt = torch.zeros(4, dtype=torch.int32, device=dev)
    if cross:
        # the teachers' last stacks of every view in one buffer, on the main stream after the join:
        # merged across the views into every view's targets (one launch), and decoded for the gate
        with torch.no_grad():
            last = torch.stack([torch.stack([outs_ema[j][a][:, -1] for j in range(M)]) for a in range(A)])
            xt = VG.cross_view_targets(rule, last, meta["viewmat"], imgs[0].shape[-1])
            tgs = [xt[a].unsqueeze(2) for a in range(A)]     # [M,B,1,K,H,W]: the pseudo losses' St = 1
            if gated:                                        # (the gate is each view's own maps' business)
                gate = VG.view_gate(rule, [last[a].unsqueeze(2) for a in range(A)], meta["viewmat"],
                                    imgs[0].shape[-1])
    elif gated:
        # the teachers' stacked outputs per view, built once: decoded for the gate here, on the
        # main stream after the join, and shared by the students' pseudo losses below
        with torch.no_grad():
            tgs = [torch.stack([outs_ema[j][a] for j in range(M)]) for a in range(A)]
            gate = VG.view_gate(rule, tgs, meta["viewmat"], imgs[0].shape[-1])
    # ---- loss sums / counts on device
    sums, ps_scores, rate_thrs = [], [], []
    rank = sel_rank(B * K, rule.sel_rate) if ranked else None     # a host integer: B and K are static
    for mi in range(M):
        ms, thr_m = [], []
        for a in range(A):
            s_d, _ = _dist_last(outs[mi][a], outs_ema[mi][a])
            s_p, c_p = _mse(outs[mi][a], hms[a], S, gates[a], sw.reshape(-1, 1))
            if gated:
                s_e, c_e, sc_e = _pseudo_gated(outs[mi][a], tgs[a], nega, S, rule.thr, gate)
                ps_scores.append(sc_e)
            elif ranked:
                tg = tgs[a] if cross else torch.stack([outs_ema[j][a] for j in range(M)])
                s_e, c_e, sc_e, thr = _pseudo_ranked(outs[mi][a], tg, nega, S, rank)
                ps_scores.append(sc_e)
                thr_m.append(thr)                            # rateThr1 [S], rateThr2 [S]
            elif use_ep:
                tg = tgs[a] if cross else torch.stack([outs_ema[j][a] for j in range(M)])
                s_e, c_e, sc_e = _pseudo(outs[mi][a], tg, nega, S, args.pseudoScoreThr)
                ps_scores.append(sc_e)
            else:
                s_e, c_e = zero, zcnt
            ms.append((s_d, s_p, c_p, s_e, c_e))
        sums.append(ms)
        rate_thrs += thr_m
    fd = []
    if args.FDLWeight > 0:
        rowmask = _fdl_rows(sw, args)
        for a in range(A):                                   # :301-330 selected rows
            fd.append(_fdl_view(feats[0][a], feats[1][a], rowmask, args))
    # pack: per model the views' sums and counts, by name; then per FDL view sum / count
    per = [{"mtc": sum(x[0] for x in ms), "pec": sum(x[1] for x in ms), "epc": sum(x[3] for x in ms),
            "pec_n": sum(x[2][0] for x in ms), "epc_n": sum(x[4][1] for x in ms), "n_sel": sum(x[4][2] for x in ms)}
           for ms in sums]
    L = _RecordLayout(M, _MT_UBPL_COUNTS, len(fd), K, rate_thr=ranked)
    loc = [p[n] for p in per for n in L.SUMS] + _fdl_record_sums(fd)
    cn = [p[n] for p in per for n in L.counts] + [n[0] for _, _, n in fd]
    counts = torch.stack([c.float() for c in cn])
    local = torch.stack([l.float() for l in loc])
    gcounts, gsums = yield from _exchange_sums(counts, local)
    W = D.world()
    mtc_n = A * B * K * W
    totals = []
    fdc = _fdl_total(fd, gcounts[L.fdl_counts], W, args.FDLWeight) if fd else 0.
    for mi in range(M):
        mtc = args.consWeight * (loc[L.s("mtc", mi)] / mtc_n)
        pec = args.poseWeight * _norm(loc[L.s("pec", mi)], gcounts[L.c("pec_n", mi)])
        epc = args.ensemblePseudoWeight * _norm(loc[L.s("epc", mi)], gcounts[L.c("epc_n", mi)]) if use_ep else 0.
        totals.append(pec + mtc + epc + fdc)
    yield from _backward_and_step(totals, [t for grp in (outs, feats) for ts in grp for t in ts], mstreams,
                                  models, models_ema, optims, args)                            # :334-344
    # ---- records: one device->host copy
    g_rec = []
    for mi in range(M):
        r = {"pec": args.poseWeight * _norm(gsums[L.s("pec", mi)], gcounts[L.c("pec_n", mi)]),
             "mtc": args.consWeight * gsums[L.s("mtc", mi)] / mtc_n,
             "epc": (args.ensemblePseudoWeight * _norm(gsums[L.s("epc", mi)], gcounts[L.c("epc_n", mi)])
                     if use_ep else zero)}
        g_rec += [r[n] for n in L.RECS]
    g_rec.append(_fdl_record(fd, gsums[L.fdl_sums], gcounts[L.fdl_counts], W, args.FDLWeight) if fd else zero)
    score = torch.stack(ps_scores).mean(0) if use_ep else torch.zeros(K, device=dev)
    blocks = [torch.stack([r.float() for r in g_rec]), gcounts, score]
    if ranked:                                               # per model: the mean over views and stacks of each
        blocks.append(torch.stack(rate_thrs).view(M, A, 2, S).mean((1, 3)).reshape(-1))
    return torch.cat(blocks), L, mtc_n, B, use_ep


def _mt_ubpl_records(host, bat, L, mtc_n, B, use_ep, counters, args, verbose, guarded=False):
    """One MT_UBPL step's host records -> the AvgCounters and the batch line.
    guarded: a step without pseudo labels prints a nan rate (see _pseudo_rate)."""
    pec_c, mtc_c, epc_c, fdc_c = counters
    for mi in range(L.M):
        pec_c[mi].update(host[L.r("pec", mi)], int(host[L.n("pec_n", mi)]))
        mtc_c[mi].update(host[L.r("mtc", mi)], mtc_n)
        # useEnsemblePseudo False: epc_counter.update(0., outs.shape[2]) (:292-293; outs.shape[2] = B)
        epc_c[mi].update(host[L.r("epc", mi)], int(host[L.n("epc_n", mi)]) if use_ep else B)
    if L.nfd:
        fdc_c.update(host[L.fdc], int(sum(host[L.fdl_n])))
    else:
        fdc_c.update(0., B)
    if use_ep:
        n_ps, n_sel = L.total(host, "epc_n"), L.total(host, "n_sel")
        # the reference's batch line divides by the pseudo-label count whether or not it
        # prints anywhere (projects/MT_UBPL.py:292-293, integer counts): a step with none
        # raises ZeroDivisionError there, and here when its records are consumed
        rate = _pseudo_rate(n_sel, n_ps, guarded)
        if verbose:
            rule = VG.options(args)
            _pseudo_line(bat, "", args, rate, n_sel, n_ps, host[L.scores()], rule.dist_thr if rule.on else None,
                         rule.sel_rate if L.rate_thr else None, host[L.rate_thr] if L.rate_thr else (),
                         rule.views if rule.cross else None)


def train_mt_ubpl(trainLoader, models, models_ema, optims, args, verbose=True, pseudo_counts=None):
    """projects/MT_UBPL.py:157-352 -> (pec_records, mtc_records, epc_records, fdc_record).
    Steps after the first two are replayed from a captured HIP graph when the
    batch shapes repeat (UBPL_STEP_GRAPH=0: every step eager).
    args.pseudoRule "uncertainty" / "score+uncertainty" (with args.distThrMax; pseudoRefine,
    pseudoBlurSigma) selects the pseudo labels by the view-consistency rule (view_gate.py); the
    batches then carry meta["viewmat"].  args.pseudoRule "rate" (with args.pseudoSelRate in (0, 1])
    keeps that share of every batch's joints, ranked by softmax score: JointPseudoLoss2 in
    JointPseudoLoss3's place ("Rank-based pseudo-label selection").  pseudo_counts: a
    dict that receives the epoch's totals of the steps' pseudo-label counts, "n_pseudo" and "n_sel"
    (what the active rule selected), and under the "rate" rule "steps" and the sums over the steps of
    the models' mean thresholds, "rate_thr1" and "rate_thr2".
    args.pseudoViews "merged" / "other" (default "own") takes the pseudo loss' targets of a view from
    every view's teacher maps warped into its frame, with or without its own (DESIGN.md §4,
    "Cross-view pseudo-label targets"); the batches then carry meta["viewmat"].  It combines with
    every pseudoRule."""
    rule = VG.options(args)
    if rule.on:
        VG.constants(rule, models[0].flat_params.device)     # host -> device, ahead of any capture

    def records(host, bat, L, mtc_n, B, use_ep, *rest):
        if pseudo_counts is not None and use_ep:             # the step's own counts, summed over the epoch
            pseudo_counts["n_sel"] = pseudo_counts.get("n_sel", 0) + L.total(host, "n_sel")
            pseudo_counts["n_pseudo"] = pseudo_counts.get("n_pseudo", 0) + L.total(host, "epc_n")
            if L.rate_thr:
                t = host[L.rate_thr]
                pseudo_counts["steps"] = pseudo_counts.get("steps", 0) + 1
                pseudo_counts["rate_thr1"] = pseudo_counts.get("rate_thr1", 0.) + sum(t[0::2]) / L.M
                pseudo_counts["rate_thr2"] = pseudo_counts.get("rate_thr2", 0.) + sum(t[1::2]) / L.M
        return _mt_ubpl_records(host, bat, L, mtc_n, B, use_ep, *rest)
    return _train_steps(_mt_ubpl_core, records, trainLoader, models, models_ema, optims, args, verbose)


# ---------------------------------------------------------------------------
# DualPose_UBPL
# ---------------------------------------------------------------------------
def _dualpose_core(models, models_ema, optims, args, stu_imgMap, stu_heatmap, ema_imgMap, meta):
    """One DualPose_UBPL step (projects/DualPose_UBPL.py:170-290) on the device
    with no host synchronisation, as a generator like _mt_ubpl_core: it yields
    its two exchanges under torch.distributed and returns the packed records
    [3M+1 losses | counts | consistency scores | pseudo scores], their
    _RecordLayout and the host-side constants the layout cannot carry."""
    VG.refuse(args, "train_dualpose_ubpl")
    M = len(models)
    dev = models[0].flat_params.device
    S = args.nStack
    for o in optims:
        o.zero_grad()
    _save_stats(optims, _guard_nets(models, models_ema))
    si = stu_imgMap.to(dev, non_blocking=True).float().contiguous()
    ei = ema_imgMap.to(dev, non_blocking=True).float().contiguous()
    if stu_heatmap is None:
        hm, kk = render_batch(meta["kps"].to(dev).float(), (si.shape[-2], si.shape[-1]), si.shape[-1],
                              si.shape[-1] // 4)
        gate = kk[:, :, 2].contiguous()
    else:
        hm = stu_heatmap.to(dev, non_blocking=True).float().contiguous()
        gate = meta["kpsWeight"].to(dev, non_blocking=True).float().contiguous()
    isl = _islabeled(meta["islabeled"], dev)
    sw = _w(isl, 1.0, 0.0)
    nega = _w(isl, 0.0, args.pseudoWeight)
    cons = _w(isl, 1.0, args.pseudoWeight)
    outs, feats, ema_l = [], [], []
    mstreams = _ModelStreams.make(M, dev)                    # one HIP stream per network
    for mi in range(M):                                       # :185-196
        with (mstreams.on(mi) if mstreams else contextlib.nullcontext()):
            o, f = models[mi](si)
        outs.append(o)
        feats.append(f)
        with (mstreams.on_teacher(mi) if mstreams else contextlib.nullcontext()), torch.no_grad():
            ema_l.append(models_ema[mi](ei)[0])
    if mstreams:
        mstreams.join(outs + feats + ema_l)
        outs = [_OnMain.apply(t) for t in outs]
        feats = [None if t is None else _OnMain.apply(t) for t in feats]
    outs_ema = torch.stack(ema_l)
    use_ep = getattr(args, "useEnsemblePseudo", True)    # :224 (False: epc = 0, no print)
    K = outs[0].shape[2]
    zero = torch.zeros((), device=dev)
    per, cons_sc, ps_sc = [], [], []
    for mi in range(M):
        s_c, c_c, sc_c = _dist_mt2_last(outs[mi], outs_ema[mi], cons, args.pseudoScoreThr)
        s_p, c_p = _mse(outs[mi], hm, S, gate, sw.reshape(-1, 1))
        if use_ep:
            s_e, c_e, sc_e = _pseudo(outs[mi], outs_ema, nega, S, args.pseudoScoreThr)
            ps_sc.append(sc_e)
        else:
            s_e, c_e = zero, torch.zeros(4, dtype=torch.int32, device=dev)
        per.append({"mtc": s_c, "pec": s_p, "epc": s_e, "mtc_n": c_c[0], "pec_n": c_p[0], "epc_n": c_e[1],
                    "c_ps": c_c[1], "c_sel": c_c[2], "e_sel": c_e[2]})
        cons_sc.append(sc_c)
    fd = []
    if args.FDLWeight > 0:                                     # :246-270 (one view)
        fd.append(_fdl_view(feats[0], feats[1], _fdl_rows(sw, args), args))
    L = _RecordLayout(M, _DUALPOSE_COUNTS, len(fd), K, blocks=2)
    loc = [p[n] for p in per for n in L.SUMS] + _fdl_record_sums(fd)
    cn = [p[n] for p in per for n in L.counts] + [n[0] for _, _, n in fd]
    counts = torch.stack([c.float() for c in cn])
    local = torch.stack([l.float() for l in loc])
    gcounts, gsums = yield from _exchange_sums(counts, local)
    W = D.world()
    fdc = _fdl_total(fd, gcounts[L.fdl_counts], W, args.FDLWeight) if fd else 0.
    totals = []
    for mi in range(M):
        mtc = args.consWeight * _norm(loc[L.s("mtc", mi)], gcounts[L.c("mtc_n", mi)])
        pec = args.poseWeight * _norm(loc[L.s("pec", mi)], gcounts[L.c("pec_n", mi)])
        epc = args.ensemblePseudoWeight * _norm(loc[L.s("epc", mi)], gcounts[L.c("epc_n", mi)]) if use_ep else 0.
        totals.append(pec + mtc + epc + fdc)
    yield from _backward_and_step(totals, outs + feats, mstreams, models, models_ema, optims, args)   # :277-287
    g_rec = []
    for mi in range(M):
        r = {"pec": args.poseWeight * _norm(gsums[L.s("pec", mi)], gcounts[L.c("pec_n", mi)]),
             "mtc": args.consWeight * _norm(gsums[L.s("mtc", mi)], gcounts[L.c("mtc_n", mi)]),
             "epc": (args.ensemblePseudoWeight * _norm(gsums[L.s("epc", mi)], gcounts[L.c("epc_n", mi)])
                     if use_ep else zero)}
        g_rec += [r[n] for n in L.RECS]
    g_rec.append(_fdl_record(fd, gsums[L.fdl_sums], gcounts[L.fdl_counts], W, args.FDLWeight) if fd else zero)
    packed = torch.cat([torch.stack([r.float() for r in g_rec]), gcounts, torch.stack(cons_sc).mean(0),
                        torch.stack(ps_sc).mean(0) if use_ep else torch.zeros(K, device=dev)])
    return packed, L, use_ep, S


def _dualpose_records(host, bat, L, use_ep, S, counters, args, verbose, guarded=False):
    """One DualPose_UBPL step's host records -> the AvgCounters and the batch lines."""
    pec_c, mtc_c, epc_c, fdc_c = counters
    for mi in range(L.M):
        pec_c[mi].update(host[L.r("pec", mi)], int(host[L.n("pec_n", mi)]))
        mtc_c[mi].update(host[L.r("mtc", mi)], int(host[L.n("mtc_n", mi)]))
        # useEnsemblePseudo False: epc_counter.update(0., outs.shape[2]) (:244-245; outs.shape[2] = nStack)
        epc_c[mi].update(host[L.r("epc", mi)], int(host[L.n("epc_n", mi)]) if use_ep else S)
    if L.nfd:
        fdc_c.update(host[L.fdc], int(sum(host[L.fdl_n])))
    else:
        fdc_c.update(0., S)                                   # :249 outs.shape[2] = nStack
    c_ps, c_sel = L.total(host, "c_ps"), L.total(host, "c_sel")
    e_ps, e_sel = L.total(host, "epc_n"), L.total(host, "e_sel")
    c_rate = _pseudo_rate(c_sel, c_ps, guarded)               # (the reference's lines raise on a zero count)
    e_rate = _pseudo_rate(e_sel, e_ps, guarded) if use_ep else None
    if verbose:
        _pseudo_line(bat, " consist-pseudo", args, c_rate, c_sel, c_ps, host[L.scores(0)])
        if use_ep:
            _pseudo_line(bat, " ensemble-pseudo", args, e_rate, e_sel, e_ps, host[L.scores(1)])


def train_dualpose_ubpl(trainLoader, models, models_ema, optims, args, verbose=True):
    """projects/DualPose_UBPL.py:156-295.  Like train_mt_ubpl, steps after the
    first two replay a captured HIP graph when the batch shapes repeat."""
    return _train_steps(_dualpose_core, _dualpose_records, trainLoader, models, models_ema, optims, args, verbose)


# ---------------------------------------------------------------------------
# MT and supervised
# ---------------------------------------------------------------------------
def train_mt(trainLoader, model, model_ema, optim, args):
    """projects/MT.py:161-268 -> (pec_avg, mtc_avg)."""
    VG.refuse(args, "train_mt")
    pec_c, mtc_c = AvgCounter(), AvgCounter()
    dev = model.flat_params.device
    S = args.nStack
    model.train()
    model_ema.train()
    pick = (lambda r: r) if args.feature_mode == "default" else (lambda r: r[0])
    nets = _guard_nets([model], [model_ema])
    _configure_guard([optim], nets, args)
    watch = _SkipWatch([optim], args)
    with watch.flushing():
        for bat, (augs_imgMap, augs_heatmaps, meta) in enumerate(trainLoader):
            optim.zero_grad()
            _save_stats([optim], nets)
            A = len(augs_imgMap)
            imgs = [x.to(dev, non_blocking=True).float().contiguous() for x in augs_imgMap]
            hms, gates = _targets(imgs, augs_heatmaps, meta, A, dev, args)
            sw = _w(_islabeled(meta["islabeled"][0], dev), 1.0, 0.0)
            outs, outs_ema = [], []
            for a in range(A):
                outs.append(pick(model(imgs[a])))
                with torch.no_grad():
                    outs_ema.append(pick(model_ema(imgs[a])))
            B, K = outs[0].shape[0], outs[0].shape[2]
            sd = sum(_dist_last(outs[a], outs_ema[a])[0] for a in range(A))
            ps = [_mse(outs[a], hms[a], S, gates[a], sw.reshape(-1, 1)) for a in range(A)]
            sp = sum(p[0] for p in ps)
            cp = sum(p[1][0] for p in ps)
            counts, sums = _sync_stats(torch.stack([sd, sp]), cp.float().reshape(1))
            mtc_n = A * B * K * D.world()
            mtc = args.consWeight * (sd / mtc_n)
            pec = args.poseWeight * _norm(sp, counts[0])
            (pec + mtc).backward()
            D.allreduce_grads([model])
            _guard_and_restore([optim], nets)
            optim.step(**_gd(optim))
            update_ema_variables(model, model_ema, args)
            watch.push(bat)
            host = torch.stack([args.poseWeight * _norm(sums[1], counts[0]), args.consWeight * sums[0] / mtc_n,
                                counts[0]]).cpu().tolist()
            mtc_c.update(host[1], mtc_n)
            pec_c.update(host[0], int(host[2]))
    return pec_c.avg, mtc_c.avg


def train_supervised(trainLoader, model, optim, args):
    """projects/supervised.py:135-175 -> pec_avg."""
    VG.refuse(args, "train_supervised")
    pec_c = AvgCounter()
    dev = model.flat_params.device
    model.train()
    pick = (lambda r: r) if args.feature_mode == "default" else (lambda r: r[0])
    nets = _guard_nets([model], [])
    _configure_guard([optim], nets, args)
    watch = _SkipWatch([optim], args)
    with watch.flushing():
        for bat, (imgMap, heatmap, meta) in enumerate(trainLoader):
            optim.zero_grad()
            _save_stats([optim], nets)
            img = imgMap.to(dev, non_blocking=True).float().contiguous()
            hm = heatmap.to(dev, non_blocking=True).float().contiguous()
            out = pick(model(img))
            s, c = _mse_plain(out, hm, args.nStack)
            counts, sums = _sync_stats(s.reshape(1), c[0].float().reshape(1))
            pec = args.poseWeight * _norm(s, counts[0])
            pec.backward()
            D.allreduce_grads([model])
            _guard_and_restore([optim], nets)
            optim.step(**_gd(optim))
            watch.push(bat)
            host = torch.stack([args.poseWeight * _norm(sums[0], counts[0]), counts[0]]).cpu().tolist()
            pec_c.update(host[0], int(host[1]))
    return pec_c.avg
