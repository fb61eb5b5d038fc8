"""validate: teachers in eval mode -> decode -> PCK (D1-D5).  Not part of a
training step: an epoch loop calls validate() after train_*(), and
Predictor.validate folds its own rows with the same helpers (both reach them
through ubpl_amd.train)."""
import torch

from . import dist as D
from . import kernels as Kn


def gather_valid_rows(rows):
    """Validation rows (batch_index or None, bs, k, host row) of this rank ->
    the rows to fold, in the single-device batch order.

    Under torch.distributed the rows of all ranks are gathered and ordered by
    batch_index only when EVERY row of every rank carries one (the sharded
    loader, mouse.valid_batches, sets meta['batch_index']).  A loader without
    it gives no global order — every rank may have iterated the whole set, or
    a DistributedSampler reuses indices 0..n on each rank — so then each rank
    keeps its own rows in its own order (per-rank records) and a warning says
    so.  One device: the rows as iterated."""
    if not D.is_dist():
        return rows
    import torch.distributed as dist
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else "cpu"
    tagged = torch.tensor([float(all(r[0] is not None for r in rows))], device=dev)
    dist.all_reduce(tagged, op=dist.ReduceOp.MIN)
    if tagged.item() < 1:
        import warnings
        warnings.warn("ubpl_amd.validate under torch.distributed: the loader sets no meta['batch_index'], "
                      "so the records are this rank's own (not gathered)", RuntimeWarning)
        return rows
    allrows = [None] * D.world()
    dist.all_gather_object(allrows, [(bi, bs, k, h.tolist()) for bi, bs, k, h in rows])
    return sorted(((int(bi), bs, k, torch.tensor(h)) for part in allrows for bi, bs, k, h in part),
                  key=lambda r: r[0])


def valid_batch_row(pm, meta, dev, args):
    """One validation batch's row (batch_index or None, bs, k, host tensor): the PCK
    errs | accs of every entry of pm (the teachers' transformed predictions and their
    mean, each [bs,k,2] on the device) followed by the predictions themselves, in one
    device->host copy."""
    from .evaluation import EvaluationUtils
    bs, k = meta["kpsMap"].shape[:2]
    gts = meta["kpsMap"].to(dev).float().contiguous()
    outs = [EvaluationUtils.acc_pck(p, gts, args.pck_ref, args.pck_thr) for p in pm]
    host = torch.cat([torch.cat([er, ac]) for er, ac in outs] + [p.reshape(-1) for p in pm]).cpu()
    return meta.get("batch_index"), bs, k, host


def fold_valid_rows(rows, n):
    """Rows of valid_batch_row (n entries each) -> (predsArray, accs_records,
    errs_records) with the reference's weights (projects/MT_UBPL.py:393-397: bs per
    keypoint entry, bs*k for the mean entry)."""
    from .losses import AvgCounters
    accs_c = [AvgCounters() for _ in range(n)]
    errs_c = [AvgCounters() for _ in range(n)]
    preds_arr = [[] for _ in range(n)]
    for _, bs, k, host in rows:
        for mi in range(n):
            errs = host[mi * 2 * (k + 1):mi * 2 * (k + 1) + k + 1]
            accs = host[mi * 2 * (k + 1) + k + 1:(mi + 1) * 2 * (k + 1)]
            for idx in range(k + 1):
                accs_c[mi].update(idx, accs[idx].item(), bs if idx < k else bs * k)
                errs_c[mi].update(idx, errs[idx].item(), bs if idx < k else bs * k)
        base = n * 2 * (k + 1)
        for mi in range(n):
            preds_arr[mi] += host[base + mi * bs * k * 2:base + (mi + 1) * bs * k * 2].reshape(bs, k, 2).tolist()
    return preds_arr, [c.avg() for c in accs_c], [c.avg() for c in errs_c]


def validate(validLoader, models_ema, args):
    """projects/MT_UBPL.py:355-408 -> (predsArray, accs_records, errs_records);
    entries per teacher plus their mean (brNum + 1).

    Teachers in eval mode, heatmaps decoded and scored on the device (D1-D4);
    one device->host copy per batch.  Batches are (imgMap, heatmap or None,
    meta) with meta center / scale / kpsMap.  Under torch.distributed every
    rank validates its share of the batches (mouse.valid_batches: batch i on
    rank i % world, meta['batch_index'] = i) with rank 0's teacher BatchNorm
    statistics (broadcast first: train-mode teachers keep per-rank running
    statistics); the per-batch (errs, accs, bs) rows are gathered and folded
    into the AvgCounters in the single-device batch order, so the records are
    exactly what one device computes (projects/MT_UBPL.py:393-397 weights:
    bs per keypoint entry, bs*k for the mean entry)."""
    from .process import inverse_transforms
    n = len(models_ema) + 1
    D.broadcast_buffers(models_ema)
    for e in models_ema:
        e.eval()
    dev = models_ema[0].flat_params.device
    rows = []                                    # (batch index, bs, k, host row)
    with torch.no_grad():
        for bat, (imgMap, heatmap, meta) in enumerate(validLoader):
            img = imgMap.to(dev, non_blocking=True).float().contiguous()
            tinv = inverse_transforms(meta["center"], meta["scale"], [args.outRes, args.outRes]).to(dev)
            pm = []
            for e in models_ema:
                o = e(img)
                o = o[0] if isinstance(o, tuple) else o
                _, p, _ = Kn.decode_heatmaps(o[:, -1].contiguous(), tinv)
                pm.append(p)
            pm.append(torch.stack(pm, -1).mean(-1))                   # :387 preds_mean
            rows.append(valid_batch_row(pm, meta, dev, args))
    out = fold_valid_rows(gather_valid_rows(rows), n)
    for e in models_ema:
        e.train()
    return out
