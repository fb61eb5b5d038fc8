"""The guarded step under data parallelism: two gloo ranks on the one GPU each
run one train_mt_ubpl step on half of the small seeded batch of
test_gpu_guard_train.py, with one NaN pixel on rank 1 only.  The guard runs
after the gradient all-reduce, so both ranks see the same (NaN) summed
gradients and both skip: each ends with its students, moments, step counts
and BatchNorm statistics bit-identical to its pre-step state, and the replicas
agree with each other.
"""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROWS = [[0, 2], [1, 3]]            # one unlabeled and one labeled row per rank


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _shard(obj, rows):
    if torch.is_tensor(obj):
        return obj[rows].clone() if obj.dim() and obj.shape[0] == 4 else obj
    if isinstance(obj, (list, tuple)):
        return type(obj)(_shard(v, rows) for v in obj)
    if isinstance(obj, dict):
        return {k: _shard(v, rows) for k, v in obj.items()}
    return obj


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["UBPL_STEP_GRAPH"] = "0"
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import test_gpu_guard_train as G
        from ubpl_amd import dist as D
        assert D.is_dist()
        models, emas, optims, batch, args = G._setup(skipNonFinite=True)
        imgs, hms, meta = _shard(batch, ROWS[rank])
        if rank == 1:
            imgs[0][0, 1, 9, 3] = float("nan")
        before = G._state(models, emas, optims)
        G._train([(imgs, hms, meta)], models, emas, optims, args)
        after = G._state(models, emas, optims)
        torch.save({"before": {k: v.cpu() for k, v in before.items()}, "after": {k: v.cpu() for k, v in after.items()},
                    "skipped": [o._skipped.cpu() for o in optims],
                    "grad_nan": [bool(torch.isnan(m.flat_grads).any()) for m in models]},
                   os.path.join(out, "guard_rank%d.pt" % rank))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_nan_on_one_rank_skips_on_both(tmp_path):
    import test_gpu_guard_train as G
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    rs = [torch.load(os.path.join(tmp_path, "guard_rank%d.pt" % r), weights_only=True) for r in range(2)]
    M = 2
    for r in rs:
        assert r["grad_nan"] == [True, True]                   # the all-reduce carried rank 1's NaN to rank 0
        assert [s.tolist() for s in r["skipped"]] == [[1, 1], [1, 1]]
        for bi in range(M):
            for k in ("params%d" % bi, "m%d" % bi, "v%d" % bi, "step%d" % bi, "stats%d" % bi, "stats%d" % (M + bi)):
                assert G._eq(r["before"][k], r["after"][k]), k
            assert not G._eq(r["before"]["params%d" % (M + bi)], r["after"]["params%d" % (M + bi)])   # the EMA ran
    for k in rs[0]["after"]:
        if k.startswith(("params", "m", "v", "step")):
            assert G._eq(rs[0]["after"][k], rs[1]["after"][k]), k
