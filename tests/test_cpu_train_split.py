"""Host-side checks of the training step's pieces (no GPU): the packed record
layout, the record decoders' counter weights, and ubpl_amd.train as the one
import for everything around the steps."""
from types import SimpleNamespace

import pytest
import torch

from ubpl_amd import train as T
from ubpl_amd.losses import AvgCounter

M, K = 2, 3


@pytest.mark.parametrize("nfd", [0, 1, 2])
def test_layout_offsets_mt_ubpl(nfd):
    """[7 records | 3 counts per model, nfd FDL counts | K scores]"""
    L = T._RecordLayout(M, T._MT_UBPL_COUNTS, nfd, K)
    assert (L.nrec, L.ncn, L.size) == (7, 6 + nfd, 16 + nfd)
    assert [L.s(n, mi) for mi in range(M) for n in ("mtc", "pec", "epc")] == [0, 1, 2, 3, 4, 5]
    assert L.fdl_sums == slice(6, 6 + nfd)
    assert [L.c(n, mi) for mi in range(M) for n in ("pec_n", "epc_n", "n_sel")] == [0, 1, 2, 3, 4, 5]
    assert L.fdl_counts == slice(6, 6 + nfd)
    assert [L.r(n, mi) for mi in range(M) for n in ("pec", "mtc", "epc")] == [0, 1, 2, 3, 4, 5]
    assert L.fdc == 6
    assert [L.n(n, mi) for mi in range(M) for n in ("pec_n", "epc_n", "n_sel")] == [7, 8, 9, 10, 11, 12]
    assert L.fdl_n == slice(13, 13 + nfd)
    assert L.scores() == slice(13 + nfd, 16 + nfd)
    host = list(range(L.size))
    assert (host[L.r("pec", 0)], host[L.r("mtc", 0)], host[L.r("epc", 1)], host[L.fdc]) == (0, 1, 5, 6)
    assert (host[L.n("pec_n", 0)], host[L.n("epc_n", 1)], host[L.n("n_sel", 1)]) == (7, 11, 12)
    assert (L.total(host, "epc_n"), L.total(host, "n_sel")) == (8 + 11, 9 + 12)
    assert host[L.fdl_n] == [13, 14][:nfd]
    assert host[L.scores()] == [13 + nfd, 14 + nfd, 15 + nfd]
    assert list(range(L.ncn))[L.fdl_counts] == [6, 7][:nfd]
    assert list(range(6 + nfd))[L.fdl_sums] == [6, 7][:nfd]


@pytest.mark.parametrize("nfd", [0, 1, 2])
def test_layout_offsets_dualpose(nfd):
    """[7 records | 6 counts per model, nfd FDL counts | K consistency scores | K pseudo scores]"""
    names = ("mtc_n", "pec_n", "epc_n", "c_ps", "c_sel", "e_sel")
    L = T._RecordLayout(M, T._DUALPOSE_COUNTS, nfd, K, blocks=2)
    assert (L.nrec, L.ncn, L.size) == (7, 12 + nfd, 25 + nfd)
    assert [L.s(n, mi) for mi in range(M) for n in ("mtc", "pec", "epc")] == [0, 1, 2, 3, 4, 5]
    assert L.fdl_sums == slice(6, 6 + nfd)
    assert [L.c(n, mi) for mi in range(M) for n in names] == list(range(12))
    assert L.fdl_counts == slice(12, 12 + nfd)
    assert [L.r(n, mi) for mi in range(M) for n in ("pec", "mtc", "epc")] == [0, 1, 2, 3, 4, 5]
    assert L.fdc == 6
    assert [L.n(n, mi) for mi in range(M) for n in names] == list(range(7, 19))
    assert L.fdl_n == slice(19, 19 + nfd)
    assert L.scores(0) == slice(19 + nfd, 22 + nfd)
    assert L.scores(1) == slice(22 + nfd, 25 + nfd)
    host = list(range(L.size))
    assert (host[L.r("pec", 1)], host[L.r("mtc", 1)], host[L.fdc]) == (3, 4, 6)
    assert (host[L.n("mtc_n", 0)], host[L.n("pec_n", 0)], host[L.n("c_sel", 1)], host[L.n("e_sel", 1)]) \
        == (7, 8, 17, 18)
    assert (L.total(host, "c_ps"), L.total(host, "c_sel"), L.total(host, "epc_n"), L.total(host, "e_sel")) \
        == (10 + 16, 11 + 17, 9 + 15, 12 + 18)
    assert host[L.fdl_n] == [19, 20][:nfd]
    assert host[L.scores(1)] == [22 + nfd, 23 + nfd, 24 + nfd]


def _counters():
    return ([AvgCounter() for _ in range(M)], [AvgCounter() for _ in range(M)], [AvgCounter() for _ in range(M)],
            AvgCounter())


@pytest.mark.parametrize("use_ep,nfd", [(False, 1), (True, 0)])
def test_mt_ubpl_records_counter_weights(use_ep, nfd):
    """Without ensemble pseudo labels / without an FDL view the reference records a
    constant 0 weighted by outs.shape[2], which in MT_UBPL is B
    (projects/MT_UBPL.py:292-293)."""
    B, mtc_n = 4, 64
    L = T._RecordLayout(M, T._MT_UBPL_COUNTS, nfd, K)
    host = [0.1] * L.nrec + [5, 3, 2] * M + [9] * nfd + [0.5] * K
    ctr = _counters()
    T._mt_ubpl_records(host, 0, L, mtc_n, B, use_ep, ctr, SimpleNamespace(pseudoScoreThr=0.95), False)
    pec_c, mtc_c, epc_c, fdc_c = ctr
    assert [c.count for c in pec_c] == [5] * M
    assert [c.count for c in mtc_c] == [mtc_n] * M
    assert [c.count for c in epc_c] == [3 if use_ep else B] * M
    assert fdc_c.count == (9 if nfd else B)
    assert fdc_c.avg == (0.1 if nfd else 0.)


@pytest.mark.parametrize("use_ep,nfd", [(False, 1), (True, 0)])
def test_dualpose_records_counter_weights(use_ep, nfd):
    """As above; in DualPose_UBPL outs.shape[2] is nStack
    (projects/DualPose_UBPL.py:244-249)."""
    S = 4
    L = T._RecordLayout(M, T._DUALPOSE_COUNTS, nfd, K, blocks=2)
    host = [0.1] * L.nrec + [6, 5, 3, 7, 1, 2] * M + [9] * nfd + [0.5] * (2 * K)
    ctr = _counters()
    T._dualpose_records(host, 0, L, use_ep, S, ctr, SimpleNamespace(pseudoScoreThr=0.95), False)
    pec_c, mtc_c, epc_c, fdc_c = ctr
    assert [c.count for c in pec_c] == [5] * M
    assert [c.count for c in mtc_c] == [6] * M
    assert [c.count for c in epc_c] == [3 if use_ep else S] * M
    assert fdc_c.count == (9 if nfd else S)
    assert fdc_c.avg == (0.1 if nfd else 0.)


# every name tests/, tools/, bench.py and predict.py read from ubpl_amd.train
FACADE = ["train_mt_ubpl", "train_dualpose_ubpl", "train_mt", "train_supervised", "validate", "valid_batch_row",
          "fold_valid_rows", "gather_valid_rows", "_StepGraph", "_ModelStreams", "_PhaseCheck", "_LaggedRecords",
          "_mt_ubpl_core", "_dualpose_core", "_mt_ubpl_records", "_dualpose_records", "_pseudo_rate", "_drive",
          "_backward_all", "_step_and_ema", "_sync_stats", "_SPLIT_BWD", "_norm", "_fdl_view", "_fdl_total",
          "_fdl_record", "_fdl_record_sums", "_RecordLayout", "_MT_UBPL_COUNTS", "_DUALPOSE_COUNTS"]


def test_train_is_the_one_import():
    missing = [n for n in FACADE if not hasattr(T, n)]
    assert not missing, missing
    assert T._StepGraph.WARM == 2 and callable(T._StepGraph.eager)
    assert (T._mt_ubpl_core.__name__, T._dualpose_core.__name__) == ("_mt_ubpl_core", "_dualpose_core")
    # the three names that are assigned to on `train` from outside are defined there and
    # read by the steps as that module's globals
    assert T._step_and_ema.__module__ == "ubpl_amd.train"
    assert T._sync_stats.__module__ == "ubpl_amd.train"
    from ubpl_amd import guard, step_graph, step_losses, streams, validation
    assert not any(hasattr(m, "_SPLIT_BWD") for m in (guard, step_graph, step_losses, streams, validation))
    assert T._mt_ubpl_core.__globals__ is vars(T) and "_SPLIT_BWD" in T._mt_ubpl_core.__code__.co_names
    assert T._backward_and_step.__globals__ is vars(T)
    assert "_step_and_ema" in T._backward_and_step.__code__.co_names
    assert T._exchange_sums.__globals__ is vars(T) and "_sync_stats" in T._exchange_sums.__code__.co_names


def test_one_rank_exchange_calls_the_patched_sync_stats(monkeypatch):
    """On one rank the steps' first exchange goes through train._sync_stats, looked
    up when it runs (tests replace it to inject global normalisers)."""
    seen = []
    monkeypatch.setattr(T, "_sync_stats", lambda s, c: (seen.append((s, c)), ("gc", "gs"))[1])
    counts, local = torch.ones(2), torch.zeros(3)
    assert T._drive(T._exchange_sums(counts, local)) == ("gc", "gs")
    assert seen == [(local, counts)]
