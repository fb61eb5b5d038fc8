"""CPU-only checks of the inference layer: the three new torch ops check their
arguments before the call, the flip pairs are validated on the host, and the
Predictor fails loudly without a GPU."""
import os

import pytest
import torch


def _ops():
    from ubpl_amd import _lib
    if not os.path.exists(_lib.OPS_PATH):
        pytest.skip("libubpl_ops.so not built (run __graft_entry__.build())")
    return _lib.load_ops()


def test_decode_flip_op_checks_arguments_before_the_call():
    ops = _ops()
    N, K, H, W = 2, 3, 4, 5
    S = 2
    sb, last = S * K * H * W, (S - 1) * K * H * W
    out = torch.zeros(2 * N * sb)
    hm, hf = out[last:], out[N * sb + last:]
    assert hf.numel() == (N - 1) * sb + K * H * W               # exactly what the strided rows need
    perm = torch.arange(K, dtype=torch.int32)
    tinv = torch.zeros(N * 6, dtype=torch.float64)
    merged, raw, preds, scores = torch.zeros(N * K * H * W), torch.zeros(N * K * 2), torch.zeros(N * K * 2), \
        torch.zeros(N * K)
    call = lambda **kw: ops.decode_heatmaps_flip(*[kw.get(n, v) for n, v in (
        ("hm", hm), ("hm_flip", hf), ("sb", sb), ("N", N), ("K", K), ("H", H), ("W", W), ("perm", perm),
        ("tinv", tinv), ("merged", merged), ("raw", raw), ("preds", preds), ("scores", scores))])
    with pytest.raises(RuntimeError, match="merged holds %d elements" % (N * K * H * W - 1)):
        call(merged=merged[1:])
    with pytest.raises(RuntimeError, match="hm_flip holds %d elements" % (hf.numel() - 1)):
        call(hm_flip=hf[1:])
    with pytest.raises(RuntimeError, match="hm holds"):
        call(hm=out[N * sb + last + 1:])
    with pytest.raises(RuntimeError, match="perm must be i32"):
        call(perm=perm.long())
    with pytest.raises(RuntimeError, match="perm holds 2 elements"):
        call(perm=perm[:2])
    with pytest.raises(RuntimeError, match="tinv must be f64"):
        call(tinv=tinv.float())
    with pytest.raises(RuntimeError, match="scores holds"):
        call(scores=scores[:-1])
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        call()                                                   # every check passes: refused on CPU
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        call(hm_flip=None, perm=None, tinv=None, merged=None, preds=None, scores=None)


def test_fliplr_and_bn_table_ops_check_arguments_before_the_call():
    ops = _ops()
    x, y = torch.zeros(2 * 3 * 5), torch.zeros(2 * 3 * 5)
    with pytest.raises(RuntimeError, match="y holds 29 elements"):
        ops.fliplr(x, 2, 3, 5, y[1:])
    with pytest.raises(RuntimeError, match="x must be f32"):
        ops.fliplr(x.double(), 2, 3, 5, y)
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        ops.fliplr(x, 2, 3, 5, y)
    nbn = 4
    params, stats, coef = torch.zeros(64), torch.zeros(64), torch.zeros(2 * nbn)
    table = torch.zeros(nbn * 6, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="coef holds 7 elements"):
        ops.bn_eval_coeffs_table(params, stats, table, nbn, 1e-5, coef[1:])
    with pytest.raises(RuntimeError, match="table must be i64"):
        ops.bn_eval_coeffs_table(params, stats, table.int(), nbn, 1e-5, coef)
    with pytest.raises(RuntimeError, match="table holds 23 elements"):
        ops.bn_eval_coeffs_table(params, stats, table[1:], nbn, 1e-5, coef)
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        ops.bn_eval_coeffs_table(params, stats, table, nbn, 1e-5, coef)


def test_bn_table_rows_are_checked_against_the_buffers():
    """The op can bound coef only from below (2 floats per BatchNorm); the host table
    builder checks every row's offsets against the real sizes."""
    from ubpl_amd import kernels as Kn
    t = Kn.bn_coeff_table([(0, 8, 0, 8, 0, 8), (16, 20, 16, 20, 32, 4)], 24, 24, 48)
    assert t.dtype == torch.int64 and t.shape == (2, 6)
    for rows, sizes in (([(0, 8, 0, 8, 0, 8)], (16, 16, 15)),           # a short coef
                        ([(0, 9, 0, 8, 0, 8)], (16, 16, 32)),           # beta past params
                        ([(0, 8, 0, 9, 0, 8)], (16, 16, 32)),           # rvar past stats
                        ([(0, 8, 0, 8, -1, 8)], (16, 16, 32)),
                        ([(0, 8, 0, 8, 0, 0)], (16, 16, 32))):
        with pytest.raises(ValueError, match="BatchNorm table row"):
            Kn.bn_coeff_table(rows, *sizes)


def test_flip_pairs_are_validated_on_the_host():
    from ubpl_amd import kernels as Kn
    p = Kn.flip_perm(6, [(0, 1), (4, 2)])
    assert p.dtype == torch.int32 and p.tolist() == [1, 0, 4, 3, 2, 5]
    assert Kn.flip_perm(3, []).tolist() == [0, 1, 2]
    for bad in ([(0, 6)], [(-1, 2)], [(0, 1), (1, 2)], [(3, 3)], [(0, 1, 2)]):
        with pytest.raises(ValueError, match="flip pair"):
            Kn.flip_perm(6, bad)


def test_predictor_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ubpl_amd
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ubpl_amd.Predictor([])
