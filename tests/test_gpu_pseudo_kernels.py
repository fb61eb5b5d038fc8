"""ubpl_ensemble_pseudo against the torch restatement of tests/test_pseudo_host.py (itself
pinned to oracle.losses.joint_pseudo3): bit for bit, except disagree, which is a float32
sum and is held to the project's fp32-loss bar of 1e-4 relative."""
import functools

import numpy as np
import pytest
import torch

from test_pseudo_host import member_maps, restate_pseudo

pytestmark = pytest.mark.gpu
DEV = "cuda"
THR = 0.5
SHAPES = [(1, 1, 1, 4, 4), (2, 3, 9, 32, 32), (3, 2, 17, 5, 7), (3, 2, 17, 24, 40), (8, 1, 2, 8, 8),
          (2, 2, 16, 64, 64), (2, 1, 16, 96, 96)]
EXACT = ("mean_hm", "ens_raw", "ens_preds", "ens_score", "member_score", "select")


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _cs(N, H, W):
    rs = np.random.RandomState(N * 131 + W)
    center = torch.from_numpy(rs.uniform(0.3, 0.7, (N, 2)) * np.array([4.0 * W, 4.0 * H])).float()
    scale = torch.from_numpy(rs.uniform(0.8, 1.6, N) * 4.0 * max(H, W) / 200.0).float()
    return center, scale


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(members' maps, center, scale, restatement) of one shape, computed once and only read."""
    M, N, K, H, W = shape
    p = member_maps(M, N, K, H, W, seed=1)
    center, scale = _cs(N, H, W)
    return p, center, scale, restate_pseudo(p, THR, center, scale)


def _thr(v):
    return torch.full((1,), v, device=DEV, dtype=torch.float32)


def _run(p, center, scale, thr, strided=False):
    """The kernel on p [M,N,K,H,W]; strided: the members as the last stacks of one
    [M,N,2,K,H,W] tensor, through the two strides and a base offset."""
    from ubpl_amd import kernels as Kn
    from ubpl_amd.process import inverse_transforms
    M, N, K, H, W = p.shape
    tinv = inverse_transforms(center, scale, [H, W]).to(DEV)
    if strided:
        S = 2
        big = torch.full((M, N, S, K, H, W), 7.0)               # the other stack would win every argmax
        big[:, :, -1] = p
        sb = S * K * H * W
        sm, hm = N * sb, big.to(DEV).reshape(-1)[(S - 1) * K * H * W:]
    else:
        sb = K * H * W
        sm, hm = N * sb, p.to(DEV).contiguous()
    out = Kn.ensemble_pseudo(hm, sm, sb, M, N, K, H, W, thr, tinv, want_mean=True)
    torch.cuda.synchronize()
    names = ("ens_raw", "ens_preds", "ens_score", "member_score", "disagree", "select", "mean_hm")
    return {n: t.cpu() for n, t in zip(names, out)}


def _same(got, want, nan=False):
    for name in EXACT:
        assert got[name].shape == want[name].shape, name
        assert np.array_equal(got[name].numpy(), want[name].numpy(), equal_nan=nan), name
    g, w = got["disagree"].double().numpy(), want["disagree"].numpy()
    ok = np.abs(g - w) <= 1e-4 * np.abs(w)
    if nan:
        ok |= np.isnan(g) & np.isnan(w)
    assert ok.all(), ("disagree", float(np.nanmax(np.abs(g - w) / np.maximum(np.abs(w), 1e-300))))


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_ensemble_pseudo_matches_the_restatement(shape, strided):
    p, center, scale, want = _case(shape)
    thr = _thr(THR)
    got = _run(p, center, scale, thr, strided)
    _same(got, want)
    again = _run(p, center, scale, thr, strided)
    assert np.array_equal(got["disagree"].numpy(), again["disagree"].numpy())    # a fixed summation order
    if shape[0] == 1:
        assert float(got["disagree"].abs().max()) == 0.0
        assert np.array_equal(got["mean_hm"].numpy(), p[0].numpy())
    if shape[1] * shape[2] >= 6:
        assert set(got["select"].reshape(-1).tolist()) == {0.0, 1.0}             # the maps straddle thr


@pytest.mark.parametrize("M", [2, 3])
def test_ensemble_pseudo_edge_maps(M):
    """Peaks exactly at thr (>= selects), an ensemble maximum <= 0 (zeros, not selected), a NaN in
    one member (the ensemble score is NaN and nothing selects) and a tie in T (the smaller flat
    index wins)."""
    N, K, H, W = 2, 5, 6, 7
    gen = torch.Generator().manual_seed(31 + M)
    p = torch.rand(M, N, K, H, W, generator=gen) * 0.25
    p[:, 0, 0, 2, 3] = 0.5                                        # T's peak: exactly 0.5 for M = 2, 3
    p[:, 0, 1] = -torch.rand(M, H, W, generator=gen)              # maximum < 0
    p[:, 1, 1] = 0.0                                              # maximum == 0
    p[:, 0, 2, 4, 4] = 0.9
    p[M - 1, 0, 2, 5, 0] = float("nan")
    p[:, 0, 3, 4, 5] = 0.8                                        # two equal maxima of T
    p[:, 0, 3, 1, 6] = 0.8
    center, scale = _cs(N, H, W)
    want = restate_pseudo(p, THR, center, scale)
    assert float(want["ens_score"][0, 0]) == 0.5 and want["select"][:, 0, 0].tolist() == [1.0] * M
    assert want["ens_raw"][0, 1].tolist() == [0, 0] and want["ens_raw"][1, 1].tolist() == [0, 0]
    assert want["select"][:, 0, 1].tolist() == [0.0] * M and want["select"][:, 1, 1].tolist() == [0.0] * M
    assert torch.isnan(want["ens_score"][0, 2]) and want["select"][:, 0, 2].tolist() == [0.0] * M
    assert want["ens_raw"][0, 3].tolist() == [7, 2] and want["select"][:, 0, 3].tolist() == [1.0] * M
    for strided in (False, True):
        got = _run(p, center, scale, _thr(THR), strided)
        _same(got, want, nan=True)
        assert torch.isnan(got["ens_score"][0, 2]) and torch.isnan(got["member_score"][M - 1, 0, 2])
        assert got["select"][:, 0, 0].tolist() == [1.0] * M


def test_member_count_is_checked():
    from ubpl_amd import _lib, kernels as Kn
    N, K, H, W = 1, 2, 4, 4
    hm = torch.zeros(9, N, K, H, W, device=DEV)
    for M in (0, 9):
        with pytest.raises(ValueError, match="1 to 8 members"):
            Kn.ensemble_pseudo(hm, N * K * H * W, K * H * W, M, N, K, H, W, _thr(THR))
        sel = torch.zeros(9 * N * K, device=DEV)
        with pytest.raises(RuntimeError, match="hipError"):     # the C entry's own guard
            _lib.op("ubpl_ensemble_pseudo")(hm, N * K * H * W, K * H * W, M, N, K, H, W, None, _thr(THR), None, None,
                                            None, None, None, None, sel)
    with pytest.raises(ValueError, match="hm holds"):
        Kn.ensemble_pseudo(hm.reshape(-1)[1:], N * K * H * W, K * H * W, 9 - 1, N + 1, K, H, W, _thr(THR))
    with pytest.raises(RuntimeError, match="hipError"):         # select is not nullable
        _lib.op("ubpl_ensemble_pseudo")(hm, N * K * H * W, K * H * W, 2, N, K, H, W, None, _thr(THR), None, None,
                                        None, None, None, None, None)
    torch.cuda.synchronize()


def test_nullable_outputs_and_the_device_threshold():
    from ubpl_amd import kernels as Kn
    shape = (3, 2, 17, 24, 40)
    p, center, scale, want = _case(shape)
    M, N, K, H, W = shape
    hm = p.to(DEV)
    thr = _thr(THR)
    sel = torch.full((M, N, K), -1.0, device=DEV)
    out = Kn.ensemble_pseudo(hm, N * K * H * W, K * H * W, M, N, K, H, W, thr, out=(None,) * 5 + (sel, None))
    assert out[:5] == (None,) * 5 and out[6] is None
    assert np.array_equal(sel.cpu().numpy(), want["select"].numpy())
    raw, dis = torch.zeros(N, K, 2, device=DEV), torch.zeros(M, N, K, device=DEV)
    Kn.ensemble_pseudo(hm, N * K * H * W, K * H * W, M, N, K, H, W, thr, out=(raw, None, None, None, dis, sel, None))
    assert np.array_equal(raw.cpu().numpy(), want["ens_raw"].numpy())
    # the threshold is read on the device: the same call, another value in thr
    args = (hm, N * K * H * W, K * H * W, M, N, K, H, W, thr)
    for v in (0.75, 2.0, -1.0, THR):
        thr.fill_(v)
        got = Kn.ensemble_pseudo(*args)[5].cpu()
        w = restate_pseudo(p, v)["select"]
        assert np.array_equal(got.numpy(), w.numpy()), v
        assert float(w.sum()) == {2.0: 0.0, -1.0: float(M * N * K)}.get(v, float(w.sum()))
