"""The inference kernels against torch CPU restatements, bit for bit:
ubpl_decode_heatmaps_flip (flip-back + pair swap + average + decode in one read),
ubpl_fliplr and ubpl_bn_eval_coeffs_table."""
import numpy as np
import pytest
import torch

from oracle import decode as OD

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 1, 4, 4), (3, 9, 32, 32), (2, 17, 24, 40), (2, 16, 64, 64), (1, 16, 96, 96)]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _pairs(K):
    """(0,1), (2,3), ... — the last joint of an odd K stays unpaired."""
    return [(i, i + 1) for i in range(0, K - 1, 2)]


def _perm(K, swap):
    from ubpl_amd import kernels as Kn
    return Kn.flip_perm(K, _pairs(K)) if swap else None


def _restate(hm, hm_flip, perm, center, scale):
    """merged, raw, preds, scores as the reference computes them on the host."""
    if hm_flip is None:
        merged = hm
    else:
        back = torch.flip(hm_flip, [-1])
        if perm is not None:
            back = back[:, perm.long()]
        merged = (hm + back) * 0.5
    H, W = hm.shape[2:]
    raw = OD.get_preds(merged)
    preds, scores = OD.kps_from_heatmap(merged, center, scale, [H, W])
    return merged, raw, preds, scores


def _cs(N, H, W):
    rs = np.random.RandomState(N * 131 + W)
    center = torch.from_numpy(rs.uniform(0.3, 0.7, (N, 2)) * np.array([4.0 * W, 4.0 * H])).float()
    scale = torch.from_numpy(rs.uniform(0.8, 1.6, N) * 4.0 * max(H, W) / 200.0).float()
    return center, scale


def _run(hm, hm_flip, perm, center, scale, strided=False):
    """The kernel on hm / hm_flip [N,K,H,W]; strided: both passed as the last-stack rows of
    one [2N,2,K,H,W] tensor through the stride and base offset."""
    from ubpl_amd import kernels as Kn
    from ubpl_amd.process import inverse_transforms
    N, K, H, W = hm.shape
    tinv = inverse_transforms(center, scale, [H, W]).to(DEV)
    pd = None if perm is None else perm.to(DEV)
    if strided:
        S = 2
        big = torch.full((2 * N, S, K, H, W), 7.0)       # the other stack would win every argmax
        big[:N, -1] = hm
        big[N:, -1] = hm_flip
        flat = big.to(DEV).reshape(-1)
        sb, last = S * K * H * W, (S - 1) * K * H * W
        a, b = flat[last:], flat[N * sb + last:]
    else:
        sb = K * H * W
        a = hm.to(DEV).contiguous()
        b = None if hm_flip is None else hm_flip.to(DEV).contiguous()
    raw, preds, scores, merged = Kn.decode_heatmaps_flip(a, b, sb, N, K, H, W, pd, tinv, want_merged=True)
    torch.cuda.synchronize()
    return merged.cpu(), raw.cpu(), preds.cpu(), scores.cpu()


def _same(got, want, nan=False):
    for g, w, name in zip(got, want, ("merged", "raw", "preds", "scores")):
        assert g.shape == w.shape, name
        assert np.array_equal(g.numpy(), w.numpy(), equal_nan=nan), name


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_decode_flip_bit_exact(shape, strided, swap):
    N, K, H, W = shape
    gen = torch.Generator().manual_seed(N * 1000 + K * 10 + W)
    hm = torch.randn(N, K, H, W, generator=gen)
    hf = torch.randn(N, K, H, W, generator=gen)
    perm = _perm(K, swap)
    center, scale = _cs(N, H, W)
    _same(_run(hm, hf, perm, center, scale, strided), _restate(hm, hf, perm, center, scale))


@pytest.mark.parametrize("shape", SHAPES)
def test_decode_flip_edge_maps(shape):
    """A symmetric tie (the smaller flat index wins), a map whose merged maximum is <= 0
    (zeros), and a NaN in one input (ranks above every number)."""
    N, K, H, W = shape
    gen = torch.Generator().manual_seed(77 + W)
    hm = torch.randn(N, K, H, W, generator=gen).clamp_(-2, 2)
    hf = torch.randn(N, K, H, W, generator=gen).clamp_(-2, 2)
    y, x = H // 2, W // 4
    # equal peaks at (y, x) of hm and (y, x) of hm_flip -> equal maxima of merged at x and W-1-x
    hm[0, 0] = -1.0
    hf[0, 0] = -1.0
    hm[0, 0, y, x] = 5.0
    hf[0, 0, y, x] = 5.0
    center, scale = _cs(N, H, W)
    want = _restate(hm, hf, None, center, scale)
    m = want[0][0, 0]
    assert m[y, x] == m[y, W - 1 - x] == 2.0 and (m <= 2.0).all()
    assert want[1][0, 0].tolist() == [min(x, W - 1 - x) + 1, y + 1]
    _same(_run(hm, hf, None, center, scale), want)
    if K > 2:
        hm[0, 1] = -torch.rand(H, W, generator=gen)          # merged maximum < 0
        hf[0, 1] = -torch.rand(H, W, generator=gen)
        hm[0, 2] = 0.0                                       # merged maximum == 0
        hf[0, 2] = 0.0
        want = _restate(hm, hf, None, center, scale)
        assert want[1][0, 1].tolist() == [0, 0] and want[1][0, 2].tolist() == [0, 0]
        _same(_run(hm, hf, None, center, scale), want)
    hf[0, 0, H - 1, 0] = float("nan")                        # lands at (H-1, W-1) of merged
    want = _restate(hm, hf, None, center, scale)
    assert torch.isnan(want[3][0, 0])
    _same(_run(hm, hf, None, center, scale), want, nan=True)
    _same(_run(hm, hf, None, center, scale, strided=True), want, nan=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_decode_without_flip_is_the_plain_decode(shape):
    from ubpl_amd import kernels as Kn
    from ubpl_amd.process import inverse_transforms
    N, K, H, W = shape
    S = 2
    o = torch.randn(N, S, K, H, W, generator=torch.Generator().manual_seed(5 + W)).to(DEV)
    center, scale = _cs(N, H, W)
    tinv = inverse_transforms(center, scale, [H, W]).to(DEV)
    last = o[:, -1].contiguous()
    raw0, preds0, scores0 = Kn.decode_heatmaps(last, tinv)
    raw, preds, scores, merged = Kn.decode_heatmaps_flip(o.reshape(-1)[(S - 1) * K * H * W:], None, S * K * H * W, N,
                                                         K, H, W, None, tinv, want_merged=True)
    for a, b in ((raw, raw0), (preds, preds0), (scores, scores0), (merged, last)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    # nullable outputs: nothing but raw
    out = (torch.zeros(N, K, 2, device=DEV), None, None, None)
    Kn.decode_heatmaps_flip(last, None, K * H * W, N, K, H, W, out=out)
    assert np.array_equal(out[0].cpu().numpy(), raw0.cpu().numpy())


@pytest.mark.parametrize("W", [1, 3, 32, 40, 256])
def test_fliplr(W):
    from ubpl_amd import kernels as Kn
    x = torch.randn(5, 3, 7, W, generator=torch.Generator().manual_seed(W))
    y = Kn.fliplr(x.to(DEV))
    assert np.array_equal(y.cpu().numpy(), torch.flip(x, [-1]).numpy())
    # a 4-byte-aligned view (no 16-byte alignment): the scalar path
    buf = torch.zeros(x.numel() + 1)
    buf[1:] = x.reshape(-1)
    xd = buf.to(DEV)[1:].view(x.shape)
    out = torch.zeros(x.numel() + 1, device=DEV)[1:].view(x.shape)
    Kn.fliplr(xd, out=out)
    assert np.array_equal(out.cpu().numpy(), torch.flip(x, [-1]).numpy())


def test_bn_eval_coeffs_table_matches_per_bn():
    from ubpl_amd import kernels as Kn
    Cs = [1, 64, 100, 256, 512, 64]
    gen = torch.Generator().manual_seed(3)
    params = torch.randn(2 * sum(Cs) + 8, generator=gen)
    stats = torch.randn(2 * sum(Cs) + 8, generator=gen)
    rows, po, so, co = [], 3, 5, 0
    for c in Cs:
        rows.append((po, po + c, so, so + c, co, c))
        stats[so + c:so + 2 * c] = torch.rand(c, generator=gen) * 4 + 1e-3     # positive variance
        po, so, co = po + 2 * c, so + 2 * c, co + 4 * c
    pd, sd = params.to(DEV), stats.to(DEV)
    coef = torch.full((co,), -7.0, device=DEV)
    Kn.bn_eval_coeffs_table(pd, sd, Kn.bn_coeff_table(rows, params.numel(), stats.numel(), co).to(DEV), 1e-5, coef)
    for g, b, rm, rv, o, c in rows:
        sc, sh = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        Kn.bn_eval_coeffs(pd[g:g + c], pd[b:b + c], sd[rm:rm + c], sd[rv:rv + c], 1e-5, sc, sh)
        assert np.array_equal(coef[o:o + c].cpu().numpy(), sc.cpu().numpy()), c
        assert np.array_equal(coef[o + c:o + 2 * c].cpu().numpy(), sh.cpu().numpy()), c
        assert (coef[o + 2 * c:o + 4 * c] == -7.0).all()                       # mean | invstd untouched
