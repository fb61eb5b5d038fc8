"""ubpl_warp_views and ubpl_decode_heatmaps_views against their numpy restatement
(tests/tta_ref.py) in float32, bit for bit, and against the decode family they extend."""
import math

import numpy as np
import pytest
import torch

import tta_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (N, K, H, W), V: one pixel row per thread slice; three small views; non-square, W not dividing
# 64 or 256, K odd; the project's heatmap size with ten views; 96x96 (36 pixels per thread)
CASES = [((1, 1, 4, 4), 1), ((1, 1, 4, 4), 2), ((2, 3, 8, 8), 3), ((2, 17, 24, 40), 5), ((2, 16, 64, 64), 10),
         ((1, 16, 96, 96), 4)]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mats(V, H, W, swap, rs):
    """View 0 the identity; the others rotate and zoom about the plane's centre and shift by a
    fraction of a pixel; with swap every second view is mirrored and carries the flag."""
    from ubpl_amd import kernels as Kn
    rows = [list(TR.IDENTITY)]
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    for v in range(1, V):
        a, z = math.radians(rs.uniform(-40, 40)), rs.uniform(0.7, 1.4)
        co, si = math.cos(a) * z, math.sin(a) * z
        tx, ty = rs.uniform(-0.7, 0.7, 2)
        rows.append([co, si, cx - co * cx - si * cy + tx, -si, co, cy + si * cx - co * cy + ty])
    m = torch.tensor(rows, dtype=torch.float64)
    flags = [0] * V
    if swap:
        for v in range(1, V, 2):
            m[v] = Kn.compose_pixels(Kn.mirror_pixels(W), m[v])[0]
            flags[v] = 1
    return m.to(torch.float32), torch.tensor(flags, dtype=torch.int32)


def _maps(V, N, K, H, W, rs):
    hm = (rs.standard_normal((V, N, K, H, W)) * 0.1).astype(np.float32)
    for v in range(V):                                              # a peak somewhere in every map
        for n in range(N):
            for k in range(K):
                hm[v, n, k, rs.randint(H), rs.randint(W)] += rs.uniform(0.5, 1.0)
    return hm


def _place(hm, strided):
    """Host [V,N,K,H,W] -> (device tensor addressed as the kernel takes it, sv, sb).  Strided:
    the last stack of a [V*N,2,K,H,W] tensor whose other stack would win every argmax."""
    V, N, K, H, W = hm.shape
    if not strided:
        return torch.from_numpy(hm).to(DEV).reshape(-1), N * K * H * W, K * H * W
    full = np.full((V * N, 2, K, H, W), 1e3, np.float32)
    full[:, 1] = hm.reshape(V * N, K, H, W)
    sb = 2 * K * H * W
    return torch.from_numpy(full).to(DEV).reshape(-1)[K * H * W:], N * sb, sb


def _tinv(N, rs):
    return torch.from_numpy(rs.uniform(-2, 2, (N, 6)) + np.array([4.0, 0, 0, 0, 4.0, 0])).to(DEV)


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%dx%d-V%d" % (c[0] + (c[1],)))
def test_merge_and_decode_match_the_restatement(case, strided, swap):
    from ubpl_amd import kernels as Kn
    (N, K, H, W), V = case
    rs = np.random.RandomState(V * 100 + H + 2 * strided + swap)
    hm = _maps(V, N, K, H, W, rs)
    mats, flags = _mats(V, H, W, swap, rs)
    perm = rs.permutation(K).astype(np.int32) if swap else None
    dev, sv, sb = _place(hm, strided)
    tinv = _tinv(N, rs)
    args = (dev, sv, sb, V, N, K, H, W, mats.to(DEV), flags.to(DEV) if swap else None,
            torch.from_numpy(perm).to(DEV) if swap else None, tinv)
    raw, preds, scores, merged = Kn.decode_heatmaps_views(*args, want_merged=True)
    want = TR.merge_views(hm, mats.numpy(), flags.numpy() if swap else None, perm)
    assert np.array_equal(_bits(merged.cpu().numpy()), _bits(want))
    r0, p0, s0 = Kn.decode_heatmaps(merged, tinv)
    for a, b in ((raw, r0), (preds, p0), (scores, s0)):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    raw_np, scores_np = TR.decode(want)
    assert np.array_equal(raw.cpu().numpy(), raw_np) and np.array_equal(scores.cpu().numpy(), scores_np)
    # again, and without the merged maps and the transform: equal bits
    again = Kn.decode_heatmaps_views(*args, want_merged=True)
    for a, b in zip(again, (raw, preds, scores, merged)):
        assert torch.equal(a, b)
    lean = Kn.decode_heatmaps_views(*args[:-1])
    assert lean[1] is None and lean[3] is None and torch.equal(lean[0], raw) and torch.equal(lean[2], scores)


@pytest.mark.parametrize("strided", [False, True])
def test_one_identity_view_is_the_plain_decode(strided):
    """V = 1: ubpl_decode_heatmaps_flip(hm, None), a NaN map, an inf and a map whose maximum is
    not positive included."""
    from ubpl_amd import kernels as Kn
    N, K, H, W = 2, 5, 24, 40
    rs = np.random.RandomState(11)
    hm = _maps(1, N, K, H, W, rs)
    hm[0, 0, 1, 3, 7] = np.nan
    hm[0, 0, 2, 5, 5] = np.inf
    hm[0, 1, 0] = -np.abs(hm[0, 1, 0])
    hm[0, 1, 1] = 0.0
    dev, sv, sb = _place(hm, strided)
    tinv = _tinv(N, rs)
    ident = torch.tensor([TR.IDENTITY], dtype=torch.float32, device=DEV)
    got = Kn.decode_heatmaps_views(dev, sv, sb, 1, N, K, H, W, ident, None, None, tinv, want_merged=True)
    want = Kn.decode_heatmaps_flip(dev, None, sb, N, K, H, W, None, tinv, want_merged=True)
    for a, b in zip(got, want):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    assert np.array_equal(_bits(got[3].cpu().numpy()), _bits(hm[0]))
    assert math.isnan(got[2][0, 1].item()) and got[0][1, 0].tolist() == [0.0, 0.0] == got[0][1, 1].tolist()


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 4, 4), (2, 17, 24, 40), (1, 16, 64, 64)])
def test_identity_plus_mirror_is_the_flip_test_decode(shape, pairs):
    from ubpl_amd import kernels as Kn
    N, K, H, W = shape
    rs = np.random.RandomState(K + pairs)
    hm = _maps(2, N, K, H, W, rs)
    dev, sv, sb = _place(hm, True)
    tinv = _tinv(N, rs)
    perm = torch.from_numpy(rs.permutation(K).astype(np.int32)).to(DEV) if pairs else None
    _, hm_mat, swap = Kn.view_matrices([(0, 1)], True, 4 * W, W)
    got = Kn.decode_heatmaps_views(dev, sv, sb, 2, N, K, H, W, hm_mat.to(DEV), swap.to(DEV), perm, tinv,
                                   want_merged=True)
    want = Kn.decode_heatmaps_flip(dev, dev[sv:], sb, N, K, H, W, perm, tinv, want_merged=True)
    for a, b in zip(got, want):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_uncovered_views_and_pixels():
    from ubpl_amd import kernels as Kn
    N, K, H, W = 2, 3, 8, 8
    rs = np.random.RandomState(5)
    hm = _maps(3, N, K, H, W, rs)
    mats, _ = _mats(3, H, W, False, rs)
    dev, sv, sb = _place(hm, False)
    run = lambda d, m, V: Kn.decode_heatmaps_views(d, sv, sb, V, N, K, H, W, m.to(DEV), want_merged=True)
    two = run(dev, mats[:2], 2)
    # a third view pushed wholly outside (far, infinite, NaN) contributes nothing
    for t in (1e6, float("inf"), float("nan"), -float(W + 1)):
        out = mats.clone()
        out[2] = torch.tensor([1, 0, t, 0, 1, 0])
        for a, b in zip(run(dev, out, 3), two):
            assert a is b or np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy())), t
    # a pixel covered by no view is 0; one covered in part is averaged over its coverage
    shift = torch.tensor([[1, 0, 2.5, 0, 1, 0]], dtype=torch.float32)
    raw, _, scores, merged = run(dev, shift, 1)
    m = merged.cpu().numpy()
    assert not m[..., W - 2:].any() and np.array_equal(_bits(m), _bits(TR.merge_views(hm[:1], shift.numpy())))
    assert np.allclose(m[..., W - 3], hm[0][..., W - 1], rtol=1e-6)   # 0.5 v / 0.5
    none = run(dev, torch.tensor([[1, 0, 1e6, 0, 1, 0]] * 2, dtype=torch.float32), 2)
    assert not none[3].any() and not none[0].any() and not none[2].any()


@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (1, 3, 24, 40), (2, 3, 128, 128)])
def test_warp_views(shape):
    from ubpl_amd import kernels as Kn
    N, C, H, W = shape
    rs = np.random.RandomState(H)
    src = rs.uniform(-0.5, 0.5, shape).astype(np.float32)
    mats, _ = _mats(4, H, W, True, rs)
    x = torch.from_numpy(src).to(DEV)
    got = Kn.warp_views(x, mats.to(DEV))
    assert got.shape == (4, N, C, H, W)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(TR.warp_views(src, mats.numpy())))
    assert torch.equal(got[0], x)                                   # the identity view is a copy
    # into the rows of a view-major batch, as Predictor does
    batch = torch.zeros(4 * N, C, H, W, device=DEV)
    batch[:N] = x
    Kn.warp_views(batch[:N], mats[1:].to(DEV), out=batch[N:])
    assert torch.equal(batch.reshape(4, N, C, H, W), got)
    with pytest.raises(ValueError, match="does not overlap"):
        Kn.warp_views(batch[:N], mats[:1].to(DEV), out=batch[:N])
    with pytest.raises(ValueError, match="3 views of"):
        Kn.warp_views(batch[:N], mats[1:].to(DEV), out=batch[2 * N:])


def test_argument_errors():
    from ubpl_amd import _lib
    from ubpl_amd import kernels as Kn
    V, N, K, H, W = 2, 1, 2, 6, 7
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    a = {"hm": z(17 * N * K * H * W), "sv": N * K * H * W, "sb": K * H * W, "V": V, "N": N, "K": K, "H": H, "W": W,
         "mat": z(17 * 6), "swap": None, "perm": None, "tinv": z(N * 6, dt=torch.float64),
         "merged": z(N * K * H * W), "raw": z(N * K * 2), "preds": z(N * K * 2), "scores": z(N * K)}
    call = lambda **kw: _lib.call("ubpl_decode_heatmaps_views", *[kw.get(n, v) for n, v in a.items()])
    call()
    call(V=16)
    for bad in ({"V": 0}, {"V": 17}, {"tinv": None}, {"K": 0}, {"sv": K * H * W - 1}, {"mat": None}):
        with pytest.raises(RuntimeError, match="failed with hipError 1"):
            call(**bad)
    call(N=0)                                                      # no maps: nothing to do
    with pytest.raises(RuntimeError, match="hm holds"):            # the op's extent check
        call(hm=a["hm"][:V * N * K * H * W - 1])
    for V_ in (0, 17):
        with pytest.raises(ValueError, match="1 to 16 views"):
            Kn.decode_heatmaps_views(a["hm"], a["sv"], a["sb"], V_, N, K, H, W, a["mat"])
    with pytest.raises(ValueError, match="swap has 3 entries"):
        Kn.decode_heatmaps_views(a["hm"], a["sv"], a["sb"], V, N, K, H, W, a["mat"][:12],
                                 z(3, dt=torch.int32))
    torch.cuda.synchronize()
