"""ubpl_merge_views_samples against its numpy restatement (tests/cross_view_ref.py) in float32,
bit for bit, and against ubpl_decode_heatmaps_views, the merge it extends."""
import math

import numpy as np
import pytest
import torch

import cross_view_ref as CR
import tta_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (V, M, N, K, H, W): non-square, 276 pixels (two 256-pixel tiles, the second in part), K not a
# multiple of the kernel's eight planes; the workload's plane with three views; K = 9, one plane into
# the second group of eight, in columns of one cell (the kernel's path without paired taps)
CASES = [(2, 2, 3, 3, 12, 23), (3, 1, 2, 2, 64, 64), (2, 1, 2, 9, 5, 1)]


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _mats(V, N, H, W, rs):
    """[V,V,N,6]: per (pair, sample) a rotation of +-30 degrees and a zoom of 0.75 to 1.25 about the
    plane's centre with a sub-cell shift, every second one mirrored; then the special entries: one
    off-diagonal identity, one translation that puts everything outside, one matrix with a NaN and
    one half-cell translation (fractional cover at the border).  The diagonal is filled with NaN:
    the kernel never reads it."""
    from ubpl_amd import kernels as Kn
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    m = torch.empty((V, V, N, 6), dtype=torch.float64)
    i = 0
    for a in range(V):
        for v in range(V):
            for n in range(N):
                ang, z = math.radians(rs.uniform(-30, 30)), rs.uniform(0.75, 1.25)
                co, si = math.cos(ang) * z, math.sin(ang) * z
                tx, ty = rs.uniform(-0.7, 0.7, 2)
                row = torch.tensor([[co, si, cx - co * cx - si * cy + tx, -si, co, cy + si * cx - co * cy + ty]],
                                   dtype=torch.float64)
                if i % 2:
                    row = Kn.compose_pixels(Kn.mirror_pixels(W), row)
                m[a, v, n] = row[0]
                i += 1
    m = m.to(torch.float32)
    m[0, 1, 0] = torch.tensor(TR.IDENTITY)
    m[1, 0, 0] = torch.tensor([1, 0, 10.0 * W, 0, 1, 0])
    m[0, 1, 1] = torch.tensor([1, 0, float("nan"), 0, 1, 0])
    m[1, 0, 1] = torch.tensor([1, 0, 0.5, 0, 1, -0.5])
    for a in range(V):
        m[a, a] = float("nan")
    return m


def _maps(shape, rs):
    hm = (rs.standard_normal(shape) * 0.1).astype(np.float32)
    flat = hm.reshape(-1, shape[-2] * shape[-1])
    flat[np.arange(len(flat)), rs.randint(flat.shape[1], size=len(flat))] += rs.uniform(0.5, 1.0, len(flat))
    return hm


def _place(hm, strided):
    """Host [V,M,N,K,H,W] -> (device tensor addressed as the kernel takes it, sv, sm, sb).  Strided:
    the last stack of a [V,M,N,2,K,H,W] buffer whose other stack is 1e3 everywhere."""
    V, M, N, K, H, W = hm.shape
    blk = K * H * W
    if not strided:
        return torch.from_numpy(hm).to(DEV).reshape(-1), M * N * blk, N * blk, blk
    full = np.full((V, M, N, 2, K, H, W), 1e3, np.float32)
    full[:, :, :, 1] = hm
    return torch.from_numpy(full).to(DEV).reshape(-1)[blk:], M * N * 2 * blk, N * 2 * blk, 2 * blk


_CASE = {}


def _case(shape):
    """(hm, mats, {include_self: (out, cover)}) of a case: made and restated once."""
    if shape not in _CASE:
        V, M, N, K, H, W = shape
        rs = np.random.RandomState(H + W)
        hm, mats = _maps(shape, rs), _mats(V, N, H, W, rs)
        _CASE[shape] = (hm, mats, {s: CR.merge_views_samples(hm, mats.numpy(), s) for s in (True, False)})
    return _CASE[shape]


@pytest.mark.parametrize("include_self", [True, False])
@pytest.mark.parametrize("shape,strided", [(CASES[0], False), (CASES[0], True), (CASES[1], False), (CASES[2], False)],
                         ids=["12x23", "12x23-strided", "64x64-V3", "5x1-K9"])
def test_merge_matches_the_restatement(shape, strided, include_self):
    from ubpl_amd import kernels as Kn
    V, M, N, K, H, W = shape
    hm, mats, want = _case(shape)
    dev, sv, sm, sb = _place(hm, strided)
    out, cover = Kn.merge_views_samples(dev, sv, sm, sb, V, M, N, K, H, W, mats.to(DEV), include_self,
                                        want_cover=True)
    ref_out, ref_cover = want[include_self]
    assert out.shape == (V, M, N, K, H, W) and cover.shape == (V, N, H, W)
    assert np.array_equal(_bits(cover), _bits(ref_cover))
    assert np.array_equal(_bits(out), _bits(ref_out))
    assert np.isfinite(ref_out).all()
    if V == 2:                                                        # the special matrices did what they are there for
        c, own = ref_cover, 1 if include_self else 0
        assert (c[0, 0] == own + 1).all()                             # the off-diagonal identity: the whole plane
        assert (c[1, 0] == own).all() and (c[0, 1] == own).all()      # far outside, and the NaN: nothing
        if include_self:
            assert np.array_equal(_bits(out[1, :, 0]), _bits(hm[1, :, 0]))
        else:
            assert np.array_equal(_bits(out[0, :, 0]), _bits(hm[1, :, 0]))
            assert not ref_out[1, :, 0].any()                         # no view covers: 0
        other = c[1, 1] - own                                         # the half-cell shift: 0.5 along two borders
        assert (other[1:, :-1] == 1).all() and (other[0, :-1] == 0.5).all() and other[0, -1] == 0.25
    # without cover, and into given tensors
    again, none = Kn.merge_views_samples(dev, sv, sm, sb, V, M, N, K, H, W, mats.to(DEV), include_self)
    assert none is None and torch.equal(again, out)


def test_one_view_is_the_input():
    from ubpl_amd import kernels as Kn
    M, N, K, H, W = 2, 2, 5, 9, 31
    rs = np.random.RandomState(1)
    hm = _maps((1, M, N, K, H, W), rs)
    hm[0, 0, 0, 0, 0, :3] = [np.inf, -np.inf, -0.0]
    dev, sv, sm, sb = _place(hm, False)
    mat = torch.full((1, 1, N, 6), float("nan"), device=DEV)
    out, cover = Kn.merge_views_samples(dev, sv, sm, sb, 1, M, N, K, H, W, mat, want_cover=True)
    # (x / 1.0f is x: the sign of a zero and an infinity survive)
    assert np.array_equal(_bits(out), _bits(hm)) and (cover == 1).all()


def test_two_identity_views_are_the_flip_merge():
    from ubpl_amd import kernels as Kn
    M, N, K, H, W = 1, 2, 3, 16, 20
    hm = _maps((2, M, N, K, H, W), np.random.RandomState(2))
    dev, sv, sm, sb = _place(hm, False)
    mat = torch.tensor(TR.IDENTITY, device=DEV).repeat(2, 2, N, 1)
    out, cover = Kn.merge_views_samples(dev, sv, sm, sb, 2, M, N, K, H, W, mat, want_cover=True)
    want = (hm[0] + hm[1]) * np.float32(0.5)
    assert np.array_equal(_bits(out[0]), _bits(want)) and np.array_equal(_bits(out[1]), _bits(want))
    assert (cover == 2).all()


def test_shared_matrices_give_the_shipped_kernels_merge():
    """Matrices shared by all samples, target view 0 the original frame: out[0] is
    ubpl_decode_heatmaps_views' merged maps."""
    from ubpl_amd import kernels as Kn
    V, N, K, H, W = 3, 2, 3, 24, 40
    rs = np.random.RandomState(3)
    hm = _maps((V, 1, N, K, H, W), rs)
    dev, sv, sm, sb = _place(hm, False)
    per_view = _mats(V, 2, H, W, rs)[2, :, 0]                          # target 2's row [V,6]: two views, the diagonal
    per_view = torch.stack([torch.tensor(TR.IDENTITY), per_view[0], per_view[1]])
    mats = torch.full((V, V, N, 6), float("nan"))
    mats[0] = per_view[:, None].expand(V, N, 6)
    out, _ = Kn.merge_views_samples(dev, sv, sm, sb, V, 1, N, K, H, W, mats.to(DEV))
    merged = Kn.decode_heatmaps_views(dev, sv, sb, V, N, K, H, W, per_view.to(DEV), want_merged=True)[3]
    assert np.array_equal(_bits(out[0, 0]), _bits(merged))


def test_writes_stay_in_bounds_and_repeat():
    from ubpl_amd import kernels as Kn
    shape = CASES[0]
    V, M, N, K, H, W = shape
    hm, mats, want = _case(shape)
    dev, sv, sm, sb = _place(hm, False)
    pad, n_out, n_cov = 1024, hm.size, V * N * H * W
    runs = []
    for _ in range(2):
        obuf = torch.full((n_out + 2 * pad,), -7.0, device=DEV)
        cbuf = torch.full((n_cov + 2 * pad,), -7.0, device=DEV)
        Kn.merge_views_samples(dev, sv, sm, sb, V, M, N, K, H, W, mats.to(DEV), True,
                               out=(obuf[pad:pad + n_out], cbuf[pad:pad + n_cov]))
        for buf, n in ((obuf, n_out), (cbuf, n_cov)):
            assert (buf[:pad] == -7.0).all() and (buf[pad + n:] == -7.0).all()
        runs.append((obuf, cbuf))
    assert np.array_equal(_bits(runs[0][0][pad:pad + n_out]), _bits(want[True][0].reshape(-1)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])   # equal bits


def test_argument_errors():
    from ubpl_amd import _lib
    from ubpl_amd import kernels as Kn
    V, M, N, K, H, W = 2, 2, 2, 2, 6, 7
    blk = K * H * W
    z = lambda n: torch.zeros(n, device=DEV)
    a = {"hm": z(17 * 9 * N * blk), "sv": 9 * N * blk, "sm": N * blk, "sb": blk, "V": V, "M": M, "N": N, "K": K,
         "H": H, "W": W, "mat": z(17 * 17 * N * 6), "include_self": 1, "out": z(17 * 9 * N * blk),
         "cover": z(17 * N * H * W)}
    call = lambda **kw: _lib.call("ubpl_merge_views_samples", *[kw.get(n, v) for n, v in a.items()])
    call()
    call(V=16, M=8)
    call(N=0)                                                          # no maps: nothing to do
    call(cover=None)
    for bad in ({"V": 17}, {"V": 0}, {"M": 9}, {"M": 0}, {"V": 1, "include_self": 0}, {"sb": -blk}, {"sm": -1},
                {"sb": blk - 1}, {"sm": blk - 1}, {"sv": blk - 1}, {"K": 0}, {"out": None}):
        with pytest.raises(RuntimeError, match="failed with hipError 1"):
            call(**bad)
    hm, mat = a["hm"], z(V * V * N * 6)
    good = (9 * N * blk, N * blk, blk, V, M, N, K, H, W)
    Kn.merge_views_samples(hm, *good, mat)
    for V_ in (0, 17):
        with pytest.raises(ValueError, match="1 to 16 views"):
            Kn.merge_views_samples(hm, 9 * N * blk, N * blk, blk, V_, M, N, K, H, W, mat)
    with pytest.raises(ValueError, match="1 to 8 members"):
        Kn.merge_views_samples(hm, 9 * N * blk, N * blk, blk, V, 9, N, K, H, W, mat)
    with pytest.raises(ValueError, match="at least 2 views"):
        Kn.merge_views_samples(hm, 9 * N * blk, N * blk, blk, 1, M, N, K, H, W, z(N * 6), include_self=False)
    with pytest.raises(ValueError, match="hm holds"):                  # a negative stride
        Kn.merge_views_samples(hm[blk:], 9 * N * blk, N * blk, -blk, V, M, N, K, H, W, mat)
    with pytest.raises(ValueError, match="at least one block"):        # a stride below K*H*W
        Kn.merge_views_samples(hm, 9 * N * blk, N * blk, blk - 1, V, M, N, K, H, W, mat)
    with pytest.raises(ValueError, match="hm holds"):                  # too few floats
        Kn.merge_views_samples(hm[:blk], *good, mat)
    with pytest.raises(ValueError, match=r"mat is \[V,V,N,6\]"):
        Kn.merge_views_samples(hm, *good, z(V * N * 6))
    with pytest.raises(ValueError, match="do not overlap"):
        Kn.merge_views_samples(hm, *good, mat, out=(hm[blk:blk + V * M * N * blk], None))
    with pytest.raises(ValueError, match="do not overlap"):
        Kn.merge_views_samples(hm, *good, mat, out=(a["out"][:V * M * N * blk], hm[:V * N * H * W]))
    with pytest.raises(ValueError, match="out holds"):
        Kn.merge_views_samples(hm, *good, mat, out=(a["out"][:7], None))
    torch.cuda.synchronize()
