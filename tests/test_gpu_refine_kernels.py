"""ubpl_refine_peaks against its numpy restatement (tests/refine_ref.py): quarter mode bit for
bit with the float32 instance, Taylor mode against the float64 instance within ten times the
float32 instance's own deviation from it."""
import math

import numpy as np
import pytest
import torch

import refine_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (N, K, H, W): the smallest map with a Taylor-eligible cell; nine maps (a tail block with two
# idle waves); two odd shapes; the two heatmap sizes of the project
SHAPES = [(1, 1, 5, 5), (3, 3, 6, 7), (2, 5, 12, 20), (2, 4, 16, 16), (1, 2, 64, 64), (1, 2, 96, 96)]
RADII = (0, 3, 5)
SIGMA_OF_RADIUS = {0: 0.0, 3: 1.0, 5: 2.0}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib
    _lib.load()


def _blobs(N, K, H, W, rs):
    """Per map a Gaussian blob of random width 1 to 3 cells at a random real-valued centre
    anywhere in the map, borders included, on a constant floor from [0.02, 0.1]."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((N, K, H, W), np.float32)
    for n in range(N):
        for k in range(K):
            cx, cy = rs.uniform(-0.5, W - 0.5), rs.uniform(-0.5, H - 0.5)
            s = rs.uniform(1.0, 3.0)
            out[n, k] = rs.uniform(0.5, 1.0) * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s)) \
                + rs.uniform(0.02, 0.1)
    return out


def _case(shape, strided, flip, seed):
    """The maps of one case -> (hm, hm_flip, sb, perm as device tensors addressed as the kernel
    takes them; hm, hm_flip, perm as host arrays [N,K,H,W] for the restatement)."""
    N, K, H, W = shape
    rs = np.random.RandomState(seed)
    T = _blobs(N, K, H, W, rs)
    perm = np.arange(K)[::-1].copy() if flip else None               # non-trivial for K >= 2
    a, f = T, None
    if flip:
        d = rs.uniform(-0.01, 0.01, T.shape).astype(np.float32)
        a = T + d
        f = np.empty_like(T)
        f[:, perm] = (T - d)[..., ::-1]                              # so that f[:, perm] mirrored = T - d
    S = 2 if strided else 1
    sb, last = S * K * H * W, (S - 1) * K * H * W

    def place(m):
        if m is None:
            return None
        buf = torch.full((N, S, K, H, W), 7.0)                       # the other stack: never a peak's value
        buf[:, -1] = torch.from_numpy(m)
        return buf.to(DEV).reshape(-1)[last:]
    return (place(a), place(f), sb, None if perm is None else torch.from_numpy(perm).int().to(DEV)), (a, f, perm)


def _tinv(N, rs):
    """Off-centre, non-unit inverse transforms."""
    t = np.zeros((N, 6))
    t[:, 0] = rs.uniform(3.0, 5.0, N)
    t[:, 4] = rs.uniform(3.0, 5.0, N)
    t[:, 1] = rs.uniform(-0.2, 0.2, N)
    t[:, 3] = rs.uniform(-0.2, 0.2, N)
    t[:, 2] = rs.uniform(-40.0, 40.0, N)
    t[:, 5] = rs.uniform(-40.0, 40.0, N)
    return t


def _refine(dev, shape, raw, mode, taps, tinv):
    from ubpl_amd import kernels as Kn
    hm, hm_flip, sb, perm = dev
    N, K, H, W = shape
    out = Kn.refine_peaks(hm, hm_flip, sb, N, K, H, W, perm, raw, mode, taps.to(DEV), tinv)
    return [None if t is None else t.cpu().numpy() for t in out]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_refine_matches_the_restatement(shape):
    from ubpl_amd import kernels as Kn
    N, K, H, W = shape
    total = left_out = taylor_taken = 0
    for ci, (strided, flip) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        dev, host = _case(shape, strided, flip, seed=100 * ci + H + W)
        tinv = _tinv(N, np.random.RandomState(ci))
        tinv_d = torch.from_numpy(tinv).to(DEV)
        raw_d = Kn.decode_heatmaps_flip(dev[0], dev[1], dev[2], N, K, H, W, dev[3])[0]
        raw = raw_d.cpu().numpy()
        # quarter: bit for bit, the transform included
        want = RR.refine_ref(host[0], raw, RR.QUARTER, np.ones(1, np.float32), np.float32, host[1], host[2], tinv)
        got = _refine(dev, shape, raw_d, "quarter", torch.ones(1), tinv_d)
        assert np.array_equal(got[0], want["raw_sub"]), (strided, flip)
        assert np.array_equal(got[1], want["preds_sub"]), (strided, flip)
        assert np.array_equal(got[2], want["how"]), (strided, flip)
        assert np.abs(got[0] - raw).max() <= 0.25
        for radius in RADII:
            taps = Kn.blur_taps(SIGMA_OF_RADIUS[radius])
            assert taps.numel() == radius + 1
            r64 = RR.refine_ref(host[0], raw, RR.TAYLOR, taps.numpy(), np.float64, host[1], host[2], tinv)
            r32 = RR.refine_ref(host[0], raw, RR.TAYLOR, taps.numpy(), np.float32, host[1], host[2], tinv)
            got = _refine(dev, shape, raw_d, "taylor", taps, tinv_d)
            again = _refine(dev, shape, raw_d, "taylor", taps, tinv_d)
            assert all(np.array_equal(a, b) for a, b in zip(got, again))       # equal bits on a repeated launch
            keep = ~RR.at_boundary(r64)
            total += keep.size
            left_out += int((~keep).sum())
            taylor_taken += int((r64["how"][keep] == 2).sum())
            dev32 = np.abs(r32["raw_sub"].astype(np.float64) - r64["raw_sub"])[keep & (r32["how"] == r64["how"])]
            tol = max(1e-6, 10.0 * (float(dev32.max()) if dev32.size else 0.0))
            err = np.abs(got[0].astype(np.float64) - r64["raw_sub"])[keep]
            print("shape %s strided %d flip %d radius %d: kept %d of %d, f32 restatement dev %.3g, kernel err %.3g, "
                  "tol %.3g" % (shape, strided, flip, radius, keep.sum(), keep.size,
                                dev32.max() if dev32.size else 0.0, err.max() if err.size else 0.0, tol))
            assert np.array_equal(got[2][keep], r64["how"][keep]), (strided, flip, radius)
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
            assert (err <= tol).all(), (strided, flip, radius, float(err.max()), tol)
            assert np.abs(got[0] - raw).max() <= 1.0
            # the transform of what the kernel wrote, bit for bit
            u, v = got[0][..., 0].astype(np.float64) - 1.0, got[0][..., 1].astype(np.float64) - 1.0
            t = tinv.reshape(N, 1, 6)
            px = ((t[..., 0] * u + t[..., 1] * v) + t[..., 2]) + 1.0
            py = ((t[..., 3] * u + t[..., 4] * v) + t[..., 5]) + 1.0
            assert np.array_equal(got[1], np.stack([px, py], -1).astype(np.float32))
    assert left_out <= math.floor(0.02 * total), (left_out, total)
    if min(H, W) >= 12:
        assert taylor_taken > 0                                     # the Taylor branch ran in this case


def _one(v, raws, mode, taps=None, tinv=None):
    """Maps v [K,H,W] (host) with hand-given raw peaks -> the kernel's and the float32
    restatement's (raw_sub, preds_sub, how)."""
    from ubpl_amd import kernels as Kn
    K, H, W = v.shape
    taps = torch.ones(1) if taps is None else taps
    raw = np.array([raws], np.float32)
    t = None if tinv is None else torch.from_numpy(tinv).to(DEV)
    got = Kn.refine_peaks(torch.from_numpy(v[None]).to(DEV), None, K * H * W, 1, K, H, W, None,
                          torch.from_numpy(raw).to(DEV), mode, taps.to(DEV), t)
    want = RR.refine_ref(v[None], raw, RR.TAYLOR if mode == "taylor" else RR.QUARTER, taps.numpy(), np.float32,
                         tinv=tinv)
    return [None if g is None else g.cpu().numpy()[0] for g in got], want


@pytest.mark.parametrize("mode", ["quarter", "taylor"])
def test_no_peak_and_raw_out_of_range(mode):
    from ubpl_amd import kernels as Kn
    H, W = 6, 7
    v = np.zeros((5, H, W), np.float32)
    v[1] = -0.5
    v[2:] = 0.5
    tinv = _tinv(1, np.random.RandomState(3))
    # decoded: all zero and all negative maps give (0, 0)
    raw = Kn.decode_heatmaps(torch.from_numpy(v[None]).to(DEV))[0].cpu().numpy()[0]
    assert raw[:2].tolist() == [[0.0, 0.0], [0.0, 0.0]]
    raws = [tuple(raw[0]), tuple(raw[1]), (W + 1.0, 3.0), (3.0, H + 5.0), (-2.0, 1.0)]
    got, want = _one(v, raws, mode, tinv=tinv)
    assert got[2].tolist() == [0.0] * 5
    assert np.array_equal(got[0], np.array(raws, np.float32))
    assert np.array_equal(got[0], want["raw_sub"][0]) and np.array_equal(got[1], want["preds_sub"][0])
    t = tinv[0]
    assert got[1][0].tolist() == [np.float32((t[0] * -1.0 + t[1] * -1.0) + t[2] + 1.0),
                                  np.float32((t[3] * -1.0 + t[4] * -1.0) + t[5] + 1.0)]   # of (-1, -1), untruncated


@pytest.mark.parametrize("mode", ["quarter", "taylor"])
def test_corners_edges_plateaus_and_non_finite_windows(mode):
    from ubpl_amd import kernels as Kn
    H = W = 7                                                      # (3, 3) is the centre: a blur's zero padding is symmetric
    v = np.full((8, H, W), 0.5, np.float32)
    v[0, 0, 0] = 0.9                                               # 0: a corner, no eligible axis
    v[1, 0, 3], v[1, 0, 4] = 0.9, 0.7                              # 1: top edge, x alone
    v[2, 2, W - 1], v[2, 1, W - 1] = 0.9, 0.7                      # 2: right edge, y alone
    v[3, 3, 3] = 0.6                                               # 3: symmetric around the peak
    #                                                                4: an exact plateau (constant)
    v[5, 3, 3], v[5, 3, 4], v[5, 2, 3] = 0.9, float("nan"), 0.7    # 5: a NaN neighbour
    v[6, 3, 3], v[6, 3, 2], v[6, 4, 3] = 0.9, float("inf"), 0.7    # 6: an inf neighbour
    v[7, 3, 3], v[7, 1, 3], v[7, 3, 5] = 0.9, float("nan"), float("-inf")   # 7: non-finite two cells away
    raws = [(1.0, 1.0), (4.0, 1.0), (float(W), 3.0)] + [(4.0, 4.0)] * 5
    for taps in (torch.ones(1), Kn.blur_taps(1.0)):
        got, want = _one(v, raws, mode, taps, tinv=_tinv(1, np.random.RandomState(4)))
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert np.array_equal(got[2], want["how"][0]), (got[2], want["how"][0])
        fallback = got[2] < 2
        assert np.array_equal(got[0][fallback], want["raw_sub"][0][fallback])
        assert np.abs(got[0] - want["raw_sub"][0]).max() <= 1e-5
        assert got[2][:3].tolist() == [0.0, 1.0, 1.0]
        assert got[0][:3].tolist() == [[1.0, 1.0], [4.25, 1.0], [float(W), 2.75]]
        assert got[0][3].tolist() == [4.0, 4.0] and got[2][3] == (2.0 if mode == "taylor" else 1.0)
        assert got[0][4].tolist() == [4.0, 4.0]
        assert got[2][5:7].tolist() == [1.0, 1.0]                  # sign(NaN) = 0, sign(-inf) = -1
        assert got[0][5].tolist() == [4.0, 3.75] and got[0][6].tolist() == [3.75, 4.25]
        assert got[0][7].tolist() == [4.0, 4.0]


def test_smallest_map_with_a_taylor_cell():
    """5 x 5: the centre cell alone is eligible; a blob peaking there takes the Taylor step at
    every radius (the window is mostly zero padding), one next to it takes quarter."""
    from ubpl_amd import kernels as Kn
    y, x = np.mgrid[0:5, 0:5].astype(np.float64)
    v = np.stack([0.8 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * 1.5 ** 2)) + 0.05
                  for cx, cy in ((2.3, 1.8), (1.7, 2.2), (1.2, 2.1))]).astype(np.float32)
    raws = [(3.0, 3.0), (3.0, 3.0), (2.0, 3.0)]
    for radius in RADII:
        taps = Kn.blur_taps(SIGMA_OF_RADIUS[radius])
        got, r32 = _one(v, raws, "taylor", taps)
        r64 = RR.refine_ref(v[None], np.array([raws], np.float32), RR.TAYLOR, taps.numpy(), np.float64)
        assert not RR.at_boundary(r64).any()
        assert r64["how"][0].tolist()[2] == 1.0 and (radius > 0 or r64["how"][0].tolist()[:2] == [2.0, 2.0])
        assert np.array_equal(got[2], r64["how"][0])
        tol = max(1e-6, 10.0 * float(np.abs(r32["raw_sub"] - r64["raw_sub"]).max()))
        assert np.abs(got[0] - r64["raw_sub"][0]).max() <= tol


def test_argument_errors():
    from ubpl_amd import _lib
    N, K, H, W = 1, 2, 6, 7
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    a = {"hm": z(N * K * H * W), "hm_flip": None, "sb": K * H * W, "N": N, "K": K, "H": H, "W": W, "perm": None,
         "raw": z(N * K * 2), "mode": 1, "taps": z(7), "radius": 0, "tinv": z(N * 6, dt=torch.float64),
         "raw_sub": z(N * K * 2), "preds_sub": z(N * K * 2), "how": z(N * K)}
    call = lambda **kw: _lib.call("ubpl_refine_peaks", *[kw.get(n, v) for n, v in a.items()])
    call()
    call(mode=2, radius=5)
    for bad in ({"mode": 0}, {"mode": 3}, {"radius": 6}, {"radius": -1}, {"tinv": None}, {"K": 0, "perm": None}):
        with pytest.raises(RuntimeError, match="failed with hipError 1"):
            call(**bad)
    call(N=0)                                                      # no maps: nothing to do
    torch.cuda.synchronize()
