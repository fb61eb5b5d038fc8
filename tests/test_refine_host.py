"""CPU-only checks of the sub-pixel decode: the header entry and its generated op's argument
checks, the blur taps, the argument errors of Predictor raised before any GPU use, and the
rule itself — the float64 restatement (tests/refine_ref.py) recovers the centres of maps drawn
by the project's own oracle renderer."""
import math
import os

import numpy as np
import pytest
import torch

import refine_ref as RR
from oracle import render as OR


def test_header_declares_refine_peaks():
    from ubpl_amd import _abi, _lib
    decls = {name: (params, ann) for _, name, params, ann in _abi.parse(open(_lib.HEADER_PATH).read())}
    params, ann = decls["ubpl_refine_peaks"]
    assert [p for _, p in params] == ["hm", "hm_flip", "sb", "N", "K", "H", "W", "perm", "raw", "mode", "taps",
                                      "radius", "tinv", "raw_sub", "preds_sub", "how", "stream"]
    assert ann["taps"] == ("f32", "radius+1") and ann["tinv"] == ("f64", "N*6") and ann["how"] == ("f32", "N*K")
    assert ann["hm"] == ann["hm_flip"] == ("f32", "(N-1)*sb+(int64_t)K*H*W")
    assert "ubpl_refine_peaks" in _lib.signatures()


def test_refine_peaks_op_checks_arguments_before_the_call():
    from ubpl_amd import _lib
    if not os.path.exists(_lib.OPS_PATH):
        pytest.skip("libubpl_ops.so not built (run __graft_entry__.build())")
    ops = _lib.load_ops()
    N, K, H, W, S, radius = 2, 3, 6, 7, 2, 3
    sb, last = S * K * H * W, (S - 1) * K * H * W
    hm = torch.zeros(N * sb)[last:]
    assert hm.numel() == (N - 1) * sb + K * H * W                  # exactly what the strided maps need
    a = {"hm": hm, "hm_flip": hm.clone(), "sb": sb, "N": N, "K": K, "H": H, "W": W,
         "perm": torch.zeros(K, dtype=torch.int32), "raw": torch.zeros(N * K * 2), "mode": 2,
         "taps": torch.zeros(radius + 1), "radius": radius, "tinv": torch.zeros(N * 6, dtype=torch.float64),
         "raw_sub": torch.zeros(N * K * 2), "preds_sub": torch.zeros(N * K * 2), "how": torch.zeros(N * K)}
    call = lambda **kw: ops.refine_peaks(*[kw.get(n, v) for n, v in a.items()])
    for name in ("hm", "hm_flip"):
        with pytest.raises(RuntimeError, match="%s holds %d elements" % (name, hm.numel() - 1)):
            call(**{name: hm[1:]})
    with pytest.raises(RuntimeError, match="taps holds %d elements" % radius):
        call(taps=a["taps"][1:])
    with pytest.raises(RuntimeError, match="taps holds %d elements, the sizes passed need %d" % (radius + 1, 6)):
        call(radius=5)
    with pytest.raises(RuntimeError, match="perm must be i32"):
        call(perm=a["perm"].long())
    with pytest.raises(RuntimeError, match="tinv must be f64"):
        call(tinv=a["tinv"].float())
    with pytest.raises(RuntimeError, match="raw must be f32"):
        call(raw=a["raw"].double())
    with pytest.raises(RuntimeError, match="how holds %d elements" % (N * K - 1)):
        call(how=a["how"][1:])
    for name in ("raw", "raw_sub", "preds_sub"):
        with pytest.raises(RuntimeError, match="%s holds %d elements" % (name, N * K * 2 - 1)):
            call(**{name: a[name][1:]})
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        call()                                                     # every check passes: refused on CPU
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        call(hm_flip=None, perm=None, tinv=None, preds_sub=None, how=None)   # the nullable ones


def test_blur_taps():
    from ubpl_amd import kernels as Kn
    for sigma in (0.0, -1.0):
        assert Kn.blur_taps(sigma).tolist() == [1.0]
    for sigma, radius in ((0.4, 1), (0.5, 2), (1.0, 3), (1.2, 3), (1.5, 4), (1.7, 5), (2.0, 5)):
        w = Kn.blur_taps(sigma)
        assert w.dtype == torch.float32 and w.shape == (radius + 1,), sigma
        g = np.exp(-np.arange(radius + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
        want = (g / (g[0] + 2.0 * g[1:].sum())).astype(np.float32)
        assert np.array_equal(w.numpy(), want), sigma
        assert abs(float(w[0].double() + 2.0 * w[1:].double().sum()) - 1.0) < 1e-6
        assert all(w[j] > w[j + 1] > 0 for j in range(radius))
    for sigma in (2.01, 3.0):
        with pytest.raises(ValueError, match="sigma <= 2.0"):
            Kn.blur_taps(sigma)


def test_predictor_refine_arguments_are_checked_before_the_gpu():
    """Raised from the arguments alone: no network, no device is looked at."""
    from ubpl_amd import Predictor
    from ubpl_amd import predict as P
    for bad in ("Quarter", "dark", "", None, 1):
        with pytest.raises(ValueError, match="refine is one of none, quarter, taylor"):
            Predictor(None, refine=bad)
    with pytest.raises(ValueError, match="sigma <= 2.0"):
        Predictor(None, refine="taylor", blur_sigma=2.5)
    assert P.check_refine("none", 99.0) == ("none", None)          # the blur belongs to Taylor alone
    mode, taps = P.check_refine("quarter", 99.0)
    assert mode == "quarter" and taps.tolist() == [1.0]
    mode, taps = P.check_refine("taylor", 1.0)
    assert mode == "taylor" and taps.shape == (4,)
    assert P.check_refine("taylor", 0.0)[1].tolist() == [1.0]
    assert 0.0 <= P.DEFAULT_BLUR_SIGMA <= 2.0


def test_wrapper_refuses_bad_modes_and_host_tensors():
    from ubpl_amd import kernels as Kn
    z = torch.zeros(1, 1, 5, 5)
    with pytest.raises(ValueError, match="refine mode is one of quarter, taylor"):
        Kn.refine_peaks(z, None, 25, 1, 1, 5, 5, None, torch.zeros(1, 1, 2), "none", torch.ones(1))
    with pytest.raises(RuntimeError):                              # no CPU fallback
        Kn.refine_peaks(z, None, 25, 1, 1, 5, 5, None, torch.zeros(1, 1, 2), "quarter", torch.ones(1))


# ---------------------------------------------------------------- the rule on rendered targets
def _rendered(seed=0, groups=12):
    """Maps of the oracle renderer at the project's settings (256 -> 64, sigma 3 cells, 0.01
    cutoff), keypoints in 24 <= x, y < 232 (visible, and the peak six cells or more from the
    border): every one of the 16 quarter-cell phases of the centre, `groups` times.
    -> (hm [G,16,64,64] float32, centres [G,16,2] in cells)."""
    rs = np.random.RandomState(seed)
    kps = np.ones((groups, 16, 3), np.float32)
    for g in range(groups):
        for p in range(16):
            kps[g, p, 0] = 4 * rs.randint(6, 58) + p % 4
            kps[g, p, 1] = 4 * rs.randint(6, 58) + p // 4
    assert kps[..., :2].min() >= 24 and kps[..., :2].max() < 232
    hm, after = OR.render_batch(kps, (256, 256), 256, 64)
    assert (after[..., 2] == 1).all()
    return hm, kps[..., :2].astype(np.float64) / 4.0


def _raw_peaks(hm):
    """The decode's 1-based (col, row) of the first maximum."""
    N, K, H, W = hm.shape
    idx = hm.reshape(N, K, -1).argmax(-1)
    return np.stack([idx % W + 1, idx // W + 1], -1).astype(np.float32)


def _errors(hm, centres, mode, sigma):
    from ubpl_amd import kernels as Kn
    raw = _raw_peaks(hm)
    ref = RR.refine_ref(hm, raw, mode, Kn.blur_taps(sigma).numpy(), np.float64)
    err = np.sqrt(((ref["raw_sub"] - 1.0 - centres) ** 2).sum(-1))
    return err, ref["how"], np.sqrt(((raw - 1.0 - centres) ** 2).sum(-1))


def test_restatement_recovers_rendered_centres():
    hm, centres = _rendered()
    quarter, how, integer = _errors(hm, centres, RR.QUARTER, 0.0)
    assert (how == 1).all()
    assert integer.max() > 0.7 and 0.3 < integer.mean() < 0.5          # what the lattice costs
    assert quarter.max() <= 0.25 * math.sqrt(2.0) + 1e-6
    for sigma in (0.0, 1.0):
        err, how, _ = _errors(hm, centres, RR.TAYLOR, sigma)
        assert (how == 2).all(), sigma
        assert err.max() <= 1e-4, (sigma, err.max())
    err, how, _ = _errors(hm, centres, RR.TAYLOR, 2.0)
    assert (how == 2).all()
    assert err.mean() < quarter.mean(), (err.mean(), quarter.mean())


def test_restatement_float32_tracks_float64_on_rendered_centres():
    """The float32 instance (the kernel's arithmetic) takes the same branch and lands within
    1e-4 cells of the float64 one on these maps."""
    from ubpl_amd import kernels as Kn
    hm, _ = _rendered(seed=1, groups=3)
    raw = _raw_peaks(hm)
    for sigma in (0.0, 1.0, 2.0):
        taps = Kn.blur_taps(sigma).numpy()
        a, b = RR.refine_ref(hm, raw, RR.TAYLOR, taps, np.float32), RR.refine_ref(hm, raw, RR.TAYLOR, taps, np.float64)
        assert a["raw_sub"].dtype == np.float32 and np.array_equal(a["how"], b["how"])
        assert np.abs(a["raw_sub"] - b["raw_sub"]).max() < 1e-4, sigma


def test_restatement_edges():
    taps = np.ones(1, np.float32)
    v = np.full((1, 1, 6, 7), 0.5, np.float32)
    for mode in (RR.QUARTER, RR.TAYLOR):
        # no peak, a raw outside the map, a peak that is not positive
        for raw in ((0, 0), (8, 3), (3, 7), (-1, 2), (float("nan"), 2)):
            r = RR.refine_ref(v, np.array([[raw]], np.float32), mode, taps, np.float32)
            assert r["how"][0, 0] == 0 and np.array_equal(r["raw_sub"][0, 0], np.array(raw, np.float32), equal_nan=True)
        z = v.copy()
        z[0, 0, 2, 3] = 0.0
        assert RR.refine_ref(z, np.array([[(4, 3)]], np.float32), mode, taps, np.float32)["how"][0, 0] == 0
        # a corner: no eligible axis; an edge: one
        r = RR.refine_ref(v, np.array([[(1, 1)]], np.float32), mode, taps, np.float32)
        assert r["how"][0, 0] == 0 and r["raw_sub"][0, 0].tolist() == [1.0, 1.0]
        e = v.copy()
        e[0, 0, 0, 3], e[0, 0, 0, 4] = 0.9, 0.7
        r = RR.refine_ref(e, np.array([[(4, 1)]], np.float32), mode, taps, np.float32)
        assert r["how"][0, 0] == 1 and r["raw_sub"][0, 0].tolist() == [4.25, 1.0]
        # a NaN neighbour: that axis stays put, the other moves; nothing is NaN
        q = v.copy()
        q[0, 0, 3, 3], q[0, 0, 3, 4], q[0, 0, 2, 3] = 0.9, float("nan"), 0.7
        r = RR.refine_ref(q, np.array([[(4, 4)]], np.float32), mode, taps, np.float32)
        assert r["how"][0, 0] == 1 and r["raw_sub"][0, 0].tolist() == [4.0, 3.75]
    # a symmetric peak: Taylor's step is zero
    s = v.copy()
    s[0, 0, 3, 3] = 0.6
    r = RR.refine_ref(s, np.array([[(4, 4)]], np.float32), RR.TAYLOR, taps, np.float32)
    assert r["how"][0, 0] == 2 and r["raw_sub"][0, 0].tolist() == [4.0, 4.0]
    # the transform is finish_map's without the truncation
    tinv = np.array([[1.5, 0.25, -3.0, -0.125, 2.0, 7.0]])
    r = RR.refine_ref(e, np.array([[(4, 1)]], np.float32), RR.QUARTER, taps, np.float32, tinv=tinv)
    assert r["preds_sub"][0, 0].tolist() == [np.float32(1.5 * 3.25 - 3.0 + 1.0), np.float32(-0.125 * 3.25 + 7.0 + 1.0)]
