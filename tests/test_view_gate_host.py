"""The view-consistency rule of the training step, host side: the cell convention of
kernels.train_back_matrices against the renderer and against the augmentation's own matrices, the
numpy restatement (tests/view_gate_ref.py) against unc_ref on shared matrices, the options and the
header.  Nothing here touches a device."""
import random
import types

import numpy as np
import pytest
import torch

import unc_ref as UR
import view_gate_ref as VR

R, H = 256, 64


def _two_views(seed):
    """Two draws of the loader's augmentation for one 256x256 image -> the views' [6] matrices."""
    from ubpl_amd.augment import draw_view
    random.seed(seed)
    torch.manual_seed(seed)
    kps = np.zeros((9, 3), np.float32)
    return [draw_view(kps, 256, 256, R, 0.25, 30.0)[0] for _ in range(2)]


def test_renderer_puts_the_peak_where_the_convention_says():
    """C(c) = (R/H) c: a keypoint at view pixel x peaks at the 0-based cell x / (R/H)."""
    from oracle import render as OR
    kps = np.array([[[40, 60, 1], [128, 8, 1], [204, 100, 1]]], np.float32)          # multiples of R/H
    hm, _ = OR.render_batch(kps, (R, R), R, H)
    for k in range(3):
        cy, cx = np.unravel_index(np.argmax(hm[0, k]), hm[0, k].shape)
        assert hm[0, k, cy, cx] == 1.0
        assert ((R / H) * cx, (R / H) * cy) == (kps[0, k, 0], kps[0, k, 1])


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_back_map_round_trip_of_two_views(seed):
    """Source keypoints -> where each view's ideal (continuous) peak lies under the renderer's
    convention -> back through train_back_matrices: both views land on the same source pixel, to
    1e-3 px (float64 arithmetic, back rounded once to float32, coordinates <= 256)."""
    from ubpl_amd import kernels as Kn
    mats = _two_views(seed)
    assert not np.allclose(mats[0], mats[1])
    rs = np.random.RandomState(seed)
    src = rs.uniform(40, 216, (9, 2))                                    # 0-based source pixels
    viewmat = torch.tensor(np.array(mats, np.float32)).reshape(2, 1, 6)
    back = Kn.train_back_matrices(viewmat, R, H)
    assert back.dtype == torch.float32 and back.shape == (2, 1, 6)
    assert np.array_equal(back.numpy(), VR.train_back(viewmat.numpy(), R, H))
    assert np.array_equal(Kn.train_back_matrices([viewmat[0], viewmat[1]], R, H).numpy(), back.numpy())
    got = []
    for v in range(2):
        m = viewmat[v, 0].double().numpy().reshape(2, 3)                 # view pixel -> source pixel
        q = np.linalg.solve(m[:, :2], (src - m[:, 2]).T).T               # the source point's view pixel
        cell = q / (R / H)                                               # the renderer's cell of a keypoint at q
        raw = cell + 1.0                                                 # a decoded peak is 1-based
        b = back[v, 0].double().numpy()
        u, w = raw[:, 0] - 1.0, raw[:, 1] - 1.0
        got.append(np.stack([b[0] * u + b[1] * w + b[2], b[3] * u + b[4] * w + b[5]], -1))
    assert np.abs(got[0] - got[1]).max() < 1e-3
    assert np.abs(got[0] - src).max() < 1e-3


def test_restatement_with_shared_matrices_is_unc_ref():
    rs = np.random.RandomState(5)
    M, V, N, K = 3, 3, 2, 4
    raw = (rs.uniform(10, 50, (N, K, 2)) + rs.normal(0, 0.5, (M, V, N, K, 2))).astype(np.float32)
    raw[0, 1, 0, 0] = 0.0                                                # no peak: not legal
    raw[1, 2, 1, 1] += 30.0                                              # one view far off
    back = rs.uniform(-0.01, 0.01, (V, 6)).astype(np.float32) + np.array([1, 0, 0, 0, 1, 0], np.float32)
    want = UR.view_uncertainty(raw, back, 6.0)
    got = VR.view_gate(raw, np.repeat(back[:, None], N, 1), 6.0)
    for key in UR.KEYS:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    assert np.array_equal(got["gate"], want["select"].all(0).astype(np.float32))
    assert 0 < got["gate"].sum() < got["gate"].size


def _args(**kw):
    return types.SimpleNamespace(pseudoScoreThr=0.9, **kw)


def test_options():
    from ubpl_amd import predict_args as PA
    from ubpl_amd import view_gate as VG
    assert not VG.GateOptions(_args()).on and not VG.GateOptions(_args(pseudoRule="score", distThrMax=3)).on
    o = VG.GateOptions(_args(pseudoRule="uncertainty", distThrMax=4))
    assert o.on and o.dist_thr == 4.0 and o.refine == "taylor" and o.thr == float("-inf")
    assert torch.equal(o.taps, PA.check_refine("taylor", PA.DEFAULT_BLUR_SIGMA)[1])
    o = VG.GateOptions(_args(pseudoRule="score+uncertainty", distThrMax=0.0, pseudoRefine="none"))
    assert o.on and o.thr == 0.9 and o.taps is None and o.refine == "none"
    o = VG.GateOptions(_args(pseudoRule="uncertainty", distThrMax=1, pseudoRefine="taylor", pseudoBlurSigma=0.5))
    assert len(o.taps) == 3
    with pytest.raises(ValueError, match="pseudoRule is one of"):
        VG.GateOptions(_args(pseudoRule="geometry"))
    with pytest.raises(ValueError, match="needs distThrMax"):
        VG.GateOptions(_args(pseudoRule="uncertainty"))
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="distance >= 0"):
            VG.GateOptions(_args(pseudoRule="uncertainty", distThrMax=bad))
    with pytest.raises(ValueError, match="refine is one of"):
        VG.GateOptions(_args(pseudoRule="uncertainty", distThrMax=1, pseudoRefine="fine"))
    on = VG.GateOptions(_args(pseudoRule="uncertainty", distThrMax=4))
    vm = [torch.zeros(2, 6)] * 2
    VG.check_batch(on, {"viewmat": vm}, 2, 2)
    with pytest.raises(ValueError, match='needs meta\\["viewmat"\\]'):
        VG.check_batch(on, {"kps": None}, 2, 2)
    with pytest.raises(ValueError, match="at least 2"):
        VG.check_batch(on, {"viewmat": vm[:1]}, 1, 2)
    # options(): one object per set of option values, whatever namespace carries them
    a1, a2 = _args(pseudoRule="uncertainty", distThrMax=4), _args(pseudoRule="uncertainty", distThrMax=4)
    assert VG.options(a1) is VG.options(a2) and VG.options(a1).on
    assert VG.options(a1) is not VG.options(_args(pseudoRule="uncertainty", distThrMax=5))
    assert not VG.options(_args()).on
    with pytest.raises(ValueError, match="needs distThrMax"):
        VG.options(_args(pseudoRule="uncertainty"))
    VG.refuse(_args(), "train_mt")
    with pytest.raises(ValueError, match="train_mt_ubpl only"):
        VG.refuse(_args(pseudoRule="uncertainty", distThrMax=4), "train_mt")


def test_wrapper_checks_raise_without_a_gpu():
    from ubpl_amd import kernels as Kn
    z = torch.zeros(64)
    for M in (0, 9):
        with pytest.raises(ValueError, match="1 to 8 members"):
            Kn.view_uncertainty_samples(z, 0, 2, M, 2, 1, 1, z, z)
    for V in (1, 17):
        with pytest.raises(ValueError, match="2 to 16 views"):
            Kn.view_uncertainty_samples(z, 0, 2, 1, V, 1, 1, z, z)
    with pytest.raises(ValueError, match="train_back_matrices|viewmat is"):
        Kn.train_back_matrices(torch.zeros(2, 6), 256, 64)
    with pytest.raises(ValueError, match="gate of"):
        Kn.loss_finalize(3, z, z, z, None, None, False, True, 2, 1, 2, 0.5)


def test_header_declares_the_new_entry():
    from ubpl_amd import _abi, _lib
    decls = {name: (params, ann) for _, name, params, ann in _abi.parse(open(_lib.HEADER_PATH).read())}
    params, ann = decls["ubpl_view_uncertainty_samples"]
    assert [p for _, p in params] == ["raw", "sm", "sv", "M", "V", "N", "K", "back", "dist_thr", "pts", "legal",
                                      "int_dist", "aug_coord", "ext_dist", "aext_dist", "ext_views", "mix_dist",
                                      "unc", "select", "gate", "stream"]
    assert ann["raw"] == ("f32", "(M-1)*sm+(V-1)*sv+(int64_t)N*K*2") and ann["back"] == ("f32", "(int64_t)V*N*6")
    assert ann["gate"] == ("f32", "N*K") and ann["select"] == ("f32", "(int64_t)M*N*K")
    assert "ubpl_view_uncertainty_samples" in _lib.signatures()


def test_keypoint_path_and_pixel_path_agree_within_a_pixel():
    """What the cell convention C(c) = (R/H) c leaves: the loader's keypoint path (transform_point:
    p - 1, a float64 product truncated, + 1; kps_fliplr: W - x) against its pixel path (warp_matrix).
    100 draws of two views on synthetic keypoints, host arithmetic: a rendered keypoint's cell
    (kp / (R/H), exact on ideal peaks) mapped back through train_back_matrices, against the
    keypoint's source pixel.  Each path truncates or shifts by at most a pixel, so the mean
    absolute error per axis stays below one source pixel at every scale draw (<= 1.25); the figures
    for both readings of the keypoint coordinate (pixel x, or 1-based index x - 1) are printed —
    DESIGN.md §4 quotes them."""
    from ubpl_amd import kernels as Kn
    from ubpl_amd.augment import draw_view
    rs = np.random.RandomState(11)
    for off in (0.0, 1.0):
        random.seed(0)
        torch.manual_seed(0)
        dist, err = [], []
        for _ in range(100):
            k = np.concatenate([rs.randint(60, 196, (9, 2)), np.ones((9, 1))], 1).astype(np.float32)
            pts, ok = [], np.ones(9, bool)
            for _ in range(2):
                m, _, ko = draw_view(k, 256, 256, R, 0.25, 30.0)
                ok &= (ko[:, :2] > 12).all(1) & (ko[:, :2] < 244).all(1)
                back = Kn.train_back_matrices(torch.tensor(m, dtype=torch.float32).reshape(1, 1, 6), R, H)
                b = back[0, 0].double().numpy()
                c = (ko[:, :2].astype(np.float64) - off) / (R / H)              # the peak's 0-based cell
                pts.append(np.stack([b[0] * c[:, 0] + b[1] * c[:, 1] + b[2],
                                     b[3] * c[:, 0] + b[4] * c[:, 1] + b[5]], -1))
            dist += list(np.linalg.norm(pts[0] - pts[1], axis=1)[ok])
            err += [p[ok] - (k[ok, :2] - 1.0) for p in pts]
        err = np.concatenate(err)
        print("keypoint read as %s: error to the source pixel mean (%.2f, %.2f), mean abs (%.2f, %.2f) px; "
              "the two views %.2f px apart on average, %.2f at most, over %d joints"
              % ("pixel x" if off == 0 else "index x - 1", *err.mean(0), *np.abs(err).mean(0), np.mean(dist),
                 np.max(dist), len(dist)))
        if off == 0.0:
            assert len(dist) > 300 and (np.abs(err).mean(0) < 1.0).all()
