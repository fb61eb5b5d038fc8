"""CPU-only checks of multi-view test-time augmentation: the float32 restatement of the kernels
(tests/tta_ref.py) against the reference's own affine_back2 (tests/golden/tta.npz), the
conversion between affine_grid's convention and pixel matrices, the view convention's round
trip, the mirror composition, Predictor's argument checks and the identity + mirror merge."""
import os

import numpy as np
import pytest
import torch

import tta_ref as TR

SHAPES = [(2, 3, 8, 8), (2, 5, 24, 40), (2, 4, 64, 64)]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tta.npz")


def _fixture():
    return dict(np.load(FIXTURE))


def fixture_distances(fx, ref=TR):
    """Per shape of the fixture: the maximum absolute distance from the reference's float64
    affine_back2 of (ours) the float32 restatement fed affine_theta_to_pixels(theta) o mirror
    and of (ref) the reference's own float32 affine_back2; for the maps and for the coverage."""
    from ubpl_amd import kernels as Kn
    out = {}
    for name in sorted({k.split("/")[0] for k in fx}):
        hm, theta, isflip = fx[name + "/hm"], fx[name + "/theta"], fx[name + "/isflip"]
        N, K, H, W = hm.shape
        mats = Kn.affine_theta_to_pixels(theta, H, W)
        ours, cov = np.empty_like(hm), np.empty((N, 1, H, W), np.float32)
        for n in range(N):
            m = Kn.compose_pixels(mats[n], Kn.mirror_pixels(W)) if isflip[n] else mats[n:n + 1]
            ours[n], cov[n, 0] = ref.sample_plane(hm[n], m.to(torch.float32).numpy()[0], np.float32)
        assert ours.dtype == np.float32 and fx[name + "/back32"].dtype == np.float32
        b64, c64 = fx[name + "/back64"], fx[name + "/cov64"]
        out[name] = {"ours": float(np.abs(ours - b64).max()), "ref": float(np.abs(fx[name + "/back32"] - b64).max()),
                     "ours_cov": float(np.abs(cov - c64).max()),
                     "ref_cov": float(np.abs(fx[name + "/cov32"] - c64).max())}
    return out


def test_restatement_against_the_reference_back_warp():
    """Two float32 roundings of the same coordinates, measured against the reference's float64
    result: the restatement's distance is at most 4x the reference's own float32 distance.
    Measured when the fixture was made (ours / ref): maps 8x8 1.69e-07 / 2.67e-07, 24x40
    1.19e-06 / 6.97e-07, 64x64 8.00e-07 / 1.19e-06; coverage 6.41e-07 / 8.49e-07, 4.21e-06 /
    3.70e-06, 5.53e-06 / 7.88e-06 (ratios 0.63 to 1.7)."""
    fx = _fixture()
    assert sorted(fx[k].shape for k in fx if k.endswith("/hm")) == sorted(SHAPES)
    assert os.path.getsize(FIXTURE) < 200 * 1024
    for name, d in fixture_distances(fx).items():
        print(name, d)
        assert d["ref"] > 0 and d["ref_cov"] > 0, name
        assert d["ours"] <= 4 * d["ref"], (name, d)
        assert d["ours_cov"] <= 4 * d["ref_cov"], (name, d)
    assert any(fx[k].any() for k in fx if k.endswith("/isflip")) and any(fx[k][:, :, 2].any() for k in fx
                                                                        if k.endswith("/theta"))


def test_theta_conversion_round_trips_on_non_square_planes():
    from ubpl_amd import kernels as Kn
    rs = np.random.RandomState(3)
    theta = rs.uniform(-1.5, 1.5, (5, 2, 3))
    for H, W in ((24, 40), (7, 3), (2, 64)):
        m = Kn.affine_theta_to_pixels(theta, H, W)
        assert m.dtype == torch.float64 and m.shape == (5, 6)
        assert np.abs(Kn.affine_pixels_to_theta(m, H, W).numpy() - theta).max() < 1e-12
        assert np.abs(Kn.affine_theta_to_pixels(Kn.affine_pixels_to_theta(m, H, W), H, W).numpy() - m.numpy()).max() < 1e-10
        # the pixel matrix samples where affine_grid does: corner (W-1, 0) of the output
        g = torch.nn.functional.affine_grid(torch.from_numpy(theta), (5, 1, H, W), align_corners=True)
        want = (g[:, 0, W - 1].numpy() + 1.0) * np.array([(W - 1) / 2.0, (H - 1) / 2.0])
        got = np.stack([m[:, 0] * (W - 1) + m[:, 2], m[:, 3] * (W - 1) + m[:, 5]], -1)
        assert np.abs(got - want).max() < 1e-10
    ident = Kn.affine_theta_to_pixels([[1.0, 0, 0], [0, 1.0, 0]], 24, 40)
    assert ident.tolist() == [list(TR.IDENTITY)]
    for H, W in ((1, 5), (5, 1)):
        with pytest.raises(ValueError, match="align_corners"):
            Kn.affine_theta_to_pixels(theta, H, W)
        with pytest.raises(ValueError, match="align_corners"):
            Kn.affine_pixels_to_theta(theta.reshape(5, 6), H, W)


BLOBS = [(20.0, 20.0), (32.0, 40.0), (45.0, 25.0), (31.5, 31.5)]
VIEWS = [(15.0, 1.0), (-30.0, 1.25), (0.0, 0.8), (30.0, 0.75)]


def _blob(cx, cy, S=64, sigma=3.0):
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    return np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma)).astype(np.float32)


@pytest.mark.parametrize("flip", [False, True])
def test_view_convention_round_trip(flip):
    """A blob warped into a view with img_mat and brought back with hm_mat (same resolution)
    peaks within 1 cell of where it was — all 16 blob x view cases (worst measured: 0.71), and
    their mirrored views too."""
    from ubpl_amd import kernels as Kn
    img_mat, hm_mat, swap = Kn.view_matrices(VIEWS, flip, 64, 64)
    assert img_mat.dtype == hm_mat.dtype == torch.float32 and swap.dtype == torch.int32
    assert swap.tolist() == [0] * 4 + [1] * 4 * flip
    worst = 0.0
    for cx, cy in BLOBS:
        src = _blob(cx, cy)
        for v in range(len(img_mat)):
            view = TR.sample_plane(src, img_mat[v].numpy())[0]
            back = TR.sample_plane(view, hm_mat[v].numpy())[0]
            r, c = np.unravel_index(back.argmax(), back.shape)
            worst = max(worst, float(np.hypot(c - cx, r - cy)))
    print("worst", worst)
    assert worst <= 1.0


def test_centres_of_image_and_heatmap_agree():
    """Heatmap cell i sits at image coordinate 4 i + 1.5: a view's image matrix and the inverse
    of its heatmap matrix are the same map in those units."""
    from ubpl_amd import kernels as Kn
    img_mat, hm_mat, _ = Kn.view_matrices(VIEWS, True, 256, 64)
    for v in range(8):
        a, b = img_mat[v].double().numpy().reshape(2, 3), hm_mat[v].double().numpy().reshape(2, 3)
        q = np.array([[3.0, 50.0], [40.0, 7.5]])                     # view heatmap cells
        p_img = (4 * q + 1.5) @ a[:, :2].T + a[:, 2]                  # view -> original, image pixels
        back = ((p_img - 1.5) / 4) @ b[:, :2].T + b[:, 2]             # original -> view, cells
        assert np.abs(back - q).max() < 1e-4, v


def test_mirrored_views_are_the_explicit_composition():
    from ubpl_amd import kernels as Kn
    S = 16
    views = [(0.0, 1.0)] + VIEWS
    img_mat, hm_mat, swap = Kn.view_matrices(views, True, S, S)
    T = len(views)
    rs = np.random.RandomState(5)
    img = rs.uniform(0, 1, (S, S)).astype(np.float64)
    for v in range(T):
        # view_f(q) = view(m(q)): the mirrored view is the plain view, mirrored
        plain = TR.sample_plane(img, img_mat[v].numpy(), np.float64)[0]
        mirrored = TR.sample_plane(img, img_mat[T + v].numpy(), np.float64)[0]
        assert np.abs(mirrored - plain[:, ::-1]).max() < 1e-5, v
        # the heatmap of a mirrored view is read at m(q): mirroring the view's map first, then
        # the plain view's matrix, gives the same
        hm = rs.uniform(0, 1, (S, S)).astype(np.float64)
        a = TR.sample_plane(hm, hm_mat[T + v].numpy(), np.float64)[0]
        b = TR.sample_plane(hm[:, ::-1].copy(), hm_mat[v].numpy(), np.float64)[0]
        assert np.abs(a - b).max() < 1e-5, v
    assert img_mat[0].tolist() == list(TR.IDENTITY) == hm_mat[0].tolist()
    assert img_mat[T].tolist() == [-1.0, 0.0, S - 1.0, 0.0, 1.0, 0.0] == hm_mat[T].tolist()


def test_check_tta_raises_without_a_gpu():
    from ubpl_amd import Predictor
    from ubpl_amd import predict as P
    assert P.check_tta(None, True) is None
    assert P.check_tta([(0, 1), (10, 1.25)], False) == [(0.0, 1.0), (10.0, 1.25)]
    for bad, match in (([(0, 1), (float("nan"), 1)], "finite"), ([(0, 1), (5, float("inf"))], "finite"),
                       ([(0, 1), (5, 0.49)], r"\[0.5, 2\]"), ([(0, 1), (5, 2.01)], r"\[0.5, 2\]"),
                       ([(5, 1), (0, 1)], "first tta view"), ([(0, 1.1)], "first tta view"), ([], "first tta view"),
                       ([(0, 1)] + [(i, 1) for i in range(16)], "at most 16"), ([0, 1], "list of"),
                       ("ab", "list of")):
        with pytest.raises(ValueError, match=match):
            Predictor(None, tta=bad)
    with pytest.raises(ValueError, match="with their mirrors make 18, at most 16"):
        Predictor(None, flip_test=True, tta=[(0, 1)] + [(i, 1) for i in range(1, 9)])
    assert len(P.check_tta([(0, 1)] + [(i, 1) for i in range(1, 8)], True)) == 8      # 16 with mirrors


def test_identity_plus_mirror_is_the_flip_test_merge():
    """V = 2, identity + mirror, restates (hm + flip-back) * 0.5f bit for bit on finite maps."""
    import refine_ref as RR
    from ubpl_amd import kernels as Kn
    rs = np.random.RandomState(7)
    for N, K, H, W in ((1, 1, 4, 4), (2, 6, 24, 40), (1, 3, 64, 64)):
        hm = (rs.standard_normal((2, N, K, H, W)) * rs.choice([1e-3, 1.0, 1e3], (2, N, K, 1, 1))).astype(np.float32)
        hm[0, 0, 0, 0, :2] = (0.0, -0.0)
        _, hm_mat, swap = Kn.view_matrices([(0, 1)], True, 4 * W, W)
        hm_mat = hm_mat.numpy()                                     # (the mirror moves x only: H may differ)
        perm = rs.permutation(K)
        for pm in (None, perm):
            want = RR.merged_maps(hm[0], hm[1], pm)
            got = TR.merge_views(hm, hm_mat, swap.numpy(), pm)
            assert got.dtype == np.float32 and np.array_equal(got, want)


def test_restatement_edges():
    hm = np.arange(2 * 12, dtype=np.float32).reshape(2, 1, 1, 3, 4) + 1
    ident = np.array(TR.IDENTITY, np.float32)
    far = np.array([1, 0, 1e9, 0, 1, 0], np.float32)
    nan = np.array([1, 0, np.nan, 0, 1, 0], np.float32)
    half = np.array([1, 0, 0.5, 0, 1, 0], np.float32)
    # a view wholly outside contributes nothing; covered by no view: 0
    assert np.array_equal(TR.merge_views(hm, [ident, far]), hm[0])
    assert np.array_equal(TR.merge_views(hm, [ident, nan]), hm[0])
    assert not TR.merge_views(hm, [far, nan]).any()
    # half a pixel to the right: the last column is half covered, and averaged over its coverage
    s, c = TR.sample_plane(hm[0, 0, 0], half)
    assert c[:, -1].tolist() == [0.5] * 3 and c[:, :-1].min() == 1.0
    assert s[0].tolist() == [1.5, 2.5, 3.5, 2.0]
    assert TR.merge_views(hm[:1], [half])[0, 0, 0].tolist() == [1.5, 2.5, 3.5, 4.0]
    # V = 1, identity: the maps themselves, NaN and inf included
    odd = hm[:1].copy()
    odd[0, 0, 0, 1, 1], odd[0, 0, 0, 2, 2] = np.nan, np.inf
    assert np.array_equal(TR.merge_views(odd, [ident]), odd[0], equal_nan=True)
