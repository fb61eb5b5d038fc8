"""Cross-view pseudo-label targets, host side: kernels.train_pair_matrices against its numpy
restatement (tests/cross_view_ref.py) and against geometry — rendered targets of two views of the
Mouse fixture's labelled rows warped into one another — the options, the wrapper's checks and the
header.  Nothing here touches a device."""
import os
import random
import types

import numpy as np
import pytest
import torch

import cross_view_ref as CR

R, H = 256, 64
PACK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mouse_100_500_0.3")


def _draws(seed, kps_rows):
    """Two draws of the loader's augmentation per row of keypoints [N,K,3] (256x256 images)
    -> (viewmat [2,N,6] float32, the views' keypoints [2,N,K,3])."""
    from ubpl_amd.augment import draw_view
    random.seed(seed)
    torch.manual_seed(seed)
    mats, kps = [], []
    for k in kps_rows:
        d = [draw_view(k, 256, 256, R, 0.25, 30.0) for _ in range(2)]
        mats.append([v[0] for v in d])
        kps.append([v[2] for v in d])
    return (np.ascontiguousarray(np.array(mats, np.float32).transpose(1, 0, 2)),
            np.ascontiguousarray(np.array(kps, np.float32).transpose(1, 0, 2, 3)))


def _viewmats(seed, N=6):
    return _draws(seed, np.zeros((N, 9, 3), np.float32))[0]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_pair_matrices_equal_the_restatement_bit_for_bit(seed):
    from ubpl_amd import kernels as Kn
    vm = _viewmats(seed)
    got = Kn.train_pair_matrices(torch.from_numpy(vm), R, H)
    assert got.dtype == torch.float32 and got.shape == (2, 2, vm.shape[1], 6) and got.is_contiguous()
    want = CR.pair_matrices(vm, R, H)
    assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
    as_list = Kn.train_pair_matrices([torch.from_numpy(vm[0]), torch.from_numpy(vm[1])], R, H)
    assert torch.equal(as_list, got)
    # three views: every pair, not only (0, 1)
    vm3 = np.concatenate([vm, _viewmats(seed + 10)[:1]])
    assert np.array_equal(Kn.train_pair_matrices(torch.from_numpy(vm3), R, H).numpy().view(np.int32),
                          CR.pair_matrices(vm3, R, H).view(np.int32))


def test_pair_matrix_properties():
    from ubpl_amd import kernels as Kn
    flips_differ = 0
    for seed in range(6):
        vm = _viewmats(seed)
        P = Kn.train_pair_matrices(torch.from_numpy(vm), R, H).numpy()
        for a in range(2):
            assert (P[a, a] == CR.IDENTITY).all()                          # exactly, no arithmetic
        p, q = P[0, 1].astype(np.float64), P[1, 0].astype(np.float64)      # P[0][1] o P[1][0] = identity
        comp = np.stack([p[:, 0] * q[:, 0] + p[:, 1] * q[:, 3], p[:, 0] * q[:, 1] + p[:, 1] * q[:, 4],
                         p[:, 0] * q[:, 2] + p[:, 1] * q[:, 5] + p[:, 2],
                         p[:, 3] * q[:, 0] + p[:, 4] * q[:, 3], p[:, 3] * q[:, 1] + p[:, 4] * q[:, 4],
                         p[:, 3] * q[:, 2] + p[:, 4] * q[:, 5] + p[:, 5]], -1)
        print("seed %d: P[0][1] o P[1][0] - identity, largest entry %.3g" % (seed, np.abs(comp - CR.IDENTITY).max()))
        assert np.abs(comp - CR.IDENTITY).max() < 1e-5
        det_view = vm[..., 0] * vm[..., 4] - vm[..., 1] * vm[..., 3]       # < 0: the view is mirrored
        det_pair = P[0, 1][:, 0] * P[0, 1][:, 4] - P[0, 1][:, 1] * P[0, 1][:, 3]
        differ = (det_view[0] < 0) != (det_view[1] < 0)
        assert ((det_pair < 0) == differ).all()
        flips_differ += int(differ.sum())
    assert flips_differ > 0


def _labelled_rows():
    with np.load(os.path.join(PACK, "meta.npz")) as z:
        kps, isl = z["train_kps"][:20], z["train_islabeled"][:20].astype(bool)
    return kps[isl].astype(np.float32)


def test_warped_targets_peak_where_the_views_own_targets_peak():
    """Geometry, independent of the convention's wording: both views' keypoints rendered, each
    view's maps warped into the other's frame under the product's matrices.  For every joint the
    renderer calls visible in both views whose own peak is at least 2 cells from the border, the
    warped map's argmax lies within one cell per axis of the own map's, and the warped peak is at
    least 0.9 (a Gaussian of sigma 1 sampled half a cell off its centre keeps exp(-1/8) = 0.88 of
    its height at worst on one axis; rotation and zoom put the sample nearer than that here)."""
    from oracle import render as OR
    from ubpl_amd import kernels as Kn
    rows = _labelled_rows()
    N, K = rows.shape[:2]
    count, worst, low = 0, 0.0, 1.0
    for seed in range(8):
        vm, kps = _draws(seed, rows)
        hm, vis = [], []
        for v in range(2):
            h, kk = OR.render_batch(kps[v], (R, R), R, H)
            hm.append(h)
            vis.append(kk[:, :, 2] > 0)
        hm = np.stack(hm)[:, None]                                         # [2,1,N,K,H,H]
        P = Kn.train_pair_matrices(torch.from_numpy(vm), R, H).numpy()
        warped, _ = CR.merge_views_samples(hm, P, include_self=False)       # warped[a] = view 1 - a in a's frame
        both = vis[0] & vis[1]
        for a in range(2):
            own = hm[a, 0].reshape(N, K, -1).argmax(-1)
            got = warped[a, 0].reshape(N, K, -1).argmax(-1)
            oy, ox, gy, gx = own // H, own % H, got // H, got % H
            ok = both & (ox >= 2) & (ox <= H - 3) & (oy >= 2) & (oy <= H - 3)
            peak = warped[a, 0].reshape(N, K, -1).max(-1)
            assert (np.abs(gx - ox)[ok] <= 1).all() and (np.abs(gy - oy)[ok] <= 1).all(), (seed, a)
            assert (peak[ok] >= 0.9).all(), (seed, a, peak[ok].min())
            count += int(ok.sum())
            worst = max(worst, float(np.hypot(gx - ox, gy - oy)[ok].max()))
            low = min(low, float(peak[ok].min()))
    print("%d joints, maximum distance %.3f cells, smallest warped peak %.3f" % (count, worst, low))
    assert count >= 300


def _args(**kw):
    return types.SimpleNamespace(pseudoScoreThr=0.9, **kw)


def test_options():
    from ubpl_amd import view_gate as VG
    assert VG.VIEWS == ("own", "merged", "other")
    for a in (_args(), _args(pseudoViews="own")):
        o = VG.GateOptions(a)
        assert o.views == "own" and not o.cross and not o.on
    for v in ("merged", "other"):
        o = VG.GateOptions(_args(pseudoViews=v))
        assert o.views == v and o.cross and not o.on and o.sel_rate is None
    o = VG.GateOptions(_args(pseudoViews="merged", pseudoRule="uncertainty", distThrMax=4))
    assert o.cross and o.on
    assert VG.GateOptions(_args(pseudoViews="other", pseudoRule="rate", pseudoSelRate=0.5)).sel_rate == 0.5
    with pytest.raises(ValueError, match="pseudoViews is one of own, merged, other"):
        VG.GateOptions(_args(pseudoViews="all"))
    # the option is part of options()' key
    assert VG.options(_args(pseudoViews="merged")) is VG.options(_args(pseudoViews="merged"))
    assert VG.options(_args(pseudoViews="merged")) is not VG.options(_args(pseudoViews="other"))
    assert VG.options(_args(pseudoViews="merged")) is not VG.options(_args())
    assert VG.options(_args(pseudoViews="own")) is VG.options(_args())
    on = VG.options(_args(pseudoViews="merged"))
    vm = [torch.zeros(2, 6)] * 2
    VG.check_batch(on, {"viewmat": vm}, 2, 2)
    VG.check_batch(VG.options(_args()), {}, 1, 2)                          # off: nothing is asked
    with pytest.raises(ValueError, match='pseudoViews \'merged\' needs meta\\["viewmat"\\]'):
        VG.check_batch(on, {"kps": None}, 2, 2)
    with pytest.raises(ValueError, match="pseudoViews 'merged' merges .* at least 2"):
        VG.check_batch(on, {"viewmat": vm[:1]}, 1, 2)
    with pytest.raises(ValueError, match="at most 16 views and 8 teachers"):
        VG.check_batch(on, {"viewmat": vm * 9}, 18, 2)
    VG.refuse(_args(pseudoViews="own"), "train_mt")
    for v in ("merged", "other"):
        with pytest.raises(ValueError, match="pseudoViews %r is built into train_mt_ubpl only, not train_mt" % v):
            VG.refuse(_args(pseudoViews=v), "train_mt")


def test_wrapper_checks_raise_without_a_gpu():
    from ubpl_amd import kernels as Kn
    z = torch.zeros(4096)
    with pytest.raises(ValueError, match="1 to 16 views"):
        Kn.merge_views_samples(z, 16, 16, 16, 17, 1, 1, 1, 4, 4, z)
    with pytest.raises(ValueError, match="1 to 8 members"):
        Kn.merge_views_samples(z, 16, 16, 16, 2, 9, 1, 1, 4, 4, z)
    with pytest.raises(ValueError, match="at least 2 views"):
        Kn.merge_views_samples(z, 16, 16, 16, 1, 1, 1, 1, 4, 4, z, include_self=False)
    with pytest.raises(ValueError, match="viewmat is"):
        Kn.train_pair_matrices(torch.zeros(2, 6), R, H)


def test_header_declares_the_new_entry():
    from ubpl_amd import _abi, _lib
    decls = {name: (params, ann) for _, name, params, ann in _abi.parse(open(_lib.HEADER_PATH).read())}
    params, ann = decls["ubpl_merge_views_samples"]
    assert [p for _, p in params] == ["hm", "sv", "sm", "sb", "V", "M", "N", "K", "H", "W", "mat", "include_self",
                                      "out", "cover", "stream"]
    assert ann["hm"] == ("f32", "(V-1)*sv+(M-1)*sm+(N-1)*sb+(int64_t)K*H*W")
    assert ann["mat"] == ("f32", "(int64_t)V*V*N*6") and ann["out"] == ("f32", "(int64_t)V*M*N*K*H*W")
    assert ann["cover"] == ("f32", "(int64_t)V*N*H*W")
    assert "ubpl_merge_views_samples" in _lib.signatures()
