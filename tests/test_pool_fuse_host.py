"""CPU-only checks of the fused pool / upsample-add + BatchNorm path: the eligibility
predicate, and the wrappers' shape checks, which run before any library call."""
import pytest
import torch


def test_pool_fuse_ok_takes_the_headline_planes_only():
    from ubpl_amd import kernels as Kn
    for hw, c in ((128, 128), (64, 256), (32, 256), (16, 256), (8, 256)):       # HG2 256x256
        assert Kn.pool_fuse_ok(hw, hw, c), (hw, c)
    assert Kn.pool_fuse_ok(4, 4, 256) and Kn.pool_fuse_ok(8, 16, 512)
    for h, w in ((96, 96), (6, 6), (48, 48), (7, 8), (8, 7), (9, 9), (2, 2), (256, 256), (6, 8), (12, 16)):
        assert not Kn.pool_fuse_ok(h, w, 64), (h, w)
    assert not Kn.pool_fuse_ok(64, 64, 513) and not Kn.pool_fuse_ok(64, 64, 0)
    # 16-byte alignment of every tensor given
    t = torch.zeros(4 * 8 * 8 + 1)
    assert Kn.pool_fuse_ok(8, 8, 4, t[:-1], None)
    assert not Kn.pool_fuse_ok(8, 8, 4, t[:-1], t[1:])


def _bn(C):
    return tuple(torch.zeros(C) for _ in range(8))


def test_wrappers_refuse_mismatched_shapes_before_any_call(monkeypatch):
    from ubpl_amd import _lib, kernels as Kn
    from ubpl_amd.kernels import _check

    def no_call(name, *a):
        raise AssertionError("library call %s after a bad argument" % name)
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(_check, "_chk", no_call)
    B, C, H = 2, 3, 8
    x, half, part = torch.zeros(B, C, H, H), torch.zeros(B, C, H // 2, H // 2), torch.zeros(8, dtype=torch.float64)
    v = torch.zeros(C)
    with pytest.raises(ValueError, match="pool_fuse_ok"):
        Kn.bn_forward_stats_maxpool(torch.zeros(B, C, 6, 6), _bn(C), _bn(C), 1e-5, 0.1, part)
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        Kn.bn_forward_stats_maxpool(torch.zeros(C, H, H), None, _bn(C), 1e-5, 0.1, part)
    with pytest.raises(ValueError, match=r"pbn\[6\] has shape \(4,\)"):
        Kn.bn_forward_stats_maxpool(x, None, _bn(C)[:6] + (torch.zeros(C + 1), v), 1e-5, 0.1, part)
    with pytest.raises(ValueError, match=r"xbn\[0\] has shape"):
        Kn.bn_forward_stats_maxpool(x, (torch.zeros(C - 1),) + _bn(C)[1:], _bn(C), 1e-5, 0.1, part)
    with pytest.raises(ValueError, match="pbn is"):
        Kn.bn_forward_stats_maxpool(x, None, _bn(C)[:7], 1e-5, 0.1, part)
    with pytest.raises(ValueError, match="out has shape"):
        Kn.bn_forward_stats_maxpool(x, None, _bn(C), 1e-5, 0.1, part, out=x)
    with pytest.raises(ValueError, match="low has shape"):
        Kn.upsample2x_add_bnstats(x, x, _bn(C), 1e-5, 0.1, part)
    with pytest.raises(ValueError, match="out has shape"):
        Kn.upsample2x_add_bnstats(x, half, _bn(C), 1e-5, 0.1, part, out=half)
    with pytest.raises(ValueError, match="bn is"):
        Kn.upsample2x_add_bnstats(x, half, _bn(C)[:7], 1e-5, 0.1, part)
    with pytest.raises(ValueError, match="pool_fuse_ok"):
        Kn.upsample2x_add_bnstats(torch.zeros(B, C, 96, 96), torch.zeros(B, C, 48, 48), _bn(C), 1e-5, 0.1, part)
    args = (v, v, v, v, v, 1, part, torch.zeros(3 * C), v, v)
    with pytest.raises(ValueError, match="pool_dy has shape"):
        Kn.bn_backward_pool(x, x, *args, pool_dy=x)
    with pytest.raises(ValueError, match="add2 has shape"):
        Kn.bn_backward_pool(x, x, *args, pool_dy=half, add2=half)
    with pytest.raises(ValueError, match="dz has shape"):
        Kn.bn_backward_pool(half, x, *args, pool_dy=half)
    with pytest.raises(ValueError, match="pool_fuse_ok"):
        Kn.bn_backward_pool(torch.zeros(B, C, 6, 8), torch.zeros(B, C, 6, 8), *args, pool_dy=torch.zeros(B, C, 3, 4))


def test_ops_check_extents_before_the_call():
    """The three new torch ops bound every pointer from the sizes passed beside it."""
    import os
    from ubpl_amd import _lib
    if not os.path.exists(_lib.OPS_PATH):
        pytest.skip("libubpl_ops.so not built (run __graft_entry__.build())")
    ops = _lib.load_ops()
    B, C, H, W = 2, 3, 8, 8
    x, half = torch.zeros(B * C * H * W), torch.zeros(B * C * H * W // 4)
    v = torch.zeros(C)
    part = torch.zeros(int(_lib.lib().ubpl_bn_part_doubles(B, C)), dtype=torch.float64)
    bn = (v,) * 8
    with pytest.raises(RuntimeError, match="y holds %d elements" % (half.numel() - 1)):
        ops.bn_forward_stats_maxpool(x, B, C, H, W, half[1:], *bn, *bn, 1e-5, 0.1, part)
    with pytest.raises(RuntimeError, match="pshift holds 2 elements"):
        ops.bn_forward_stats_maxpool(x, B, C, H, W, half, *bn, *(bn[:7] + (v[1:],)), 1e-5, 0.1, part)
    with pytest.raises(RuntimeError, match="part must be f64"):
        ops.bn_forward_stats_maxpool(x, B, C, H, W, half, *bn, *bn, 1e-5, 0.1, part.float())
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        ops.bn_forward_stats_maxpool(x, B, C, H, W, half, *((None,) * 8), *bn, 1e-5, 0.1, part)
    with pytest.raises(RuntimeError, match="low holds %d elements" % (half.numel() - 1)):
        ops.upsample2x_add_forward_bnstats(x, half[1:], B, C, H, W, x, v, v, 1e-5, 0.1, v, v, part, v, v, v, v)
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        ops.upsample2x_add_forward_bnstats(x, half, B, C, H, W, x, v, v, 1e-5, 0.1, v, v, part, v, v, v, v)
    coef = torch.zeros(3 * C)
    with pytest.raises(RuntimeError, match="pool_dy holds %d elements" % (half.numel() - 1)):
        ops.bn_backward_pool(x, x, B, C, H, W, v, v, v, v, v, 1, part, None, coef, v, v, None, half[1:], None, x)
    with pytest.raises(RuntimeError, match="expected a device tensor"):
        ops.bn_backward_pool(x, x, B, C, H, W, v, v, v, v, v, 1, part, None, coef, v, v, None, half, None, x)
