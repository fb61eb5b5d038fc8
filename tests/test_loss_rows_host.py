"""kernels.RowSpec on the host: every layout constructor against the stride tuples the loss code
spelt out by hand before there was a spec, and against plain torch indexing of an arange tensor —
every stride the loss kernels are handed, checked without a GPU."""
import pytest
import torch

from ubpl_amd import kernels as Kn

# (B, S, K, H, W)
SHAPES = [(3, 1, 4, 2, 2), (3, 2, 4, 2, 2), (3, 2, 4, 3, 2)]


def _flat_reads(rows):
    """[M, B, S, K] element index where the kernels start target map (b,s,k) of member m."""
    m, b, s, k = torch.meshgrid(torch.arange(rows.M), torch.arange(rows.B), torch.arange(rows.S),
                                torch.arange(rows.K), indexing="ij")
    return rows.base + m * rows.t_sm + b * rows.t_sb + s * rows.t_ss + k * rows.HW


def _check_reads(rows, t, maps):
    """maps [M,B,S,K,HW]: the target map of every row by plain indexing of t; the flat reads of
    rows must be those maps, and rows.target(t) the view the kernels' offsets are relative to."""
    assert tuple(maps.shape) == (rows.M, rows.B, rows.S, rows.K, rows.HW)
    start = _flat_reads(rows)
    got = t.reshape(-1)[start[..., None] + torch.arange(rows.HW)]
    assert torch.equal(got, maps)
    view = rows.target(t)
    assert view.data_ptr() == t.data_ptr() + 4 * rows.base and view.numel() == t.numel() - rows.base
    # (the last read ends inside the tensor)
    assert int(start.max()) + rows.HW <= t.numel()


@pytest.mark.parametrize("B,S,K,H,W", SHAPES)
def test_ground_truth_rows(B, S, K, H, W):
    HW = H * W
    rows = Kn.RowSpec.ground_truth(B, S, K, HW)
    assert rows == (B, S, K, HW, K * HW, 0, 0, 1, 0)                      # losses.py / step_losses.py: (K*HW, 0, 0, 1)
    assert (rows.a_sb, rows.a_ss, rows.t_stacks) == (S * K * HW, K * HW, 1)
    t = torch.arange(B * K * HW, dtype=torch.float32).reshape(B, K, H, W)
    _check_reads(rows, t, t.reshape(1, B, 1, K, HW).expand(1, B, S, K, HW))


@pytest.mark.parametrize("B,S,K,H,W", SHAPES)
def test_same_layout_rows(B, S, K, H, W):
    HW = H * W
    rows = Kn.RowSpec.same(B, S, K, HW)
    assert rows == (B, S, K, HW, S * K * HW, K * HW, 0, 1, 0)              # (S*K*HW, K*HW, 0, 1)
    assert rows.t_stacks == S
    t = torch.arange(B * S * K * HW, dtype=torch.float32).reshape(B, S, K, H, W)
    _check_reads(rows, t, t.reshape(1, B, S, K, HW))
    # the last stacks of both inputs, each made contiguous (step_losses._dist_last): (K*HW, K*HW, 0, 1)
    assert Kn.RowSpec.same(B, 1, K, HW)[4:] == (K * HW, K * HW, 0, 1, 0)


@pytest.mark.parametrize("B,S,K,H,W", SHAPES)
@pytest.mark.parametrize("M,St", [(2, 2), (1, 3)])
def test_ensemble_rows_read_the_last_stack(B, S, K, H, W, M, St):
    HW = H * W
    rows = Kn.RowSpec.ensemble(B, S, K, HW, M, St)
    # (St*K*HW, 0, B*St*K*HW, M, (St-1)*K*HW), spelt out three times in step_losses.py and once in losses.py
    assert rows == (B, S, K, HW, St * K * HW, 0, B * St * K * HW, M, (St - 1) * K * HW)
    assert rows.t_stacks == 1
    t = torch.arange(M * B * St * K * HW, dtype=torch.float32).reshape(M, B, St, K, H, W)
    _check_reads(rows, t, t[:, :, -1].reshape(M, B, 1, K, HW).expand(M, B, S, K, HW))


@pytest.mark.parametrize("B,S,K,H,W", SHAPES[:1])
def test_ensemble_rows_of_the_5d_form(B, S, K, H, W):
    HW, M = H * W, 2
    t = torch.arange(M * B * K * HW, dtype=torch.float32).reshape(M, B, K, H, W)
    rows = Kn.RowSpec.ensemble(B, S, K, HW, M)
    # losses.py with nStack == 1: (K*HW, 0, numel/M, M), base 0
    assert rows == (B, S, K, HW, K * HW, 0, t.numel() // M, M, 0)
    _check_reads(rows, t, t.reshape(M, B, 1, K, HW))


def test_flat_feature_rows():
    bs, n, c, H, W = 3, 2, 4, 3, 2
    HW = H * W
    rows = Kn.RowSpec.flat(bs, n * c, HW)
    assert rows == (bs, 1, n * c, HW, n * c * HW, 0, 0, 1, 0)              # (n*c*HW, 0, 0, 1) with S = 1, K = n*c
    t = torch.arange(bs * n * c * HW, dtype=torch.float32).reshape(bs, n, c, H, W)
    _check_reads(rows, t, t.reshape(1, bs, 1, n * c, HW))


def test_pred_rows_is_the_reference_reshape():
    B, K, R = 3, 4, 2
    assert Kn.pred_rows(torch.zeros(B, 2, K, R, R), 2) == (B, 2, K, R * R)
    assert Kn.pred_rows(torch.zeros(B, 2, K, 3, R), 2) == (B, 2, K, 3 * R)
    assert Kn.pred_rows(torch.zeros(B, K, R, R), 1) == (B, 1, K, R * R)
    # nStack == 1 with a [B,1,K,R,R] prediction: ONE row per sample over K*R*R pixels
    p = torch.arange(B * K * R * R, dtype=torch.float32).reshape(B, 1, K, R, R)
    dims = Kn.pred_rows(p, 1)
    assert dims == (B, 1, 1, K * R * R)
    rows = Kn.RowSpec.ground_truth(*dims)
    assert rows == (B, 1, 1, K * R * R, K * R * R, 0, 0, 1, 0)
    gts = p.reshape(B, K, R, R) + 0.5
    _check_reads(rows, gts, gts.reshape(1, B, 1, 1, K * R * R))
    # and its ensemble target [M,B,1,K,R,R] under nStack == 1: member stride numel / M
    t = torch.arange(2 * B * K * R * R, dtype=torch.float32).reshape(2, B, 1, K, R, R)
    rows = Kn.RowSpec.ensemble(*dims, 2)
    assert rows[4:] == (K * R * R, 0, t.numel() // 2, 2, 0)
    _check_reads(rows, t, t.reshape(2, B, 1, 1, K * R * R))


def test_spec_is_immutable_and_the_old_geometry_is_gone():
    rows = Kn.RowSpec.same(2, 2, 3, 4)
    with pytest.raises(AttributeError):
        rows.base = 1
    for name in ("RowGeom", "geom_stack", "geom_rows"):
        assert not hasattr(Kn, name)
