"""Predictor from raw frames, end to end, on 8 Mouse validation images from the pack: the
device crop at the image centre and scale 256 / 200 is mouse.to_device_images bit for bit (every
weight of the crop is then exactly 1 or 0), so predict_frames / pseudo_label_frames / validate
over FrameBank.batches return what the existing paths return on the same images; pasted into
larger zero frames at an offset, the crops stay bit-equal and the predictions come back shifted
by exactly that offset.  The smallest network of the Predictor tests (K = 9, one stack) at the
Mouse images' own 256 x 256."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, R = 8, 256


@pytest.fixture(scope="module")
def mouse8():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ubpl_amd import _lib, mouse
    from ubpl_amd.frames import FrameBank
    from ubpl_amd.hourglass import StackedHourglass
    _lib.load()
    data = mouse.MouseData.from_pack()
    means = data.getSemiData(100, 500, 0.3)[6]
    imgs = np.ascontiguousarray(data.images("valid")[:N])
    batch = mouse.valid_batches(data, N, DEV)[:1]
    models = []
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = StackedHourglass(data.kpsCount, 1, "AvgPool")
        with torch.no_grad():
            for _ in range(2):                       # running statistics off their initial values
                m(batch[0][0][:4])
        models.append(m)
    return types.SimpleNamespace(data=data, means=means, imgs=imgs, batch=batch, models=models,
                                 bank=FrameBank(imgs, means, DEV), center=batch[0][2]["center"],
                                 scale=batch[0][2]["scale"])


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k] or (a[k] is None and b[k] is None), k


def test_identity_crop_is_to_device_images(mouse8):
    from ubpl_amd import Predictor, mouse
    x = mouse.to_device_images(mouse8.imgs, mouse8.means, DEV)
    assert torch.equal(x, mouse8.batch[0][0])
    got = mouse8.bank.crop(None, mouse8.center, mouse8.scale, R)
    assert got.shape == x.shape and torch.equal(got, x)
    P = Predictor(mouse8.models[0])
    _same(P.predict_frames(mouse8.bank, mouse8.center, mouse8.scale, R, return_heatmaps=True),
          P.predict(x, mouse8.center, mouse8.scale, return_heatmaps=True))
    # several boxes of one frame, in another order, through the frame index
    order = [5, 0, 5, 7]
    _same(P.predict_frames(mouse8.bank, mouse8.center[order], mouse8.scale[order], R, frame=order),
          P.predict(x[order], mouse8.center[order], mouse8.scale[order]))
    P.release()


def test_every_byte_value_scales_as_in_to_device_images(mouse8):
    """The crop's u8 -> [0, 1] is v * (1/255.f) because to_device_images' `.float().div_(255.)` on
    the device is that product, not the correctly rounded quotient v / 255.f: a 16 x 16 frame
    holding all 256 byte values, cropped as itself, is to_device_images bit for bit.  The counts
    behind that choice are printed (the GPU test log keeps them)."""
    from ubpl_amd import mouse
    from ubpl_amd.frames import FrameBank
    v = np.arange(256, dtype=np.uint8)
    frame = np.stack([v, np.roll(v, 85), v[::-1]], -1).reshape(16, 16, 3)
    got = FrameBank([frame], mouse8.means, DEV).crop(None, [(8, 8)], [16 / 200.0], 16)
    assert torch.equal(got, mouse.to_device_images(frame[None], mouse8.means, DEV))
    dev_div = torch.from_numpy(v).to(DEV).float().div_(255.).cpu().numpy()
    product = v.astype(np.float32) * (np.float32(1) / np.float32(255))
    quotient = v.astype(np.float32) / np.float32(255)
    print("of 256 byte values, div_(255.) on the device differs from v * (1/255.f) for %d and from the correctly "
          "rounded v / 255.f for %d; the product and the quotient differ for %d"
          % ((dev_div != product).sum(), (dev_div != quotient).sum(), (product != quotient).sum()))


def test_padded_frames_shift_the_predictions_by_the_offset(mouse8):
    from ubpl_amd import Predictor
    from ubpl_amd.frames import FrameBank
    rs = np.random.RandomState(4)
    frames, offs = [], []
    for i in range(N):                               # mixed sizes: a ragged bank
        dx, dy = int(rs.randint(0, 90)), int(rs.randint(0, 70))
        f = np.zeros((R + dy + int(rs.randint(0, 60)), R + dx + int(rs.randint(0, 60)), 3), np.uint8)
        f[dy:dy + R, dx:dx + R] = mouse8.imgs[i]
        frames.append(f)
        offs.append((dx, dy))
    assert len({f.shape for f in frames}) > 1
    off = torch.tensor(offs, dtype=torch.int64)
    bank = FrameBank(frames, mouse8.means, DEV)
    assert torch.equal(bank.crop(None, mouse8.center + off, mouse8.scale, R), mouse8.batch[0][0])
    P = Predictor(mouse8.models[0])
    a = P.predict_frames(bank, mouse8.center + off, mouse8.scale, R)
    b = P.predict(mouse8.batch[0][0], mouse8.center, mouse8.scale)
    assert torch.equal(a["raw"], b["raw"]) and torch.equal(a["scores"], b["scores"])
    assert torch.equal(a["preds"], b["preds"] + off.to(DEV).view(1, N, 1, 2).to(b["preds"].dtype))
    assert torch.equal(a["preds_mean"], b["preds_mean"] + off.to(DEV).view(N, 1, 2).to(b["preds_mean"].dtype))
    P.release()


def test_validate_over_frame_batches(mouse8):
    from ubpl_amd import Predictor
    args = types.SimpleNamespace(outRes=64, pck_ref=mouse8.data.pck_ref, pck_thr=mouse8.data.pck_thr)
    P = Predictor(mouse8.models)
    kps = mouse8.batch[0][2]["kpsMap"]
    got = P.validate(mouse8.bank.batches(mouse8.center, mouse8.scale, R, N, kps=kps), args)
    assert got == P.validate(mouse8.batch, args)
    parts = list(mouse8.bank.batches(mouse8.center, mouse8.scale, R, 3, kps=kps))
    assert [p[0].shape[0] for p in parts] == [3, 3, 2] and [p[2]["batch_index"] for p in parts] == [0, 1, 2]
    assert torch.equal(torch.cat([p[0] for p in parts]), mouse8.batch[0][0])
    first = next(mouse8.bank.batches(mouse8.center, mouse8.scale, R, N, kps=kps))
    assert first[1] is None and set(first[2]) == set(mouse8.batch[0][2])
    for k, v in mouse8.batch[0][2].items():
        assert (torch.equal(first[2][k], v) and first[2][k].dtype == v.dtype) if torch.is_tensor(v) else first[2][k] == v
    pool_a = P.label_pool(mouse8.bank.batches(mouse8.center, mouse8.scale, R, N), args, thr=0.0)
    pool_b = P.label_pool(mouse8.batch, args, thr=0.0)
    assert pool_a == pool_b
    P.release()


def test_pseudo_label_frames_with_tta_and_taylor(mouse8):
    from ubpl_amd import Predictor, mouse
    x = mouse.to_device_images(mouse8.imgs, mouse8.means, DEV)
    P = Predictor(mouse8.models, tta=[(0, 1), (0, 0.85), (10, 1)], refine="taylor")
    _same(P.pseudo_label_frames(mouse8.bank, mouse8.center, mouse8.scale, R, thr=0.0, return_heatmaps=True),
          P.pseudo_label(x, mouse8.center, mouse8.scale, thr=0.0, return_heatmaps=True))
    P.release()


def test_mismatched_boxes_are_refused_before_any_launch(mouse8):
    from ubpl_amd import Predictor
    P = Predictor(mouse8.models[0])
    with pytest.raises(ValueError, match="do not describe one set"):
        P.predict_frames(mouse8.bank, mouse8.center, mouse8.scale[:3], R)
    with pytest.raises(ValueError, match="frame index"):
        P.predict_frames(mouse8.bank, mouse8.center[:1], mouse8.scale[:1], R, frame=[N])
    P.release()
