"""The oracle's crop rule against torch's own nearest interpolation (CPU only, no GPU code is built or loaded).

fo.crop_resize_pad restates CropResizePad in C, including torch's nearest-neighbour source index (csrc/pose.hip header and
nearest_src): clip the (extended) box, F.interpolate(scale_factor = target / longest side), centre-pad to a square unless the crop is
already one, F.interpolate(scale_factor = target / side) again.  The goldens pin that restatement at 30, 42, 56 and 420 px only.  Here
the chain is written with torch.nn.functional on CPU tensors and compared bit for bit at targets on both sides of ATen's small-size
kernel switch (out_h + out_w <= 128) and at odd sizes.

The index rule was probed on torch 2.10 (oracle/fp_oracle.c); the version this test ran with is reported on failure.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _crop_cases as cc

TARGETS = (31, 32, 63, 64, 65, 98, 129)


def _torch_crop_resize_pad(image: torch.Tensor, boxes: torch.Tensor, target: int, ext) -> torch.Tensor:
    """image f32 [3,H,W] shared by all boxes, boxes int [n,4] xyxy -> f32 [n,3,target,target].  `ext` is the Python number the caller
    configured: an int 0 keeps the box arithmetic in integers, a float moves it to float32 tensors whose assignment back into the
    integer box tensor truncates (the call order of src/utils/bbox_utils.py)."""
    h, w = image.shape[-2:]
    boxes = boxes.clone()
    for b in boxes:                                     # rows are views: the assignments write through
        bw, bh = b[2] - b[0], b[3] - b[1]
        b[0] = max(0, b[0] - ext * bw)
        b[2] = min(w, b[2] + ext * bw)
        b[1] = max(0, b[1] - ext * bh)
        b[3] = min(h, b[3] + ext * bh)
    longest = (boxes[:, 2:] - boxes[:, :2]).max(dim=-1).values
    scales = target / longest                           # float32 tensor: reciprocal * scalar
    out = []
    for b, s in zip(boxes, scales):
        crop = image[:, b[1]:b[3], b[0]:b[2]]
        crop = F.interpolate(crop[None], scale_factor=s.item())[0]          # default mode: nearest
        ch, cw = crop.shape[1:]
        if cw / ch != 1.0:
            top, left = max((target - ch) // 2, 0), max((target - cw) // 2, 0)
            crop = F.pad(crop, (left, target - cw - left, top, target - ch - top))
        assert crop.shape[1] == crop.shape[2]
        out.append(F.interpolate(crop[None], scale_factor=target / crop.shape[1])[0])
    return torch.stack(out)


@pytest.fixture(scope="module")
def image():
    return cc.float_image()


@pytest.mark.parametrize("ext", [0, 0.2])
@pytest.mark.parametrize("target", TARGETS)
def test_oracle_crop_equals_torch_nearest_chain(image, target, ext):
    from oracle import fp_oracle as fo
    want = _torch_crop_resize_pad(torch.from_numpy(image[0]), torch.from_numpy(cc.BOXES.astype(np.int64)), target, ext)
    got = fo.crop_resize_pad(image, cc.BOXES, target, float(ext))           # raises if a box does not resize: none may
    assert want.shape == got.shape == (len(cc.BOXES), 3, target, target)
    diff = np.flatnonzero([not np.array_equal(got[i].view(np.uint32), want[i].numpy().view(np.uint32)) for i in range(len(cc.BOXES))])
    assert len(diff) == 0, f"oracle and torch {torch.__version__} differ at target {target}, ext {ext}, boxes {diff.tolist()}"


def test_box_set_reaches_both_paddings():
    """mask mode 2 with an all-ones mask gives 1 inside the resized crop and 0 in the padding: the square box has none, the wide box
    is padded above and below, the tall box left and right"""
    from oracle import fp_oracle as fo
    n = len(cc.BOXES)
    for ext in cc.EXTS:
        inside = fo.crop_resize_pad(cc.float_image(), cc.BOXES, 64, ext, np.ones((n, cc.H, cc.W), np.uint8), 2)[:, 0] > 0
        pad_rows, pad_cols = (~inside.any(axis=2)).sum(axis=1), (~inside.any(axis=1)).sum(axis=1)
        if ext == 0.0:
            assert pad_rows[1] == 0 and pad_cols[1] == 0                                           # square
        # wide, tall (the long side may come out one pixel short of the target: floor(side * float32(1/side * target)))
        assert pad_rows[2] > 1 >= pad_cols[2] and pad_cols[3] > 1 >= pad_rows[3]
        assert pad_rows[0] > 0 and inside.any(axis=(1, 2)).all()                                   # whole image; no empty crop


def test_u8_conversions_agree_on_every_byte():
    """u8 pixels become float(double(b) / 255.0) on the render path and float(b) / 255.f on the detection path (u8_float_div).  The two
    are the same float for all 256 bytes, in numpy and in the oracle — which is why the GPU tests cannot tell the two conversions
    apart by value and make no such assertion."""
    from oracle import fp_oracle as fo
    b = np.arange(256, dtype=np.uint8)
    via_double = (b.astype(np.float64) / 255.0).astype(np.float32)
    via_float = b.astype(np.float32) / np.float32(255.0)
    assert np.array_equal(via_double.view(np.uint32), via_float.view(np.uint32))
    ramp = b.reshape(1, 16, 16, 1)
    box = np.array([[0, 0, 16, 16]], np.int32)
    o1, o2 = fo.crop_resize_pad(ramp, box, 16, 0.0), fo.crop_resize_pad(ramp, box, 16, 0.0, u8_float_div=True)
    assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32)) and np.array_equal(o1.reshape(-1).view(np.uint32), via_double.view(np.uint32))


def test_targets_straddle_the_small_kernel_switch():
    """the rule has two regimes (nearest_src): every target <= 64 resizes with out_h + out_w <= 128, every larger one does not"""
    assert max(t for t in TARGETS if 2 * t <= 128) == 64 and min(t for t in TARGETS if 2 * t > 128) == 65
