"""Inputs shared by tests/test_gpu_pose_kernels.py and tests/test_crop_vs_torch_cpu.py: one small odd-sized image geometry and a box
set that reaches every geometric branch of CropResizePad (square / wide / tall crops, both paddings, clipping at the borders, an
extension that crosses a border).  Every box resizes to every target both files use, with bbox_extend 0 and 0.2 — the tests assert it."""
import numpy as np

H, W = 47, 61          # both odd, H != W
EXTS = (0.0, 0.2)

BOXES = np.array([
    [0, 0, W, H],          # the whole image (wide: pad_t > 0)
    [10, 8, 40, 38],       # square, 30 x 30
    [3, 15, 57, 30],       # wide: pad_t > 0, pad_l == 0
    [20, 2, 33, 45],       # tall: pad_l > 0, pad_t == 0
    [45, 30, 80, 70],      # clipped by the right and the bottom border
    [-5, -4, 20, 18],      # clipped by the left and the top border
    [2, 3, 30, 25],        # inside the image; its 0.2 extension crosses the left and the top border
    [30, 20, 37, 26],      # 7 x 6: magnified at every target
], dtype=np.int32)


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def float_image(seed=7):
    """f32 [1,3,H,W], every value distinct enough that a wrong source pixel shows"""
    return rng(seed).random((1, 3, H, W)).astype(np.float32)


def u8_images(n_img, C, seed):
    """u8 [n_img,H,W,C]; every image holds all 256 byte values (a shuffled ramp, not a draw that merely makes it likely)"""
    g = rng(seed)
    out = np.empty((n_img, H, W, C), dtype=np.uint8)
    for i in range(n_img):
        ramp = (np.arange(H * W * C) % 256).astype(np.uint8)
        g.shuffle(ramp)
        out[i] = ramp.reshape(H, W, C)
        assert len(np.unique(out[i])) == 256
    return out


def masks(n, seed=11):
    """u8 [n,H,W], about 70 % set, one per box"""
    return (rng(seed).random((n, H, W)) < 0.7).astype(np.uint8)
