"""tests/golden/refiner_track.npz: the host arithmetic of the tracking half of TrackingRefiner and of the trajectory smoothing, computed by
the REFERENCE's own functions (build container only: it imports the reference checkout through oracle.gen_golden's shims).  Arrays only.

    python -m tools.gen_golden_refiner_track

  - `_compute_3d_points` (tracking_refiner.py:102-130) with a stub mesh whose `sample` returns the recorded [10000,3] array: 3 poses, the
    query cells of each (occupied cells plus two empty ones), the returned points.
  - `get_query_frames` (:195-205) on 3 inlier vectors.
  - `smooth_transforms`, `average_quaternions`, `moving_average` (refiner_utils.py:173-221) on a 30-pose trajectory that turns through more
    than a full revolution (the quaternions of neighbouring poses change sign on the way) and on explicit quaternion / vector sets.
  - the cell -> pixel mapping of `compute_2d3d_correspondences` (:132-158) with `_crop_image`, `_render` and `cv2.resize` replaced by
    recorders returning prepared masks: with a proposal mask, without one, and with a mask that leaves fewer than 4 cells (the fallback).
"""
from __future__ import annotations

import sys
import types

import numpy as np
import torch

from oracle.gen_golden import OUT, REF, install_shims


def rodrigues(axis, angle):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


class StubMesh:
    def __init__(self, vertices, samples):
        self.vertices, self._samples = vertices, samples

    def sample(self, n):
        assert n == 10000
        return self._samples

    def copy(self):
        return StubMesh(self.vertices.copy(), self._samples)


def main():
    assert REF.exists(), "the reference checkout is only present in the build container"
    install_shims()
    for name in ("open3d",):
        sys.modules[name] = types.ModuleType(name)
    tv = sys.modules["torchvision"]
    tv.transforms.ToTensor = tv.transforms.Compose = type("Unused", (), {"__init__": lambda self, *a, **kw: None})   # import-time names only
    tv.ops = types.ModuleType("torchvision.ops")
    tv.ops.roi_align = None
    sys.modules["torchvision.ops"] = tv.ops
    cv2 = sys.modules["cv2"]
    cv2.INTER_CUBIC = 2

    from src.pipeline import refiner_utils
    from src.pipeline.estimators.tracking_refiner import TrackingRefiner

    rng = np.random.Generator(np.random.PCG64(2024))
    tr = TrackingRefiner.__new__(TrackingRefiner)
    tr.patch_size, tr.image_size, tr.feats_size = 14, 518, 37
    out = {}

    # ---- _compute_3d_points --------------------------------------------------------------------------------------------------------------
    d = rng.standard_normal((10000, 3))
    samples = d / np.linalg.norm(d, axis=1, keepdims=True) * np.array([0.09, 0.05, 0.12])      # an ellipsoid's surface
    mesh = StubMesh(samples[:500].copy(), samples)
    K = np.array([[2100.0, 0, 259.0], [0, 2100.0, 259.0], [0, 0, 1]])
    out["samples"], out["p3d_K"] = samples, K
    for i, (ang, tz) in enumerate(((0.4, 0.9), (1.9, 1.1), (2.7, 0.75))):
        T = np.eye(4)
        T[:3, :3] = rodrigues(rng.standard_normal(3), ang)
        T[:3, 3] = [rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), tz]
        cam = samples @ T[:3, :3].T + T[:3, 3]
        uv = (cam @ K.T)[:, :2] / (cam @ K.T)[:, 2:]
        cells = np.unique(np.floor(uv / 14).astype(np.int32), axis=0)
        cells = np.concatenate([cells, np.array([[-40, 3], [90, 90]], np.int32)])               # two cells nothing projects into
        cells = cells[rng.permutation(len(cells))]
        out[f"p3d_T{i}"], out[f"p3d_cells{i}"] = T, cells
        out[f"p3d_points{i}"] = tr._compute_3d_points(mesh, cells, K, T)

    # ---- get_query_frames ----------------------------------------------------------------------------------------------------------------
    for i, n in enumerate((48, 100, 33)):
        v = rng.integers(1, 400, n)
        out[f"gqf_in{i}"], out[f"gqf_out{i}"] = v, np.asarray(tr.get_query_frames(v.copy()))

    # ---- smoothing -----------------------------------------------------------------------------------------------------------------------
    axis = np.array([0.3, -0.5, 0.8])
    T30 = np.tile(np.eye(4), (30, 1, 1))
    for i in range(30):
        T30[i, :3, :3] = rodrigues(axis + 0.02 * rng.standard_normal(3), 0.2 + i * (7.5 / 29)) @ rodrigues(rng.standard_normal(3), 0.03)
        T30[i, :3, 3] = [0.1 * np.sin(i / 5), 0.05 * np.cos(i / 7), 0.8 + 0.01 * i] + 0.004 * rng.standard_normal(3)
    out["smooth_in"], out["smooth_out"] = T30, refiner_utils.smooth_transforms(T30)
    q = rng.standard_normal((9, 4)) * 0.1 + np.array([0.1, 0.2, -0.3, 0.9])
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    q[[1, 4, 5]] *= -1                                                                           # the same rotations, other sign
    out["avgq_in"], out["avgq_out"] = q, refiner_utils.average_quaternions(q)
    vec = rng.standard_normal((11, 3))
    out["mavg_in"] = vec
    out["mavg_out5"] = refiner_utils.moving_average(vec, window_size=5, fun=lambda a: np.mean(a, axis=0))
    out["mavg_out9"] = refiner_utils.smooth_3dvec(vec, window_size=9)
    out["smoothq_out"] = refiner_utils.smooth_quaternions(q, window_size=5)

    # ---- cell -> pixel mapping of compute_2d3d_correspondences -------------------------------------------------------------------------------
    yy, xx = np.mgrid[:37, :37]
    render37 = (((xx - 18) / 13.0) ** 2 + ((yy - 17) / 9.0) ** 2 < 1).astype(np.float32)        # what cv2.resize returns for the render
    mask_half = (render37 * (xx > 15)).astype(np.float32)
    mask_tiny = np.zeros((37, 37), np.float32)
    mask_tiny[17, 18] = mask_tiny[17, 19] = 1
    T = out["p3d_T0"]
    bbox = torch.tensor([101.25, 60.5, 417.0, 388.75])
    new_K = torch.from_numpy(K).float()
    state = {}
    tr._crop_image = lambda mesh, image, K, transform: (torch.zeros(1, 518, 518), bbox, new_K)
    tr._render = lambda mesh, w, h, K, transform: (None, np.ones((518, 518), np.float32))
    cv2.resize = lambda img, size, interpolation=None: state["queue"].pop(0)
    for name, m37 in (("masked", mask_half), ("unmasked", None), ("fallback", mask_tiny)):
        state["queue"] = [render37] if m37 is None else [m37, render37]
        q2d, p3d = tr.compute_2d3d_correspondences(mesh, None, K, T, mask=None if m37 is None else np.ones((4, 4)))
        assert not state["queue"]
        out[f"map_{name}_query"], out[f"map_{name}_points"] = q2d, p3d
    out["map_render37"], out["map_mask_half"], out["map_mask_tiny"] = render37, mask_half, mask_tiny
    out["map_bbox"], out["map_new_K"] = bbox.numpy(), new_K.numpy()

    np.savez_compressed(OUT / "refiner_track.npz", **out)
    print("wrote", OUT / "refiner_track.npz", {k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
