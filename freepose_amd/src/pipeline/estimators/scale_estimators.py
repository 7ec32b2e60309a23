"""`--depth_method depthmap` of scripts/dino_inference.py (reference :82-85): object scale from the scene's depth map.

Host-side numpy, upstream of the GPU hot path (SURVEY §2 row 14 lists the scale estimators as out of scope; this one function is
here because it is a flag of the a12 CLI).  Restates src/pipeline/estimators/scale_estimators.py:117-187 of the reference:

  largest connected component of the proposal mask -> isotropic erosion (radius 8, halved until more than `min_vertices` pixels
  survive; the un-eroded component once the radius drops below 1) -> depth samples ordered by |z - median z|, cut at the first one
  farther than `std_factor` standard deviations (never fewer than `min_vertices`; NOTE the reference's quirk: when NO sample is that
  far, numpy's argmax of an all-False array is 0, so only `min_vertices` samples are kept) -> back-projection with the pinhole
  intrinsics -> rotation into the principal axes (right singular vectors of X^T X) -> half of the largest axis-aligned extent.

Connected components: the reference's `extract_largest_component` (src/pipeline/utils.py:8,71-84) labels with
`scipy.ndimage.label(mask)` — default structure, i.e. 4-connectivity: parts that touch only diagonally stay separate — and this module
makes exactly that call (scipy is in the image).  skimage is not, so its two calls are restated from their published definitions:
`skimage.measure.regionprops(...).area` -> pixel counts per label (first maximum wins, like Python's max over regionprops in label
order); `skimage.morphology.isotropic_erosion(mask, r)` -> `distance_transform_edt(mask) > r`.  PARITY UNPINNED for those two (DESIGN
§5); the arithmetic after them is plain numpy on both sides.
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage


def largest_component(mask: np.ndarray) -> np.ndarray:
    """reference src/pipeline/utils.py:71-84: scipy.ndimage.label with its default (4-connected) structure + the largest regionprops area"""
    lab, n = ndimage.label(np.asarray(mask).astype(bool))
    if n == 0:
        raise ValueError("depthmap scale: empty proposal mask")
    area = np.bincount(lab.ravel())[1:]
    return lab == (int(np.argmax(area)) + 1)


def eroded(mask: np.ndarray, radius: float) -> np.ndarray:
    return ndimage.distance_transform_edt(mask) > radius


def pointcloud_from_depth(depth, K, mask, erosion_radius=8, std_factor=1.5, min_vertices=25, align=True) -> np.ndarray:
    """reference scale_estimators.py:132-187 (`generate_pointcloud(..., svd=True)`) -> [n, 3] points"""
    comp = largest_component(mask)
    radius = float(erosion_radius)
    keep = eroded(comp, radius)
    while int(keep.sum()) <= min_vertices:
        if radius < 1:
            keep = comp
            break
        radius /= 2
        keep = eroded(comp, radius)
    rows, cols = np.nonzero(keep)
    z = np.asarray(depth)[rows, cols]
    far = np.abs(z - np.median(z))
    order = np.argsort(far)
    far, z = far[order], z[order]
    n = max(int(np.argmax(far > np.std(z) * std_factor)), min_vertices)      # (argmax of all-False is 0: the quirk in the docstring)
    z, cols, rows = z[:n], cols[order][:n], rows[order][:n]
    K = np.asarray(K, dtype=np.float64)
    pts = np.column_stack(((cols - K[0, 2]) * z / K[0, 0], (rows - K[1, 2]) * z / K[1, 1], z)).reshape(-1, 3)
    if align:
        centred = pts - pts.mean(axis=0)
        _, _, vh = np.linalg.svd(centred.T @ centred)
        pts = pts @ vh.T
    return pts


def extent_scale(points: np.ndarray) -> float:
    """reference :117-122: half of the largest axis-aligned extent"""
    span = points.max(axis=0) - points.min(axis=0)
    return float(max(max(float(span[0]), float(span[1])), float(span[2])) / 2.0)


def depthmap_scale(depth, K, mask) -> float:
    """what dino_inference.py:83-84 computes per proposal"""
    return extent_scale(pointcloud_from_depth(depth, K, mask, align=True))


def depthmap_scales(depth, K, masks, svd: bool = True) -> np.ndarray:
    """depthmap_scale for all proposal masks [n,H,W] of one image in ONE device call (freepose_amd.ops.depthmap_scales: connected
    components, erosion chain, robust cut and extent as HIP kernels) -> float64 [n].  Same discrete decisions as the host function;
    where ties in |z - median| straddle the cut the device takes them in raster order, the host in whatever order numpy's unstable
    argsort leaves them (DESIGN "Depth-map scale")."""
    import torch
    from freepose_amd import ops
    m = masks if isinstance(masks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(masks)).astype(np.uint8))
    if m.dim() == 2:
        m = m[None]
    if m.shape[0] == 0:
        return np.zeros((0,), dtype=np.float64)
    d = depth if isinstance(depth, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(depth, dtype=np.float64)))
    scales, _ = ops.depthmap_scales(d, m, K, align=svd)
    return scales.cpu().numpy()


class ConstantScaleEstimator:
    """reference scale_estimators.py:12-17"""

    def __init__(self, const) -> None:
        self.const = const

    def estimate(self, proposals, depth_image=None, K=None):
        return self.const


class MeanScaleEstimator:
    """reference scale_estimators.py:20-32: depth-map scales of all proposals, rescaled so that their mean diameter is `mean_scale`.
    The per-mask scales come from one device call."""

    def __init__(self, mean_scale, svd=True):
        self.mean_scale = mean_scale
        self.svd = svd

    def estimate(self, proposals, depth_image, K):
        import torch
        masks = torch.stack([torch.as_tensor(mask) for mask in proposals.masks])
        scales = depthmap_scales(depth_image, K, masks, svd=self.svd)
        correction = self.mean_scale / (2 * np.mean(scales))
        scales *= correction
        return scales
