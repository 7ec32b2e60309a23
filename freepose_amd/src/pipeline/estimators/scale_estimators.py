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


class GPT4ScaleEstimator:
    """reference scale_estimators.py:35-80: CLIP embedding of each proposal crop -> the `query_k` nearest text embeddings of a table of
    object names with LLM-given sizes -> median of their sizes -> optionally rescaled so that the median ratio to the depth-map scales
    of the same image is 1 -> / 2.  The embeddings (one tower call for all crops of the image: a crop's embedding does not depend on
    its batch), the nearest rows (ops.knn_l2, the brute-force form of the reference's KDTree query; exact ties in index order) and the
    depth-map scales run on the device; the medians are float64 on the host like the reference's.  The text embeddings are read from
    `feats_path`, or with `scale_file` computed by the extractor's text tower first (generate_clip_features, which also writes them to
    `feats_path`); an extractor without a text tower refuses `scale_file`."""

    def __init__(self, clip, query_k=11, scale_file=None, feats_path="data/scale_feats.pt", svd=True) -> None:
        import torch
        self.clip = clip
        self.query_k = query_k
        self.svd = svd
        if scale_file is not None:
            gpt_feats_scales = self.generate_clip_features(scale_file, clip, feats_path=feats_path)
        else:
            gpt_feats_scales = torch.load(feats_path, map_location="cpu")
        self.text_features = torch.as_tensor(gpt_feats_scales["feats"]).float().contiguous()
        self.scales = torch.as_tensor(gpt_feats_scales["scales"])
        self._table = self.text_features.cuda()

    def embed(self, proposals):
        """normalised float32 CLIP embeddings [n, E] of the proposal crops (reference :59-64: bf16 forward, bf16 division by the bf16
        norm, then float)"""
        import torch
        crops = torch.stack([torch.as_tensor(p) for p in proposals.proposals]).to("cuda", dtype=torch.bfloat16)
        feats = self.clip(crops)
        with torch.inference_mode():
            feats = feats / feats.norm(dim=-1, keepdim=True)
        return feats.float()

    def neighbours(self, image_features):
        from freepose_amd import ops
        idx, _ = ops.knn_l2(self._table, image_features, self.query_k)
        return idx.cpu().numpy().astype(np.int64)

    def estimate(self, proposals, depth_image=None, K=None):
        import torch
        assert (depth_image is None) == (K is None)
        use_depth = depth_image is not None and len(proposals.masks) > 1
        if use_depth:
            masks = torch.stack([torch.as_tensor(mask) for mask in proposals.masks])
            depth_scales = depthmap_scales(depth_image, K, masks, svd=self.svd)
        idx = self.neighbours(self.embed(proposals))
        if self.query_k == 1:
            chatgpt_scales = self.scales[idx[:, 0]].numpy()
        else:
            # torch's median of k values: the lower of the middle two for even k
            chatgpt_scales = self.scales[idx.reshape(-1)].reshape(idx.shape).median(axis=1).values
        if use_depth:
            correction = np.median(np.asarray(chatgpt_scales) / depth_scales)
            scales = depth_scales * correction
        else:
            scales = chatgpt_scales
        return scales / 2.0

    @staticmethod
    def generate_clip_features(scale_file, clip, feats_path="data/scale_feats.pt"):
        """reference :83-102: the names and sizes of `scale_file` (JSON object, in file order) -> tokenizer -> text tower -> each
        embedding divided by its norm -> {"feats": float32 [N, E] on the CPU, "scales": float32 [N]}, saved to `feats_path` unless it
        is None.  The reference runs the tower under fp16 autocast on a bf16 module; here it is the bf16 module regime of the image
        side: bf16 forward, bf16 division by the bf16 norm (what `embed` does), then float."""
        import json
        import torch
        if clip is None or not getattr(clip, "has_text_tower", False):
            raise NotImplementedError("generate_clip_features needs a CLIP text tower: the extractor's weights hold no text tensors "
                                      "(or no extractor was given); compute the scale table's embeddings elsewhere and pass feats_path")
        with open(scale_file) as f:
            gpt_scales = list(json.load(f).items())
        object_names = [x[0] for x in gpt_scales]
        scales = [x[1] for x in gpt_scales]
        text = clip.tokenizer(object_names)
        with torch.inference_mode():
            text_features = clip.model.encode_text(text)
            text_features = text_features / text_features.norm(dim=-1, keepdim=True)
        feats_scales = {"feats": text_features.float().cpu(), "scales": torch.Tensor(scales)}
        if feats_path is not None:
            torch.save(feats_scales, feats_path)
        return feats_scales

    @staticmethod
    def mask_to_bbox(mask):
        import torch
        if isinstance(mask, torch.Tensor):
            mask = mask.numpy()
        rows = np.any(mask, axis=1)
        cols = np.any(mask, axis=0)
        rmin, rmax = np.where(rows)[0][[0, -1]]
        cmin, cmax = np.where(cols)[0][[0, -1]]
        return rmin, rmax, cmin, cmax
