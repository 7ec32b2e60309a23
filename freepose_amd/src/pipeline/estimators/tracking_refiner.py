"""Drop-in for the reference's `src/pipeline/estimators/tracking_refiner.py`.

GPU-bound half: per-frame pose confidence (`pose_confidence`, :70-93) and the inlier count used to pick trustworthy frames
(`n_inliers_per_pose`, `_get_threshold_for_confidence`, :60-68, :95-104).  Same two device kernels as the main path at other shapes
— the ViT (ViT-B/14-reg, 518^2, all 12 blocks + final norm = `x_norm_patchtokens`) and the rasteriser (518^2, cropped intrinsics,
ambient 5) — plus `fp_roi_align` for the photo crop.

Tracking half: 2D-3D correspondences of a trusted frame (`compute_2d3d_correspondences`, `_compute_3d_points`, :102-158), the point
tracker call (`_track_frames`, :160-166), pose from tracks (`_compute_pnp`, `compute_pnp_or_need_resample`, :168-193) and
`get_query_frames` (:195-205).  What the reference does on the host there — a Python loop over a dictionary of projected samples,
cv2.solvePnP(SOLVEPNP_EPNP) per frame — runs on the device in fp64 (`ops.patch_points`, `ops.pnp_epnp`, csrc/refine.hip), batched.

Deviations, on purpose: features are computed in bf16 with fp32 accumulation (the reference runs this model in fp32 on
`dino_device`); the render comes from the HIP rasteriser instead of pyrender/EGL; EPnP is a stated restatement of the algorithm
OpenCV ships, not pinned to OpenCV; CoTracker is not vendored — the tracker is a callable the caller passes
(`tracker=`); the 10 000 surface samples are drawn once per mesh (seeded for this package's TriMesh) instead of on
every call.
"""
from __future__ import annotations

import logging
import math

import numpy as np
import torch

from freepose_amd import ops
from freepose_amd.mesh_io import TriMesh, device_mesh, mesh_signature
from freepose_amd.src.pipeline import refiner_utils

log = logging.getLogger(__name__)


class TrackingRefiner:
    def __init__(self, dino_model="dinov2_vitb14_reg", dino_device="cuda", cotracker_device="cpu", state_dict=None, seed=0, tracker=None):
        """tracker: callable(frames_u8 [T,H,W,3], queries_f32 [N,3] = (t, x, y)) -> (tracks [T,N,2], visibility bool [T,N])"""
        self.dino_device = dino_device
        self.cotracker_device = cotracker_device
        self.tracker = tracker
        self.dinov2 = ops.ViT(dino_model, state_dict=state_dict, seed=seed)
        self._host_state()

    def _host_state(self):
        """everything but the ViT and the tracker (the host-only tests build the object without a device)"""
        self.patch_size = 14
        self.image_size = int(math.sqrt(1370 - 1) * self.patch_size)     # 518 (tracking_refiner.py:26)
        self.feats_size = self.image_size // self.patch_size              # 37
        self.n_samples = 10000                                            # surface samples per mesh (tracking_refiner.py:103)
        self.sample_seed = 0                                              # seed of TriMesh.sample
        self._sample_cache = None
        self._mesh_cache = {}
        return self

    # ---- rendering / cropping --------------------------------------------------------------------------------------
    def _device_mesh(self, mesh) -> ops.Mesh:
        # keyed by identity AND content: the pipeline scales meshes in place (online_pose_estimator.py:60,64) and ids are recycled
        key, sig = id(mesh), mesh_signature(mesh)
        hit = self._mesh_cache.get(key)
        if hit is None or hit[1] != sig:
            hit = (device_mesh(mesh).set_ambient(5.0), sig)              # ambient_light=[5,5,5] (tracking_refiner.py:33)
            self._mesh_cache = {key: hit}
        return hit[0]

    def _render(self, mesh, width, height, K, transform):
        """colour u8 [H,W,3] and metric depth f32 [H,W] of `mesh` under `transform` (object -> OpenCV camera)"""
        K = np.asarray(K, dtype=np.float64)
        pose = torch.from_numpy(np.asarray(transform, dtype=np.float32).reshape(1, 4, 4))
        rgb, depth = ops.rasterize(self._device_mesh(mesh), pose, 1.0, K[0, 0], K[1, 1], K[0, 2], K[1, 2], width, height)
        return rgb[0], depth[0]

    @staticmethod
    def _sample_points(mesh) -> torch.Tensor:
        """100 homogeneous object points: the reference seeds the global NumPy generator with 42 and draws vertex indices
        with np.random.choice (:45-48); the same legacy stream without the global side effect"""
        vertices = np.asarray(mesh.vertices)
        pick = np.random.RandomState(42).choice(np.arange(len(vertices)), 100)
        return torch.from_numpy(np.pad(vertices[pick], ((0, 0), (0, 1)), constant_values=1.).copy()).float()

    def _crop_inputs(self, mesh, K, transform):
        """what the crop arithmetic takes, as float32 tensors: the 100 object points, K [3,3], the pose [1,4,4]"""
        return (self._sample_points(mesh), torch.from_numpy(np.asarray(K)).view(3, 3).float(),
                torch.from_numpy(np.asarray(transform)).view(1, 4, 4).float())

    def _crop_image(self, mesh, image, K, transform):
        vertices, K, transform = self._crop_inputs(mesh, K, transform)
        image = refiner_utils.MaybeToTensor()(image)
        cropped_images, recomputed_bboxes = refiner_utils.crop_image(image, transform, vertices, K, 518, 518)
        new_Ks = refiner_utils.update_K_with_crop(K, recomputed_bboxes, 518, 518)
        return cropped_images[0], recomputed_bboxes[0], new_Ks[0]

    # ---- confidence ------------------------------------------------------------------------------------------------
    def _get_threshold_for_confidence(self, similarity_matrices, top_quantile=0.2):
        """lower edge of the histogram bin (50 bins over the positive similarities) at which the mass counted from the top
        first exceeds `top_quantile` of the total (tracking_refiner.py:60-68)"""
        counts, edges = np.histogram(similarity_matrices[similarity_matrices > 0], bins=50)
        budget = counts.sum() * top_quantile
        seen = 0
        edge = edges[0]
        for k in range(len(counts) - 1, -1, -1):
            seen += counts[k]
            edge = edges[k]
            if seen > budget:
                break
        return edge

    def _patch_features(self, chw_01: torch.Tensor) -> torch.Tensor:
        """x_norm_patchtokens of one image in [0,1] (ImageNet normalisation happens inside the ViT's im2col kernel)"""
        x = chw_01.unsqueeze(0).to(torch.bfloat16).cuda()
        f = self.dinov2(x, layer=len_blocks(self.dinov2), feature_type="patch")          # [1, 1369, D]
        return f[0].float()

    def pose_confidence(self, mesh, photo, K, transform):
        return self.pose_confidences(mesh, [photo], K, [transform])[0]

    def pose_confidences(self, mesh, frames, K, transforms, window=16):
        """pose_confidence (reference :70-96) for a list of (frame, pose) pairs: [n, 37, 37] masked patch cosines between the photo crop and
        the render of `mesh` under the pose.  The reference visits the pairs one by one with two B = 1 ViT-B forwards each
        (n_inliers_per_pose :98-103); they are independent, so the photo crops and renders of `window` pairs share ONE ViT call — a crop's
        features do not depend on its batch: the same confidences, pair for pair."""
        g = self.feats_size
        out = []
        pairs = list(zip(frames, transforms))
        for w0 in range(0, len(pairs), max(1, int(window))):
            chunk = pairs[w0:w0 + max(1, int(window))]
            crops, valids = [], []
            for photo, transform in chunk:
                cropped_photo, _new_bbox, new_K = self._crop_image(mesh, photo, K, transform)
                rendered, rendered_depth = self._render(mesh, 518, 518, new_K.numpy(), transform)
                valids.append(rendered_depth > 0)
                crops.append(cropped_photo.clamp(0, 1).to(torch.bfloat16))
                crops.append(rendered.permute(2, 0, 1).float().div(255).to(torch.bfloat16))
            feats = self.dinov2(torch.stack([c.cuda() for c in crops]), layer=len_blocks(self.dinov2), feature_type="patch").float()   # [2n, 1369, D]
            feats = feats / torch.linalg.norm(feats, dim=-1, keepdim=True)
            cos = (feats[0::2] * feats[1::2]).sum(-1).view(len(chunk), g, g).cpu()
            valid = torch.stack(valids).float().cpu().numpy()                                   # one device -> host copy per window
            for i in range(len(chunk)):
                render_valid_37x37_mask = refiner_utils.cubic_resize(valid[i], (37, 37)) > 0.5  # cv2.INTER_CUBIC (:78)
                out.append((cos[i] * torch.from_numpy(render_valid_37x37_mask).float()).numpy())
        return np.stack(out) if out else np.zeros((0, g, g), np.float32)

    def n_inliers_per_pose(self, mesh, frames, K, transforms):
        confidences = self.pose_confidences(mesh, frames, K, transforms)
        thr = self._get_threshold_for_confidence(confidences)
        return (confidences > thr).sum(-1).sum(-1), thr

    # ---- 2D-3D correspondences (reference :102-158) -----------------------------------------------------------------------------
    def _surface_samples(self, mesh) -> np.ndarray:
        """the 10 000 surface samples of `mesh` (reference :103 draws new ones on every call; here one draw per mesh content, and
        for this package's TriMesh a seeded one, so a clip gives the same poses twice)"""
        sig = mesh_signature(mesh)
        hit = self._sample_cache
        if hit is None or hit[0] != sig:
            pts = mesh.sample(self.n_samples, seed=self.sample_seed) if isinstance(mesh, TriMesh) else mesh.sample(self.n_samples)
            hit = self._sample_cache = (sig, np.ascontiguousarray(np.asarray(pts, dtype=np.float64)))
        return hit[1]

    def _compute_3d_points(self, mesh, render_valid_coords, K, transform, points=None):
        """object-frame point [n,3] for each patch cell (x, y) of `render_valid_coords` [n,2]: of the surface samples that project
        into the cell, the quarter closest to its centre, and of those the one nearest the camera (reference :102-130; the selection
        runs on the device, ops.patch_points).  A cell nothing projects into gives (0, 0, 0) and a warning, like the reference.
        `points`: the surface samples [S,3] to use instead of mesh.sample(10000)."""
        samples = self._surface_samples(mesh) if points is None else np.ascontiguousarray(np.asarray(points, dtype=np.float64))
        cells = np.asarray(render_valid_coords).reshape(-1, 2).astype(np.int32)
        if len(cells) == 0:
            return np.zeros((0, 3))
        pose = np.asarray(transform, dtype=np.float64).reshape(1, 4, 4)
        intrinsics = np.asarray(K, dtype=np.float64).reshape(1, 3, 3)
        chosen = ops.patch_points(samples, pose, intrinsics, cells[None], patch=float(self.patch_size))[0].cpu().numpy()
        empty = chosen < 0
        for cell in cells[empty]:
            log.warning("no surface sample projects into patch cell %s: its point is (0, 0, 0)", cell.tolist())
        out = samples[np.where(empty, 0, chosen)]
        out[empty] = 0.0
        return out

    def _crop_box(self, mesh, K, transform):
        """the box and intrinsics `_crop_image` returns, without resampling any pixels"""
        points, K, pose = self._crop_inputs(mesh, K, transform)
        boxes = refiner_utils.crop_boxes(pose, points, K, 518, 518)
        return boxes[0], refiner_utils.update_K_with_crop(K, boxes, 518, 518)[0]

    @staticmethod
    def _valid_cells(render_mask, proposal_mask=None):
        """(x, y) cells to query, in raster order: the cells of the 37 x 37 grid covered by the render of the shrunk mesh and, when a
        proposal mask is given, by that mask too — unless the intersection holds fewer than 4 cells, then the render alone"""
        keep = np.asarray(render_mask, dtype=bool)
        if proposal_mask is not None:
            both = keep & np.asarray(proposal_mask, dtype=bool)
            if np.count_nonzero(both) >= 4:
                keep = both
            else:
                log.warning("fewer than 4 patch cells inside the proposal mask: querying every cell of the render")
        rows, cols = np.nonzero(keep)
        return np.stack([cols, rows], axis=1)

    def _cells_to_pixels(self, cells, crop_box):
        """centres of patch cells of the 518^2 crop -> pixels of the full image the crop box (x1, y1, x2, y2) was cut from.
        float32 throughout: centre = cell * 14 + 7, scaled by box size / 518, shifted by the box corner."""
        box = np.asarray(crop_box, dtype=np.float32).reshape(4)
        corner, size = box[:2], box[2:] - box[:2]
        centres = np.asarray(cells).astype(np.float32) * np.float32(self.patch_size) + np.float32(self.patch_size * 0.5)
        return centres / np.float32(self.image_size) * size[None, :] + corner[None, :]

    def _grid_mask(self, image_518) -> np.ndarray:
        """bool [37,37]: the 518^2 float image resized to the patch grid (cubic) and thresholded at one half"""
        return refiner_utils.cubic_resize(np.asarray(image_518, dtype=np.float32), (self.feats_size, self.feats_size)) > 0.5

    def compute_2d3d_correspondences(self, mesh, photo, K, transform, mask=None, points=None):
        """query pixels [n,2] (full image) and their object-frame points [n,3] under `transform` (reference :132-158): the patch
        cells covered by the render of the mesh shrunk to 0.8 (and by `mask`), each with the surface sample `_compute_3d_points`
        picks for it.  `photo` is accepted for the reference's signature; only its crop box is needed, which does not depend on
        the pixels."""
        crop_box, crop_K = self._crop_box(mesh, K, transform)
        crop_K = crop_K.numpy()
        proposal = None
        if mask is not None:
            mask_crop, _, _ = self._crop_image(mesh, np.asarray(mask, dtype=np.float32)[:, :, None], K, transform)
            proposal = self._grid_mask(mask_crop[0].float().cpu().numpy())
        shrunk = mesh.copy()
        shrunk.vertices = np.asarray(shrunk.vertices) * 0.8
        if getattr(shrunk, "vertices_f64", None) is not None:
            shrunk.vertices_f64 = shrunk.vertices_f64 * 0.8
        _, depth = self._render(shrunk, self.image_size, self.image_size, crop_K, transform)
        cells = self._valid_cells(self._grid_mask((depth > 0).float().cpu().numpy()), proposal)
        return self._cells_to_pixels(cells, crop_box.numpy()), self._compute_3d_points(mesh, cells, crop_K, transform, points=points)

    # ---- tracking and pose from tracks (reference :160-205) ------------------------------------------------------------------
    def _track_frames(self, frames, query_points):
        """tracks [T,N,2] and visibility bool [T,N] of the query points (t, x, y) [N,3] over `frames` [T,H,W,3], from the tracker
        passed to the constructor (the reference calls CoTracker2 with backward_tracking=True here, :160-166)"""
        if self.tracker is None:
            raise RuntimeError(
                "TrackingRefiner: no point tracker. CoTracker is not shipped with this package (the reference fetches it from torch.hub); "
                "pass tracker=callable(frames_u8[T,H,W,3], queries_f32[N,3] = (t, x, y)) -> (tracks [T,N,2], visibility bool [T,N]) to the "
                "constructor, or --tracker module:factory to scripts/smooth_poses_video.py (INTEGRATION.md shows CoTracker wrapped that way)")
        frames = np.ascontiguousarray(np.asarray(frames, dtype=np.uint8))
        queries = np.ascontiguousarray(np.asarray(query_points, dtype=np.float32))
        tracks, visibility = self.tracker(frames, queries)
        to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)   # noqa: E731
        tracks, visibility = to_np(tracks).astype(np.float64), to_np(visibility).astype(bool)
        if tracks.shape != (len(frames), len(queries), 2) or visibility.shape != tracks.shape[:2]:
            raise ValueError(f"tracker returned tracks {tracks.shape} / visibility {visibility.shape} for {len(frames)} frames and "
                             f"{len(queries)} queries ([T,N,2] and [T,N])")
        return tracks, visibility

    @staticmethod
    def _pose_from_pnp(row) -> np.ndarray:
        """4 x 4 pose from one ops.pnp_epnp record (R row-major, then t)"""
        pose = np.eye(4)
        pose[:3, :3] = row[:9].reshape(3, 3)
        pose[:3, 3] = row[9:12]
        return pose

    def _compute_pnp(self, image_keypoints, render_real_3d_points, matches, K):
        """pose by EPnP on the matched pairs and the indices of the matches kept (all of them: no outlier rejection, like the
        reference :168-179; ops.pnp_epnp).  `matches`: objects with queryIdx / trainIdx (cv2.DMatch) or (query index, train index)
        pairs; the query index addresses `image_keypoints`, the train index `render_real_3d_points`."""
        pairs = np.array([(m.queryIdx, m.trainIdx) if hasattr(m, "queryIdx") else (int(m[0]), int(m[1])) for m in matches],
                         dtype=np.int64).reshape(-1, 2)
        pixels = np.asarray(image_keypoints, dtype=np.float64).reshape(-1, 2)[pairs[:, 0]]
        points = np.asarray(render_real_3d_points, dtype=np.float64).reshape(-1, 3)[pairs[:, 1]]
        row = ops.pnp_epnp(points, pixels[None], K)[0].cpu().numpy()
        if row[14] != ops.PNP_OK:
            raise ValueError(f"TrackingRefiner._compute_pnp: EPnP status {int(row[14])} on {len(pairs)} matches "
                             "(1: fewer than 4 points, 2: coplanar or coincident points)")
        return self._pose_from_pnp(row), np.arange(len(pairs))

    def compute_pnp_or_need_resample(self, mesh, photo, points2d, points2d_visibility, points3d, K):
        """(need new query points?, pose from the visible tracks) (reference :181-193).  Fewer than half of the points visible: yes,
        and no pose.  Otherwise the pose by EPnP on the visible ones, fresh query points under that pose, and the answer is yes when
        the fresh points lie further from the tracked ones (median distance to the nearest tracked point) than from each other
        (median distance to the nearest other fresh point)."""
        visible = np.flatnonzero(np.asarray(points2d_visibility))
        if 2 * len(visible) < len(points2d_visibility):
            return True, None
        pose, _ = self._compute_pnp(points2d, points3d, [(int(i), int(i)) for i in visible], K)
        fresh, _ = self.compute_2d3d_correspondences(mesh, photo, K, pose)
        fresh = np.asarray(fresh, dtype=np.float64)
        tracked = np.asarray(points2d, dtype=np.float64).reshape(-1, 2)
        to_tracked = np.sqrt(((fresh[:, None, :] - tracked[None, :, :]) ** 2).sum(-1).min(axis=1))
        among = ((fresh[:, None, :] - fresh[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(among, np.inf)
        return bool(np.median(to_tracked) > np.median(np.sqrt(among.min(axis=1)))), pose

    def get_query_frames(self, n_inliers_per_frame, n_reference_detections=8):
        """sorted indices of `n_reference_detections` query frames (reference :195-205): greedily the frame with the most inliers,
        after which it and its neighbours within int(n_frames / n_reference_detections / 2) frames no longer count"""
        score = np.array(n_inliers_per_frame, copy=True)
        reach = int(len(score) / n_reference_detections / 2)
        picked = np.empty(n_reference_detections, dtype=np.int64)
        for k in range(n_reference_detections):
            best = int(np.argmax(score))
            picked[k] = best
            score[max(best - reach, 0):best + reach + 1] = 0
        return np.sort(picked)

    # ---- names that are no reference methods ------------------------------------------------------------------------------------
    def __getattr__(self, name):
        if name in ("refine", "refine_poses", "track", "smooth_poses"):
            raise NotImplementedError(f"TrackingRefiner.{name}: not a method of the reference's class; the tracked trajectory is "
                                      "assembled by scripts/smooth_poses_video.py")
        raise AttributeError(name)


def len_blocks(vit: ops.ViT) -> int:
    return int(getattr(vit, "depth", 12))
