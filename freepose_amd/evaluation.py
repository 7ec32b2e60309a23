"""Pose-error evaluation on the GPU: the error functions of the reference's modified BOP toolkit (bop_toolkit_lib/pose_error.py: cus,
chamfer, chamfer_proj, vsd, re, te) for many estimate x ground-truth pairs at once.

The reference renders two depth images per pair with an OpenGL renderer and builds two kd-trees per pair
(scripts/eval_calc_errors.py:311-570).  Here the renders are two batches of the HIP rasteriser feeding one per-pixel compare
(fp_depth_compare), and the chamfer distances are one batched brute-force nearest-neighbour launch (fp_chamfer).  The kernels return
integer pixel counts / float64 distances; the error values are formed below in float64, in the reference's expression order.

Numerics (DESIGN.md "Scoring"): cus / vsd are integer-exact given the same depth images; chamfer / chamfer_proj are within
2e-6 (r + e) of the kd-tree result; re / te are the reference's host expressions.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional, Sequence

import numpy as np
import torch

from . import ops
from .mesh_io import device_mesh, mesh_cloud_f64, mesh_signature

ERROR_TYPES = ("cus", "chamfer", "chamfer_proj", "vsd", "re", "te")
VSD_TAUS_DEFAULT = list(np.arange(0.05, 0.51, 0.05))      # eval_calc_errors.py:45


def cus_from_counts(inter: int, union: int) -> float:
    """pose_error.py:381-386"""
    union_count = float(union)
    if union_count > 0:
        return float(1.0 - int(inter) / union_count)
    return 1.0


def vsd_from_counts(visib_inter: int, visib_union: int, costs: Sequence[int]) -> list:
    """pose_error.py:84-110 with the step cost: (sum(dists >= tau) + |union| - |inter|) / |union| per tau"""
    if int(visib_union) == 0:
        return [1.0] * len(costs)
    comp = int(visib_union) - int(visib_inter)
    return [float((int(c) + comp) / float(int(visib_union))) for c in costs]


def re(R_est, R_gt) -> float:
    """rotational error in degrees (pose_error.py:288-303)"""
    R_est, R_gt = np.asarray(R_est, np.float64), np.asarray(R_gt, np.float64)
    assert R_est.shape == R_gt.shape == (3, 3)
    error_cos = float(0.5 * (np.trace(R_est.dot(np.linalg.inv(R_gt))) - 1.0))
    error_cos = min(1.0, max(-1.0, error_cos))
    return 180.0 * math.acos(error_cos) / np.pi


def te(t_est, t_gt) -> float:
    """translational error (pose_error.py:306-315)"""
    t_est, t_gt = np.asarray(t_est, np.float64), np.asarray(t_gt, np.float64)
    assert t_est.size == t_gt.size == 3
    return np.linalg.norm(t_gt.reshape(3, 1) - t_est.reshape(3, 1))


def _pose44(R, t) -> np.ndarray:
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.asarray(R, np.float64).reshape(3, 3)
    T[:3, 3] = np.asarray(t, np.float64).reshape(3)
    return T


class PoseErrorEvaluator:
    """errors of (inferred mesh, s_e, R_e, t_e) against (ground-truth object, R_g, t_g) pairs of one image or of many.

    width, height: size of the rendered depth images (the dataset's image size).  Ground-truth models are registered once with
    add_gt_model; inferred meshes are uploaded on first use and kept in a small cache keyed by identity and content."""

    def __init__(self, width: int, height: int, max_batch: int = 64, mesh_cache_size: int = 32):
        self.width, self.height = int(width), int(height)
        self.max_batch = int(max_batch)             # pairs rendered per chunk: 2 depth stacks + 1 colour stack of this many images
        self._gt = {}                               # obj_id -> (mesh, ops.Mesh | None, f64 cloud on device | None)
        self._mesh_cache = OrderedDict()            # id(mesh) -> (signature, ops.Mesh | None, cloud | None, mesh)
        self._mesh_cache_size = int(mesh_cache_size)

    # ---- models ----------------------------------------------------------------------------------------------------------------------
    def add_gt_model(self, obj_id, mesh):
        self._gt[obj_id] = [mesh, None, None]
        return self

    def _gt_entry(self, obj_id, want: str):
        if obj_id not in self._gt:
            raise KeyError(f"ground-truth model {obj_id!r} was not registered (add_gt_model)")
        e = self._gt[obj_id]
        if want == "mesh" and e[1] is None:
            e[1] = device_mesh(e[0])
        if want == "cloud" and e[2] is None:
            e[2] = torch.from_numpy(mesh_cloud_f64(e[0])).cuda()
        return e[1] if want == "mesh" else e[2]

    def _inf_entry(self, mesh, want: str):
        # keyed by identity AND content, like TrackingRefiner._device_mesh: callers scale meshes in place and ids are recycled
        key, sig = id(mesh), mesh_signature(mesh)
        hit = self._mesh_cache.get(key)
        if hit is None or hit[0] != sig:
            hit = [sig, None, None, mesh]           # holding the mesh keeps its id from being recycled while cached
            self._mesh_cache[key] = hit
            while len(self._mesh_cache) > self._mesh_cache_size:
                self._mesh_cache.popitem(last=False)
        else:
            self._mesh_cache.move_to_end(key)
        if want == "mesh" and hit[1] is None:
            hit[1] = device_mesh(mesh)
        if want == "cloud" and hit[2] is None:
            hit[2] = torch.from_numpy(mesh_cloud_f64(mesh)).cuda()
        return hit[1] if want == "mesh" else hit[2]

    # ---- renders ---------------------------------------------------------------------------------------------------------------------
    def _render_group(self, out: torch.Tensor, dmesh, rows, poses, scale, Ks):
        """rows of `out` [n,H,W] <- depth renders of one device mesh; one rasteriser call per distinct (scale, intrinsics)"""
        groups = OrderedDict()
        for r, T, s, K in zip(rows, poses, scale, Ks):
            k = (float(np.float32(s)), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
            groups.setdefault(k, []).append((r, T))
        for (s, fx, fy, cx, cy), items in groups.items():
            P = torch.from_numpy(np.stack([T for _, T in items]))
            _, depth, _, _ = ops.rasterize_extents(dmesh, P, s, fx, fy, cx, cy, self.width, self.height, want_depth=True)
            out[torch.as_tensor([r for r, _ in items], device=out.device)] = depth

    def _depth_stacks(self, pairs, Ks):
        n = len(pairs)
        dev = torch.device("cuda", torch.cuda.current_device())
        d_est = torch.empty((n, self.height, self.width), dtype=torch.float32, device=dev)
        d_gt = torch.empty_like(d_est)
        by_inf, by_gt = OrderedDict(), OrderedDict()
        for i, p in enumerate(pairs):
            by_inf.setdefault(id(p[0]), []).append(i)
            by_gt.setdefault(p[4], []).append(i)
        for rows in by_inf.values():                 # estimates grouped by inferred mesh
            dm = self._inf_entry(pairs[rows[0]][0], "mesh")
            self._render_group(d_est, dm, rows, [_pose44(pairs[i][2], pairs[i][3]) for i in rows], [pairs[i][1] for i in rows],
                               [Ks[i] for i in rows])
        for obj_id, rows in by_gt.items():           # ground truths grouped by object
            dm = self._gt_entry(obj_id, "mesh")
            self._render_group(d_gt, dm, rows, [_pose44(pairs[i][5], pairs[i][6]) for i in rows], [1.0] * len(rows), [Ks[i] for i in rows])
        return d_est, d_gt

    # ---- errors ----------------------------------------------------------------------------------------------------------------------
    def errors(self, error_type: str, pairs, K, depth_test=None, vsd_delta: float = 15.0, vsd_taus=None,
               vsd_normalized_by_diameter: bool = True, diameters=None, img_idx=None) -> list:
        """pairs: list of (inf_mesh, s_e, R_e, t_e, gt_obj_id, R_g, t_g).  K: [3,3] for all pairs or one per pair.  vsd: depth_test
        [H,W] (or [n_img,H,W] with img_idx per pair) in the unit of the models, diameters = {gt_obj_id: diameter} or one per pair.
        Returns one value per pair: a float, or for vsd a list with one float per tau."""
        if error_type not in ERROR_TYPES:
            raise ValueError(f"unknown error type '{error_type}': supported are {', '.join(ERROR_TYPES)}")
        pairs = list(pairs)
        n = len(pairs)
        if n == 0:
            return []
        if error_type == "re":
            return [re(p[2], p[5]) for p in pairs]
        if error_type == "te":
            return [te(p[3], p[6]) for p in pairs]
        Ka = np.asarray(K, np.float64)
        Ks = [Ka.reshape(3, 3)] * n if Ka.size == 9 else list(Ka.reshape(n, 3, 3))
        if error_type in ("chamfer", "chamfer_proj"):
            clouds, index, pr = [], {}, []
            for p in pairs:
                ke, kg = ("e", id(p[0])), ("g", p[4])
                if ke not in index:
                    index[ke] = len(clouds)
                    clouds.append(self._inf_entry(p[0], "cloud"))
                if kg not in index:
                    index[kg] = len(clouds)
                    clouds.append(self._gt_entry(p[4], "cloud"))
                pr.append((index[ke], index[kg]))
            args = (clouds, np.asarray(pr), [float(p[1]) for p in pairs], np.stack([np.asarray(p[2], np.float64).reshape(3, 3) for p in pairs]),
                    np.stack([np.asarray(p[3], np.float64).reshape(3) for p in pairs]),
                    np.stack([np.asarray(p[5], np.float64).reshape(3, 3) for p in pairs]),
                    np.stack([np.asarray(p[6], np.float64).reshape(3) for p in pairs]))
            e = ops.chamfer(*args) if error_type == "chamfer" else ops.chamfer_proj(*args, np.stack(Ks))
            return [float(x) for x in e.cpu().numpy()]
        # cus / vsd: two render batches feed the per-pixel compare, max_batch pairs at a time
        if error_type == "vsd":
            if depth_test is None:
                raise ValueError("vsd needs the test depth image")
            taus = [float(t) for t in (VSD_TAUS_DEFAULT if vsd_taus is None else vsd_taus)]
            dt = torch.as_tensor(np.asarray(depth_test, np.float32) if not isinstance(depth_test, torch.Tensor) else depth_test)
            dt = dt.to("cuda", torch.float32)
            dt = dt[None] if dt.dim() == 2 else dt
            idx = np.zeros(n, np.int32) if img_idx is None else np.asarray(img_idx, np.int32).reshape(n)
            if vsd_normalized_by_diameter:
                if diameters is None:
                    raise ValueError("vsd_normalized_by_diameter needs the diameters")
                div = [float(diameters[p[4]]) if isinstance(diameters, dict) else float(diameters[i]) for i, p in enumerate(pairs)]
            else:
                div = [1.0] * n
        out = []
        for b0 in range(0, n, self.max_batch):
            b1 = min(n, b0 + self.max_batch)
            d_est, d_gt = self._depth_stacks(pairs[b0:b1], Ks[b0:b1])
            if error_type == "cus":
                c = ops.depth_compare(d_est, d_gt).cpu().numpy()
                out += [cus_from_counts(r[0], r[1]) for r in c]
            else:
                c = ops.depth_compare(d_est, d_gt, dt, idx[b0:b1], np.stack(Ks[b0:b1]), float(vsd_delta), taus, div[b0:b1]).cpu().numpy()
                out += [vsd_from_counts(r[2], r[3], r[4:]) for r in c]
        return out
