"""Pose-error evaluation on the GPU: the error functions of the reference's modified BOP toolkit (bop_toolkit_lib/pose_error.py: cus,
chamfer, chamfer_proj, vsd, re, te) for many estimate x ground-truth pairs at once.

The reference renders two depth images per pair with an OpenGL renderer and builds two kd-trees per pair
(scripts/eval_calc_errors.py:311-570).  Here the renders are two batches of the HIP rasteriser feeding one per-pixel compare
(fp_depth_compare), and the chamfer distances are one batched brute-force nearest-neighbour launch (fp_chamfer).  The kernels return
integer pixel counts / float64 distances; the error values are formed below in float64, in the reference's expression order.

Numerics (DESIGN.md "Scoring"): cus / vsd are integer-exact given the same depth images; chamfer / chamfer_proj are within
2e-6 (r + e) of the kd-tree result; re / te are the reference's host expressions.

The second half turns those errors into scores: `BopScorer` packs the groups of an errors directory once and matches estimates to ground
truths and counts recalls for all thresholds in one device call (fp_bop_scores; eval_calc_scores.py:188-290, pose_matching.py, score.py;
DESIGN.md §16), exactly.

The third part prepares the inputs of that chain: `GtInfoCalculator` computes the scene_gt_info records and the mask / mask_visib images
of ground-truth instances (fp_gt_visibility over canvases of the HIP rasteriser; bop_toolkit/scripts/calc_gt_info.py, calc_gt_masks.py)
and `models_info` the diameter and bounding box of models (fp_pts_diameter; calc_model_info.py, misc.calc_pts_diameter).
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


# ---- BOP scores: matching, recalls (csrc/bop_score.hip) --------------------------------------------------------------------------------
BOP_NORMALIZED_BY_DIAMETER = ("ad", "add", "adi", "mssd", "chamfer")       # eval_calc_scores.py:55,57
BOP_NORMALIZED_BY_IM_WIDTH = ("mspd", "chamfer_proj")


def score_signature(correct_th, visib_gt_min) -> str:
    """misc.get_score_signature"""
    return "th=" + "-".join("{:.3f}".format(t) for t in correct_th) + "_min-visib={:.3f}".format(visib_gt_min)


def bop_json_text(content) -> str:
    """the text inout.save_json writes: a dict with its top-level keys sorted, one per line; a list with one record per line; inner
    values through json.dumps(sort_keys=True)"""
    import json
    if isinstance(content, dict):
        items = sorted(content.items(), key=lambda x: x[0])
        return "{\n" + ",\n".join('  "{}": {}'.format(k, json.dumps(v, sort_keys=True)) for k, v in items) + ("\n" if items else "") + "}"
    if isinstance(content, list):
        return "[\n" + ",\n".join("  {}".format(json.dumps(e, sort_keys=True)) for e in content) + ("\n" if content else "") + "]"
    return json.dumps(content, sort_keys=True)


def bop_gt_valid(im_gt, im_gt_info, im_targets, visib_gt_min) -> list:
    """which ground truths of one image may be matched (eval_calc_scores.py:225-253).  im_targets: obj_id -> target of the image."""
    if visib_gt_min >= 0:
        return [bool(gt["obj_id"] in im_targets and im_gt_info[gt_id]["visib_fract"] >= visib_gt_min) for gt_id, gt in enumerate(im_gt)]
    valid = [False] * len(im_gt)
    to_add = {obj_id: trg["inst_count"] for obj_id, trg in im_targets.items()}
    for gt_id in sorted(range(len(im_gt)), key=lambda i: im_gt_info[i]["visib_fract"], reverse=True):   # stable: ties keep gt_id order
        obj_id = im_gt[gt_id]["obj_id"]
        if to_add.get(obj_id, 0) > 0:
            valid[gt_id] = True
            to_add[obj_id] -= 1
    return valid


def _recall(tp_count, targets_count) -> float:
    """score.py calc_recall"""
    return 0.0 if targets_count == 0 else tp_count / float(targets_count)


class BopScorer:
    """The matching and scoring of bop_toolkit/scripts/eval_calc_scores.py:188-290 for all thresholds in one device call.

    targets: the list of the targets file; scene_gt / scene_gt_info: scene_id -> im_id -> list per ground truth (integer keys; only
    "obj_id" and "visib_fract" are read); obj_ids / scene_ids: the objects and scenes the recalls are listed for.  The groups — one per
    (scene, image, target object with a ground truth in the image) — and the validity of every ground truth are built once, here; no
    file is read."""

    def __init__(self, targets, scene_gt, scene_gt_info, obj_ids, scene_ids, visib_gt_min=-1):
        self.obj_ids, self.scene_ids = [int(i) for i in obj_ids], [int(i) for i in scene_ids]
        self.visib_gt_min = float(visib_gt_min)
        obj_index = {o: k for k, o in enumerate(self.obj_ids)}
        scene_index = {s: k for k, s in enumerate(self.scene_ids)}
        targets_org = {}
        for t in targets:
            targets_org.setdefault(t["scene_id"], {}).setdefault(t["im_id"], {})[t["obj_id"]] = t
        self.records = []         # the reference's match records before matching, in its order: scene, image (targets order), gt_id
        self.groups = []          # (scene_id, im_id, obj_id, [record index per ground truth, ascending gt_id], obj index, scene index)
        for scene_id, scene_targets in targets_org.items():
            for im_id, im_targets in scene_targets.items():
                im_gt = scene_gt[scene_id][im_id]
                valid = bop_gt_valid(im_gt, scene_gt_info[scene_id][im_id], im_targets, self.visib_gt_min)
                row0 = len(self.records)
                by_obj = {}
                for gt_id, gt in enumerate(im_gt):
                    self.records.append({"scene_id": scene_id, "im_id": im_id, "obj_id": gt["obj_id"], "gt_id": gt_id, "est_id": -1,
                                         "score": -1, "error": -1, "error_norm": -1, "valid": valid[gt_id]})
                    by_obj.setdefault(gt["obj_id"], []).append(row0 + gt_id)
                    if valid[gt_id] and (gt["obj_id"] not in obj_index or scene_id not in scene_index):
                        raise ValueError(f"scene {scene_id}, image {im_id}: the valid ground truth {gt_id} of object {gt['obj_id']} is "
                                         f"outside the object list {self.obj_ids} or the scene list {self.scene_ids}")
                for obj_id, rows in by_obj.items():
                    if obj_id not in im_targets or obj_id not in obj_index or scene_id not in scene_index:
                        continue          # no ground truth of it is valid: nothing can match and there is no target
                    self.groups.append((scene_id, im_id, obj_id, rows, obj_index[obj_id], scene_index[scene_id]))

    # ---- host packing ------------------------------------------------------------------------------------------------------------------
    def pack(self, scene_errs_by_scene, n_top, diameters=None, im_width=None) -> dict:
        """the tables of fp_bop_scores (numpy) + what is needed to read its answer back: `row_record` [R] record index of each table row,
        `ests` per group the estimates in matching order, each (record of the errors file, normalised errors per column)."""
        org = {}
        for scene_id, errs in scene_errs_by_scene.items():
            for e in errs:
                org.setdefault((scene_id, e["im_id"], e["obj_id"]), []).append(e)
        factor = None if im_width is None else 640.0 / float(im_width)
        err, groups, row_record, gt_obj, gt_scene, ests_out = [], [], [], [], [], []
        in_group = np.zeros(len(self.records), bool)
        for scene_id, im_id, obj_id, rows, oi, si in self.groups:
            gt_ids = [self.records[r]["gt_id"] for r in rows]
            ests = org.get((scene_id, im_id, obj_id), [])
            cols = gt_ids
            if ests:
                keys = [int(k) for k in ests[0]["errors"]]
                for e in ests:
                    if [int(k) for k in e["errors"]] != keys:
                        raise ValueError(f"scene {scene_id}, image {im_id}, object {obj_id}: estimate {e['est_id']} lists the ground truths "
                                         f"{list(e['errors'])}, the group's first estimate {keys} (one visiting order per group)")
                if len(set(keys)) != len(keys) or not set(keys) <= set(gt_ids):
                    raise ValueError(f"scene {scene_id}, image {im_id}, object {obj_id}: errors against the ground truths {keys}; the "
                                     f"object's ground truths in this image are {gt_ids}")
                cols = keys + [g for g in gt_ids if g not in keys]            # a ground truth without an error can never match: NaN
            ests = sorted(ests, key=lambda e: e["score"], reverse=True)       # stable: ties keep the file's order
            if n_top > 0:
                ests = ests[:n_top]
            packed = []
            for e in ests:
                vals = list(e["errors"].values())
                if any(len(v) != 1 for v in vals):
                    raise ValueError(f"scene {scene_id}, image {im_id}, object {obj_id}: an error with {len(vals[0])} elements; only "
                                     "one-element errors are scored here (rete needs two thresholds)")
                x = [v[0] for v in vals]
                if diameters is not None:
                    d = float(diameters[e["obj_id"]])
                    x = [v / d for v in x]
                if factor is not None:
                    x = [factor * v for v in x]
                packed.append((e, x))
                err.extend(x + [float("nan")] * (len(cols) - len(x)))
            groups.append((len(err) - len(ests) * len(cols), len(ests), len(cols), len(row_record)))
            row0 = rows[0] - gt_ids[0]
            for g in cols:
                row_record.append(row0 + g)
                in_group[row0 + g] = True
            gt_obj += [oi] * len(cols)
            gt_scene += [si] * len(cols)
            ests_out.append(packed)
        rest = np.flatnonzero(~in_group)          # ground truths of non-target objects: rows of no group, never valid
        row_record = np.asarray(row_record + rest.tolist(), np.int64)
        return {"err": np.asarray(err, np.float64), "groups": np.asarray(groups, np.int32).reshape(-1, 4),
                "gt_valid": np.asarray([self.records[r]["valid"] for r in row_record], np.uint8),
                "gt_obj": np.asarray(gt_obj + [0] * len(rest), np.int32), "gt_scene": np.asarray(gt_scene + [0] * len(rest), np.int32),
                "row_record": row_record, "ests": ests_out, "n_top": int(n_top)}

    def unpack(self, tables, thresholds, match, tp_obj, tp_scene, tar_obj, tar_scene) -> list:
        """the answer of fp_bop_scores (host arrays) -> [(scores dict, match records)] per threshold, the reference's keys and values"""
        out = []
        tars = int(tar_obj.sum())
        row_record = tables["row_record"].tolist()
        row_group = {}                                       # table row -> (the group's estimates, column)
        for (off, E, G, first), ests in zip(tables["groups"].tolist(), tables["ests"]):
            for c in range(G):
                row_group[first + c] = (ests, c)
        for ti, th in enumerate(thresholds):
            records = [dict(r) for r in self.records]
            for row in np.flatnonzero(match[ti] >= 0).tolist():
                ests, c = row_group[row]
                e, x = ests[int(match[ti, row])]
                records[row_record[row]].update(est_id=e["est_id"], score=e["score"], error=[x[c]], error_norm=[x[c] / float(th)])
            tps = int(tp_obj[ti].sum())
            obj_recalls = {o: _recall(int(tp_obj[ti, k]), int(tar_obj[k])) for k, o in enumerate(self.obj_ids)}
            scene_recalls = {s: float(_recall(int(tp_scene[ti, k]), int(tar_scene[k]))) for k, s in enumerate(self.scene_ids)}
            scores = {"recall": float(_recall(tps, tars)), "obj_recalls": obj_recalls,
                      "mean_obj_recall": float(np.mean(list(obj_recalls.values())).squeeze()), "scene_recalls": scene_recalls,
                      "mean_scene_recall": float(np.mean(list(scene_recalls.values())).squeeze()), "gt_count": len(records),
                      "targets_count": tars, "tp_count": tps}
            out.append((scores, records))
        return out

    def scores(self, scene_errs_by_scene, error_type, thresholds, n_top, diameters=None, im_width=None) -> list:
        """scene_errs_by_scene: scene_id -> the list of an errors_<scene>.json; thresholds: one number per score to compute; diameters
        {obj_id: diameter} / im_width are given when the error type is normalised by them (e / diameter, e * (640.0 / im_width), in
        fp64 on the host, before matching).  One device call for all thresholds -> [(scores dict, match records)] per threshold."""
        if error_type == "rete":
            raise ValueError("rete has two thresholds per score; only one-element errors are scored here")
        thresholds = [float(t) for t in thresholds]
        tables = self.pack(scene_errs_by_scene, int(n_top), diameters, im_width)
        res = ops.bop_scores(tables["err"], tables["groups"], tables["gt_valid"], tables["gt_obj"], tables["gt_scene"], thresholds,
                             len(self.obj_ids), len(self.scene_ids), int(n_top))
        return self.unpack(tables, thresholds, *[r.cpu().numpy() for r in res])


# ---- ground-truth info: visibility, boxes, masks, model diameters (csrc/gt_info.hip) ----------------------------------------------------
GT_INFO_KEYS = ("px_count_all", "px_count_valid", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib")    # calc_gt_info.py:176-185
MODEL_INFO_KEYS = ("min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "diameter")                         # calc_model_info.py:42-50
RASTER_MAX_SIDE = 8192                 # the rasteriser's largest canvas side (csrc/raster.hip)
# Canvas pixels rendered per batch.  The rasteriser holds 8 bytes of depth/id buffer per pixel in the context's workspace and the batch
# holds its float32 depth and uint8 colour images next to it: 15 bytes per pixel, so one batch stays at or below 480 MiB (one canvas is
# always rendered, whatever its size: 8192 x 8192 is 960 MiB).
GT_INFO_CANVAS_PIXELS_PER_BATCH = 32 << 20


def gt_info_from_counts(row) -> dict:
    """one row of ops.gt_visibility -> the dict of calc_gt_info.py:154-185, keys in its order.  BOTH boxes are [-1, -1, -1, -1] when no
    pixel is visible: the reference conditions bbox_obj on px_count_visib as well (:163)."""
    r = [int(v) for v in row]
    px_all, px_valid, px_visib = r[0], r[1], r[2]
    visib_fract = px_visib / float(px_all) if px_all > 0 else 0.0
    bbox, bbox_visib = [-1, -1, -1, -1], [-1, -1, -1, -1]
    if px_visib > 0:
        bbox = [r[4], r[5], r[6] - r[4], r[7] - r[5]]                    # misc.calc_2d_bbox: [x, y, max - min, max - min]
        bbox_visib = [r[8], r[9], r[10] - r[8], r[11] - r[9]]
    return {"px_count_all": px_all, "px_count_valid": px_valid, "px_count_visib": px_visib, "visib_fract": float(visib_fract),
            "bbox_obj": bbox, "bbox_visib": bbox_visib}


def model_info_from_row(row) -> dict:
    """one row of ops.pts_diameter -> the dict of calc_model_info.py:42-50, keys in its order"""
    r = [float(v) for v in row]
    return {"min_x": r[1], "min_y": r[2], "min_z": r[3], "size_x": r[4], "size_y": r[5], "size_z": r[6], "diameter": r[0]}


def models_info(clouds_by_obj: dict) -> dict:
    """obj_id -> [N,3] float64 vertices  ->  obj_id -> model info, all models in one device call"""
    ids = list(clouds_by_obj)
    rows = ops.pts_diameter([clouds_by_obj[i] for i in ids]).cpu().numpy() if ids else []
    return {i: model_info_from_row(r) for i, r in zip(ids, rows)}


class GtInfoCalculator:
    """scene_gt_info records and mask / mask_visib images of ground-truth instances (bop_toolkit/scripts/calc_gt_info.py, calc_gt_masks.py).

    width, height: the dataset's image size.  An instance is (image key, obj_id, R [3,3], t [3]); depth_test_by_image maps the image key
    to its depth image [height, width] in the unit of the models (float32, depth_scale applied), K_by_image to its 3x3 intrinsics.  The
    instances of many images are rendered in batches of at most GT_INFO_CANVAS_PIXELS_PER_BATCH canvas pixels and handed to one fused
    pass each (ops.gt_visibility)."""

    def __init__(self, width: int, height: int, delta: float = 15):
        self.width, self.height, self.delta = int(width), int(height), delta
        if self.width < 1 or self.height < 1:
            raise ValueError(f"image size {width} x {height}")
        self._models = {}                           # obj_id -> [mesh, ops.Mesh | None]

    def add_model(self, obj_id, mesh):
        self._models[obj_id] = [mesh, None]
        return self

    def _device_model(self, obj_id):
        if obj_id not in self._models:
            raise KeyError(f"model {obj_id!r} was not registered (add_model)")
        e = self._models[obj_id]
        if e[1] is None:
            e[1] = device_mesh(e[0])
        return e[1]

    def _run(self, instances, depth_test_by_image, K_by_image, large: bool, want_masks: bool):
        W, H = self.width, self.height
        Wr, Hr, ox, oy = (3 * W, 3 * H, W, H) if large else (W, H, 0, 0)
        if Wr > RASTER_MAX_SIDE or Hr > RASTER_MAX_SIDE:
            raise ValueError(f"image size {W} x {H}: the {Wr} x {Hr} canvas exceeds the rasteriser's {RASTER_MAX_SIDE} x {RASTER_MAX_SIDE}")
        instances = list(instances)
        n = len(instances)
        rows = np.zeros((n, ops.GT_INFO_OUT_LD), np.int32)
        masks = np.zeros((n, H, W), np.uint8) if want_masks else None
        visibs = np.zeros((n, H, W), np.uint8) if want_masks else None
        if n == 0:
            return rows, masks, visibs
        keys = []
        for inst in instances:
            if inst[0] not in keys:
                keys.append(inst[0])
        stack = []
        for k in keys:
            d = np.asarray(depth_test_by_image[k], np.float32)
            if d.shape != (H, W):
                raise ValueError(f"depth image of {k!r} is {d.shape[1]} x {d.shape[0]}, the dataset's image size is {W} x {H}")
            stack.append(d)
        dev = torch.device("cuda", torch.cuda.current_device())
        d_test = torch.from_numpy(np.stack(stack)).to(dev)
        Ks = [np.asarray(K_by_image[inst[0]], np.float64).reshape(3, 3) for inst in instances]
        idx = [keys.index(inst[0]) for inst in instances]
        per_batch = max(1, GT_INFO_CANVAS_PIXELS_PER_BATCH // (Wr * Hr))
        for b0 in range(0, n, per_batch):
            b1 = min(n, b0 + per_batch)
            canvas = torch.empty((b1 - b0, Hr, Wr), dtype=torch.float32, device=dev)
            groups = OrderedDict()                  # one rasteriser call per (object, intrinsics)
            for i in range(b0, b1):
                K = Ks[i]
                g = (instances[i][1], float(K[0, 0]), float(K[1, 1]), float(K[0, 2] + ox), float(K[1, 2] + oy))
                groups.setdefault(g, []).append(i)
            for (obj_id, fx, fy, cx, cy), members in groups.items():
                P = torch.from_numpy(np.stack([_pose44(instances[i][2], instances[i][3]) for i in members]))
                _, depth = ops.rasterize(self._device_model(obj_id), P, 1.0, fx, fy, cx, cy, Wr, Hr)
                canvas[torch.as_tensor([i - b0 for i in members], device=dev)] = depth
            c, m, v = ops.gt_visibility(canvas, d_test, idx[b0:b1], np.stack(Ks[b0:b1]), float(self.delta), window=(ox, oy),
                                        want_masks=want_masks)
            rows[b0:b1] = c.cpu().numpy()
            if want_masks:
                masks[b0:b1], visibs[b0:b1] = m.cpu().numpy(), v.cpu().numpy()
        return rows, masks, visibs

    def gt_info(self, instances, depth_test_by_image, K_by_image) -> list:
        """one dict per instance, the reference's keys in its order (calc_gt_info.py:176-185); rendered on the 3W x 3H canvas with the
        principal point shifted by (W, H), so that truncated silhouettes are counted (:70-74)"""
        rows, _, _ = self._run(instances, depth_test_by_image, K_by_image, large=True, want_masks=False)
        return [gt_info_from_counts(r) for r in rows]

    def gt_masks(self, instances, depth_test_by_image, K_by_image):
        """(mask u8 [n,H,W], mask_visib u8 [n,H,W]) on the host, 255 / 0 (calc_gt_masks.py:110-126); rendered at image size"""
        _, masks, visibs = self._run(instances, depth_test_by_image, K_by_image, large=False, want_masks=True)
        return masks, visibs
