"""Drop-in for the reference's `src/utils/video_evaluation.py`: the velocity errors of a pose track against the ground truth (relative
rotation with the symmetry sweep, projected translation, depth) over a set of time offsets.

The reference walks offset x frame pair x 101 symmetries in Python, with pinocchio's SO(3) log / exp per step; here every function is
one call of `ops.video_errors` (csrc/video_eval.hip, fp64), and `video_errors_table` scores all the (video, method) tracks of a results
table in a single call.  There is no host fallback: without the device library these functions raise.

Poses are accepted as [N,4,4] arrays or as sequences of objects that carry `.rotation` and `.translation` (pinocchio's SE3, `Pose`
below).  `svd_pointcloud_align` (reference :143-148) is used by nothing and is not carried over; the unused `est_pts` arguments are kept
in the signatures.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from freepose_amd import ops

GT_SCALE = 0.15                                            # scripts/eval_videos.py:47


class Pose:
    """the two attributes the functions below read of a pose (what pinocchio's SE3 offers)"""

    def __init__(self, rotation, translation):
        self.rotation, self.translation = np.asarray(rotation, dtype=np.float64), np.asarray(translation, dtype=np.float64)


def as_matrices(poses) -> np.ndarray:
    """[N,4,4] array, or a sequence of poses with .rotation / .translation -> f64 [N,4,4]"""
    if isinstance(poses, np.ndarray) or (len(poses) and not hasattr(poses[0], "rotation")):
        T = np.asarray(poses, dtype=np.float64)
        if T.ndim != 3 or T.shape[1:] != (4, 4):
            raise ValueError(f"poses {T.shape} ([N,4,4])")
        return T
    T = np.tile(np.eye(4), (len(poses), 1, 1))
    for i, p in enumerate(poses):
        T[i, :3, :3], T[i, :3, 3] = p.rotation, p.translation
    return T


def _like(poses, T):
    """T [N,4,4] in the form `poses` came in"""
    if isinstance(poses, np.ndarray) or (len(poses) and not hasattr(poses[0], "rotation")):
        return T
    return [Pose(t[:3, :3], t[:3, 3]) for t in T]


def _one(est_poses, gt_poses, dts, est_scale=1.0, gt_scale=1.0, w=1.0, h=1.0, sym_axis=None, n_sym=101, K=None, **kw):
    est, gt = as_matrices(est_poses), as_matrices(gt_poses)
    if len(est) != len(gt):
        raise ValueError(f"{len(est)} estimated and {len(gt)} ground-truth poses")
    dts = np.atleast_1d(np.asarray(dts))
    return ops.video_errors(est[None], gt[None], dts[None].astype(np.int64), est_scale, gt_scale, w, h,
                            sym_axis=None if sym_axis is None else np.asarray(sym_axis, dtype=np.float64).reshape(3), n_sym=n_sym,
                            K=None if K is None else np.asarray(K, dtype=np.float64).reshape(3, 3), **kw)


def _averaged(est_poses, gt_poses, dts, column, **kw):
    """the final number of one metric over offsets too many for one call (16) or not: np.mean over all of them"""
    dts = np.atleast_1d(np.asarray(dts))
    per = [_one(est_poses, gt_poses, dts[i:i + ops.VIDEO_MAX_OFFSETS], **kw)[0][0, :, column].cpu().numpy()
           for i in range(0, len(dts), ops.VIDEO_MAX_OFFSETS)]
    return np.mean(np.concatenate(per))


def get_average_rot_errors_dt(est_poses, gt_poses, dts, sym_axis=None, N_symmetries=101):
    """radians per frame, as the reference returns it (eval_videos converts to degrees)"""
    return _averaged(est_poses, gt_poses, dts, 0, sym_axis=sym_axis, n_sym=N_symmetries)


def get_average_depth_errors_dt(est_poses, gt_poses, est_scale, gt_scale, dts, est_pts=None):
    return _averaged(est_poses, gt_poses, dts, 2, est_scale=est_scale, gt_scale=gt_scale)


def get_average_proj_errors_dt(est_poses, gt_poses, est_scale, gt_scale, dts, w, h, K=None, est_pts=None):
    return _averaged(est_poses, gt_poses, dts, 1, est_scale=est_scale, gt_scale=gt_scale, w=w, h=h, K=K) / np.sqrt(w ** 2 + h ** 2) * 100


def _pair_errors(est_poses, gt_poses, dt, column, **kw):
    n = len(est_poses) - int(dt)
    pairs = _one(est_poses, gt_poses, [int(dt)], return_pairs=True, **kw)[2]
    return pairs[0, 0, :n, column].cpu().numpy().tolist()


def get_rot_errors(est_poses, gt_poses, dt, sym_axis=None, N_symmetries=101):
    return _pair_errors(est_poses, gt_poses, dt, 0, sym_axis=sym_axis, n_sym=N_symmetries)


def get_translation_errors_depth(est_poses, gt_poses, est_scale, gt_scale, dt):
    """the poses are scored as given (it is get_average_depth_errors_dt that aligns them first): align=False"""
    return _pair_errors(est_poses, gt_poses, dt, 2, est_scale=est_scale, gt_scale=gt_scale, align=False)


def get_translation_errors_proj(est_poses, gt_poses, dt, w, h, K=None):
    return _pair_errors(est_poses, gt_poses, dt, 1, w=w, h=h, K=K, align=False)


def project(x, w, h, K=None):
    """host arithmetic on one point, as in the reference (:100-109)"""
    if K is None:
        f = np.sqrt(w ** 2 + h ** 2)
        K = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1.0]])
    u = K @ x
    return u[:2] / u[2]


def align_object_origins(poses1, poses2, scale, ref_frame_idxs=None, est_pts=None):
    """poses1 with the object origin moved to where poses2's origin lies on average (limited to scale / 2); computed by the alignment
    kernel of fp_video_errors.  ref_frame_idxs selects the frames the mean is taken over (default: all)."""
    est, gt = as_matrices(poses1), as_matrices(poses2)
    if ref_frame_idxs is None:
        out = est.copy()
        out[:, :3, 3] = _one(est, gt, [1], est_scale=scale, return_aligned=True)[2][0].cpu().numpy()
        return _like(poses1, out)
    idx = np.asarray(list(ref_frame_idxs))
    if len(idx) < 2:
        raise ValueError("align_object_origins: at least 2 reference frames (fp_video_errors scores tracks of N >= 2)")
    moved = _one(est[idx], gt[idx], [1], est_scale=scale, return_aligned=True)[2][0].cpu().numpy()
    origin = est[idx[0], :3, :3].T @ (moved[0] - est[idx[0], :3, 3])       # moved = R o + t
    return change_object_origin(poses1, origin)


def change_object_origin(poses, new_origin):
    """pose * SE3(I, new_origin) for every pose (:151-155): host arithmetic, N small products"""
    T = as_matrices(poses).copy()
    T[:, :3, 3] = np.einsum("nij,j->ni", T[:, :3, :3], np.asarray(new_origin, dtype=np.float64)) + T[:, :3, 3]
    return _like(poses, T)


def video_errors_table(tracks: Sequence[Optional[dict]], gts: Sequence[dict]) -> np.ndarray:
    """Every track of a results table in ONE device call.  gts: per video dict(poses [N,4,4] or pose sequence, w, h, sym_axis or None,
    gt_scale (default 0.15), dts (default linspace(1, N / 2, 10) as eval_videos.py:186)); tracks: per cell dict(video = index into gts,
    poses, scale) or None for a cell that could not be loaded -> f64 [len(tracks), 3] (rot in degrees, proj in % of the image
    diagonal, depth), NaN rows for the None cells."""
    out = np.full((len(tracks), 3), np.nan)
    live = [i for i, t in enumerate(tracks) if t is not None]
    if not live:
        return out
    gt_T = [as_matrices(g["poses"]) for g in gts]
    Nmax = max(len(g) for g in gt_T)
    dts_v = [np.asarray(g["dts"]) if g.get("dts") is not None else np.linspace(1, len(T) / 2, num=10, dtype=int) for g, T in zip(gts, gt_T)]
    D = len(dts_v[0])
    if any(len(d) != D for d in dts_v):
        raise ValueError("video_errors_table: every video needs the same number of offsets")
    gt = np.tile(np.eye(4), (len(gts), Nmax, 1, 1))
    for v, T in enumerate(gt_T):
        gt[v, :len(T)] = T
    est = np.tile(np.eye(4), (len(live), Nmax, 1, 1))
    for m, i in enumerate(live):
        T, v = as_matrices(tracks[i]["poses"]), tracks[i]["video"]
        if len(T) != len(gt_T[v]):
            raise ValueError(f"video_errors_table: track {i} has {len(T)} poses, its video {len(gt_T[v])}")
        est[m, :len(T)] = T
    vid = [tracks[i]["video"] for i in live]
    _, final = ops.video_errors(est, gt, np.stack([dts_v[v] for v in vid]).astype(np.int64), [tracks[i]["scale"] for i in live],
                                [gts[v].get("gt_scale", GT_SCALE) for v in vid], [gts[v]["w"] for v in vid], [gts[v]["h"] for v in vid],
                                video=vid, n_frames=[len(gt_T[v]) for v in vid], sym_axis=[gts[v].get("sym_axis") for v in vid])
    out[live] = final.cpu().numpy()
    return out
