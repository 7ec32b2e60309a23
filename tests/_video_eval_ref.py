"""Test reference of the video scorer: a VECTORISED numpy / scipy fp64 restatement of the reference's src/utils/video_evaluation.py
(the per-pair Python loop costs 8 s at 130 frames), the seeded cases of tests/test_video_eval_cpu.py and tests/test_gpu_video_eval.py, the
file formats of tools/video_eval_host_check.cpp, and a writer of small data trees for the CLIs.

Rotations are built from rotation vectors, so they are orthonormal to 1e-16: scipy's `from_matrix` leaves such input alone, and its log
agrees with a plain log.  tests/golden/video_eval.npz (tools/gen_golden_video_eval.py) holds what the reference's own loops return for
`cases()`, `known_answers()` and the alignment cases."""
from __future__ import annotations

import json
import subprocess
from pathlib import Path

import numpy as np
from scipy.spatial.transform import Rotation

SYM_AXIS = np.array([0.3, -0.5, 0.81])          # not a unit vector: the reference does not normalise it
GT_SCALE = 0.15
W, H = 640, 480
LENGTHS = (2, 3, 21, 37, 130)
META_LD, PARAM_LD = 20, 16                       # csrc/video_eval_core.h FP_VE_META_LD / FP_VE_PARAM_LD


def tol(ref):
    """fp64 eps 1.1e-16 x the log map's conditioning (theta / sin(theta) <= 100 at pi - 0.01) x about 100 operations is about 1e-12;
    summation order adds at most N eps relative: three orders of margin"""
    return 1e-9 + 1e-10 * np.abs(ref)


# ---- the maps ---------------------------------------------------------------------------------------------------------------------------------
def so3_log(R):
    R = np.asarray(R, dtype=np.float64)
    return Rotation.from_matrix(R.reshape(-1, 3, 3)).as_rotvec().reshape(R.shape[:-2] + (3,))


def so3_exp(w):
    w = np.asarray(w, dtype=np.float64)
    return Rotation.from_rotvec(w.reshape(-1, 3)).as_matrix().reshape(w.shape[:-1] + (3, 3))


def sym_rotations(sym_axis, n_sym):
    if sym_axis is None:
        return np.eye(3)[None]
    return so3_exp(np.asarray(sym_axis, dtype=np.float64)[None] * np.linspace(-np.pi, np.pi, n_sym)[:, None])


# ---- video_evaluation.py, vectorised over the pairs (and the symmetries) --------------------------------------------------------------------
def rot_error_table(est, gt, dt, sym_axis=None, n_sym=101):
    """-> [pairs, symmetries] |log(R2e R1e^T) - log(R2g S R1g^T)|, and the angles of the two logs"""
    Re, Rg = est[:, :3, :3], gt[:, :3, :3]
    a = so3_log(Re[dt:] @ Re[:-dt].transpose(0, 2, 1))
    S = sym_rotations(sym_axis, n_sym)
    b = so3_log((Rg[dt:, None] @ S[None]) @ Rg[:-dt, None].transpose(0, 1, 3, 2))
    return np.linalg.norm(a[:, None] - b, axis=-1), np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1)


def get_rot_errors(est, gt, dt, sym_axis=None, N_symmetries=101):
    return rot_error_table(est, gt, dt, sym_axis, N_symmetries)[0].min(axis=1)


def project(x, w, h, K=None):
    if K is None:
        f = np.sqrt(w ** 2 + h ** 2)
        K = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1.0]])
    u = x @ np.asarray(K, dtype=np.float64).T
    return u[..., :2] / u[..., 2:]


def get_translation_errors_proj(est, gt, dt, w, h, K=None):
    pe, pg = project(est[:, :3, 3], w, h, K), project(gt[:, :3, 3], w, h, K)
    return np.linalg.norm((pe[dt:] - pe[:-dt]) - (pg[dt:] - pg[:-dt]), axis=-1)


def get_translation_errors_depth(est, gt, est_scale, gt_scale, dt):
    ne, ng = np.linalg.norm(est[:, :3, 3], axis=-1), np.linalg.norm(gt[:, :3, 3], axis=-1)
    return np.abs((ne[:-dt] / est_scale - ne[dt:] / est_scale) - (ng[:-dt] / gt_scale - ng[dt:] / gt_scale))


def align_object_origins(est, gt, scale):
    """-> (poses with the moved origin, kept frames, origin)"""
    Re, te, tg = est[:, :3, :3], est[:, :3, 3], gt[:, :3, 3]
    x = tg / np.linalg.norm(tg, axis=-1, keepdims=True) * np.linalg.norm(te, axis=-1, keepdims=True)
    o = np.einsum("nji,nj->ni", Re, x - te)
    keep = np.linalg.norm(o, axis=-1) < scale
    if not keep.any():
        return est, 0, np.zeros(3)
    origin = o[keep].mean(axis=0)
    norm = np.linalg.norm(origin)
    if norm > scale / 2.0:
        origin = origin / norm * (scale / 2.0)
    out = est.copy()
    out[:, :3, 3] = np.einsum("nij,j->ni", Re, origin) + te
    return out, int(keep.sum()), origin


def offsets(N):
    return np.linspace(1, N / 2, num=10, dtype=int)


def score_track(est, gt, est_scale, gt_scale=GT_SCALE, w=W, h=H, sym_axis=None, n_sym=101, K=None, dts=None):
    """-> per_offset [D,3] (mean over the pairs / dt for rot, proj, depth), final [3] (rot in degrees, proj in % of the diagonal)"""
    dts = offsets(len(est)) if dts is None else np.asarray(dts)
    moved = align_object_origins(est, gt, est_scale)[0]
    per = np.array([[get_rot_errors(est, gt, dt, sym_axis, n_sym).mean() / dt,
                     get_translation_errors_proj(moved, gt, dt, w, h, K).mean() / dt,
                     get_translation_errors_depth(moved, gt, est_scale, gt_scale, dt).mean() / dt] for dt in dts])
    mean = per.mean(axis=0)
    return per, np.array([np.rad2deg(mean[0]), mean[1] / np.sqrt(w ** 2 + h ** 2) * 100, mean[2]])


def score(track):
    return score_track(track["est"], track["gt"], track["est_scale"], track["gt_scale"], track["w"], track["h"], track["sym_axis"],
                       track["n_sym"], track.get("K"))


# ---- seeded cases -----------------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def poses(R, t):
    T = np.tile(np.eye(4), (len(R), 1, 1))
    T[:, :3, :3], T[:, :3, 3] = R, t
    return T


def estimate(gt, rng):
    """0.1 rad of rotation noise, 5 mm of translation noise and an object origin that sits 2 cm off (what the alignment is for)"""
    N, Rg, tg = len(gt), gt[:, :3, :3], gt[:, :3, 3]
    Re = so3_exp(so3_log(Rg @ so3_exp(0.1 * _unit(rng, N) * rng.uniform(0.2, 1.0, (N, 1)))))
    te = tg + np.einsum("nij,j->ni", Re, np.array([0.012, -0.01, 0.013])) + 0.005 * rng.standard_normal((N, 3))
    return poses(Re, te)


def trajectory(seed, N):
    """-> (estimate, ground truth): the ground truth is a random walk of 0.05 rad per frame in front of the camera"""
    rng = np.random.Generator(np.random.PCG64(seed))
    steps = so3_exp(0.05 * _unit(rng, N))
    Rg = np.empty((N, 3, 3))
    Rg[0] = so3_exp(rng.standard_normal(3))
    for i in range(1, N):
        Rg[i] = so3_exp(so3_log(Rg[i - 1] @ steps[i]))                     # back through a rotation vector: orthonormal to 1e-16
    tg = np.array([0.05, -0.03, 0.8]) + np.cumsum(0.004 * rng.standard_normal((N, 3)), axis=0)
    gt = poses(Rg, tg)
    return estimate(gt, rng), gt


def track(est, gt, sym_axis=None, n_sym=101, est_scale=0.17, gt_scale=GT_SCALE, w=W, h=H, K=None, video=0):
    return dict(est=est, gt=gt, sym_axis=None if sym_axis is None else np.asarray(sym_axis, dtype=np.float64), n_sym=n_sym,
                est_scale=est_scale, gt_scale=gt_scale, w=w, h=h, K=K, video=video)


def cases():
    """name -> track: every length with and without the symmetry axis (seed = position of the length), the grid sizes 1, 64, 65 at 21
    frames, and one track with an explicit K"""
    out = {}
    for seed, N in enumerate(LENGTHS):
        est, gt = trajectory(seed % 3, N)
        out[f"N{N}"] = track(est, gt)
        out[f"N{N}_sym"] = track(est, gt, SYM_AXIS)
    est, gt = trajectory(2, 21)
    for n in (1, 64, 65):
        out[f"N21_sym{n}"] = track(est, gt, SYM_AXIS, n_sym=n)
    K = np.array([[700.0, 0.5, 310.0], [0, 705.0, 250.0], [0, 0, 1]])
    out["N21_K"] = track(est, gt, K=K)
    return out


def mixed_batch():
    """M = 7 tracks over V = 5 ground-truth trajectories of all five lengths; two tracks share video 3, two video 4 -> (tracks, gts)"""
    gts, tracks = [], []
    for v, N in enumerate(LENGTHS):
        est, gt = trajectory(v % 3, N)
        gts.append(gt)
        tracks.append(track(est, gt, SYM_AXIS if v % 2 == 0 else None, video=v))
        if N == 37:                                                       # another method's estimate of the same video
            tracks.append(track(estimate(gt, np.random.Generator(np.random.PCG64(1000))), gt, None, est_scale=0.2, video=v))
    tracks.append(track(estimate(gts[4], np.random.Generator(np.random.PCG64(1001))), gts[4], SYM_AXIS, n_sym=65, est_scale=0.12, video=4))
    assert len(tracks) == 7 and len(gts) == 5
    return tracks, gts


def conditions(t, n_check=100):
    """what the reference's result silently depends on: -> (largest angle of log(R2e R1e^T) and of every minimising log(R2g S R1g^T),
    smallest gap between the best and the second-best symmetry among the first `n_check` grid points)"""
    worst, gap = 0.0, np.inf
    for dt in np.unique(offsets(len(t["est"]))):
        e, na, nb = rot_error_table(t["est"], t["gt"], dt, t["sym_axis"], t["n_sym"])
        best = e.argmin(axis=1)
        worst = max(worst, na.max(), nb[np.arange(len(best)), best].max())
        if t["sym_axis"] is not None and e.shape[1] >= 2:
            s = np.sort(e[:, :min(n_check, e.shape[1])], axis=1)
            gap = min(gap, (s[:, 1] - s[:, 0]).min())
    return worst, gap


def known_answers():
    """name -> track whose rot error is known: est == gt; est = gt C (a constant rotation on the object side); est = gt exp(axis 2 pi k_t /
    100) with random integers k_t, scored with and without the axis"""
    rng = np.random.Generator(np.random.PCG64(11))
    _, gt = trajectory(1, 37)
    Rg, tg = gt[:, :3, :3], gt[:, :3, 3]
    C = so3_exp(np.array([0.4, -0.7, 0.2]))
    k = rng.integers(0, 31, len(gt))          # |k2 - k1| <= 30: the relative spin stays on the grid's [-pi, pi] and 1.9 rad at most
    spin = so3_exp(SYM_AXIS[None] * (2 * np.pi * k / 100)[:, None])
    Rs = so3_exp(so3_log(Rg @ spin))
    return {"same": track(gt.copy(), gt, est_scale=GT_SCALE), "same_sym": track(gt.copy(), gt, SYM_AXIS, est_scale=GT_SCALE),
            "const": track(poses(so3_exp(so3_log(Rg @ C)), tg), gt),
            "spin_sym": track(poses(Rs, tg), gt, SYM_AXIS), "spin_nosym": track(poses(Rs, tg), gt)}


def alignment_cases():
    """name -> (track, expected branch): every frame rejected, the mean clamped to scale / 2, the mean not clamped"""
    est, gt = trajectory(0, 21)
    far = est.copy()
    far[:, :3, 3] += np.array([0.5, 0.4, 0.0])                              # |o| = 0.6 m >= scale: no frame is kept
    return {"rejected": (track(far, gt, est_scale=0.17), "rejected"),
            "clamped": (track(est, gt, est_scale=0.03), "clamped"),         # |o| ~ 0.02 < 0.03, mean 0.02 > 0.015
            "free": (track(est, gt, est_scale=0.17), "free")}


# ---- the formats of tools/video_eval_host_check.cpp and of fp_video_errors' host tables -------------------------------------------------------
def flat12(T):
    return np.concatenate([T[:, :3, :3].reshape(len(T), 9), T[:, :3, 3]], axis=1).astype(np.float64)


def tables(tracks, dts=None):
    """-> meta i32 [M,20], params f64 [M,16], D"""
    M = len(tracks)
    meta, params = np.zeros((M, META_LD), np.int32), np.zeros((M, PARAM_LD), np.float64)
    D = 10 if dts is None else len(dts[0])
    for m, t in enumerate(tracks):
        d = offsets(len(t["est"])) if dts is None else dts[m]
        meta[m, :4] = [t["video"], len(t["est"]), t["n_sym"], (t["sym_axis"] is not None) + 2 * (t.get("K") is not None)]
        meta[m, 4:4 + D] = d
        params[m, :4] = [t["est_scale"], t["gt_scale"], t["w"], t["h"]]
        if t["sym_axis"] is not None:
            params[m, 4:7] = t["sym_axis"]
        if t.get("K") is not None:
            params[m, 7:16] = np.asarray(t["K"]).ravel()
    return meta, params, D


def run_host_check(exe, tmp, tracks, gts):
    """-> per track dict(per_offset [D,3], final [3], kept, origin [3], aligned [N,3]); asserts exit status 0 (under the sanitizers)"""
    meta, params, D = tables(tracks)
    fin, fout = Path(tmp) / "in.bin", Path(tmp) / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.array([len(tracks), len(gts), D], np.int32).tobytes())
        for g in gts:
            f.write(np.array([len(g)], np.int32).tobytes() + flat12(g).tobytes())
        for m, t in enumerate(tracks):
            f.write(meta[m].tobytes() + params[m].tobytes() + flat12(t["est"]).tobytes())
    r = subprocess.run([str(exe), "errors", str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(fout, np.float64)
    out, p = [], 0
    for t in tracks:
        N = len(t["est"])
        n = D * 3 + 7 + N * 3
        c = raw[p:p + n]
        out.append(dict(per_offset=c[:D * 3].reshape(D, 3), final=c[D * 3:D * 3 + 3], kept=int(c[D * 3 + 3]), origin=c[D * 3 + 4:D * 3 + 7],
                        aligned=c[D * 3 + 7:].reshape(N, 3)))
        p += n
    assert p == len(raw)
    return out


def run_host_so3(exe, tmp, R):
    """-> log R [n,3], exp(log R) [n,3,3]"""
    fin, fout = Path(tmp) / "so3_in.bin", Path(tmp) / "so3_out.bin"
    R = np.ascontiguousarray(R, dtype=np.float64).reshape(-1, 9)
    with open(fin, "wb") as f:
        f.write(np.array([len(R)], np.int32).tobytes() + R.tobytes())
    r = subprocess.run([str(exe), "so3", str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = np.fromfile(fout, np.float64).reshape(len(R), 12)
    return raw[:, :3], raw[:, 3:].reshape(-1, 3, 3)


# ---- data trees for the CLIs ------------------------------------------------------------------------------------------------------------------
def _vec(a):
    return " ".join(repr(float(x)) for x in np.asarray(a).ravel())


def gt_boxes(N, seed):
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    xy = np.array([200, 150]) + np.cumsum(rng.integers(-3, 4, (N, 2)), axis=0)
    return [np.array([x, y, 80, 60]) for x, y in xy]                        # [x, y, w, h] as bbox_iou reads them


def write_gt(data, video, gt, boxes, sym_axis=None, ann_id=1):
    d = {"poses": gt, "mesh_id": "mesh0", "focal_length": 600.0, "bboxes": boxes}
    if sym_axis is not None:
        d["sym_axis"] = np.asarray(sym_axis)
    path = Path(data) / "video_gt"
    path.mkdir(parents=True, exist_ok=True)
    np.save(path / f"{video}_poses_id{ann_id}.npy", d, allow_pickle=True)


def write_pred_csv(path, est, boxes, scale, decoys=0, best_at=0, box_shift=0, scales=None):
    """one row per (frame, object): `decoys` other objects per frame with boxes far from the ground truth's, the real one at position
    `best_at`; `box_shift` moves the real object's boxes (a low IoU)"""
    rows = ["scene_id,im_id,obj_id,score,R,t,bbox_visib,scale,time"]
    rng = np.random.Generator(np.random.PCG64(5))
    for i, T in enumerate(est):
        for j in range(decoys + 1):
            if j == best_at:
                b = boxes[i] + np.array([box_shift, 0, 0, 0])
                R, t = T[:3, :3], T[:3, 3]
            else:
                b = boxes[i] + np.array([150 * (j + 1), 90, 10, -5])
                R, t = so3_exp(rng.standard_normal(3)), T[:3, 3] + 0.1 * rng.standard_normal(3)
            s = scale if scales is None else scales[i]
            rows.append(f"0,{i},mesh0,1.0,{_vec(R)},{_vec(t)},{' '.join(str(int(x)) for x in b)},{s!r},0.0")
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text("\n".join(rows) + "\n")


def write_frames(data, video, w, h, n=2):
    """2 x 2-pixel content is all the scorer needs of a frame: its size.  Written at (h, w) with PIL."""
    from PIL import Image
    d = Path(data) / "datasets" / "videos" / video
    d.mkdir(parents=True, exist_ok=True)
    for i in range(n):
        Image.new("RGB", (w, h)).save(d / f"{i:06d}.png")


def write_proposals(path, boxes, n_obj=3, best_at=1):
    """the proposals JSON filter_predictions reads: n_obj entries per frame, frame-major"""
    out = []
    for i, b in enumerate(boxes):
        for j in range(n_obj):
            bb = b if j == best_at else b + np.array([120 * (j + 1), 40, 5, 5])
            out.append({"image_id": i, "bbox": [int(x) for x in bb], "score": 0.9 - 0.1 * j, "category_id": j})
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text(json.dumps(out))
    return out
