"""tests/golden/video_eval.npz and tests/golden/video_eval/: what the REFERENCE's own video scorer returns for the trajectories of
tests/_video_eval_ref.py, and the small CSV / JSON / npy inputs its `load_pred_csv` and `filter_predictions.main` were run on (build
container only: it imports the reference checkout through oracle.gen_golden's shims).  Arrays and inputs only.

    python -m tools.gen_golden_video_eval

Imported from the reference: src/utils/video_evaluation.py (every function), scripts/eval_videos.py (`load_pred_csv`, `load_gt`) and
scripts/filter_predictions.py (`main`).  pinocchio is not installed here, so this file defines a stand-in module `pinocchio` with `SE3`
(rotation, translation, `*`, `actInv`), `log` and `exp` through scipy's Rotation; trimesh, loguru and tqdm are stubs (the sampled mesh
points are used by no metric).

What the fixture pins: the reference's loops — offsets, pairs, the symmetry grid and its minimum, `mean / dt`, the mean over offsets,
the degrees and image-diagonal normalisations — its alignment (kept frames, clamp, moved origin), its projection and depth formulas, the
object choice, checks and non-finite repair of `load_pred_csv`, and the JSON `filter_predictions` writes.  What it does NOT pin:
pinocchio's own `log3` near pi (its series and branch thresholds), which stays *stated* like EPnP versus OpenCV: every recorded case
keeps its logs at least 0.01 rad from pi except the n_sym = 1 case, whose only grid point is -pi.
"""
from __future__ import annotations

import importlib.util
import json
import sys
import types

import numpy as np
from scipy.spatial.transform import Rotation

from oracle.gen_golden import OUT, REF, install_shims
from tests import _video_eval_ref as ref          # imported before the shims drop the repository from sys.path


class SE3:
    def __init__(self, a, b=None):
        if b is None:
            a = np.asarray(a, dtype=np.float64)
            self.rotation, self.translation = a[:3, :3].copy(), a[:3, 3].copy()
        else:
            self.rotation, self.translation = np.asarray(a, dtype=np.float64).copy(), np.asarray(b, dtype=np.float64).copy()

    def __mul__(self, o):
        return SE3(self.rotation @ o.rotation, self.rotation @ o.translation + self.translation)

    def actInv(self, x):
        return self.rotation.T @ (np.asarray(x) - self.translation)


def pin_log(R):
    return Rotation.from_matrix(np.asarray(R)).as_rotvec()


def pin_exp(w):
    return Rotation.from_rotvec(np.asarray(w)).as_matrix()


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


class StubMesh:
    def copy(self):
        return self

    def apply_scale(self, s):
        pass

    def sample(self, n):
        return np.zeros((n, 3))


def main():
    assert REF.exists(), "the reference checkout is only present in the build container"
    install_shims()
    pin = types.ModuleType("pinocchio")
    pin.SE3, pin.log, pin.exp = SE3, pin_log, pin_exp
    sys.modules["pinocchio"] = pin
    sys.modules["trimesh"].load_mesh = lambda path: StubMesh()
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, **kw: it
    sys.modules["tqdm"] = tq
    warnings = []
    sys.modules["loguru"].logger = types.SimpleNamespace(warning=warnings.append, error=warnings.append, info=lambda *a: None)
    ve = load("utils.video_evaluation", REF / "src" / "utils" / "video_evaluation.py")
    utils = types.ModuleType("utils")
    utils.video_evaluation = ve
    sys.modules["utils"] = utils
    ev = load("ref_eval_videos", REF / "scripts" / "eval_videos.py")
    fp = load("ref_filter_predictions", REF / "scripts" / "filter_predictions.py")

    out = {}
    se3 = lambda T: [SE3(t) for t in T]   # noqa: E731

    def score(t):
        est, gt, dts = se3(t["est"]), se3(t["gt"]), ref.offsets(len(t["est"]))
        axis, n = t["sym_axis"], t["n_sym"]
        per = np.array([[np.mean(ve.get_rot_errors(est, gt, dt, sym_axis=axis, N_symmetries=n)) / dt,
                         np.mean(ve.get_translation_errors_proj(ve.align_object_origins(est, gt, t["est_scale"]), gt, dt=dt, w=t["w"],
                                                                h=t["h"], K=t["K"])) / dt,
                         np.mean(ve.get_translation_errors_depth(ve.align_object_origins(est, gt, t["est_scale"]), gt, t["est_scale"],
                                                                 t["gt_scale"], dt)) / dt] for dt in dts])
        fin = np.array([np.rad2deg(ve.get_average_rot_errors_dt(est, gt, dts=dts, sym_axis=axis, N_symmetries=n)),
                        ve.get_average_proj_errors_dt(est, gt, t["est_scale"], t["gt_scale"], dts=dts, w=t["w"], h=t["h"], K=t["K"]),
                        ve.get_average_depth_errors_dt(est, gt, t["est_scale"], t["gt_scale"], dts=dts)])
        return per, fin

    named = dict(ref.cases())
    named.update({f"known_{k}": v for k, v in ref.known_answers().items()})
    named.update({f"align_{k}": v[0] for k, v in ref.alignment_cases().items()})
    for i, t in enumerate(ref.mixed_batch()[0]):
        named[f"mixed_{i}"] = t
    for name, t in named.items():
        out[f"{name}_per_offset"], out[f"{name}_final"] = score(t)
        moved = ve.align_object_origins(se3(t["est"]), se3(t["gt"]), t["est_scale"])
        out[f"{name}_aligned"] = np.array([p.translation for p in moved])
        out[f"{name}_checksum"] = np.array([t["est"].sum(), t["gt"].sum()])
        print(name, out[f"{name}_final"], flush=True)

    # ---- load_pred_csv and filter_predictions on a small data tree (committed under tests/golden/video_eval/) ----------------------------
    tree = OUT / "video_eval"
    N = 12
    est, gt = ref.trajectory(3, N)
    boxes = ref.gt_boxes(N, 0)
    ref.write_gt(tree, "vid", gt, boxes, sym_axis=ref.SYM_AXIS)
    res = tree / "results" / "videos" / "vid"
    ref.write_pred_csv(res / "three_objects.csv", est, boxes, 0.17, decoys=2, best_at=1)
    ref.write_pred_csv(res / "low_iou.csv", est, boxes, 0.17, box_shift=60)
    bad = est.copy()
    bad[0, :3, 3] = np.nan
    bad[5, 1, 3] = np.inf
    bad[3, 0, 0] = np.nan
    ref.write_pred_csv(res / "non_finite.csv", bad, boxes, 0.17)
    ref.write_pred_csv(res / "two_scales.csv", est, boxes, 0.17, scales=[0.17] * 6 + [0.2] * 6)
    ev.DATA_PATH = tree
    g_poses, g_scale, g_axis, g_mesh, _, g_boxes = ev.load_gt("vid", 1)
    out["csv_gt_poses"], out["csv_gt_scale"], out["csv_gt_axis"] = np.array([np.vstack([np.c_[p.rotation, p.translation], [0, 0, 0, 1]])
                                                                            for p in g_poses]), np.array(g_scale), np.asarray(g_axis)
    for name in ("three_objects", "low_iou", "non_finite"):
        del warnings[:]
        pred, scale, obj_id, bbox0, _ = ev.load_pred_csv(res / f"{name}.csv", bbox=g_boxes)
        out[f"csv_{name}_R"] = np.array([p.rotation for p in pred])
        out[f"csv_{name}_t"] = np.array([p.translation for p in pred])
        out[f"csv_{name}_scale"] = np.array(scale)
        out[f"csv_{name}_bbox0"] = np.array(bbox0)
        out[f"csv_{name}_warnings"] = np.array(len(warnings))
        print(name, len(warnings), "warnings")
    try:
        ev.load_pred_csv(res / "two_scales.csv", bbox=g_boxes)
        raise SystemExit("two_scales.csv must be refused")
    except AssertionError as ex:
        out["csv_two_scales_error"] = np.array(str(ex))

    props = ref.write_proposals(res / "props.json", boxes, n_obj=3, best_at=1)
    fp.DATA_PATH = tree
    fp.main(types.SimpleNamespace(video="vid", proposals="props.json", ann_id=1))
    best = json.loads((res / "props_best_object.json").read_text())
    assert best == props[1::3]
    np.savez_compressed(OUT / "video_eval.npz", **out)
    print("wrote", OUT / "video_eval.npz", len(out), "arrays")


if __name__ == "__main__":
    main()
