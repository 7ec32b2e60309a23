"""Writes tests/golden/bop_scores.npz: what the reference's own matching and scoring return on the cases of tests/_bop_score_ref.py.

    python tools/gen_golden_bop_scores.py [path to the reference's bop_toolkit folder]

Runs on the CPU.  Imports bop_toolkit_lib.pose_matching (match_poses, match_poses_scene), score (calc_localization_scores), inout
(save_json) and misc (get_score_signature); imageio, png and trimesh, which inout imports and these functions do not use, are stubbed
when missing.  The glue between them lives in the body of the reference's scripts/eval_calc_scores.py (:192-283: organising the targets,
the validity of the ground truths, the two normalisations), which cannot be imported; it is taken from the restatement
(tests/_bop_score_ref.py: organize_targets, gt_valid, normalised_errs), so the golden pins the matching, the counting and the text, and
the validity rule is pinned by the hand-worked expectations of tests/test_bop_scores_cpu.py.

The file holds data only, as one JSON string in a compressed npz:
  tables    name -> match [T][R], tp_obj, tp_scene, tar_obj, tar_scene from match_poses run per group and threshold
  datasets  name -> per threshold {th, sign, scores_text, matches_text}: the text inout.save_json wrote for the scores dict and the match
            list of calc_localization_scores / match_poses_scene
"""
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tests import _bop_score_ref as ref  # noqa: E402  (before the toolkit is on the path: it has a `tests` package of its own)

REF = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("/root/reference/bop_toolkit")
sys.path.insert(0, str(REF))
for missing in ("imageio", "png", "trimesh"):
    try:
        __import__(missing)
    except ImportError:
        sys.modules[missing] = types.ModuleType(missing)

from bop_toolkit_lib import inout, misc, pose_matching, score  # noqa: E402


def saved_text(content, tmp):
    p = Path(tmp) / "x.json"
    inout.save_json(str(p), content)
    return p.read_text()


def table_golden(t):
    T, R = len(t["th"]), len(t["gt_valid"])
    match = np.full((T, R), -1, int)
    tp_obj, tp_scene = np.zeros((T, t["n_obj"]), int), np.zeros((T, t["n_scene"]), int)
    tar_obj, tar_scene = np.zeros(t["n_obj"], int), np.zeros(t["n_scene"], int)
    for off, E, G, first in t["groups"].tolist():
        if G == 0:
            continue
        o, s = int(t["gt_obj"][first]), int(t["gt_scene"][first])
        mask = [bool(v) for v in t["gt_valid"][first:first + G]]
        n = sum(mask)
        tar = int(np.minimum(t["n_top"], n)) if t["n_top"] > 0 else n         # score.py:92-95
        tar_obj[o] += tar
        tar_scene[s] += tar
        errs = [{"est_id": e, "score": float(-e), "errors": {g: [float(t["err"][off + e * G + g])] for g in range(G)}} for e in range(E)]
        for ti, th in enumerate(t["th"].tolist()):
            for m in pose_matching.match_poses(errs, [th], 0, mask):
                match[ti, first + m["gt_id"]] = m["est_id"]
                tp_obj[ti, o] += 1
                tp_scene[ti, s] += 1
    return {"match": match.tolist(), "tp_obj": tp_obj.tolist(), "tp_scene": tp_scene.tolist(), "tar_obj": tar_obj.tolist(),
            "tar_scene": tar_scene.tolist()}


def dataset_golden(case, tmp):
    out = []
    for th in case["thresholds"]:
        matches = []
        for scene_id, scene_targets in ref.organize_targets(case["targets"]).items():
            gt_curr = {im: case["scene_gt"][scene_id][im] for im in scene_targets}
            valid = {im: ref.gt_valid(case["scene_gt"][scene_id][im], case["scene_gt_info"][scene_id][im], t, case["visib_gt_min"])
                     for im, t in scene_targets.items()}
            matches += pose_matching.match_poses_scene(scene_id, gt_curr, valid, ref.normalised_errs(case, scene_id), [th], case["n_top"])
        scores = score.calc_localization_scores(case["scene_ids"], case["obj_ids"], matches, case["n_top"], do_print=False)
        out.append({"th": th, "sign": misc.get_score_signature([th], case["visib_gt_min"]), "scores_text": saved_text(scores, tmp),
                    "matches_text": saved_text(matches, tmp)})
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        gold = {"tables": {k: table_golden(t) for k, t in ref.table_cases().items()},
                "datasets": {k: dataset_golden(c, tmp) for k, c in ref.dataset_cases().items()}}
    path = ROOT / "tests" / "golden" / "bop_scores.npz"
    np.savez_compressed(path, json=np.array(json.dumps(gold, separators=(",", ":"))))      # one JSON string, deflated
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
