"""python -m scripts.eval_calc_scores --error_dir_paths method_ycbv-test/error=cus_ntop=-1 --correct_th_cus "0.05;0.1;0.15" --eval_path data/evals

Counterpart of bop_toolkit/scripts/eval_calc_scores.py: turns the `errors_<scene>.json` files of `scripts.eval_calc_errors` into
`scores_<sign>.json` and `matches_<sign>.json`, with the reference's flags, defaults, path templates, keys and text layout.  The greedy
matching of estimates to ground truths and the recall counts run on the device (csrc/bop_score.hip through
freepose_amd.evaluation.BopScorer), for every threshold of an errors directory in one call.

What differs from the reference script:
  * `--correct_th_<type>` may hold several thresholds separated by `;`: each writes its own scores_ / matches_ pair.  A single
    comma-separated value means what it means there (one score with one threshold per error element; only one-element errors are scored
    here, so `rete` is refused).
  * the scene list of the split and the object list come from the dataset on disk instead of the toolkit's dataset_params.py: the numeric
    scene folders under the split directory (or `--scene_ids`), the keys of models_eval/models_info.json (or `--obj_ids`); the image width
    is read from an image of the first targeted scene.  On a complete dataset these are the lists and the width dataset_params holds.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from pathlib import Path

from freepose_amd.evaluation import (BOP_NORMALIZED_BY_DIAMETER, BOP_NORMALIZED_BY_IM_WIDTH, BopScorer, bop_json_text, score_signature)
from freepose_amd.scripts.eval_calc_errors import _image_size, load_json, log

CORRECT_TH = {"vsd": [0.3], "mssd": [0.2], "chamfer": [0.2], "chamfer_proj": [10.0], "mspd": [10], "cus": [0.5], "rete": [5.0, 5.0], "re": [5.0],
              "te": [5.0], "proj": [5.0], "ad": [0.1], "add": [0.1], "adi": [0.1]}                  # eval_calc_scores.py:39-53
ERROR_TPATH = os.path.join("{eval_path}", "{error_dir_path}", "errors_{scene_id:06d}.json")
OUT_MATCHES_TPATH = os.path.join("{eval_path}", "{error_dir_path}", "matches_{score_sign}.json")
OUT_SCORES_TPATH = os.path.join("{eval_path}", "{error_dir_path}", "scores_{score_sign}.json")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    for err_type, th in CORRECT_TH.items():
        ap.add_argument("--correct_th_" + err_type, default=",".join(map(str, th)),
                        help="threshold of correctness; several scores: thresholds separated by ';'")
    ap.add_argument("--normalized_by_diameter", default=",".join(BOP_NORMALIZED_BY_DIAMETER))
    ap.add_argument("--normalized_by_im_width", default=",".join(BOP_NORMALIZED_BY_IM_WIDTH))
    ap.add_argument("--visib_gt_min", default=-1)
    ap.add_argument("--error_dir_paths", default="/path/to/calculated/errors", help="Comma-sep. paths to errors from eval_calc_errors.py.")
    ap.add_argument("--eval_path", default=os.getcwd())
    ap.add_argument("--datasets_path", default=os.environ.get("BOP_PATH", "bop_datasets"))
    ap.add_argument("--targets_filename", default="test_targets_bop19.json")
    ap.add_argument("--error_tpath", default=ERROR_TPATH)
    ap.add_argument("--out_matches_tpath", default=OUT_MATCHES_TPATH)
    ap.add_argument("--out_scores_tpath", default=OUT_SCORES_TPATH)
    ap.add_argument("--scene_ids", default="", help="comma-sep. scenes the recalls are listed for (default: the scene folders of the split)")
    ap.add_argument("--obj_ids", default="", help="comma-sep. objects the recalls are listed for (default: the keys of models_info.json)")
    return ap


def params_from_args(args) -> dict:
    a = vars(args)
    return {
        # per error type a list of scores, each a list with one threshold per error element
        "correct_th": {t: [list(map(float, one.split(","))) for one in str(a["correct_th_" + t]).split(";")] for t in CORRECT_TH},
        "normalized_by_diameter": str(args.normalized_by_diameter).split(","),
        "normalized_by_im_width": str(args.normalized_by_im_width).split(","),
        "visib_gt_min": float(args.visib_gt_min),
        "error_dir_paths": str(args.error_dir_paths).split(","),
        "eval_path": str(args.eval_path), "datasets_path": str(args.datasets_path), "targets_filename": str(args.targets_filename),
        "error_tpath": str(args.error_tpath), "out_matches_tpath": str(args.out_matches_tpath), "out_scores_tpath": str(args.out_scores_tpath),
        "scene_ids": [int(s) for s in str(args.scene_ids).split(",") if s], "obj_ids": [int(s) for s in str(args.obj_ids).split(",") if s],
    }


def parse_error_dir(error_dir_path):
    """(error type, n_top, method, dataset, split, split_type) from the folder names (eval_calc_scores.py:154-166)"""
    error_sign = os.path.basename(error_dir_path)
    if "chamfer_proj" not in error_sign:
        err_type = str(error_sign.split("_")[0].split("=")[1])
        n_top = int(error_sign.split("_")[1].split("=")[1])
    else:
        err_type = "chamfer_proj"
        n_top = int(error_sign.split("_")[2].split("=")[1])
    result_info = os.path.basename(os.path.dirname(error_dir_path)).split("_")
    dataset_info = result_info[1].split("-")
    return err_type, n_top, result_info[0], dataset_info[0], dataset_info[1], (dataset_info[2] if len(dataset_info) > 2 else None)


class Dataset:
    """what the scoring reads of a BOP dataset on disk, loaded once per (dataset, split): targets, GT and GT info of the targeted scenes,
    models_info, the scene and object lists, the image width"""

    def __init__(self, datasets_path, dataset, split, split_type, targets_filename, scene_ids=(), obj_ids=()):
        base = Path(datasets_path) / dataset
        self.split_path = base / (split + ("_" + split_type if split_type else ""))
        self.models_info = load_json(base / "models_eval" / "models_info.json", keys_to_int=True)
        self.targets = load_json(base / targets_filename)
        self.scene_gt, self.scene_gt_info = {}, {}
        for t in self.targets:
            s = t["scene_id"]
            if s not in self.scene_gt:
                self.scene_gt[s] = load_json(self.split_path / f"{s:06d}" / "scene_gt.json", keys_to_int=True)
                self.scene_gt_info[s] = load_json(self.split_path / f"{s:06d}" / "scene_gt_info.json", keys_to_int=True)
        self.scene_ids = list(scene_ids) or sorted(int(d.name) for d in self.split_path.iterdir() if d.is_dir() and d.name.isdigit())
        self.obj_ids = list(obj_ids) or sorted(self.models_info)
        self._width = None

    @property
    def im_width(self):
        if self._width is None:
            t = self.targets[0]
            self._width = _image_size(self.split_path, t["scene_id"], t["im_id"])[0]
        return self._width

    def scorer(self, visib_gt_min) -> BopScorer:
        return BopScorer(self.targets, self.scene_gt, self.scene_gt_info, self.obj_ids, self.scene_ids, visib_gt_min)


def score_error_dir(error_dir_path, p, correct_ths, ds: Dataset = None, scorer: BopScorer = None) -> list:
    """scores and matches of one errors directory for every entry of correct_ths ([[th], ...]), one device call; writes the files and
    returns [(scores path, scores dict)]"""
    t0 = time.time()
    err_type, n_top, method, dataset, split, split_type = parse_error_dir(error_dir_path)
    if any(len(th) != 1 for th in correct_ths):
        raise ValueError(f"{err_type}: a score with {max(len(th) for th in correct_ths)} thresholds; only one-element errors are scored here "
                         "(separate the thresholds of several scores with ';')")
    log("Calculating score - error: {}, method: {}, dataset: {}.".format(err_type, method, dataset))
    if ds is None:
        ds = Dataset(p["datasets_path"], dataset, split, split_type, p["targets_filename"], p.get("scene_ids", ()), p.get("obj_ids", ()))
    if scorer is None:
        scorer = ds.scorer(p["visib_gt_min"])
    errs = {}
    for scene_id in ds.scene_gt:                             # the scenes of the targets, each errors file read once
        errs[scene_id] = load_json(p["error_tpath"].format(eval_path=p["eval_path"], error_dir_path=error_dir_path, scene_id=scene_id),
                                   keys_to_int=True)
    diameters = {k: v["diameter"] for k, v in ds.models_info.items()} if err_type in p["normalized_by_diameter"] else None
    im_width = ds.im_width if err_type in p["normalized_by_im_width"] else None
    results = scorer.scores(errs, err_type, [th[0] for th in correct_ths], n_top, diameters=diameters, im_width=im_width)
    out = []
    for th, (scores, matches) in zip(correct_ths, results):
        sign = score_signature(th, p["visib_gt_min"])
        scores_path = p["out_scores_tpath"].format(eval_path=p["eval_path"], error_dir_path=error_dir_path, score_sign=sign)
        matches_path = p["out_matches_tpath"].format(eval_path=p["eval_path"], error_dir_path=error_dir_path, score_sign=sign)
        for path, content in ((scores_path, scores), (matches_path, matches)):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                f.write(bop_json_text(content))
        log("th {}: recall {:.4f} (targets {:d}, tp {:d}) -> {}".format(th[0], scores["recall"], scores["targets_count"], scores["tp_count"],
                                                                       scores_path))
        out.append((scores_path, scores))
    log("Matching and score calculation took {}s.".format(time.time() - t0))
    return out


def run(argv=None):
    p = params_from_args(build_parser().parse_args(argv))
    out = []
    for error_dir_path in p["error_dir_paths"]:
        log("Processing: {}".format(error_dir_path))
        err_type = parse_error_dir(error_dir_path)[0]
        if err_type not in p["correct_th"]:
            sys.exit("no threshold of correctness for error type '{}'".format(err_type))
        out += score_error_dir(error_dir_path, p, p["correct_th"][err_type])
    log("Done.")
    return out


main = run

if __name__ == "__main__":
    run()
