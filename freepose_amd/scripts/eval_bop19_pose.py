"""python -m scripts.eval_bop19_pose --result_filenames method_ycbv-test.csv --results_path . --eval_path data/evals

Counterpart of bop_toolkit/scripts/eval_bop19_pose.py for the errors of the FreePose paper: for every results CSV it scores `cus`
(thresholds 0.05 ... 0.5), `chamfer` (0.05 ... 0.5) and `chamfer_proj` (5 ... 50), n_top = -1, and writes
`<eval_path>/<result name>/scores_bop19.json` with bop19_average_recall_<type>, bop19_average_recall (the mean over the types computed)
and bop19_average_time_per_image (:133-157: -1 when an estimate has no time, ValueError when the times of one image differ).

The reference starts one Python process per (error type, threshold) — 30 for this table — and each reloads the targets, the ground truth
and the errors.  Here everything runs in this process: the dataset is loaded once, the errors that are not yet on disk are computed by
`scripts.eval_calc_errors.evaluate_result_file` (`--reuse_errors 0` recomputes them), each errors directory is read once and all its
thresholds are matched in one device call (`scripts.eval_calc_scores.score_error_dir`), which writes every scores_*.json and
matches_*.json the reference would.  With SLURM_JOB_ID > 0 only the errors are computed, as there (:163-193).

`--errors` selects a subset of cus,chamfer,chamfer_proj or adds `vsd` (the reference's commented-out entry: delta per dataset, taus
0.05 ... 0.5, one errors directory per tau, thresholds 0.05 ... 0.5).  `--renderer_type` is accepted and ignored.
"""
from __future__ import annotations

import argparse
import os
from pathlib import Path

import numpy as np

from freepose_amd.evaluation import bop_json_text
from freepose_amd.scripts import eval_calc_errors as calc_errors
from freepose_amd.scripts import eval_calc_scores as calc_scores
from freepose_amd.scripts.eval_calc_errors import log

VISIB_GT_MIN = -1
ERRORS = {                                                  # eval_bop19_pose.py:34-69
    "cus": {"n_top": -1, "type": "cus", "correct_th": [[th] for th in np.arange(0.05, 0.51, 0.05)]},
    "chamfer": {"n_top": -1, "type": "chamfer", "correct_th": [[th] for th in np.arange(0.05, 0.51, 0.05)]},
    "chamfer_proj": {"n_top": -1, "type": "chamfer_proj", "correct_th": [[th] for th in np.arange(5, 51, 5)]},
    "vsd": {"n_top": -1, "type": "vsd", "vsd_deltas": dict(calc_errors.VSD_DELTAS), "vsd_taus": list(np.arange(0.05, 0.51, 0.05)),
            "vsd_normalized_by_diameter": True, "correct_th": [[th] for th in np.arange(0.05, 0.51, 0.05)]},
}
DEFAULT_ERRORS = ("cus", "chamfer", "chamfer_proj")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--renderer_type", default="vispy", help="accepted with any value and ignored")
    ap.add_argument("--result_filenames", default="/relative/path/to/csv/with/results", help="Comma-separated names of files with results.")
    ap.add_argument("--results_path", default=os.getcwd())
    ap.add_argument("--eval_path", default=os.getcwd())
    ap.add_argument("--targets_filename", default="test_targets_bop19.json")
    ap.add_argument("--errors", default=",".join(DEFAULT_ERRORS), help="comma-sep. error types out of: " + ", ".join(ERRORS))
    ap.add_argument("--reuse_errors", default=1, help="1: errors files already on disk are used as they are; 0: recompute them")
    ap.add_argument("--models_inference_path", default=os.environ.get("BOP_MODELS_INFERENCE_PATH", "models_normalized"))
    ap.add_argument("--datasets_path", default=os.environ.get("BOP_PATH", "bop_datasets"))
    ap.add_argument("--scene_ids", default="", help="as in scripts.eval_calc_scores")
    ap.add_argument("--obj_ids", default="", help="as in scripts.eval_calc_scores")
    return ap


def average_time_per_image(ests) -> float:
    """eval_bop19_pose.py:137-157"""
    times = {}
    for est in ests:
        key = "{:06d}_{:06d}".format(est["scene_id"], est["im_id"])
        if est["time"] < 0:
            return -1.0                                      # all estimation times must be provided
        if key in times:
            if abs(times[key] - est["time"]) > 0.001:
                raise ValueError("The running time for scene {} and image {} is not the same for all estimates.".format(
                    est["scene_id"], est["im_id"]))
        else:
            times[key] = est["time"]
    return np.mean(list(times.values()))


def _error_params(args, error) -> dict:
    argv = ["--n_top={}".format(error["n_top"]), "--error_type={}".format(error["type"]), "--result_filenames={}".format(args.result_filenames),
            "--renderer_type={}".format(args.renderer_type), "--results_path={}".format(args.results_path),
            "--eval_path={}".format(args.eval_path), "--targets_filename={}".format(args.targets_filename), "--skip_missing=1",
            "--models_inference_path={}".format(args.models_inference_path), "--datasets_path={}".format(args.datasets_path)]
    if error["type"] == "vsd":
        argv += ["--vsd_deltas={}".format(",".join("{}:{}".format(k, v) for k, v in error["vsd_deltas"].items())),
                 "--vsd_taus={}".format(",".join(map(str, error["vsd_taus"]))),
                 "--vsd_normalized_by_diameter={}".format(error["vsd_normalized_by_diameter"])]
    return calc_errors.params_from_args(calc_errors.build_parser().parse_args(argv))


def _error_signs(error, dataset) -> list:
    if error["type"] == "vsd":
        return [calc_errors.error_signature("vsd", error["n_top"], vsd_delta=error["vsd_deltas"][dataset], vsd_tau=tau) for tau in error["vsd_taus"]]
    return [calc_errors.error_signature(error["type"], error["n_top"])]


def evaluate(result_filename, args, errors) -> dict:
    """one results CSV -> the final scores (None under SLURM_JOB_ID > 0, where only the errors are computed)"""
    log("===========")
    log("EVALUATING: {}".format(result_filename))
    log("===========")
    result_name, _, dataset, split, split_type = calc_errors.split_result_name(result_filename)
    ests = calc_errors.load_results_csv(os.path.join(str(args.results_path), result_filename))
    time_per_image = average_time_per_image(ests)
    slurm_job_id = int(os.environ.get("SLURM_JOB_ID", -1))
    sp = {"visib_gt_min": float(VISIB_GT_MIN), "eval_path": str(args.eval_path), "error_tpath": calc_scores.ERROR_TPATH,
          "out_matches_tpath": calc_scores.OUT_MATCHES_TPATH, "out_scores_tpath": calc_scores.OUT_SCORES_TPATH,
          "normalized_by_diameter": list(calc_scores.BOP_NORMALIZED_BY_DIAMETER),
          "normalized_by_im_width": list(calc_scores.BOP_NORMALIZED_BY_IM_WIDTH)}
    ds = scorer = None
    average_recalls = {}
    for error in errors:
        ep = _error_params(args, error)
        if slurm_job_id > 0:
            calc_errors.evaluate_result_file(result_filename, ep)
            continue
        if ds is None:                                       # the dataset, the groups and the validity: once for all error types
            ds = calc_scores.Dataset(str(args.datasets_path), dataset, split, split_type, str(args.targets_filename),
                                     [int(s) for s in str(args.scene_ids).split(",") if s], [int(s) for s in str(args.obj_ids).split(",") if s])
            scorer = ds.scorer(sp["visib_gt_min"])
        error_dir_paths = [os.path.join(result_name, sign) for sign in _error_signs(error, dataset)]
        on_disk = all(Path(sp["error_tpath"].format(eval_path=sp["eval_path"], error_dir_path=d, scene_id=s)).exists()
                      for d in error_dir_paths for s in ds.scene_gt)
        if not on_disk or not int(args.reuse_errors):
            calc_errors.evaluate_result_file(result_filename, ep)
        else:
            log("Errors of {} are on disk: reused.".format(error["type"]))
        recalls = []
        correct_ths = [[float(t) for t in th] for th in error["correct_th"]]
        for d in error_dir_paths:
            recalls += [scores["recall"] for _, scores in calc_scores.score_error_dir(d, sp, correct_ths, ds, scorer)]
        average_recalls[error["type"]] = np.mean(recalls)
        log("Recall scores: {}".format(" ".join(map(str, recalls))))
        log("Average recall: {}".format(average_recalls[error["type"]]))
    if slurm_job_id != -1:
        return None
    final_scores = {"bop19_average_recall_{}".format(e["type"]): average_recalls[e["type"]] for e in errors}
    log("AR over errors: {}".format(list(average_recalls.keys())))
    final_scores["bop19_average_recall"] = np.mean([e for e in average_recalls.values()])
    final_scores["bop19_average_time_per_image"] = time_per_image
    path = os.path.join(str(args.eval_path), result_name, "scores_bop19.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(bop_json_text(final_scores))
    log("FINAL SCORES:")
    for name, value in final_scores.items():
        log("- {}: {}".format(name, value))
    return final_scores


def run(argv=None):
    args = build_parser().parse_args(argv)
    names = [e for e in str(args.errors).split(",") if e]
    unknown = [e for e in names if e not in ERRORS]
    if unknown or not names:
        raise SystemExit("--errors: unknown error type(s) {}; choose from {}".format(unknown, ", ".join(ERRORS)))
    out = {}
    for result_filename in str(args.result_filenames).split(","):
        out[result_filename] = evaluate(result_filename, args, [ERRORS[e] for e in names])
    log("Done.")
    return out


main = run

if __name__ == "__main__":
    run()
