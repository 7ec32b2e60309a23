"""python -m scripts.calc_model_info --dataset ycbv --model_type eval --datasets_path data/bop_datasets

Counterpart of bop_toolkit/scripts/calc_model_info.py: writes `models_info.json` of a models folder — min_x, min_y, min_z, size_x, size_y,
size_z (the 3D bounding box, :36-37) and diameter (misc.calc_pts_diameter, the largest distance between two vertices) per model.  The
reference loops over all vertex pairs in Python, which takes hours on a dense model; here all models go through one brute-force device
call in float64 whose answer is the reference's bit for bit (freepose_amd.evaluation.models_info, csrc/gt_info.hip).

`--dataset`, `--model_type` (default: the `models` folder; `eval` = `models_eval`) and `--datasets_path` (BOP_PATH) are the reference's
parameters; the other flags of `scripts.calc_gt_info` are accepted and not used.  An existing models_info.json keeps every key this
script does not compute (the `symmetries_discrete` / `symmetries_continuous` entries the dataset authors wrote by hand): only the seven
computed keys of each model are rewritten.
"""
from __future__ import annotations

import time

from freepose_amd.scripts import calc_gt_info as common
from freepose_amd.scripts.calc_gt_info import params_from_args  # noqa: F401
from freepose_amd.scripts.eval_calc_errors import load_json, log


def build_parser():
    return common.build_parser(__doc__)


def run(argv=None):
    from freepose_amd import mesh_io
    from freepose_amd.evaluation import bop_json_text, models_info
    p = params_from_args(build_parser().parse_args(argv))
    t0 = time.time()
    files = common.model_files(p)
    clouds = {}
    for obj_id, f in files.items():
        log("Processing model of object {}...".format(obj_id))
        clouds[obj_id] = mesh_io.mesh_cloud_f64(mesh_io.load_ply(f))                   # inout.load_ply: model["pts"] in float64
    path = common.models_path(p) / "models_info.json"
    info = load_json(path, keys_to_int=True) if path.exists() else {}
    for obj_id, computed in models_info(clouds).items():
        info.setdefault(obj_id, {}).update(computed)
    path.write_text(bop_json_text(info))
    log("Model info of {} models took {}s.".format(len(files), time.time() - t0))
    return str(path)


if __name__ == "__main__":
    run()
