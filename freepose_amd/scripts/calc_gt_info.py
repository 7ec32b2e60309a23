"""python -m scripts.calc_gt_info --dataset ycbv --dataset_split test --datasets_path data/bop_datasets

Counterpart of bop_toolkit/scripts/calc_gt_info.py: writes `scene_gt_info.json` of every scene of a dataset split — px_count_all,
px_count_valid, px_count_visib, visib_fract, bbox_obj, bbox_visib per ground-truth instance (:176-185) — which `scripts.eval_calc_errors`,
`scripts.eval_calc_scores` and `scripts.eval_bop19_pose` read.  The reference script has a parameter dict and needs an OpenGL renderer;
here its keys are flags with its defaults, the silhouettes come from this package's HIP rasteriser on the reference's 3W x 3H canvas
(:70-74), and the counts, boxes and the visibility test of all instances of many images are one fused device pass each
(freepose_amd.evaluation.GtInfoCalculator, csrc/gt_info.hip).  Given the depth images every integer is the reference's;
the JSON text is what inout.save_json writes.

What is kept from the reference script:
  * `--dataset`, `--dataset_split` (test), `--dataset_split_type`, `--delta` (15; the toolkit uses 5 for itodd), `--datasets_path`
    (BOP_PATH), `--renderer_type` (accepted with any value and ignored);
  * the depth image is loaded and multiplied by depth_scale in float32 (:106-107);
  * the scenes are the numbered folders present under the split directory.
Added: `--model_type` (default: the `models` folder, as there; `eval` = `models_eval`, `cad` = `models_cad`, ...), `--scene_ids` (comma
separated), and SLURM_ARRAY_TASK_ID selects one scene by its index in that list, as in `scripts.eval_calc_errors`.  The toolkit's
visibility visualisations (`vis_visibility_masks`) are not written.
"""
from __future__ import annotations

import argparse
import os
import time
from pathlib import Path

from freepose_amd.scripts.eval_calc_errors import _image_size, _load_depth, load_scene_camera, load_scene_gt, log

IMAGES_PER_FLUSH = 32         # test depth images held on the device at once


def build_parser(doc=None) -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=doc or __doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dataset", default="lm")
    ap.add_argument("--dataset_split", default="test")
    ap.add_argument("--dataset_split_type", default=None)
    ap.add_argument("--delta", default=15, help="tolerance of the visibility test in mm (5 for itodd, 15 for the other datasets)")
    ap.add_argument("--model_type", default=None, help="folder of the models: none = models, eval = models_eval, cad = models_cad, ...")
    ap.add_argument("--renderer_type", default="vispy",
                    help="accepted with any value: depth images are always rendered by this package's HIP rasteriser")
    ap.add_argument("--datasets_path", default=os.environ.get("BOP_PATH", "bop_datasets"))
    ap.add_argument("--scene_ids", default="", help="comma-separated scene ids (default: every scene folder of the split)")
    return ap


def params_from_args(args) -> dict:
    delta = float(args.delta)
    return {
        "dataset": str(args.dataset), "dataset_split": str(args.dataset_split),
        "dataset_split_type": None if args.dataset_split_type in (None, "", "None") else str(args.dataset_split_type),
        "delta": int(delta) if delta == int(delta) else delta,
        "model_type": None if args.model_type in (None, "", "None") else str(args.model_type),
        "renderer_type": str(args.renderer_type), "datasets_path": str(args.datasets_path),
        "scene_ids": [int(s) for s in str(args.scene_ids).split(",") if s.strip()],
    }


def split_path(p) -> Path:
    return Path(p["datasets_path"]) / p["dataset"] / (p["dataset_split"] + ("_" + p["dataset_split_type"] if p["dataset_split_type"] else ""))


def models_path(p) -> Path:
    return Path(p["datasets_path"]) / p["dataset"] / ("models" + ("_" + p["model_type"] if p["model_type"] else ""))


def model_files(p) -> dict:
    """obj_id -> obj_XXXXXX.ply of the models folder"""
    files = {int(f.stem.split("_")[1]): f for f in sorted(models_path(p).glob("obj_*.ply"))}
    if not files:
        raise FileNotFoundError(f"no obj_*.ply under {models_path(p)}")
    return files


def scene_ids(p) -> list:
    """dataset_params.get_present_scene_ids, cut to --scene_ids and to the scene SLURM_ARRAY_TASK_ID selects"""
    sp = split_path(p)
    ids = sorted(int(d.name) for d in sp.iterdir() if d.is_dir() and d.name.isdigit()) if sp.is_dir() else []
    if not ids:
        raise FileNotFoundError(f"no scene folders under {sp}")
    if p["scene_ids"]:
        missing = [s for s in p["scene_ids"] if s not in ids]
        if missing:
            raise FileNotFoundError(f"scenes {missing} not found under {sp}")
        ids = [s for s in ids if s in p["scene_ids"]]
    slurm = int(os.environ.get("SLURM_ARRAY_TASK_ID", -1))
    if slurm != -1:
        if not 0 <= slurm < len(ids):
            raise IndexError(f"SLURM_ARRAY_TASK_ID={slurm} for {len(ids)} scenes")
        ids = [ids[slurm]]
    return ids


def make_calculator(p, scenes):
    """a GtInfoCalculator of the split's image size holding the models that the scenes' ground truths name"""
    from freepose_amd import mesh_io
    from freepose_amd.evaluation import GtInfoCalculator
    sp = split_path(p)
    first_gt = load_scene_gt(sp / f"{scenes[0]:06d}" / "scene_gt.json")
    w, h = _image_size(sp, scenes[0], sorted(first_gt)[0])
    calc = GtInfoCalculator(w, h, p["delta"])
    files = model_files(p)
    needed = set()
    for s in scenes:
        for im_gt in load_scene_gt(sp / f"{s:06d}" / "scene_gt.json").values():
            needed.update(int(gt["obj_id"]) for gt in im_gt)
    for obj_id in sorted(needed):
        if obj_id not in files:
            raise FileNotFoundError(f"model of object {obj_id} not found under {models_path(p)}")
        calc.add_model(obj_id, mesh_io.load_ply(files[obj_id]))
    return calc


def scene_batches(p, scene_id):
    """yields (instances, depths, Ks, [(im_id, gt_id)], im_ids) for IMAGES_PER_FLUSH images of a scene at a time, images in ascending order"""
    sp = split_path(p)
    cams = load_scene_camera(sp / f"{scene_id:06d}" / "scene_camera.json")
    scene_gt = load_scene_gt(sp / f"{scene_id:06d}" / "scene_gt.json")
    im_ids = sorted(scene_gt)
    for i0 in range(0, len(im_ids), IMAGES_PER_FLUSH):
        instances, depths, Ks, ids = [], {}, {}, []
        for im_id in im_ids[i0:i0 + IMAGES_PER_FLUSH]:
            depths[im_id] = _load_depth(sp, scene_id, im_id, cams[im_id]["depth_scale"])       # to mm, in float32 (:106-107)
            Ks[im_id] = cams[im_id]["cam_K"]
            for gt_id, gt in enumerate(scene_gt[im_id]):
                instances.append((im_id, int(gt["obj_id"]), gt["cam_R_m2c"], gt["cam_t_m2c"]))
                ids.append((im_id, gt_id))
        yield instances, depths, Ks, ids, [im for im in im_ids[i0:i0 + IMAGES_PER_FLUSH]]


def run(argv=None):
    from freepose_amd.evaluation import bop_json_text
    p = params_from_args(build_parser().parse_args(argv))
    t0 = time.time()
    scenes = scene_ids(p)
    calc = make_calculator(p, scenes)
    written, n = [], 0
    for scene_id in scenes:
        log("Calculating GT info - dataset: {} ({}, {}), scene: {}".format(p["dataset"], p["dataset_split"], p["dataset_split_type"], scene_id))
        scene_gt_info = {}
        for instances, depths, Ks, ids, ims in scene_batches(p, scene_id):
            for im_id in ims:
                scene_gt_info[im_id] = []               # an image without ground truths keeps its empty list (:113)
            for (im_id, _), info in zip(ids, calc.gt_info(instances, depths, Ks)):
                scene_gt_info[im_id].append(info)
            n += len(instances)
        path = split_path(p) / f"{scene_id:06d}" / "scene_gt_info.json"
        path.write_text(bop_json_text(scene_gt_info))
        written.append(str(path))
    log("GT info of {} instances took {}s.".format(n, time.time() - t0))
    return written


if __name__ == "__main__":
    run()
