"""python -m scripts.calc_gt_masks --dataset ycbv --dataset_split test --datasets_path data/bop_datasets

Counterpart of bop_toolkit/scripts/calc_gt_masks.py: writes `mask/{im_id:06d}_{gt_id:06d}.png` (the full silhouette of the model in the
ground-truth pose) and `mask_visib/{im_id:06d}_{gt_id:06d}.png` (its visible part, visibility.estimate_visib_mask_gt mode bop19) of every
ground-truth instance of a dataset split, as 8-bit greyscale PNGs holding 0 and 255 (:110-126).  The silhouettes are rendered at image
size by this package's HIP rasteriser and both masks of an instance are written by one fused device pass
(freepose_amd.evaluation.GtInfoCalculator, csrc/gt_info.hip).  The flags are those of `scripts.calc_gt_info`.
"""
from __future__ import annotations

import time

from freepose_amd.scripts import calc_gt_info as common
from freepose_amd.scripts.calc_gt_info import params_from_args  # noqa: F401
from freepose_amd.scripts.eval_calc_errors import log


def build_parser():
    return common.build_parser(__doc__)


def run(argv=None):
    from PIL import Image
    p = params_from_args(build_parser().parse_args(argv))
    t0 = time.time()
    scenes = common.scene_ids(p)
    calc = common.make_calculator(p, scenes)
    written, n = [], 0
    for scene_id in scenes:
        log("Calculating masks - dataset: {} ({}, {}), scene: {}".format(p["dataset"], p["dataset_split"], p["dataset_split_type"], scene_id))
        sd = common.split_path(p) / f"{scene_id:06d}"
        (sd / "mask").mkdir(exist_ok=True)
        (sd / "mask_visib").mkdir(exist_ok=True)
        for instances, depths, Ks, ids, _ in common.scene_batches(p, scene_id):
            masks, visibs = calc.gt_masks(instances, depths, Ks)
            for (im_id, gt_id), m, v in zip(ids, masks, visibs):
                for folder, img in (("mask", m), ("mask_visib", v)):
                    path = sd / folder / f"{im_id:06d}_{gt_id:06d}.png"
                    Image.fromarray(img, mode="L").save(path)
                    written.append(str(path))
            n += len(instances)
    log("Masks of {} instances took {}s.".format(n, time.time() - t0))
    return written


if __name__ == "__main__":
    run()
