"""python -m scripts.eval_calc_errors --error_type cus --result_filenames method_ycbv-test.csv --results_path . --eval_path data/evals

Counterpart of bop_toolkit/scripts/eval_calc_errors.py for the model-free errors of the FreePose paper: `--error_type` in
{cus, chamfer, chamfer_proj, vsd, re, te}.  Reads the pose CSV that `scripts.dino_inference` / `scripts.merge_results` write
(scene_id,im_id,obj_id,score,R,t,bbox_visib,scale,time — inout.load_bop_results_bbox_visib, :297-347) and the BOP dataset as it is on
disk (scene_gt.json, scene_gt_info.json, scene_camera.json, the targets JSON, models_eval/obj_*.ply + models_info.json, depth PNG x
depth_scale), and writes `errors_<scene>.json` files with the keys and under the path template the reference uses
(eval_calc_errors.py:72-74,571-579,592-624), so `scripts.eval_calc_scores` / `scripts.eval_bop19_pose` of this package — or the
toolkit's eval_calc_scores.py — take them unchanged.

What is kept from the reference script:
  * the flag names and their defaults (`--renderer_type` is accepted with any value: the depth images always come from the HIP
    rasteriser of this package — the MI355X hosts have no OpenGL);
  * the pairing rule (:321-368): EVERY estimate of the image is compared against every ground truth of the target's object, s_e =
    scale * 1000, estimates sorted by score (descending, stable), est_id = position before the sort;
  * `--skip_missing` / `--vsd_normalized_by_diameter` are bool(<string>) as there: any non-empty value is true;
  * SLURM_ARRAY_TASK_ID selects one scene (:233-239, index into the scenes of the targets file in file order); unset = all scenes.
The work of a scene is batched: the estimate x ground-truth pairs of many images go through freepose_amd.evaluation.PoseErrorEvaluator
in a few launches instead of one render pair / two kd-trees per pair.  Matching and recalls: `scripts.eval_calc_scores`; the whole
table of the paper in one process: `scripts.eval_bop19_pose`.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

from freepose_amd.evaluation import ERROR_TYPES as SUPPORTED_ERROR_TYPES, VSD_TAUS_DEFAULT as VSD_TAUS

VSD_DELTAS = {"hb": 15, "icbin": 15, "icmi": 15, "itodd": 5, "lm": 15, "lmo": 15, "ruapc": 15, "tless": 15, "tudl": 15, "tyol": 15,
              "ycbv": 15, "hope": 15}
OUT_ERRORS_TPATH = os.path.join("{eval_path}", "{result_name}", "{error_sign}", "errors_{scene_id:06d}.json")
CSV_HEADER = "scene_id,im_id,obj_id,score,R,t,bbox_visib,scale,time"
PAIRS_PER_FLUSH = 256         # estimate x ground-truth pairs handed to the evaluator at once
IMAGES_PER_FLUSH = 32         # vsd: test depth images held on the device at once


def log(s):
    print(time.strftime("%m/%d|%H:%M:%S: ") + str(s), flush=True)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n_top", default=1)
    ap.add_argument("--error_type", default="vsd", help="one of: " + ", ".join(SUPPORTED_ERROR_TYPES))
    ap.add_argument("--vsd_deltas", default=",".join(f"{k}:{v}" for k, v in VSD_DELTAS.items()))
    ap.add_argument("--vsd_taus", default=",".join(map(str, VSD_TAUS)))
    ap.add_argument("--vsd_normalized_by_diameter", default=True)
    ap.add_argument("--max_sym_disc_step", default=0.01, help="accepted for compatibility (mssd / mspd are not computed here)")
    ap.add_argument("--skip_missing", default=True)
    ap.add_argument("--renderer_type", default="vispy",
                    help="accepted with any value: depth images are always rendered by this package's HIP rasteriser")
    ap.add_argument("--result_filenames", default="/path/to/csv/with/results", help="Comma-separated names of files with results.")
    ap.add_argument("--results_path", default=os.getcwd())
    ap.add_argument("--eval_path", default=os.getcwd())
    ap.add_argument("--models_inference_path", default=os.environ.get("BOP_MODELS_INFERENCE_PATH", "models_normalized"))
    ap.add_argument("--datasets_path", default=os.environ.get("BOP_PATH", "bop_datasets"))
    ap.add_argument("--targets_filename", default="test_targets_bop19.json")
    ap.add_argument("--out_errors_tpath", default=OUT_ERRORS_TPATH)
    return ap


def params_from_args(args) -> dict:
    return {
        "n_top": int(args.n_top),
        "error_type": str(args.error_type),
        "vsd_deltas": {str(e.split(":")[0]): float(e.split(":")[1]) for e in str(args.vsd_deltas).split(",")},
        "vsd_taus": list(map(float, str(args.vsd_taus).split(","))),
        "vsd_normalized_by_diameter": bool(args.vsd_normalized_by_diameter),
        "max_sym_disc_step": float(args.max_sym_disc_step),
        "skip_missing": bool(args.skip_missing),
        "renderer_type": str(args.renderer_type),
        "result_filenames": str(args.result_filenames).split(","),
        "results_path": str(args.results_path),
        "eval_path": str(args.eval_path),
        "models_inference_path": str(args.models_inference_path),
        "datasets_path": str(args.datasets_path),
        "targets_filename": str(args.targets_filename),
        "out_errors_tpath": str(args.out_errors_tpath),
    }


# ---- files -----------------------------------------------------------------------------------------------------------------------------
def load_results_csv(path) -> list:
    """the columns inout.load_bop_results_bbox_visib reads; obj_id stays a string (the name of the mesh used at inference)"""
    results = []
    with open(path, "r") as f:
        for line_id, line in enumerate(f):
            if line_id == 0 and CSV_HEADER in line:
                continue
            if not line.strip():
                continue
            elems = line.split(",")
            if len(elems) != 9:
                raise ValueError("A line does not have 9 comma-sep. elements: {}".format(line))
            results.append({
                "scene_id": int(elems[0]), "im_id": int(elems[1]), "obj_id": elems[2], "score": float(elems[3]),
                "R": np.array(list(map(float, elems[4].split())), np.float64).reshape((3, 3)),
                "t": np.array(list(map(float, elems[5].split())), np.float64).reshape((3, 1)),
                "bbox_visib": np.array(list(map(float, elems[6].split())), np.float64).reshape((4, 1)),
                "scale": float(elems[7]), "time": float(elems[8]),
            })
    return results


def _int_keys(x):
    return {int(k) if k.lstrip("-").isdigit() else k: v for k, v in x.items()}


def load_json(path, keys_to_int=False):
    with open(path, "r") as f:
        return json.load(f, object_hook=_int_keys) if keys_to_int else json.load(f)


def load_scene_gt(path) -> dict:
    scene_gt = load_json(path, keys_to_int=True)
    for im_gt in scene_gt.values():
        for gt in im_gt:
            gt["cam_R_m2c"] = np.array(gt["cam_R_m2c"], np.float64).reshape((3, 3))
            gt["cam_t_m2c"] = np.array(gt["cam_t_m2c"], np.float64).reshape((3, 1))
    return scene_gt


def load_scene_camera(path) -> dict:
    cam = load_json(path, keys_to_int=True)
    for c in cam.values():
        c["cam_K"] = np.array(c["cam_K"], np.float64).reshape((3, 3))
    return cam


def errors_json(scene_errs: list) -> str:
    """the text inout.save_json writes for a list: one record per line, keys sorted"""
    return "[\n" + ",\n".join("  {}".format(json.dumps(e, sort_keys=True)) for e in scene_errs) + "\n]"


def error_signature(error_type, n_top, vsd_delta=None, vsd_tau=None) -> str:
    sign = "error=" + error_type + "_ntop=" + str(n_top)
    if error_type == "vsd":
        tau = "inf" if vsd_tau == float("inf") else "{:.3f}".format(vsd_tau)
        sign += "_delta={:.3f}_tau={}".format(vsd_delta, tau)
    return sign


def split_result_name(result_filename):
    """<method>_<dataset>-<split>[-<split_type>].csv -> (result_name, method, dataset, split, split_type)"""
    result_name = os.path.splitext(os.path.basename(result_filename))[0]
    info = result_name.split("_")
    ds = info[1].split("-")
    return result_name, str(info[0]), str(ds[0]), str(ds[1]), (str(ds[2]) if len(ds) > 2 else None)


# ---- pairing ---------------------------------------------------------------------------------------------------------------------------
def organize(targets, ests):
    targets_org, ests_org = {}, {}
    for t in targets:
        targets_org.setdefault(t["scene_id"], {}).setdefault(t["im_id"], {})[t["obj_id"]] = t
    for e in ests:
        ests_org.setdefault(e["scene_id"], {}).setdefault(e["im_id"], {}).setdefault(e["obj_id"], []).append(e)
    return targets_org, ests_org


def pair_image(scene_id, im_id, im_targets, ests_org, im_gt, n_top, skip_missing) -> list:
    """eval_calc_errors.py:311-368 for one image: one record per (target object, estimate) in the order the reference appends them,
    each with the ground truths it is compared against: [{"obj_id", "est_id", "est", "gts": [(gt_id, gt), ...]}]"""
    records = []
    for obj_id, target in im_targets.items():
        if n_top == 0:
            n_top_curr = None
        elif n_top == -1:
            n_top_curr = target["inst_count"]
        else:
            n_top_curr = n_top
        try:
            obj_ests = []
            for est in ests_org[scene_id][im_id].values():     # every estimate of the image, whatever mesh it used
                obj_ests += est
        except KeyError:
            obj_ests = []
        if not skip_missing and n_top_curr is not None and len(obj_ests) < n_top_curr:
            raise ValueError("Not enough estimates for scene: {}, im: {}, obj: {} (provided: {}, expected: {})".format(
                scene_id, im_id, obj_id, len(obj_ests), n_top_curr))
        for est_id, est in sorted(enumerate(obj_ests), key=lambda x: x[1]["score"], reverse=True):
            gts = [(gt_id, gt) for gt_id, gt in enumerate(im_gt) if gt["obj_id"] == obj_id]
            records.append({"im_id": im_id, "obj_id": obj_id, "est_id": est_id, "est": est, "gts": gts})
    return records


def scene_errors(records, values) -> list:
    """records of pair_image (any number of images, in order) + one error list per (record, gt) in the same order -> the reference's
    scene_errs (:571-579)"""
    out, k = [], 0
    for r in records:
        errs = {}
        for gt_id, _ in r["gts"]:
            errs[gt_id] = values[k]
            k += 1
        out.append({"im_id": r["im_id"], "obj_id": r["obj_id"], "est_id": r["est_id"], "score": r["est"]["score"], "errors": errs})
    assert k == len(values)
    return out


# ---- driver ----------------------------------------------------------------------------------------------------------------------------
class _SceneRunner:
    """turns records into error values through a PoseErrorEvaluator, a few hundred pairs per call"""

    def __init__(self, p, dataset, evaluator, models_info, load_inferred):
        self.p, self.dataset, self.ev, self.models_info, self.load_inferred = p, dataset, evaluator, models_info, load_inferred

    def values(self, records, cams, depths) -> list:
        """cams: im_id -> scene_camera entry; depths: im_id -> test depth in mm (vsd only)"""
        et = self.p["error_type"]
        pairs, Ks, idx, im_ids = [], [], [], []
        for r in records:
            est = r["est"]
            for _, gt in r["gts"]:
                pairs.append((self.load_inferred(est["obj_id"]), est["scale"] * 1000, est["R"], est["t"], r["obj_id"], gt["cam_R_m2c"],
                              gt["cam_t_m2c"]))
                Ks.append(cams[r["im_id"]]["cam_K"])
                if r["im_id"] not in im_ids:
                    im_ids.append(r["im_id"])
                idx.append(im_ids.index(r["im_id"]))
        if not pairs:
            return []
        if et == "vsd":
            e = self.ev.errors("vsd", pairs, np.stack(Ks), depth_test=np.stack([depths[i] for i in im_ids]), img_idx=idx,
                               vsd_delta=self.p["vsd_deltas"][self.dataset], vsd_taus=self.p["vsd_taus"],
                               vsd_normalized_by_diameter=self.p["vsd_normalized_by_diameter"],
                               diameters={k: v["diameter"] for k, v in self.models_info.items()})
            return e
        return [[v] for v in self.ev.errors(et, pairs, np.stack(Ks))]


def _image_size(split_path: Path, scene_id: int, im_id: int):
    from PIL import Image
    for sub in ("depth", "rgb", "gray"):
        for ext in (".png", ".tif", ".jpg"):
            f = split_path / f"{scene_id:06d}" / sub / f"{im_id:06d}{ext}"
            if f.exists():
                with Image.open(f) as im:
                    return im.size
    raise FileNotFoundError(f"no image of scene {scene_id} / image {im_id} under {split_path} to take the image size from")


def _load_depth(split_path: Path, scene_id: int, im_id: int, depth_scale) -> np.ndarray:
    from PIL import Image
    for ext in (".png", ".tif"):
        f = split_path / f"{scene_id:06d}" / "depth" / f"{im_id:06d}{ext}"
        if f.exists():
            d = np.asarray(Image.open(f)).astype(np.float32)
            d *= depth_scale                           # to mm, in float32 like the reference's in-place multiply (:308-309)
            return d
    raise FileNotFoundError(f"depth image of scene {scene_id} / image {im_id} not found under {split_path}")


def evaluate_result_file(result_filename: str, p: dict) -> list:
    """errors of one results CSV; returns the paths written"""
    from freepose_amd import mesh_io
    from freepose_amd.evaluation import PoseErrorEvaluator

    t0 = time.time()
    result_name, method, dataset, split, split_type = split_result_name(result_filename)
    base = Path(p["datasets_path"]) / dataset
    split_path = base / (split + ("_" + split_type if split_type else ""))
    models_path = base / "models_eval"
    ests = load_results_csv(os.path.join(p["results_path"], result_filename))
    targets = load_json(base / p["targets_filename"])
    targets_org, ests_org = organize(targets, ests)
    et = p["error_type"]
    models_info = load_json(models_path / "models_info.json", keys_to_int=True) if et == "vsd" else {}      # the diameters
    slurm = int(os.environ.get("SLURM_ARRAY_TASK_ID", -1))
    written, n_ests, ev = [], 0, None
    for scene_ind, (scene_id, scene_targets) in enumerate(targets_org.items()):
        if slurm != -1 and scene_ind != slurm:
            continue
        log(f"Processing scene {scene_id} by SLURM array job index {slurm}...")
        cams = load_scene_camera(split_path / f"{scene_id:06d}" / "scene_camera.json")
        scene_gt = load_scene_gt(split_path / f"{scene_id:06d}" / "scene_gt.json")
        load_json(split_path / f"{scene_id:06d}" / "scene_gt_info.json", keys_to_int=True)     # read (and required) as in the reference
        if ev is None and et not in ("re", "te"):
            w, h = _image_size(split_path, scene_id, next(iter(scene_targets)))
            ev = PoseErrorEvaluator(w, h)
            for f in sorted(models_path.glob("obj_*.ply")):
                obj_id = int(f.stem.split("_")[1])
                if any(obj_id in im_t for st in targets_org.values() for im_t in st.values()):
                    ev.add_gt_model(obj_id, mesh_io.load_ply(f))
        elif ev is None:
            ev = PoseErrorEvaluator(1, 1)
        inferred = {}                                  # meshes used at inference, per scene like the reference (:581-590)

        def load_inferred(inf_id):
            if inf_id not in inferred:
                if et in ("re", "te"):
                    inferred[inf_id] = None
                else:
                    f = os.path.join(p["models_inference_path"], inf_id, inf_id + ".obj")
                    inferred[inf_id] = mesh_io.load_obj(f)     # float32 vertices for the rasteriser, vertices_f64 for the chamfer clouds
            return inferred[inf_id]

        runner = _SceneRunner(p, dataset, ev, models_info, load_inferred)
        records_all, values_all = [], []
        pending, depths, n_pending = [], {}, 0

        def flush():
            nonlocal pending, depths, n_pending
            values_all.extend(runner.values(pending, cams, depths))
            records_all.extend(pending)
            pending, depths, n_pending = [], {}, 0

        for im_ind, (im_id, im_targets) in enumerate(scene_targets.items()):
            if im_ind % 10 == 0:
                log(f"Calculating error {et} - method: {method}, dataset: {dataset}, scene: {scene_id}, im: {im_ind}")
            recs = pair_image(scene_id, im_id, im_targets, ests_org, scene_gt[im_id], p["n_top"], p["skip_missing"])
            n_ests += len(recs)
            if et == "vsd" and recs:
                depths[im_id] = _load_depth(split_path, scene_id, im_id, cams[im_id]["depth_scale"])
            pending += recs
            n_pending += sum(len(r["gts"]) for r in recs)
            if n_pending >= PAIRS_PER_FLUSH or len(depths) >= IMAGES_PER_FLUSH:
                flush()
        flush()
        scene_errs = scene_errors(records_all, values_all)

        def save(error_sign, errs):
            path = p["out_errors_tpath"].format(eval_path=p["eval_path"], result_name=result_name, error_sign=error_sign, scene_id=scene_id)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            log("Saving errors to: {}".format(path))
            with open(path, "w") as f:
                f.write(errors_json(errs))
            written.append(path)

        if et == "vsd":                                # one file per tau (:605-621)
            for tau_id, tau in enumerate(p["vsd_taus"]):
                cur = copy.deepcopy(scene_errs)
                for err in cur:
                    for gt_id in err["errors"]:
                        err["errors"][gt_id] = [err["errors"][gt_id][tau_id]]
                save(error_signature(et, p["n_top"], vsd_delta=p["vsd_deltas"][dataset], vsd_tau=tau), cur)
        else:
            save(error_signature(et, p["n_top"]), scene_errs)
    log("Calculation of errors for {} estimates took {}s.".format(n_ests, time.time() - t0))
    return written


def run(argv=None):
    p = params_from_args(build_parser().parse_args(argv))
    if p["error_type"] not in SUPPORTED_ERROR_TYPES:
        sys.exit("error type '{}' is not computed here; supported: {}".format(p["error_type"], ", ".join(SUPPORTED_ERROR_TYPES)))
    written = []
    for result_filename in p["result_filenames"]:
        log("Processing: {}".format(result_filename))
        written += evaluate_result_file(result_filename, p)
    log("Done.")
    return written


if __name__ == "__main__":
    run()
