"""python -m scripts.eval_videos [-v VIDEO ...] [-l LABEL ...] [-p PATTERN ...] [-i ANN_ID] [--data_path data]

Counterpart of the reference's scripts/eval_videos.py: scores the pose CSVs of the video pipeline (`scripts.dino_inference_video`: the
coarse CSV, `scripts.smooth_poses_video`: `{video}-tracked.csv`, and other methods' files) against `video_gt/{video}_poses_id{ann}.npy`
— relative-rotation, projected-translation and depth velocity errors over 10 time offsets `linspace(1, N / 2, 10)`, with the 101-step
symmetry sweep for objects that have a `sym_axis` — and writes `results_rot.csv`, `results_proj.csv`, `results_depth.csv` (videos x
methods) and `results_mean.csv` (methods x metrics) under `<data_path>/results/videos/`, printing the rounded tables.

Kept from the reference: the flags and their defaults (32 videos, six labels and patterns), the ground-truth file (a pickled dict with
`poses`, `mesh_id`, `focal_length`, `bboxes` and optionally `sym_axis`; gt_scale = 0.15), the frame size from the first file of
`datasets/videos/{video}`, and `load_pred_csv` (:54-115): the object with the highest mean bbox IoU against the ground-truth boxes (a
warning below 0.5), exactly one object per frame, one scale for all frames, non-finite rotations / translations repaired by forward fill
(frame 0 takes the first finite value).  A pattern that fails to load is an error line and a NaN cell, as there.

Two deviations:
  * the reference samples 1000 points of the object's mesh per CSV (`sample_mesh_points`) that no metric uses; the mesh is not loaded
    here, and `load_pred_csv` returns None in their place;
  * every track of the table goes to the device in ONE call (`video_errors_table` -> fp_video_errors) instead of a Python loop over
    offset x frame pair x symmetry per cell.
`--data_path` (default `data`, the reference's fixed DATA_PATH) is an addition.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import pandas as pd
from PIL import Image

from freepose_amd.src.utils.bbox_utils import bbox_iou

GT_SCALE = 0.15

video_names = [
    'bowl1', 'bowl2', 'bowl3', 'bowl4', 'bowl5', 'bowl6', 'bowl7', 'campbells1', 'campbells2', 'campbells3', 'campbells4', 'cups', 'jug',
    'juice', 'pour_268', 'pour_805', 'pour_2100', 'pour_2257', 'pour_2866', 'pour_4168', 'pour_4711', 'pour_from_7369', 'pour_from_8021',
    'pour_from_10591', 'pour_in_1110', 'pour_in_10109', 'pour_into_1771', 'pour_into_6685', 'pour_onto_10437', 'pour_into_8625',
    'pour_onto_8316', 'spoons',
]
DEFAULT_LABELS = ["MegaPose coarse", "MegaPose fine", "GigaPose", "FoundPose", "Ours coarse", "Ours fine"]
DEFAULT_PATTERNS = [
    "props-ground-box-0.2-text-0.2-ffa-22-top-25_{video}_gpt4_scaled_best_object_megapose_coarse.csv",
    "props-ground-box-0.2-text-0.2-ffa-22-top-25_{video}_gpt4_scaled_best_object_megapose_coarse_ref.csv",
    "gigapose_{video}_rescaled.csv",
    "foundpose_{video}_rescaled.csv",
    "props-ground-box-0.2-text-0.2-ffa-22-top-25_{video}_gpt4_scaled_best_object_dinopose_layer_22_bbext_0.05_depth_zoedepth.csv",
    "{video}-tracked.csv",
]


def warn(msg):
    print(f"WARNING: {msg}", file=sys.stderr, flush=True)


def error(msg):
    print(f"ERROR: {msg}", file=sys.stderr, flush=True)


def load_gt(data_path, vid, ann_id):
    """-> (poses f64 [N,4,4], gt_scale, sym_axis or None, mesh id, focal length, bboxes)"""
    d = np.load(Path(data_path) / "video_gt" / f"{vid}_poses_id{ann_id}.npy", allow_pickle=True).item()
    sym_axis = d["sym_axis"] if "sym_axis" in d else None
    gt = np.asarray([np.asarray(p, dtype=np.float64) for p in d["poses"]])
    return gt, GT_SCALE, sym_axis, d["mesh_id"], d["focal_length"], d["bboxes"]


def _forward_fill(a, what, filepath):
    """rows of a [N, k] with a non-finite entry take the previous row; row 0 the first finite row (load_pred_csv :94-113)"""
    for i in range(len(a)):
        if not np.isfinite(a[i]).all():
            warn(f"Found non-finite {what} at index {i} ({filepath})")
            if i == 0:
                idx = np.where(np.all(np.isfinite(a), axis=1))[0][0].item()
                a[0] = a[idx]
            else:
                a[i] = a[i - 1]


def load_pred_csv(filepath, obj_id=None, bbox=None):
    """-> (poses f64 [N,4,4], scale, obj_id, bbox_visib of frame 0, None).  bbox: the ground-truth boxes [x, y, w, h] per frame; the object
    (position within a frame's rows) with the highest mean IoU is the track."""
    df = pd.read_csv(filepath)
    if obj_id is not None:
        df = df[df["obj_id"] == obj_id]
    if ((isinstance(bbox, np.ndarray) and bbox.ndim == 2) or
            (isinstance(bbox, list) and len(bbox) > 0 and isinstance(bbox[0], np.ndarray) and bbox[0].ndim == 1)):
        N = np.sum(df["im_id"] == 0)
        object_ious = []
        for obj_idx in range(N):
            obj_bboxes = [np.array(list(map(int, x.split(" ")))) for x in df["bbox_visib"].values[obj_idx::N]]
            object_ious.append(np.mean([bbox_iou(a, b) for a, b in zip(obj_bboxes, bbox)]))
        object_index = np.argmax(object_ious)
        max_iou = object_ious[object_index]
        if max_iou < 0.5:
            warn(f"The best object has mean IoU = {max_iou:.4f} < 0.5. Maybe the detection for the correct object is missing?")
        df = df.iloc[object_index::N].reset_index(drop=True)
    elif bbox is not None:
        raise ValueError(f"Unsupported bbox type: {bbox}")

    obj_id = df["obj_id"].values[0]
    N = np.sum(df["im_id"] == 0)
    assert N != 0, "Could not find any relevant object!"
    assert N == 1, "Found multiple objects!"
    pred_scales = df["scale"].values
    assert len(np.unique(pred_scales)) == 1, "Found different scales for different frames!"
    pred_scale = pred_scales[0]

    R = np.array([np.array(s.split(), dtype=np.float64) for s in df["R"].values]).reshape(-1, 9)
    t = np.array([np.array(s.split(), dtype=np.float64) for s in df["t"].values]).reshape(-1, 3)
    _forward_fill(t, "translation", filepath)
    _forward_fill(R, "rotation", filepath)
    T = np.tile(np.eye(4), (len(R), 1, 1))
    T[:, :3, :3], T[:, :3, 3] = R.reshape(-1, 3, 3), t
    return T, pred_scale, obj_id, df["bbox_visib"].values[0], None


def frame_size(data_path, video):
    frame_path = list((Path(data_path) / "datasets" / "videos" / video).iterdir())[0]
    h, w = np.asarray(Image.open(frame_path)).shape[:2]
    return w, h


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--videos", "-v", type=str, nargs="*", default=None, help="Video names")
    ap.add_argument("--labels", "-l", type=str, nargs="*", default=None, help="Method names")
    ap.add_argument("--patterns", "-p", type=str, nargs="*", default=None,
                    help="Output .csv filename patterns with the {video} placeholder for each method")
    ap.add_argument("--ann_id", "-i", type=int, default=1, help="Ground-truth annotation ID")
    ap.add_argument("--data_path", type=str, default="data", help="root of video_gt/, datasets/videos/ and results/videos/")
    return ap


def resolve_defaults(args):
    if args.labels is None and args.patterns is None:
        args.labels, args.patterns = list(DEFAULT_LABELS), list(DEFAULT_PATTERNS)
    assert args.labels is not None and args.patterns is not None and len(args.labels) == len(args.patterns)
    if args.videos is None:
        args.videos = list(video_names)
        print(f"Running evaluation on {len(args.videos)} videos")
    return args


def main(args):
    from freepose_amd.src.utils.video_evaluation import video_errors_table

    args = resolve_defaults(args)
    data = Path(args.data_path).resolve()
    videos, labels = args.videos, args.labels
    results = {x: pd.DataFrame(np.nan, index=videos, columns=labels) for x in ["rot", "proj", "depth"]}

    gts, tracks = [], []
    for v, video in enumerate(videos):
        w, h = frame_size(data, video)
        gt, gt_scale, gt_sym_axis, _, _, gt_bboxes = load_gt(data, video, args.ann_id)
        dts = np.linspace(1, len(gt) / 2, num=10, dtype=int)
        print(video, dts)
        gts.append(dict(poses=gt, w=w, h=h, sym_axis=gt_sym_axis, gt_scale=gt_scale, dts=dts))
        for pattern in args.patterns:
            try:
                pred_path = data / "results" / "videos" / video / pattern.format(video=video)
                pred_poses, pred_scale, _, _, _ = load_pred_csv(pred_path, bbox=gt_bboxes)
            except Exception as ex:
                error(f"failed to load video={video}, pattern={pattern}:\n{ex}")
                tracks.append(None)
                continue
            assert len(pred_poses) == len(gt)
            tracks.append(dict(video=v, poses=pred_poses, scale=pred_scale))

    table = video_errors_table(tracks, gts).reshape(len(videos), len(labels), 3)
    for k, metric in enumerate(["rot", "proj", "depth"]):
        for v, video in enumerate(videos):
            for m, method in enumerate(labels):
                if tracks[v * len(labels) + m] is None:
                    continue
                err = table[v, m, k]
                if not np.isfinite(err):
                    error(f"[{metric}]! video={video}, method={method}: {err}")
                results[metric].loc[video, method] = err

    out_dir = data / "results" / "videos"
    out_dir.mkdir(parents=True, exist_ok=True)
    for k, v in results.items():
        v.to_csv(str(out_dir / f"results_{k}.csv"))
        print(f"{k} errors")
        print(np.round(v, 2))
        print()
        print("-" * 80)

    mean_results = pd.DataFrame(-1.0, index=labels, columns=["rot", "proj", "depth"])
    for method in labels:
        for metric in ["rot", "proj", "depth"]:
            mean_results.loc[method, metric] = np.mean(results[metric][method])
    print("Mean results:")
    print(np.round(mean_results, 2))
    mean_results.to_csv(str(out_dir / "results_mean.csv"))
    return results, mean_results


def run(argv=None):
    return main(build_parser().parse_args(argv))


if __name__ == "__main__":
    run()
