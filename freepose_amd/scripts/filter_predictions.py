"""python -m scripts.filter_predictions --video VIDEO --proposals PROPOSALS.json [--ann_id 1] [--data_path data]

Counterpart of the reference's scripts/filter_predictions.py (:24-50): of the objects proposed in every frame of a video (the proposals
JSON under `<data_path>/results/videos/<video>/`, frame-major, the same number of objects per frame as in frame 0), keep the one whose
boxes have the highest mean IoU with the ground-truth boxes of `video_gt/{video}_poses_id{ann}.npy`, and write its entries to
`<proposals stem>_best_object.json` next to the input — the file `scripts.dino_inference_video` and the default patterns of
`scripts.eval_videos` read.  Host work (a few hundred box pairs); `--data_path` is an addition.
"""
from __future__ import annotations

import argparse
import json
from itertools import takewhile
from pathlib import Path

import numpy as np

from freepose_amd.src.utils.bbox_utils import bbox_iou


def read_json(json_path):
    with open(json_path, "r") as f:
        return json.load(f)


def load_gt_boxes(data_path, vid, ann_id):
    d = np.load(Path(data_path) / "video_gt" / f"{vid}_poses_id{ann_id}.npy", allow_pickle=True).item()
    return d["bboxes"]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--video", type=str, required=True)
    ap.add_argument("--proposals", type=str, required=True)
    ap.add_argument("--ann_id", type=int, default=1)
    ap.add_argument("--data_path", type=str, default="data", help="root of video_gt/ and results/videos/")
    return ap


def main(args):
    data = Path(args.data_path).resolve()
    gt_bboxes = load_gt_boxes(data, args.video, args.ann_id)
    proposals_path = data / "results" / "videos" / args.video / args.proposals
    proposals = read_json(proposals_path)

    N = len(list(takewhile(lambda x: x["image_id"] == 0, proposals)))
    object_proposals = [proposals[i::N] for i in range(N)]
    object_ious = []
    for i in range(N):
        object_bboxes = [x["bbox"] for x in object_proposals[i]]
        object_ious.append(np.mean([bbox_iou(a, b) for a, b in zip(gt_bboxes, object_bboxes)]).item())
    idx = int(np.argmax(object_ious))
    iou = object_ious[idx]
    if iou < 0.5:
        print(f"Warning: The best object ({idx}) has IoU={iou} < 0.5. Maybe the detection for the correct object is missing?")
    print(f"Best object: {idx} with IoU: {iou}")

    best_object_path = proposals_path.with_name(proposals_path.stem + "_best_object.json")
    with open(best_object_path, "w") as f:
        json.dump(object_proposals[idx], f)
    return best_object_path


def run(argv=None):
    return main(build_parser().parse_args(argv))


if __name__ == "__main__":
    run()
