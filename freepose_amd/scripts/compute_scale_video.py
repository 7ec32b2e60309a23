"""python -m scripts.compute_scale_video --video <name> --proposals <props>.json [--depth_dir <dir>]

Drop-in for the reference CLI (scripts/compute_scale_video.py:17-97): the clip's proposals JSON in, the same JSON with a `scale` field
out (`data/results/videos/<video>/<props>_gpt4_scaled.json`) — the file scripts.dino_inference_video reads.  Per frame:
GPT4ScaleEstimator.estimate on the 224 px crops of its proposals with the guessed intrinsics (f = image diagonal, centre principal
point); then every tracked object's scale is replaced by its median over the frames (:89-95), so the file ends with ONE scale per
object.

Depth: the reference predicts each frame's depth with ZoeDepth, which is not provided here.  `--depth_dir` names a directory with
one `<frame stem>.npy` per frame (float [H,W], metres) computed elsewhere; a relative path is looked up under the video's dataset
directory first.  WITHOUT `--depth_dir` the estimator runs without depth: the median table size per crop, no depth correction.

New flags: `--depth_dir`, `--clip_model`, `--scale_feats`, `--scale_file` / `--bpe_vocab` (compute the scale table with the text tower
first, see scripts.compute_scale), `--allow_random_weights`, `--query_k`, `--gpus`.  Under a
torch.distributed.run launch the frames are dealt round-robin over the ranks (a frame's scales depend on that frame only), the
scales all-gathered, and rank 0 takes the medians and writes the file: the same bytes as one rank."""
from __future__ import annotations

import argparse
import json
from itertools import takewhile
from pathlib import Path

import numpy as np
from PIL import Image

from freepose_amd import parallel
from freepose_amd.scripts.compute_scale import OUT_SUFFIX, add_common_flags, gather_scales, image_scales, make_estimator
from freepose_amd.scripts.dino_inference_video import guessed_intrinsics


def object_medians(scales, n_objects):
    """reference :89-95: proposals are frame-major with the objects in a fixed order; each object's scales -> their numpy median"""
    scales = list(scales)
    for o in range(n_objects):
        scales[o::n_objects] = [float(np.median(scales[o::n_objects]))] * len(scales[o::n_objects])
    return scales


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--video", type=str, required=True)
    ap.add_argument("--proposals", type=str, required=True)
    ap.add_argument("--depth_dir", type=str, default=None,
                    help="directory of per-frame depth maps <frame stem>.npy (float [H,W], metres) standing in for the reference's ZoeDepth "
                         "prediction; without it the scales are the table's median sizes with NO depth correction")
    return add_common_flags(ap)


def main(args):
    rank, world, _ = parallel.init_from_env()
    if world > 1:
        parallel.announce("dist")
    video_dir = (Path("data") / "datasets" / "videos" / args.video).resolve()
    frames = sorted(p for p in video_dir.iterdir() if p.suffix.lower() in (".jpg", ".jpeg"))
    results_dir = (Path("data") / "results" / "videos" / args.video).resolve()
    out_path = results_dir / args.proposals.replace(".json", OUT_SUFFIX)
    props = json.loads((results_dir / args.proposals).read_text())
    n_objects = len(list(takewhile(lambda x: x["image_id"] == 0, props)))
    by_frame = {}
    for n, p in enumerate(props):
        by_frame.setdefault(int(p["image_id"]), []).append(n)
    depth_dir = None
    if args.depth_dir is not None:
        depth_dir = video_dir / args.depth_dir if (video_dir / args.depth_dir).is_dir() else Path(args.depth_dir).resolve()
        if not depth_dir.is_dir():
            raise FileNotFoundError(f"compute_scale_video: --depth_dir {args.depth_dir} is not a directory")
    scale_estimator = make_estimator(args)
    h, w = np.asarray(Image.open(frames[0])).shape[:2]
    K = guessed_intrinsics(h, w)

    rows = []
    for f in parallel.shard_items(len(frames), rank, world):
        ids = by_frame.get(f, [])
        if not ids:
            continue
        image = np.asarray(Image.open(frames[f]).convert("RGB"), dtype=np.uint8)
        depth_pred = None
        if depth_dir is not None:
            depth_pred = np.load(depth_dir / f"{frames[f].stem}.npy")
            if depth_pred.shape != image.shape[:2]:
                raise ValueError(f"compute_scale_video: depth map {frames[f].stem}.npy is {depth_pred.shape}, the frame {image.shape[:2]}")
        rows += [[n, s] for n, s in zip(ids, image_scales(scale_estimator, image, [props[n] for n in ids], depth_pred, K))]
    scales = gather_scales(rows, len(props))
    if rank == 0:
        assert all(s is not None for s in scales), "compute_scale_video: a proposal names a frame the video does not have"
        for p, s in zip(props, object_medians(scales, n_objects)):
            p["scale"] = s
        out_path.write_text(json.dumps(props))
    return out_path


def run(argv=None):
    import sys
    args = build_parser().parse_args(argv)
    parallel.self_launch(args.gpus, ["-m", "scripts.compute_scale_video"], sys.argv[1:] if argv is None else list(argv))
    return main(args)


if __name__ == "__main__":
    run()
