"""python -m scripts.compute_scale --dataset ycbv --proposals <props>.json [--split test]

Drop-in for the reference CLI (scripts/compute_scale.py:15-63): proposals JSON in, the same JSON with a `scale` field per proposal out
(`data/results/<dataset>/<props>_gpt4_scaled.json`) — the file scripts.dino_inference reads with `--depth_method zoedepth`.  Per
image: 224 px crops of its proposals (bbox_extend 0.05) -> GPT4ScaleEstimator.estimate(proposals, entry['depth_pred'], K).

The scale table is read from `--scale_feats` (default data/scale_feats.pt: {"feats", "scales"}).  The reference computes it from
data/gpt4_scales.json with the CLIP text tower on every start (:28-29); `--scale_file data/gpt4_scales.json` does the same here
(tokenizer merges: `--bpe_vocab` or FREEPOSE_CLIP_BPE) and writes the table to `--scale_feats` first.  The predicted depth is the dataset entry's `depth_pred`
(BOPDataset: `<scene>/depth_pred/<frame>.png`, 16-bit / 65535).  An image without one is an error unless `--no_depth` is given; then
the estimator runs without depth for every image (the table's medians, no correction).

New flags: `--clip_model`, `--scale_feats`, `--scale_file`, `--bpe_vocab`, `--allow_random_weights`, `--no_depth`, `--query_k`, `--gpus`.  Under a
torch.distributed.run launch the images are dealt round-robin over the ranks, the scales all-gathered, and rank 0 writes the file:
the same bytes as one rank (an image's scales depend on that image only)."""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np
import torch

from freepose_amd import parallel
from freepose_amd.src.dataloader.bop import BOPDataset
from freepose_amd.src.pipeline.estimators.scale_estimators import GPT4ScaleEstimator
from freepose_amd.src.pipeline.retrieval.clip import CLIPFeatureExtractor
from freepose_amd.src.pipeline.utils import Proposals, rle_to_mask

OUT_SUFFIX = "_gpt4_scaled.json"


def image_scales(scale_estimator, image, frame_props, depth_pred, K):
    """scales of one image's proposals-JSON entries (reference :43-57, video script :67-84): float list in entry order"""
    masks = torch.from_numpy(np.stack([rle_to_mask(p["segmentation"]) for p in frame_props]))
    boxes = torch.from_numpy(np.stack([np.array(p["bbox"]) for p in frame_props]))
    boxes[:, 2] += boxes[:, 0]                       # xywh -> xyxy
    boxes[:, 3] += boxes[:, 1]
    proposals = Proposals(image, {"boxes": boxes, "masks": masks}, 224, bbox_extend=0.05)
    if depth_pred is None:
        scales = scale_estimator.estimate(proposals)
    else:
        scales = scale_estimator.estimate(proposals, depth_pred, K)
    return [float(s) for s in scales]


def gather_scales(rows, n_total):
    """(proposal index, scale) pairs of every rank -> float list [n_total] on every rank; an index nobody computed stays None"""
    packed = torch.tensor(rows, dtype=torch.float64).reshape(-1, 2)
    if parallel.world()[1] > 1:
        packed = parallel.all_gather_rows(packed.cuda()).cpu()
    out = [None] * n_total
    for i, s in packed.tolist():
        out[int(i)] = s
    return out


def make_estimator(args):
    """the extractor and the estimator on the table of `--scale_feats`.  With `--scale_file` the table is computed first, as the
    reference does on every run (compute_scale.py:28-29): rank 0 runs the text tower over the file's names and writes `--scale_feats`,
    the other ranks wait at a barrier; then every rank loads the same file."""
    clip = CLIPFeatureExtractor(args.clip_model, allow_random_weights=args.allow_random_weights or None, bpe_vocab=args.bpe_vocab)
    if args.scale_file is not None:
        clip.require_text_tower()
        rank, world = parallel.world()
        if rank == 0:
            GPT4ScaleEstimator.generate_clip_features(args.scale_file, clip, feats_path=args.scale_feats)
        if world > 1:
            torch.distributed.barrier()
    return GPT4ScaleEstimator(clip, query_k=args.query_k, feats_path=args.scale_feats)


def add_common_flags(ap):
    # not in the reference (defaults reproduce it)
    ap.add_argument("--clip_model", type=str, default="ViT-bigG-14", help="CLIP image tower (weights: FREEPOSE_CLIP_WEIGHTS)")
    ap.add_argument("--scale_feats", type=str, default="data/scale_feats.pt",
                    help="torch file {'feats': [N,E] text embeddings, 'scales': [N]} of the scale table (the text tower is not provided)")
    ap.add_argument("--scale_file", type=str, default=None,
                    help="JSON object {name: size} (the reference's data/gpt4_scales.json): compute the scale table with the CLIP text tower "
                         "at start-up and write it to --scale_feats (needs a checkpoint with the text tensors and --bpe_vocab)")
    ap.add_argument("--bpe_vocab", type=str, default=None,
                    help="the tokenizer's merges file, open_clip's bpe_simple_vocab_16e6.txt.gz or its .txt (default: FREEPOSE_CLIP_BPE)")
    ap.add_argument("--allow_random_weights", action="store_true", help="run without the CLIP checkpoint (tests, benches)")
    ap.add_argument("--query_k", type=int, default=11, help="nearest table rows per crop (the reference's constant)")
    ap.add_argument("--gpus", type=int, default=1, help="self-launch N ranks, one per GPU")
    return ap


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", type=str, required=True)
    ap.add_argument("--proposals", type=str, required=True)
    ap.add_argument("--split", type=str, default="test")
    ap.add_argument("--no_depth", action="store_true",
                    help="ignore the dataset's depth_pred maps: the table's median sizes without the depth correction")
    return add_common_flags(ap)


def main(args):
    rank, world, _ = parallel.init_from_env()
    if world > 1:
        parallel.announce("dist")
    res_dir = Path("./data/results").resolve() / args.dataset
    out_path = res_dir / args.proposals.replace(".json", OUT_SUFFIX)
    props = json.loads((res_dir / args.proposals).read_text())
    by_image = {}
    for n, p in enumerate(props):
        by_image.setdefault((int(p["scene_id"]), int(p["image_id"])), []).append(n)
    scale_estimator = make_estimator(args)
    dataset = BOPDataset(f"data/datasets/{args.dataset}/", args.split)

    rows = []
    for idx in parallel.shard_items(len(dataset), rank, world):
        ids = by_image.get(dataset.frame_key(idx), [])
        if not ids:
            continue
        entry = dataset[idx]
        depth_pred = None
        if not args.no_depth:
            if "depth_pred" not in entry:
                raise FileNotFoundError(f"compute_scale: scene {entry['scene_id']} frame {entry['frame_id']} has no depth_pred map "
                                        "(<scene>/depth_pred/<frame>.png); pass --no_depth to estimate without depth")
            depth_pred = entry["depth_pred"]
        scales = image_scales(scale_estimator, entry["image"], [props[n] for n in ids], depth_pred, entry["intrinsic"])
        rows += [[n, s] for n, s in zip(ids, scales)]
    for p, s in zip(props, gather_scales(rows, len(props))):
        if s is not None:                             # (a proposal of an image the split does not hold keeps its entry unchanged, as in the reference)
            p["scale"] = s
    if rank == 0:
        out_path.write_text(json.dumps(props))
    return out_path


def run(argv=None):
    import sys
    args = build_parser().parse_args(argv)
    parallel.self_launch(args.gpus, ["-m", "scripts.compute_scale"], sys.argv[1:] if argv is None else list(argv))
    return main(args)


if __name__ == "__main__":
    run()
