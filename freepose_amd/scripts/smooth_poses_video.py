"""python -m scripts.smooth_poses_video --video <name> --poses <coarse>.csv --proposals <props>.json --tracker module:factory

Drop-in for the reference CLI (scripts/smooth_poses_video.py:67-192, :286-373, flags :381-391): the step behind the paper's best video
result, `{video}-tracked.csv`.  Per object: the frame whose coarse pose the ViT-B confidence trusts most (`n_inliers_per_pose`), the clip
cut into intervals of about 12 frames, the start interval first, then forwards from the previous interval's last pose and backwards from
the following interval's first pose; per interval one `compute_2d3d_correspondences`, one tracker call and ONE `ops.pnp_epnp` call for all
its frames; rotation from PnP, translation from the coarse poses (:356), `smooth_transforms`.

Not in the reference: `--tracker module:factory` / `--tracker_args JSON` — CoTracker is fetched from torch.hub by the reference and is not
shipped here, so the point tracker is a callable `tracker(frames_u8 [T,H,W,3], queries_f32 [N,3] = (t, x, y)) -> (tracks [T,N,2],
visibility bool [T,N])` returned by `factory(**JSON)` (INTEGRATION.md wraps CoTracker that way); `--model`, `--allow_random_weights`.
The draw that adds invisible points when fewer than 15 are visible comes from a generator seeded with FILL_SEED (the reference shuffles
with the global generator, :175).  `--vis` is accepted; the overlays stay out of scope like `--viz` elsewhere.
"""
from __future__ import annotations

import argparse
import importlib
import json
import logging
from pathlib import Path

import numpy as np
from PIL import Image

log = logging.getLogger(__name__)

INTERVAL_LENGTH = 12          # reference :98
MIN_VISIBLE = 15              # reference :169
FILL_SEED = 0
IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png")


def load_tracker(spec: str, args_json: str | None = None):
    """`module:factory` -> factory(**json) (the tracker callable)"""
    if not spec or ":" not in spec:
        raise ValueError(f"--tracker {spec!r}: expected module:factory")
    module, factory = spec.split(":", 1)
    kwargs = json.loads(args_json) if args_json else {}
    if not isinstance(kwargs, dict):
        raise ValueError("--tracker_args: a JSON object of keyword arguments")
    return getattr(importlib.import_module(module), factory)(**kwargs)


def interval_boundaries(n_frames: int) -> np.ndarray:
    """round(linspace(0, n, n // 12)) (reference :101).  A clip shorter than 24 frames gets fewer than two boundaries, i.e. no interval;
    the reference dies with an IndexError at :109-112 there."""
    if n_frames // INTERVAL_LENGTH < 2:
        raise ValueError(f"smooth_poses_video: a clip of {n_frames} frames has no tracking interval — at least {2 * INTERVAL_LENGTH} frames "
                         "are needed (the reference fails with an IndexError on such a clip)")
    return np.round(np.linspace(0, n_frames, n_frames // INTERVAL_LENGTH)).astype(int)


def visibility_for_pnp(pred_visibility: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """bool [T,N]: the points each frame's PnP uses — the visible ones, and in a frame with fewer than 15 of them as many hidden ones,
    drawn without replacement, as bring it to 15 (all of them when there are not enough)"""
    use = np.array(pred_visibility, dtype=bool, copy=True)
    for row in use:
        missing = MIN_VISIBLE - int(row.sum())
        if missing > 0:
            log.warning("only %d tracked points visible: %d hidden ones join the pose estimate", int(row.sum()), missing)
            hidden = np.flatnonzero(~row)
            row[rng.choice(hidden, size=min(missing, len(hidden)), replace=False)] = True
    return use


def poses_from_tracks(points3d, tracks, visibility, K, rng) -> np.ndarray:
    """poses [T,4,4] of an interval's frames from its tracks [T,N,2]: ONE batched EPnP call (the reference loops cv2.solvePnP over
    the frames, :162-192)"""
    from freepose_amd import ops
    if len(tracks) == 0:
        raise RuntimeError("an interval without frames: no pose to estimate")
    out = ops.pnp_epnp(points3d, tracks, K, visibility_for_pnp(visibility, rng)).cpu().numpy()
    bad = np.nonzero(out[:, 14] != ops.PNP_OK)[0]
    if len(bad):
        raise RuntimeError(f"EPnP failed on frame(s) {bad.tolist()} of the interval (status {out[bad, 14].astype(int).tolist()}: 1 = fewer "
                           f"than 4 points, 2 = coplanar or coincident points; {len(points3d)} tracked points)")
    poses = np.tile(np.eye(4), (len(out), 1, 1))
    poses[:, :3, :3] = out[:, :9].reshape(-1, 3, 3)
    poses[:, :3, 3] = out[:, 9:12]
    return poses


def track_interval(frames, masks, mesh, K, first, last, anchor, anchor_pose, tracref, rng):
    """poses of frames [first, last) from points planted on frame `anchor` under `anchor_pose`, and the interval's record
    (anchor, (first, last), points3d, tracks, visibility).  The tracker sees exactly the interval's frames; a query's time is the
    anchor's position inside it."""
    pixels, points3d = tracref.compute_2d3d_correspondences(mesh, frames[anchor], K, anchor_pose, mask=masks[anchor])
    queries = np.concatenate([np.full((len(pixels), 1), anchor - first, dtype=pixels.dtype), pixels], axis=1)
    tracks, visibility = tracref._track_frames(frames[first:last], queries)
    return poses_from_tracks(points3d, tracks, visibility, K, rng), (anchor, (first, last), points3d, tracks, visibility)


def predict_transforms(frames, transforms, mesh, K, masks, tracref, rng=None):
    """tracked poses [n,4,4], the record of every interval and the start frame (reference :92-159).  The interval that holds the most
    trusted frame is solved first, anchored on that frame and its coarse pose; then the later intervals in order, each anchored on
    its first frame with the last pose of its predecessor; then the earlier ones going back, each anchored on its last frame with
    the first pose of its successor."""
    rng = np.random.default_rng(FILL_SEED) if rng is None else rng
    bounds = interval_boundaries(len(frames))
    n_intervals = len(bounds) - 1
    n_inliers, _ = tracref.n_inliers_per_pose(mesh, frames, K, transforms)
    start = int(np.argmax(n_inliers))
    home = int(np.searchsorted(bounds, start, side="right")) - 1
    plan = [(home, start, None)]
    plan += [(i, int(bounds[i]), i - 1) for i in range(home + 1, n_intervals)]
    plan += [(i, int(bounds[i + 1]) - 1, i + 1) for i in range(home - 1, -1, -1)]
    poses, records = {}, {}
    for i, anchor, neighbour in plan:
        if neighbour is None:
            anchor_pose = transforms[start]
        else:
            anchor_pose = poses[neighbour][-1] if neighbour < i else poses[neighbour][0]
        poses[i], records[i] = track_interval(frames, masks, mesh, K, int(bounds[i]), int(bounds[i + 1]), anchor, anchor_pose, tracref, rng)
    return np.concatenate([poses[i] for i in range(n_intervals)]), [records[i] for i in range(n_intervals)], start


def _vit_state_dict(model_name: str, allow_random_weights: bool):
    """the hub checkpoint's state dict, or None for seeded random weights when that was asked for; a missing checkpoint is an error"""
    import torch

    from freepose_amd.src.pipeline.retrieval import dino
    ckpt = dino._find_checkpoint(model_name)
    if ckpt is None:
        if not allow_random_weights:
            raise FileNotFoundError(f"DINOv2 checkpoint for {model_name} not found (set FREEPOSE_DINOV2_WEIGHTS to the file or its "
                                    "directory); --allow_random_weights runs on seeded random weights (tests and benchmarks only)")
        log.warning("no DINOv2 checkpoint: seeded random weights, the confidences are not meaningful for real images")
        return None
    state = torch.load(ckpt, map_location="cpu")
    return state["model"] if isinstance(state, dict) and "model" in state and "pos_embed" not in state else state


def main(args, tracker=None):
    import pandas as pd

    from freepose_amd.mesh_io import load_obj
    from freepose_amd.scripts.dino_inference_video import guessed_intrinsics
    from freepose_amd.src.pipeline.estimators.tracking_refiner import TrackingRefiner
    from freepose_amd.src.pipeline.refiner_utils import smooth_transforms
    from freepose_amd.src.pipeline.utils import rle_to_mask

    if args.poses is None and args.proposals is None:        # the reference's default file names (:389-391)
        stem = f"props-ground-box-0.2-text-0.2-ffa-22-top-25_{args.video}_gpt4_scaled_best_object"
        args.poses, args.proposals = f"{stem}_dinopose_layer_22_bbext_0.05_depth_zoedepth.csv", f"{stem}.json"
    data_dir = Path("data")
    frames_dir = data_dir / "datasets" / "videos" / args.video
    results_dir = data_dir / "results" / "videos" / args.video
    frame_paths = sorted(p for p in frames_dir.iterdir() if p.suffix.lower() in IMAGE_SUFFIXES)
    interval_boundaries(len(frame_paths))                    # a clip that is too short fails before any model is loaded
    if tracker is None:
        if not args.tracker:
            raise RuntimeError("smooth_poses_video: no point tracker. CoTracker is not shipped with this package; pass "
                               "--tracker module:factory (and --tracker_args JSON), see INTEGRATION.md")
        tracker = load_tracker(args.tracker, args.tracker_args)

    K_file = results_dir / "K.txt"
    if K_file.exists():
        K = np.loadtxt(K_file)
    else:
        w, h = Image.open(frame_paths[0]).size
        K = guessed_intrinsics(h, w)
    table = pd.read_csv(results_dir / args.poses)
    image_ids = table["im_id"].to_numpy()
    later = np.flatnonzero(image_ids != image_ids[0])
    n_objects = int(later[0]) if len(later) else len(image_ids)          # rows of the first image = objects per frame
    obj_idxs = list(range(n_objects)) if args.obj_idxs is None else list(args.obj_idxs)
    proposals_all = json.loads((results_dir / args.proposals).read_text())

    tracref = TrackingRefiner(dino_model=args.model, state_dict=_vit_state_dict(args.model, args.allow_random_weights), tracker=tracker)
    rng = np.random.default_rng(FILL_SEED)
    frames = np.stack([np.array(Image.open(p).convert("RGB")) for p in frame_paths])
    tracked = []
    for obj in obj_idxs:
        if not 0 <= obj < n_objects:
            raise ValueError(f"--obj-idxs {obj}: the CSV has {n_objects} objects per frame")
        rows = table.iloc[obj::n_objects]
        proposals = proposals_all[obj::n_objects]
        if not len(frame_paths) == len(rows) == len(proposals):
            raise ValueError(f"{len(frame_paths)} frames, {len(rows)} pose rows and {len(proposals)} proposals for object {obj}")
        masks = [rle_to_mask(p["segmentation"]) for p in proposals]
        scale = float(rows["scale"].iloc[0])
        if not (rows["scale"] == rows["scale"].iloc[0]).all():
            raise ValueError(f"object {obj}: the scale changes along the clip")
        coarse = np.tile(np.eye(4), (len(rows), 1, 1))
        coarse[:, :3, :3] = np.stack([np.array(r.split(" "), dtype=np.float64).reshape(3, 3) for r in rows["R"]])
        coarse[:, :3, 3] = np.stack([np.array(t.split(" "), dtype=np.float64) for t in rows["t"]])
        mesh_id = rows["obj_id"].iloc[0]
        mesh = load_obj(data_dir / "mesh_cache" / str(mesh_id) / f"{mesh_id}.obj")
        mesh.apply_scale(scale)

        poses, _records, start = predict_transforms(frames, coarse, mesh, K, masks, tracref, rng)
        log.info("object %d: start frame %d", obj, start)
        poses[:, :3, 3] = coarse[:, :3, 3]                   # rotation from the tracks, translation from the coarse poses (reference :356)
        poses = smooth_transforms(poses)

        rows = rows.copy()
        rows["R"] = [" ".join(str(x) for x in R.reshape(9)) for R in poses[:, :3, :3]]
        rows["t"] = [" ".join(str(x) for x in t) for t in poses[:, :3, 3]]
        tracked.append(rows)
    out_csv = results_dir / f"{args.video}-tracked.csv"
    pd.concat(tracked).sort_index().to_csv(out_csv, index=False)     # the input's rows, in the input's order
    if args.vis:
        log.warning("--vis: the overlays of the reference are out of scope; no images are written")
    return out_csv


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--video", type=str, required=True)
    ap.add_argument("--obj-idxs", type=int, default=None, nargs="+")
    ap.add_argument("--poses", type=str, default=None)
    ap.add_argument("--proposals", type=str, default=None)
    ap.add_argument("--vis", action="store_true", help="accepted for CLI parity; visualisation is out of scope")
    # not in the reference
    ap.add_argument("--tracker", type=str, default=None, help="module:factory returning the point tracker callable")
    ap.add_argument("--tracker_args", type=str, default=None, help="JSON object: keyword arguments of the factory")
    ap.add_argument("--model", type=str, default="dinov2_vitb14_reg")
    ap.add_argument("--allow_random_weights", action="store_true")           # run without the DINOv2 checkpoint (tests, benches)
    return ap


def run(argv=None):
    return main(build_parser().parse_args(argv))


if __name__ == "__main__":
    run()
