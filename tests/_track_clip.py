"""The synthetic mesh clip of the tracking tests as a plain helper (the builder of tests/test_gpu_refiner_track.py's `clip` fixture with the
number of frames as a parameter): bench.synthetic_mesh rendered on a planted trajectory, the coarse CSV, proposals with the rendered masks,
K.txt and the scene file of the planted-truth tracker tests/_synth_tracker.py.  Needs the rasteriser, i.e. a GPU."""
import json

import numpy as np
import torch

from tests import _refiner_ref as ref

FRAME_W, FRAME_H = 320, 240
COARSE_SEED = 11                 # axes of the 40-degree errors
TRAJ_START = 4.0                 # first angle (rad) of the planted turn
K_CLIP = np.array([[300.0, 0, 160.0], [0, 300.0, 120.0], [0, 0, 1]])


def planted_trajectory(n_frames):
    poses = np.tile(np.eye(4), (n_frames, 1, 1))
    for i in range(n_frames):
        poses[i, :3, :3] = ref.rodrigues([0.2, 1.0, 0.3], TRAJ_START + i * np.deg2rad(2.0)) @ ref.rodrigues([1.0, 0.1, -0.2], 0.4)
        poses[i, :3, 3] = [0.06 * np.sin(i / 9.0), 0.03 * np.cos(i / 7.0), 0.85 + 0.002 * i]
    return poses


def coarse_poses(poses):
    rng = np.random.default_rng(COARSE_SEED)
    coarse = poses.copy()
    exact = list(range(0, len(poses), 6))
    for i in range(len(poses)):
        if i not in exact:
            coarse[i, :3, :3] = ref.rodrigues(rng.standard_normal(3), np.deg2rad(40.0)) @ poses[i, :3, :3]
    return coarse, exact


def build_clip(root, n_frames=24):
    """data/ tree under `root` of an n-frame clip (planted translation; planted rotation on every 6th frame of the coarse CSV, 40 degrees
    off about a seeded axis elsewhere) -> dict(root, rdir, scene, poses, coarse, exact, frames, masks, scale, mesh = (v, f, c))"""
    import bench
    import pandas as pd
    from PIL import Image

    from freepose_amd import ops
    from freepose_amd.scripts.dino_inference import CSV_COLUMNS, pose_row
    from freepose_amd.src.pipeline.utils import mask_to_rle_pytorch
    v, f, c = bench.synthetic_mesh(3)
    scale = 0.25
    poses = planted_trajectory(n_frames)
    dm = ops.Mesh(v * scale, f, c).set_ambient(5.0)
    rgb, depth = ops.rasterize(dm, torch.from_numpy(poses.astype(np.float32)), 1.0, K_CLIP[0, 0], K_CLIP[1, 1], K_CLIP[0, 2], K_CLIP[1, 2],
                               FRAME_W, FRAME_H)
    frames, masks = rgb.cpu().numpy(), (depth > 0).cpu().numpy()
    fdir = root / "data" / "datasets" / "videos" / "synth"
    rdir = root / "data" / "results" / "videos" / "synth"
    mdir = root / "data" / "mesh_cache" / "synthobj"
    for d in (fdir, rdir, mdir):
        d.mkdir(parents=True)
    for i, fr in enumerate(frames):
        Image.fromarray(fr).save(fdir / f"{i:06d}.png")
    (mdir / "synthobj.obj").write_text("".join(f"v {x:.9g} {y:.9g} {z:.9g} {r} {g} {b}\n" for (x, y, z), (r, g, b) in zip(v.tolist(), c.tolist()))
                                       + "".join(f"f {a + 1} {b + 1} {cc + 1}\n" for a, b, cc in np.asarray(f).tolist()))
    coarse, exact = coarse_poses(poses)
    rows, props = [], []
    for i in range(n_frames):
        ys, xs = np.nonzero(masks[i])
        box = [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]
        rows.append(pose_row(0, i, "synthobj", 1.0, coarse[i], box, scale, t_scale=1, time_value=-1))
        props.append({"image_id": i, "bbox": [box[0], box[1], box[2] - box[0], box[3] - box[1]], "mesh": "synthobj", "scale": scale,
                      "segmentation": mask_to_rle_pytorch(masks[i:i + 1])[0]})
    pd.DataFrame(rows, columns=CSV_COLUMNS).to_csv(rdir / "coarse.csv", index=False, header=True)
    (rdir / "props.json").write_text(json.dumps(props))
    np.savetxt(rdir / "K.txt", K_CLIP)
    scene = root / "scene.npz"
    np.savez(scene, vertices=v * scale, faces=f, colors=c, K=K_CLIP, poses=poses, frames=frames)
    return dict(root=root, rdir=rdir, scene=scene, poses=poses, coarse=coarse, exact=exact, frames=frames, masks=masks, scale=scale,
                mesh=(v * scale, f, c))


def read_poses(csv):
    import pandas as pd
    df = pd.read_csv(csv)
    R = np.stack([np.array(s.split(" "), dtype=np.float64).reshape(3, 3) for s in df["R"]])
    t = np.stack([np.array(s.split(" "), dtype=np.float64) for s in df["t"]])
    return df, R, t
