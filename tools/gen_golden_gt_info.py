"""Writes tests/golden/gt_info.npz: the fixture of tests/test_gt_info_cpu.py and tests/test_gpu_gt_info.py.

    python tools/gen_golden_gt_info.py <path to the reference's bop_toolkit folder>

Runs on the CPU.  Every expected value is RETURNED BY THE REFERENCE'S OWN FUNCTIONS — misc.calc_pts_diameter,
misc.depth_im_to_dist_im_fast, visibility.estimate_visib_mask_gt, misc.calc_2d_bbox, inout.save_json — called in the order of
bop_toolkit/scripts/calc_gt_info.py:102-185 and calc_gt_masks.py:91-126 (those two are scripts without functions of their own, and
calc_model_info.py:36-50 is restated with the Python 3 reading of its map() calls).  The rendered depth comes from
oracle.fp_oracle.rasterize, the rasteriser contract the HIP kernels are bit-exact against: 64 x 48 images, 192 x 144 canvases with the
principal point shifted by (W, H).  The same functions are also run over the planted depth stacks of tests/_gt_info_ref.vis_cases() and
the small clouds of diam_cases().  The file holds data only: one procedural mesh, poses, intrinsics, a synthetic test depth image, the
rendered depth images, and the expected dicts, JSON text, masks and diameters.
"""
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
if len(sys.argv) < 2:
    sys.exit(__doc__)
REF = Path(sys.argv[1])
from tests import _gt_info_ref as cases  # noqa: E402  (before the toolkit is on the path: it has a `tests` package of its own)
from tools.gen_golden_eval import icosphere, rot  # noqa: E402
sys.path.insert(0, str(REF))
for missing in ("imageio", "png", "trimesh"):          # imported by inout at module level, not used by save_json
    try:
        __import__(missing)
    except ImportError:
        sys.modules[missing] = types.ModuleType(missing)

from bop_toolkit_lib import inout, misc, visibility  # noqa: E402
from oracle import fp_oracle as fo  # noqa: E402

W, H = 64, 48
K = np.array([[106.6778, 0.0, 31.29869], [0.0, 106.7487, 24.13109], [0.0, 0.0, 1.0]])      # YCB-V at a tenth of its size
DELTA = 15


def mesh():
    v, f = icosphere(2)                                  # 162 vertices
    x, y, z = v.T
    r = 60.0 * (1.0 + 0.10 * np.sin(4 * x) * np.cos(3 * y) + 0.06 * z * z + 0.015 * x)
    return (v * r[:, None]).astype(np.float32), f


def render(v, f, R, t, fx, fy, cx, cy, w, h):
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3], pose[:3, 3] = R, np.asarray(t).reshape(3)
    return fo.rasterize(v, f, None, pose[None], 1.0, fx, fy, cx, cy, w, h)[1][0]


def gt_info_of(canvas, depth, Kc, delta, ox, oy):
    """one instance: the reference's functions on the operands, and in the order, that calc_gt_info.py:125-185 gives them"""
    h, w = depth.shape
    dist_gt = misc.depth_im_to_dist_im_fast(canvas[oy:oy + h, ox:ox + w], Kc)
    dist_test = misc.depth_im_to_dist_im_fast(depth, Kc)
    visible = visibility.estimate_visib_mask_gt(dist_test, dist_gt, delta, visib_mode="bop19")
    silhouette = canvas > 0
    n_all, n_valid, n_visib = int(silhouette.sum()), int((dist_test[dist_gt > 0] > 0).sum()), int(visible.sum())
    boxes = {"bbox_obj": [-1, -1, -1, -1], "bbox_visib": [-1, -1, -1, -1]}
    if n_visib > 0:                                      # the reference takes BOTH boxes only when something is visible
        rows, cols = np.nonzero(silhouette)
        boxes["bbox_obj"] = [int(e) for e in misc.calc_2d_bbox(cols - ox, rows - oy, (w, h))]
        rows, cols = np.nonzero(visible)
        boxes["bbox_visib"] = [int(e) for e in misc.calc_2d_bbox(cols, rows, (w, h))]
    return {"px_count_all": n_all, "px_count_valid": n_valid, "px_count_visib": n_visib,
            "visib_fract": float(n_visib / float(n_all)) if n_all > 0 else 0.0, **boxes}


def masks_of(render_im, depth, Kc, delta):
    """one instance: the two images calc_gt_masks.py:98-126 saves"""
    dist_test = misc.depth_im_to_dist_im_fast(depth, Kc)
    dist_gt = misc.depth_im_to_dist_im_fast(render_im, Kc)
    visible = visibility.estimate_visib_mask_gt(dist_test, dist_gt, delta, visib_mode="bop19")
    return 255 * (dist_gt > 0).astype(np.uint8), 255 * visible.astype(np.uint8)


def saved_text(content):
    with tempfile.TemporaryDirectory() as d:
        inout.save_json(str(Path(d) / "x.json"), content)
        return (Path(d) / "x.json").read_text()


def main():
    rng = np.random.default_rng(20241020)
    v, f = mesh()
    R0 = rot([0.3, 1.0, 0.2], 37.0) @ rot([1, 0, 0], 20.0)
    R1 = rot([1.0, 0.2, -0.5], 115.0)
    poses = [(R0, [10.0, -5.0, 700.0]),        # 0 inside the image
             (R1, [-170.0, 20.0, 640.0]),      # 1 cut by the left image border: part of the silhouette only on the canvas
             (R0, [40.0, 150.0, 560.0]),       # 2 cut by the bottom border, nearer than 0
             (R1, [420.0, -60.0, 700.0]),      # 3 wholly in the truncated ring: px_count_all > 0, nothing visible, both boxes -1
             (R0, [5000.0, 0.0, 700.0]),       # 4 outside the canvas: all counts 0
             (R1, [60.0, 10.0, 900.0])]        # 5 behind the occluder strip
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    canvases = np.stack([render(v, f, R, t, fx, fy, cx + W, cy + H, 3 * W, 3 * H) for R, t in poses])
    renders = np.stack([render(v, f, R, t, fx, fy, cx, cy, W, H) for R, t in poses])
    # synthetic test depth image: instances 0, 1, 2 in front of a wall, an occluder strip, holes of missing depth
    depth = np.full((H, W), 1200.0)
    for i in (0, 1, 2):
        depth = np.where((renders[i] > 0) & (renders[i] < depth), renders[i], depth)
    depth[:, 36:44] = 450.0
    depth[5:12, 8:30] = 0.0
    depth[22:27, 28:34] = 0.0
    depth[rng.random((H, W)) < 0.02] = 0.0
    depth_u16 = np.round(depth * 10.0).astype(np.uint16)
    depth_scale = 0.1
    depth_test = depth_u16.astype(np.float32)
    depth_test *= depth_scale                           # calc_gt_info.py:106-107

    infos = [gt_info_of(c, depth_test, K, DELTA, W, H) for c in canvases]
    masks = [masks_of(r, depth_test, K, DELTA) for r in renders]
    for i, info in enumerate(infos):
        print(i, info)
    assert infos[3]["px_count_all"] > 0 and infos[3]["px_count_visib"] == 0 and infos[3]["bbox_obj"] == [-1] * 4
    assert infos[4]["px_count_all"] == 0 and infos[1]["bbox_obj"][0] < 0 and 0 < infos[5]["visib_fract"] < 0.9
    scene_gt_info = {7: infos[:4], 12: infos[4:]}
    info_text = saved_text(scene_gt_info)

    # the planted depth stacks of the kernel tests through the same functions
    planted = {}
    planted_masks = {}
    for name, c in cases.vis_cases().items():
        ox, oy = c["window"]
        H_, W_ = c["depth_test"].shape[1:]
        out, mm = [], []
        for b in range(len(c["depth_gt"])):
            test = c["depth_test"][c["img_idx"][b]]
            out.append(gt_info_of(c["depth_gt"][b], test, c["K"][b], c["delta"], ox, oy))
            mm.append(masks_of(c["depth_gt"][b][oy:oy + H_, ox:ox + W_], test, c["K"][b], c["delta"]))
        planted[name] = out
        planted_masks[name] = np.packbits(np.array(mm, np.uint8) > 0)

    # diameters: the reference's loop on the small clouds, the 1025-point cloud and the mesh
    clouds = cases.diam_cases(big=False)
    diam = {name: [float(misc.calc_pts_diameter(np.asarray(p, np.float64))) for p in cl] for name, cl in clouds.items() if name != "tiles"}
    diam["tile_plus_1"] = [float(misc.calc_pts_diameter(clouds["tiles"][2]))]
    pts = v.astype(np.float64)                           # inout.load_ply: model["pts"] in float64
    ref_pt = list(map(float, pts.min(axis=0).flatten()))
    size = list(map(float, (pts.max(axis=0) - ref_pt).flatten()))
    models_info = {3: {"min_x": ref_pt[0], "min_y": ref_pt[1], "min_z": ref_pt[2], "size_x": size[0], "size_y": size[1], "size_z": size[2],
                       "diameter": misc.calc_pts_diameter(pts)}}
    models_text = saved_text(models_info)

    golden = ROOT / "tests" / "golden" / "gt_info.npz"
    np.savez_compressed(
        golden, K=K, width=W, height=H, delta=DELTA, mesh_v=v, mesh_f=f, pose_R=np.stack([p[0] for p in poses]),
        pose_t=np.array([p[1] for p in poses], np.float64), depth_u16=depth_u16, depth_scale=depth_scale, canvases=canvases, renders=renders,
        infos=np.array(json.dumps(infos)), info_text=np.array(info_text), masks=np.packbits(np.array(masks, np.uint8) > 0),
        planted=np.array(json.dumps(planted)), **{"planted_masks_" + k: m for k, m in planted_masks.items()},
        diameters=np.array(json.dumps(diam)), models_info_text=np.array(models_text))
    print(f"wrote {golden} ({golden.stat().st_size} bytes)")
    assert golden.stat().st_size < 600 * 1024


if __name__ == "__main__":
    main()
