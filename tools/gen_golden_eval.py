"""Writes tests/golden/pose_errors.npz: the pose-error fixture of tests/test_eval_cpu.py and tests/test_gpu_eval.py.

    python tools/gen_golden_eval.py [path to the reference's bop_toolkit folder]

Runs on the CPU.  Every expected value is RETURNED BY THE REFERENCE'S OWN FUNCTIONS (bop_toolkit_lib.pose_error.{cus, vsd, chamfer,
chamfer_proj, re, te}); for cus and vsd they are handed a stand-in `renderer` whose render_object returns the depth image of
oracle.fp_oracle.rasterize (the rasteriser contract the HIP kernels are bit-exact against), the way the feature extractor was stood
in for when the pose-estimator fixture was made.  The integer pixel counts are taken with the reference's own mask / distance-image
functions.  The file holds data only: two procedural meshes, poses, intrinsics, a synthetic test depth image, tolerances, the expected
values and counts, and the errors-JSON text the reference's inout.save_json writes for a toy scene.
"""
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REF = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("/root/reference/bop_toolkit")
sys.path.insert(0, str(REF))
for missing in ("imageio", "png", "trimesh"):          # imported by inout at module level, not used by save_json
    try:
        __import__(missing)
    except ImportError:
        sys.modules[missing] = types.ModuleType(missing)

from bop_toolkit_lib import inout, misc, pose_error, visibility  # noqa: E402
from oracle import fp_oracle as fo  # noqa: E402

W, H = 640, 480
K = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])      # YCB-V


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def icosphere(level):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2],
         [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.asarray(p, float) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.asarray(v), np.asarray(f, np.int32)


def displaced_icosphere():
    """2562 vertices, about 60 mm radius, a smooth bump pattern: nearly but not exactly symmetric about z"""
    v, f = icosphere(4)
    x, y, z = v.T
    r = 60.0 * (1.0 + 0.10 * np.sin(4 * x) * np.cos(3 * y) + 0.06 * z * z + 0.015 * x)
    return (v * r[:, None]).astype(np.float32), f


def torus(nu=40, nv=30, R=0.40, r=0.15):
    """1200 vertices, model units of a normalised retrieved mesh (rendered with s_e)"""
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), 1.3 * r * np.sin(w)], -1).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [[a, b, c], [a, c, d]]
    return v.astype(np.float32), np.asarray(f, np.int32)


def rot(axis, deg):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


class OracleRenderer:
    """render_object(obj_id, R, t, fx, fy, cx, cy) -> {'depth'} like bop_toolkit_lib.renderer; the image is the oracle rasteriser's"""

    def __init__(self):
        self.models, self.cache = {}, {}

    def add(self, obj_id, verts, faces, scale):
        self.models[obj_id] = (verts, faces, float(scale))

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        v, f, s = self.models[obj_id]
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3], pose[:3, 3] = R, np.asarray(t).reshape(3)
        key = (obj_id, pose.tobytes())
        if key not in self.cache:
            _, d = fo.rasterize(v, f, None, pose[None], s, fx, fy, cx, cy, W, H)
            self.cache[key] = d[0]
        return {"depth": self.cache[key]}


def main():
    rng = np.random.default_rng(20240607)
    vA, fA = displaced_icosphere()
    vT, fT = torus()
    vTmm = (vT * np.float32(100.0)).astype(np.float32)
    gt_models = {1: (vA, fA), 2: (vTmm, fT)}
    inf_models = {"A": (vA, fA), "T": (vT, fT)}
    R0 = rot([0.3, 1.0, 0.2], 37.0) @ rot([1, 0, 0], 20.0)
    R1 = rot([1.0, 0.2, -0.5], 115.0)
    R2 = rot([0.1, 0.3, 1.0], -63.0)
    t0, t1, t2 = np.array([20.0, -10.0, 800.0]), np.array([-90.0, 40.0, 650.0]), np.array([150.0, -60.0, 1000.0])
    z = np.array([0.0, 0.0, 1.0])

    pairs = []   # (inf name, s_e, R_e, t_e, gt id, R_g, t_g)

    def add(inf, s, Re, te, gt, Rg, tg):
        pairs.append((inf, float(s), np.asarray(Re, float), np.asarray(te, float), int(gt), np.asarray(Rg, float), np.asarray(tg, float)))

    add("A", 1.0, R0, t0, 1, R0, t0)                                        # 0 identical mesh and pose: CUS 0, chamfer 0
    add("T", 100.0, R1, t1, 2, R1, t1)                                      # 1 the same shape through s_e
    add("A", 1.0, R0, t0 + [300.0, 0, 0], 1, R0, t0)                        # 2 disjoint silhouettes: CUS 1
    add("A", 1.0, R0, [5000.0, 0.0, 800.0], 1, R0, [5200.0, 100.0, 800.0])  # 3 both outside the frame: union 0 -> 1.0
    add("T", 120.0, R0 @ rot([0, 1, 0], 8.0), t0 + [3.0, -2.0, 6.0], 1, R0, t0)     # 4 other mesh, s_e != 1
    add("T", 80.0, R0, t0 + [-6.0, 4.0, -12.0], 1, R0, t0)                  # 5
    add("A", 1.0, R0 @ rot(z, 180.0), t0, 1, R0, t0)                        # 6 near-symmetric flip
    add("A", 1.0, R0, t0 - 40.0 * z, 1, R0, t0)                             # 7 VSD: estimate in front of the test surface
    add("A", 1.0, R0, t0 + 40.0 * z, 1, R0, t0)                             # 8 behind it
    add("A", 1.0, R0, t0 + 5.0 * z, 1, R0, t0)                              # 9 inside the delta band
    add("A", 1.0, R0 @ rot([1, 0, 0], 2.0), t0 - 8.0 * z, 1, R0, t0)        # 10 inside the band, slightly rotated
    add("A", 0.5, R0, t0, 1, R0, t0)                                        # 11 shrunk estimate
    add("A", 1.0, R0, [-205.0, 0.0, 800.0], 1, R0, t0)                      # 12 estimate cut by the image border
    add("A", 1.0, R0, [-900.0, 0.0, 800.0], 1, R0, t0)                      # 13 estimate outside, GT inside: CUS 1
    add("A", 1.0, R2, t2, 2, R2, t2)                                        # 14 wrong shape at the right pose
    add("T", 100.0, R1 @ rot(z, 180.0), t1, 2, R1, t1)                      # 15 symmetric flip of the torus
    for k in range(10):                                                     # 16.. growing random perturbations, mixed meshes / scales
        mag = 0.6 * (k + 1)
        ax = rng.normal(size=3)
        Rg, tg = [(R0, t0), (R1, t1), (R2, t2)][k % 3]
        gt = 1 if k % 2 == 0 else 2
        inf, s = [("A", 1.0), ("T", 100.0), ("T", 137.5), ("A", 0.9)][k % 4]
        add(inf, s, Rg @ rot(ax, 3.0 * mag), tg + rng.normal(size=3) * [2.0, 2.0, 6.0] * mag, gt, Rg, tg)
    n = len(pairs)
    assert n >= 24

    ren = OracleRenderer()
    for gid, (v, f) in gt_models.items():
        ren.add(gid, v, f, 1.0)

    # ---- synthetic test depth image: the scene of pose (R0, t0) + background wall + occluder strip + holes ---------------------------
    scene = ren.render_object(1, R0, t0.reshape(3, 1), K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"].astype(np.float64)
    depth = np.where(scene > 0, scene, 1200.0)
    depth[:, 330:352] = 520.0                        # occluder in front of part of the object
    depth[40:90, 60:200] = 0.0                       # holes of missing depth: background ...
    depth[215:245, 280:320] = 0.0                    # ... and on the object
    depth[rng.random((H, W)) < 0.01] = 0.0
    depth_u16 = np.round(depth * 10.0).astype(np.uint16)          # 0.1 mm units, like a BOP depth PNG with depth_scale 0.1
    depth_scale = 0.1
    depth_test = depth_u16.astype(np.float32)
    depth_test *= depth_scale

    diam = {gid: float(np.linalg.norm(v.astype(np.float64).max(0) - v.astype(np.float64).min(0))) for gid, (v, f) in gt_models.items()}
    vsd_cfg = [   # (delta, normalized_by_diameter, taus)
        (15.0, True, list(np.arange(0.05, 0.51, 0.05))),
        (7.3, False, [1.0, 2.0, 5.0, 10.0, 15.0, 20.0, 30.0, 50.0]),
    ]

    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    out = {k: [] for k in ("cus", "chamfer", "chamfer_proj", "re", "te", "cus_counts")}
    vsd_vals = [[] for _ in vsd_cfg]
    vsd_counts = [[] for _ in vsd_cfg]
    for i, (inf, s, Re, te, gid, Rg, tg) in enumerate(pairs):
        te, tg = te.reshape(3, 1), tg.reshape(3, 1)
        inf_id = f"inf{i}"
        ren.add(inf_id, inf_models[inf][0], inf_models[inf][1], s)          # add_object_from_mesh(inf_id, model, scale=s_e)
        pts_e = inf_models[inf][0].astype(np.float64) * s                   # models[inf_id]["pts"] *= s_e
        pts_g = gt_models[gid][0].astype(np.float64)
        out["cus"].append(pose_error.cus(Re, te, Rg, tg, K, ren, inf_id, gid))
        out["chamfer"].append(pose_error.chamfer(Re, te, Rg, tg, pts_e, pts_g))
        out["chamfer_proj"].append(pose_error.chamfer_proj(Re, te, Rg, tg, K, pts_e, pts_g))
        out["re"].append(pose_error.re(Re, Rg))
        out["te"].append(pose_error.te(te, tg))
        d_e = ren.render_object(inf_id, Re, te, fx, fy, cx, cy)["depth"]
        d_g = ren.render_object(gid, Rg, tg, fx, fy, cx, cy)["depth"]
        out["cus_counts"].append([int(((d_e > 0) & (d_g > 0)).sum()), int(((d_e > 0) | (d_g > 0)).sum())])
        dist_t, dist_g, dist_e = (misc.depth_im_to_dist_im_fast(d, K) for d in (depth_test, d_g, d_e))
        for c, (delta, norm, taus) in enumerate(vsd_cfg):
            vsd_vals[c].append(pose_error.vsd(Re, te, Rg, tg, depth_test, K, delta, taus, norm, diam[gid], ren, inf_id, gid, "step"))
            vg = visibility.estimate_visib_mask_gt(dist_t, dist_g, delta, visib_mode="bop19")
            ve = visibility.estimate_visib_mask_est(dist_t, dist_e, vg, delta, visib_mode="bop19")
            both = vg & ve
            dd = np.abs(dist_g[both] - dist_e[both]) / (diam[gid] if norm else 1.0)
            vsd_counts[c].append([int(both.sum()), int((vg | ve).sum())] + [int((dd >= t).sum()) for t in taus])
        print(f"pair {i:2d}: cus {out['cus'][-1]:.6f} chamfer {out['chamfer'][-1]:.6f} proj {out['chamfer_proj'][-1]:.6f} "
              f"vsd {vsd_vals[0][-1][0]:.4f}..{vsd_vals[0][-1][-1]:.4f} | {vsd_vals[1][-1][0]:.4f}", flush=True)

    # ---- schema pin: the text the reference writes for a toy scene (three estimates of two meshes in one image, two target objects) ---
    toy_csv = ("scene_id,im_id,obj_id,score,R,t,bbox_visib,scale,time\n"
               "3,1,meshA,0.3,1 0 0 0 1 0 0 0 1,10 20 800,5 6 70 80,0.12,0.5\n"
               "3,1,meshB,0.9,0 -1 0 1 0 0 0 0 1,-15 25 750.5,15 16 40 30,0.2,0.5\n"
               "3,1,meshA,0.6,1 0 0 0 0 -1 0 1 0,11 21 801,5 6 70 80,0.12,0.5\n")
    toy_targets = [{"scene_id": 3, "im_id": 1, "obj_id": 2, "inst_count": 2}, {"scene_id": 3, "im_id": 1, "obj_id": 5, "inst_count": 1}]
    eye = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    toy_scene_gt = {"1": [{"cam_R_m2c": eye, "cam_t_m2c": [0, 0, 800], "obj_id": 5}, {"cam_R_m2c": eye, "cam_t_m2c": [30, 0, 820], "obj_id": 2},
                          {"cam_R_m2c": eye, "cam_t_m2c": [-30, 5, 790], "obj_id": 2}]}
    # the stub evaluator of the test returns 0.125 * (est position in the CSV + 1) + gt_id for every pair.  Estimates of an image are
    # gathered mesh by mesh in first-appearance order (meshA: rows 0 and 2, then meshB: row 1), est_id = position in that list, then
    # sorted by score: meshB (est_id 2, csv row 1), meshA' (est_id 1, csv row 2), meshA (est_id 0, csv row 0)
    order = [(2, 0.9, 1), (1, 0.6, 2), (0, 0.3, 0)]          # (est_id, score, csv row)
    toy_errs = []
    for obj_id, gt_ids in ((2, [1, 2]), (5, [0])):
        for est_id, score, row in order:
            toy_errs.append({"im_id": 1, "obj_id": obj_id, "est_id": est_id, "score": score,
                             "errors": {g: [0.125 * (row + 1) + g] for g in gt_ids}})
    with tempfile.TemporaryDirectory() as d:
        inout.save_json(str(Path(d) / "errors.json"), toy_errs)
        toy_json = (Path(d) / "errors.json").read_text()

    golden = ROOT / "tests" / "golden" / "pose_errors.npz"
    np.savez_compressed(
        golden, K=K, width=W, height=H,
        mesh_A_v=vA, mesh_A_f=fA, mesh_T_v=vT, mesh_T_f=fT, gt_1_v=vA, gt_1_f=fA, gt_2_v=vTmm, gt_2_f=fT,
        pair_inf=np.array([p[0] for p in pairs]), pair_s=np.array([p[1] for p in pairs]), pair_Re=np.stack([p[2] for p in pairs]),
        pair_te=np.stack([p[3] for p in pairs]), pair_gt=np.array([p[4] for p in pairs]), pair_Rg=np.stack([p[5] for p in pairs]),
        pair_tg=np.stack([p[6] for p in pairs]),
        depth_u16=depth_u16, depth_scale=depth_scale, diameters=np.array([diam[1], diam[2]]),
        cus=np.array(out["cus"], np.float64), cus_counts=np.array(out["cus_counts"], np.int64),
        chamfer=np.array(out["chamfer"], np.float64), chamfer_proj=np.array(out["chamfer_proj"], np.float64),
        re=np.array(out["re"], np.float64), te=np.array(out["te"], np.float64),
        vsd0_delta=vsd_cfg[0][0], vsd0_norm=vsd_cfg[0][1], vsd0_taus=np.array(vsd_cfg[0][2]), vsd0=np.array(vsd_vals[0], np.float64),
        vsd0_counts=np.array(vsd_counts[0], np.int64),
        vsd1_delta=vsd_cfg[1][0], vsd1_norm=vsd_cfg[1][1], vsd1_taus=np.array(vsd_cfg[1][2]), vsd1=np.array(vsd_vals[1], np.float64),
        vsd1_counts=np.array(vsd_counts[1], np.int64),
        toy_csv=np.array(toy_csv), toy_targets=np.array(json.dumps(toy_targets)), toy_scene_gt=np.array(json.dumps(toy_scene_gt)),
        toy_errors_json=np.array(toy_json))
    print(f"wrote {golden} ({golden.stat().st_size} bytes), {n} pairs")
    assert golden.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
