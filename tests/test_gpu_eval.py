"""Pose-error evaluation on the MI355X against the reference's own outputs (tests/golden/pose_errors.npz, made by
tools/gen_golden_eval.py from bop_toolkit_lib.pose_error with the oracle rasteriser standing in for the OpenGL renderer).

Contract (DESIGN.md "Scoring"):
  * cus / vsd: every pixel count equals the reference's, so every float64 error is IDENTICAL (==);
  * chamfer / chamfer_proj: |e - e_ref| <= 2e-6 (r + e_ref), r = the largest absolute centred coordinate of the pair (mm or px):
    one fp32 rounding of each centred coordinate (<= 2^-24 r), a few fp32 ulps of the squared-difference form relative to the
    distance, fp64 means; 2e-6 leaves about 5x over that sum;
  * two runs give identical bits; a batch gives the bits of pair-by-pair calls.
"""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from tests._eval_ref import centred_r as _centred_r

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CHAMFER_REL = 2e-6


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir / "pose_errors.npz")


class _M:
    """minimal mesh object (vertices, faces) as the evaluator and mesh_io.device_mesh take it"""

    def __init__(self, v, f):
        self.vertices, self.faces = v, f


def _depth_test(gold):
    d = gold["depth_u16"].astype(np.float32)
    d *= float(gold["depth_scale"])
    return d


def _pose(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, np.asarray(t).reshape(3)
    return T


def _clouds(gold):
    inf = {"A": gold["mesh_A_v"].astype(np.float64), "T": gold["mesh_T_v"].astype(np.float64)}
    gt = {1: gold["gt_1_v"].astype(np.float64), 2: gold["gt_2_v"].astype(np.float64)}
    return inf, gt


def _check_chamfer(got, gold, key, K=None):
    inf, gt = _clouds(gold)
    worst = 0.0
    for i in range(len(gold[key])):
        r = _centred_r(inf[str(gold["pair_inf"][i])], gt[int(gold["pair_gt"][i])], gold["pair_s"][i], gold["pair_Re"][i], gold["pair_te"][i],
                       gold["pair_Rg"][i], gold["pair_tg"][i], K)
        ref = float(gold[key][i])
        bound = CHAMFER_REL * (r + ref)
        print(f"{key} pair {i:2d}: got {got[i]!r} ref {ref!r} |diff| {abs(got[i] - ref):.3e} bound {bound:.3e} r {r:.3f}")
        worst = max(worst, abs(got[i] - ref) / bound)
        assert abs(got[i] - ref) <= bound, (key, i, got[i], ref, r)
    print(f"{key}: worst |diff| / bound = {worst:.4f}")


def _chamfer_args(gold):
    inf, gt = _clouds(gold)
    clouds = [inf["A"], inf["T"], gt[1], gt[2]]
    idx_e, idx_g = {"A": 0, "T": 1}, {1: 2, 2: 3}
    pairs = [(idx_e[str(a)], idx_g[int(g)]) for a, g in zip(gold["pair_inf"], gold["pair_gt"])]
    return clouds, pairs, gold["pair_s"], gold["pair_Re"], gold["pair_te"], gold["pair_Rg"], gold["pair_tg"]


# ---- 1. kernels vs fixture -----------------------------------------------------------------------------------------------------------
def test_depth_compare_and_chamfer_kernels_match_the_reference(gold):
    from freepose_amd import evaluation as ev, ops
    K, W, H = gold["K"], int(gold["width"]), int(gold["height"])
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    inf_mesh = {"A": ops.Mesh(gold["mesh_A_v"], gold["mesh_A_f"]), "T": ops.Mesh(gold["mesh_T_v"], gold["mesh_T_f"])}
    gt_mesh = {1: ops.Mesh(gold["gt_1_v"], gold["gt_1_f"]), 2: ops.Mesh(gold["gt_2_v"], gold["gt_2_f"])}
    n = len(gold["cus"])
    d_est, d_gt = [], []
    for i in range(n):
        pe = torch.from_numpy(_pose(gold["pair_Re"][i], gold["pair_te"][i])[None])
        pg = torch.from_numpy(_pose(gold["pair_Rg"][i], gold["pair_tg"][i])[None])
        d_est.append(ops.rasterize(inf_mesh[str(gold["pair_inf"][i])], pe, float(gold["pair_s"][i]), fx, fy, cx, cy, W, H)[1])
        d_gt.append(ops.rasterize(gt_mesh[int(gold["pair_gt"][i])], pg, 1.0, fx, fy, cx, cy, W, H)[1])
    d_est, d_gt = torch.cat(d_est), torch.cat(d_gt)
    c = ops.depth_compare(d_est, d_gt).cpu().numpy()
    assert np.array_equal(c[:, :2], gold["cus_counts"]), (c[:, :2] - gold["cus_counts"])
    for i in range(n):
        assert ev.cus_from_counts(c[i, 0], c[i, 1]) == gold["cus"][i], i
    dt = torch.from_numpy(_depth_test(gold))
    for cfg in ("vsd0", "vsd1"):
        taus, delta, norm = gold[cfg + "_taus"], float(gold[cfg + "_delta"]), bool(gold[cfg + "_norm"])
        div = [float(gold["diameters"][int(g) - 1]) if norm else 1.0 for g in gold["pair_gt"]]
        v = ops.depth_compare(d_est, d_gt, dt, None, K, delta, taus, div).cpu().numpy()
        assert np.array_equal(v[:, :2], gold["cus_counts"])
        print(cfg, "counts differ at", np.argwhere(v[:, 2:] != gold[cfg + "_counts"]).tolist())
        assert np.array_equal(v[:, 2:], gold[cfg + "_counts"]), cfg
        for i in range(n):
            assert ev.vsd_from_counts(v[i, 2], v[i, 3], v[i, 4:]) == list(gold[cfg][i]), (cfg, i)
    args = _chamfer_args(gold)
    e3 = ops.chamfer(*args).cpu().numpy()
    _check_chamfer(e3, gold, "chamfer")
    e2 = ops.chamfer_proj(*args, K).cpu().numpy()
    _check_chamfer(e2, gold, "chamfer_proj", K)
    assert np.array_equal(ops.chamfer(*args).cpu().numpy().view(np.int64), e3.view(np.int64))           # same bits on a second run
    assert np.array_equal(ops.chamfer_proj(*args, K).cpu().numpy().view(np.int64), e2.view(np.int64))
    assert e3[0] == 0.0 and e2[0] == 0.0                                                                # identical mesh and pose


def test_depth_compare_scalar_path_and_bad_chamfer_table():
    """stacks that are not 16-byte aligned (or whose image size is not a multiple of 4) take the scalar loop: same counts; a chamfer
    table row that reaches outside the clouds yields NaN for that pair only"""
    import ctypes as C
    from freepose_amd import _lib, ops
    from freepose_amd._lib import check, current_stream, ptr
    g = torch.Generator().manual_seed(4)
    for H, W in ((6, 10), (7, 9)):
        buf = [((torch.rand((3 * H * W + 1,), generator=g) - 0.4).clamp(min=0) * 900).cuda() for _ in range(3)]
        for off in (0, 1):                                   # off = 1: base pointers 4 bytes past a 16-byte boundary
            e, gt, t = (b[off:off + 3 * H * W].view(3, H, W) for b in buf)
            assert off == 0 or e.data_ptr() % 16 == 4
            c = ops.depth_compare(e, gt).cpu().numpy()
            assert np.array_equal(c[:, 0], ((e > 0) & (gt > 0)).sum((1, 2)).cpu().numpy())
            assert np.array_equal(c[:, 1], ((e > 0) | (gt > 0)).sum((1, 2)).cpu().numpy())
            K = np.array([[50.0, 0, W / 2], [0, 55.0, H / 2], [0, 0, 1]])
            v = ops.depth_compare(e, gt, t[:1], None, K, 15.0, [0.1, 0.5], 100.0).cpu().numpy()
            v0 = ops.depth_compare(e.clone(), gt.clone(), t[:1].clone(), None, K, 15.0, [0.1, 0.5], 100.0).cpu().numpy()   # aligned copies
            assert np.array_equal(v, v0) and np.array_equal(v[:, :2], c[:, :2])
    lib = _lib.load()
    pts = torch.randn((30, 3), dtype=torch.float64, device="cuda")
    xf = np.zeros((2, ops.EVAL_XF_LD)); xf[:, 0] = 1.0; xf[:, 1:10] = np.eye(3).reshape(-1); xf[:, 13:22] = np.eye(3).reshape(-1)
    table = np.zeros((2, ops.EVAL_TABLE_LD), np.int32)
    table[0] = [0, 10, 10, 20, 0, 10, 0, 0]
    table[1] = [0, 10, 25, 20, 30, 40, 0, 0]                 # GT cloud rows 25..44 of 30: outside d_pts
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    d_table, d_xf = torch.from_numpy(table).cuda(), torch.from_numpy(xf).cuda()   # named: a temporary's block is free for the next upload
    check(lib.fp_chamfer(ops.context(), ptr(pts), 30, ptr(d_table), ptr(d_xf), 2, 20, 60, 0, ptr(out), current_stream()), "fp_chamfer")
    o = out.cpu().numpy()
    ref = float(torch.cdist(pts[:10], pts[10:]).min(1).values.mean() + torch.cdist(pts[:10], pts[10:]).min(0).values.mean())
    assert np.isnan(o[1]) and abs(o[0] - ref) <= 2e-6 * (float(pts.abs().max()) * 2 + ref)


# ---- 2. evaluator --------------------------------------------------------------------------------------------------------------------
def test_evaluator_batch_equals_pair_by_pair_and_the_reference(gold):
    from freepose_amd.evaluation import PoseErrorEvaluator
    K, W, H = gold["K"], int(gold["width"]), int(gold["height"])
    ev = PoseErrorEvaluator(W, H, max_batch=16)                 # 26 pairs: two chunks, the second one partial
    ev.add_gt_model(1, _M(gold["gt_1_v"], gold["gt_1_f"])).add_gt_model(2, _M(gold["gt_2_v"], gold["gt_2_f"]))
    inf = {"A": _M(gold["mesh_A_v"], gold["mesh_A_f"]), "T": _M(gold["mesh_T_v"], gold["mesh_T_f"])}
    n = len(gold["cus"])
    pairs = [(inf[str(gold["pair_inf"][i])], float(gold["pair_s"][i]), gold["pair_Re"][i], gold["pair_te"][i], int(gold["pair_gt"][i]),
              gold["pair_Rg"][i], gold["pair_tg"][i]) for i in range(n)]
    dt = _depth_test(gold)
    diam = {1: float(gold["diameters"][0]), 2: float(gold["diameters"][1])}
    kw = {"vsd0": dict(depth_test=dt, vsd_delta=float(gold["vsd0_delta"]), vsd_taus=list(gold["vsd0_taus"]), vsd_normalized_by_diameter=True,
                       diameters=diam),
          "vsd1": dict(depth_test=dt, vsd_delta=float(gold["vsd1_delta"]), vsd_taus=list(gold["vsd1_taus"]), vsd_normalized_by_diameter=False)}
    for key, et in (("cus", "cus"), ("chamfer", "chamfer"), ("chamfer_proj", "chamfer_proj"), ("vsd0", "vsd"), ("vsd1", "vsd"), ("re", "re"),
                    ("te", "te")):
        batch = ev.errors(et, pairs, K, **kw.get(key, {}))      # ONE call over all pairs: mixed meshes and scales
        single = [ev.errors(et, [p], K, **kw.get(key, {}))[0] for p in pairs]
        assert len(batch) == n
        if et == "vsd":
            assert all(isinstance(b, list) and len(b) == len(gold[key + "_taus"]) for b in batch)
            assert batch == single and batch == [list(x) for x in gold[key]], key
        elif et in ("cus", "re", "te"):
            assert all(isinstance(b, float) for b in batch)
            assert batch == single and batch == list(gold[key]), key
        else:
            assert np.array_equal(np.array(batch).view(np.int64), np.array(single).view(np.int64)), key    # bit for bit
            _check_chamfer(batch, gold, key, K if et == "chamfer_proj" else None)


# ---- 3. scale ------------------------------------------------------------------------------------------------------------------------
def _cdist_chamfer(X, Y, rows=256):
    """mean_y min_x + mean_x min_y in fp64 on the device, the distance matrix in row chunks (no matrix-multiply shortcut).  torch's
    direct cdist kernel runs one 256-thread workgroup per matrix entry and a HIP launch holds fewer than 2^32 threads: chunks of
    256 x 40 000 entries stay below that (a 5000-row chunk came back mostly unwritten); sampled entries of every chunk are checked
    against the plain expression so that a short launch cannot pass for a reference."""
    assert rows * Y.shape[0] * 256 < 2 ** 32
    min_y = torch.full((Y.shape[0],), float("inf"), dtype=torch.float64, device=Y.device)
    sum_x = torch.zeros((), dtype=torch.float64, device=Y.device)
    ok = torch.ones((), dtype=torch.bool, device=Y.device)
    ja = torch.tensor([0, Y.shape[0] // 3, Y.shape[0] - 1], device=Y.device)
    for a in range(0, X.shape[0], rows):
        Xa = X[a:a + rows]
        D = torch.cdist(Xa, Y, compute_mode="donot_use_mm_for_euclid_dist")
        ia = torch.tensor([0, Xa.shape[0] // 2, Xa.shape[0] - 1], device=Y.device)
        want = (Xa[ia] - Y[ja]).pow(2).sum(1).sqrt()
        ok &= ((D[ia, ja] - want).abs() <= 1e-12 * want.abs().max()).all()
        sum_x += D.min(dim=1).values.sum()
        min_y = torch.minimum(min_y, D.min(dim=0).values)
    assert bool(ok), "torch.cdist returned entries that are not the distances"
    return float(min_y.mean() + sum_x / X.shape[0])


def test_chamfer_at_scale_64_pairs_of_50000_by_40000_points(gold):
    from freepose_amd import ops
    B, NE, NG = 64, 50000, 40000
    g = torch.Generator(device="cuda").manual_seed(11)
    K = gold["K"]
    Kt = torch.from_numpy(K).cuda()
    est = [torch.randn((NE, 3), generator=g, dtype=torch.float64, device="cuda") * 45.0 for _ in range(B)]
    gt = [torch.randn((NG, 3), generator=g, dtype=torch.float64, device="cuda") * 50.0 for _ in range(B)]
    rng = np.random.default_rng(12)
    Re, Rg = np.empty((B, 3, 3)), np.empty((B, 3, 3))
    for b in range(B):
        for R in (Re, Rg):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            R[b] = q * np.sign(np.linalg.det(q))
    tg = np.stack([rng.normal(size=B) * 80, rng.normal(size=B) * 60, 900 + rng.normal(size=B) * 100], 1)
    te = tg + rng.normal(size=(B, 3)) * 10
    s = 0.8 + 0.4 * rng.random(B)
    pairs = [(b, B + b) for b in range(B)]
    for proj in (False, True):
        t0 = time.time()
        fn = (lambda: ops.chamfer_proj(est + gt, pairs, s, Re, te, Rg, tg, K)) if proj else (lambda: ops.chamfer(est + gt, pairs, s, Re, te, Rg, tg))
        e = fn().cpu().numpy()
        t1 = time.time()
        assert np.array_equal(fn().cpu().numpy().view(np.int64), e.view(np.int64)), "second run differs"
        worst = 0.0
        for b in range(B):
            X = (est[b] * s[b]) @ torch.from_numpy(Re[b]).cuda().T + torch.from_numpy(te[b]).cuda()
            Y = gt[b] @ torch.from_numpy(Rg[b]).cuda().T + torch.from_numpy(tg[b]).cuda()
            o = gt[b].mean(0, keepdim=True) @ torch.from_numpy(Rg[b]).cuda().T + torch.from_numpy(tg[b]).cuda()
            if proj:
                X, Y, o = (((p @ Kt.T)[:, :2] / (p @ Kt.T)[:, 2:3]) for p in (X, Y, o))
            r = float(max((X - o).abs().max(), (Y - o).abs().max()))
            ref = _cdist_chamfer(X, Y)
            bound = CHAMFER_REL * (r + ref)
            worst = max(worst, abs(e[b] - ref) / bound)
            assert abs(e[b] - ref) <= bound, (proj, b, e[b], ref, r)
        print(f"scale test projected={proj}: first call {t1 - t0:.3f} s wall (incl. upload), worst |diff| / bound = {worst:.4f}")


# ---- 4. CLI end to end ---------------------------------------------------------------------------------------------------------------
def _write_ply(path, v, f):
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y", "property float z",
            f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    r = np.zeros(len(f), dtype=[("k", "u1"), ("v", "<i4", (3,))])
    r["k"], r["v"] = 3, f
    Path(path).write_bytes(("\n".join(head) + "\n").encode() + np.asarray(v, "<f4").tobytes() + r.tobytes())


def _write_obj(path, v, f):
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Path(path).write_text("\n".join([f"v {float(a)!r} {float(b)!r} {float(c)!r}" for a, b, c in v] +
                                    [f"f {a + 1} {b + 1} {c + 1}" for a, b, c in f]) + "\n")


SHIFTS = (0.0, 1.0, 3.0, 8.0)        # known perturbation of the estimates: t_e = t_g + k * (3, 0, -6) mm


def _make_dataset(gold, root):
    from PIL import Image
    from freepose_amd import ops
    K, W, H = gold["K"], int(gold["width"]), int(gold["height"])
    ds = root / "datasets" / "toyds"
    (ds / "models_eval").mkdir(parents=True)
    _write_ply(ds / "models_eval" / "obj_000001.ply", gold["gt_1_v"], gold["gt_1_f"])
    _write_ply(ds / "models_eval" / "obj_000002.ply", gold["gt_2_v"], gold["gt_2_f"])
    (ds / "models_eval" / "models_info.json").write_text(json.dumps({"1": {"diameter": float(gold["diameters"][0])},
                                                                       "2": {"diameter": float(gold["diameters"][1])}}))
    _write_obj(root / "models_inf" / "meshA" / "meshA.obj", gold["mesh_A_v"], gold["mesh_A_f"])      # the GT shape in mm: scale 0.001 -> s_e = 1
    meshes = {1: ops.Mesh(gold["gt_1_v"], gold["gt_1_f"]), 2: ops.Mesh(gold["gt_2_v"], gold["gt_2_f"])}
    rng = np.random.default_rng(3)
    targets, rows = [], ["scene_id,im_id,obj_id,score,R,t,bbox_visib,scale,time"]
    for scene in (1, 2):
        sd = ds / "test" / f"{scene:06d}"
        (sd / "depth").mkdir(parents=True)
        gts, cams, infos = {}, {}, {}
        for im in (1, 2, 3):
            ims = []
            depth = np.full((H, W), 1500.0, np.float32)
            for obj, x0 in ((1, -110.0), (2, 120.0)):
                q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
                R = q * np.sign(np.linalg.det(q))
                t = np.array([x0 + rng.normal() * 10, rng.normal() * 20, 780.0 + 40.0 * im])
                ims.append({"cam_R_m2c": R.reshape(-1).tolist(), "cam_t_m2c": t.tolist(), "obj_id": obj})
                d = ops.rasterize(meshes[obj], torch.from_numpy(_pose(R, t)[None]), 1.0, K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H)[1][0].cpu().numpy()
                depth = np.where((d > 0) & (d < depth), d, depth)
                targets.append({"scene_id": scene, "im_id": im, "obj_id": obj, "inst_count": 1})
                if obj == 1:
                    for k, sh in enumerate(SHIFTS):
                        te = t + sh * np.array([3.0, 0.0, -6.0])
                        rows.append(f"{scene},{im},meshA,{0.9 - 0.1 * k},{' '.join(repr(float(x)) for x in R.reshape(-1))},"
                                    f"{' '.join(repr(float(x)) for x in te)},0 0 10 10,0.001,0.25")
            gts[str(im)], cams[str(im)] = ims, {"cam_K": K.reshape(-1).tolist(), "depth_scale": 0.1}
            infos[str(im)] = [{"bbox_visib": [0, 0, 10, 10]}, {"bbox_visib": [0, 0, 10, 10]}]
            Image.fromarray(np.round(depth * 10.0).astype(np.uint16)).save(sd / "depth" / f"{im:06d}.png")
        (sd / "scene_gt.json").write_text(json.dumps(gts))
        (sd / "scene_camera.json").write_text(json.dumps(cams))
        (sd / "scene_gt_info.json").write_text(json.dumps(infos))
    (ds / "test_targets_bop19.json").write_text(json.dumps(targets))
    (root / "results").mkdir()
    (root / "results" / "hip_toyds-test.csv").write_text("\n".join(rows) + "\n")


def _run_cli(root, error_type, eval_dir, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    if env_extra is None:
        env.pop("SLURM_ARRAY_TASK_ID", None)
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "scripts.eval_calc_errors", "--error_type", error_type,
           "--result_filenames", "hip_toyds-test.csv", "--results_path", str(root / "results"), "--eval_path", str(eval_dir),
           "--models_inference_path", str(root / "models_inf"), "--datasets_path", str(root / "datasets"), "--vsd_deltas", "toyds:15",
           "--renderer_type", "vispy"]
    t0 = time.time()
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)      # a fresh child process per run
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    print(f"CLI {error_type}: {time.time() - t0:.2f} s wall")
    return r


def test_cli_end_to_end_on_a_synthetic_bop_dataset(gold, tmp_path):
    from PIL import Image
    from freepose_amd import mesh_io
    from freepose_amd.evaluation import PoseErrorEvaluator
    from freepose_amd.scripts import eval_calc_errors as cli
    _make_dataset(gold, tmp_path)
    K, W, H = gold["K"], int(gold["width"]), int(gold["height"])
    schema = set(json.loads(str(gold["toy_errors_json"]))[0])
    # the same pairs through the evaluator in this process
    ev = PoseErrorEvaluator(W, H)
    ds = tmp_path / "datasets" / "toyds"
    for o in (1, 2):
        ev.add_gt_model(o, mesh_io.load_ply(ds / "models_eval" / f"obj_{o:06d}.ply"))
    inf = mesh_io.load_obj(tmp_path / "models_inf" / "meshA" / "meshA.obj")
    assert inf.vertices_f64 is not None and inf.vertices_f64.dtype == np.float64
    ests = cli.load_results_csv(tmp_path / "results" / "hip_toyds-test.csv")
    diam = {1: float(gold["diameters"][0]), 2: float(gold["diameters"][1])}
    taus = cli.VSD_TAUS
    for et in ("cus", "chamfer", "chamfer_proj", "vsd"):
        out = tmp_path / f"eval_{et}"
        _run_cli(tmp_path, et, out)
        signs = [cli.error_signature("vsd", 1, 15.0, t) for t in taus] if et == "vsd" else [cli.error_signature(et, 1)]
        for scene in (1, 2):
            scene_gt = cli.load_scene_gt(ds / "test" / f"{scene:06d}" / "scene_gt.json")
            for ti, sign in enumerate(signs):
                f = out / "hip_toyds-test" / sign / f"errors_{scene:06d}.json"
                assert f.exists(), f
                recs = json.loads(f.read_text())
                assert len(recs) == 3 * 2 * len(SHIFTS) and all(set(r) == schema for r in recs)
                for im in (1, 2, 3):
                    mine = [r for r in recs if r["im_id"] == im and r["obj_id"] == 1]
                    assert [r["est_id"] for r in mine] == [0, 1, 2, 3] and all(list(r["errors"]) == ["0"] for r in mine)
                    vals = [r["errors"]["0"][0] for r in mine]
                    es = [e for e in ests if e["scene_id"] == scene and e["im_id"] == im]
                    gt = scene_gt[im][0]
                    pairs = [(inf, e["scale"] * 1000, e["R"], e["t"], 1, gt["cam_R_m2c"], gt["cam_t_m2c"]) for e in es]
                    if et == "vsd":
                        dpt = np.asarray(Image.open(ds / "test" / f"{scene:06d}" / "depth" / f"{im:06d}.png")).astype(np.float32)
                        dpt *= 0.1
                        want = [v[ti] for v in ev.errors("vsd", pairs, K, depth_test=dpt, vsd_delta=15.0, vsd_taus=taus,
                                                         vsd_normalized_by_diameter=True, diameters=diam)]
                        assert vals == want, (scene, im, sign)
                        # the step cost counts pixels whose distance difference reaches tau: between two neighbouring shifts no pixel
                        # may cross a large tau, so neighbours may tie; from the exact pose (0) to the largest shift the error must rise
                        assert all(b >= a for a, b in zip(vals, vals[1:])) and vals[0] == 0.0 and vals[-1] > vals[0], (sign, vals)
                    else:
                        assert vals == ev.errors(et, pairs, K), (et, scene, im)
                        assert all(b > a for a, b in zip(vals, vals[1:])), (et, vals)         # grows with the perturbation
                        if et == "cus":
                            assert vals[0] == 0.0                                            # the unperturbed estimate
                    other = [r for r in recs if r["im_id"] == im and r["obj_id"] == 2]       # every estimate also meets the other target
                    assert len(other) == len(SHIFTS) and all(list(r["errors"]) == ["1"] for r in other)
    out = tmp_path / "eval_slurm"
    _run_cli(tmp_path, "cus", out, {"SLURM_ARRAY_TASK_ID": "1"})
    files = sorted(p.name for p in out.rglob("errors_*.json"))
    assert files == ["errors_000002.json"], files
    assert (out / "hip_toyds-test" / "error=cus_ntop=1" / "errors_000002.json").read_text() == \
        (tmp_path / "eval_cus" / "hip_toyds-test" / "error=cus_ntop=1" / "errors_000002.json").read_text()
