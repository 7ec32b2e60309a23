"""Ground-truth visibility / masks / boxes and model diameters on the MI355X (csrc/gt_info.hip) against the numpy restatement of
tests/_gt_info_ref.py and tests/golden/gt_info.npz, which the reference's own depth_im_to_dist_im_fast / estimate_visib_mask_gt /
calc_2d_bbox / calc_pts_diameter / save_json wrote (tools/gen_golden_gt_info.py).

Everything is compared with ==.  The visibility pass forms the reference's float64 expressions per pixel and adds integers; the diameter
is a maximum of one fixed-order fp64 expression and one correctly rounded square root: there is no tolerance to choose."""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import _gt_info_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir / "gt_info.npz")


@pytest.fixture(scope="module")
def vis():
    """name -> (case, the restatement's answer), computed once"""
    cases = dict(ref.vis_cases(), big=ref.big_case())
    return {name: (c, ref.run_case(c)) for name, c in cases.items()}


@pytest.fixture(scope="module")
def diam():
    """name -> (clouds, the restatement's rows), computed once"""
    return {name: (cl, np.stack([ref.model_row(p) for p in cl])) for name, cl in ref.diam_cases().items()}


def _vis(c, sl=slice(None), want_masks=True):
    from freepose_amd import ops
    window = None if c["window"] == (0, 0) else c["window"]
    out = ops.gt_visibility(c["depth_gt"][sl], c["depth_test"], c["img_idx"][sl], c["K"][sl], c["delta"], window=window, want_masks=want_masks)
    return [None if t is None else t.cpu().numpy() for t in out]


# ---- visibility --------------------------------------------------------------------------------------------------------------------
def test_visibility_equals_the_restatement_on_every_case(vis, gold):
    planted = json.loads(str(gold["planted"]))
    from freepose_amd.evaluation import gt_info_from_counts
    for name, (c, (infos, rows, masks, visibs)) in vis.items():
        got, m, v = _vis(c)
        assert got.dtype == np.int32 and got.shape == rows.shape and np.array_equal(got, rows), (name, got.tolist(), rows.tolist())
        assert m.dtype == np.uint8 and np.array_equal(m, masks) and np.array_equal(v, visibs), name
        assert [gt_info_from_counts(r) for r in got] == infos, name
        if name in planted:
            assert [gt_info_from_counts(r) for r in got] == planted[name], name         # what the reference's functions returned
        again, m2, v2 = _vis(c)
        assert np.array_equal(again, got) and np.array_equal(m2, m) and np.array_equal(v2, v), name     # two calls, the same bits
        bare, none_m, none_v = _vis(c, want_masks=False)                                               # both mask outputs NULL
        assert none_m is None and none_v is None and np.array_equal(bare, rows), name
    big = vis["big"][0]["depth_gt"]
    assert big.shape == (1, 1440, 1920) and big.size // 4 > 128 * 256                    # more groups of 4 than the launch has lanes
    assert vis["odd_canvas"][0]["depth_gt"].shape[2] % 4 == 3 and vis["odd_image"][0]["window"] == (0, 0)


def test_visibility_batch_sizes_and_split_launches(vis, monkeypatch):
    from freepose_amd import ops
    c, (_, rows, masks, visibs) = vis["edges"]
    assert len(rows) == 7 and c["depth_test"].shape[0] == 3 and sorted(set(c["img_idx"])) == [0, 1, 2]
    for n in (1, 5):
        got, m, v = _vis(c, slice(0, n))
        assert np.array_equal(got, rows[:n]) and np.array_equal(m, masks[:n]) and np.array_equal(v, visibs[:n]), n
    monkeypatch.setattr(ops, "GT_INFO_MAX_BATCH", 3)                                      # 7 instances: launches of 3, 3 and 1
    got, m, v = _vis(c)
    assert np.array_equal(got, rows) and np.array_equal(m, masks) and np.array_equal(v, visibs)
    empty, m, v = _vis(c, slice(0, 0))
    assert empty.shape == (0, 12) and m.shape == (0, 48, 64)


def test_visibility_refusals(vis):
    import torch
    from freepose_amd import _lib, ops
    c = vis["odd_canvas"][0]
    for window in ((75, 29), (37, 59), (-1, 0), None):                                    # leaves the canvas; None: canvases are not image-size
        with pytest.raises(ValueError):
            ops.gt_visibility(c["depth_gt"], c["depth_test"], c["img_idx"], c["K"], c["delta"], window=window)
    for idx in ([0, 2], [-1, 0], [0]):
        with pytest.raises(ValueError):
            ops.gt_visibility(c["depth_gt"], c["depth_test"], idx, c["K"], c["delta"], window=c["window"])
    # the C entry reads the indices back and refuses the call itself: nothing is launched, the output keeps its bytes
    lib = _lib.load()
    gt, test = torch.from_numpy(c["depth_gt"]).cuda(), torch.from_numpy(c["depth_test"]).cuda()
    idx = torch.tensor([1, 2], dtype=torch.int32).cuda()
    prm = torch.zeros((2, 8), dtype=torch.float64).cuda()
    out = torch.full((2, 12), 77, dtype=torch.int32).cuda()
    rc = lib.fp_gt_visibility(ops.context(), _lib.ptr(gt), 2, gt.shape[1], gt.shape[2], 37, 29, _lib.ptr(test), 2, 29, 37, _lib.ptr(idx),
                              _lib.ptr(prm), None, None, _lib.ptr(out), _lib.current_stream())
    assert rc == 1 and b"d_img_idx[1] = 2" in lib.fp_last_error()
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 77).all()


def test_calculator_on_the_rendered_fixture(gold):
    """the fixture's six instances through the HIP rasteriser and the fused pass: the dicts, JSON text and masks the reference's functions
    gave on the oracle rasteriser's depth images"""
    from freepose_amd import evaluation as ev
    from freepose_amd.mesh_io import TriMesh
    W, H = int(gold["width"]), int(gold["height"])
    test = gold["depth_u16"].astype(np.float32)
    test *= float(gold["depth_scale"])
    calc = ev.GtInfoCalculator(W, H, int(gold["delta"])).add_model(3, TriMesh(gold["mesh_v"], gold["mesh_f"]))
    inst = [("im7" if i < 4 else "im12", 3, R, t) for i, (R, t) in enumerate(zip(gold["pose_R"], gold["pose_t"]))]
    depths, Ks = {"im7": test, "im12": test.copy()}, {"im7": gold["K"], "im12": gold["K"]}
    infos = calc.gt_info(inst, depths, Ks)
    assert infos == json.loads(str(gold["infos"])) and all(list(i) == list(ev.GT_INFO_KEYS) for i in infos)
    assert ev.bop_json_text({7: infos[:4], 12: infos[4:]}) == str(gold["info_text"])
    masks, visibs = calc.gt_masks(inst, depths, Ks)
    want = 255 * np.unpackbits(gold["masks"])[:6 * 2 * H * W].reshape(6, 2, H, W)
    assert np.array_equal(masks, want[:, 0]) and np.array_equal(visibs, want[:, 1])
    saved = ev.GT_INFO_CANVAS_PIXELS_PER_BATCH
    try:                                                                                 # one canvas per batch: the same answers
        ev.GT_INFO_CANVAS_PIXELS_PER_BATCH = 1
        assert calc.gt_info(inst, depths, Ks) == infos
    finally:
        ev.GT_INFO_CANVAS_PIXELS_PER_BATCH = saved
    with pytest.raises(KeyError):
        calc.gt_info([("im7", 4, np.eye(3), [0, 0, 500])], depths, Ks)
    with pytest.raises(ValueError, match="64 x 48"):
        calc.gt_info(inst[:1], {"im7": test[:, :60]}, Ks)


# ---- diameter ----------------------------------------------------------------------------------------------------------------------
def test_diameter_equals_the_restatement_on_every_case(diam, gold):
    from freepose_amd import ops
    golden = json.loads(str(gold["diameters"]))
    sizes = [len(p) for p in diam["tiles"][0]]
    assert sizes[:4] == [ref.TILE - 1, ref.TILE, ref.TILE + 1, 2 * ref.TILE + 5] and [len(p) for p in diam["tiny"][0]] == [1, 2, 3]
    assert len(diam["big"][0][0]) == 8192
    for name, (clouds, want) in diam.items():
        got = ops.pts_diameter(clouds).cpu().numpy()
        assert got.dtype == np.float64 and got.shape == want.shape
        assert np.array_equal(got, want), (name, got[:, 0].tolist(), want[:, 0].tolist())
        assert np.array_equal(ops.pts_diameter(clouds).cpu().numpy(), got), name          # two calls, the same bits
        if name in golden:
            assert got[:, 0].tolist() == golden[name], name                               # misc.calc_pts_diameter's own values
    assert diam["tiles"][1][2, 0] == golden["tile_plus_1"][0]
    for k, (a, b) in enumerate(((0, ref.TILE - 2), (5, 900), (10, ref.TILE), (10, 2 * ref.TILE + 2))):     # the planted farthest pairs
        p = diam["tiles"][0][k]
        assert diam["tiles"][1][k, 0] == float(np.sqrt(ref.pair_d2(p[a] - p[b])))
    p = diam["assoc"][0][0]
    assert diam["assoc"][1][0, 0] != ref.pts_diameter(p, d2=ref.pair_d2_other)            # checked on the CPU: the associations differ here
    # one model of the mesh: the reference's models_info text
    from freepose_amd.evaluation import bop_json_text, models_info
    assert bop_json_text(models_info({3: gold["mesh_v"].astype(np.float64)})) == str(gold["models_info_text"])


def test_diameter_several_models_and_split_launches(diam, monkeypatch):
    from freepose_amd import ops
    names = ("tiny", "dup", "scales", "tiles", "assoc")
    clouds = [p for n in names for p in diam[n][0]]
    want = np.concatenate([diam[n][1] for n in names])
    assert np.array_equal(ops.pts_diameter(clouds).cpu().numpy(), want)                   # 14 models of 1 .. 2053 points in one call
    monkeypatch.setattr(ops, "DIAMETER_MAX_MODELS", 4)
    assert np.array_equal(ops.pts_diameter(clouds).cpu().numpy(), want)
    monkeypatch.setattr(ops, "DIAMETER_MAX_SLOTS", 6)                                     # a 3-tile model needs 6 slots: launches of one such model
    assert np.array_equal(ops.pts_diameter(clouds).cpu().numpy(), want)
    monkeypatch.setattr(ops, "DIAMETER_MAX_SLOTS", 5)
    with pytest.raises(ValueError, match="slots"):
        ops.pts_diameter(clouds)
    assert ops.pts_diameter([]).shape == (0, 8)


def test_diameter_refusals(diam):
    import torch
    from freepose_amd import _lib, ops
    with pytest.raises(ValueError, match="cloud 1 is empty"):
        ops.pts_diameter([np.zeros((3, 3)), np.zeros((0, 3))])
    lib = _lib.load()
    pts = torch.from_numpy(np.concatenate(diam["tiny"][0])).cuda()                        # 6 points
    out = torch.full((1, 8), 5.0, dtype=torch.float64).cuda()
    for first, count in ((0, 0), (-1, 2), (5, 2), (0, 7)):
        rg = torch.tensor([[first, count]], dtype=torch.int32).cuda()
        rc = lib.fp_pts_diameter(ops.context(), _lib.ptr(pts), 6, _lib.ptr(rg), 1, _lib.ptr(out), _lib.current_stream())
        assert rc == 1 and b"is empty or outside [0, 6]" in lib.fp_last_error(), (first, count)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 5.0).all()


# ---- the three commands, end to end -------------------------------------------------------------------------------------------------
def test_clis_end_to_end_then_eval_bop19_pose(golden_dir, tmp_path, monkeypatch):
    """the toy dataset of tests/test_gpu_eval.py without its scene_gt_info.json files and without the computed keys of models_info.json:
    the three commands write them, as the restatement gives them on the oracle rasteriser's depth images, and eval_bop19_pose runs on top"""
    from PIL import Image
    from freepose_amd.scripts import calc_gt_info, calc_gt_masks, calc_model_info, eval_bop19_pose as bop, eval_calc_errors as ce
    from oracle import fp_oracle as fo
    from tests.test_gpu_eval import _make_dataset, _pose
    for k in ("SLURM_JOB_ID", "SLURM_ARRAY_TASK_ID"):
        monkeypatch.delenv(k, raising=False)
    pe = np.load(golden_dir / "pose_errors.npz")
    _make_dataset(pe, tmp_path)
    ds = tmp_path / "datasets" / "toyds"
    W, H, K = int(pe["width"]), int(pe["height"]), pe["K"]
    for scene in (1, 2):
        (ds / "test" / f"{scene:06d}" / "scene_gt_info.json").unlink()
    (ds / "models_eval" / "models_info.json").write_text(json.dumps({"1": {"symmetries_discrete": [[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]]}}))
    common = ["--dataset", "toyds", "--datasets_path", str(tmp_path / "datasets"), "--model_type", "eval", "--renderer_type", "vispy"]
    # models_info.json
    calc_model_info.run(common)
    models = {o: ref.model_info(pe[f"gt_{o}_v"].astype(np.float64)) for o in (1, 2)}
    models[1]["symmetries_discrete"] = [[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]]    # kept
    assert (ds / "models_eval" / "models_info.json").read_text() == ref.save_json_text(models)
    # scene_gt_info.json and the masks
    calc_gt_info.run(common)
    calc_gt_masks.run(common + ["--scene_ids", "1,2"])
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    n_visible = 0
    for scene in (1, 2):
        sd = ds / "test" / f"{scene:06d}"
        scene_gt = ce.load_scene_gt(sd / "scene_gt.json")
        cams = ce.load_scene_camera(sd / "scene_camera.json")
        want = {}
        for im_id in sorted(scene_gt):
            depth = ce._load_depth(ds / "test", scene, im_id, cams[im_id]["depth_scale"])
            want[im_id] = []
            for gt_id, gt in enumerate(scene_gt[im_id]):
                v, f = pe[f"gt_{gt['obj_id']}_v"], pe[f"gt_{gt['obj_id']}_f"]
                pose = _pose(gt["cam_R_m2c"], gt["cam_t_m2c"].reshape(3))[None]
                canvas = fo.rasterize(v, f, None, pose, 1.0, fx, fy, cx + W, cy + H, 3 * W, 3 * H)[1][0]
                want[im_id].append(ref.instance(canvas, depth, K, 15, W, H)[0])
                render = fo.rasterize(v, f, None, pose, 1.0, fx, fy, cx, cy, W, H)[1][0]
                _, _, mask, visib = ref.instance(render, depth, K, 15, 0, 0)
                for folder, img in (("mask", mask), ("mask_visib", visib)):
                    with Image.open(sd / folder / f"{im_id:06d}_{gt_id:06d}.png") as png:
                        assert png.mode == "L" and np.array_equal(np.asarray(png), img), (scene, im_id, gt_id, folder)
                n_visible += want[im_id][-1]["px_count_visib"] > 0
        assert (sd / "scene_gt_info.json").read_text() == ref.save_json_text(want), scene
    assert n_visible == 12
    # the scoring chain on top, with the visib_fract values the command computed
    argv = ["--result_filenames", "hip_toyds-test.csv", "--results_path", str(tmp_path / "results"), "--eval_path", str(tmp_path / "evals"),
            "--datasets_path", str(tmp_path / "datasets"), "--models_inference_path", str(tmp_path / "models_inf"), "--renderer_type", "cpp"]
    final = bop.run(argv)["hip_toyds-test.csv"]
    saved = json.loads((tmp_path / "evals" / "hip_toyds-test" / "scores_bop19.json").read_text())
    assert saved == {k: float(v) for k, v in final.items()} and 0.0 < saved["bop19_average_recall"] < 1.0
    assert sorted(saved) == ["bop19_average_recall", "bop19_average_recall_chamfer", "bop19_average_recall_chamfer_proj", "bop19_average_recall_cus",
                             "bop19_average_time_per_image"]
