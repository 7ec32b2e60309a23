"""No-GPU checks of the ground-truth info feature: (1) the numpy restatement of tests/_gt_info_ref.py against tests/golden/gt_info.npz,
which the reference's own depth_im_to_dist_im_fast / estimate_visib_mask_gt / calc_2d_bbox / calc_pts_diameter / save_json wrote
(tools/gen_golden_gt_info.py), dicts, masks, diameters and JSON text included; (2) tools/gt_info_host_check.cpp — csrc/gt_info_core.h run
serially, built with -fsanitize=address,undefined — against both, exactly; (3) the host layer of freepose_amd.evaluation: dict keys and
their order, the JSON text, refusals; (4) the boundary: parser defaults, header / ctypes entries, the C entries' refusals.  Everything is
compared with ==: the device side does comparisons, integer sums and one fixed-order fp64 expression."""
import ctypes as C
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _gt_info_ref as ref

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir / "gt_info.npz")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("gi_host") / "gt_info_host_check"
    cmd = [gxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "freepose_amd" / "csrc"), str(ROOT / "tools" / "gt_info_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def vis():
    cases = ref.vis_cases()
    return {name: (c, ref.run_case(c)) for name, c in cases.items()}


def rendered_case(gold, large):
    """the fixture's six instances as a case of the restatement: the canvases (calc_gt_info) or the image-size renders (calc_gt_masks)"""
    W, H = int(gold["width"]), int(gold["height"])
    test = gold["depth_u16"].astype(np.float32)
    test *= float(gold["depth_scale"])
    n = len(gold["canvases"])
    return dict(depth_gt=gold["canvases"] if large else gold["renders"], depth_test=test[None], img_idx=[0] * n, K=np.stack([gold["K"]] * n),
                delta=int(gold["delta"]), window=(W, H) if large else (0, 0))


def unpacked(bits, shape):
    return 255 * np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape)


# ---- (1) the restatement against the reference's values ----------------------------------------------------------------------------
def test_restatement_matches_the_reference_on_rendered_instances(gold):
    infos, rows, _, _ = ref.run_case(rendered_case(gold, True))
    want = json.loads(str(gold["infos"]))
    assert infos == want and [list(i) for i in infos] == [ref.INFO_KEYS] * len(want)
    assert ref.save_json_text({7: infos[:4], 12: infos[4:]}) == str(gold["info_text"])
    # the fixture holds what it was made for: a truncated silhouette, one only in the ring, an empty one, an occluded one
    assert want[1]["bbox_obj"][0] < 0 and want[3]["px_count_all"] > 0 and want[3]["bbox_obj"] == [-1] * 4 == want[3]["bbox_visib"]
    assert want[4]["px_count_all"] == 0 and want[4]["visib_fract"] == 0.0 and 0 < want[5]["visib_fract"] < 0.9
    _, _, masks, visibs = ref.run_case(rendered_case(gold, False))
    assert (np.stack([masks, visibs], axis=1) == unpacked(gold["masks"], (len(want), 2) + masks.shape[1:])).all()


def test_restatement_matches_the_reference_on_planted_stacks(gold, vis):
    planted = json.loads(str(gold["planted"]))
    assert sorted(planted) == sorted(vis)
    for name, (c, (infos, rows, masks, visibs)) in vis.items():
        assert infos == planted[name], name
        assert (np.stack([masks, visibs], axis=1) == unpacked(gold["planted_masks_" + name], (len(infos), 2) + masks.shape[1:])).all(), name


def test_planted_cases_hold_what_they_are_named_for(vis):
    rows = vis["truth"][1][1][0]
    # 12 columns of 4 x 48 pixels: d_gt > 0 in 6 of them; d_test > 0 in 3 of those; visible = test missing (3) or in front of / inside the band (2)
    assert rows[:3].tolist() == [6 * 192, 3 * 192, 5 * 192] and rows[4:].tolist() == [24, 0, 47, 47, 24, 0, 43, 47]
    infos = vis["ulp"][1][0]
    assert [i["px_count_visib"] for i in infos] == [1, 0, 1] and infos[0]["bbox_visib"] == [18, 14, 0, 0] and infos[1]["bbox_obj"] == [-1] * 4
    e = vis["edges"][1][0]
    assert e[1]["px_count_valid"] == 0 and e[1]["px_count_visib"] > 0                       # all-zero test image: the whole mask is visible
    assert (vis["edges"][1][3][1] == vis["edges"][1][2][1]).all()
    assert e[2] == {"px_count_all": 0, "px_count_valid": 0, "px_count_visib": 0, "visib_fract": 0.0, "bbox_obj": [-1] * 4, "bbox_visib": [-1] * 4}
    assert e[3]["px_count_all"] > 0 and e[3]["bbox_obj"] == [-1] * 4 == e[3]["bbox_visib"]  # only in the truncated ring
    assert e[4]["px_count_visib"] == 1 and e[4]["bbox_visib"][2:] == [0, 0]                 # one visible pixel
    assert e[5]["px_count_visib"] == 4 and e[5]["bbox_visib"] == [0, 0, 63, 47]             # the four corners
    assert e[6]["bbox_obj"] == [-64, -48, 191, 143]                                         # touching the canvas border all round
    c = vis["odd_canvas"][0]
    assert c["depth_gt"].shape[2] % 4 and c["window"][0] % 2 == 1 and c["delta"] == 7.3


def test_diameter_restatement_matches_the_reference(gold):
    want = json.loads(str(gold["diameters"]))
    clouds = ref.diam_cases(big=False)
    for name, values in want.items():
        cl = [clouds["tiles"][2]] if name == "tile_plus_1" else clouds[name]
        assert [ref.pts_diameter(p) for p in cl] == values, name
    assert want["tiny"][0] == 0.0 and want["dup"] == [0.0, 13.0]
    p = clouds["assoc"][0]
    d = p[:, None, :] - p[None, :, :]
    assert ref.pair_d2(d).max() != ref.pair_d2_other(d).max()                # the two associations differ on this cloud ...
    assert ref.pts_diameter(p) != ref.pts_diameter(p, d2=ref.pair_d2_other)  # ... and so do the diameters
    info = ref.model_info(gold["mesh_v"].astype(np.float64))
    assert list(info) == ref.MODEL_KEYS and ref.save_json_text({3: info}) == str(gold["models_info_text"])


# ---- (2) the host check ------------------------------------------------------------------------------------------------------------
def test_host_check_matches_on_every_case(host_check, tmp_path, gold, vis):
    for name, (c, (_, rows, masks, visibs)) in list(vis.items()) + [("rendered", (rendered_case(gold, True), ref.run_case(rendered_case(gold, True))))]:
        got_rows, got_m, got_v = ref.host_visibility(host_check, tmp_path, c)
        assert (got_rows == rows).all() and (got_m == masks).all() and (got_v == visibs).all(), name
        assert (ref.host_visibility(host_check, tmp_path, c, want_masks=False)[0] == rows).all(), name
    for name, cl in ref.diam_cases(big=False).items():
        got = ref.host_diameter(host_check, tmp_path, cl)
        assert (got == np.stack([ref.model_row(p) for p in cl])).all(), name


def test_host_check_refuses_what_the_entries_refuse(host_check, tmp_path, vis):
    c = dict(vis["odd_canvas"][0])
    for window in ((75, 29), (37, 59), (-1, 0)):                             # the window leaves the canvas
        bad = dict(c, window=window)
        fin = tmp_path / "bad.bin"
        gt, test = bad["depth_gt"], bad["depth_test"]
        head = np.array([2, gt.shape[1], gt.shape[2], window[0], window[1], 2, test.shape[1], test.shape[2], 0], np.int32)
        fin.write_bytes(head.tobytes() + np.zeros(2, np.int32).tobytes() + np.zeros(16).tobytes() + gt.tobytes() + test.tobytes())
        assert subprocess.run([str(host_check), "visibility", str(fin), str(tmp_path / "o.bin")]).returncode == 3, window
    with pytest.raises(AssertionError):
        ref.host_visibility(host_check, tmp_path, dict(c, img_idx=[0, 2]))    # image index outside [0, n_img)
    cl = ref.diam_cases(big=False)["tiny"]
    for ranges in ([[0, 0]], [[-1, 2]], [[5, 2]], [[0, 7]]):                  # count 0, before the table, beyond it
        assert ref.host_diameter(host_check, tmp_path, cl, ranges) is None, ranges
    assert ref.host_diameter(host_check, tmp_path, cl, [[4, 2]]) is not None  # the last two of the six points


# ---- (3) the host layer ------------------------------------------------------------------------------------------------------------
def test_gt_info_from_counts_is_the_reference_dict(gold, vis):
    from freepose_amd.evaluation import GT_INFO_KEYS, MODEL_INFO_KEYS, bop_json_text, gt_info_from_counts, model_info_from_row
    assert list(GT_INFO_KEYS) == ref.INFO_KEYS and list(MODEL_INFO_KEYS) == ref.MODEL_KEYS
    for name, (c, (infos, rows, _, _)) in vis.items():
        got = [gt_info_from_counts(r) for r in rows]
        assert got == infos and all(list(g) == ref.INFO_KEYS for g in got), name
        assert all(type(v) is int for g in got for k in ("px_count_all", "px_count_valid", "px_count_visib") for v in [g[k]])
        assert all(type(g["visib_fract"]) is float for g in got)
    infos, rows, _, _ = ref.run_case(rendered_case(gold, True))
    got = [gt_info_from_counts(r) for r in rows.astype(np.int32)]
    assert bop_json_text({7: got[:4], 12: got[4:]}) == str(gold["info_text"])
    # px_count_all > 0 without a visible pixel: BOTH boxes are -1 although the silhouette has a box
    r = [40, 0, 0, 0, -30, -20, -21, -11, *ref.BOX_EMPTY]
    assert gt_info_from_counts(r) == {"px_count_all": 40, "px_count_valid": 0, "px_count_visib": 0, "visib_fract": 0.0, "bbox_obj": [-1] * 4,
                                      "bbox_visib": [-1] * 4}
    row = ref.model_row(gold["mesh_v"].astype(np.float64))
    info = model_info_from_row(row)
    assert list(info) == ref.MODEL_KEYS and bop_json_text({3: info}) == str(gold["models_info_text"])


def test_calculator_refusals_need_no_device():
    from freepose_amd.evaluation import GtInfoCalculator
    with pytest.raises(ValueError, match="2731 x 100"):                       # 3 x 2731 = 8193 > 8192
        GtInfoCalculator(2731, 100).gt_info([("a", 1, np.eye(3), [0, 0, 500])], {"a": np.zeros((100, 2731), np.float32)}, {"a": np.eye(3)})
    with pytest.raises(ValueError, match="100 x 2731"):
        GtInfoCalculator(100, 2731).gt_info([("a", 1, np.eye(3), [0, 0, 500])], {"a": np.zeros((2731, 100), np.float32)}, {"a": np.eye(3)})
    with pytest.raises(ValueError):
        GtInfoCalculator(0, 10)
    assert GtInfoCalculator(64, 48).gt_info([], {}, {}) == []
    m, v = GtInfoCalculator(64, 48).gt_masks([], {}, {})
    assert m.shape == v.shape == (0, 48, 64) and m.dtype == np.uint8


# ---- (4) the boundary --------------------------------------------------------------------------------------------------------------
def test_parser_defaults_are_the_reference_parameters(monkeypatch):
    from freepose_amd.scripts import calc_gt_info, calc_gt_masks, calc_model_info
    import scripts.calc_gt_info, scripts.calc_gt_masks, scripts.calc_model_info  # noqa: F401,E401  (the aliases import)
    monkeypatch.delenv("BOP_PATH", raising=False)
    for mod in (calc_gt_info, calc_gt_masks, calc_model_info):
        p = mod.params_from_args(mod.build_parser().parse_args([]))
        assert p == {"dataset": "lm", "dataset_split": "test", "dataset_split_type": None, "delta": 15, "model_type": None,
                     "renderer_type": "vispy", "datasets_path": "bop_datasets", "scene_ids": []}, mod.__name__
        assert type(p["delta"]) is int
    monkeypatch.setenv("BOP_PATH", "/data/bop")
    p = calc_gt_info.params_from_args(calc_gt_info.build_parser().parse_args(
        ["--dataset", "itodd", "--delta", "5", "--model_type", "eval", "--scene_ids", "3,1", "--dataset_split_type", "primesense", "--renderer_type", "cpp"]))
    assert p["datasets_path"] == "/data/bop" and p["delta"] == 5 and p["scene_ids"] == [3, 1] and p["dataset_split_type"] == "primesense"
    assert calc_gt_info.models_path(p) == Path("/data/bop/itodd/models_eval") and calc_gt_info.split_path(p) == Path("/data/bop/itodd/test_primesense")
    assert calc_gt_info.params_from_args(calc_gt_info.build_parser().parse_args(["--delta", "7.5"]))["delta"] == 7.5


def test_scene_selection(tmp_path, monkeypatch):
    from freepose_amd.scripts import calc_gt_info as cli
    for s in (4, 9, 2):
        (tmp_path / "toy" / "test" / f"{s:06d}").mkdir(parents=True)
    (tmp_path / "toy" / "test" / "notes").mkdir()
    p = cli.params_from_args(cli.build_parser().parse_args(["--dataset", "toy", "--datasets_path", str(tmp_path)]))
    monkeypatch.delenv("SLURM_ARRAY_TASK_ID", raising=False)
    assert cli.scene_ids(p) == [2, 4, 9] and cli.scene_ids(dict(p, scene_ids=[9, 2])) == [2, 9]
    monkeypatch.setenv("SLURM_ARRAY_TASK_ID", "1")
    assert cli.scene_ids(p) == [4] and cli.scene_ids(dict(p, scene_ids=[9, 2])) == [9]
    monkeypatch.setenv("SLURM_ARRAY_TASK_ID", "3")
    with pytest.raises(IndexError):
        cli.scene_ids(p)
    monkeypatch.delenv("SLURM_ARRAY_TASK_ID")
    with pytest.raises(FileNotFoundError):
        cli.scene_ids(dict(p, scene_ids=[5]))


def test_entries_are_declared_and_refuse_bad_sizes_without_a_gpu():
    from freepose_amd import _lib, ops
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "freepose_hip.h").read_text(), flags=re.S)
    for name, n in (("fp_gt_visibility", 17), ("fp_pts_diameter", 7)):
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(proto.split(",")) == n == len(_lib.SIGNATURES[name][1]), name
    text = (ROOT / "include" / "freepose_hip.h").read_text()
    for cited in ("calc_gt_info.py:125-173", "calc_gt_masks.py:107-126", "misc.py:289-303", "calc_model_info.py:36-37", "visibility.py:34-38"):
        assert cited in text, cited
    core = (ROOT / "freepose_amd" / "csrc" / "gt_info_core.h").read_text()
    assert int(re.search(r"#define FP_GI_OUT_LD (\d+)", core).group(1)) == ops.GT_INFO_OUT_LD == 12
    hip = (ROOT / "freepose_amd" / "csrc" / "gt_info.hip").read_text()
    assert "DM_THREADS = 256" in hip and "DM_IPL = 4" in hip and ops.DIAMETER_TILE == ref.TILE == 1024
    internal = (ROOT / "freepose_amd" / "csrc" / "internal.h").read_text()
    assert "#define FP_DIAM_MAX_POINTS (1 << 21)" in internal and ops.DIAMETER_MAX_POINTS == 1 << 21
    lib = _lib.load()
    buf = np.zeros(64)
    p = C.c_void_p(buf.ctypes.data)              # never dereferenced: every call below is refused before it touches the device
    vis = lambda *a: lib.fp_gt_visibility(*a)    # noqa: E731
    assert vis(None, p, 1, 12, 12, 4, 4, p, 1, 4, 4, p, p, None, None, p, None) == 1 and b"gt_visibility: null context" in lib.fp_last_error()
    for B, Hr, Wr, ox, oy, n_img, H, W in ((-1, 12, 12, 4, 4, 1, 4, 4), (65536, 12, 12, 4, 4, 1, 4, 4), (1, 0, 12, 0, 0, 1, 4, 4),
                                           (1, 12, 12, 9, 4, 1, 4, 4), (1, 12, 12, 4, 9, 1, 4, 4), (1, 12, 12, -1, 4, 1, 4, 4),
                                           (1, 12, 12, 4, 4, 1, 0, 4), (1, 12, 12, 4, 4, 0, 4, 4), (1, 40000, 40000, 0, 0, 1, 4, 4)):
        assert vis(p, p, B, Hr, Wr, ox, oy, p, n_img, H, W, p, p, None, None, p, None) == 1, (B, Hr, Wr, ox, oy, n_img, H, W)
        assert b"gt_visibility" in lib.fp_last_error()
    assert vis(p, p, 1, 12, 12, 9, 4, p, 1, 4, 4, p, p, None, None, p, None) == 1 and b"leaves the canvas" in lib.fp_last_error()
    for args in ((None, 1, p, p, p), (p, 1, None, p, p), (p, 1, p, None, p), (p, 1, p, p, None)):      # null stacks
        gt, _, test, idx, out = args
        assert vis(p, gt, 1, 12, 12, 4, 4, test, 1, 4, 4, idx, p, None, None, out, None) == 1 and b"null" in lib.fp_last_error()
    assert vis(p, None, 0, 12, 12, 4, 4, None, 1, 4, 4, None, None, None, None, None, None) == 0       # B = 0: nothing to do
    dia = lambda *a: lib.fp_pts_diameter(*a)     # noqa: E731
    assert dia(None, p, 4, p, 1, p, None) == 1 and b"pts_diameter: null context" in lib.fp_last_error()
    for M, n_pts in ((-1, 4), (65536, 4), (1, -1)):
        assert dia(p, p, n_pts, p, M, p, None) == 1 and b"pts_diameter" in lib.fp_last_error(), (M, n_pts)
    assert dia(p, None, 4, p, 1, p, None) == 1 and b"null" in lib.fp_last_error()
    assert dia(p, None, 0, None, 0, None, None) == 0
