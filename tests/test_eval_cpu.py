"""No-GPU checks of the pose-error evaluation: the C ABI entries exist and refuse bad sizes, the PLY reader, the CLI's flags, CSV reader,
pairing rule and errors-JSON schema, and the fixture's own consistency.  tests/golden/pose_errors.npz is made by
tools/gen_golden_eval.py: its error values and pixel counts come from the reference's functions; of the toy errors JSON only the
SERIALISATION (keys, key order, text layout) is the reference's inout.save_json — the record list behind it (which estimate meets
which ground truth, est_id, order) was written down by hand from eval_calc_errors.py:311-368 in the generator, so the pairing test
pins this implementation to that reading, not to an execution of the reference's loop."""
import ctypes as C
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
REF_SCRIPT = Path("/root/reference/bop_toolkit/scripts/eval_calc_errors.py")


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir / "pose_errors.npz")


def test_eval_entry_points_refuse_bad_sizes_without_a_gpu():
    """fp_chamfer / fp_depth_compare are exported and check every size before they touch the device: status 1 + a message"""
    from freepose_amd import _lib, build
    build.build_hip(verbose=False)
    lib = _lib.load()
    assert hasattr(lib, "fp_chamfer") and hasattr(lib, "fp_depth_compare")
    buf = (C.c_double * 64)()
    ctx = C.c_void_p(1)                       # never dereferenced: every call below is refused on its sizes
    p = C.cast(buf, C.c_void_p)
    assert lib.fp_chamfer(None, p, 10, p, p, 1, 5, 10, 0, p, None) == 1 and b"chamfer: null" in lib.fp_last_error()
    for B, n_pts, max_n, ws, proj in ((0, 10, 5, 10, 0), (70000, 10, 5, 10, 0), (1, 0, 5, 10, 0), (1, 10, 0, 10, 0), (1, 10, 11, 10, 0),
                                      (1, 10, 5, 1, 0), (1, 10, 5, 11, 0), (1, 10, 5, 10, 2)):
        assert lib.fp_chamfer(ctx, p, n_pts, p, p, B, max_n, ws, proj, p, None) == 1, (B, n_pts, max_n, ws, proj)
        assert b"chamfer" in lib.fp_last_error()
    assert lib.fp_depth_compare(None, p, p, 1, 4, 4, None, 0, None, None, None, 0, p, None) == 1
    assert b"depth_compare: null" in lib.fp_last_error()
    for B, H, W, test, n_img, n_tau in ((0, 4, 4, None, 0, 0), (70000, 4, 4, None, 0, 0), (1, 0, 4, None, 0, 0), (1, 4, -1, None, 0, 0),
                                        (1, 4, 4, None, 0, 3), (1, 4, 4, p, 0, 3), (1, 4, 4, p, 1, 0), (1, 4, 4, p, 1, 17)):
        assert lib.fp_depth_compare(ctx, p, p, B, H, W, test, n_img, p, p, p, n_tau, p, None) == 1, (B, H, W, n_img, n_tau)
        assert b"depth_compare" in lib.fp_last_error()
    assert lib.fp_depth_compare(ctx, p, p, 1, 4, 4, p, 1, None, p, p, 3, p, None) == 1 and b"d_img_idx" in lib.fp_last_error()


def test_nn_kernel_has_no_scratch(tmp_path):
    """the nearest-neighbour kernel keeps its queries and running minima in registers: zero scratch in both instantiations"""
    from freepose_amd import build
    build.build_hip(verbose=False)
    obj = ROOT / "freepose_amd" / "lib" / "obj" / "eval.o"
    llvm = Path("/opt/rocm/lib/llvm/bin")
    if not (llvm / "clang-offload-bundler").exists() or not (llvm / "llvm-readelf").exists():
        pytest.skip("ROCm LLVM tools not found")
    fat, co = tmp_path / "eval.fatbin", tmp_path / "eval.co"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(obj), str(fat)], check=True)
    subprocess.run([str(llvm / "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950:sramecc+", f"--input={fat}",
                    f"--output={co}", "--unbundle"], check=True)
    notes = subprocess.run([str(llvm / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    kernels, name = {}, None
    for ln in notes.splitlines():
        m = re.search(r"\.name:\s+(\S+)", ln)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count"):
            m = re.search(r"\.%s:\s+(\d+)" % key, ln)
            if m and name:
                kernels[name][key] = int(m.group(1))
    nn = {k: v for k, v in kernels.items() if "eval_nn_kernel" in k}
    assert len(nn) == 2, sorted(kernels)
    for k, v in nn.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 128, (k, v)


def _write_ascii_ply(path, v, f, colors=None):
    lines = ["ply", "format ascii 1.0", "comment written by the test", f"element vertex {len(v)}", "property float x", "property float y",
             "property float z"]
    if colors is not None:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    for i, p in enumerate(v):
        lines.append(" ".join(repr(float(x)) for x in p) + ("" if colors is None else " " + " ".join(str(int(c)) for c in colors[i])))
    lines += ["3 " + " ".join(str(int(i)) for i in t) for t in f]
    Path(path).write_text("\n".join(lines) + "\n")


def _write_binary_ply(path, v, f, with_normals=False):
    props = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if with_normals else [])
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"] + [f"property float {n}" for n, _ in props]
    head += [f"element face {len(f)}", "property list uchar uint vertex_indices", "end_header"]
    a = np.zeros(len(v), dtype=props)
    a["x"], a["y"], a["z"] = np.asarray(v, np.float32).T
    r = np.zeros(len(f), dtype=[("k", "u1"), ("v", "<u4", (3,))])
    r["k"], r["v"] = 3, f
    Path(path).write_bytes(("\n".join(head) + "\n").encode() + a.tobytes() + r.tobytes())


def test_load_ply_round_trips_ascii_and_binary(tmp_path):
    from freepose_amd.mesh_io import load_mesh, load_ply
    rng = np.random.default_rng(5)
    v = rng.normal(size=(37, 3)) * 50
    f = rng.integers(0, 37, size=(61, 3)).astype(np.int32)
    col = rng.integers(0, 256, size=(37, 3))
    _write_ascii_ply(tmp_path / "a.ply", v, f, col)
    m = load_ply(tmp_path / "a.ply")
    assert m.pts.dtype == np.float64 and np.array_equal(m.pts, v) and np.array_equal(m.faces, f) and np.array_equal(m.vertex_colors, col)
    assert m.pts is m.vertices
    for normals in (False, True):
        _write_binary_ply(tmp_path / "b.ply", v, f, normals)
        m = load_mesh(tmp_path / "b.ply")
        assert np.array_equal(m.pts, v.astype(np.float32).astype(np.float64)) and np.array_equal(m.faces, f) and m.vertex_colors is None
    (tmp_path / "q.ply").write_text("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                                    "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError, match="triangular"):
        load_ply(tmp_path / "q.ply")
    (tmp_path / "be.ply").write_text("ply\nformat binary_big_endian 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError, match="binary_big_endian"):
        load_ply(tmp_path / "be.ply")


def test_cli_flags_match_the_reference_script():
    from freepose_amd.scripts import eval_calc_errors as e
    ap = e.build_parser()
    ours = {s for a in ap._actions for s in a.option_strings if s.startswith("--")} - {"--help"}
    expected = {"--n_top", "--error_type", "--vsd_deltas", "--vsd_taus", "--vsd_normalized_by_diameter", "--max_sym_disc_step",
                "--skip_missing", "--renderer_type", "--result_filenames", "--results_path", "--eval_path", "--models_inference_path",
                "--datasets_path", "--targets_filename", "--out_errors_tpath"}
    assert ours == expected
    ns = ap.parse_args([])
    p = e.params_from_args(ns)
    assert p["n_top"] == 1 and p["error_type"] == "vsd" and p["vsd_deltas"]["ycbv"] == 15.0 and p["vsd_deltas"]["itodd"] == 5.0
    assert p["vsd_taus"] == list(map(float, map(str, np.arange(0.05, 0.51, 0.05)))) and p["skip_missing"] is True
    assert p["targets_filename"] == "test_targets_bop19.json"
    assert p["out_errors_tpath"].endswith("errors_{scene_id:06d}.json") and "{error_sign}" in p["out_errors_tpath"]
    assert "HIP rasteriser" in ap.format_help()
    assert e.params_from_args(ap.parse_args(["--renderer_type", "anything"]))["renderer_type"] == "anything"
    assert e.params_from_args(ap.parse_args(["--skip_missing", "False"]))["skip_missing"] is True      # bool("False"), as in the reference
    with pytest.raises(SystemExit) as ex:
        e.run(["--error_type", "mssd"])
    assert all(t in str(ex.value.code) for t in e.SUPPORTED_ERROR_TYPES)
    import scripts.eval_calc_errors as alias
    assert alias.run is e.run
    if REF_SCRIPT.exists():                   # the recorded list above IS the reference's: checked where its source is at hand
        ref_flags = set(re.findall(r"add_argument\(\s*\"(--[a-z_]+)\"", REF_SCRIPT.read_text()))
        assert ref_flags == expected


def _toy(gold, tmp_path):
    from freepose_amd.scripts import eval_calc_errors as e
    csv = tmp_path / "m_toy-test.csv"
    csv.write_text(str(gold["toy_csv"]))
    ests = e.load_results_csv(csv)
    targets = json.loads(str(gold["toy_targets"]))
    (tmp_path / "scene_gt.json").write_text(str(gold["toy_scene_gt"]))
    scene_gt = e.load_scene_gt(tmp_path / "scene_gt.json")
    return e, ests, targets, scene_gt


def test_csv_reader_and_pairing_rule_reproduce_the_reference_json(gold, tmp_path):
    e, ests, targets, scene_gt = _toy(gold, tmp_path)
    assert len(ests) == 3 and ests[0]["obj_id"] == "meshA" and ests[1]["score"] == 0.9 and ests[1]["scale"] == 0.2
    assert ests[1]["R"].shape == (3, 3) and ests[1]["R"][0, 1] == -1.0 and ests[1]["t"].shape == (3, 1) and ests[1]["t"][2, 0] == 750.5
    assert ests[2]["bbox_visib"].shape == (4, 1) and ests[2]["time"] == 0.5 and ests[0]["scene_id"] == 3 and ests[0]["im_id"] == 1
    targets_org, ests_org = e.organize(targets, ests)
    assert list(targets_org) == [3] and list(targets_org[3][1]) == [2, 5]
    records = e.pair_image(3, 1, targets_org[3][1], ests_org, scene_gt[1], 1, True)
    # every estimate of the image against every GT of the target's object, sorted by score
    assert [(r["obj_id"], r["est_id"]) for r in records] == [(2, 2), (2, 1), (2, 0), (5, 2), (5, 1), (5, 0)]
    assert [[g for g, _ in r["gts"]] for r in records] == [[1, 2]] * 3 + [[0]] * 3
    rows = {id(x): i for i, x in enumerate(ests)}
    values = []                                     # the stub evaluator: 0.125 * (CSV row + 1) + gt_id, and s_e = scale * 1000
    for r in records:
        for gt_id, gt in r["gts"]:
            assert gt["cam_R_m2c"].shape == (3, 3) and gt["cam_t_m2c"].shape == (3, 1)
            values.append([0.125 * (rows[id(r["est"])] + 1) + gt_id])
    text = e.errors_json(e.scene_errors(records, values))
    want = str(gold["toy_errors_json"])
    assert json.loads(text) == json.loads(want)      # key for key
    assert text == want                              # and byte for byte
    assert set(json.loads(text)[0]) == {"im_id", "obj_id", "est_id", "score", "errors"}
    # not enough estimates: only an error without skip_missing
    assert e.pair_image(3, 7, {2: {"inst_count": 1}}, ests_org, [], 1, True) == []
    with pytest.raises(ValueError, match="Not enough estimates"):
        e.pair_image(3, 7, {2: {"inst_count": 1}}, ests_org, [], 1, False)
    assert e.error_signature("cus", 1) == "error=cus_ntop=1"
    assert e.error_signature("vsd", -1, vsd_delta=15.0, vsd_tau=0.05) == "error=vsd_ntop=-1_delta=15.000_tau=0.050"
    assert e.split_result_name("x/my-method_ycbv-test.csv") == ("my-method_ycbv-test", "my-method", "ycbv", "test", None)
    assert e.split_result_name("m_tless-test-primesense.csv")[2:] == ("tless", "test", "primesense")


def test_scene_runner_hands_the_evaluator_the_reference_pairs(gold, tmp_path):
    """s_e = scale * 1000, the estimate's pose, the target's object id and the GT pose, in record order"""
    e, ests, targets, scene_gt = _toy(gold, tmp_path)
    targets_org, ests_org = e.organize(targets, ests)
    records = e.pair_image(3, 1, targets_org[3][1], ests_org, scene_gt[1], 1, True)
    seen = {}

    class Stub:
        def errors(self, error_type, pairs, K, **kw):
            seen["type"], seen["pairs"], seen["K"] = error_type, pairs, K
            return [float(i) for i in range(len(pairs))]

    p = e.params_from_args(e.build_parser().parse_args(["--error_type", "cus"]))
    runner = e._SceneRunner(p, "toy", Stub(), {}, lambda inf_id: "mesh:" + inf_id)
    Kc = np.arange(9.0).reshape(3, 3)
    vals = runner.values(records, {1: {"cam_K": Kc}}, {})
    assert vals == [[float(i)] for i in range(9)] and seen["type"] == "cus" and seen["K"].shape == (9, 3, 3)
    first = seen["pairs"][0]
    assert first[0] == "mesh:meshB" and first[1] == 0.2 * 1000 and first[4] == 2 and np.array_equal(first[3], ests[1]["t"])
    assert np.array_equal(first[6], scene_gt[1][1]["cam_t_m2c"]) and np.array_equal(seen["pairs"][1][6], scene_gt[1][2]["cam_t_m2c"])


def test_host_error_expressions_match_the_fixture(gold):
    """the float64 error values are formed on the host from the integer counts, in the reference's expression order"""
    from freepose_amd import evaluation as ev
    n = len(gold["cus"])
    assert n >= 24
    for i in range(n):
        inter, union = (int(x) for x in gold["cus_counts"][i])
        assert gold["cus"][i] == (1.0 - inter / float(union) if union > 0 else 1.0)          # guards the fixture itself
        assert ev.cus_from_counts(inter, union) == gold["cus"][i]
        for c in ("vsd0", "vsd1"):
            cnt = gold[c + "_counts"][i]
            assert ev.vsd_from_counts(cnt[0], cnt[1], cnt[2:]) == list(gold[c][i])
        assert ev.re(gold["pair_Re"][i], gold["pair_Rg"][i]) == gold["re"][i]
        assert ev.te(gold["pair_te"][i], gold["pair_tg"][i]) == gold["te"][i]
    # the cases the fixture must hold
    assert gold["cus"][0] == 0.0 and gold["chamfer"][0] == 0.0 and gold["cus"][2] == 1.0 and gold["cus_counts"][2][0] == 0
    assert gold["cus_counts"][3][1] == 0 and gold["cus"][3] == 1.0 and gold["vsd0_counts"][3][1] == 0 and (gold["vsd0"][3] == 1.0).all()
    assert (gold["pair_s"] != 1.0).any() and len(set(gold["pair_inf"].tolist())) == 2
    assert gold["mesh_A_v"].shape[0] != gold["mesh_T_v"].shape[0]
    assert bool(gold["vsd0_norm"]) and not bool(gold["vsd1_norm"])
    ev2 = ev.PoseErrorEvaluator(4, 4)
    assert ev2.errors("re", [(None, 1.0, gold["pair_Re"][6], gold["pair_te"][6], 1, gold["pair_Rg"][6], gold["pair_tg"][6])], None) == [gold["re"][6]]
    with pytest.raises(ValueError, match="supported are cus, chamfer, chamfer_proj, vsd, re, te"):
        ev2.errors("mssd", [], None)
