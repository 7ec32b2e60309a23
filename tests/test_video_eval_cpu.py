"""No-GPU checks of the video scorer: (1) tools/video_eval_host_check.cpp — csrc/video_eval_core.h run serially in the kernels' order,
built with -fsanitize=address,undefined — against the vectorised numpy restatement of tests/_video_eval_ref.py and against
tests/golden/video_eval.npz, which the reference's own loops wrote (tools/gen_golden_video_eval.py); the SO(3) maps; the known answers
and the alignment branches; (2) the `load_pred_csv` mirror and `filter_predictions` against the golden; (3) the boundary: parser flags,
header / ctypes entries, the import path."""
import json
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from tests import _video_eval_ref as ref

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "video_eval.npz")


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("video_host") / "video_eval_host_check"
    cmd = [gxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "freepose_amd" / "csrc"), str(ROOT / "tools" / "video_eval_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def named():
    """name -> track, the names of the golden"""
    out = dict(ref.cases())
    out.update({f"known_{k}": v for k, v in ref.known_answers().items()})
    out.update({f"align_{k}": v[0] for k, v in ref.alignment_cases().items()})
    return out


@pytest.fixture(scope="module")
def scored(host_check, named, tmp_path_factory):
    """name -> (track, host-check output, (per_offset, final) of the restatement); every case alone, then the mixed batch in one file"""
    tmp = tmp_path_factory.mktemp("video_io")
    out = {}
    for name, t in named.items():
        out[name] = (t, ref.run_host_check(host_check, tmp, [dict(t, video=0)], [t["gt"]])[0], ref.score(t))
    tracks, gts = ref.mixed_batch()
    for i, (t, h) in enumerate(zip(tracks, ref.run_host_check(host_check, tmp, tracks, gts))):
        out[f"mixed_{i}"] = (t, h, ref.score(t))
    return out


def close(got, want):
    return bool((np.abs(np.asarray(got) - np.asarray(want)) <= ref.tol(np.asarray(want))).all())


# ---- (1) the arithmetic ---------------------------------------------------------------------------------------------------------------------
def test_case_set_covers_the_stated_shapes():
    c = ref.cases()
    for N in ref.LENGTHS:
        assert len(c[f"N{N}"]["est"]) == N and c[f"N{N}"]["sym_axis"] is None and np.array_equal(c[f"N{N}_sym"]["sym_axis"], ref.SYM_AXIS)
    assert abs(np.linalg.norm(ref.SYM_AXIS) - 1) > 1e-3                                          # not a unit vector
    assert ref.offsets(2).tolist() == [1] * 10 and ref.offsets(3).tolist() == [1] * 10           # one and two pairs
    assert ref.offsets(21).tolist() == list(range(1, 11)) and ref.offsets(130)[-1] == 65         # pairs cross the 64-lane boundary
    assert {c[f"N21_sym{n}"]["n_sym"] for n in (1, 64, 65)} == {1, 64, 65} and c["N21_sym"]["n_sym"] == 101
    tracks, gts = ref.mixed_batch()
    assert len(tracks) == 7 and len(gts) == 5 and sorted(len(g) for g in gts) == list(ref.LENGTHS)
    videos = [t["video"] for t in tracks]
    assert any(videos.count(v) == 2 for v in videos) and all(len(t["est"]) == len(gts[t["video"]]) for t in tracks)


def test_cases_meet_the_conditions_the_reference_relies_on():
    """every log(R2e R1e^T) and every minimising log(R2g S R1g^T) stays 0.01 rad from pi, and the best symmetry beats the second best
    among the first 100 grid points (the 101st repeats the first) by 1e-7.  n_sym = 1 cannot: its only grid point is -pi, |axis| pi =
    pi - 0.005 on top of the motion; there the logs must stay 1e-4 from pi, where theta / sin(theta) <= 3.2e4 still leaves
    3.2e4 x 1.1e-16 x 100 operations = 3.5e-10 under the tolerance."""
    tracks = dict(ref.cases())
    tracks.update({f"mixed_{i}": t for i, t in enumerate(ref.mixed_batch()[0])})
    for name, t in tracks.items():
        worst, gap = ref.conditions(t)
        print(name, "worst angle", worst, "smallest gap", gap)
        if t["sym_axis"] is not None and t["n_sym"] == 1:
            assert worst <= np.pi - 1e-4, name
        else:
            assert worst <= np.pi - 0.01 and gap >= 1e-7, (name, worst, gap)


def test_restatement_reproduces_the_reference(golden, named):
    """the vectorised restatement against what the reference's own loops returned (same seeds: the checksums)"""
    tracks = dict(named)
    tracks.update({f"mixed_{i}": t for i, t in enumerate(ref.mixed_batch()[0])})
    for name, t in tracks.items():
        assert np.array_equal(golden[f"{name}_checksum"], [t["est"].sum(), t["gt"].sum()]), name
        per, fin = ref.score(t)
        assert close(per, golden[f"{name}_per_offset"]) and close(fin, golden[f"{name}_final"]), name
        moved = ref.align_object_origins(t["est"], t["gt"], t["est_scale"])[0]
        assert close(moved[:, :3, 3], golden[f"{name}_aligned"]), name


def test_host_check_agrees_with_the_restatement_and_the_golden(scored, golden):
    worst = 0.0
    for name, (t, h, (per, fin)) in scored.items():
        assert h["per_offset"].shape == per.shape == (10, 3)
        worst = max(worst, np.abs(h["per_offset"] - per).max(), np.abs(h["final"] - fin).max())
        assert close(h["per_offset"], per) and close(h["final"], fin), name
        assert close(h["per_offset"], golden[f"{name}_per_offset"]) and close(h["final"], golden[f"{name}_final"]), name
        assert close(h["aligned"], golden[f"{name}_aligned"]), name
    print("host check vs restatement, worst absolute difference:", worst)


def test_so3_maps_round_trip(host_check, tmp_path):
    """max |exp(log R) - R| <= 1e-9 and |log R| in [0, pi], at angles down to 0 and up to exactly pi.  1e-9 at pi - 1e-9 is what needs the
    near-pi branch: theta / sin(theta) x v loses 7 of 16 digits there."""
    axes = [np.array([0.0, 0.0, 1.0]), np.array([0.6, 0.0, -0.8]), ref.SYM_AXIS / np.linalg.norm(ref.SYM_AXIS)]
    angles = [0.0, 1e-10, 1e-5, 1.0, np.pi - 1e-3, np.pi - 1e-6, np.pi - 1e-9, np.pi]
    R = np.array([Rotation.from_rotvec(a * ang).as_matrix() for ang in angles for a in axes])
    w, E = ref.run_host_so3(host_check, tmp_path, R)
    norm = np.linalg.norm(w, axis=1)
    assert np.isfinite(w).all() and (norm >= 0).all() and (norm <= np.pi).all()
    err = np.abs(E - R).reshape(len(angles), -1).max(axis=1)
    print("round trip per angle:", dict(zip(angles, err)))
    assert (err <= 1e-9).all()
    assert np.abs(norm.reshape(len(angles), 3) - np.array(angles)[:, None]).max() <= 1e-9
    # the axis itself, wherever it is defined, including its sign just below pi
    for i, ang in enumerate(angles[1:-1], start=1):
        for j, a in enumerate(axes):
            assert np.abs(w[i * 3 + j] - a * ang).max() <= 1e-5 * max(ang, 1e-10) + 1e-9, (ang, j)
    # exactly pi with v == 0: the largest component is positive
    Rpi = np.array([2 * np.outer(a, a) - np.eye(3) for a in axes])
    wpi, Epi = ref.run_host_so3(host_check, tmp_path, Rpi)
    for a, x in zip(axes, wpi):
        k = np.argmax(np.abs(a))
        assert x[k] > 0 and np.abs(x - np.sign(a[k]) * a * np.pi).max() <= 1e-9
    assert np.abs(Epi - Rpi).max() <= 1e-9


def test_known_answers(scored):
    t, h, _ = scored["known_same"]
    assert np.abs(h["per_offset"]).max() <= 1e-12 and np.abs(h["final"]).max() <= 1e-12
    assert np.abs(scored["known_same_sym"][1]["per_offset"]).max() <= 1e-12
    assert np.abs(scored["known_const"][1]["per_offset"][:, 0]).max() <= 1e-12              # est = gt C: the same spatial velocity
    assert np.abs(scored["known_spin_sym"][1]["per_offset"][:, 0]).max() <= 1e-12           # spins about the axis by grid steps
    dts = ref.offsets(len(t["est"]))
    mean_pair_error = scored["known_spin_nosym"][1]["per_offset"][:, 0] * dts
    print("spin without the axis, mean pair error per offset (rad):", mean_pair_error)
    assert (mean_pair_error > 0.1).all()


def test_alignment_branches(scored):
    for name, (t, branch) in ref.alignment_cases().items():
        h = scored[f"align_{name}"][1]
        moved, kept, origin = ref.align_object_origins(t["est"], t["gt"], t["est_scale"])
        assert h["kept"] == kept and close(h["aligned"], moved[:, :3, 3]), name
        norm = np.linalg.norm(h["origin"])
        if branch == "rejected":
            assert kept == 0 and np.array_equal(h["aligned"], t["est"][:, :3, 3])          # unchanged, bit for bit
        elif branch == "clamped":
            assert kept == len(t["est"]) and abs(norm - t["est_scale"] / 2) <= 1e-15
        else:
            assert kept == len(t["est"]) and 1e-3 < norm < t["est_scale"] / 2 - 1e-3


# ---- (2) load_pred_csv and filter_predictions against the reference's -----------------------------------------------------------------------
def test_load_pred_csv_mirrors_the_reference(golden, golden_dir, capsys):
    from freepose_amd.scripts import eval_videos as ev
    tree = golden_dir / "video_eval"
    gt, gt_scale, axis, mesh_id, _, boxes = ev.load_gt(tree, "vid", 1)
    assert np.array_equal(gt, golden["csv_gt_poses"]) and gt_scale == golden["csv_gt_scale"] == 0.15 and np.array_equal(axis, golden["csv_gt_axis"])
    res = tree / "results" / "videos" / "vid"
    for name in ("three_objects", "low_iou", "non_finite"):
        capsys.readouterr()
        T, scale, obj_id, bbox0, pts = ev.load_pred_csv(res / f"{name}.csv", bbox=boxes)
        warnings = capsys.readouterr().err.count("WARNING")
        assert np.array_equal(T[:, :3, :3], golden[f"csv_{name}_R"]) and np.array_equal(T[:, :3, 3], golden[f"csv_{name}_t"]), name
        assert scale == golden[f"csv_{name}_scale"] and bbox0 == str(golden[f"csv_{name}_bbox0"]) and pts is None and obj_id == "mesh0"
        assert warnings == int(golden[f"csv_{name}_warnings"]), name
        assert np.isfinite(T).all()
    assert int(golden["csv_three_objects_warnings"]) == 0 and int(golden["csv_low_iou_warnings"]) == 1
    assert int(golden["csv_non_finite_warnings"]) == 3                                       # t at frames 0 and 5, R at frame 3
    # the best object of three is the second of every frame
    import pandas as pd
    df = pd.read_csv(res / "three_objects.csv")
    assert (df["im_id"] == 0).sum() == 3 and golden["csv_three_objects_bbox0"] == df["bbox_visib"].values[1]
    with pytest.raises(AssertionError, match=re.escape(str(golden["csv_two_scales_error"]))):
        ev.load_pred_csv(res / "two_scales.csv", bbox=boxes)
    with pytest.raises(FileNotFoundError):
        ev.load_pred_csv(res / "missing.csv", bbox=boxes)


def test_filter_predictions_writes_the_reference_json(golden_dir, tmp_path):
    from freepose_amd.scripts import filter_predictions as fp
    src = golden_dir / "video_eval"
    shutil.copytree(src, tmp_path / "data")
    (tmp_path / "data" / "results" / "videos" / "vid" / "props_best_object.json").unlink()
    out = fp.run(["--video", "vid", "--proposals", "props.json", "--data_path", str(tmp_path / "data")])
    assert out.name == "props_best_object.json"
    assert out.read_text() == (src / "results" / "videos" / "vid" / "props_best_object.json").read_text()
    props = json.loads((src / "results" / "videos" / "vid" / "props.json").read_text())
    assert json.loads(out.read_text()) == props[1::3]                                         # three objects, the best one not first


# ---- (3) boundary ---------------------------------------------------------------------------------------------------------------------------
def test_parsers_equal_the_reference():
    import scripts.eval_videos as ev_alias
    import scripts.filter_predictions as fp_alias
    from freepose_amd.scripts import eval_videos as ev, filter_predictions as fp
    assert ev_alias.main is ev.main and fp_alias.main is fp.main
    p = ev.build_parser()
    opts = {tuple(a.option_strings): a for a in p._actions}
    for flags in (("--videos", "-v"), ("--labels", "-l"), ("--patterns", "-p")):
        assert opts[flags].nargs == "*" and opts[flags].default is None and opts[flags].type is str
    assert opts[("--ann_id", "-i")].default == 1 and opts[("--ann_id", "-i")].type is int and opts[("--data_path",)].default == "data"
    args = ev.resolve_defaults(p.parse_args([]))
    assert len(args.videos) == 32 and args.videos[0] == "bowl1" and args.videos[-1] == "spoons" and args.videos[29] == "pour_into_8625"
    assert args.labels == ["MegaPose coarse", "MegaPose fine", "GigaPose", "FoundPose", "Ours coarse", "Ours fine"]
    assert len(args.patterns) == 6 and args.patterns[5] == "{video}-tracked.csv" and args.patterns[2] == "gigapose_{video}_rescaled.csv"
    assert all("{video}" in x for x in args.patterns)
    assert args.patterns[4] == "props-ground-box-0.2-text-0.2-ffa-22-top-25_{video}_gpt4_scaled_best_object_dinopose_layer_22_bbext_0.05_depth_zoedepth.csv"
    q = fp.build_parser()
    fo = {a.option_strings[0]: a for a in q._actions if a.option_strings}
    assert fo["--video"].required and fo["--proposals"].required and fo["--ann_id"].default == 1 and fo["--data_path"].default == "data"


def test_entry_point_is_declared_and_refuses_bad_arguments_without_a_gpu():
    import ctypes as C

    from freepose_amd import _lib
    header = (ROOT / "include" / "freepose_hip.h").read_text()
    proto = re.search(r"\bint fp_video_errors\(([^;]*)\);", header).group(1)
    assert len(proto.split(",")) == 14 == len(_lib.SIGNATURES["fp_video_errors"][1])
    assert "video_evaluation.py" in header and "eval_videos.py" in header                      # the reference lines it replaces
    lib = _lib.load()
    assert lib.fp_video_errors(None, None, None, None, None, 1, 1, 2, 1, None, None, None, None, None) == 1
    assert b"video_errors" in lib.fp_last_error()
    # ill-shaped: the sizes are looked at before any pointer is used (a made-up non-null context is never dereferenced)
    meta, params, buf = np.zeros((1, 20), np.int32), np.zeros((1, 16)), np.zeros(64)
    p = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    meta[0, :5] = [0, 2, 101, 0, 1]
    params[0, :4] = [0.1, 0.15, 640, 480]
    for M, V, Nmax, D, what in ((1, 1, 1, 1, b"Nmax=1"), (1, 1, 2, 17, b"D=17"), (1, 0, 2, 1, b"V=0"), (70000, 1, 2, 1, b"M=70000")):
        assert lib.fp_video_errors(p(buf), p(buf), p(buf), p(meta), p(params), M, V, Nmax, D, p(buf), p(buf), None, None, None) == 1
        assert what in lib.fp_last_error(), what
    for col, value, what in ((4, 2, b"dt[0]=2"), (4, 0, b"dt[0]=0"), (2, 0, b"n_sym=0"), (2, 1025, b"n_sym=1025"), (1, 1, b"N=1"), (0, 1, b"video 1")):
        bad = meta.copy()
        bad[0, col] = value
        assert lib.fp_video_errors(p(buf), p(buf), p(buf), p(bad), p(params), 1, 1, 2, 1, p(buf), p(buf), None, None, None) == 1
        assert what in lib.fp_last_error(), (what, lib.fp_last_error())


def test_reference_import_path_resolves():
    import src.utils.video_evaluation as alias
    from freepose_amd.src.utils import video_evaluation as ve
    assert alias is ve
    for name in ("get_average_rot_errors_dt", "get_average_depth_errors_dt", "get_average_proj_errors_dt", "get_rot_errors",
                 "get_translation_errors_depth", "get_translation_errors_proj", "project", "align_object_origins", "change_object_origin",
                 "video_errors_table"):
        assert callable(getattr(ve, name)), name
    assert np.abs(ve.project(np.array([0.1, -0.2, 0.8]), 640, 480) - ref.project(np.array([0.1, -0.2, 0.8]), 640, 480)).max() <= 1e-12
    moved = ve.change_object_origin(np.tile(np.eye(4), (2, 1, 1)), [1.0, 2.0, 3.0])
    assert np.array_equal(moved[:, :3, 3], [[1, 2, 3], [1, 2, 3]])
    poses = [ve.Pose(np.eye(3), np.zeros(3))]
    assert np.array_equal(ve.change_object_origin(poses, [1.0, 0, 0])[0].translation, [1, 0, 0])
