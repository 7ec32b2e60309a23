"""No-GPU checks of the tracking half of TrackingRefiner: (1) the numpy restatements of tests/_refiner_ref.py and the host mirrors
against tests/golden/refiner_track.npz, which the reference's own functions wrote (tools/gen_golden_refiner_track.py); (2)
tools/pnp_host_check.cpp — csrc/pnp_core.h run serially in the kernel's phase order, built with -fsanitize=address,undefined — against
the numpy EPnP restatement and the planted poses; (3) the new boundary: header / ctypes entries, CLI flags, the errors, TriMesh.sample."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _refiner_ref as ref

ROOT = Path(__file__).resolve().parent.parent
CAP = 1e-6        # rad / relative: what the GPU test allows the device at most


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(golden_dir / "refiner_track.npz")


# ---- (1) restatements and mirrors against the reference-made fixture ----------------------------------------------------------------------
@pytest.mark.parametrize("order", ["elementwise", "matmul"])
def test_compute_3d_points_restatements_reproduce_the_reference(fixture, order):
    g = fixture
    for i in range(3):
        pts = ref.compute_3d_points(g["samples"], g[f"p3d_cells{i}"], g["p3d_K"], g[f"p3d_T{i}"], order=order)
        assert np.array_equal(pts, g[f"p3d_points{i}"]), i            # the same sample for every cell
        idx, counts = ref.chosen_samples(g["samples"], g[f"p3d_T{i}"], g["p3d_K"], g[f"p3d_cells{i}"], order=order)
        assert (idx < 0).sum() == 2 and counts.max() > 8 and (counts == 1).any()


def test_mirror_query_frames_and_cell_mapping_equal_the_reference(fixture):
    from freepose_amd.src.pipeline.estimators.tracking_refiner import TrackingRefiner
    g = fixture
    tr = TrackingRefiner.__new__(TrackingRefiner)._host_state()     # no device: everything but the ViT
    tr.tracker = None
    for i in range(3):
        assert np.array_equal(tr.get_query_frames(g[f"gqf_in{i}"]), g[f"gqf_out{i}"])
    render = g["map_render37"] > 0.5
    for name, mask in (("masked", g["map_mask_half"] > 0.5), ("unmasked", None), ("fallback", g["map_mask_tiny"] > 0.5)):
        cells = tr._valid_cells(render, mask)
        query = tr._cells_to_pixels(cells, g["map_bbox"])
        assert query.dtype == g[f"map_{name}_query"].dtype and np.array_equal(query, g[f"map_{name}_query"]), name
        pts = ref.compute_3d_points(g["samples"], cells, g["map_new_K"].astype(np.float64), g["p3d_T0"])
        assert np.array_equal(pts, g[f"map_{name}_points"]), name
    assert len(g["map_fallback_query"]) == len(g["map_unmasked_query"]) > len(g["map_masked_query"]) >= 4


def test_mirror_smoothing_matches_the_reference(fixture):
    from scipy.spatial.transform import Rotation

    from freepose_amd.src.pipeline import refiner_utils as ru
    g = fixture
    assert np.abs(ru.smooth_transforms(g["smooth_in"]) - g["smooth_out"]).max() <= 1e-12
    q = Rotation.from_matrix(g["smooth_in"][:, :3, :3]).as_quat()
    assert ((q[1:] * q[:-1]).sum(1) < 0).any()                          # the trajectory does contain a quaternion sign flip
    assert np.abs(ru.moving_average(g["mavg_in"], 5, lambda a: np.mean(a, axis=0)) - g["mavg_out5"]).max() <= 1e-12
    assert np.abs(ru.smooth_3dvec(g["mavg_in"], 9) - g["mavg_out9"]).max() <= 1e-12
    as_R = lambda quat: Rotation.from_quat(quat).as_matrix()           # noqa: E731  (the eigenvector's sign is free)
    assert np.abs(as_R(ru.average_quaternions(g["avgq_in"])) - as_R(g["avgq_out"])).max() <= 1e-12
    assert np.abs(as_R(ru.smooth_quaternions(g["avgq_in"], 5)) - as_R(g["smoothq_out"])).max() <= 1e-12


# ---- (2) pnp_host_check ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("pnp_host") / "pnp_host_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           str(ROOT / "freepose_amd" / "csrc"), str(ROOT / "tools" / "pnp_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def solved(host_check, tmp_path_factory):
    """every row of every batch: (name, row, host-check output [16], restatement dict)"""
    tmp = tmp_path_factory.mktemp("pnp_io")
    out = []
    for name, b in ref.batches().items():
        rows = ref.rows(b)
        for i, (r, h) in enumerate(zip(rows, ref.run_host_check(host_check, tmp, rows))):       # exit status 0 under the sanitizers
            out.append((f"{name}[{i}]", r, h, ref.epnp(r["p3"], r["p2"], r["K"], r["vis"])))
    return out


def test_problem_set_covers_the_stated_cases():
    p = ref.problems()
    for N in (4, 5, 6, 63, 64, 65, 257, 1369):
        assert p[f"clean_{N}"]["N"] == N and p[f"noisy_{N}"]["N"] == N
        assert np.abs(p[f"noisy_{N}"]["p2"] - ref._project_noisy(p[f"noisy_{N}"]["p3"], p[f"noisy_{N}"]["R"], p[f"noisy_{N}"]["t"], 0, None)).std() \
            == pytest.approx(ref.SIGMA, rel=0.5)
    b = ref.batches()
    assert {v["p2"].shape[0] for v in b.values()} == {1, 3, 12}
    v3, v12 = b["mixed_3"]["vis"], b["mixed_12"]["vis"]
    assert v3[0].all() and not v3[1].any() and 0.3 < v3[2].mean() < 0.7
    assert sorted(v12.sum(1).tolist())[:5] == [0, 2, 3, 4, 10] and v12[0].all() and 0.3 < v12[1].mean() < 0.7


def test_host_check_recovers_planted_poses_noise_free(solved):
    """noise-free, N >= 6, points not coplanar: the host check and the restatement both return the planted pose"""
    worst = {"host": [0.0, 0.0], "restatement": [0.0, 0.0]}
    n = 0
    for name, r, h, e in solved:
        if not name.startswith("clean_") or r["N"] < 6:
            continue
        planted = np.concatenate([r["R"].ravel(), r["t"]])
        for who, got in (("host", h), ("restatement", e["out"])):
            assert got[14] == 0
            d = ref.pose_diff(got, planted)
            worst[who] = [max(worst[who][0], d[0]), max(worst[who][1], d[1])]
            assert d[0] < 1e-10 and d[1] < 1e-10, (name, who, d)
            assert got[12] < 1e-9, (name, who, got[12])                  # reprojection error in pixels
        n += 1
    assert n == 6
    print("noise-free vs planted (rad, relative):", worst)


def test_host_check_agrees_with_the_restatement(solved):
    """status and used count everywhere; for status 0 and >= 6 used points the two poses agree within ref.CPU_HOST_VS_REF (recorded in
    profiles/refiner_track.md; the GPU test allows the device 100 x that), far below the cap; and a near-tie among the candidates cannot
    move the pose: their errors differ by more than 1 % or the three candidates are one pose to ref.CANDIDATE_SPREAD_MAX."""
    worst = [0.0, 0.0]
    n = 0
    for name, r, h, e in solved:
        want = e["out"]
        assert h[14] == want[14] and h[13] == want[13] and h[15] == 0, (name, h[13:], want[13:])
        if want[14] != 0 or want[13] < 6:
            continue
        errs = np.sort(e["errs"])
        margin = min((errs[1] - errs[0]) / errs[0], (errs[2] - errs[1]) / errs[1]) if errs[0] > 0 else 0.0
        spread = max(max(ref.pose_diff(a, b)) for a in e["cands"] for b in e["cands"])
        assert margin > 0.01 or spread <= ref.CANDIDATE_SPREAD_MAX, (name, margin, spread)
        d = ref.pose_diff(h, want)
        worst = [max(worst[0], d[0]), max(worst[1], d[1])]
        assert d[0] <= ref.CPU_HOST_VS_REF[0] and d[1] <= ref.CPU_HOST_VS_REF[1], (name, d)
        assert abs(h[12] - want[12]) <= 1e-9 * max(1.0, want[12]), name
        n += 1
    assert n >= 20 and 100 * max(ref.CPU_HOST_VS_REF) < CAP
    print("host check vs restatement (rad, relative):", worst)


def test_host_check_small_and_degenerate_problems(solved):
    seen = set()
    for name, r, h, e in solved:
        used = int(h[13])
        if h[14] == 0 and used in (4, 5):                                  # the null space is not one-dimensional: a finite proper rotation
            for got in (h, e["out"]):
                R = got[:9].reshape(3, 3)
                assert np.isfinite(got[:13]).all() and np.abs(R.T @ R - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1) < 1e-9, name
            seen.add(used)
        if h[14] != 0:
            assert np.isnan(h[:13]).all() and np.isnan(e["out"][:13]).all(), name
            seen.add(("status", int(h[14]), used))
    assert {4, 5, ("status", 1, 3), ("status", 1, 0), ("status", 2, 64), ("status", 2, 10)} <= seen


# ---- (3) boundary ---------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_and_refuse_bad_arguments_without_a_gpu():
    from freepose_amd import _lib
    header = (ROOT / "include" / "freepose_hip.h").read_text()
    assert "f-3b: TrackingRefiner correspondences and pose from tracks" in header
    for name, n_args in (("fp_patch_points", 12), ("fp_pnp_epnp", 9)):
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        assert len(proto.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    lib = _lib.load()
    assert lib.fp_patch_points(None, None, 1, None, None, None, None, 1, 1, 14.0, None, None) == 1 and b"patch_points" in lib.fp_last_error()
    assert lib.fp_pnp_epnp(None, None, None, None, None, 1, 6, None, None) == 1 and b"pnp_epnp" in lib.fp_last_error()


def test_smooth_poses_video_flags_and_errors(tmp_path, monkeypatch):
    import scripts.smooth_poses_video as alias
    from freepose_amd.scripts import smooth_poses_video as spv
    from freepose_amd.src.pipeline.estimators.tracking_refiner import TrackingRefiner
    assert alias.main is spv.main and alias.build_parser is spv.build_parser
    flags = {s for a in spv.build_parser()._actions for s in a.option_strings}
    assert {"--video", "--obj-idxs", "--poses", "--proposals", "--vis"} <= flags                    # the reference's
    assert {"--tracker", "--tracker_args", "--model", "--allow_random_weights"} <= flags
    args = spv.build_parser().parse_args(["--video", "v", "--obj-idxs", "0", "2", "--vis"])
    assert args.obj_idxs == [0, 2] and args.vis and args.poses is None and args.model == "dinov2_vitb14_reg"
    tr = TrackingRefiner.__new__(TrackingRefiner)._host_state()     # no device: everything but the ViT
    tr.tracker = None
    with pytest.raises(RuntimeError, match="CoTracker is not shipped.*tracker="):
        tr._track_frames(np.zeros((2, 4, 4, 3), np.uint8), np.zeros((1, 3), np.float32))
    with pytest.raises(NotImplementedError):
        tr.refine
    tr.tracker = lambda frames, queries: (np.zeros((len(frames), len(queries), 2), np.float32), np.ones((len(frames), len(queries)), bool))
    tracks, vis = tr._track_frames(np.zeros((2, 4, 4, 3), np.uint8), np.zeros((5, 3), np.float32))
    assert tracks.shape == (2, 5, 2) and vis.dtype == bool and vis.shape == (2, 5)
    # a 20-frame clip has no interval
    with pytest.raises(ValueError, match="20 frames has no tracking interval"):
        spv.interval_boundaries(20)
    assert spv.interval_boundaries(24).tolist() == [0, 24] and spv.interval_boundaries(48).tolist() == [0, 16, 32, 48]
    from PIL import Image
    fdir = tmp_path / "data" / "datasets" / "videos" / "short"
    fdir.mkdir(parents=True)
    for i in range(20):
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(fdir / f"{i:06d}.png")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="20 frames has no tracking interval"):
        spv.main(spv.build_parser().parse_args(["--video", "short", "--poses", "p.csv", "--proposals", "p.json"]))
    # the fewer-than-15-visible rule, seeded
    vis = np.zeros((3, 40), bool)
    vis[0, :20] = True
    vis[1, :6] = True
    a = spv.visibility_for_pnp(vis, np.random.default_rng(5))
    assert np.array_equal(a, spv.visibility_for_pnp(vis, np.random.default_rng(5)))
    assert np.array_equal(a[0], vis[0]) and a[1].sum() == 15 and a[1, :6].all() and a[2].sum() == 15 and not vis[1, 6:].any()
    with pytest.raises(ValueError, match="module:factory"):
        spv.load_tracker("nomodule")
    assert spv.load_tracker("builtins:dict", '{"a": 1}') == {"a": 1}


def test_trimesh_sample():
    from freepose_amd.mesh_io import TriMesh
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 0], [5, 5, 5], [5, 6, 5], [5, 5, 5.5]], dtype=np.float32)
    F = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 4, 2], [5, 6, 7]])                 # areas 0.5, 0.5, 0.5, 1.0, 0.25
    mesh = TriMesh(V, F)
    n = 20000
    pts = mesh.sample(n, seed=3)
    assert pts.shape == (n, 3) and pts.dtype == np.float64
    assert np.array_equal(pts, mesh.sample(n, seed=3)) and not np.array_equal(pts, mesh.sample(n, seed=4))
    assert np.array_equal(mesh.sample(50, seed=np.random.default_rng(9)), mesh.sample(50, seed=np.random.default_rng(9)))
    # every point lies on some triangle: in its plane, barycentrics in [0, 1]
    on = np.zeros(n, bool)
    share = []
    for tri in F:
        a, e1, e2 = V[tri[0]].astype(np.float64), (V[tri[1]] - V[tri[0]]).astype(np.float64), (V[tri[2]] - V[tri[0]]).astype(np.float64)
        uv, *_ = np.linalg.lstsq(np.stack([e1, e2], 1), (pts - a).T, rcond=None)
        res = np.abs(np.stack([e1, e2], 1) @ uv - (pts - a).T).max(0)
        inside = (res < 1e-12) & (uv >= -1e-12).all(0) & (uv.sum(0) <= 1 + 1e-12)
        share.append(inside & ~on)
        on |= inside
    assert on.all()
    area = np.array([0.5, 0.5, 0.5, 1.0, 0.25])
    p = area / area.sum()
    counts = np.array([s.sum() for s in share])      # points on shared edges (measure zero) go to the first triangle
    assert (np.abs(counts - n * p) <= 4 * np.sqrt(n * p * (1 - p))).all(), (counts, n * p)
    with pytest.raises(ValueError):
        TriMesh(V, F[:0]).sample(3)
