"""The tracking half of TrackingRefiner on the MI355X: fp_patch_points and fp_pnp_epnp (csrc/refine.hip) against the numpy fp64
restatements of tests/_refiner_ref.py and the reference-made fixture tests/golden/refiner_track.npz, then the class and the
smooth_poses_video CLI end to end on a synthetic clip with a synthetic tracker (tests/_synth_tracker.py)."""
import numpy as np
import pytest
import torch

from tests import _refiner_ref as ref

pytestmark = pytest.mark.gpu

K518 = np.array([[2100.0, 0, 259.0], [0, 2100.0, 259.0], [0, 0, 1]])


def _bits(t):
    return t.cpu().numpy().view(np.int64) if t.dtype == torch.float64 else t.cpu().numpy()


# ---- fp_patch_points --------------------------------------------------------------------------------------------------------------------------
def _cloud(S, seed):
    d = np.random.default_rng(seed).standard_normal((S, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True) * np.array([0.09, 0.05, 0.12])


def _patch_case(S, B):
    """samples, transforms [B,4,4], cells i32 [B,C,2], ncells [B], expected i32 [B,C], per-item member counts"""
    rng = np.random.default_rng([S, B])
    samples = _cloud(S, S)
    poses = [(0.4, (0.004, -0.003, 0.9)), (1.3, (0.0, 0.0, 0.02)), (2.2, (0.01, 0.0, 40.0))][:B]   # ordinary; camera inside; far away
    Ts, lists, counts = [], [], []
    for ang, t in poses:
        T = np.eye(4)
        T[:3, :3] = ref.rodrigues(rng.standard_normal(3), ang)
        T[:3, 3] = t
        occ = {c: m for c, m in ref.cell_lists(samples, T, K518).items() if max(abs(c[0]), abs(c[1])) < 100000}
        cells = np.array(list(occ) + [(-40, 3), (90, 90)], dtype=np.int32)      # two cells nothing projects into
        assert (-40, 3) not in occ and (90, 90) not in occ
        cells = cells[rng.permutation(len(cells))]
        Ts.append(T)
        lists.append(cells)
        counts.append(occ)
    C = max(len(c) for c in lists) + 3                                           # every item has fewer real cells than slots
    cells = np.zeros((B, C, 2), np.int32)
    want = np.full((B, C), -1, np.int32)
    for b, c in enumerate(lists):
        cells[b, :len(c)] = c
        cells[b, len(c):] = c[0]                                                 # slots past ncells hold a cell that has members
        want[b, :len(c)] = ref.chosen_samples(samples, Ts[b], K518, c)[0]
    return samples, np.stack(Ts), cells, np.array([len(c) for c in lists], np.int32), want, counts


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S", [1, 255, 256, 10000])
def test_patch_points_equals_the_elementwise_restatement(S, B):
    from freepose_amd import ops
    samples, Ts, cells, ncells, want, counts = _patch_case(S, B)
    got = ops.patch_points(samples, Ts, K518, cells, ncells)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(ops.patch_points(samples, Ts, K518, cells, ncells), got)              # two calls: the same bits
    assert (want[:, -3:] == -1).all() and (want == -1).sum() >= B * 5                        # padding slots and the two empty cells
    ms = [m for occ in counts for m in occ.values()]
    assert 1 in ms or S > 1                                                                  # a cell with a single member (q = 1)
    if S == 10000:
        assert 1 in ms and any(m % -(-m // 4) for m in ms)                                   # m = 1; an m that ceil(m / 4) does not divide
        if B == 3:
            cam, uv = ref.project(samples, Ts[1], K518)
            assert (cam[:, 2] < 0).any() and np.isfinite(uv[cam[:, 2] < 0]).all()            # samples behind the camera still own cells
            assert max(counts[2].values()) > 1024                                            # the path that scans all keys every pass


def test_patch_points_reproduces_the_reference_fixture(golden_dir):
    from freepose_amd import ops
    g = np.load(golden_dir / "refiner_track.npz")
    samples = g["samples"]
    n = [len(g[f"p3d_cells{i}"]) for i in range(3)]
    cells = np.zeros((3, max(n), 2), np.int32)
    for i in range(3):
        cells[i, :n[i]] = g[f"p3d_cells{i}"]
    Ts = np.stack([g[f"p3d_T{i}"] for i in range(3)])
    idx = ops.patch_points(samples, Ts, g["p3d_K"], cells, np.array(n, np.int32)).cpu().numpy()
    for i in range(3):
        pts = samples[np.maximum(idx[i, :n[i]], 0)]
        pts[idx[i, :n[i]] < 0] = 0.0
        assert np.array_equal(pts, g[f"p3d_points{i}"]), i
        assert (idx[i, :n[i]] < 0).sum() == 2 and (idx[i, n[i]:] == -1).all()


# ---- fp_pnp_epnp ------------------------------------------------------------------------------------------------------------------------------
def test_pnp_epnp_matches_the_restatement_and_isolates_bad_problems(capsys):
    """Statuses equal the restatement's; for status 0 and >= 6 used points the pose differs from the numpy restatement by at most
    100 x the CPU host-check-vs-restatement difference (ref.CPU_HOST_VS_REF, asserted by test_refiner_track_cpu.py) and in any case by
    less than 1e-6 rad / 1e-6 relative; with 4 or 5 used points only a finite proper rotation is required (the null space is not
    one-dimensional).  Valid neighbours of a bad-status problem equal their stand-alone solutions bit for bit; two calls are identical."""
    from freepose_amd import ops
    bound = (min(100 * ref.CPU_HOST_VS_REF[0], 1e-6), min(100 * ref.CPU_HOST_VS_REF[1], 1e-6))
    worst = [0.0, 0.0]
    sizes = set()
    for name, b in ref.batches().items():
        B = b["p2"].shape[0]
        sizes.add(B)
        out = ops.pnp_epnp(b["p3"], b["p2"], b["K"], b["vis"])
        assert np.array_equal(_bits(out), _bits(ops.pnp_epnp(b["p3"], b["p2"], b["K"], b["vis"]))), name
        got = out.cpu().numpy()
        if b["vis"] is not None and (b["vis"] != 0).all(axis=1).any():                      # all ones == NULL
            rows_all = np.nonzero((b["vis"] != 0).all(axis=1))[0]
            null = ops.pnp_epnp(b["p3"], b["p2"][rows_all], b["K"], None)
            assert np.array_equal(_bits(null), _bits(out)[rows_all]), name
        for i, r in enumerate(ref.rows(b)):
            want = ref.epnp(r["p3"], r["p2"], r["K"], r["vis"])["out"]
            assert got[i, 14] == want[14] and got[i, 13] == want[13] and got[i, 15] == 0, (name, i, got[i, 13:], want[13:])
            if want[14] != 0:
                assert np.isnan(got[i, :13]).all(), (name, i)
                continue
            R = got[i, :9].reshape(3, 3)
            assert np.isfinite(got[i, :13]).all() and np.abs(R.T @ R - np.eye(3)).max() < 1e-9 and abs(np.linalg.det(R) - 1) < 1e-9, (name, i)
            if B > 1:                                                                        # alone == among (bad) neighbours
                alone = ops.pnp_epnp(r["p3"], r["p2"][None], r["K"], None if r["vis"] is None else r["vis"][None])
                assert np.array_equal(_bits(alone)[0], _bits(out)[i]), (name, i)
            if want[13] >= 6:
                d = ref.pose_diff(got[i], want)
                worst = [max(worst[0], d[0]), max(worst[1], d[1])]
                assert d[0] <= bound[0] and d[1] <= bound[1], (name, i, d, bound)
                if r["vis"] is None and name.startswith("clean"):
                    planted = np.concatenate([r["R"].ravel(), r["t"]])
                    dp = ref.pose_diff(got[i], planted)
                    assert dp[0] < 1e-9 and dp[1] < 1e-9, (name, i, dp)
    assert sizes == {1, 3, 12}
    # empty batches: an empty result, no call
    some = next(iter(ref.batches().values()))
    assert tuple(ops.pnp_epnp(some["p3"], np.zeros((0, some["N"], 2)), some["K"]).shape) == (0, 16)
    assert tuple(ops.patch_points(some["p3"], np.zeros((0, 4, 4)), K518, np.zeros((0, 3, 2), np.int32)).shape) == (0, 3)
    assert tuple(ops.patch_points(some["p3"], np.eye(4)[None], K518, np.zeros((1, 0, 2), np.int32)).shape) == (1, 0)
    with capsys.disabled():
        print(f"\n[refiner_track] pnp_epnp device vs numpy restatement: max rotation {worst[0]:.3e} rad, max relative translation {worst[1]:.3e}"
              f" (bound {bound[0]:.1e}, {bound[1]:.1e})")


# ---- class and CLI end to end ---------------------------------------------------------------------------------------------------------------
N_FRAMES, FRAME_W, FRAME_H = 48, 320, 240
COARSE_SEED = 11                 # axes of the 40-degree errors; the ViT-B weights are the CLI's seeded random ones (--allow_random_weights)
TRAJ_START = 4.0                 # first angle (rad) of the planted turn: fixed once on the GPU so that the most trusted frame (24) is a middle one
K_CLIP = np.array([[300.0, 0, 160.0], [0, 300.0, 120.0], [0, 0, 1]])


def _planted_trajectory():
    poses = np.tile(np.eye(4), (N_FRAMES, 1, 1))
    for i in range(N_FRAMES):
        poses[i, :3, :3] = ref.rodrigues([0.2, 1.0, 0.3], TRAJ_START + i * np.deg2rad(2.0)) @ ref.rodrigues([1.0, 0.1, -0.2], 0.4)
        poses[i, :3, 3] = [0.06 * np.sin(i / 9.0), 0.03 * np.cos(i / 7.0), 0.85 + 0.002 * i]
    return poses


def _coarse_poses(poses):
    rng = np.random.default_rng(COARSE_SEED)
    coarse = poses.copy()
    exact = list(range(0, N_FRAMES, 6))
    for i in range(N_FRAMES):
        if i not in exact:
            coarse[i, :3, :3] = ref.rodrigues(rng.standard_normal(3), np.deg2rad(40.0)) @ poses[i, :3, :3]
    return coarse, exact


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """data/ tree of a 48-frame clip rendered from bench.synthetic_mesh on a planted trajectory, the coarse CSV (planted translation;
    planted rotation on every 6th frame, 40 degrees off about a seeded axis elsewhere), proposals with the rendered masks, K.txt and
    the synthetic tracker's scene file"""
    import json

    import bench
    import pandas as pd
    from PIL import Image

    from freepose_amd import ops
    from freepose_amd.scripts.dino_inference import CSV_COLUMNS, pose_row
    from freepose_amd.src.pipeline.utils import mask_to_rle_pytorch
    root = tmp_path_factory.mktemp("clip")
    v, f, c = bench.synthetic_mesh(3)
    scale = 0.25
    poses = _planted_trajectory()
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
    coarse, exact = _coarse_poses(poses)
    rows, props = [], []
    for i in range(N_FRAMES):
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
    return dict(root=root, rdir=rdir, scene=scene, poses=poses, coarse=coarse, exact=exact, frames=frames, masks=masks, scale=scale)


def _read_poses(csv):
    import pandas as pd
    df = pd.read_csv(csv)
    R = np.stack([np.array(s.split(" "), dtype=np.float64).reshape(3, 3) for s in df["R"]])
    t = np.stack([np.array(s.split(" "), dtype=np.float64) for s in df["t"]])
    return df, R, t


def test_class_and_cli_end_to_end(clip, monkeypatch, capsys):
    """48 frames, 3 intervals, the start frame in the middle one (forward and backward chains both run).  The tracked CSV keeps the
    input's rows and order, its translations are smooth_3dvec of the coarse ones exactly, its median rotation error against the planted
    trajectory is strictly smaller than the coarse CSV's, and the CLI in a fresh process writes the same bytes."""
    import subprocess
    import sys
    import time
    from pathlib import Path

    from freepose_amd.scripts import smooth_poses_video as spv
    from freepose_amd.src.pipeline.estimators.tracking_refiner import TrackingRefiner
    from freepose_amd.src.pipeline.refiner_utils import smooth_3dvec
    from tests import _synth_tracker
    repo = Path(__file__).resolve().parent.parent
    argv = ["--video", "synth", "--poses", "coarse.csv", "--proposals", "props.json", "--allow_random_weights"]
    monkeypatch.chdir(clip["root"])
    tracker = _synth_tracker.make(str(clip["scene"]))
    picked = {}
    orig = TrackingRefiner.n_inliers_per_pose

    def spy(self, mesh, frames, K, transforms):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n, thr = orig(self, mesh, frames, K, transforms)
        torch.cuda.synchronize()
        picked["n"], picked["seconds"] = n, time.perf_counter() - t0
        return n, thr
    monkeypatch.setattr(TrackingRefiner, "n_inliers_per_pose", spy)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out_csv = clip["root"] / spv.main(spv.build_parser().parse_args(argv), tracker=tracker)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    monkeypatch.undo()
    assert out_csv == clip["rdir"] / "synth-tracked.csv"
    start = int(np.argmax(picked["n"]))
    assert start in clip["exact"], (start, picked["n"].tolist())
    assert 16 <= start < 32, start                                       # the middle interval of round(linspace(0, 48, 4))
    assert tracker.calls == 3
    blob = out_csv.read_bytes()
    df, R, t = _read_poses(out_csv)
    df_in, R_in, t_in = _read_poses(clip["rdir"] / "coarse.csv")
    assert len(df) == N_FRAMES and list(df.columns) == list(df_in.columns) and df["im_id"].tolist() == df_in["im_id"].tolist()
    for col in df_in.columns:
        if col not in ("R", "t"):
            assert df[col].tolist() == df_in[col].tolist(), col
    assert np.array_equal(t, smooth_3dvec(t_in, window_size=5))
    err = np.array([ref.rot_angle(R[i], clip["poses"][i, :3, :3]) for i in range(N_FRAMES)])
    err_in = np.array([ref.rot_angle(R_in[i], clip["poses"][i, :3, :3]) for i in range(N_FRAMES)])
    with capsys.disabled():
        print(f"\n[refiner_track] median rotation error: coarse {np.degrees(np.median(err_in)):.3f} deg -> tracked {np.degrees(np.median(err)):.3f} deg;"
              f" start frame {start}; in-process run {total:.2f} s of which tracker {tracker.seconds:.2f} s and n_inliers_per_pose "
              f"{picked['seconds']:.2f} s")
    assert np.median(err) < np.median(err_in)
    # the same run through the CLI in a fresh process
    out_csv.unlink()
    r = subprocess.run([sys.executable, "-m", "scripts.smooth_poses_video", *argv, "--tracker", "tests._synth_tracker:make", "--tracker_args",
                        '{"scene": "%s"}' % clip["scene"]], cwd=clip["root"], capture_output=True, text=True,
                       env={**__import__("os").environ, "PYTHONPATH": str(repo)})
    assert r.returncode == 0, r.stderr[-3000:]
    assert out_csv.read_bytes() == blob
