"""The built-in point tracker on the MI355X (csrc/lk_track.hip through ops.lk_pyramid / ops.lk_track and freepose_amd.tracker) against
the numpy restatement tests/_lk_ref.py and the planted truth of the synthetic clips, the dispatch edges, determinism, refusals, and
scripts.smooth_poses_video end to end on the mesh clip with `--tracker freepose_amd.tracker:klt`."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _lk_ref as ref

pytestmark = pytest.mark.gpu

TRACK_TOL = 10 * ref.CPU_HOST_VS_REF[0]          # px; the kernel and the host check run the same fp64 expressions in the same order
RECORD_ROUNDING = 5e-5                           # REF_VS_TRUTH is recorded to four decimals
DIAG_TOL = 10 * ref.CPU_HOST_VS_REF[1]
DEVICE_BAND = (TRACK_TOL, DIAG_TOL)
REPO = Path(__file__).resolve().parent.parent


def _run(frames, queries, p):
    """-> (pyramid levels as numpy, tracks f32, vis u8, diag f32)"""
    from freepose_amd import ops
    T, H, W = frames.shape[:3]
    pyr = ops.lk_pyramid(frames, p["levels"], p["radius"])
    tracks, vis, diag = ops.lk_track(pyr, T, H, W, queries, **p)
    levels = [lv.cpu().numpy() for lv in ops.lk_levels(pyr, T, H, W, p["levels"], p["radius"])]
    return levels, tracks.cpu().numpy(), vis.cpu().numpy(), diag.cpu().numpy()


_GOT = {}


def _device(name):
    if name not in _GOT:
        c = ref.case(name)
        _GOT[name] = _run(c["frames"], c["queries"], c["params"])
    return _GOT[name]


def _check_against_restatement(name, c, r, got, capsys):
    levels, tracks, vis, diag = got
    assert len(levels) == len(r["pyr"])
    for a, b in zip(levels, r["pyr"]):
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), name
    assert tracks.dtype == np.float32 and vis.dtype == np.uint8 and np.isfinite(tracks).all() and np.isfinite(diag).all()
    assert set(np.unique(vis)) <= {0, 1}
    m = ref.compare(r, tracks, vis, diag, c["queries"], c["params"], DEVICE_BAND)
    with capsys.disabled():
        print(f"\n[lk] case {name}: device vs restatement track {m['track']:.3e} px (bound {TRACK_TOL:.1e}), diagnostics {m['diag']:.3e}, "
              f"compared {m['n_compared']} rows ({m['compared_share']:.3f} of visible), in band {m['band_share']:.4f}")
    assert m["compared_share"] >= 0.9 and m["band_share"] <= 0.02
    assert m["track"] <= TRACK_TOL and m["diag"] <= DIAG_TOL and m["flags_equal"] and m["vis_equal_settled"]
    return m


# ---- 1. every case against the restatement and the truth -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "B1", "C5", "C1", "C0", "C_T1", "D", "E", "F", "G"])
def test_cases_against_restatement_and_truth(name, capsys):
    assert TRACK_TOL <= 0.05
    c, r = ref.case(name), ref.reference(name)
    got = _device(name)
    _check_against_restatement(name, c, r, got, capsys)
    if name in ref.REF_VS_TRUTH:
        med, p95, share = ref.truth_error(got[1], got[2], c["truth"], c["queries"])
        want = ref.REF_VS_TRUTH[name]
        with capsys.disabled():
            print(f"[lk] case {name}: device vs truth median {med:.4f} px, p95 {p95:.4f} px, visible share {share:.4f} (restatement {want})")
        assert med <= want[0] + TRACK_TOL + RECORD_ROUNDING and p95 <= want[1] + TRACK_TOL + RECORD_ROUNDING
        assert abs(share - want[2]) <= RECORD_ROUNDING
    if name.startswith("C"):
        assert len(got[0]) == 2                                     # two of the four requested levels are dropped at 61 x 47, radius 7
    if name == "C_T1":
        assert np.array_equal(got[1][0], c["queries"][:, 1:]) and got[2].all()


def test_named_expectations_of_occluder_flat_region_and_leaving():
    ref.assert_named_expectations(lambda name: (_device(name)[1], _device(name)[2]), tol=TRACK_TOL)


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    from tests import _track_clip
    return _track_clip.build_clip(tmp_path_factory.mktemp("lkclip"), 24)


H_PARAMS = dict(ref.PARAMS)
H_ANCHOR = 12


def test_mesh_clip(clip, capsys):
    """case H: the 24 frames of the rendered mesh clip, every query of compute_2d3d_correspondences on planted frame 12 (both chains
    run), truth from tests/_synth_tracker.py.  Prints REF_VS_TRUTH["H"] as measured here.  The device's errors against the truth lie
    within the restatement's plus the device tolerance: the visible sets are equal (asserted) and every row moves by at most that."""
    from freepose_amd.mesh_io import load_obj
    from freepose_amd.src.pipeline.estimators.tracking_refiner import TrackingRefiner
    from tests import _synth_tracker, _track_clip
    mesh = load_obj(clip["root"] / "data" / "mesh_cache" / "synthobj" / "synthobj.obj")
    mesh.apply_scale(clip["scale"])
    tracref = TrackingRefiner(dino_model="dinov2_vitb14_reg", state_dict=None, tracker=None)
    pixels, _ = tracref.compute_2d3d_correspondences(mesh, clip["frames"][H_ANCHOR], _track_clip.K_CLIP, clip["poses"][H_ANCHOR],
                                                     mask=clip["masks"][H_ANCHOR])
    pixels = np.asarray(pixels, dtype=np.float32)
    assert len(pixels) >= 30
    q = np.concatenate([np.full((len(pixels), 1), H_ANCHOR, np.float32), pixels], 1)
    frames = clip["frames"]
    assert len(frames) == 24
    truth, truth_vis = _synth_tracker.make(str(clip["scene"]))(frames, q)
    r = ref.track(frames, q, **H_PARAMS)
    got = _run(frames, q, H_PARAMS)
    _check_against_restatement("H", dict(queries=q, params=H_PARAMS), r, got, capsys)
    want = ref.truth_error(r["tracks"], r["vis"], truth, q, truth_vis)
    have = ref.truth_error(got[1], got[2], truth, q, truth_vis)
    with capsys.disabled():
        print(f'[lk] case H ({len(q)} queries): restatement vs truth "H": (%.4f, %.4f, %.4f); device (%.4f, %.4f, %.4f)' % (want + have))
    rec = ref.REF_VS_TRUTH["H"]
    assert abs(want[0] - rec[0]) <= 1e-3 + 0.02 * rec[0] and abs(want[1] - rec[1]) <= 1e-3 + 0.02 * rec[1] and abs(want[2] - rec[2]) <= 0.01
    assert have[0] <= rec[0] + TRACK_TOL + RECORD_ROUNDING and have[1] <= rec[1] + TRACK_TOL + RECORD_ROUNDING
    assert abs(have[2] - rec[2]) <= RECORD_ROUNDING


# ---- 2. dispatch edges ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_clip():
    H, W, T = 72, 88, 3
    return ref.render(ref.Texture(7), ref.Translation(0.9, -0.6), T, H, W), T, H, W


@pytest.mark.parametrize("N", [1, 3, 4, 5, 257])
def test_workgroup_tail(edge_clip, N, capsys):
    """4 items (2 queries) per workgroup: odd and even item counts, one and many workgroups; t_q on the first, a middle and the last frame
    in one call"""
    frames, T, H, W = edge_clip
    rng = np.random.default_rng(N)
    q = np.stack([np.arange(N) % 3, rng.uniform(16, W - 17, N), rng.uniform(16, H - 17, N)], 1).astype(np.float32)
    r = ref.track(frames, q, **ref.PARAMS)
    _check_against_restatement(f"N={N}", dict(queries=q, params=ref.PARAMS), r, _run(frames, q, ref.PARAMS), capsys)


@pytest.mark.parametrize("radius", [1, 7, 15])
def test_window_radii(edge_clip, radius, capsys):
    """radius 1 (9 pixels on 64 lanes), 7 (225: four slots with a masked tail), 15 (961: the sixteen-slot kernel)"""
    frames, T, H, W = edge_clip
    p = dict(ref.PARAMS, radius=radius, levels=2)
    rng = np.random.default_rng(radius)
    q = np.stack([np.arange(12) % 3, rng.uniform(20, W - 21, 12), rng.uniform(20, H - 21, 12)], 1).astype(np.float32)
    r = ref.track(frames, q, **p)
    assert len(r["pyr"]) == 2
    _check_against_restatement(f"radius={radius}", dict(queries=q, params=p), r, _run(frames, q, p), capsys)


def test_corner_point_empty_calls_and_single_frame(edge_clip, capsys):
    from freepose_amd import ops
    frames, T, H, W = edge_clip
    q = np.array([[0, 0, 0], [1, W - 1, H - 1], [2, W - 1, 0], [0, 30.5, 30.25]], np.float32)      # exactly on three corners
    r = ref.track(frames, q, **ref.PARAMS)
    levels, tracks, vis, diag = _run(frames, q, ref.PARAMS)
    assert np.isfinite(tracks).all() and np.isfinite(diag).all()
    assert np.array_equal(tracks[q[:, 0].astype(int), np.arange(4)], q[:, 1:]) and vis[q[:, 0].astype(int), np.arange(4)].all()
    ok = np.abs(tracks[:, 3] - r["tracks"][:, 3]).max()
    assert ok <= TRACK_TOL and np.array_equal(vis[:, 3].astype(bool), r["vis"][:, 3])
    # N = 0: empty results, nothing launched; T = 1: the query rows only
    pyr = ops.lk_pyramid(frames, 4, 7)
    t0, v0, d0 = ops.lk_track(pyr, T, H, W, np.zeros((0, 3), np.float32), **ref.PARAMS)
    assert tuple(t0.shape) == (T, 0, 2) and tuple(v0.shape) == (T, 0) and tuple(d0.shape) == (T, 0, 4)
    _, t1, v1, d1 = _run(frames[:1], q[[0, 3]], ref.PARAMS)
    assert np.array_equal(t1[0], q[[0, 3], 1:]) and v1.all() and not d1.any()
    outside = np.array([[0, -3.0, 5.0], [0, 5.0, H + 2.0]], np.float32)                              # a query outside: invisible at home
    _, t2, v2, d2 = _run(frames, outside, ref.PARAMS)
    assert not v2.any() and np.isfinite(t2).all() and (d2[0, :, 3] == ops.LK_FLAG_OUTSIDE).all()


# ---- 3. determinism and inputs ------------------------------------------------------------------------------------------------------------------
def test_same_bits_for_every_input_form_and_call():
    from freepose_amd.tracker import LKTracker
    c = ref.case("A")
    tr = LKTracker(**c["params"])
    t0, v0 = tr(c["frames"], c["queries"])
    d0 = tr.last["diag"]
    assert t0.dtype == np.float32 and v0.dtype == bool and t0.shape == (c["T"], len(c["queries"]), 2) and v0.shape == t0.shape[:2]
    levels, tracks, vis, diag = _device("A")
    assert np.array_equal(t0.view(np.int32), tracks.view(np.int32)) and np.array_equal(v0, vis.astype(bool))
    wide = np.zeros((c["T"], c["H"], c["W"] + 5, 4), np.uint8)
    wide[:, :, 2:2 + c["W"], :3] = c["frames"]
    view = wide[:, :, 2:2 + c["W"], :3]
    assert not view.flags["C_CONTIGUOUS"]
    for frames, queries in ((c["frames"], c["queries"]), (view, c["queries"].astype(np.float64)),
                            (torch.from_numpy(c["frames"]).cuda(), torch.from_numpy(c["queries"])),
                            (torch.from_numpy(c["frames"]), c["queries"].tolist())):
        t, v = tr(frames, queries)
        assert np.array_equal(t.view(np.int32), t0.view(np.int32)) and np.array_equal(v, v0)
        assert np.array_equal(tr.last["diag"].view(np.int32), d0.view(np.int32))
    assert tr.last["sizes"] == ref.layout(c["H"], c["W"], 4, 7)


def test_bad_arguments_are_refused_before_any_launch():
    from freepose_amd import ops
    c = ref.case("C5")
    T, H, W = c["frames"].shape[:3]
    pyr = ops.lk_pyramid(c["frames"], 4, 7)
    for kw, msg in ((dict(radius=0), "radius=0"), (dict(radius=16), "radius=16"), (dict(levels=0), "levels=0"), (dict(levels=9), "levels=9"),
                    (dict(iters=0), "iters=0"), (dict(iters=65), "iters=65")):
        with pytest.raises(RuntimeError, match=msg):
            ops.lk_track(pyr, T, H, W, c["queries"], **dict(ref.PARAMS, **kw))
    for kw, msg in ((dict(levels=0), "levels=0"), (dict(radius=16), "radius=16")):
        with pytest.raises(RuntimeError, match=msg):
            ops.lk_pyramid(c["frames"], **dict(dict(levels=4, radius=7), **kw))
    with pytest.raises(RuntimeError, match="T=0"):
        ops.lk_track(pyr, 0, H, W, c["queries"], **ref.PARAMS)
    with pytest.raises(ValueError, match="floats"):
        ops.lk_track(pyr[:100], T, H, W, c["queries"], **ref.PARAMS)
    with pytest.raises(ValueError, match="uint8"):
        ops.lk_pyramid(c["frames"].astype(np.float32))
    torch.cuda.synchronize()                                                # nothing was launched that could fail later
    _, tracks, vis, _ = _run(c["frames"], c["queries"], c["params"])
    assert np.array_equal(tracks, _device("C5")[1])


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------------
def test_smooth_poses_video_with_the_built_in_tracker(clip, monkeypatch, capsys):
    """24 frames, one interval.  With `--tracker freepose_amd.tracker:klt` the tracked CSV keeps the input's rows and order and its median
    rotation error against the planted trajectory is below the coarse input's; a fresh process writes the same bytes.  The error with the
    planted-truth tracker is measured beside it and printed; there is no gate on their ratio."""
    from freepose_amd import tracker as trk
    from freepose_amd.scripts import smooth_poses_video as spv
    from tests import _refiner_ref, _synth_tracker, _track_clip
    argv = ["--video", "synth", "--poses", "coarse.csv", "--proposals", "props.json", "--allow_random_weights"]
    monkeypatch.chdir(clip["root"])
    n = len(clip["poses"])

    def errors(csv):
        _, R, _ = _track_clip.read_poses(csv)
        return np.degrees([_refiner_ref.rot_angle(R[i], clip["poses"][i, :3, :3]) for i in range(n)])
    df_in, _, _ = _track_clip.read_poses(clip["rdir"] / "coarse.csv")
    err_in = errors(clip["rdir"] / "coarse.csv")
    out_csv = clip["root"] / spv.main(spv.build_parser().parse_args(argv), tracker=_synth_tracker.make(str(clip["scene"])))
    err_truth = errors(out_csv)
    out_csv.unlink()
    klt = trk.klt(**H_PARAMS)
    out_csv = clip["root"] / spv.main(spv.build_parser().parse_args(argv), tracker=klt)
    assert out_csv == clip["rdir"] / "synth-tracked.csv" and klt.last is not None
    blob = out_csv.read_bytes()
    df, _, _ = _track_clip.read_poses(out_csv)
    err = errors(out_csv)
    assert len(df) == n and list(df.columns) == list(df_in.columns) and df["im_id"].tolist() == df_in["im_id"].tolist()
    for col in df_in.columns:
        if col not in ("R", "t"):
            assert df[col].tolist() == df_in[col].tolist(), col
    with capsys.disabled():
        print(f"\n[lk] smooth_poses_video on the mesh clip, median rotation error: coarse {np.median(err_in):.3f} deg, klt {np.median(err):.3f} deg, "
              f"planted-truth tracker {np.median(err_truth):.3f} deg")
    assert np.median(err) < np.median(err_in)
    out_csv.unlink()
    r = subprocess.run([sys.executable, "-m", "scripts.smooth_poses_video", *argv, "--tracker", "freepose_amd.tracker:klt", "--tracker_args",
                        json.dumps(H_PARAMS)], cwd=clip["root"], capture_output=True, text=True, timeout=300,
                       env={**__import__("os").environ, "PYTHONPATH": str(REPO)})
    assert r.returncode == 0, r.stderr[-3000:]
    assert out_csv.read_bytes() == blob
