"""Times the built-in point tracker (freepose_amd.tracker, csrc/lk_track.hip) on one MI355X, sweeps its two quality thresholds on the
synthetic mesh clip and writes profiles/klt_tracker.md.

    python -m tools.klt_tracker_perf [--out profiles/klt_tracker.md] [--repeats 7]

What is measured:
  timings       12 frames of 720 x 1280 (a seeded analytic texture under a sub-pixel translation), 1369 queries on a 37 x 37 grid with
                t_q = 6, the tracker's default parameters.  Host clock around work that ends in a device synchronise, after one warm-up
                call, median of the repeats: the copy in (pageable host memory -> device; the same buffer every repeat, so the run-time's
                staging path is warm and the figure is not that of a first copy of fresh frames), ops.lk_pyramid, ops.lk_track (init + 11 chain
                steps), the copy back of tracks, visibility and diagnostics, and the whole LKTracker call.
  restatement   tests/_lk_ref.track (numpy, float64) on 12 frames of 180 x 320 with 150 queries, the stated smaller size, once.
  sweep         the 24-frame mesh clip of tests/_track_clip.py, queries from compute_2d3d_correspondences on planted frame 12 of the
                interval [0, 24): visibility recomputed from one run's diagnostics for a grid of (min_eig, max_residual) — positions do
                not depend on the thresholds — against the planted truth of tests/_synth_tracker.py: precision = rows both call visible /
                rows the tracker calls visible, recall = the same / rows the truth calls visible, and the median error on the
                tracker's visible rows.
  end to end    scripts.smooth_poses_video on that clip with the planted-truth tracker and with klt at its defaults: median rotation
                error against the planted trajectory; the same with a few other values of min_eig.
None of these numbers is a gate.
"""
import argparse
import datetime
import os
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

from tests import _lk_ref as ref

T_BIG, H_BIG, W_BIG, GRID = 12, 720, 1280, 37
MIN_EIGS = (0.0, 0.02, 0.05, 0.1, 0.25, 0.5, 1.0, 2.0, 5.0, 10.0)
E2E_MIN_EIGS = (0.02, 0.05, 0.1, 0.25, 1.0)     # smooth_poses_video is also run with these, beside the default
MAX_RESIDUALS = (3.0, 5.0, 8.0, 12.0, 16.0, 24.0, 255.0)


def sync_time(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(min(ts)) * 1e3, float(max(ts)) * 1e3


def timings(repeats):
    from freepose_amd import ops, tracker
    frames = ref.render(ref.Texture(21), ref.Translation(1.3, -0.7), T_BIG, H_BIG, W_BIG)
    gx, gy = np.meshgrid(np.linspace(60, W_BIG - 61, GRID), np.linspace(60, H_BIG - 61, GRID))
    q = np.stack([np.full(GRID * GRID, 6.0), gx.ravel(), gy.ravel()], 1).astype(np.float32)
    tr = tracker.LKTracker()
    p = dict(levels=tr.levels, radius=tr.radius, iters=tr.iters, fb_thresh=tr.fb_thresh, min_eig=tr.min_eig, max_residual=tr.max_residual)
    host = torch.from_numpy(frames)
    dev = host.cuda()
    qd = torch.from_numpy(q).cuda()
    pyr = ops.lk_pyramid(dev, p["levels"], p["radius"])
    out = ops.lk_track(pyr, T_BIG, H_BIG, W_BIG, qd, **p)
    rows = [("copy in (%.1f MB, the same pageable buffer each repeat: warm staging path)" % (frames.nbytes / 1e6), sync_time(lambda: host.cuda(), repeats)),
            ("ops.lk_pyramid (grey + 3 levels, 12 frames)", sync_time(lambda: ops.lk_pyramid(dev, p["levels"], p["radius"]), repeats)),
            ("ops.lk_track (init + 11 chain steps, 2738 items each)", sync_time(lambda: ops.lk_track(pyr, T_BIG, H_BIG, W_BIG, qd, **p), repeats)),
            ("copy back (tracks, visibility, diagnostics)", sync_time(lambda: [o.cpu() for o in out], repeats)),
            ("LKTracker call, numpy in, numpy out", sync_time(lambda: tr(frames, q), repeats))]
    tracks, vis = tr(frames, q)
    err = np.sqrt(((tracks - ref.truth_tracks(ref.Translation(1.3, -0.7), q, T_BIG)) ** 2).sum(-1))
    small = ref.render(ref.Texture(21), ref.Translation(1.3, -0.7), 12, 180, 320)
    qs = ref.grid_queries(np.random.default_rng(5), 30, 30, 289, 149, 15, 10, (6,))
    t0 = time.perf_counter()
    ref.track(small, qs, **p)
    return rows, (float(np.median(err[vis])), float(vis.mean())), time.perf_counter() - t0, p


def sweep_and_end_to_end():
    from freepose_amd import ops, tracker
    from freepose_amd.mesh_io import load_obj
    from freepose_amd.scripts import smooth_poses_video as spv
    from freepose_amd.src.pipeline.estimators.tracking_refiner import TrackingRefiner
    from tests import _refiner_ref, _synth_tracker, _track_clip
    with tempfile.TemporaryDirectory() as d:
        clip = _track_clip.build_clip(Path(d), 24)
        mesh = load_obj(clip["root"] / "data" / "mesh_cache" / "synthobj" / "synthobj.obj")
        mesh.apply_scale(clip["scale"])
        tracref = TrackingRefiner(dino_model="dinov2_vitb14_reg", state_dict=None, tracker=None)
        pixels, _ = tracref.compute_2d3d_correspondences(mesh, clip["frames"][12], _track_clip.K_CLIP, clip["poses"][12], mask=clip["masks"][12])
        q = np.concatenate([np.full((len(pixels), 1), 12.0), np.asarray(pixels)], 1).astype(np.float32)
        frames = clip["frames"]
        T, H, W = frames.shape[:3]
        synth = _synth_tracker.make(str(clip["scene"]))
        truth, truth_vis = synth(frames, q)
        tr = tracker.LKTracker()
        pyr = ops.lk_pyramid(frames, tr.levels, tr.radius)
        tracks, _, diag = (o.cpu().numpy() for o in ops.lk_track(pyr, T, H, W, q, tr.levels, tr.radius, tr.iters, tr.fb_thresh, 0.0, 1e9))
        err = np.sqrt(((tracks - truth) ** 2).sum(-1))
        inside = (diag[..., 3].astype(int) & ops.LK_FLAG_OUTSIDE) == 0
        nq = np.ones((T, len(q)), bool)
        nq[12] = False
        table = []
        for me in MIN_EIGS:
            for mr in MAX_RESIDUALS:
                good = (diag[..., 0] <= tr.fb_thresh) & (diag[..., 1] >= me) & (diag[..., 2] <= mr) & inside
                good[12] = True
                vis = np.zeros_like(good)
                vis[12] = True
                for t in range(13, T):
                    vis[t] = vis[t - 1] & good[t]
                for t in range(11, -1, -1):
                    vis[t] = vis[t + 1] & good[t]
                v, tv = vis & nq, truth_vis & nq
                both = (v & tv).sum()
                table.append((me, mr, both / max(v.sum(), 1), both / max(tv.sum(), 1), float(np.median(err[v])) if v.any() else float("nan")))
        cwd = os.getcwd()
        os.chdir(clip["root"])
        try:
            argv = ["--video", "synth", "--poses", "coarse.csv", "--proposals", "props.json", "--allow_random_weights"]
            n = len(clip["poses"])

            def med(csv):
                _, R, _ = _track_clip.read_poses(csv)
                return float(np.median(np.degrees([_refiner_ref.rot_angle(R[i], clip["poses"][i, :3, :3]) for i in range(n)])))
            coarse = med(clip["rdir"] / "coarse.csv")
            e_truth = med(clip["root"] / spv.main(spv.build_parser().parse_args(argv), tracker=synth))
            e_klt = med(clip["root"] / spv.main(spv.build_parser().parse_args(argv), tracker=tracker.klt()))
            e_more = [(me, med(clip["root"] / spv.main(spv.build_parser().parse_args(argv), tracker=tracker.klt(min_eig=me)))) for me in E2E_MIN_EIGS]
        finally:
            os.chdir(cwd)
    return table, len(q), (coarse, e_truth, e_klt, e_more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/klt_tracker.md")
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("klt_tracker_perf: no GPU; these numbers are only taken on the device")
    from freepose_amd import tracker
    rows, (big_err, big_vis), ref_s, p = timings(args.repeats)
    table, n_q, (coarse, e_truth, e_klt, e_more) = sweep_and_end_to_end()
    L = [f"# Built-in point tracker (pyramidal Lucas-Kanade): timings, threshold sweep, end to end", "",
         f"Written by `python -m tools.klt_tracker_perf` on {datetime.date.today().isoformat()}, one MI355X.  "
         "None of these numbers is a gate.  The tracker is a classical stand-in for the learned tracker of the reference (DESIGN.md §18): "
         "no parity claim.", "",
         f"## Timings: {T_BIG} frames of {H_BIG} x {W_BIG}, {GRID * GRID} queries, t_q = 6, defaults {p}", "",
         f"Host clock around work that ends in a device synchronise, one warm-up call, {args.repeats} repeats.", "",
         "| step | median ms | min | max |", "|---|---|---|---|"]
    L += [f"| {name} | {m:.3f} | {lo:.3f} | {hi:.3f} |" for name, (m, lo, hi) in rows]
    L += ["", f"On this clip (analytic truth) the median error over visible rows is {big_err:.4f} px and {big_vis:.3f} of all rows are visible.",
          f"The numpy restatement (tests/_lk_ref.track, float64) takes {ref_s:.2f} s on the host for 12 frames of 180 x 320 with 150 queries "
          "(a sixteenth of the pixels, a ninth of the queries).", "",
          f"## Threshold sweep on the mesh clip (24 frames of 320 x 240, {n_q} queries on frame 12, fb_thresh = 1 px)", "",
          "Visibility against the planted truth over the non-query rows: precision / recall / median error (px) of the rows called visible.", "",
          "| min_eig \\ max_residual | " + " | ".join(f"{mr:g}" for mr in MAX_RESIDUALS) + " |", "|---|" + "---|" * len(MAX_RESIDUALS)]
    for me in MIN_EIGS:
        cells = [f"{pr:.3f} / {rc:.3f} / {e:.2f}" for m, mr, pr, rc, e in table if m == me]
        L.append(f"| {me:g} | " + " | ".join(cells) + " |")
    L += ["", f"Defaults chosen from this table: min_eig = {tracker.DEFAULT_MIN_EIG:g}, max_residual = {tracker.DEFAULT_MAX_RESIDUAL:g}.", "",
          "## scripts.smooth_poses_video on the mesh clip", "",
          "Median rotation error against the planted trajectory (degrees): "
          f"coarse input {coarse:.3f}, planted-truth tracker {e_truth:.3f}, klt at its defaults {e_klt:.3f}.",
          "With other values of min_eig (everything else at its default): " + ", ".join(f"{me:g}: {e:.3f}" for me, e in e_more) + ".", ""]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(L))
    print("\n".join(L))


if __name__ == "__main__":
    main()
