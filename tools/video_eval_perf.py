"""Time the video scorer on one results table: 32 videos x 6 methods x 300 frames, half of the videos symmetric (a stated stand-in: the
real clips and their lengths are not part of this repository).

    python -m tools.video_eval_perf [--out FILE.json] [--repeats 20] [--device-only]

Three times, in seconds, for the same table:
  device      `video_errors_table` — host packing, the copy in, fp_video_errors, the copy out — a host clock around calls that end in a
              device synchronise (the results are read back), after two warm-up calls; median and spread of `--repeats` calls.
              `resident`: device events around `ops.video_errors` with the poses already on the device (host packing of the per-track
              tables, their copy and the three kernels; results stay on the device).  Kernel times come from a profiler run of
              `--device-only` (rocprofv3 --kernel-trace --stats), not from this script.
  vectorised  the numpy / scipy restatement of tests/_video_eval_ref.py, on 4 symmetric + 4 plain tracks, scaled to the table (x 24).
  per-pair    the loop as the reference runs it (offset x pair x 101 symmetries, one scipy log / exp per step standing in for
              pinocchio's), on 1 symmetric + 1 plain track, scaled to the table (x 96).
The device outputs are compared with the vectorised ones on the tracks both computed.
"""
from __future__ import annotations

import argparse
import json
import statistics
import time

import numpy as np
from scipy.spatial.transform import Rotation

from tests import _video_eval_ref as ref

VIDEOS, METHODS, FRAMES = 32, 6, 300


def table():
    gts, tracks = [], []
    for v in range(VIDEOS):
        est, gt = ref.trajectory(v, FRAMES)
        axis = ref.SYM_AXIS if v % 2 == 0 else None
        gts.append(dict(poses=gt, w=ref.W, h=ref.H, sym_axis=axis))
        for m in range(METHODS):
            e = est if m == 0 else ref.estimate(gt, np.random.Generator(np.random.PCG64(1000 * v + m)))
            tracks.append(dict(video=v, poses=e, scale=0.17))
    return tracks, gts


def per_pair_loop(est, gt, est_scale, w, h, sym_axis):
    """the reference's loops with scipy single-rotation calls in the place of pinocchio's log / exp"""
    log = lambda R: Rotation.from_matrix(R).as_rotvec()   # noqa: E731
    dts = ref.offsets(len(est))
    rot = []
    for dt in dts:
        errs = []
        for t1 in range(len(est) - dt):
            t2 = t1 + dt
            syms = [np.eye(3)] if sym_axis is None else [Rotation.from_rotvec(sym_axis * a).as_matrix() for a in np.linspace(-np.pi, np.pi, 101)]
            best = np.inf
            for S in syms:                                   # both logs per symmetry, as rot_error_in_cframe takes them
                a = log(est[t2, :3, :3] @ est[t1, :3, :3].T)
                best = min(best, np.linalg.norm(a - log(gt[t2, :3, :3] @ S @ gt[t1, :3, :3].T)))
            errs.append(best)
        rot.append(np.mean(errs) / dt)
    return np.rad2deg(np.mean(rot))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--device-only", action="store_true", help="skip the two host timings (for a profiler run)")
    args = ap.parse_args(argv)
    import torch

    from freepose_amd import ops
    from freepose_amd.src.utils.video_evaluation import video_errors_table
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    tracks, gts = table()
    for _ in range(2):
        got = video_errors_table(tracks, gts)
    times = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        got = video_errors_table(tracks, gts)
        times.append(time.perf_counter() - t0)
    # poses already on the device, device events
    est = torch.as_tensor(np.stack([t["poses"] for t in tracks])).cuda()
    gt = torch.as_tensor(np.stack([g["poses"] for g in gts])).cuda()
    dts = np.tile(ref.offsets(FRAMES), (len(tracks), 1))
    kw = dict(video=[t["video"] for t in tracks], sym_axis=[gts[t["video"]]["sym_axis"] for t in tracks])
    ev = []
    for i in range(args.repeats + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.video_errors(est, gt, dts, 0.17, ref.GT_SCALE, ref.W, ref.H, **kw)
        b.record()
        b.synchronize()
        if i >= 2:
            ev.append(a.elapsed_time(b) / 1e3)

    res = dict(tracks=len(tracks), frames=FRAMES, symmetric_tracks=sum(g["sym_axis"] is not None for g in gts) * METHODS,
               device_call_s_median=statistics.median(times), device_call_s_min=min(times), device_call_s_max=max(times),
               resident_call_s_median=statistics.median(ev), resident_call_s_min=min(ev), resident_call_s_max=max(ev), repeats=args.repeats)
    if args.device_only:
        print(json.dumps(res))
        return
    sub = [v * METHODS for v in range(8)]                 # method 0 of videos 0..7: 4 symmetric, 4 plain
    t0 = time.perf_counter()
    want = [ref.score_track(tracks[i]["poses"], gts[tracks[i]["video"]]["poses"], 0.17, sym_axis=gts[tracks[i]["video"]]["sym_axis"])[1] for i in sub]
    t_vec = (time.perf_counter() - t0) * (len(tracks) / len(sub))
    diff = max(np.abs(got[i] - w).max() for i, w in zip(sub, want))
    t0 = time.perf_counter()
    loop = [per_pair_loop(tracks[i]["poses"], gts[tracks[i]["video"]]["poses"], 0.17, ref.W, ref.H, gts[tracks[i]["video"]]["sym_axis"]) for i in sub[:2]]
    t_loop = (time.perf_counter() - t0) * (len(tracks) / 2)
    diff_loop = max(abs(got[i][0] - x) for i, x in zip(sub[:2], loop))
    res.update(vectorised_host_s_scaled=t_vec, vectorised_tracks_timed=len(sub), per_pair_host_s_scaled=t_loop, per_pair_tracks_timed=2,
               max_abs_diff_device_vs_vectorised=float(diff), max_abs_diff_device_vs_per_pair_rot_deg=float(diff_loop))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
