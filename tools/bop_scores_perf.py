"""Time the BOP scorer on a stand-in table of ycbv-test size (a stated stand-in: the dataset is not part of this repository): 12 scenes x
75 images, 3-6 target objects per image with one instance each, 5 estimates per image — every estimate is compared against every target
of its image, as scripts.eval_calc_errors pairs them, so every group is 5 estimates x 1 ground truth — and 30 thresholds.

    python -m tools.bop_scores_perf [--out profiles/bop_scores.md] [--repeats 20]

Times, in seconds, on the same host and for the same table:
  scorer       one `BopScorer.scores` call: host packing, upload, fp_bop_scores, download and the 30 (scores dict, match list) pairs — a
               host clock around calls that end with the results on the host, after two warm-up calls; median, min and max.
  its parts    `pack` alone, `ops.bop_scores` + download alone (tables already packed), `unpack` alone.
  restatement  tests/_bop_score_ref.score_dataset once per threshold: the dict loops of the reference, one threshold at a time, in
               this process (the reference's driver additionally starts a process and reloads every file per threshold).
The scorer's answer is compared with the restatement's for every threshold before anything is written.
"""
from __future__ import annotations

import argparse
import datetime
import statistics
import time

import numpy as np

from tests import _bop_score_ref as ref

SCENES, IMAGES, ESTS, OBJECTS = 12, 75, 5, 21
THRESHOLDS = [float(t) for t in np.arange(0.05, 0.51, 0.05)] * 3          # 30 values; equal thresholds are matched independently


def table():
    rng = np.random.Generator(np.random.PCG64(2019))
    targets, scene_gt, info, errs = [], {}, {}, {}
    for s in range(48, 48 + SCENES):
        scene_gt[s], info[s], errs[s] = {}, {}, []
        for im in range(1, IMAGES + 1):
            objs = sorted(rng.choice(np.arange(1, OBJECTS + 1), size=int(rng.integers(3, 7)), replace=False).tolist())
            scene_gt[s][im] = [{"obj_id": o} for o in objs]
            info[s][im] = [{"visib_fract": float(v)} for v in rng.uniform(0.2, 1.0, len(objs))]
            scores = rng.random(ESTS).tolist()
            for g, o in enumerate(objs):
                targets.append({"scene_id": s, "im_id": im, "obj_id": o, "inst_count": 1})
                for k in range(ESTS):
                    errs[s].append({"im_id": im, "obj_id": o, "est_id": k, "score": scores[k], "errors": {g: [float(rng.uniform(0, 0.7))]}})
    return {"targets": targets, "scene_gt": scene_gt, "scene_gt_info": info, "errs": errs, "obj_ids": list(range(1, OBJECTS + 1)),
            "scene_ids": list(range(48, 48 + SCENES)), "n_top": -1, "visib_gt_min": -1, "error_type": "cus", "thresholds": THRESHOLDS,
            "diameters": None, "im_width": 640}


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = fn()
        out.append(time.perf_counter() - t0)
    return r, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/bop_scores.md")
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args(argv)
    import torch

    from freepose_amd import ops
    from freepose_amd.evaluation import BopScorer
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    c = table()
    sc = BopScorer(c["targets"], c["scene_gt"], c["scene_gt_info"], c["obj_ids"], c["scene_ids"], c["visib_gt_min"])
    call = lambda: sc.scores(c["errs"], "cus", THRESHOLDS, c["n_top"])   # noqa: E731
    call(), call()
    got, t_call = timed(call, args.repeats)
    tab, t_pack = timed(lambda: sc.pack(c["errs"], c["n_top"]), args.repeats)

    def device():
        res = ops.bop_scores(tab["err"], tab["groups"], tab["gt_valid"], tab["gt_obj"], tab["gt_scene"], THRESHOLDS, len(c["obj_ids"]),
                             len(c["scene_ids"]), c["n_top"])
        return [r.cpu().numpy() for r in res]
    host, t_dev = timed(device, args.repeats)
    _, t_unpack = timed(lambda: sc.unpack(tab, THRESHOLDS, *host), args.repeats)
    t0 = time.perf_counter()
    want = [ref.score_dataset(c, th) for th in THRESHOLDS]
    t_ref = time.perf_counter() - t0
    for (s, m), (ws, wm) in zip(got, want):
        assert s == ws and m == wm, "the scorer and the restatement disagree"
    med = statistics.median
    recalls = [s["recall"] for s, _ in got[:10]]
    lines = [
        "# BOP scores: one device call against the per-threshold dict loops",
        "",
        f"Measured {datetime.date.today().isoformat()} on one MI355X with `python -m tools.bop_scores_perf` ({args.repeats} repeats after two warm-up calls).",
        "",
        f"Stand-in table of ycbv-test size: {SCENES} scenes x {IMAGES} images, 3-6 target objects per image, {ESTS} estimates per image, i.e. "
        f"{len(tab['groups'])} groups of {ESTS} x 1, {len(tab['gt_valid'])} ground truths, {len(tab['err'])} errors, {len(THRESHOLDS)} thresholds.",
        "",
        "| what | seconds |",
        "|---|---|",
        f"| `BopScorer.scores`, all {len(THRESHOLDS)} thresholds (median; min - max) | {med(t_call):.4f} ({min(t_call):.4f} - {max(t_call):.4f}) |",
        f"| - `pack` (host: group, sort, normalise) | {med(t_pack):.4f} |",
        f"| - `ops.bop_scores` + download (check, upload, kernel, copy back) | {med(t_dev):.4f} |",
        f"| - `unpack` (host: {len(THRESHOLDS)} match lists and score dicts) | {med(t_unpack):.4f} |",
        f"| restatement, one threshold at a time, {len(THRESHOLDS)} thresholds, same host (one run) | {t_ref:.4f} |",
        "",
        f"Both give the same {len(THRESHOLDS)} score dicts and match lists (compared with == before this file was written); recalls of the "
        f"first ten thresholds: {', '.join(f'{r:.4f}' for r in recalls)}.",
        "",
        "The restatement runs in one process with everything in memory.  The reference's driver starts one Python process per (error type, "
        "threshold) and each reloads the targets, every scene's ground truth and every errors file; that start-up and file time is not in "
        "the figure above and was not measured here.",
        "",
    ]
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
