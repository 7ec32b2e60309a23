"""Restatement of the BOP toolkit's matching and scoring, written from its semantics with dict loops, one threshold at a time
(pose_matching.py match_poses / match_poses_scene, score.py calc_localization_scores, eval_calc_scores.py:188-290, inout.save_json,
misc.get_score_signature), and the case builder of the BOP-score tests.  No device, no package import.

Two levels:
  * a DATASET case is what the scorer reads: targets, scene_gt, scene_gt_info, the errors files' content, the object and scene lists and
    the settings.  `score_dataset(case, th)` gives the reference's (scores dict, match records) for one threshold.
  * a TABLE is what fp_bop_scores reads (err, groups, gt_valid, gt_obj, gt_scene, th).  `score_table(table)` gives match [T,R] and the
    four count arrays, again by dict loops per group and threshold.
"""
import copy
import json
import subprocess

import numpy as np

TH10 = [float(t) for t in np.arange(0.05, 0.51, 0.05)]       # the table of eval_bop19_pose.py for cus / chamfer
TH10_PX = [float(t) for t in np.arange(5, 51, 5)]            # ... for chamfer_proj
NAN, INF = float("nan"), float("inf")


# ---- the reference's text ------------------------------------------------------------------------------------------------------------
def score_signature(correct_th, visib_gt_min):
    return "th=" + "-".join(["{:.3f}".format(t) for t in correct_th]) + "_min-visib={:.3f}".format(visib_gt_min)


def save_json_text(content):
    lines = []
    if isinstance(content, dict):
        items = sorted(content.items(), key=lambda x: x[0])
        for i, (k, v) in enumerate(items):
            lines.append('  "{}": {}'.format(k, json.dumps(v, sort_keys=True)) + ("," if i != len(items) - 1 else ""))
        return "{\n" + "".join(ln + "\n" for ln in lines) + "}"
    for i, e in enumerate(content):
        lines.append("  {}".format(json.dumps(e, sort_keys=True)) + ("," if i != len(content) - 1 else ""))
    return "[\n" + "".join(ln + "\n" for ln in lines) + "]"


# ---- matching of one group -----------------------------------------------------------------------------------------------------------
def match_group(errs, th, n_top, valid_mask):
    """errs: [{'est_id', 'score', 'errors': {gt_id: [e]}}] -> [{'est_id', 'gt_id', 'score', 'error', 'error_norm'}]"""
    order = sorted(errs, key=lambda e: e["score"], reverse=True)
    if n_top > 0:
        order = order[:n_top]
    taken, out = [], []
    for e in order:
        best_gt, best = -1, [th]
        for gt_id, error in e["errors"].items():
            if valid_mask[gt_id] and gt_id not in taken and error[0] < best[0]:
                best_gt, best = gt_id, error
        if best_gt >= 0:
            taken.append(best_gt)
            out.append({"est_id": e["est_id"], "gt_id": best_gt, "score": e["score"], "error": best, "error_norm": [best[0] / float(th)]})
    return out


def gt_valid(im_gt, im_gt_info, im_targets, visib_gt_min):
    if visib_gt_min >= 0:
        return [gt["obj_id"] in im_targets and im_gt_info[i]["visib_fract"] >= visib_gt_min for i, gt in enumerate(im_gt)]
    valid = [None] * len(im_gt)
    left = {o: t["inst_count"] for o, t in im_targets.items()}
    for i in sorted(range(len(im_gt)), key=lambda i: im_gt_info[i]["visib_fract"], reverse=True):
        o = im_gt[i]["obj_id"]
        if o in left and left[o] > 0:
            valid[i] = True
            left[o] -= 1
        else:
            valid[i] = False
    return valid


def organize_targets(targets):
    org = {}
    for t in targets:
        org.setdefault(t["scene_id"], {}).setdefault(t["im_id"], {})[t["obj_id"]] = t
    return org


def normalised_errs(case, scene_id):
    errs = copy.deepcopy(case["errs"].get(scene_id, []))
    for e in errs:
        if case["error_type"] in ("ad", "add", "adi", "mssd", "chamfer"):
            d = float(case["diameters"][e["obj_id"]])
            e["errors"] = {g: [x / d for x in v] for g, v in e["errors"].items()}
        if case["error_type"] in ("mspd", "chamfer_proj"):
            f = 640.0 / float(case["im_width"])
            e["errors"] = {g: [f * x for x in v] for g, v in e["errors"].items()}
    return errs


def match_dataset(case, th):
    matches = []
    for scene_id, scene_targets in organize_targets(case["targets"]).items():
        by = {}
        for e in normalised_errs(case, scene_id):
            by.setdefault(e["im_id"], {}).setdefault(e["obj_id"], []).append(e)
        for im_id, im_targets in scene_targets.items():
            im_gt = case["scene_gt"][scene_id][im_id]
            valid = gt_valid(im_gt, case["scene_gt_info"][scene_id][im_id], im_targets, case["visib_gt_min"])
            im_matches = [{"scene_id": scene_id, "im_id": im_id, "obj_id": gt["obj_id"], "gt_id": g, "est_id": -1, "score": -1, "error": -1,
                           "error_norm": -1, "valid": valid[g]} for g, gt in enumerate(im_gt)]
            for obj_id in set(gt["obj_id"] for gt in im_gt):
                for m in match_group(by.get(im_id, {}).get(obj_id, []), th, case["n_top"], valid):
                    im_matches[m["gt_id"]].update(est_id=m["est_id"], score=m["score"], error=m["error"], error_norm=m["error_norm"])
            matches += im_matches
    return matches


def recall(tp, tars):
    return 0.0 if tars == 0 else tp / float(tars)


def localization_scores(scene_ids, obj_ids, matches, n_top):
    insts = {}
    for m in matches:
        if m["valid"]:
            k = (m["obj_id"], m["scene_id"], m["im_id"])
            insts[k] = insts.get(k, 0) + 1
    obj_tars, scene_tars = {i: 0 for i in obj_ids}, {i: 0 for i in scene_ids}
    for (o, s, _), n in insts.items():
        n = min(n_top, n) if n_top > 0 else n
        obj_tars[o] += n
        scene_tars[s] += n
    obj_tps, scene_tps = {i: 0 for i in obj_ids}, {i: 0 for i in scene_ids}
    for m in matches:
        if m["valid"] and m["est_id"] != -1:
            obj_tps[m["obj_id"]] += 1
            scene_tps[m["scene_id"]] += 1
    tars, tps = sum(obj_tars.values()), sum(obj_tps.values())
    obj_recalls = {i: recall(obj_tps[i], obj_tars[i]) for i in obj_ids}
    scene_recalls = {i: float(recall(scene_tps[i], scene_tars[i])) for i in scene_ids}
    return {"recall": float(recall(tps, tars)), "obj_recalls": obj_recalls, "mean_obj_recall": float(np.mean(list(obj_recalls.values()))),
            "scene_recalls": scene_recalls, "mean_scene_recall": float(np.mean(list(scene_recalls.values()))), "gt_count": len(matches),
            "targets_count": int(tars), "tp_count": int(tps)}


def score_dataset(case, th):
    matches = match_dataset(case, th)
    return localization_scores(case["scene_ids"], case["obj_ids"], matches, case["n_top"]), matches


# ---- tables --------------------------------------------------------------------------------------------------------------------------
def build_table(groups, th, n_obj, n_scene, n_top=0):
    """groups: [(err [E][G] nested list, valid [G], obj index, scene index)] -> the tables of fp_bop_scores"""
    err, rows, valid, obj, scene = [], [], [], [], []
    for e, v, o, s in groups:
        G = len(v)
        assert all(len(r) == G for r in e)
        rows.append([len(err), len(e), G, len(valid)])
        err += [x for r in e for x in r]
        valid += list(v)
        obj += [o] * G
        scene += [s] * G
    return {"err": np.asarray(err, np.float64), "groups": np.asarray(rows, np.int32).reshape(-1, 4), "gt_valid": np.asarray(valid, np.uint8),
            "gt_obj": np.asarray(obj, np.int32), "gt_scene": np.asarray(scene, np.int32), "th": np.asarray(th, np.float64), "n_obj": n_obj,
            "n_scene": n_scene, "n_top": n_top}


def score_table(t):
    """dict loops per threshold and group -> (match [T,R], tp_obj [T,n_obj], tp_scene [T,n_scene], tar_obj, tar_scene), int32"""
    T, R = len(t["th"]), len(t["gt_valid"])
    match = np.full((T, R), -1, np.int32)
    tp_obj, tp_scene = np.zeros((T, t["n_obj"]), np.int32), np.zeros((T, t["n_scene"]), np.int32)
    tar_obj, tar_scene = np.zeros(t["n_obj"], np.int32), np.zeros(t["n_scene"], np.int32)
    for off, E, G, first in t["groups"].tolist():
        if G == 0:
            continue
        mask = {g: bool(t["gt_valid"][first + g]) for g in range(G)}
        o, s = int(t["gt_obj"][first]), int(t["gt_scene"][first])
        n = sum(mask.values())
        n = min(t["n_top"], n) if t["n_top"] > 0 else n
        tar_obj[o] += n
        tar_scene[s] += n
        # rows are in matching order already: a strictly decreasing score keeps it under the sort
        errs = [{"est_id": e, "score": -e, "errors": {g: [float(t["err"][off + e * G + g])] for g in range(G)}} for e in range(E)]
        for ti, th in enumerate(t["th"].tolist()):
            for m in match_group(errs, th, 0, mask):
                match[ti, first + m["gt_id"]] = m["est_id"]
                tp_obj[ti, o] += 1
                tp_scene[ti, s] += 1
    return match, tp_obj, tp_scene, tar_obj, tar_scene


def edge_groups():
    """(E, G) in (0,1) (1,1) (1,0) (2,1) (2,2) (2,2) (7,3) (3,65) with the named edge values; thresholds TH10"""
    rng = np.random.Generator(np.random.PCG64(65))
    big = rng.uniform(0.0, 0.6, size=(3, 65))
    big[0, 7] = big[0, 40] = 0.01                            # an error tie far apart: the earlier column wins
    big[1, 7] = 0.02
    big_valid = (rng.random(65) < 0.8).astype(int).tolist()
    big_valid[7] = big_valid[40] = 1
    return [
        ([], [1], 0, 0),                                                         # no estimate: one target, never matched
        ([[TH10[3]]], [1], 0, 0),                                                # error == threshold 3: matched only above it
        ([[]], [], 1, 0),                                                        # one estimate, no ground truth
        ([[0.12], [0.07]], [1], 1, 1),                                           # below 0.12 the second estimate gets the ground truth
        ([[0.1, 0.1], [0.3, 0.11]], [1, 1], 2, 1),                               # error tie across two ground truths
        ([[0.06, 0.2], [0.07, 0.3]], [1, 1], 2, 0),                              # the loser's second choice exists only above 0.3
        ([[NAN, 0.01, 0.3], [0.2, 0.0, INF], [INF, NAN, NAN], [0.26, 0.02, 0.04], [0.4, 0.4, 0.4], [-INF, 0.3, 0.2], [0.0, 0.0, 0.0]],
         [1, 0, 1], 0, 1),                                                       # NaN, inf, the invalid column holds the lowest errors
        (big.tolist(), big_valid, 1, 0),
    ]


def table_cases():
    g = edge_groups()
    out = {"edge_T10": build_table(g, TH10, 4, 3), "edge_T1": build_table(g, [TH10[3]], 4, 3), "edge_ntop1": build_table(g, TH10, 4, 3, n_top=1),
           "edge_ntop2": build_table(g, TH10[:2], 4, 3, n_top=2), "reversed": build_table(g[::-1], TH10, 4, 3),
           "no_group": build_table([], TH10, 2, 2), "only_empty": build_table([g[2]], TH10, 2, 2)}
    return out


# ---- dataset cases -------------------------------------------------------------------------------------------------------------------
def _gt(objs):
    return [{"obj_id": o} for o in objs]


def _info(fracts):
    return [{"visib_fract": f} for f in fracts]


def _est(im_id, obj_id, est_id, score, errors):
    return {"im_id": im_id, "obj_id": obj_id, "est_id": est_id, "score": score, "errors": {g: [e] for g, e in errors.items()}}


def edge_dataset(error_type="cus", n_top=-1, visib_gt_min=-1, thresholds=TH10, scale=1.0):
    """Objects 1..4 (4 has no target anywhere), scenes 1..3 (3 is not in the targets).  `scale` multiplies every error, so that the same
    decisions come out after the normalisation of chamfer (diameter) or chamfer_proj (image width)."""
    targets = [{"scene_id": 1, "im_id": 3, "obj_id": 1, "inst_count": 2}, {"scene_id": 1, "im_id": 3, "obj_id": 3, "inst_count": 1},
               {"scene_id": 1, "im_id": 7, "obj_id": 1, "inst_count": 1}, {"scene_id": 1, "im_id": 7, "obj_id": 3, "inst_count": 3},
               {"scene_id": 2, "im_id": 1, "obj_id": 2, "inst_count": 1}, {"scene_id": 2, "im_id": 1, "obj_id": 1, "inst_count": 1}]
    scene_gt = {1: {3: _gt([1, 2, 1, 1, 3]), 7: _gt([1, 3, 3, 3]), 9: _gt([4])}, 2: {1: _gt([2, 2, 1])}}
    # image (1,3): object 1 has three instances, inst_count 2, equal fractions 0.7 for gt 0 and 3 and 0.9 for gt 2: valid = 2 and 0;
    # object 2 is no target.  visib_gt_min = 0.6 makes 0, 2, 3 valid instead.
    info = {1: {3: _info([0.7, 1.0, 0.9, 0.7, 0.65]), 7: _info([0.5, 0.8, 0.8, 0.3]), 9: _info([1.0])}, 2: {1: _info([0.9, 0.95, 0.61])}}
    s = scale
    errs = {1: [
        # (1,3) object 1: a score tie between est 0 and 1 (file order decides), est 2 has the lowest error on gt 3 (invalid under -1)
        _est(3, 1, 0, 0.8, {0: 0.1 * s, 2: 0.1 * s, 3: 0.3 * s}), _est(3, 1, 1, 0.8, {0: 0.04 * s, 2: 0.21 * s, 3: 0.3 * s}),
        _est(3, 1, 2, 0.5, {0: 0.02 * s, 2: 0.33 * s, 3: 0.001 * s}), _est(3, 1, 3, 0.9, {0: NAN, 2: INF, 3: TH10[5] * s}),
        _est(3, 2, 4, 0.99, {1: 0.0}),                                         # an estimate of the non-target object
        _est(3, 3, 5, 0.3, {4: TH10[1] * s}),                                   # error == threshold 1
        # (1,7) object 3: three instances, all wanted; object 1: no estimate
        _est(7, 3, 0, 0.6, {1: 0.06 * s, 2: 0.2 * s, 3: 0.45 * s}), _est(7, 3, 1, 0.5, {1: 0.07 * s, 2: 0.3 * s, 3: 0.12 * s}),
        _est(7, 3, 2, 0.4, {1: 0.01 * s, 2: 0.31 * s, 3: 0.13 * s}),
        _est(9, 4, 0, 0.9, {0: 0.0}),                                          # an image that is not in the targets
    ], 2: [
        _est(1, 2, 0, 1, {0: 0.12 * s, 1: 0.09 * s}), _est(1, 2, 1, 0.5, {0: 0.07 * s, 1: 0.08 * s}),      # an integer score, as read
        _est(1, 5, 2, 0.5, {2: 0.0}),                                          # an object with no ground truth in the image
    ]}
    return {"targets": targets, "scene_gt": scene_gt, "scene_gt_info": info, "errs": errs, "obj_ids": [1, 2, 3, 4], "scene_ids": [1, 2, 3],
            "n_top": n_top, "visib_gt_min": visib_gt_min, "error_type": error_type, "thresholds": list(thresholds),
            "diameters": {1: 200.0, 2: 150.0, 3: 75.5, 4: 10.0, 5: 1.0}, "im_width": 1280}


def crowd_dataset():
    """one image with 65 instances of one object and 3 estimates (E, G) = (3, 65); inst_count 40 < 65"""
    rng = np.random.Generator(np.random.PCG64(6565))
    fr = np.round(rng.uniform(0.1, 1.0, 65), 1).tolist()                        # many equal fractions
    e = rng.uniform(0.0, 0.6, (3, 65))
    e[0, 11] = e[0, 50] = 0.01
    errs = {4: [_est(0, 7, k, [0.5, 0.9, 0.5][k], {g: float(e[k, g]) for g in range(65)}) for k in range(3)]}
    return {"targets": [{"scene_id": 4, "im_id": 0, "obj_id": 7, "inst_count": 40}], "scene_gt": {4: {0: _gt([7] * 65)}},
            "scene_gt_info": {4: {0: _info(fr)}}, "errs": errs, "obj_ids": [7], "scene_ids": [4], "n_top": -1, "visib_gt_min": -1,
            "error_type": "cus", "thresholds": [0.05, 0.3], "diameters": {7: 1.0}, "im_width": 640}


def random_dataset(seed=2019, scenes=4, images=25, n_top=0, visib_gt_min=-1, thresholds=(0.1, 0.25, 0.4)):
    """about 200 groups: per image 1-3 target objects with 1-3 instances each, 0-5 estimates per group, errors on a coarse grid so that
    ties and errors equal to a threshold occur"""
    rng = np.random.Generator(np.random.PCG64(seed))
    targets, scene_gt, info, errs = [], {}, {}, {}
    for s in range(1, scenes + 1):
        scene_gt[s], info[s], errs[s] = {}, {}, []
        for im in range(images):
            objs = rng.choice(np.arange(1, 7), size=rng.integers(1, 4), replace=False).tolist()
            gts = []
            for o in objs:
                gts += [o] * int(rng.integers(1, 4))
            gts = [gts[i] for i in rng.permutation(len(gts))]
            scene_gt[s][im], info[s][im] = _gt(gts), _info(np.round(rng.uniform(0, 1, len(gts)), 1).tolist())
            for o in objs[:max(1, len(objs) - (im % 3 == 0))]:                  # every third image: the last object is no target
                targets.append({"scene_id": s, "im_id": im, "obj_id": o, "inst_count": int(rng.integers(1, 3))})
            for o in objs:
                cols = [g for g, x in enumerate(gts) if x == o]
                for k in range(int(rng.integers(0, 6))):
                    vals = np.round(rng.uniform(0, 0.5, len(cols)), 2).tolist()
                    if rng.random() < 0.05:
                        vals[0] = NAN
                    errs[s].append(_est(im, o, k, float(np.round(rng.random(), 1)), dict(zip(cols, vals))))
    return {"targets": targets, "scene_gt": scene_gt, "scene_gt_info": info, "errs": errs, "obj_ids": list(range(1, 8)),
            "scene_ids": list(range(1, scenes + 2)), "n_top": n_top, "visib_gt_min": visib_gt_min, "error_type": "cus",
            "thresholds": list(thresholds), "diameters": {o: 100.0 for o in range(1, 8)}, "im_width": 640}


def dataset_cases():
    out = {}
    for n_top in (-1, 0, 1, 2):
        for vis in (-1, 0.6):
            et, scale, ths = [("cus", 1.0, TH10), ("chamfer", 200.0, TH10), ("chamfer_proj", 200.0, TH10_PX)][(n_top + 1 + (vis > 0)) % 3]
            out[f"edge_ntop{n_top}_vis{vis}_{et}"] = edge_dataset(et, n_top, vis, ths, scale)
    out["edge_T1"] = edge_dataset("cus", -1, -1, [TH10[1]])
    out["crowd"] = crowd_dataset()
    out["random"] = random_dataset()
    out["random_ntop1_vis"] = random_dataset(seed=7, scenes=2, images=10, n_top=1, visib_gt_min=0.3, thresholds=(0.25,))
    return out


def case_norm_args(case):
    """the `diameters` / `im_width` arguments BopScorer.scores takes for the case's error type"""
    return {"diameters": case["diameters"] if case["error_type"] in ("ad", "add", "adi", "mssd", "chamfer") else None,
            "im_width": case["im_width"] if case["error_type"] in ("mspd", "chamfer_proj") else None}


# ---- the host check ------------------------------------------------------------------------------------------------------------------
def run_host_check(exe, tmp, t):
    """tools/bop_score_host_check.cpp on one table -> (match, tp_obj, tp_scene, tar_obj, tar_scene)"""
    fin, fout = tmp / "bop_table.bin", tmp / "bop_out.bin"
    P, Gr, R, T = len(t["err"]), len(t["groups"]), len(t["gt_valid"]), len(t["th"])
    with open(fin, "wb") as f:
        f.write(np.asarray([P, Gr, R, T, t["n_obj"], t["n_scene"], t["n_top"]], np.int32).tobytes())
        for a, dt in ((t["err"], np.float64), (t["th"], np.float64), (t["groups"], np.int32), (t["gt_obj"], np.int32), (t["gt_scene"], np.int32),
                      (t["gt_valid"], np.uint8)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    o = np.fromfile(fout, np.int32)
    n = [T * R, T * t["n_obj"], T * t["n_scene"], t["n_obj"], t["n_scene"]]
    assert len(o) == sum(n), (len(o), n)
    parts = np.split(o, np.cumsum(n)[:-1])
    return parts[0].reshape(T, R), parts[1].reshape(T, t["n_obj"]), parts[2].reshape(T, t["n_scene"]), parts[3], parts[4]
