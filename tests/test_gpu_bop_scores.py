"""BOP pose matching and recall counts on the MI355X (csrc/bop_score.hip) against the dict-loop restatement of tests/_bop_score_ref.py
and tests/golden/bop_scores.npz, which the reference's own match_poses / match_poses_scene / calc_localization_scores / save_json wrote.

Everything is compared with ==.  The device does no floating-point arithmetic beyond `<`, and the floats in the files are produced on the
host from the fp64 operations the reference performs: there is no tolerance to choose."""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import _bop_score_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("match", "tp_obj", "tp_scene", "tar_obj", "tar_scene")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.loads(str(np.load(golden_dir / "bop_scores.npz")["json"]))


@pytest.fixture(scope="module")
def datasets():
    return ref.dataset_cases()


def _scorer(case):
    from freepose_amd.evaluation import BopScorer
    return BopScorer(case["targets"], case["scene_gt"], case["scene_gt_info"], case["obj_ids"], case["scene_ids"], case["visib_gt_min"])


@pytest.fixture(scope="module")
def tables(datasets):
    """name -> (table, restatement's answer, computed once): the hand-made tables and the packed table of every dataset case"""
    out = dict(ref.table_cases())
    for name, c in datasets.items():
        t = _scorer(c).pack(c["errs"], c["n_top"], **ref.case_norm_args(c))
        t.update(th=np.asarray(c["thresholds"], np.float64), n_obj=len(c["obj_ids"]), n_scene=len(c["scene_ids"]))
        out["packed_" + name] = t
    return {k: (t, ref.score_table(t)) for k, t in out.items()}


def _run(t, th=None):
    from freepose_amd import ops
    res = ops.bop_scores(t["err"], t["groups"], t["gt_valid"], t["gt_obj"], t["gt_scene"], t["th"] if th is None else th, t["n_obj"],
                         t["n_scene"], t["n_top"])
    return [r.cpu().numpy() for r in res]


def test_kernel_equals_the_restatement_on_every_case(tables, golden):
    assert len(tables["packed_random"][0]["groups"]) >= 150
    for name, (t, want) in tables.items():
        got = _run(t)
        for a, w, n in zip(got, want, NAMES):
            assert a.dtype == np.int32 and a.shape == w.shape and np.array_equal(a, w), (name, n, np.argwhere(a != w)[:5].tolist())
        if name in golden["tables"]:
            for a, n in zip(got, NAMES):
                assert np.array_equal(a, np.asarray(golden["tables"][name][n]).reshape(a.shape)), (name, n)


def test_two_calls_give_the_same_bits_and_T10_equals_ten_T1(tables):
    for name in ("edge_T10", "packed_random", "packed_crowd"):
        t = tables[name][0]
        a, b = _run(t), _run(t)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), name
    t = tables["edge_T10"][0]
    all10 = _run(t)
    for i, th in enumerate(t["th"]):
        one = _run(t, [th])
        assert np.array_equal(one[0][0], all10[0][i]) and np.array_equal(one[1][0], all10[1][i]) and np.array_equal(one[2][0], all10[2][i])
        assert np.array_equal(one[3], all10[3]) and np.array_equal(one[4], all10[4])


def test_bad_tables_are_refused_with_a_message_without_a_launch(tables):
    import torch
    from freepose_amd import _lib, ops
    from freepose_amd._lib import current_stream, ptr
    t = tables["edge_T10"][0]
    R = len(t["gt_valid"])
    for row, what in (([0, 3, 65, R - 10], "reaches outside"), ([len(t["err"]) - 2, 1, 3, 0], "reaches outside"),
                      ([0, 1, 2, 1], "share ground-truth rows")):
        g = t["groups"].copy()
        g[0] = row
        with pytest.raises(ValueError, match=what):
            _run(dict(t, groups=g))
    o = t["gt_obj"].copy()
    o[3] = 4
    with pytest.raises(ValueError, match="gt_obj"):
        _run(dict(t, gt_obj=o))
    with pytest.raises(ValueError, match="T=0"):
        _run(t, [])
    # the C entry with a live context: bad sizes and null tables come back as FP_ERR_INVALID with a message; the outputs stay untouched
    lib = _lib.load()
    out = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    d = torch.zeros(64, dtype=torch.float64, device="cuda")
    for P, Gr, Rr, T, n_obj, what in ((1, 1, 1, 0, 1, b"T=0"), (1, 1, -1, 1, 1, b"R=-1"), (1, 1, 1, 1, 0, b"n_obj=0")):
        rc = lib.fp_bop_scores(ops.context(), ptr(d), ptr(d), ptr(d), ptr(d), ptr(d), ptr(d), P, Gr, Rr, T, n_obj, 1, 0, ptr(out), ptr(out),
                               ptr(out), ptr(out), ptr(out), current_stream())
        assert rc == 1 and what in lib.fp_last_error(), (what, lib.fp_last_error())
    rc = lib.fp_bop_scores(ops.context(), None, ptr(d), ptr(d), ptr(d), ptr(d), ptr(d), 1, 1, 1, 1, 1, 1, 0, ptr(out), ptr(out), ptr(out),
                           ptr(out), ptr(out), current_stream())
    assert rc == 1 and b"d_err" in lib.fp_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all())


def test_scorer_equals_the_golden_dicts_and_match_lists(datasets, golden):
    from freepose_amd.evaluation import bop_json_text
    for name, c in datasets.items():
        res = _scorer(c).scores(c["errs"], c["error_type"], c["thresholds"], c["n_top"], **ref.case_norm_args(c))
        assert len(res) == len(c["thresholds"])
        for w, (scores, matches) in zip(golden["datasets"][name], res):
            want_scores, want_matches = ref.score_dataset(c, w["th"])
            assert scores == want_scores and list(scores) == list(want_scores), (name, w["th"])
            assert bop_json_text(scores) == w["scores_text"], (name, w["th"])
            assert bop_json_text(matches) == w["matches_text"], (name, w["th"])
            assert len(matches) == len(want_matches)


# ---- CLIs ------------------------------------------------------------------------------------------------------------------------------
def _write_dataset(case, root, error_sign):
    """the case as a dataset directory + one errors directory: targets, scene_gt, scene_gt_info, models_info, errors files and one image
    of the case's width.  No meshes."""
    from PIL import Image
    from freepose_amd.scripts.eval_calc_errors import errors_json
    ds = root / "datasets" / "toyds"
    (ds / "models_eval").mkdir(parents=True)
    (ds / "models_eval" / "models_info.json").write_text(json.dumps({str(o): {"diameter": case["diameters"][o]} for o in case["obj_ids"]}))
    (ds / "test_targets_bop19.json").write_text(json.dumps(case["targets"]))
    for s in case["scene_ids"]:
        (ds / "test" / f"{s:06d}").mkdir(parents=True)
    for s, gt in case["scene_gt"].items():
        (ds / "test" / f"{s:06d}" / "scene_gt.json").write_text(json.dumps(gt))
        (ds / "test" / f"{s:06d}" / "scene_gt_info.json").write_text(json.dumps(case["scene_gt_info"][s]))
    t = case["targets"][0]
    (ds / "test" / f"{t['scene_id']:06d}" / "depth").mkdir()
    Image.fromarray(np.zeros((2, case["im_width"]), np.uint16)).save(ds / "test" / f"{t['scene_id']:06d}" / "depth" / f"{t['im_id']:06d}.png")
    ed = root / "evals" / "hip_toyds-test" / error_sign
    ed.mkdir(parents=True)
    for s, errs in case["errs"].items():
        (ed / f"errors_{s:06d}.json").write_text(errors_json(errs))
    return ed


@pytest.mark.parametrize("name", ["edge_ntop-1_vis-1_cus", "edge_ntop-1_vis0.6_chamfer", "edge_ntop0_vis0.6_chamfer_proj", "edge_ntop2_vis-1_cus"])
def test_eval_calc_scores_writes_the_reference_files(name, datasets, golden, tmp_path):
    from freepose_amd.scripts import eval_calc_scores as cs
    c = datasets[name]
    sign = f"error={c['error_type']}_ntop={c['n_top']}"
    ed = _write_dataset(c, tmp_path, sign)
    cs.run(["--error_dir_paths", f"hip_toyds-test/{sign}", "--eval_path", str(tmp_path / "evals"), "--datasets_path", str(tmp_path / "datasets"),
            f"--correct_th_{c['error_type']}", ";".join(str(t) for t in c["thresholds"]), "--visib_gt_min", str(c["visib_gt_min"])])
    written = sorted(p.name for p in ed.glob("*.json") if not p.name.startswith("errors_"))
    assert len(written) == 2 * len(c["thresholds"])
    for w in golden["datasets"][name]:
        assert (ed / f"scores_{w['sign']}.json").read_bytes() == w["scores_text"].encode(), (name, w["th"])
        assert (ed / f"matches_{w['sign']}.json").read_bytes() == w["matches_text"].encode(), (name, w["th"])


def test_eval_bop19_pose_end_to_end(golden_dir, tmp_path, monkeypatch):
    from freepose_amd.scripts import eval_bop19_pose as bop, eval_calc_errors as ce
    from tests.test_gpu_eval import _make_dataset
    for k in ("SLURM_JOB_ID", "SLURM_ARRAY_TASK_ID"):
        monkeypatch.delenv(k, raising=False)
    gold = np.load(golden_dir / "pose_errors.npz")
    _make_dataset(gold, tmp_path)
    ds = tmp_path / "datasets" / "toyds"
    for scene in (1, 2):                                     # that dataset's scene_gt_info has no visibility: everything fully visible
        f = ds / "test" / f"{scene:06d}" / "scene_gt_info.json"
        f.write_text(json.dumps({im: [dict(g, visib_fract=1.0) for g in gts] for im, gts in json.loads(f.read_text()).items()}))
    argv = ["--result_filenames", "hip_toyds-test.csv", "--results_path", str(tmp_path / "results"), "--eval_path", str(tmp_path / "evals"),
            "--datasets_path", str(tmp_path / "datasets"), "--models_inference_path", str(tmp_path / "models_inf"), "--renderer_type", "cpp"]
    final = bop.run(argv)["hip_toyds-test.csv"]
    out = tmp_path / "evals" / "hip_toyds-test"
    text = (out / "scores_bop19.json").read_text()
    saved = json.loads(text)
    keys = ["bop19_average_recall", "bop19_average_recall_chamfer", "bop19_average_recall_chamfer_proj", "bop19_average_recall_cus",
            "bop19_average_time_per_image"]
    assert sorted(saved) == keys and saved == {k: float(v) for k, v in final.items()} and saved["bop19_average_time_per_image"] == 0.25
    # the restatement on the errors files the run wrote
    targets = json.loads((ds / "test_targets_bop19.json").read_text())
    case = {"targets": targets, "obj_ids": [1, 2], "scene_ids": [1, 2], "n_top": -1, "visib_gt_min": -1,
            "scene_gt": {s: ce.load_json(ds / "test" / f"{s:06d}" / "scene_gt.json", keys_to_int=True) for s in (1, 2)},
            "scene_gt_info": {s: ce.load_json(ds / "test" / f"{s:06d}" / "scene_gt_info.json", keys_to_int=True) for s in (1, 2)},
            "diameters": {k: v["diameter"] for k, v in ce.load_json(ds / "models_eval" / "models_info.json", keys_to_int=True).items()},
            "im_width": int(gold["width"])}
    recalls = {}
    for et, ths in (("cus", ref.TH10), ("chamfer", ref.TH10), ("chamfer_proj", ref.TH10_PX)):
        ed = out / f"error={et}_ntop=-1"
        c = dict(case, error_type=et, errs={s: ce.load_json(ed / f"errors_{s:06d}.json", keys_to_int=True) for s in (1, 2)})
        per_th = []
        for th in ths:
            scores, matches = ref.score_dataset(c, th)
            sign = ref.score_signature([th], -1.0)
            assert (ed / f"scores_{sign}.json").read_text() == ref.save_json_text(scores), (et, th)
            assert (ed / f"matches_{sign}.json").read_text() == ref.save_json_text(matches), (et, th)
            per_th.append(scores["recall"])
        recalls[et] = float(np.mean(per_th))
        assert saved[f"bop19_average_recall_{et}"] == recalls[et], et
        print(et, "recalls", per_th)
    assert saved["bop19_average_recall"] == float(np.mean(list(recalls.values())))
    assert 0.0 < saved["bop19_average_recall"] < 1.0         # half of the targets have no estimate of their own; the exact pose matches
    # a second run finds the errors on disk: none is recomputed, the scores are the same text
    files = sorted(out.rglob("errors_*.json"))
    assert len(files) == 6
    stamps = [f.stat().st_mtime_ns for f in files]
    bop.run(argv)
    assert [f.stat().st_mtime_ns for f in files] == stamps and (out / "scores_bop19.json").read_text() == text
    # --errors selects a subset
    sub = bop.run(argv + ["--errors", "cus", "--eval_path", str(tmp_path / "evals_cus")])["hip_toyds-test.csv"]
    assert sorted(sub) == ["bop19_average_recall", "bop19_average_recall_cus", "bop19_average_time_per_image"]
    assert float(sub["bop19_average_recall"]) == saved["bop19_average_recall_cus"] == float(sub["bop19_average_recall_cus"])
