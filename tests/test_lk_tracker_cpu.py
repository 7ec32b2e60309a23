"""The built-in point tracker without a GPU: the numpy restatement (tests/_lk_ref.py) against the planted truth of the synthetic clips,
the sanitised host check (tools/lk_host_check.cpp: csrc/lk_core.h in the kernel's order) against the restatement, and the host logic of
freepose_amd.tracker."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import _lk_ref as ref

ROOT = Path(__file__).resolve().parent.parent


# ---- 1. the restatement against the truth ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_restatement_against_the_planted_truth(name):
    """REF_VS_TRUTH was measured with `python -m tests._lk_ref`; recomputed here.  (Case H, the rendered mesh clip, needs the rasteriser:
    tests/test_gpu_lk_tracker.py::test_mesh_clip.)"""
    c, r = ref.case(name), ref.reference(name)
    med, p95, share = ref.truth_error(r["tracks"], r["vis"], c["truth"], c["queries"])
    want = ref.REF_VS_TRUTH[name]
    print(f"\n[lk] case {name}: restatement vs truth median {med:.4f} px, p95 {p95:.4f} px, visible share {share:.4f} (recorded {want})")
    assert abs(med - want[0]) <= 1e-3 + 0.02 * want[0] and abs(p95 - want[1]) <= 1e-3 + 0.02 * want[1] and abs(share - want[2]) <= 0.01
    assert np.isfinite(r["tracks"]).all()


def test_a_single_level_loses_the_large_translation():
    """case B with levels = 1: the restatement itself loses at least half of the points (so B exercises the pyramid), with levels = 4 it
    keeps almost all"""
    c1, r1, c4, r4 = ref.case("B1"), ref.reference("B1"), ref.case("B"), ref.reference("B")
    err1 = np.sqrt(((r1["tracks"] - c1["truth"]) ** 2).sum(-1))
    lost = (~r1["vis"][-1]) | (err1[-1] > 1.0)
    assert lost.mean() >= 0.5, lost.mean()
    assert len(r1["pyr"]) == 1 and len(r4["pyr"]) == 4
    assert ref.truth_error(r4["tracks"], r4["vis"], c4["truth"], c4["queries"])[2] > 0.9


def test_named_expectations_hold_for_the_restatement():
    """E: points under the block at frame 3 are invisible from frame 3 on, also at frame 5 where the block is gone (sticky); points
    further than 2 r + 4 from it are unaffected.  "Under the block" is narrowed to points whose whole (2 r + 1)^2 window lies under it at
    frame 3: a window that straddles the block's edge still sees moving texture and may legitimately keep its point, so nothing is
    claimed for those.  F: points inside the flat rectangle are invisible in every frame but
    their own.  G: points are invisible once the true position is outside.  All tracks finite."""
    ref.assert_named_expectations(lambda name: (ref.reference(name)["tracks"], ref.reference(name)["vis"]))


# ---- 2. the host check against the restatement ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("lk_host_check")
    return ref.build_host_check(d), d


@pytest.mark.parametrize("name", ref.HOST_CASES)
def test_host_check_against_the_restatement(host_check, name):
    """lk_core.h in the kernel's order, built with -fsanitize=address,undefined: the pyramid equals the float32 restatement bit for bit;
    on compared rows the tracks and diagnostics lie within CPU_HOST_VS_REF (measured with `python -m tests._lk_ref`) and the visibility
    flags are equal; compared rows are at least 90 % of the rows the restatement calls visible and at most 2 % of all rows lie inside
    the threshold band (properties of the inputs and the restatement alone)."""
    exe, work = host_check
    c, r = ref.case(name), ref.reference(name)
    run = ref.run_host_check(exe, c, work)
    assert len(run["pyr"]) == len(r["pyr"])
    for a, b in zip(run["pyr"], r["pyr"]):
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
    if name.startswith("C"):
        assert len(r["pyr"]) == 2                                   # 61 x 47 at radius 7: levels 2 and 3 of the 4 requested are dropped
    m = ref.compare(r, run["tracks"], run["vis"], run["diag"], c["queries"], c["params"], ref.CPU_HOST_VS_REF)
    print(f"\n[lk] case {name}: host check vs restatement track {m['track']:.3e} px, diagnostics {m['diag']:.3e}, compared "
          f"{m['n_compared']} rows ({m['compared_share']:.3f} of visible), in band {m['band_share']:.4f}")
    assert m["compared_share"] >= 0.9 and m["band_share"] <= 0.02
    assert m["track"] <= ref.CPU_HOST_VS_REF[0] and m["diag"] <= ref.CPU_HOST_VS_REF[1]
    assert m["flags_equal"] and m["vis_equal_settled"]             # visible rows, and every row whose verdict is settled, lost ones included
    assert np.isfinite(run["tracks"]).all() and np.isfinite(run["diag"]).all() and set(np.unique(run["vis"])) <= {0, 1}
    if name == "C_T1":
        assert np.array_equal(run["tracks"][0], c["queries"][:, 1:]) and run["vis"].all()


def test_recorded_difference_leaves_the_device_bound_below_a_twentieth_of_a_pixel():
    assert 10 * ref.CPU_HOST_VS_REF[0] <= 0.05


# ---- 3. host logic ---------------------------------------------------------------------------------------------------------------------------
def test_tracker_refusals():
    from freepose_amd.tracker import LKTracker
    frames = np.zeros((3, 20, 24, 3), np.uint8)
    q = np.array([[0, 5.0, 5.0]], np.float32)
    tr = LKTracker()
    with pytest.raises(ValueError, match="dtype"):
        tr(frames.astype(np.float32), q)
    with pytest.raises(ValueError, match="shape"):
        tr(frames[0], q)
    with pytest.raises(ValueError, match="shape"):
        tr(frames[..., :2], q)
    with pytest.raises(ValueError, match="queries of shape"):
        tr(frames, q[:, :2])
    for t in (-1, 3, 7.5):
        with pytest.raises(ValueError, match="query time outside"):
            tr(frames, np.array([[t, 5.0, 5.0]], np.float32))
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="non-finite"):
            tr(frames, np.array([[0, bad, 5.0]], np.float32))
    for kw in (dict(levels=0), dict(levels=9), dict(radius=0), dict(radius=16), dict(iters=0), dict(iters=65)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            LKTracker(**kw)


def test_load_tracker_round_trip():
    from freepose_amd import tracker
    from freepose_amd.scripts.smooth_poses_video import load_tracker
    t = load_tracker("freepose_amd.tracker:klt", '{"radius": 9, "min_eig": 2.5}')
    assert isinstance(t, tracker.LKTracker) and t.radius == 9 and t.min_eig == 2.5 and t.levels == 4 and t.iters == 10 and t.fb_thresh == 1.0
    d = load_tracker("freepose_amd.tracker:klt")
    assert (d.min_eig, d.max_residual) == (tracker.DEFAULT_MIN_EIG, tracker.DEFAULT_MAX_RESIDUAL) and d.last is None


def test_header_and_ctypes_rows():
    from freepose_amd import _lib, ops
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "freepose_hip.h").read_text(), flags=re.S)
    for name, n_args in (("fp_lk_pyramid", 9), ("fp_lk_track", 17)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m and len(m.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    lib = _lib.load()
    assert hasattr(lib, "fp_lk_pyramid") and hasattr(lib, "fp_lk_track")
    core = (ROOT / "freepose_amd" / "csrc" / "lk_core.h").read_text()
    for macro, value in (("FP_LK_MAX_LEVELS", ops.LK_MAX_LEVELS), ("FP_LK_MAX_RADIUS", ops.LK_MAX_RADIUS), ("FP_LK_MAX_ITERS", ops.LK_MAX_ITERS),
                         ("FP_LK_FLAG_FB", ops.LK_FLAG_FB), ("FP_LK_FLAG_EIG", ops.LK_FLAG_EIG), ("FP_LK_FLAG_RESIDUAL", ops.LK_FLAG_RESIDUAL),
                         ("FP_LK_FLAG_OUTSIDE", ops.LK_FLAG_OUTSIDE), ("FP_LK_FLAG_LOST_BEFORE", ops.LK_FLAG_LOST_BEFORE)):
        assert re.search(r"#define %s\s+%d\b" % (macro, value), core), macro
    assert re.search(r"#define FP_LK_EIG_FLOOR\s+1e-4\s", core) and ref.EIG_FLOOR == 1e-4
    assert ops.lk_layout(61, 47, 4, 7) == ref.layout(61, 47, 4, 7) == [(61, 47), (31, 24)]
    assert ops.lk_layout(720, 1280, 4, 7) == [(720, 1280), (360, 640), (180, 320), (90, 160)]
    # refused before anything is launched (no device here either): status + message
    import ctypes
    one = ctypes.c_void_p(8)
    ctx = one
    assert lib.fp_lk_pyramid(None, one, 2, 8, 8, 4, 7, one, None) == 1 and b"lk_pyramid: null" in lib.fp_last_error()
    for args, msg in (((0, 8, 8, 4, 7), b"T=0"), ((2, 0, 8, 4, 7), b"0 x 8"), ((2, 8, 8, 0, 7), b"levels=0"), ((2, 8, 8, 9, 7), b"levels=9"),
                      ((2, 8, 8, 4, 0), b"radius=0"), ((2, 8, 8, 4, 16), b"radius=16")):
        assert lib.fp_lk_pyramid(ctx, one, *args, one, None) == 1 and msg in lib.fp_last_error(), args
    assert lib.fp_lk_track(ctx, one, 2, 8, 8, 4, one, -1, 7, 10, 1.0, 1.0, 10.0, one, one, one, None) == 1 and b"N=-1" in lib.fp_last_error()
    assert lib.fp_lk_track(ctx, one, 2, 8, 8, 4, None, 3, 7, 10, 1.0, 1.0, 10.0, one, one, one, None) == 1 and b"null" in lib.fp_last_error()
    for it in (0, 65):
        assert lib.fp_lk_track(ctx, one, 2, 8, 8, 4, one, 3, 7, it, 1.0, 1.0, 10.0, one, one, one, None) == 1 and b"iters=" in lib.fp_last_error()
    assert lib.fp_lk_track(ctx, one, 0, 8, 8, 4, one, 3, 7, 10, 1.0, 1.0, 10.0, one, one, one, None) == 1 and b"T=0" in lib.fp_last_error()
