"""No-GPU proof obligations of tests/_raster_cases.py: every branch label is claimed, every case reaches what it claims (classify), the
construction really is exact (the oracle's vertex stage returns the integers put in), the oracle equals the integer known answer on every
constructed case (coverage, owner, colour exactly; depth within DEPTH_ULP), and the launch-plan mirror is the library's own statement
(csrc/raster_plan.h through tools/raster_plan_host_check.cpp, built under the host sanitizers).  The last test prints the ledger: which
cases reach which label, and which labels the random soups of tests/test_gpu_fuzz.py happen to reach."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import fp_oracle as fo
from tests import _raster_cases as rc

ROOT = Path(__file__).resolve().parent.parent
KNOWN = [c for c in rc.CASES if c.known]
ISSUE_LABELS = [   # the list of the issue that asked for this table, spelled out once more so that a label cannot leave LABELS unnoticed
    "tiled-T64", "tiled-T72", "tiled-T80", "tiled-T88", "global-forced", "global-by-size", "global-by-count", "tiled-at-count-limit",
    "tiles-exact-x", "tiles-exact-y", "tiles-partial-x", "tiles-partial-y", "flush-dword", "flush-bytes-w1", "flush-bytes-w2", "flush-bytes-w3",
    "views-lt8", "views-groups-only", "views-8", "views-16", "views-groups+rem", "views-11", "views-19", "chunks-1-partial", "chunks-exact",
    "chunks-tail", "bin-grid-tail", "rounds-1-full", "rounds-2", "tile-untouched", "tile-hit-but-empty", "drop-behind", "drop-zero-area",
    "drop-no-centre", "drop-offscreen", "swapped", "unswapped", "cull-front", "cull-back", "small-32767", "wide-32768", "global-own-256",
    "global-queue-257", "tile-lane-32", "tile-wave-33", "tile-lane-w1", "tile-lane-w3", "tile-lane-w7", "tile-lane-w32", "tile-wave-w1",
    "tile-wave-w3", "tile-wave-w7", "tile-wave-w32", "spans-2x2-tiles", "spans-all-tiles", "clamp-30000", "straddler-1front", "straddler-2front",
    "edge-through-centres", "shared-edge-watertight", "tie-lowest-id", "box-0px-wide", "box-0px-narrow", "box-1..99px-wide",
    "box-1..99px-narrow", "box-ge100px-wide", "box-ge100px-narrow", "ext-negative-X"]


def test_every_label_is_claimed():
    assert set(ISSUE_LABELS) <= set(rc.LABELS), sorted(set(ISSUE_LABELS) - set(rc.LABELS))
    claimed = set().union(*(c.claims for c in rc.CASES))
    assert not set(rc.LABELS) - claimed, sorted(set(rc.LABELS) - claimed)
    assert not claimed - set(rc.LABELS), sorted(claimed - set(rc.LABELS))
    # the shapes the issue names: 65 triangles for the chunk tail, exactly the count limit and one more, both strategies for the culling
    # and the threshold cases, the global path for its own thresholds
    assert any(rc.n_faces(c) == 65 and "chunks-tail" in c.claims for c in rc.CASES)
    assert any(rc.n_faces(c) == rc.TILED_MAX_TRIS and -1 in c.modes and "tiled-at-count-limit" in c.claims for c in rc.CASES)
    assert any(rc.n_faces(c) == rc.TILED_MAX_TRIS + 1 and -1 in c.modes and "global-by-count" in c.claims for c in rc.CASES)
    assert any(rc.plan(c.W, c.H, rc.n_faces(c), 1, 1)["chunks"] >= rc.HITS_ROUND + 1 and "rounds-2" in c.claims for c in rc.CASES)
    for c in rc.CASES:
        if c.claims & {"cull-front", "cull-back", "small-32767", "wide-32768", "tie-lowest-id", "edge-through-centres", "clamp-30000",
                       "straddler-1front", "straddler-2front"} or c.extents:
            assert {0, 1} <= set(c.modes), c.name
        if c.claims & {"global-own-256", "global-queue-257", "global-forced"}:
            assert 0 in c.modes, c.name
        if any(label.startswith("tile-") for label in c.claims):
            assert 1 in c.modes, c.name


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.id)
def test_case_reaches_what_it_claims(case):
    reached = rc.classify(case)
    assert case.claims <= reached, sorted(case.claims - reached)
    assert case.W <= 708 and case.H <= 352 and case.Hn <= 19                     # small frames: the cases stay cheap
    xs, ys, zc = rc.geometry(case)
    front = zc > rc.ZNEAR
    assert np.isin(zc[front], [2.0 ** k for k in range(-4, 7)]).all() and (zc[~front] <= rc.ZNEAR).all()


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.id)
def test_vertex_stage_returns_the_constructed_integers(case):
    v, _, _ = rc.mesh(case)
    xy, z = fo.project_vertices(v, rc.poses(case), 1.0, *rc.intrinsics(case))
    for view in range(case.Hn):
        xi, yi, zc = rc.projected(case, view)
        front = (zc > rc.ZNEAR).reshape(-1)
        assert np.array_equal(z[view], zc.reshape(-1).astype(np.float32)), (case.name, view)
        assert np.array_equal(xy[view][front, 0], xi.reshape(-1)[front]) and np.array_equal(xy[view][front, 1], yi.reshape(-1)[front]), (case.name, view)


def _oracle_vs_known(case):
    """largest depth deviation (float32 ulp) of the oracle from the integer answer; coverage, owner and colour must be equal"""
    rgb, depth = rc.oracle_render(case)
    worst = 0
    for view in range(case.Hn):
        covered, owner, d_known, _ = rc.known_answer(case, view)
        assert np.array_equal(depth[view] > 0, covered), (case.name, view, "coverage")
        assert np.array_equal(depth[view] != 0, covered), (case.name, view, "background depth must be 0")
        assert np.array_equal(rgb[view], rc.expected_rgb(owner)), (case.name, view, "owner / colour")
        if covered.any():
            worst = max(worst, int(rc.depth_ulps(depth[view], d_known)[covered].max()))
    return worst


@pytest.mark.parametrize("case", KNOWN, ids=lambda c: c.id)
def test_oracle_equals_the_integer_known_answer(case):
    dev = _oracle_vs_known(case)
    print(f"{case.name}: oracle depth within {dev} ulp of the plane depth")
    assert dev <= rc.DEPTH_ULP <= 4, (case.name, dev)


def test_depth_ulp_is_the_measured_maximum():
    """DEPTH_ULP is what the oracle itself shows over the table, not a guess, and as a condition of its own at most 4 ulp"""
    worst = max(_oracle_vs_known(c) for c in KNOWN)
    print(f"largest oracle deviation over {len(KNOWN)} constructed cases: {worst} ulp; DEPTH_ULP = {rc.DEPTH_ULP}")
    assert worst == rc.DEPTH_ULP and rc.DEPTH_ULP <= 4


def test_threshold_boxes_cover_their_last_candidate():
    """a wrong row / column split of the per-lane coverage mask (the float-reciprocal divide) shows at the last candidate and along the
    box's first or last column: they must be lit (box_tri)"""
    case = rc.BY_NAME["tile-candidates-96x80"]
    s = rc.case_setup(case, 0)
    _, owner, _, _ = rc.known_answer(case, 0)
    for f in range(rc.n_faces(case)):
        x0, y0, x1, y1 = s.bbox[f]
        mine = owner[y0:y1 + 1, x0:x1 + 1] == f
        assert mine[-1, -1], (f, s.bbox[f])
        if x0 == x1 or y0 == y1:
            assert mine.all(), (f, s.bbox[f])
        else:
            assert mine[:, 0].sum() >= (y1 - y0) or mine[:, -1].sum() >= (y1 - y0), (f, s.bbox[f])


def test_one_triangle_per_pixel_cases_own_every_pixel_once():
    case = rc.BY_NAME["round-full-512x256"]
    _, owner, _, info = rc.known_answer(case, 0)
    assert np.array_equal(owner.reshape(-1), np.arange(case.W * case.H)) and (info["cover_n"] == 1).all()


# ---- the library's own statement of the launch arithmetic (csrc/raster_plan.h) against the mirror -----------------------------------------------
@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tools/raster_plan_host_check.cpp under the host sanitizers: [(W, H, F, Hn, mode)] -> [plan dict]; exit status 0 covers its own sweep
    of the invariants the kernels rely on, and the sanitizers"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("raster_plan") / "raster_plan_host_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "freepose_amd" / "csrc"),
           str(ROOT / "tools" / "raster_plan_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(shapes):
        text = "".join(" ".join(str(int(v)) for v in s) + "\n" for s in shapes)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        out = [rc.parse_plan(ln) for ln in r.stdout.splitlines()]
        assert len(out) == len(shapes)
        return out
    return run


def test_plan_of_every_case_is_the_headers(plan_check):
    shapes = [(c.W, c.H, rc.n_faces(c), c.Hn, m) for c in rc.CASES for m in (-1, 0, 1)]
    for s, got in zip(shapes, plan_check(shapes)):
        assert got == rc.plan(*s), f"W H F Hn mode = {s}: raster_plan.h says {got}, the mirror {rc.plan(*s)}"


def test_plan_mirror_on_a_sweep(plan_check):
    rng = np.random.Generator(np.random.PCG64(20251021))
    shapes = [(int(rng.integers(1, 8193)), int(rng.integers(1, 8193)), int(rng.integers(1, 2 ** 21 + 1)), int(rng.integers(0, 601)), int(rng.integers(-1, 2)))
              for _ in range(2000)]
    shapes += [(w, h, f, hn, m) for w in (512, 513, 576, 577, 640, 641, 704, 705) for h in (1, 480, 704, 705) for f in (1, 131072, 131073)
               for hn in (0, 7, 8, 19) for m in (-1, 0, 1)]
    for s, got in zip(shapes, plan_check(shapes)):
        assert got == rc.plan(*s), s
    documented = rc.plan(640, 24, 300, 11, -1)                                   # one plan spelled out by hand
    assert (documented["path"], documented["T"], documented["tiles"], documented["chunks"], documented["rounds"], documented["views"],
            documented["flush"]) == ("tiled", 80, (8, 1), 5, 1, (1, 3), "dword")


# ---- the library's own statement of the triangle set-up (csrc/raster_core.h) against the mirror ------------------------------------------------
@pytest.fixture(scope="module")
def core_check(tmp_path_factory):
    """tools/raster_core_host_check.cpp under the host sanitizers: rows [W, H, cull, x0, y0, z0, x1, y1, z1, x2, y2, z2] -> int array
    [n, 10] (ok, strad, swapped, area2, bx0, by0, bx1, by1, small, back_facing) of tri_setup_v; exit status 0 covers its own sweeps of the
    header's arithmetic claims (row / column split, 32-bit == 64-bit edge functions, reciprocal == quotient, key order), and the sanitizers"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("raster_core") / "raster_core_host_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "freepose_amd" / "csrc"),
           str(ROOT / "tools" / "raster_core_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(rows):
        text = "".join("%d %d %d %d %d %.9g %d %d %.9g %d %d %.9g\n" % tuple(row) for row in rows)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        out = np.array(r.stdout.split(), dtype=np.int64).reshape(-1, 10)
        assert len(out) == len(rows)
        return out
    return run


def test_setup_of_every_case_is_the_headers(core_check):
    """every triangle of every view of every case: tri_setup_v of csrc/raster_core.h, run on the CPU, against the mirror setup().  For a
    near-plane straddler set-up stores area2 = 1 (nothing reads it) where the mirror keeps the integer area, and the mirror does not judge
    its facing: area2 is held to 1 there, `culled` compared on the other triangles only."""
    rows, mirrors = [], []
    for c in rc.CASES:
        for view in range(c.Hn):
            xi, yi, zc = rc.projected(c, view)
            z32 = zc.astype(np.float32).astype(np.float64)
            head = np.broadcast_to(np.array([c.W, c.H, c.cull], np.float64), (len(xi), 3))
            rows.append(np.concatenate([head] + [np.stack([xi[:, k], yi[:, k], z32[:, k]], 1) for k in range(3)], 1))
            mirrors.append((c, view, rc.setup(xi, yi, zc, c.W, c.H, c.cull)))
    got = core_check(np.concatenate(rows))
    at = 0
    for c, view, s in mirrors:
        g = got[at:at + len(s.ok)]
        at += len(s.ok)
        where = (c.name, view)
        assert np.array_equal(g[:, 0], s.ok) and np.array_equal(g[:, 1], s.strad) and np.array_equal(g[:, 2], s.swapped), where
        assert np.array_equal(g[:, 3], np.where(s.strad, 1, s.area2)), where
        assert np.array_equal(g[:, 4:8], s.bbox) and np.array_equal(g[:, 8], s.small), where
        plain = ~s.strad
        assert np.array_equal((g[:, 0] & g[:, 9] & c.cull)[plain], s.culled[plain]), where
    assert at == len(got)


# ---- the ledger -------------------------------------------------------------------------------------------------------------------------------
def _fuzz_scenes():
    """the twelve rasteriser scenes of tests/test_gpu_fuzz.py (6 vertex-coloured soups, 6 textured ones), their geometry regenerated by the
    same draws: (name, verts, faces, poses, scale, fx, fy, W, H, cull)"""
    from tests import test_gpu_fuzz as fz
    for case in range(6):
        rng = fz._rng("raster", case)
        nv, nf = int(rng.integers(3, 400)), int(rng.integers(1, 900))
        v = rng.standard_normal((nv, 3)).astype(np.float32)
        v /= np.abs(v).max()
        if rng.integers(0, 2):
            v[:, int(rng.integers(0, 3))] *= 0.02
        f = rng.integers(0, nv, size=(nf, 3)).astype(np.int32)
        rng.integers(0, 256, size=(nv, 3), dtype=np.uint8)
        n = int(rng.integers(1, 7))
        poses = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
        poses[:, :3, :3] = fo.generate_rotations(max(n, 2))[:n]
        poses[:, :3, 3] = np.stack([rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n), rng.choice([0.12, 0.3, 0.8, 1.5], n)], 1)
        W, H = int(rng.integers(16, 560)), int(rng.integers(16, 560))
        fx = float(rng.uniform(200, 900))
        scale = float(rng.choice([0.1, 0.25, 0.6]))
        yield f"fuzz-raster-{case}", v, f, poses, scale, fx, fx, W, H, 0
    for case in range(6):
        rng = fz._rng("rastex", case)
        nv, nf = int(rng.integers(3, 200)), int(rng.integers(1, 400))
        v = rng.standard_normal((nv, 3)).astype(np.float32)
        v /= np.abs(v).max()
        f = rng.integers(0, nv, size=(nf, 3)).astype(np.int32)
        rng.standard_normal((nf, 3, 2)); rng.choice([0.3, 1.0, 4.0])
        th, tw = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        rng.integers(0, 256, size=(th, tw, 3), dtype=np.uint8)
        if not rng.integers(0, 2):
            rng.uniform(0.1, 1.0, 3)
        _, _, cull = int(rng.integers(0, 2)), int(rng.integers(0, 2)), int(rng.integers(0, 2))
        rng.choice([1.0, 2.0, 5.0])
        n = int(rng.integers(1, 5))
        poses = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
        poses[:, :3, :3] = fo.generate_rotations(max(n, 2))[:n]
        poses[:, :3, 3] = np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.choice([0.15, 0.5, 1.2], n)], 1)
        W, H = int(rng.integers(16, 540)), int(rng.integers(16, 540))
        fx, fy = float(rng.uniform(200, 900)), float(rng.uniform(200, 900))
        yield f"fuzz-rastex-{case}", v, f, poses, 0.25, fx, fy, W, H, cull


def test_ledger_of_labels_and_cases():
    """printed with -s: label -> the constructed cases that reach it (* = claimed), then what the fixed-seed random soups reach — for
    information; the gate is that every label has a constructed case"""
    reach = {}
    for c in rc.CASES:
        for label in rc.classify(c):
            reach.setdefault(label, []).append(c.name + ("*" if label in c.claims else ""))
    fuzz = {}
    for name, v, f, poses, scale, fx, fy, W, H, cull in _fuzz_scenes():
        xy, z = fo.project_vertices(v, poses, scale, fx, fy, W / 2, H / 2)
        labels = set()
        for mode in (1, 0):
            labels |= rc.launch_labels(W, H, len(f), len(poses), mode)
        for view in range(len(poses)):
            s = rc.setup(xy[view][f, 0], xy[view][f, 1], z[view][f], W, H, cull)
            labels |= rc.classify_setup(s, (1, 0), len(f), len(poses), cover=rc.coverage_info(s))
        for label in labels:
            fuzz.setdefault(label, []).append(name.replace("fuzz-", ""))
    print()
    for label in rc.LABELS:
        print(f"{label:24s} {', '.join(reach.get(label, [])) or '-'}")
        print(f"{'':24s}   random soups: {', '.join(fuzz.get(label, [])) or 'none'}")
    missing = [label for label in rc.LABELS if not any(n.endswith('*') for n in reach.get(label, []))]
    assert not missing, missing
