"""Pins tests/_eval_ref.py, the numpy restatement the GPU edge tests compare the kernels with, to what the reference's own functions
returned: the 26 pairs of tests/golden/pose_errors.npz (rendered here with the CPU oracle rasteriser, as tools/gen_golden_eval.py did)
and the planted pixels of tests/golden/pose_errors_edges.npz (tools/gen_golden_eval_edges.py).  No GPU.

Bounds: counts and the float64 errors formed from them are exact (==).  chamfer / chamfer_proj: 1e-9 relative, brute force against the
reference's kd-tree, both in float64 (measured worst gap on the fixture: see the printed figure; about 1e-15)."""
import numpy as np
import pytest

from tests import _eval_ref as ref

CHAMFER_PIN_REL = 1e-9

# every pixel class tools/gen_golden_eval_edges.py plants; written out here so that an edit of the generator cannot drop one unnoticed
TRUTH_TABLE = (["tt_e0_g0_t0", "tt_e0_g1_t0", "tt_e1_g0_t0", "tt_e1_g1_t0", "tt_e0_g0_t1"] +
               [f"tt_e1:{p}_g0_t1" for p in ("front", "band", "beyond")] + [f"tt_e0_g1:{p}_t1" for p in ("front", "band", "beyond")] +
               [f"tt_e1:{a}_g1:{b}_t1" for a in ("front", "band", "beyond") for b in ("front", "band", "beyond")])
DELTA_EDGES = [f"delta_{k}_{side}" for side in ("est", "gt") for k in ("eq", "below", "above")]
TAU_EDGES = [f"tau_{k}_{d}" for d in ("div1", "div_pow2") for k in ("eq", "below", "above")]
DEGENERATE = ["empty_visible_union", "empty_cus_union"]
EDGE_CLASSES = TRUTH_TABLE + DELTA_EDGES + TAU_EDGES + DEGENERATE


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir / "pose_errors.npz")


@pytest.fixture(scope="module")
def edges(golden_dir):
    return np.load(golden_dir / "pose_errors_edges.npz")


def _fixture_clouds(gold, i):
    inf = {"A": gold["mesh_A_v"], "T": gold["mesh_T_v"]}[str(gold["pair_inf"][i])].astype(np.float64)
    gt = {1: gold["gt_1_v"], 2: gold["gt_2_v"]}[int(gold["pair_gt"][i])].astype(np.float64)
    return inf, gt


def test_depth_counts_ref_reproduces_the_fixture_counts(gold):
    from freepose_amd import build
    from oracle import fp_oracle as fo
    build.build_oracle(verbose=False)
    K, W, H = gold["K"], int(gold["width"]), int(gold["height"])
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    inf = {"A": (gold["mesh_A_v"], gold["mesh_A_f"]), "T": (gold["mesh_T_v"], gold["mesh_T_f"])}
    gt = {1: (gold["gt_1_v"], gold["gt_1_f"]), 2: (gold["gt_2_v"], gold["gt_2_f"])}
    d_test = gold["depth_u16"].astype(np.float32)
    d_test *= float(gold["depth_scale"])
    cache = {}

    def render(v, f, s, R, t):
        pose = np.eye(4, dtype=np.float32)
        pose[:3, :3], pose[:3, 3] = R, np.asarray(t).reshape(3)
        key = (v.tobytes(), float(s), pose.tobytes())
        if key not in cache:
            cache[key] = fo.rasterize(v, f, None, pose[None], float(s), fx, fy, cx, cy, W, H)[1][0]
        return cache[key]

    n = len(gold["cus"])
    assert n == 26
    for i in range(n):
        d_e = render(*inf[str(gold["pair_inf"][i])], gold["pair_s"][i], gold["pair_Re"][i], gold["pair_te"][i])
        d_g = render(*gt[int(gold["pair_gt"][i])], 1.0, gold["pair_Rg"][i], gold["pair_tg"][i])
        inter, union, _, _, _ = ref.depth_counts_ref(d_e, d_g)
        assert [inter, union] == list(gold["cus_counts"][i]), i
        assert ref.cus_ref(inter, union) == gold["cus"][i], i
        for cfg in ("vsd0", "vsd1"):
            div = float(gold["diameters"][int(gold["pair_gt"][i]) - 1]) if bool(gold[cfg + "_norm"]) else 1.0
            row = ref.depth_counts_row(d_e, d_g, d_test, K, float(gold[cfg + "_delta"]), gold[cfg + "_taus"], div)
            assert list(row[:2]) == list(gold["cus_counts"][i]) and np.array_equal(row[2:], gold[cfg + "_counts"][i]), (cfg, i, row)
            assert ref.vsd_ref(row[2], row[3], row[4:]) == list(gold[cfg][i]), (cfg, i)


def test_chamfer_ref_reproduces_the_fixture_distances(gold):
    K = gold["K"]
    worst = {"chamfer": 0.0, "chamfer_proj": 0.0}
    for i in range(len(gold["chamfer"])):
        pe, pg = _fixture_clouds(gold, i)
        a = (pe, pg, gold["pair_s"][i], gold["pair_Re"][i], gold["pair_te"][i], gold["pair_Rg"][i], gold["pair_tg"][i])
        for key, got in (("chamfer", ref.chamfer_pair_ref(*a)), ("chamfer_proj", ref.chamfer_pair_ref(*a, K))):
            want = float(gold[key][i])
            if want == 0.0:
                assert got == 0.0, (key, i, got)
                continue
            worst[key] = max(worst[key], abs(got - want) / want)
            assert abs(got - want) <= CHAMFER_PIN_REL * want, (key, i, got, want)
    print("brute force vs kd-tree, worst relative gap:", worst)


def test_edge_fixture_holds_every_planted_class_and_the_ref_reproduces_it(edges):
    names = [str(x) for x in edges["class_names"]]
    assert sorted(names) == sorted(EDGE_CLASSES)
    taus = edges["taus"]
    assert taus[2] == 0.5 and taus[1] == np.nextafter(0.5, 0.0) and taus[3] == np.nextafter(0.5, 1.0)
    for tag, hw in (("S", (23, 37)), ("L", (48, 64))):
        lab = edges[tag + "_labels"]
        assert lab.shape[1:] == hw and edges[tag + "_d_est"].dtype == np.float32
        population = {nm: int((lab == names.index(nm)).sum()) for nm in EDGE_CLASSES}
        print(tag, population)
        assert all(v > 0 for v in population.values()), [k for k, v in population.items() if v == 0]
        B = lab.shape[0]
        idx = edges[tag + "_img_idx"]
        assert sorted(idx.tolist()) == list(range(B)) and idx.tolist() != list(range(B))
        assert len(np.unique(edges[tag + "_K"][:, 0, 2])) > 1 and len(np.unique(edges[tag + "_div"])) >= 3
        for b in range(B):
            K = edges[tag + "_K"][b]
            assert K[0, 2] == int(K[0, 2]) and K[1, 2] == int(K[1, 2])                    # the principal point is a pixel
            row = ref.depth_counts_row(edges[tag + "_d_est"][b], edges[tag + "_d_gt"][b], edges[tag + "_d_test"][idx[b]], K,
                                       edges[tag + "_delta"][b], taus, edges[tag + "_div"][b])
            assert np.array_equal(row, edges[tag + "_counts"][b]), (tag, b, row, edges[tag + "_counts"][b])
            assert ref.cus_ref(row[0], row[1]) == edges[tag + "_cus"][b] and ref.vsd_ref(row[2], row[3], row[4:]) == list(edges[tag + "_vsd"][b])
        # the two degenerate images are what they claim to be
        assert (edges[tag + "_vsd"][B - 2] == 1.0).all() and edges[tag + "_counts"][B - 2][3] == 0 and edges[tag + "_counts"][B - 2][1] > 0
        assert edges[tag + "_cus"][B - 1] == 1.0 and edges[tag + "_counts"][B - 1][1] == 0


def test_the_ref_sees_what_the_planted_pixels_are_for(edges):
    """each comparison the planted pixels guard, flipped in the restatement, changes the counts of the edge fixture: the fixture
    discriminates <= delta from < delta, >= tau from > tau (in float64, not float32), the missing-depth rule and the OR with the
    ground truth's mask"""
    taus = edges["taus"]

    def counts(tag, **kw):
        idx = edges[tag + "_img_idx"]
        return np.stack([_variant_counts(edges[tag + "_d_est"][b], edges[tag + "_d_gt"][b], edges[tag + "_d_test"][idx[b]], edges[tag + "_K"][b],
                                         edges[tag + "_delta"][b], taus, edges[tag + "_div"][b], **kw) for b in range(len(idx))])

    for tag in ("S", "L"):
        assert np.array_equal(counts(tag), edges[tag + "_counts"])
        for kw in (dict(strict_delta=True), dict(strict_tau=True), dict(missing_visible=False), dict(or_gt=False),
                   dict(f32_tau=True)):
            assert not np.array_equal(counts(tag, **kw), edges[tag + "_counts"]), (tag, kw)


def _variant_counts(d_est, d_gt, d_test, K, delta, taus, divisor, strict_delta=False, strict_tau=False,
                    missing_visible=True, or_gt=True, f32_tau=False):
    dist_t, dist_g, dist_e = (ref.dist_image(d, K) for d in (d_test, d_gt, d_est))
    cast = lambda a: a.astype(np.float32)  # noqa: E731
    tol = np.float32(delta)
    inside = (lambda d: d < tol) if strict_delta else (lambda d: d <= tol)
    missing = (dist_t == 0) if missing_visible else np.zeros_like(dist_t, bool)
    vg = (inside(cast(dist_g) - cast(dist_t)) | missing) & (dist_g > 0)
    ve = (inside(cast(dist_e) - cast(dist_t)) | missing) & (dist_e > 0)
    if or_gt:
        ve = ve | (vg & (dist_e > 0))
    both = vg & ve
    dd = np.abs(dist_g[both] - dist_e[both]) / np.float64(divisor)
    if f32_tau:
        dd, taus = dd.astype(np.float32), np.asarray(taus).astype(np.float32)
    cost = [int(((dd > t) if strict_tau else (dd >= t)).sum()) for t in taus]
    return np.array([int(((d_est > 0) & (d_gt > 0)).sum()), int(((d_est > 0) | (d_gt > 0)).sum()), int(both.sum()), int((vg | ve).sum())] + cost)
