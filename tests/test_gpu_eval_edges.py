"""Pose-error kernels (csrc/eval.hip) at the shapes and values where kernels of their kind go wrong, against tests/_eval_ref.py: a plain
numpy float64 restatement that tests/test_eval_ref_cpu.py pins to the reference's own outputs on the CPU.

Contract (DESIGN.md "Scoring"):
  * depth compare: every count is integer-equal to the truth; cus / vsd formed from the counts are == the float64 truth;
  * chamfer / chamfer_proj: |e - e_ref| <= 2e-6 (r + e_ref), e_ref brute force in float64 on the CPU, r = the largest absolute centred
    coordinate of the pair; each section prints its worst |diff| / bound;
  * two runs give the same bits; a pair gives the same bits alone, in a batch, in a reversed batch and across split launches.
"""
import time

import numpy as np
import pytest
import torch

from tests import _eval_ref as ref

pytestmark = pytest.mark.gpu

K_CAM = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])
SIZES = (1, 2, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir / "pose_errors.npz")


@pytest.fixture(scope="module")
def edges(golden_dir):
    return np.load(golden_dir / "pose_errors_edges.npz")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def _rot_axis(axis, deg):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


# ======================================================================================================================================
# depth compare
# ======================================================================================================================================
def _offset_view(a, off):
    """device copy of a float32 stack whose base pointer is 4 * off bytes past a 16-byte boundary"""
    flat = torch.zeros(a.size + 4, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    v = flat[off:off + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return v.view(*a.shape)


def test_edge_fixture_counts_on_the_vector_and_the_scalar_path(edges):
    from freepose_amd import evaluation as ev, ops
    taus = edges["taus"]
    for tag in ("S", "L"):
        want = edges[tag + "_counts"]
        for off in (0, 1):
            e, g, t = (_offset_view(edges[tag + k], off) for k in ("_d_est", "_d_gt", "_d_test"))
            B, H, W = e.shape
            vector = (H * W) % 4 == 0 and off == 0
            assert e.data_ptr() % 16 == 4 * off and vector == (tag == "L" and off == 0)
            v = ops.depth_compare(e, g, t, edges[tag + "_img_idx"], edges[tag + "_K"], edges[tag + "_delta"], taus, edges[tag + "_div"]).cpu().numpy()
            print(f"edge fixture {tag} offset {4 * off} B ({'vector' if vector else 'scalar'} loop): counts differ at", np.argwhere(v != want).tolist())
            assert np.array_equal(v, want), (tag, off)
            c = ops.depth_compare(e, g).cpu().numpy()
            assert np.array_equal(c[:, :2], want[:, :2]) and not c[:, 2:].any()
            for b in range(B):
                assert ev.cus_from_counts(c[b, 0], c[b, 1]) == edges[tag + "_cus"][b], (tag, b)
                assert ev.vsd_from_counts(v[b, 2], v[b, 3], v[b, 4:]) == list(edges[tag + "_vsd"][b]), (tag, b)


def _random_stacks(rng, B, H, W, n_img):
    """sparse foregrounds near a test surface, everything quantised like a u16 x 0.1 depth image, ~10 % of the test depth missing"""
    def quant(x):
        return np.round(np.clip(x, 0, 6500.0) * 10.0).astype(np.uint16).astype(np.float32) * np.float32(0.1)
    small = H * W < 64
    d_test = 600.0 + 150.0 * rng.random((n_img, 1, 1)) + 30.0 * rng.random((n_img, H, W))
    d_test[rng.random((n_img, H, W)) < 0.10] = 0.0
    img_idx = np.array([2, 0, 2, 1, 0, 1, 2, 2][:B], np.int32)
    surface = np.where(d_test[img_idx] > 0, d_test[img_idx], 640.0)
    blob = rng.random((B, H, W)) < (0.7 if small else 0.12)
    m_e = blob ^ (rng.random((B, H, W)) < (0.2 if small else 0.03))
    m_g = blob ^ (rng.random((B, H, W)) < (0.2 if small else 0.03))
    d_e = np.where(m_e, surface + rng.normal(size=(B, H, W)) * 18.0, 0.0)
    d_g = np.where(m_g, surface + rng.normal(size=(B, H, W)) * 18.0, 0.0)
    return quant(d_e), quant(d_g), quant(d_test), img_idx


TAUS16 = np.concatenate([np.arange(0.05, 0.51, 0.05), [1.0, 2.0, 5.0, 10.0, 20.0, 50.0]])


@pytest.mark.parametrize("W,H", [(1, 1), (5, 3), (641, 479), (1280, 720), (2048, 2048)])
def test_random_stacks_match_the_float64_restatement(W, H):
    """n_img = 3 with a permuted, repeating img_idx; K, delta and divisor differ per pair; n_tau 1, 10 and 16; the CUS-only call.
    2048 x 2048 has more than 64 x 1024 pixels per pair: the grid-stride loop runs more than once."""
    from freepose_amd import ops
    B, n_img = 4, 3
    rng = np.random.default_rng(1000 + W)
    d_e, d_g, d_t, img_idx = _random_stacks(rng, B, H, W, n_img)
    assert sorted(set(img_idx.tolist())) == [0, 1, 2] and len(img_idx) > 3
    K = np.stack([np.array([[900.0 + 70.0 * b, 0, W / 2 + 1.3 * b], [0, 950.0 - 40.0 * b, H / 2 - 0.7 * b], [0, 0, 1]]) for b in range(B)])
    delta = np.array([15.0, 7.3, 20.0, 10.5])
    div = np.array([1.0, 103.7, 128.0, 61.25])
    t0 = time.time()
    want = np.stack([ref.depth_counts_row(d_e[b], d_g[b], d_t[img_idx[b]], K[b], delta[b], TAUS16, div[b]) for b in range(B)])
    t_ref = time.time() - t0
    e, g, t = (torch.from_numpy(x).cuda() for x in (d_e, d_g, d_t))
    for cols in (np.arange(16), np.arange(10), np.array([3])):
        v = ops.depth_compare(e, g, t, img_idx, K, delta, TAUS16[cols], div).cpu().numpy()
        w = np.concatenate([want[:, :4], want[:, 4 + cols]], 1)
        print(f"{W} x {H}, n_tau {len(cols)}: visible union {w[:, 3].tolist()}, counts differ at {np.argwhere(v != w).tolist()}")
        assert v.shape == w.shape and np.array_equal(v, w), (W, H, len(cols))
        assert np.array_equal(ops.depth_compare(e, g, t, img_idx, K, delta, TAUS16[cols], div).cpu().numpy(), v)
    c = ops.depth_compare(e, g).cpu().numpy()
    assert c.shape == (B, 4) and np.array_equal(c[:, :2], want[:, :2]) and not c[:, 2:].any()
    if H * W >= 64:
        assert (want[:, 2] > 0).all() and (want[:, 3] > want[:, 2]).all() and (want[:, 4] > want[:, -1]).all()   # the cases are not trivial
    print(f"{W} x {H}: CPU restatement {t_ref:.2f} s")


def test_depth_compare_refuses_too_many_taus_and_a_bad_img_idx():
    from freepose_amd import ops
    z = torch.zeros((2, 4, 4), dtype=torch.float32, device="cuda")
    t = torch.zeros((3, 4, 4), dtype=torch.float32, device="cuda")
    K = np.array([[50.0, 0, 2], [0, 50.0, 2], [0, 0, 1]])
    with pytest.raises(ValueError, match=r"depth_compare: 17 taus \(1\.\.16\)"):
        ops.depth_compare(z, z, t, [0, 1], K, 15.0, np.linspace(0.1, 1.0, 17), 1.0)
    with pytest.raises(ValueError, match=r"depth_compare: 0 taus"):
        ops.depth_compare(z, z, t, [0, 1], K, 15.0, [], 1.0)
    for bad in ([0, 3], [-1, 0]):
        with pytest.raises(ValueError, match="img_idx outside the test depth stack"):
            ops.depth_compare(z, z, t, bad, K, 15.0, [0.1], 1.0)
    assert ops.depth_compare(z, z, t, [2, 0], K, 15.0, np.linspace(0.1, 1.0, 16), 1.0).shape == (2, 20)


@pytest.mark.parametrize("W,H", [(8, 6), (7, 5)])
def test_depth_compare_split_into_launches_of_three_pairs(monkeypatch, W, H):
    """EVAL_MAX_PAIRS = 3, B = 8: launches of 3, 3 and 2 pairs; with H W = 35 the chunks start at 420 and 840 bytes"""
    from freepose_amd import ops
    B, n_img = 8, 3
    rng = np.random.default_rng(77 + W)
    d_e, d_g, d_t, img_idx = _random_stacks(rng, B, H, W, n_img)
    K = np.stack([np.array([[60.0 + 3.0 * b, 0, W / 2 + 0.3 * b], [0, 66.0 - 2.0 * b, H / 2 - 0.2 * b], [0, 0, 1]]) for b in range(B)])
    delta = 5.0 + 2.5 * np.arange(B)
    div = np.array([1.0, 103.7, 128.0, 61.25, 1.0, 77.7, 64.0, 90.0])
    want = np.stack([ref.depth_counts_row(d_e[b], d_g[b], d_t[img_idx[b]], K[b], delta[b], TAUS16[:10], div[b]) for b in range(B)])
    e, g, t = (torch.from_numpy(x).cuda() for x in (d_e, d_g, d_t))
    whole = ops.depth_compare(e, g, t, img_idx, K, delta, TAUS16[:10], div).cpu().numpy()
    whole_cus = ops.depth_compare(e, g).cpu().numpy()
    monkeypatch.setattr(ops, "EVAL_MAX_PAIRS", 3)
    split = ops.depth_compare(e, g, t, img_idx, K, delta, TAUS16[:10], div).cpu().numpy()
    split_cus = ops.depth_compare(e, g).cpu().numpy()
    print(f"{W} x {H}: split vs whole differ at {np.argwhere(split != whole).tolist()}, vs truth at {np.argwhere(split != want).tolist()}")
    assert np.array_equal(split, whole) and np.array_equal(split, want)
    assert np.array_equal(split_cus, whole_cus) and np.array_equal(split_cus[:, :2], want[:, :2])
    assert len(set(map(tuple, want.tolist()))) == B            # every pair has its own counts: a launch reading the wrong rows shows


# ======================================================================================================================================
# chamfer / chamfer_proj
# ======================================================================================================================================
class _Cases:
    """pairs of model-frame clouds with poses; runs them through ops.chamfer / chamfer_proj in any order"""

    def __init__(self):
        self.clouds, self.pairs, self.s, self.Re, self.te, self.Rg, self.tg, self.names = [], [], [], [], [], [], [], []

    def cloud(self, p):
        self.clouds.append(np.ascontiguousarray(p, np.float64))
        return len(self.clouds) - 1

    def add(self, ie, ig, s, Re, te, Rg, tg, name=""):
        self.pairs.append((ie, ig)); self.s.append(float(s)); self.Re.append(np.asarray(Re, float)); self.te.append(np.asarray(te, float))
        self.Rg.append(np.asarray(Rg, float)); self.tg.append(np.asarray(tg, float)); self.names.append(name)

    def __len__(self):
        return len(self.pairs)

    def run(self, K=None, order=None):
        from freepose_amd import ops
        o = np.arange(len(self)) if order is None else np.asarray(order)
        a = (self.clouds, np.asarray(self.pairs)[o], np.asarray(self.s)[o], np.stack(self.Re)[o], np.stack(self.te)[o], np.stack(self.Rg)[o],
             np.stack(self.tg)[o])
        out = (ops.chamfer(*a) if K is None else ops.chamfer_proj(*a, K)).cpu().numpy()
        assert out.shape == (len(o),)
        return out

    def truth(self, K=None):
        t0 = time.time()
        refs, rs = [], []
        for (ie, ig), s, Re, te, Rg, tg in zip(self.pairs, self.s, self.Re, self.te, self.Rg, self.tg):
            refs.append(ref.chamfer_pair_ref(self.clouds[ie], self.clouds[ig], s, Re, te, Rg, tg, K))
            rs.append(ref.centred_r(self.clouds[ie], self.clouds[ig], s, Re, te, Rg, tg, K))
        print(f"  CPU float64 brute force of {len(self)} pairs: {time.time() - t0:.1f} s")
        return np.array(refs), np.array(rs)


def _check(section, got, want, r, names=None):
    bound = ref.CHAMFER_REL * (r + want)
    frac = np.abs(got - want) / bound
    i = int(np.argmax(frac))
    print(f"{section}: worst |diff| / bound = {frac[i]:.4f} (pair {i}{' ' + names[i] if names else ''}: got {got[i]!r} ref {want[i]!r} r {r[i]:.4g})")
    bad = np.flatnonzero(~(np.abs(got - want) <= bound))
    assert bad.size == 0, (section, [(int(b), names[b] if names else "", float(got[b]), float(want[b]), float(r[b])) for b in bad[:8]])


def _size_sweep():
    rng = np.random.default_rng(2024)
    sizes = [(s, int(rng.choice(SIZES))) for s in SIZES] + [(int(rng.choice(SIZES)), s) for s in SIZES] + [(1, 4097), (4097, 1), (4097, 4097)]
    c = _Cases()
    for n_e, n_g in sizes:
        shape = rng.normal(size=(max(n_e, n_g), 3)) * [40.0, 25.0, 15.0]
        pe = shape[rng.permutation(len(shape))[:n_e]] / 80.0 + rng.normal(size=(n_e, 3)) * 0.01       # model units, s_e = 80 brings it to mm
        pg = shape[rng.permutation(len(shape))[:n_g]] + rng.normal(size=(n_g, 3)) * 0.5
        Rg = _rot(rng)
        tg = np.array([rng.normal() * 80, rng.normal() * 60, 900 + rng.normal() * 100])
        c.add(c.cloud(pe), c.cloud(pg), 80.0 * (1 + 0.05 * rng.normal()), Rg @ _rot_axis(rng.normal(size=3), 4.0), tg + rng.normal(size=3) * 4, Rg, tg,
              f"{n_e}x{n_g}")
    return c


@pytest.fixture(scope="module")
def sweep():
    c = _size_sweep()
    assert {p for p in map(lambda n: tuple(map(int, n.split("x"))), c.names)} >= {(1, 4097), (4097, 1)}
    assert {int(n.split("x")[0]) for n in c.names} >= set(SIZES) and {int(n.split("x")[1]) for n in c.names} >= set(SIZES)
    return c, {None: c.truth(), "proj": c.truth(K_CAM)}


@pytest.mark.parametrize("proj", [False, True])
def test_size_sweep_in_one_mixed_batch_alone_and_reversed(sweep, proj):
    """n_e, n_g from {1 .. 4097} across the 8-group, 1024-tile and 2048-chunk seams in ONE batch: max_n = 4097, so every shorter pair
    has surplus chunks whose slots must hold 0.0"""
    c, truth = sweep
    K = K_CAM if proj else None
    want, r = truth["proj" if proj else None]
    batch = c.run(K)
    _check(f"size sweep {'chamfer_proj' if proj else 'chamfer'} ({len(c)} pairs, mixed batch)", batch, want, r, c.names)
    assert np.array_equal(_bits(c.run(K)), _bits(batch)), "second run differs"
    rev = c.run(K, np.arange(len(c))[::-1])[::-1]
    assert np.array_equal(_bits(rev), _bits(batch)), ("reversed batch", np.flatnonzero(_bits(rev) != _bits(batch)).tolist())
    alone = np.array([c.run(K, [i])[0] for i in range(len(c))])
    assert np.array_equal(_bits(alone), _bits(batch)), ("pair alone", np.flatnonzero(_bits(alone) != _bits(batch)).tolist())
    alone2 = np.array([c.run(K, [i])[0] for i in range(len(c))])
    assert np.array_equal(_bits(alone2), _bits(alone))


class _CountingLib:
    """the loaded library with fp_chamfer calls recorded: (pairs, workspace points) per launch"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "fp_chamfer":
            return fn

        def spy(ctx, pts, n_pts, table, xf, B, max_n, ws_pts, *rest):
            self.calls.append((int(B), int(ws_pts)))
            return fn(ctx, pts, n_pts, table, xf, B, max_n, ws_pts, *rest)
        return spy


@pytest.mark.parametrize("proj", [False, True])
def test_size_sweep_split_by_workspace_and_by_pair_count(sweep, monkeypatch, proj):
    from freepose_amd import _lib, ops
    c, truth = sweep
    K = K_CAM if proj else None
    want, r = truth["proj" if proj else None]
    whole = c.run(K)
    spy = _CountingLib(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda *a: spy)
    c.run(K)
    assert spy.calls == [(len(c), sum(len(c.clouds[a]) + len(c.clouds[b]) for a, b in c.pairs))]
    # by workspace: 6000 points per launch; 4097 + 4097 (and every 4097 + >= 2047) exceeds it alone and goes in a launch of its own
    spy.calls.clear()
    monkeypatch.setattr(ops, "EVAL_MAX_WS_POINTS", 6000)
    by_ws = c.run(K)
    print("launches by workspace (pairs, points):", spy.calls)
    assert len(spy.calls) >= 3 and sum(b for b, _ in spy.calls) == len(c)
    assert any(b == 1 and w > 6000 for b, w in spy.calls) and all(w <= 6000 or b == 1 for b, w in spy.calls)
    assert np.array_equal(_bits(by_ws), _bits(whole)), np.flatnonzero(_bits(by_ws) != _bits(whole)).tolist()
    assert np.array_equal(_bits(c.run(K)), _bits(whole))
    # by pair count
    spy.calls.clear()
    monkeypatch.setattr(ops, "EVAL_MAX_WS_POINTS", 32 << 20)
    monkeypatch.setattr(ops, "EVAL_MAX_PAIRS", 4)
    by_pairs = c.run(K)
    assert [b for b, _ in spy.calls] == [4] * (len(c) // 4) + ([len(c) % 4] if len(c) % 4 else [])
    assert np.array_equal(_bits(by_pairs), _bits(whole)), np.flatnonzero(_bits(by_pairs) != _bits(whole)).tolist()
    assert np.array_equal(_bits(c.run(K)), _bits(whole))
    _check(f"split launches {'chamfer_proj' if proj else 'chamfer'}", by_pairs, want, r, c.names)


def _planted():
    """query 0's only near target sits at a chosen index of the target cloud (its end, 1023, 1024), the last query's at index 0; every
    other target is >= 100x farther from those two queries"""
    rng = np.random.default_rng(5)
    c, planted = _Cases(), []                              # planted: (side of the target cloud: 0 estimate / 1 ground truth, index)
    R = _rot(rng)
    t = np.array([30.0, -20.0, 2000.0])
    for n_t in (8, 9, 1024, 1025, 2049):
        for at in sorted({n_t - 1, 1023, 1024}):
            if at >= n_t:
                continue
            for n_q in (3, 300):
                Q = rng.normal(size=(n_q, 3)) * 2.0
                Q[0], Q[-1] = [0.0, 300.0, 0.0], [0.0, -300.0, 0.0]
                T = rng.normal(size=(n_t, 3)) * 2.0 + [400.0, 0.0, 0.0]
                T[at], T[0] = Q[0] + [1.0, 0.0, 0.0], Q[-1] + [0.0, 1.0, 0.0]
                d0, dl = np.linalg.norm(T - Q[0], axis=1), np.linalg.norm(T - Q[-1], axis=1)
                assert np.argmin(d0) == at and np.sort(d0)[1] >= 100 * d0[at] and np.argmin(dl) == 0 and np.sort(dl)[1] >= 100 * dl[0]
                iq, it = c.cloud(Q), c.cloud(T)
                c.add(it, iq, 1.0, R, t, R, t, f"targets={n_t} est, nearest at {at}, {n_q} queries")     # direction 0: queries = the GT cloud
                c.add(iq, it, 1.0, R, t, R, t, f"targets={n_t} gt, nearest at {at}, {n_q} queries")      # direction 1: queries = the estimate
                planted += [(0, at), (1, at)]
    return c, planted


@pytest.mark.parametrize("proj", [False, True])
def test_planted_nearest_neighbours_at_the_tail_and_the_tile_seam(proj):
    c, planted = _planted()
    K = K_CAM if proj else None
    want, r = c.truth(K)
    got = c.run(K)
    _check(f"planted neighbours {'chamfer_proj' if proj else 'chamfer'} ({len(c)} pairs)", got, want, r, c.names)
    assert np.array_equal(_bits(c.run(K)), _bits(got))
    if not proj:       # what a dropped target would do: the truth without the planted target is > 100 bounds away
        for i, (side, at) in enumerate(planted):
            cl = [c.clouds[c.pairs[i][0]], c.clouds[c.pairs[i][1]]]
            cl[side] = np.delete(cl[side], at, 0)
            dropped = ref.chamfer_pair_ref(cl[0], cl[1], c.s[i], c.Re[i], c.te[i], c.Rg[i], c.tg[i])
            assert abs(dropped - want[i]) > 100 * ref.CHAMFER_REL * (r[i] + want[i]), (c.names[i], dropped, want[i])


@pytest.mark.parametrize("proj", [False, True])
def test_shared_clouds_same_cloud_on_both_sides_and_duplicated_points(proj):
    rng = np.random.default_rng(8)
    c = _Cases()
    A = c.cloud(rng.normal(size=(700, 3)) * [30.0, 20.0, 10.0])
    Rg, tg = _rot(rng), np.array([40.0, -30.0, 850.0])
    for k in range(4):                                     # one cloud as the estimate of several pairs
        G = c.cloud(c.clouds[A][rng.permutation(700)[:300 + 100 * k]] + rng.normal(size=(300 + 100 * k, 3)) * 0.7)
        c.add(A, G, 1.0 + 0.02 * k, Rg @ _rot_axis([1, 2, 3], 2.0 * k), tg + [k, -k, 3 * k], Rg, tg, f"A as estimate {k}")
    c.add(A, A, 1.0, Rg, tg, Rg, tg, "A against itself, same pose")
    zero = len(c) - 1
    c.add(A, A, 1.0, Rg @ _rot_axis([0, 0, 1], 5.0), tg + [2.0, 1.0, -4.0], Rg, tg, "A against itself, other pose")
    c.add(A, A, 0.9, Rg, tg, Rg, tg, "A against itself, s_e 0.9")
    base = rng.normal(size=(200, 3)) * 25.0
    D = c.cloud(np.concatenate([base, base[:50], base[10:11].repeat(30, 0)]))          # duplicated points inside a cloud
    c.add(D, A, 1.0, Rg, tg + [1.0, 0, 0], Rg, tg, "duplicates in the estimate")
    c.add(A, D, 1.0, Rg, tg, Rg, tg + [0, 1.0, 0], "duplicates in the ground truth")
    c.add(D, D, 1.0, Rg, tg, Rg, tg, "duplicates on both sides, same pose")
    zero2 = len(c) - 1
    K = K_CAM if proj else None
    want, r = c.truth(K)
    got = c.run(K)
    _check(f"shared clouds {'chamfer_proj' if proj else 'chamfer'}", got, want, r, c.names)
    assert got[zero] == 0.0 and got[zero2] == 0.0 and want[zero] == 0.0
    assert np.array_equal(_bits(c.run(K)), _bits(got))
    rev = c.run(K, np.arange(len(c))[::-1])[::-1]
    assert np.array_equal(_bits(rev), _bits(got))


def _centring():
    """the same object and relative pose at 1 m, 100 m and 1 km: r, and with it the bound, stays the object's size"""
    rng = np.random.default_rng(21)
    d = rng.normal(size=(600, 3))
    ball = d / np.linalg.norm(d, axis=1, keepdims=True) * 50.0 * rng.random((600, 1)) ** (1 / 3) * [1.0, 0.7, 0.5]
    est0, gt0 = ball[:350], ball[250:] + rng.normal(size=(350, 3)) * 0.3
    Rg = _rot(rng)
    Re = Rg @ _rot_axis([1.0, -2.0, 0.5], 3.0)
    c, in_front = _Cases(), []
    for tz in (1e3, 1e5, 1e6):
        for s in (1e-3, 1.0, 1e3):
            tg = np.array([0.08 * tz, -0.05 * tz, tz])
            # a. the estimate's cloud in model units (1 / s_e of the object), the ground truth in mm: the posed object stays 50 mm
            c.add(c.cloud(est0 / s), c.cloud(gt0), s, Re, tg + [1.0, 0.5, -1.5], Rg, tg, f"t_z {tz:g} s_e {s:g} object 50 mm")
            in_front.append(True)
            # b. the ground-truth cloud scaled by s_e as well: the posed object itself is 0.05 mm, 50 mm or 50 m
            c.add(c.cloud(est0), c.cloud(gt0 * s), s, Re, tg + np.array([1.0, 0.5, -1.5]) * s, Rg, tg, f"t_z {tz:g} s_e {s:g} object {50 * s:g} mm")
            in_front.append(50.0 * s * 1.1 < tz)           # the 50 m object around t_z = 1 m reaches behind the camera
    return c, np.array(in_front)


def test_centring_keeps_the_bound_relative_to_the_object_far_from_the_camera():
    c, in_front = _centring()
    want, r = c.truth()
    got = c.run()
    _check("centring chamfer (t_z 1e3 1e5 1e6 mm, s_e 1e-3 1 1e3)", got, want, r, c.names)
    small = np.array(["object 50 mm" in n for n in c.names])
    assert (r[small] < 120.0).all(), "r is the object's size, not its distance"
    assert np.array_equal(_bits(c.run()), _bits(got))
    assert int((~in_front).sum()) == 1
    keep = np.flatnonzero(in_front)                        # chamfer_proj: every point in front of the camera
    for i in keep:
        (ie, ig) = c.pairs[i]
        assert ref.pose_points(c.clouds[ie], c.s[i], c.Re[i], c.te[i])[:, 2].min() > 0 and ref.pose_points(c.clouds[ig], 1, c.Rg[i], c.tg[i])[:, 2].min() > 0
    want2, r2 = c.truth(K_CAM)
    got2 = c.run(K_CAM, keep)
    _check("centring chamfer_proj", got2, want2[keep], r2[keep], [c.names[i] for i in keep])
    assert np.array_equal(_bits(c.run(K_CAM, keep)), _bits(got2))


# ======================================================================================================================================
# evaluator
# ======================================================================================================================================
class _M:
    def __init__(self, v, f):
        self.vertices, self.faces = v, f


def _alternating_pairs(gold):
    inf = {"A": _M(gold["mesh_A_v"], gold["mesh_A_f"]), "T": _M(gold["mesh_T_v"], gold["mesh_T_f"])}
    ia = [i for i in range(len(gold["cus"])) if str(gold["pair_inf"][i]) == "A"]
    it = [i for i in range(len(gold["cus"])) if str(gold["pair_inf"][i]) == "T"]
    order = [i for ab in zip(ia, it) for i in ab]          # A, T, A, T, ...
    assert len(order) >= 12 and all(str(gold["pair_inf"][a]) != str(gold["pair_inf"][b]) for a, b in zip(order, order[1:]))
    pairs = [(inf[str(gold["pair_inf"][i])], float(gold["pair_s"][i]), gold["pair_Re"][i], gold["pair_te"][i], int(gold["pair_gt"][i]),
              gold["pair_Rg"][i], gold["pair_tg"][i]) for i in order]
    return order, pairs


def _evaluator(gold, **kw):
    from freepose_amd.evaluation import PoseErrorEvaluator
    ev = PoseErrorEvaluator(int(gold["width"]), int(gold["height"]), **kw)
    return ev.add_gt_model(1, _M(gold["gt_1_v"], gold["gt_1_f"])).add_gt_model(2, _M(gold["gt_2_v"], gold["gt_2_f"]))


def _vsd_kw(gold):
    dt = gold["depth_u16"].astype(np.float32)
    dt *= float(gold["depth_scale"])
    return dict(depth_test=dt, vsd_delta=float(gold["vsd0_delta"]), vsd_taus=list(gold["vsd0_taus"]), vsd_normalized_by_diameter=True,
                diameters={1: float(gold["diameters"][0]), 2: float(gold["diameters"][1])})


def test_evaluator_with_a_mesh_cache_of_one_entry(gold):
    """pairs that alternate between the two inference meshes evict the cached mesh at every switch: same values as the default cache"""
    order, pairs = _alternating_pairs(gold)
    K = gold["K"]
    for max_batch in (64, 3):                              # 3: every chunk of pairs switches meshes and uploads again
        small, big = _evaluator(gold, mesh_cache_size=1, max_batch=max_batch), _evaluator(gold, max_batch=max_batch)
        for key, et in (("cus", "cus"), ("chamfer", "chamfer"), ("chamfer_proj", "chamfer_proj"), ("vsd0", "vsd"), ("re", "re"), ("te", "te")):
            kw = _vsd_kw(gold) if et == "vsd" else {}
            a, b = small.errors(et, pairs, K, **kw), big.errors(et, pairs, K, **kw)
            assert len(small._mesh_cache) <= 1
            if et in ("chamfer", "chamfer_proj"):
                assert np.array_equal(_bits(a), _bits(b)), key
                r = np.array([ref.centred_r(p[0].vertices.astype(np.float64), {1: gold["gt_1_v"], 2: gold["gt_2_v"]}[p[4]].astype(np.float64),
                                            p[1], p[2], p[3], p[5], p[6], K if et == "chamfer_proj" else None) for p in pairs])
                _check(f"evaluator, cache of one, {key}", np.array(a), gold[key][order], r)
            elif et == "vsd":
                assert a == b and a == [list(x) for x in gold[key][order]], key
            else:
                assert a == b and a == list(gold[key][order]), key
            assert small.errors(et, pairs, K, **kw) == a   # and again, now starting from whatever the cache holds


def test_evaluator_takes_one_K_per_pair(gold):
    """errors() accepts K [n,3,3]: pairs under two different cameras in one call equal the same pairs one by one under their own camera,
    chamfer_proj equals the float64 restatement and vsd equals the restatement on this rasteriser's renders"""
    from freepose_amd import ops
    order, pairs = _alternating_pairs(gold)
    order, pairs = order[:8], pairs[:8]
    K2 = gold["K"].copy()
    K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2] = 980.5, 1003.25, 330.0, 228.5
    Ks = np.stack([gold["K"] if i % 3 else K2 for i in range(len(pairs))])
    ev = _evaluator(gold, max_batch=5)
    kw = _vsd_kw(gold)
    for et in ("cus", "vsd", "chamfer_proj"):
        k = kw if et == "vsd" else {}
        batch = ev.errors(et, pairs, Ks, **k)
        single = [ev.errors(et, [p], Ks[i], **k)[0] for i, p in enumerate(pairs)]
        one_cam = ev.errors(et, pairs, gold["K"], **k)
        assert batch == single, et
        assert any(batch[i] != one_cam[i] for i in range(len(pairs)) if i % 3 == 0), "the second camera changes nothing?"
        assert all(batch[i] == one_cam[i] for i in range(len(pairs)) if i % 3), et
    gtv = {1: gold["gt_1_v"], 2: gold["gt_2_v"]}
    got = np.array(ev.errors("chamfer_proj", pairs, Ks))
    want = np.array([ref.chamfer_pair_ref(p[0].vertices.astype(np.float64), gtv[p[4]].astype(np.float64), p[1], p[2], p[3], p[5], p[6], Ks[i])
                     for i, p in enumerate(pairs)])
    r = np.array([ref.centred_r(p[0].vertices.astype(np.float64), gtv[p[4]].astype(np.float64), p[1], p[2], p[3], p[5], p[6], Ks[i])
                  for i, p in enumerate(pairs)])
    _check("evaluator, K per pair, chamfer_proj", got, want, r)
    # vsd / cus under the second camera against the restatement, on renders of this rasteriser
    W, H = int(gold["width"]), int(gold["height"])
    gtm = {1: ops.Mesh(gold["gt_1_v"], gold["gt_1_f"]), 2: ops.Mesh(gold["gt_2_v"], gold["gt_2_f"])}
    vsd, cus = ev.errors("vsd", pairs, Ks, **kw), ev.errors("cus", pairs, Ks)
    for i, p in enumerate(pairs):
        Kp = Ks[i]
        pe, pg = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
        pe[:3, :3], pe[:3, 3], pg[:3, :3], pg[:3, 3] = p[2], np.asarray(p[3]).reshape(3), p[5], np.asarray(p[6]).reshape(3)
        d_e = ops.rasterize(ops.Mesh(p[0].vertices, p[0].faces), torch.from_numpy(pe[None]), p[1], Kp[0, 0], Kp[1, 1], Kp[0, 2], Kp[1, 2], W, H)[1][0]
        d_g = ops.rasterize(gtm[p[4]], torch.from_numpy(pg[None]), 1.0, Kp[0, 0], Kp[1, 1], Kp[0, 2], Kp[1, 2], W, H)[1][0]
        row = ref.depth_counts_row(d_e.cpu().numpy(), d_g.cpu().numpy(), kw["depth_test"], Kp, kw["vsd_delta"], kw["vsd_taus"], kw["diameters"][p[4]])
        assert cus[i] == ref.cus_ref(row[0], row[1]) and vsd[i] == ref.vsd_ref(row[2], row[3], row[4:]), i
