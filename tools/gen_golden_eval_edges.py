"""Writes tests/golden/pose_errors_edges.npz: planted edge pixels for the depth-compare kernel (tests/test_eval_ref_cpu.py,
tests/test_gpu_eval_edges.py).

    python tools/gen_golden_eval_edges.py [path to the reference's bop_toolkit folder]

Runs on the CPU.  Like tools/gen_golden_eval.py every expected value is RETURNED BY THE REFERENCE'S OWN FUNCTIONS: pose_error.cus and
pose_error.vsd are handed a stand-in renderer whose render_object returns a prepared depth array, and the integer counts are taken with
the reference's own mask / distance-image functions.  No meshes: the depth arrays are written by hand so that named pixel classes exist.

Two stacks of pairs, "S" 37 x 23 (H W odd: the kernel's scalar loop) and "L" 64 x 48 (H W % 4 == 0: the 16-byte loop).  Every pair has
its own K with an INTEGER principal point, so that at that one pixel pre_x = pre_y = 0 and distance == depth exactly; that pixel carries
the pair's equality class.  All other pixels cycle through the truth table of (d_est > 0, d_gt > 0, d_test > 0) x {in front of the test
surface, inside the delta band, beyond it}.  `labels` names the class of every pixel; the CPU test asserts that no class is empty.
"""
import sys
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
REF = Path(sys.argv[1]) if len(sys.argv) > 1 else Path("/root/reference/bop_toolkit")
sys.path.insert(0, str(REF))
for missing in ("imageio", "png", "trimesh"):
    try:
        __import__(missing)
    except ImportError:
        sys.modules[missing] = types.ModuleType(missing)

from bop_toolkit_lib import misc, pose_error, visibility  # noqa: E402

F = np.float32
POS = {"front": 0, "band": 1, "beyond": 2}
# offsets (mm, depth) of a render from the test surface.  The distance of a pixel is depth * c with 1 <= c < 1.9 for these
# intrinsics, so front stays negative, band stays within (0, 5 * 1.9] < delta and beyond stays >= 40 > delta
OFFS = {"front": (-40.0, -7.5), "band": (2.5, 5.0), "beyond": (40.0, 80.0)}


def truth_table_classes():
    names = []
    for e in (0, 1):
        for g in (0, 1):
            names.append(f"tt_e{e}_g{g}_t0")
    names.append("tt_e0_g0_t1")
    for p in POS:
        names.append(f"tt_e1:{p}_g0_t1")
        names.append(f"tt_e0_g1:{p}_t1")
    for pe in POS:
        for pg in POS:
            names.append(f"tt_e1:{pe}_g1:{pg}_t1")
    return names


TT = truth_table_classes()
assert len(TT) == 20
EQ = ["delta_eq_est", "delta_below_est", "delta_above_est", "delta_eq_gt", "delta_below_gt", "delta_above_gt",
      "tau_eq_div1", "tau_below_div1", "tau_above_div1", "tau_eq_div_pow2", "tau_below_div_pow2", "tau_above_div_pow2"]
DEGENERATE = ["empty_visible_union", "empty_cus_union"]
CLASSES = TT + EQ + DEGENERATE
POW2_DIAMETER = 128.0
TAUS = np.array([0.25, np.nextafter(0.5, 0.0), 0.5, np.nextafter(0.5, 1.0), 1.0, 3.0, 45.0])


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


class PreparedRenderer:
    """render_object(obj_id, ...) -> {'depth': the array prepared for obj_id}"""

    def __init__(self):
        self.depth = {}

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        return {"depth": self.depth[obj_id]}


def dist_im(depth, K):
    misc.Precomputer.depth_im_shape, misc.Precomputer.K = None, None      # its cache keeps stale pre_Xs when only the shape changes
    return misc.depth_im_to_dist_im_fast(depth, K)


def make_stack(W, H, seed, delta):
    rng = np.random.default_rng(seed)
    kinds = EQ + DEGENERATE
    B = len(kinds)
    d_e, d_g, d_t = (np.zeros((B, H, W), F) for _ in range(3))
    labels = np.zeros((B, H, W), np.uint8)
    Ks, deltas, divs = np.zeros((B, 3, 3)), np.full(B, float(delta)), np.ones(B)
    surf = (np.round(np.array([500.0, 612.53, 733.37, 480.11]) * 10.0).astype(np.uint16).astype(F)) * F(0.1)   # u16 x depth_scale
    for b, kind in enumerate(kinds):
        cx, cy = int(rng.integers(3, W - 3)), int(rng.integers(3, H - 3))
        Ks[b] = [[50.0 + b, 0.0, cx], [0.0, 55.0 - 0.5 * b, cy], [0.0, 0.0, 1.0]]
        if kind.endswith("div_pow2") or (kind.startswith("delta_") and b % 3 == 1):
            divs[b] = POW2_DIAMETER
        elif not kind.endswith("div1") and b % 3 == 2:
            divs[b] = 103.7                                 # a diameter whose division is inexact
        if kind == "empty_cus_union":                       # nothing rendered at all
            d_t[b] = surf[rng.integers(0, 4, (H, W))]
            labels[b] = CLASSES.index(kind)
            continue
        if kind == "empty_visible_union":                   # both renders everywhere, both hidden behind the test surface
            d_t[b] = surf[rng.integers(0, 4, (H, W))]
            d_e[b] = d_t[b] + F(OFFS["beyond"][0])
            d_g[b] = d_t[b] + F(OFFS["beyond"][1])
            labels[b] = CLASSES.index(kind)
            continue
        for y in range(H):
            for x in range(W):
                k = (y * W + x + 7 * b) % len(TT)
                name = TT[k]
                labels[b, y, x] = k
                f = name.split("_")
                has_t = f[3] == "t1"
                t = surf[(x + 2 * y + b) % 4] if has_t else F(0.0)
                d_t[b, y, x] = t
                base = t if has_t else surf[(x + y) % 4]
                v = (x * 3 + y) % 2
                for tag, arr in ((f[1], d_e), (f[2], d_g)):
                    if tag[1] == "0":
                        continue
                    pos = tag.split(":")[1] if ":" in tag else ("front", "band", "beyond")[(x + y) % 3]
                    arr[b, y, x] = F(base + F(OFFS[pos][v]))
        # the principal-point pixel: distance == depth exactly; binary-exact values so that the float32 subtraction is exact too
        T0, dl = F(512.0), F(delta)
        e = g = F(0.0)
        t = T0
        if kind.startswith("delta_"):
            edge = {"eq": F(T0 + dl), "below": down(T0 + dl), "above": up(T0 + dl)}[kind.split("_")[1]]
            e, g = (edge, F(0.0)) if kind.endswith("est") else (F(0.0), edge)
        else:
            div = divs[b]
            gap = F(0.5 * div)                              # |dist_g - dist_e| / div == 0.5 == a tau
            g = F(400.0)
            e = {"eq": F(g + gap), "below": down(g + gap), "above": up(g + gap)}[kind.split("_")[1]]
            if b % 2:
                e, g = g, e
            if b % 4 < 2:
                t = F(0.0)                                  # missing test depth: visible whatever the renders say
        d_e[b, cy, cx], d_g[b, cy, cx], d_t[b, cy, cx] = e, g, t
        labels[b, cy, cx] = CLASSES.index(kind)
    return dict(d_est=d_e, d_gt=d_g, d_test=d_t, labels=labels, K=Ks, delta=deltas, div=divs, kinds=kinds)


def evaluate(st):
    """counts and errors of every pair by the reference's functions; checks that the planted pixels are what their label says"""
    B = len(st["kinds"])
    perm = np.random.default_rng(B).permutation(B)           # pair b reads test image img_idx[b] of the stored stack
    img_idx = np.argsort(perm).astype(np.int32)
    stored_test = st["d_test"][perm]
    assert all(np.array_equal(stored_test[img_idx[b]], st["d_test"][b]) for b in range(B))
    ren = PreparedRenderer()
    counts, cus, vsd = [], [], []
    R, t = np.eye(3), np.zeros((3, 1))
    for b in range(B):
        K, delta, div = st["K"][b], float(st["delta"][b]), float(st["div"][b])
        norm = div != 1.0
        ren.depth[("e", b)], ren.depth[("g", b)] = st["d_est"][b], st["d_gt"][b]
        depth_test = stored_test[img_idx[b]]
        misc.Precomputer.depth_im_shape, misc.Precomputer.K = None, None
        cus.append(pose_error.cus(R, t, R, t, K, ren, ("e", b), ("g", b)))
        misc.Precomputer.depth_im_shape, misc.Precomputer.K = None, None
        vsd.append(pose_error.vsd(R, t, R, t, depth_test, K, delta, list(TAUS), norm, div, ren, ("e", b), ("g", b), "step"))
        dist_t, dist_g, dist_e = (dist_im(d, K) for d in (depth_test, st["d_gt"][b], st["d_est"][b]))
        vg = visibility.estimate_visib_mask_gt(dist_t, dist_g, delta, visib_mode="bop19")
        ve = visibility.estimate_visib_mask_est(dist_t, dist_e, vg, delta, visib_mode="bop19")
        both = vg & ve
        dd = np.abs(dist_g[both] - dist_e[both])
        if norm:
            dd /= div
        me, mg = st["d_est"][b] > 0, st["d_gt"][b] > 0
        counts.append([int((me & mg).sum()), int((me | mg).sum()), int(both.sum()), int((vg | ve).sum())] + [int((dd >= tau).sum()) for tau in TAUS])
        # ---- the labels tell the truth ----
        lab, kind = st["labels"][b], st["kinds"][b]
        cy, cx = int(K[1, 2]), int(K[0, 2])
        for k, name in enumerate(TT):
            m = lab == k
            if not m.any():
                continue
            f = name.split("_")
            assert ((st["d_est"][b][m] > 0) == (f[1][1] == "1")).all() and ((st["d_gt"][b][m] > 0) == (f[2][1] == "1")).all()
            assert ((depth_test[m] > 0) == (f[3] == "t1")).all()
            for tag, dist in ((f[1], dist_e), (f[2], dist_g)):
                if ":" in tag:
                    diff = dist[m].astype(F) - dist_t[m].astype(F)
                    pos = tag.split(":")[1]
                    assert ((diff < 0) if pos == "front" else ((diff > 0) & (diff <= F(delta))) if pos == "band" else (diff > F(delta))).all(), name
        if kind in EQ:
            assert lab[cy, cx] == CLASSES.index(kind) and (lab == CLASSES.index(kind)).sum() == 1
            assert dist_e[cy, cx] == float(st["d_est"][b][cy, cx]) and dist_g[cy, cx] == float(st["d_gt"][b][cy, cx]) and \
                dist_t[cy, cx] == float(depth_test[cy, cx])                                          # distance == depth here
            if kind.startswith("delta_"):
                d = (dist_e if kind.endswith("est") else dist_g)[cy, cx].astype(F) - dist_t[cy, cx].astype(F)
                vis = (ve if kind.endswith("est") else vg)[cy, cx]
                ulp = float(up(512.0 + delta)) - (512.0 + delta)
                want = {"eq": 0.0, "below": -ulp, "above": ulp}[kind.split("_")[1]]
                assert float(d) - delta == want and bool(vis) == (want <= 0), (kind, d, vis)
                assert not (vg if kind.endswith("est") else ve)[cy, cx]
            else:
                q = abs(dist_g[cy, cx] - dist_e[cy, cx]) / div
                assert both[cy, cx] and {"eq": q == 0.5, "below": q < TAUS[1], "above": q > TAUS[3]}[kind.split("_")[1]], (kind, q)
        if kind == "empty_visible_union":
            assert counts[-1][1] == lab.size and counts[-1][3] == 0 and vsd[-1] == [1.0] * len(TAUS)
        if kind == "empty_cus_union":
            assert counts[-1][1] == 0 and cus[-1] == 1.0 and counts[-1][3] == 0
    return stored_test, img_idx, np.array(counts, np.int64), np.array(cus, np.float64), np.array(vsd, np.float64)


def main():
    out = {"taus": TAUS, "class_names": np.array(CLASSES), "pow2_diameter": POW2_DIAMETER}
    for tag, (W, H, seed, delta) in {"S": (37, 23, 1, 15.0), "L": (64, 48, 2, 11.5)}.items():
        st = make_stack(W, H, seed, delta)
        stored_test, img_idx, counts, cus, vsd = evaluate(st)
        present = set(np.unique(st["labels"]).tolist())
        assert present == set(range(len(CLASSES))), (tag, sorted(set(range(len(CLASSES))) - present))
        out.update({f"{tag}_d_est": st["d_est"], f"{tag}_d_gt": st["d_gt"], f"{tag}_d_test": stored_test, f"{tag}_img_idx": img_idx,
                    f"{tag}_K": st["K"], f"{tag}_delta": st["delta"], f"{tag}_div": st["div"], f"{tag}_labels": st["labels"],
                    f"{tag}_counts": counts, f"{tag}_cus": cus, f"{tag}_vsd": vsd})
        print(tag, "counts\n", counts)
    golden = ROOT / "tests" / "golden" / "pose_errors_edges.npz"
    np.savez_compressed(golden, **out)
    size, limit = golden.stat().st_size, (ROOT / "tests" / "golden" / "pose_errors.npz").stat().st_size
    print(f"wrote {golden} ({size} bytes; pose_errors.npz has {limit})")
    assert size <= limit


if __name__ == "__main__":
    main()
