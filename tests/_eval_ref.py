"""Plain numpy restatement of the pose-error operations of csrc/eval.hip, for the tests only (DESIGN.md "Scoring").

Nothing here is fast or clever: every function is the formula written out in float64 (with float32 exactly where the toolkit's
numpy code rounds to float32).  tests/test_eval_ref_cpu.py pins it to the fixtures the reference's own functions produced before any
GPU test trusts it.

    chamfer_ref(X, Y)                 mean_y min_x |x - y| + mean_x min_y |x - y|, full distance matrix in float64
    pose_points / project_points      s_e first, then R p + t; P = K [R|t], P [p;1], then the divide
    centred_r                         the r of the chamfer contract |e - e_ref| <= 2e-6 (r + e_ref)
    depth_counts_ref                  the integer pixel counts behind cus and vsd
"""
import numpy as np

CHAMFER_REL = 2e-6


# ---- clouds ------------------------------------------------------------------------------------------------------------------------
def pose_points(p, s, R, t):
    """[n,3] model points -> camera frame: scaled by s first, then rotated and translated"""
    p = np.asarray(p, np.float64) * float(s)
    return (np.asarray(R, np.float64).reshape(3, 3) @ p.T + np.asarray(t, np.float64).reshape(3, 1)).T


def project_points(p, s, R, t, K):
    """[n,3] model points -> [n,2] pixels through the 3x4 matrix K [R|t] and the perspective divide"""
    p = np.asarray(p, np.float64) * float(s)
    P = np.asarray(K, np.float64).reshape(3, 3) @ np.hstack([np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3, 1)])
    q = P @ np.vstack([p.T, np.ones((1, p.shape[0]))])
    return (q[:2] / q[2:3]).T


def chamfer_ref(X, Y, rows=256):
    """brute force: every |x - y| of X [n,d] against Y [m,d] in float64, `rows` rows of the matrix at a time"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    assert X.ndim == 2 and Y.ndim == 2 and X.shape[1] == Y.shape[1] and X.shape[0] > 0 and Y.shape[0] > 0
    best_y = np.full(Y.shape[0], np.inf)          # squared distance of every y to its nearest x
    sum_x = 0.0
    for a in range(0, X.shape[0], rows):
        diff = X[a:a + rows, None, :] - Y[None, :, :]
        d2 = (diff * diff).sum(-1)
        sum_x += float(np.sqrt(d2.min(1)).sum())
        best_y = np.minimum(best_y, d2.min(0))
    return float(np.sqrt(best_y).mean() + sum_x / X.shape[0])


def chamfer_pair_ref(pe, pg, s, Re, te, Rg, tg, K=None):
    """chamfer (K None) or chamfer_proj of one estimate x ground-truth pair from the model-frame clouds"""
    if K is None:
        return chamfer_ref(pose_points(pe, s, Re, te), pose_points(pg, 1.0, Rg, tg))
    return chamfer_ref(project_points(pe, s, Re, te, K), project_points(pg, 1.0, Rg, tg, K))


def _project(K, R, t, p):
    q = (K @ (R @ p.T + np.asarray(t).reshape(3, 1))).T
    return q[:, :2] / q[:, 2:3]


def centred_r(pe, pg, s, Re, te, Rg, tg, K=None):
    """largest absolute coordinate of the two posed (projected) clouds about the posed (projected) GT centroid"""
    c = pg.mean(0, keepdims=True)
    if K is None:
        X, Y, o = (Re @ (pe * s).T).T + te, (Rg @ pg.T).T + tg, (Rg @ c.T).T + tg
    else:
        X, Y, o = _project(K, Re, te, pe * s), _project(K, Rg, tg, pg), _project(K, Rg, tg, c)
    return float(max(np.abs(X - o).max(), np.abs(Y - o).max()))


# ---- depth images ------------------------------------------------------------------------------------------------------------------
def dist_image(depth, K):
    """depth (z) image -> distance-from-the-camera-centre image, float64: sqrt((u z)^2 + (v z)^2 + z^2) with u = (x - cx) / fx,
    v = (y - cy) / fy"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    H, W = depth.shape
    u = (np.arange(W, dtype=np.float64) - K[0, 2]) / K[0, 0]
    v = (np.arange(H, dtype=np.float64) - K[1, 2]) / K[1, 1]
    z = depth.astype(np.float64)
    a, b = u[None, :] * z, v[:, None] * z
    return np.sqrt(a * a + b * b + z * z)


def depth_counts_ref(d_est, d_gt, d_test=None, K=None, delta=None, taus=None, divisor=1.0):
    """(inter, union, visib_inter, visib_union, cost counts [n_tau]) of one pair of rendered float32 depth images [H,W].

    inter / union: pixels where both / either render is > 0 (cus).  With a test depth image (vsd, visibility mode bop19):
      * a render is visible where its distance image, cast to float32, minus the test distance image, cast to float32, is <= delta
        compared as float32, or where the test distance is 0 (missing depth counts as visible); and only where the render is > 0;
      * the estimate is also visible wherever the ground truth is visible and the estimate is > 0;
      * on the pixels visible in both, |dist_gt - dist_est| / divisor >= tau in float64 is a cost-1 pixel of that tau.
    Without d_test the last three are 0, 0 and an empty array."""
    d_est, d_gt = np.asarray(d_est), np.asarray(d_gt)
    assert d_est.dtype == np.float32 and d_gt.dtype == np.float32 and d_est.shape == d_gt.shape and d_est.ndim == 2
    me, mg = d_est > 0, d_gt > 0
    inter, union = int((me & mg).sum()), int((me | mg).sum())
    if d_test is None:
        return inter, union, 0, 0, np.zeros(0, np.int64)
    d_test = np.asarray(d_test)
    assert d_test.dtype == np.float32 and d_test.shape == d_est.shape
    dist_t, dist_g, dist_e = dist_image(d_test, K), dist_image(d_gt, K), dist_image(d_est, K)
    ft, fg, fe = dist_t.astype(np.float32), dist_g.astype(np.float32), dist_e.astype(np.float32)
    tol = np.float32(delta)
    missing = dist_t == 0
    vis_g = (((fg - ft) <= tol) | missing) & (dist_g > 0)
    vis_e = (((fe - ft) <= tol) | missing) & (dist_e > 0)
    vis_e = vis_e | (vis_g & (dist_e > 0))
    both = vis_g & vis_e
    dd = np.abs(dist_g[both] - dist_e[both]) / np.float64(divisor)
    costs = np.array([int((dd >= np.float64(t)).sum()) for t in np.asarray(taus, np.float64).reshape(-1)], np.int64)
    return inter, union, int(both.sum()), int((vis_g | vis_e).sum()), costs


def depth_counts_row(d_est, d_gt, d_test=None, K=None, delta=None, taus=None, divisor=1.0):
    """depth_counts_ref as one int64 row [4 + n_tau], the layout of ops.depth_compare"""
    i, u, vi, vu, c = depth_counts_ref(d_est, d_gt, d_test, K, delta, taus, divisor)
    return np.concatenate([[i, u, vi, vu], c]).astype(np.int64)


def cus_ref(inter, union):
    return 1.0 - inter / float(union) if union > 0 else 1.0


def vsd_ref(visib_inter, visib_union, costs):
    if visib_union == 0:
        return [1.0] * len(costs)
    return [(int(c) + (int(visib_union) - int(visib_inter))) / float(int(visib_union)) for c in costs]
