"""numpy fp64 restatements for the TrackingRefiner kernels (csrc/refine.hip) and the problem sets the CPU and GPU tests share.

`compute_3d_points` restates tracking_refiner.py:102-130 twice: `order="elementwise"` with the operation order include/freepose_hip.h
documents for fp_patch_points, `order="matmul"` with `@` as the reference writes it.  `epnp` restates EPnP once, with numpy.linalg.eigh,
lstsq and svd in place of the kernel's Jacobi solvers and Householder least squares."""
from __future__ import annotations

import math
import struct
import subprocess
from collections import defaultdict

import numpy as np

PATCH = 14


# ---- _compute_3d_points -------------------------------------------------------------------------------------------------------------------
def project(samples, T, K, order="elementwise"):
    s = np.asarray(samples, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64).reshape(4, 4)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    if order == "matmul":
        homogeneous = np.concatenate([s, np.ones((len(s), 1))], axis=1)
        cam = (homogeneous @ T.T)[:, :3]                 # one BLAS product for the pose, one for the intrinsics, as the reference does
        proj = cam @ K.T
    else:
        x, y, z = s[:, 0], s[:, 1], s[:, 2]
        cam = np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)
        proj = np.stack([(K[r, 0] * cam[:, 0] + K[r, 1] * cam[:, 1]) + K[r, 2] * cam[:, 2] for r in range(3)], 1)
    with np.errstate(all="ignore"):
        uv = proj[:, :2] / proj[:, 2:]
    return cam, uv


def chosen_samples(samples, T, K, cells, patch=PATCH, order="elementwise"):
    """index of the sample chosen for every query cell (-1: no sample projects into it) and the members' count per cell"""
    cam, uv = project(samples, T, K, order)
    with np.errstate(all="ignore"):
        local = uv / patch
        fl = np.floor(local)
        d2 = np.square(local - fl - 0.5).sum(1)
    members = defaultdict(list)
    for i in np.nonzero(np.isfinite(uv).all(1))[0]:
        members[(fl[i, 0], fl[i, 1])].append(int(i))
    out, counts = [], []
    for c in np.asarray(cells).reshape(-1, 2):
        idx = np.array(members.get((float(c[0]), float(c[1])), []), dtype=np.int64)
        counts.append(len(idx))
        if not len(idx):
            out.append(-1)
            continue
        closest = np.argsort(d2[idx], kind="stable")[:int(math.ceil(len(idx) * 0.25))]      # (d2, sample index): idx is ascending
        out.append(int(idx[closest[np.argmin(cam[idx[closest], 2])]]))                       # first minimum = (Zc, d2, sample index)
    return np.array(out, dtype=np.int32), np.array(counts)


def compute_3d_points(samples, cells, K, T, patch=PATCH, order="elementwise"):
    idx, _ = chosen_samples(samples, T, K, cells, patch, order)
    s = np.asarray(samples, dtype=np.float64)
    return np.stack([s[i] if i >= 0 else np.zeros(3) for i in idx])


def cell_lists(samples, T, K, patch=PATCH):
    """occupied cells by member count: {(x, y): m}"""
    _, uv = project(samples, T, K)
    ok = np.isfinite(uv).all(1)
    cells, counts = np.unique(np.floor(uv[ok] / patch).astype(np.int64), axis=0, return_counts=True)
    return {(int(c[0]), int(c[1])): int(m) for c, m in zip(cells, counts)}


# ---- EPnP ---------------------------------------------------------------------------------------------------------------------------------
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
BETA_COLS = [[0, 1, 3, 6], [0, 1, 2], [0, 1, 2, 3, 4]]


def _betas_init(L, rho, which):
    x = np.linalg.lstsq(L[:, BETA_COLS[which]], rho, rcond=None)[0]
    be = np.zeros(4)
    if which == 0:
        s = -1.0 if x[0] < 0 else 1.0
        be[0] = math.sqrt(s * x[0])
        be[1:] = s * x[1:] / be[0] if be[0] > 0 else 0.0
        return be
    if x[0] < 0:
        be[0], be[1] = math.sqrt(-x[0]), (math.sqrt(-x[2]) if x[2] < 0 else 0.0)
    else:
        be[0], be[1] = math.sqrt(x[0]), (math.sqrt(x[2]) if x[2] > 0 else 0.0)
    if x[1] < 0:
        be[0] = -be[0]
    if which == 2 and be[0] != 0:
        be[2] = x[3] / be[0]
    return be


def _gauss_newton(L, rho, be, steps=5):
    be = be.copy()
    for _ in range(steps):
        b0, b1, b2, b3 = be
        A = np.stack([2 * L[:, 0] * b0 + L[:, 1] * b1 + L[:, 3] * b2 + L[:, 6] * b3,
                      L[:, 1] * b0 + 2 * L[:, 2] * b1 + L[:, 4] * b2 + L[:, 7] * b3,
                      L[:, 3] * b0 + L[:, 4] * b1 + 2 * L[:, 5] * b2 + L[:, 8] * b3,
                      L[:, 6] * b0 + L[:, 7] * b1 + L[:, 8] * b2 + 2 * L[:, 9] * b3], 1)
        quad = np.array([b0 * b0, b0 * b1, b1 * b1, b0 * b2, b1 * b2, b2 * b2, b0 * b3, b1 * b3, b2 * b3, b3 * b3])
        be = be + np.linalg.lstsq(A, rho - L @ quad, rcond=None)[0]
    return be


def epnp(pts3d, pts2d, K, vis=None):
    """-> dict(out=[16] as fp_pnp_epnp writes it, errs=[3] mean reprojection error of the three candidates)"""
    p3 = np.asarray(pts3d, dtype=np.float64)
    p2 = np.asarray(pts2d, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    use = np.ones(len(p3), bool) if vis is None else np.asarray(vis).astype(bool)
    n = int(use.sum())
    out = np.full(16, np.nan)
    out[13], out[15] = n, 0.0

    def bad(status):
        out[14] = status
        return dict(out=out, errs=np.full(3, np.nan), cands=[])
    if n < 4:
        return bad(1)
    p3, p2 = p3[use], p2[use]
    mu = p3.mean(0)
    lam, E = np.linalg.eigh((p3 - mu).T @ (p3 - mu))
    lam, E = lam[::-1], E[:, ::-1]
    # the control points depend on the axes' signs, and with noise so does the pose: largest-magnitude component positive (pnp_core.h)
    E = E * np.where(E[np.argmax(np.abs(E), 0), np.arange(3)] < 0, -1.0, 1.0)
    if not (lam[0] > 0 and lam[2] > 1e-12 * lam[0]):
        return bad(2)
    k = np.sqrt(lam / n)
    cw = np.vstack([mu, mu + (E * k).T])
    a123 = (p3 - mu) @ (E / k)
    al = np.hstack([1 - a123.sum(1, keepdims=True), a123])
    x, y = (p2[:, 0] - K[0, 2]) / K[0, 0], (p2[:, 1] - K[1, 2]) / K[1, 1]
    M = np.zeros((2 * n, 12))
    for i in range(4):
        M[0::2, 3 * i], M[0::2, 3 * i + 2] = al[:, i], -al[:, i] * x
        M[1::2, 3 * i + 1], M[1::2, 3 * i + 2] = al[:, i], -al[:, i] * y
    _, V = np.linalg.eigh(M.T @ M)
    v = V[:, :4].T.reshape(4, 4, 3)                                   # v[k, i] = control point i of null vector k, smallest eigenvalue first
    L, rho = np.zeros((6, 10)), np.zeros(6)
    for r, (a, b) in enumerate(PAIRS):
        dv = v[:, a] - v[:, b]
        g = dv @ dv.T
        L[r] = [g[0, 0], 2 * g[0, 1], g[1, 1], 2 * g[0, 2], 2 * g[1, 2], g[2, 2], 2 * g[0, 3], 2 * g[1, 3], 2 * g[2, 3], g[3, 3]]
        rho[r] = ((cw[a] - cw[b]) ** 2).sum()
    cands, errs = [], []
    for which in range(3):
        be = _gauss_newton(L, rho, _betas_init(L, rho, which))
        cc = np.tensordot(be, v, 1)
        pc = al @ cc
        if pc[:, 2].mean() < 0:
            pc = -pc
        pc0 = pc.mean(0)
        U, _, Vt = np.linalg.svd((pc - pc0).T @ (p3 - mu))
        R = U @ np.diag([1, 1, np.sign(np.linalg.det(U @ Vt))]) @ Vt
        t = pc0 - R @ mu
        cam = p3 @ R.T + t
        with np.errstate(all="ignore"):
            ue = K[0, 2] + K[0, 0] * cam[:, 0] / cam[:, 2]
            ve = K[1, 2] + K[1, 1] * cam[:, 1] / cam[:, 2]
            errs.append(np.sqrt((p2[:, 0] - ue) ** 2 + (p2[:, 1] - ve) ** 2).mean())
        cands.append((R, t))
    errs = np.array(errs)
    best = 0
    for c in (1, 2):
        if errs[c] < errs[best] or (np.isnan(errs[best]) and not np.isnan(errs[c])):
            best = c
    out[:9], out[9:12], out[12], out[14] = cands[best][0].ravel(), cands[best][1], errs[best], 0
    return dict(out=out, errs=errs, cands=[np.concatenate([R.ravel(), t]) for R, t in cands])


def rot_angle(Ra, Rb):
    """geodesic angle between two rotations (radians), accurate near 0"""
    D = np.asarray(Ra).reshape(3, 3) @ np.asarray(Rb).reshape(3, 3).T
    s = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return math.atan2(s, 0.5 * (np.trace(D) - 1.0))


def pose_diff(a, b):
    """(rotation angle, relative translation difference) between two [16] outputs"""
    return rot_angle(a[:9], b[:9]), float(np.linalg.norm(a[9:12] - b[9:12]) / np.linalg.norm(b[9:12]))


def rodrigues(axis, angle):
    k = np.asarray(axis, dtype=np.float64)
    k = k / np.linalg.norm(k)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


# ---- problems ------------------------------------------------------------------------------------------------------------------------------
K_TEST = np.array([[1066.778, 0, 312.9869], [0, 1067.487, 241.3109], [0, 0, 1]])
SIZES = (4, 5, 6, 63, 64, 65, 257, 1369)
# Noisy problems and near-ties among the three beta candidates.  With N >= 6 and sigma = 0.5 px, five Gauss-Newton steps take all
# three initialisations to the SAME minimum: their mean reprojection errors agree to 1e-8 relative or better (over 300 seeds per
# size the largest gap was 0.44 % at N = 6, 7e-9 at 63, 1.9e-8 at 64, 5.9e-9 at 65, 1.3e-9 at 257, 2e-13 at 1369), so which
# candidate wins is decided in the last places.  A flipped choice is harmless exactly when the three candidates are one pose: the
# seeds below are those at which the restatement's candidates agree to 1e-13 (rotation angle and relative translation), below the
# comparisons' bounds.  tests/test_refiner_track_cpu.py asserts for every row with >= 6 used points: the errors are more than 1 %
# apart, or the candidates' spread is at most CANDIDATE_SPREAD_MAX.
NOISY_SEEDS = {4: 0, 5: 0, 6: 0, 63: 1, 64: 0, 65: 0, 257: 0, 1369: 0}
CANDIDATE_SPREAD_MAX = 1e-13
# largest host-check-vs-restatement difference over the N >= 6 problems (rotation angle in rad, relative translation), measured by
# test_refiner_track_cpu.py on x86-64 and recorded in profiles/refiner_track.md; the GPU test allows the device 100 x this
CPU_HOST_VS_REF = (2e-14, 6e-15)          # measured 1.83e-14 rad, 5.06e-15
SIGMA = 0.5


def problem(N, seed, sigma=0.0, coplanar=False):
    rng = np.random.Generator(np.random.PCG64([N, seed, int(coplanar)]))
    p3 = rng.uniform(-1, 1, (N, 3)) * np.array([0.09, 0.06, 0.12])
    if coplanar:
        p3[:, 2] = 0.0
        p3 = p3 @ rodrigues(rng.standard_normal(3), 0.7).T
    R = rodrigues(rng.standard_normal(3), rng.uniform(0.2, 2.8))
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.08, 0.08), rng.uniform(0.6, 1.2)])
    cam = p3 @ R.T + t
    p2 = np.stack([K_TEST[0, 2] + K_TEST[0, 0] * cam[:, 0] / cam[:, 2], K_TEST[1, 2] + K_TEST[1, 1] * cam[:, 1] / cam[:, 2]], 1)
    if sigma:
        p2 = p2 + sigma * rng.standard_normal(p2.shape)
    return dict(N=N, p3=p3, p2=p2, R=R, t=t, K=K_TEST, vis=None)


def problems():
    """name -> problem: every size noise-free and noisy, then the degenerate ones"""
    out = {}
    for N in SIZES:
        out[f"clean_{N}"] = problem(N, 1)
        out[f"noisy_{N}"] = problem(N, NOISY_SEEDS[N], SIGMA)
    three = problem(64, 2)
    three["vis"] = np.zeros(64, np.uint8)
    three["vis"][[3, 17, 40]] = 1
    out["three_used"] = three
    out["coplanar"] = problem(64, 3, coplanar=True)
    return out


def _project_noisy(p3, R, t, sigma, rng):
    cam = p3 @ R.T + t
    p2 = np.stack([K_TEST[0, 2] + K_TEST[0, 0] * cam[:, 0] / cam[:, 2], K_TEST[1, 2] + K_TEST[1, 1] * cam[:, 1] / cam[:, 2]], 1)
    return p2 + sigma * rng.standard_normal(p2.shape) if sigma else p2


def batches():
    """name -> dict(N, p3 [N,3], p2 [B,N,2], vis u8 [B,N] or None, R [B,3,3], t [B,3], K): the problems as fp_pnp_epnp takes them.
    B = 1: every problem of problems().  B = 3 and B = 12: frames of one point set under different poses with mixed visibility —
    all ones, about half, exactly 4 used, 3 used (status 1), none (status 1) between two valid rows, and a row that sees only the
    coplanar first 10 points (status 2)."""
    out = {}
    for name, p in problems().items():
        out[name] = dict(N=p["N"], p3=p["p3"], p2=p["p2"][None], vis=None if p["vis"] is None else p["vis"][None], R=p["R"][None],
                         t=p["t"][None], K=p["K"])
    for name, N, B, seed in (("mixed_3", 64, 3, 0), ("mixed_12", 257, 12, 2)):
        rng = np.random.Generator(np.random.PCG64([N, B, seed]))
        p3 = rng.uniform(-1, 1, (N, 3)) * np.array([0.09, 0.06, 0.12])
        p3[:10, 2] = 0.02                                                    # the first 10 points share a plane
        R = np.stack([rodrigues(rng.standard_normal(3), rng.uniform(0.2, 2.8)) for _ in range(B)])
        t = np.stack([[rng.uniform(-0.1, 0.1), rng.uniform(-0.08, 0.08), rng.uniform(0.6, 1.2)] for _ in range(B)])
        p2 = np.stack([_project_noisy(p3, R[b], t[b], SIGMA if b % 2 else 0.0, rng) for b in range(B)])
        vis = np.ones((B, N), np.uint8)
        half = (rng.random((B, N)) < 0.5).astype(np.uint8)
        if B == 3:
            vis[1] = 0                                                       # an all-zero row between two valid ones
            vis[2] = half[2]
        else:
            vis[1] = half[1]
            vis[2] = 0; vis[2, [5, 50, 100, 200]] = 1                        # exactly 4 used  # noqa: E702
            vis[3] = 0; vis[3, [7, 70, 170]] = 1                             # 3 used  # noqa: E702
            vis[5] = 0
            vis[6] = half[6]
            vis[8] = 0; vis[8, :10] = 1                                      # coplanar subset  # noqa: E702
            vis[9] = half[9]
            vis[10] = 0; vis[10, [0, 1]] = 1                                 # noqa: E702
        out[name] = dict(N=N, p3=p3, p2=p2, vis=vis, R=R, t=t, K=K_TEST)
    return out


def rows(batch):
    """the single problems of a batch, as problems() shapes them"""
    return [dict(N=batch["N"], p3=batch["p3"], p2=batch["p2"][b], vis=None if batch["vis"] is None else batch["vis"][b],
                 R=batch["R"][b], t=batch["t"][b], K=batch["K"]) for b in range(batch["p2"].shape[0])]


def write_problems(path, probs):
    blob = struct.pack("<i", len(probs))
    for p in probs:
        blob += struct.pack("<2i", p["N"], int(p["vis"] is not None)) + np.asarray(p["K"], "<f8").tobytes()
        blob += np.ascontiguousarray(p["p3"], "<f8").tobytes() + np.ascontiguousarray(p["p2"], "<f8").tobytes()
        if p["vis"] is not None:
            blob += np.asarray(p["vis"], np.uint8).tobytes()
    path.write_bytes(blob)


def run_host_check(exe, tmp_path, probs):
    fin, fout = tmp_path / "pnp_in.bin", tmp_path / "pnp_out.bin"
    write_problems(fin, probs)
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])       # a sanitizer report ends the program with a non-zero status
    return np.frombuffer(fout.read_bytes(), dtype="<f8").reshape(len(probs), 16)
