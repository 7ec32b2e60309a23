"""numpy restatement of the built-in point tracker (freepose_amd/csrc/lk_core.h, lk_track.hip) and the seeded synthetic
clips its tests run on.

The pyramid is restated in float32 with the kernel's expression order (numpy never contracts into FMAs), so it must equal the device's
and the host check's bit for bit.  The tracker is restated in float64 on that float32 pyramid, vectorised over points: the same samples,
sums and updates, no early exit; the device and the host check also work in fp64 and differ from it by the order of their sums and the one
rounding of each float32 result they store.

    python -m tests._lk_ref            # prints REF_VS_TRUTH for the CPU cases (A, B, D) and CPU_HOST_VS_REF as measured here

REF_VS_TRUTH["H"] (the rendered mesh clip needs the rasteriser, i.e. a GPU) is printed by tests/test_gpu_lk_tracker.py::test_mesh_clip:
all 24 frames, every query of compute_2d3d_correspondences on planted frame 12.  The planted truth of that clip is defined only where the
point is visible, so H's errors are taken over the rows both the tracker and the truth call visible; its share, like the others, is rows
called visible / non-query rows.
"""
from __future__ import annotations

import numpy as np

EIG_FLOOR = 1e-4                 # lk_core.h FP_LK_EIG_FLOOR
FLAG_FB, FLAG_EIG, FLAG_RESIDUAL, FLAG_OUTSIDE, FLAG_LOST_BEFORE = 1, 2, 4, 8, 16
# thresholds the tests pass explicitly (no test depends on a default of freepose_amd.tracker)
PARAMS = dict(levels=4, radius=7, iters=10, fb_thresh=1.0, min_eig=1.0, max_residual=10.0)

# restatement against the planted truth over the (frame, point) pairs it calls visible, query rows excluded:
# (median error px, 95th percentile px, share of non-query rows called visible); measured by `python -m tests._lk_ref` (A, B, D) and by
# tests/test_gpu_lk_tracker.py::test_mesh_clip (H)
REF_VS_TRUTH = {
    "A": (0.0150, 0.0431, 0.9333),
    "B": (0.0000, 0.0000, 0.9375),
    "D": (0.3195, 1.0730, 0.9094),
    "H": (0.5821, 2.4068, 0.4853),     # 24 frames, 272 queries on frame 12; errors over the rows the tracker and the truth both call visible
}
# largest difference between tools/lk_host_check.cpp (fp64 on the fp32 pyramid in the kernel's order, float32 results) and this restatement over compared points of cases
# A to G: (track px, diagnostics: eigenvalue and residual, |difference| / max(1, |value|)); measured by `python -m tests._lk_ref`
CPU_HOST_VS_REF = (7.7e-6, 6e-8)           # measured 7.63e-06 px, 5.84e-08; recorded rounded up.  These are the one rounding of a stored
#                                            float32: half an ulp at coordinates in [128, 256) and 2^-24 relative; the fp64 sums differ far below that


# ---- pyramid (float32, the kernel's order) --------------------------------------------------------------------------------------------
def grey(frames):
    f = np.asarray(frames).astype(np.int32)
    return ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).astype(np.float32)


def tap5(a, b, c, d, e):
    return (((a + e) + np.float32(4) * (b + d)) + np.float32(6) * c) * np.float32(0.0625)


def down(img):
    """[T,h,w] float32 -> [T,(h+1)//2,(w+1)//2]: rows (along x) first, then columns, replicate border, even pixels"""
    T, h, w = img.shape
    hd, wd = (h + 1) // 2, (w + 1) // 2
    cols = [np.clip(2 * np.arange(wd) + o, 0, w - 1) for o in range(-2, 3)]
    rows = [np.clip(2 * np.arange(hd) + o, 0, h - 1) for o in range(-2, 3)]
    r = tap5(*[img[:, :, c] for c in cols])
    out = tap5(*[r[:, y, :] for y in rows])
    assert out.dtype == np.float32
    return out


def layout(H, W, levels, radius):
    sizes = [(H, W)]
    for _ in range(1, levels):
        h, w = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if min(h, w) < 2 * radius + 1:
            break
        sizes.append((h, w))
    return sizes


def pyramid(frames, levels, radius):
    """list of float32 [T,h_l,w_l]"""
    out = [grey(frames)]
    for _ in layout(frames.shape[1], frames.shape[2], levels, radius)[1:]:
        out.append(down(out[-1]))
    return out


# ---- tracker (float64) -------------------------------------------------------------------------------------------------------------------
def _clamp(v, hi):
    v = np.where(v >= 0.0, v, 0.0)
    return np.where(v > hi, float(hi), v)


def sample(img, x, y):
    h, w = img.shape
    x, y = _clamp(x, w - 1), _clamp(y, h - 1)
    x0, y0 = x.astype(np.int64), y.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    fx, fy = x - x0, y - y0
    a, b, c, d = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    top, bot = a + fx * (b - a), c + fx * (d - c)
    return top + fy * (bot - top)


def _min_eig(gxx, gxy, gyy, npix):
    d = gxx - gyy
    return 0.5 * ((gxx + gyy) - np.sqrt(d * d + 4.0 * (gxy * gxy))) / npix


def lk_run(pyr, ta, tb, p, radius, iters):
    """p [M,2] points of frame ta -> (positions in frame tb [M,2], eigenvalue [M], residual [M])"""
    M = len(p)
    win = 2 * radius + 1
    k = np.arange(win * win)
    dx, dy = (k % win - radius).astype(np.float64)[None], (k // win - radius).astype(np.float64)[None]
    npix = win * win
    g = np.zeros((M, 2))
    for l in range(len(pyr) - 1, -1, -1):
        A, B = pyr[l][ta].astype(np.float64), pyr[l][tb].astype(np.float64)
        pl = p * (1.0 / (1 << l))
        x, y = pl[:, :1] + dx, pl[:, 1:] + dy
        a = sample(A, x, y)
        ix = 0.5 * (sample(A, x + 1.0, y) - sample(A, x - 1.0, y))
        iy = 0.5 * (sample(A, x, y + 1.0) - sample(A, x, y - 1.0))
        gxx, gxy, gyy = (ix * ix).sum(1), (ix * iy).sum(1), (iy * iy).sum(1)
        det = gxx * gyy - gxy * gxy
        eig = _min_eig(gxx, gxy, gyy, npix)
        ok = (det > 0.0) & (eig >= EIG_FLOOR)
        safe = np.where(ok, det, 1.0)
        v = np.zeros((M, 2))
        for _ in range(iters):
            q = pl + (g + v)
            d = a - sample(B, q[:, :1] + dx, q[:, 1:] + dy)
            bx, by = (d * ix).sum(1), (d * iy).sum(1)
            v = v + np.where(ok[:, None], np.stack([(gyy * bx - gxy * by) / safe, (gxx * by - gxy * bx) / safe], 1), 0.0)
        if l == 0:
            q = pl + (g + v)
            res = np.abs(a - sample(B, q[:, :1] + dx, q[:, 1:] + dy)).sum(1) / npix
            return q, eig, res
        g = 2.0 * (g + v)


def track(frames, queries, levels=4, radius=7, iters=10, fb_thresh=1.0, min_eig=1.0, max_residual=10.0, pyr=None):
    """-> dict(tracks f64 [T,N,2], vis bool [T,N], diag f64 [T,N,4], pyr)"""
    frames = np.asarray(frames)
    T, H, W = frames.shape[:3]
    pyr = pyramid(frames, levels, radius) if pyr is None else pyr
    q = np.asarray(queries, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    N = len(q)
    tq = np.clip(q[:, 0].astype(int), 0, T - 1)
    tracks, vis, diag = np.zeros((T, N, 2)), np.zeros((T, N), bool), np.zeros((T, N, 4))

    def inside(p):
        return (p[:, 0] >= 0) & (p[:, 0] <= W - 1) & (p[:, 1] >= 0) & (p[:, 1] <= H - 1)
    idx = np.arange(N)
    tracks[tq, idx] = q[:, 1:]
    vis[tq, idx] = inside(q[:, 1:])
    diag[tq, idx, 3] = np.where(vis[tq, idx], 0, FLAG_OUTSIDE)
    for step in range(1, T):
        for sign in (1, -1):
            src, dst = tq + sign * (step - 1), tq + sign * step
            for s, d in sorted(set(zip(src[(dst >= 0) & (dst < T)].tolist(), dst[(dst >= 0) & (dst < T)].tolist()))):
                sel = np.nonzero((src == s) & (dst == d))[0]
                p = tracks[s, sel]
                f, eig, res = lk_run(pyr, s, d, p, radius, iters)
                back, _, _ = lk_run(pyr, d, s, f, radius, iters)
                fb = np.sqrt(((back - p) ** 2).sum(1))
                flags = (np.where(fb <= fb_thresh, 0, FLAG_FB) | np.where(eig >= min_eig, 0, FLAG_EIG)
                         | np.where(res <= max_residual, 0, FLAG_RESIDUAL) | np.where(inside(f), 0, FLAG_OUTSIDE)
                         | np.where(vis[s, sel], 0, FLAG_LOST_BEFORE))
                tracks[d, sel] = f
                vis[d, sel] = flags == 0
                diag[d, sel] = np.stack([fb, eig, res, flags.astype(np.float64)], 1)
    return dict(tracks=tracks, vis=vis, diag=diag, pyr=pyr, size=(H, W))


# ---- comparing a float32 run with the restatement ------------------------------------------------------------------------------------------
def chain_order(tq, T):
    """per query the frames of its two chains in visiting order (query row excluded)"""
    return [[list(range(t + 1, T)), list(range(t - 1, -1, -1))] for t in tq]


def compared_mask(ref, queries, fb_thresh, min_eig, max_residual, band):
    """[T,N] bool: rows the restatement calls visible whose three deciding quantities — and those of every earlier row of the same chain,
    because loss is sticky — lie further from their thresholds than the band (track px for the distance; for eigenvalue and residual the
    diagnostics band, which is relative to max(1, value): their size grows with the image's contrast).  Query rows are compared when visible."""
    T, N = ref["vis"].shape
    d = ref["diag"]
    clear = (np.abs(d[..., 0] - fb_thresh) > band[0]) & (np.abs(d[..., 1] - min_eig) > band[1] * max(1.0, min_eig)) & (np.abs(d[..., 2] - max_residual) > band[1] * max(1.0, max_residual))
    tq = np.clip(np.asarray(queries, dtype=np.float32)[:, 0].astype(int), 0, T - 1) if N else np.zeros(0, int)
    out = np.zeros((T, N), bool)
    for n, chains in enumerate(chain_order(tq, T)):
        out[tq[n], n] = ref["vis"][tq[n], n]
        for ch in chains:
            ok = True
            for t in ch:
                ok = ok and clear[t, n]
                out[t, n] = ok and ref["vis"][t, n]
    return out


def settled_mask(ref, queries, fb_thresh, min_eig, max_residual, band):
    """[T,N] bool: rows, visible or not, whose verdict cannot depend on rounding: the three deciding quantities and the distance of the
    forward result from the image border — theirs and those of every earlier row of the chain — lie further from their thresholds than
    the band.  Once a chain is lost in both runs it stays lost in both, whatever the positions do afterwards.  Query rows are settled."""
    T, N = ref["vis"].shape
    H, W = ref["size"]
    d, tr = ref["diag"], ref["tracks"]
    border = np.minimum(np.minimum(np.abs(tr[..., 0]), np.abs(tr[..., 0] - (W - 1))), np.minimum(np.abs(tr[..., 1]), np.abs(tr[..., 1] - (H - 1))))
    clear = ((np.abs(d[..., 0] - fb_thresh) > band[0]) & (np.abs(d[..., 1] - min_eig) > band[1] * max(1.0, min_eig))
             & (np.abs(d[..., 2] - max_residual) > band[1] * max(1.0, max_residual)) & (border > band[0]))
    tq = np.clip(np.asarray(queries, dtype=np.float32)[:, 0].astype(int), 0, T - 1) if N else np.zeros(0, int)
    out = np.zeros((T, N), bool)
    for n, chains in enumerate(chain_order(tq, T)):
        out[tq[n], n] = True
        for ch in chains:
            ok = True
            for t in ch:
                ok = ok and clear[t, n]
                out[t, n] = ok
    return out


def band_mask(ref, queries, fb_thresh, min_eig, max_residual, band):
    """[T,N] bool: non-query rows with a deciding quantity inside the band around its threshold"""
    d = ref["diag"]
    inb = (np.abs(d[..., 0] - fb_thresh) <= band[0]) | (np.abs(d[..., 1] - min_eig) <= band[1] * max(1.0, min_eig)) | (np.abs(d[..., 2] - max_residual) <= band[1] * max(1.0, max_residual))
    T, N = ref["vis"].shape
    if N:
        tq = np.clip(np.asarray(queries, dtype=np.float32)[:, 0].astype(int), 0, T - 1)
        inb[tq, np.arange(N)] = False
    return inb


def compare(ref, got_tracks, got_vis, got_diag, queries, p, band):
    """-> dict(track = largest track difference over compared rows, diag = largest relative eigenvalue / residual difference there, flags_equal
    = visibility equal on compared rows, vis_equal_settled = visibility equal on every settled row (invisible ones included), compared_share
    = compared / rows the restatement calls visible, band_share = rows inside the band / all rows)"""
    cm = compared_mask(ref, queries, p["fb_thresh"], p["min_eig"], p["max_residual"], band)
    bm = band_mask(ref, queries, p["fb_thresh"], p["min_eig"], p["max_residual"], band)
    n_vis = int(ref["vis"].sum())
    out = dict(track=0.0, diag=0.0, flags_equal=True, compared_share=1.0 if n_vis == 0 else cm.sum() / n_vis,
               band_share=0.0 if bm.size == 0 else bm.sum() / bm.size, n_compared=int(cm.sum()))
    sm = settled_mask(ref, queries, p["fb_thresh"], p["min_eig"], p["max_residual"], band)
    out["n_settled"] = int(sm.sum())
    out["vis_equal_settled"] = bool((np.asarray(got_vis).astype(bool)[sm] == ref["vis"][sm]).all())
    if cm.any():
        out["track"] = float(np.abs(np.asarray(got_tracks, dtype=np.float64) - ref["tracks"])[cm].max())
        want = ref["diag"][..., 1:3]
        out["diag"] = float((np.abs(np.asarray(got_diag, dtype=np.float64)[..., 1:3] - want) / np.maximum(1.0, np.abs(want)))[cm].max())
        out["flags_equal"] = bool((np.asarray(got_vis).astype(bool)[cm] == ref["vis"][cm]).all())
    return out


def truth_error(tracks, vis, truth, queries, truth_vis=None):
    """(median, 95th percentile, share visible) over non-query rows: the share is rows called visible / non-query rows; the errors are
    taken over the rows called visible (where a truth visibility is given, as for the mesh clip whose truth is undefined on hidden
    points: over the rows both call visible)"""
    T, N = vis.shape
    nq = np.ones((T, N), bool)
    nq[np.asarray(queries)[:, 0].astype(int), np.arange(N)] = False
    sel = np.asarray(vis).astype(bool) & nq
    share = float(sel.sum() / max(nq.sum(), 1))
    if truth_vis is not None:
        sel = sel & np.asarray(truth_vis).astype(bool)
    err = np.sqrt(((np.asarray(tracks, dtype=np.float64) - truth) ** 2).sum(-1))[sel]
    if err.size == 0:
        return 0.0, 0.0, share
    return float(np.median(err)), float(np.percentile(err, 95)), share


# ---- seeded synthetic clips ------------------------------------------------------------------------------------------------------------------
class Texture:
    """sum of 2-D sinusoids with periods between 12 and 48 px, three channels with different mixes, scaled into [20, 235]"""

    def __init__(self, seed, n=6):
        rng = np.random.default_rng(seed)
        period = rng.uniform(12.0, 48.0, (3, n))
        ang = rng.uniform(0.0, 2 * np.pi, (3, n))
        self.kx, self.ky = 2 * np.pi / period * np.cos(ang), 2 * np.pi / period * np.sin(ang)
        self.phase = rng.uniform(0.0, 2 * np.pi, (3, n))
        self.amp = rng.uniform(0.5, 1.0, (3, n))

    def __call__(self, x, y):
        x, y = np.asarray(x, dtype=np.float64)[..., None, None], np.asarray(y, dtype=np.float64)[..., None, None]
        s = (self.amp * np.sin(self.kx * x + self.ky * y + self.phase)).sum(-1) / self.amp.sum(-1)
        return 127.5 + 107.5 * s


class Translation:
    def __init__(self, sx, sy):
        self.s = np.array([sx, sy], dtype=np.float64)

    def fwd(self, k, p):
        return np.asarray(p, dtype=np.float64) + k * self.s

    def inv(self, k, p):
        return np.asarray(p, dtype=np.float64) - k * self.s


class Similarity:
    def __init__(self, deg, zoom, centre):
        self.a, self.z, self.c = np.deg2rad(deg), zoom, np.asarray(centre, dtype=np.float64)

    def _m(self, k):
        c, s = np.cos(k * self.a), np.sin(k * self.a)
        return self.z ** k * np.array([[c, -s], [s, c]])

    def fwd(self, k, p):
        return (np.asarray(p, dtype=np.float64) - self.c) @ self._m(k).T + self.c

    def inv(self, k, p):
        return (np.asarray(p, dtype=np.float64) - self.c) @ np.linalg.inv(self._m(k)).T + self.c


def render(tex, motion, T, H, W, flat=None):
    """frame k shows the texture at motion.inv(k, pixel), quantised to u8; flat = (x0, y0, x1, y1, grey): a constant rectangle of the
    texture's own frame (it moves with it)"""
    ys, xs = np.mgrid[0:H, 0:W]
    pix = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    frames = np.zeros((T, H, W, 3), np.uint8)
    for k in range(T):
        p0 = motion.inv(k, pix)
        v = tex(p0[:, 0], p0[:, 1])
        if flat is not None:
            inr = (p0[:, 0] >= flat[0]) & (p0[:, 0] <= flat[2]) & (p0[:, 1] >= flat[1]) & (p0[:, 1] <= flat[3])
            v[inr] = flat[4]
        frames[k] = np.rint(v).reshape(H, W, 3).astype(np.uint8)
    return frames


def grid_queries(rng, x0, y0, x1, y1, nx, ny, tqs):
    """nx * ny points on a jittered grid inside [x0, x1] x [y0, y1]; query times cycle through tqs in thirds (or len(tqs) parts)"""
    sx, sy = (x1 - x0) / nx, (y1 - y0) / ny
    gx, gy = np.meshgrid(x0 + (np.arange(nx) + 0.5) * sx, y0 + (np.arange(ny) + 0.5) * sy)
    pts = np.stack([gx.ravel(), gy.ravel()], 1) + rng.uniform(-0.25, 0.25, (nx * ny, 2)) * [sx, sy]
    t = np.array(tqs)[(np.arange(nx * ny) * len(tqs)) // (nx * ny)]
    perm = rng.permutation(nx * ny)
    return np.concatenate([t[:, None].astype(np.float64), pts[perm]], 1).astype(np.float32)


def truth_tracks(motion, queries, T):
    q = np.asarray(queries, dtype=np.float64)
    out = np.zeros((T, len(q), 2))
    for n in range(len(q)):
        p0 = motion.inv(int(q[n, 0]), q[n, 1:])
        for k in range(T):
            out[k, n] = motion.fwd(k, p0)
    return out


_CACHE = {}


def case(name):
    """dict(frames u8 [T,H,W,3], queries f32 [N,3], truth f64 [T,N,2], params, ...); built once per process and not to be modified"""
    if name in _CACHE:
        return _CACHE[name]
    p = dict(PARAMS)
    extra = {}
    if name in ("A", "F"):
        H, W, T = 96, 128, 6
        mo = Translation(1.3, -0.7)
        rng = np.random.default_rng(101)
        if name == "A":
            frames = render(Texture(1), mo, T, H, W)
            q = grid_queries(rng, 20, 20, W - 21, H - 21, 15, 10, (0, 5, 2))
        else:
            flat = (34.0, 24.0, 94.0, 84.0, 128.0)                         # in the texture's frame; moves (6.5, -3.5) over the clip
            frames = render(Texture(1), mo, T, H, W, flat=flat)
            qi = grid_queries(rng, 52, 42, 76, 66, 4, 4, (0,))             # >= 18 px inside the rectangle at t_q = 0
            qo = grid_queries(rng, 100, 20, W - 15, H - 21, 2, 5, (0,))    # textured ground, >= 6 px + radius from the rectangle
            q = np.concatenate([qi, qo])
            extra = dict(flat_points=np.arange(len(q)) < len(qi))
    elif name in ("B", "B1"):
        H, W, T = 160, 208, 4
        mo = Translation(11.0, -6.0)
        frames = render(Texture(2), mo, T, H, W)
        q = grid_queries(np.random.default_rng(102), 20, 40, W - 55, H - 21, 8, 6, (0,))
        if name == "B1":
            p["levels"] = 1
    elif name.startswith("C"):
        H, W = 61, 47
        T = 1 if name == "C_T1" else 3
        mo = Translation(0.8, 0.5)
        frames = render(Texture(3), mo, T, H, W)
        n = {"C5": 5, "C1": 1, "C0": 0, "C_T1": 5}[name]
        q = grid_queries(np.random.default_rng(103), 12, 12, W - 13, H - 13, 5, 1, (0, T - 1, T // 2))[:n]
    elif name == "D":
        H, W, T = 128, 128, 6
        mo = Similarity(2.0, 1.01, (63.5, 63.5))
        frames = render(Texture(4), mo, T, H, W)
        q = grid_queries(np.random.default_rng(104), 24, 24, W - 25, H - 25, 8, 8, (0, 5, 3))
    elif name == "E":
        H, W, T = 96, 128, 6
        mo = Translation(1.3, -0.7)
        frames = render(Texture(5), mo, T, H, W)
        block = render(Texture(55), Translation(0.0, 0.0), 1, 40, 40)[0]
        bx, by = 50, 30
        for k in (3, 4):
            frames[k, by:by + 40, bx:bx + 40] = block
        q = grid_queries(np.random.default_rng(105), 20, 24, W - 28, H - 21, 12, 8, (0,))
        extra = dict(block=(bx, by, bx + 39, by + 39))
    elif name == "G":
        H, W, T = 96, 128, 5
        mo = Translation(-9.0, 0.0)
        frames = render(Texture(6), mo, T, H, W)
        rng = np.random.default_rng(106)
        ql = np.stack([np.zeros(8), np.full(8, 20.0), np.linspace(20, H - 21, 8) + rng.uniform(-1, 1, 8)], 1).astype(np.float32)
        qr = grid_queries(rng, 70, 20, W - 21, H - 21, 4, 4, (0,))
        q = np.concatenate([ql, qr])
        extra = dict(left_points=np.arange(len(q)) < len(ql))
    else:
        raise KeyError(name)
    out = dict(name=name, frames=frames, queries=q, truth=truth_tracks(mo, q, T), params=p, T=T, H=H, W=W, **extra)
    _CACHE[name] = out
    return out


def assert_named_expectations(result, tol=0.0):
    """the expectations the cases E, F and G are named for, on result(name) -> (tracks, vis).  E's "points under the block" are the
    points whose whole (2 r + 1)^2 window lies under it at frame 3, a narrowing: a window that straddles the block's edge still holds
    moving texture and may keep its point, so nothing is asserted for those."""
    R = PARAMS["radius"]
    c = case("E")
    tracks, vis = result("E")
    tr = c["truth"]
    x0, y0, x1, y1 = c["block"]
    under = (tr[3, :, 0] >= x0 + R) & (tr[3, :, 0] <= x1 - R) & (tr[3, :, 1] >= y0 + R) & (tr[3, :, 1] <= y1 - R)

    def dist(p):
        return np.hypot(np.maximum(np.maximum(x0 - p[:, 0], p[:, 0] - x1), 0), np.maximum(np.maximum(y0 - p[:, 1], p[:, 1] - y1), 0))
    far = np.all([dist(tr[k]) > 2 * R + 4 for k in range(c["T"])], axis=0)
    assert under.sum() >= 10 and far.sum() >= 5
    assert np.asarray(vis)[:3, under].all() and not np.asarray(vis)[3:, under].any()
    assert np.asarray(vis)[:, far].all()
    assert np.sqrt(((np.asarray(tracks, dtype=np.float64) - tr) ** 2).sum(-1))[:, far].max() < 0.1 + tol
    c = case("F")
    tracks, vis = result("F")
    fp = c["flat_points"]
    assert np.asarray(vis)[0, fp].all() and not np.asarray(vis)[1:, fp].any() and np.isfinite(tracks).all()
    c = case("G")
    tracks, vis = result("G")
    outside = (c["truth"][..., 0] < 0)
    assert outside[:, c["left_points"]].sum() == 2 * c["left_points"].sum() and not outside[:, ~c["left_points"]].any()
    assert not np.asarray(vis)[outside].any() and np.asarray(vis)[:, ~c["left_points"]].all() and np.isfinite(tracks).all()


HOST_CASES = ("A", "B", "C5", "C1", "C0", "C_T1", "D", "E", "F", "G")
_REF = {}


def reference(name):
    """the restatement's result on a case, computed once per process"""
    if name not in _REF:
        c = case(name)
        _REF[name] = track(c["frames"], c["queries"], **c["params"])
    return _REF[name]


# ---- the host check ----------------------------------------------------------------------------------------------------------------------------
def build_host_check(out_dir):
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    exe = Path(out_dir) / "lk_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(root / "freepose_amd" / "csrc"), str(root / "tools" / "lk_host_check.cpp"), "-o", str(exe)], check=True)
    return exe


def run_host_check(exe, c, work_dir):
    """-> dict(pyr list of float32 levels, tracks f32, vis u8, diag f32)"""
    import subprocess
    from pathlib import Path
    p = c["params"]
    T, H, W = c["frames"].shape[:3]
    N = len(c["queries"])
    fin, fout = Path(work_dir) / f"{c['name']}.in", Path(work_dir) / f"{c['name']}.out"
    with open(fin, "wb") as f:
        f.write(np.array([T, H, W, N, p["levels"], p["radius"], p["iters"]], np.int32).tobytes())
        f.write(np.array([p["fb_thresh"], p["min_eig"], p["max_residual"]], np.float32).tobytes())
        f.write(np.ascontiguousarray(c["frames"]).tobytes())
        f.write(np.ascontiguousarray(c["queries"], dtype=np.float32).tobytes())
    subprocess.run([str(exe), str(fin), str(fout)], check=True)
    blob = fout.read_bytes()
    n_levels, total = np.frombuffer(blob, np.int32, 2)
    sizes = layout(H, W, p["levels"], p["radius"])
    assert n_levels == len(sizes) and total == sum(T * h * w for h, w in sizes)
    off = 8
    pyr = []
    for h, w in sizes:
        pyr.append(np.frombuffer(blob, np.float32, T * h * w, off).reshape(T, h, w))
        off += 4 * T * h * w
    tracks = np.frombuffer(blob, np.float32, T * N * 2, off).reshape(T, N, 2)
    off += 4 * T * N * 2
    vis = np.frombuffer(blob, np.uint8, T * N, off).reshape(T, N)
    off += T * N
    diag = np.frombuffer(blob, np.float32, T * N * 4, off).reshape(T, N, 4)
    assert off + 4 * T * N * 4 == len(blob)
    return dict(pyr=pyr, tracks=tracks, vis=vis, diag=diag)


if __name__ == "__main__":
    import tempfile
    for nm in ("A", "B", "D"):
        c, r = case(nm), reference(nm)
        print(f'    "{nm}": (%.4f, %.4f, %.4f),' % truth_error(r["tracks"], r["vis"], c["truth"], c["queries"]))
    with tempfile.TemporaryDirectory() as d:
        exe = build_host_check(d)
        worst = [0.0, 0.0]
        for nm in HOST_CASES:
            c, r = case(nm), reference(nm)
            h = run_host_check(exe, c, d)
            m = compare(r, h["tracks"], h["vis"], h["diag"], c["queries"], c["params"], CPU_HOST_VS_REF)
            print(nm, {k: (round(v, 6) if isinstance(v, float) else v) for k, v in m.items()})
            worst = [max(worst[0], m["track"]), max(worst[1], m["diag"])]
        print("CPU_HOST_VS_REF = (%.3g, %.3g)" % tuple(worst))
