"""Depth-map-scale fixtures shared by tests/test_scale_host_cpu.py (reference against the production host function) and
tests/test_gpu_scale.py (device against the reference).  Shapes: 70 x 90 and 97 x 131 span 3 x 3 (4 x 5) of the kernels' 32 x 32 tiles
and are no multiple of the tile or the wave; one 480 x 640 case with 5 proposals.

A case is a dict: depth [H,W] f64, K [3,3], masks [n,H,W] bool, kwargs of the call, and flags
  scale     the scatter matrix of every mask's kept points has eigenvalues apart by a ratio >= 2 (asserted by the test on the host), so the
            relative difference of the scale measures arithmetic, not conditioning
  host_tie  there are ties in |z - median|: where they straddle the cut the production host function's unstable argsort may keep other
            samples than the canonical (far, raster index) rule, where they lie inside the kept set it keeps them in another order"""
import numpy as np


def intrinsics(H, W, f=600.0):
    return np.array([[f, 0.0, W / 2 - 0.25], [0.0, f * 1.01, H / 2 + 0.125], [0.0, 0.0, 1.0]])


def plane(H, W, sx=0.0007, sy=0.0003, noise=1e-4, seed=0, z0=1.0):
    rng = np.random.Generator(np.random.PCG64(seed))
    yy, xx = np.mgrid[:H, :W]
    return z0 + sx * (xx - W / 2) + sy * (yy - H / 2) + noise * rng.standard_normal((H, W))


def rect(H, W, y0, x0, h, w):
    m = np.zeros((H, W), dtype=bool)
    m[y0:y0 + h, x0:x0 + w] = True
    return m


def _case(depth, masks, scale=False, host_tie=False, **kwargs):
    H, W = depth.shape
    return dict(depth=np.ascontiguousarray(depth, dtype=np.float64), K=intrinsics(H, W), masks=np.stack(masks).astype(bool), kwargs=kwargs,
                scale=scale, host_tie=host_tie)


# (h, w) of a rectangle away from the image border -> survivors of radius r: (h - 2r)(w - 2r) for r >= 1, h * w for r = 0.5
CHAIN_RECTS = [((20, 25), (21, 21)),    # r = 8: 5 x 5 = exactly 25 survivors, not enough -> r = 4: 13 x 13
               ((25, 20), (18, 29)),    # r = 8: 2 x 13 = exactly 26, enough
               ((28, 30), (9, 30)),     # r = 4: 1 x 22 -> r = 2: 5 x 26
               ((30, 28), (5, 29)),     # r = 2: 1 x 25 = exactly 25 again -> r = 1: 3 x 27
               ((31, 20), (2, 40)),     # r = 1: none -> r = 0.5: all 80 (rows 31 and 32: across a tile seam)
               ((30, 29), (4, 6))]      # 24 pixels: no radius leaves more than 25 -> un-eroded, n_keep clipped to 24
CHAIN_EXPECT = [(1, 169), (0, 26), (2, 130), (3, 81), (4, 80), (5, 24)]      # (radius index, survivors)


def chain_case():
    H, W = 70, 90
    return _case(plane(H, W, seed=1), [rect(H, W, y, x, h, w) for (y, x), (h, w) in CHAIN_RECTS])


def erosion_shapes():
    H, W = 97, 131
    yy, xx = np.mgrid[:H, :W]
    border = rect(H, W, 0, 30, 40, 50)                   # touches the top border: the border is not background
    corner = rect(H, W, 60, 90, 37, 41)                  # the bottom-right corner of the image
    holes = rect(H, W, 20, 20, 55, 80)
    for y, x in ((31, 31), (32, 64), (47, 60), (60, 33), (40, 90)):
        holes[y, x] = False                              # holes of one pixel (two of them on tile seams)
    r2 = (yy - 48) ** 2 + (xx - 65) ** 2
    ring = (r2 <= 40 ** 2) & (r2 >= 28 ** 2)             # 12 thick: nothing survives radius 8
    return dict(border=border, corner=corner, holes=holes, ring=ring)


def erosion_case(radius, min_vertices=1):
    """constant depth 1 with a few pixels at 2 (`outliers`): far is 0 or 1 and the threshold lies strictly between for every survivor
    count >= 2, so the kept set is the survivor set minus the outliers in it — the keep mask reveals the eroded mask"""
    from scipy import ndimage
    shapes = erosion_shapes()
    H, W = next(iter(shapes.values())).shape
    depth = np.ones((H, W))
    outliers = np.zeros((H, W), dtype=bool)
    for m in shapes.values():
        d = ndimage.distance_transform_edt(m)
        outliers[np.unravel_index(int(np.argmax(d)), d.shape)] = True      # the deepest pixel: survives every radius that leaves anything
    depth[outliers] = 2.0
    c = _case(depth, list(shapes.values()), host_tie=True, erosion_radius=radius, min_vertices=min_vertices)
    c["outliers"] = outliers
    return c


def cut_cases():
    H, W = 70, 90
    out = {}
    out["odd"] = _case(plane(H, W, seed=2), [rect(H, W, 15, 20, 37, 55)], scale=True)            # 21 x 39 = 819 survivors
    out["even"] = _case(plane(H, W, seed=3), [rect(H, W, 14, 18, 38, 56)], scale=True)           # 22 x 40 = 880
    out["quirk_constant"] = _case(np.full((H, W), 2.0), [rect(H, W, 10, 20, 40, 40)], host_tie=True)
    q = np.round(plane(H, W, sx=0.00013, sy=0.00007, noise=0.0, seed=0) * 1e4) / 1e4               # 0.1 mm steps: ties on both sides
    out["quantised"] = _case(q, [rect(H, W, 10, 12, 45, 66)], scale=True)
    d = plane(H, W, seed=4)
    d[33, 47] += 0.5
    out["outlier"] = _case(d, [rect(H, W, 15, 20, 37, 55)], scale=True)
    # the min_vertices clamp on quantised depth: 40 survivors, 23 near the median, 8 at exactly -0.25 and 9 at exactly +0.25.
    # thr = 1.5 sigma = 0.245 < 0.25: 23 within -> n_keep = 25 -> two of the 17 tied samples, the first two in raster order
    z = np.array([0.9999] * 7 + [1.0] * 9 + [1.0001] * 7 + [0.75] * 8 + [1.25] * 9)
    z = z[np.random.Generator(np.random.PCG64(5)).permutation(40)]
    d = np.full((H, W), 1.0)
    d[30:35, 28:36] = z.reshape(5, 8)
    out["clamp_ties"] = _case(d, [rect(H, W, 30, 28, 5, 8)], host_tie=True)
    return out


def largest_tie_case():
    """equal-area components: the first in scan order wins — partner in the same tile row, in another tile, and a larger one that
    starts later"""
    H, W = 70, 90
    a = rect(H, W, 5, 40, 6, 7) | rect(H, W, 40, 8, 6, 7)                 # tie across tiles: the upper one wins
    b = rect(H, W, 36, 50, 6, 7) | rect(H, W, 36, 10, 6, 7)               # same rows: the left one wins
    c = rect(H, W, 3, 3, 5, 6) | rect(H, W, 50, 60, 6, 7) | rect(H, W, 20, 70, 6, 7)   # the two larger tie; the smaller comes first
    return _case(plane(H, W, seed=6), [a, b, c])


def vga_case():
    H, W = 480, 640
    yy, xx = np.mgrid[:H, :W]
    d = plane(H, W, sx=0.0004, sy=0.0001, noise=2e-4, seed=7, z0=1.2)
    masks = [rect(H, W, 100, 150, 90, 160),
             ((yy - 300) / 60.0) ** 2 + ((xx - 420) / 110.0) ** 2 <= 1.0,
             rect(H, W, 0, 0, 70, 130),                                      # in the image corner
             rect(H, W, 350, 40, 100, 170) | rect(H, W, 200, 20, 12, 12),    # two components
             ((yy - 150) / 80.0) ** 2 + ((xx - 500) / 45.0) ** 2 <= 1.0]
    d[140, 200] += 0.3
    d[300, 420] -= 0.2
    return _case(d, masks, scale=True)
