"""numpy / scipy reference of the depth-map object scale with every intermediate, and the mask fixtures of its tests.

`reference()` is the production host function's algorithm (freepose_amd/src/pipeline/estimators/scale_estimators.py, itself the
reference's scale_estimators.py:117-187) with ONE thing pinned: the samples are ordered by `np.argsort(far, kind="stable")` over
`np.nonzero`'s row-major order, i.e. by (far ascending, raster index ascending) — the canonical tie rule of the device path.  The host
function's plain `np.argsort` (introsort) leaves equal `far` values in an unspecified order, so the two agree wherever no tie straddles
the cut (tests/test_scale_host_cpu.py says which fixtures are not of that kind)."""
import numpy as np
from scipy import ndimage

D2_CAP = 65
STRUCT8 = np.ones((3, 3), dtype=bool)


def d2_capped(comp: np.ndarray) -> np.ndarray:
    """min(d^2, 65) of distance_transform_edt (d^2 is an integer: rint removes the square root's rounding)"""
    d = ndimage.distance_transform_edt(comp)
    return np.minimum(np.rint(d * d).astype(np.int64), D2_CAP)


def reference(depth, K, mask, erosion_radius=8, std_factor=1.5, min_vertices=25, align=True) -> dict:
    mask = np.asarray(mask).astype(bool)
    lab, n = ndimage.label(mask)
    if n == 0:
        raise ValueError("depthmap scale: empty proposal mask")
    area = np.bincount(lab.ravel())[1:]
    comp = lab == (int(np.argmax(area)) + 1)
    radius, idx = float(erosion_radius), 0
    surv = ndimage.distance_transform_edt(comp) > radius
    while int(surv.sum()) <= min_vertices:
        idx += 1
        if radius < 1:
            surv = comp
            break
        radius /= 2
        surv = ndimage.distance_transform_edt(comp) > radius
    rows, cols = np.nonzero(surv)
    z = np.asarray(depth, dtype=np.float64)[rows, cols]
    far = np.abs(z - np.median(z))
    thr = np.std(z) * std_factor
    order = np.argsort(far, kind="stable")
    n_keep = min(max(int(np.argmax(far[order] > thr)), min_vertices), len(z))
    sel = order[:n_keep]
    keep = np.zeros(mask.shape, dtype=bool)
    keep[rows[sel], cols[sel]] = True
    z, cols, rows = z[sel], cols[sel], rows[sel]
    K = np.asarray(K, dtype=np.float64)
    pts = np.column_stack(((cols - K[0, 2]) * z / K[0, 0], (rows - K[1, 2]) * z / K[1, 1], z)).reshape(-1, 3)
    eig = None
    if align:
        centred = pts - pts.mean(axis=0)
        _, sv, vh = np.linalg.svd(centred.T @ centred)
        eig = sv
        pts = pts @ vh.T
    span = pts.max(axis=0) - pts.min(axis=0)
    return dict(component=comp, area=int(comp.sum()), d2=d2_capped(comp), radius_index=idx, survivors=int(surv.sum()), survivor_mask=surv,
                n_keep=n_keep, keep=keep, scale=float(span.max() / 2.0), far=far, thr=float(thr), eig=eig)


def cut_is_clear(ref: dict, rel: float = 1e-9) -> bool:
    """no |z - median| within `rel` of the threshold, so a last-bit difference in the standard deviation cannot move the count.  A sample
    AT the median (far == 0) is on the near side of every threshold >= 0 whatever its last bits."""
    far, thr = ref["far"], ref["thr"]
    return bool(np.all((far == 0) | (np.abs(far - thr) > rel * thr)))


# ---- labelling fixtures ---------------------------------------------------------------------------------------------------------------
def serpentine(H, W):
    m = np.zeros((H, W), dtype=bool)
    m[0::2] = True
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def spiral(H, W):
    """a one-pixel-wide inward spiral with one-pixel gaps (a walker that turns right when the cell two steps ahead is taken)"""
    m = np.zeros((H, W), dtype=bool)
    y = x = d = turns = 0
    m[0, 0] = True
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    inside = lambda a, b: 0 <= a < H and 0 <= b < W      # noqa: E731
    while turns < 2:
        dy, dx = dirs[d]
        ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if inside(ny, nx) and not m[ny, nx] and not (inside(fy, fx) and m[fy, fx]):
            y, x, turns = ny, nx, 0
            m[y, x] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def label_masks(H, W, tile=32):
    """name -> mask: the shapes of the labelling tests (the kernel's tile is 32 x 32; H, W span at least 3 x 3 tiles)"""
    rng = np.random.Generator(np.random.PCG64(H * 1000 + W))
    out = {"empty": np.zeros((H, W), dtype=bool), "full": np.ones((H, W), dtype=bool)}
    m = np.zeros((H, W), dtype=bool)
    m[H // 2, W // 2] = True
    out["single"] = m
    yy, xx = np.mgrid[:H, :W]
    out["checkerboard"] = (yy + xx) % 2 == 0
    m = np.zeros((H, W), dtype=bool)
    k = np.arange(min(H, W))
    m[k, k] = True
    out["diagonal"] = m
    out["serpentine"] = serpentine(H, W)
    out["spiral"] = spiral(H, W)
    m = np.zeros((H, W), dtype=bool)          # blobs that touch only across a tile corner, on both diagonals
    m[tile - 4:tile, tile - 4:tile] = True
    m[tile:tile + 4, tile:tile + 4] = True
    m[tile - 4:tile, 2 * tile:2 * tile + 4] = True
    m[tile:tile + 4, 2 * tile - 4:2 * tile] = True
    out["tile_corner"] = m
    for dens in (0.3, 0.5, 0.59):
        out[f"random_{dens}"] = rng.random((H, W)) < dens
    return out


def scipy_labels(mask, connectivity):
    return ndimage.label(mask, structure=STRUCT8 if connectivity == 8 else None)[0]


def ranked(labels):
    """canonical labels (1 + raster index of the first pixel) -> 1, 2, ... in increasing order: scipy's numbering"""
    labels = np.asarray(labels)
    u = np.unique(labels[labels > 0])
    return np.where(labels > 0, np.searchsorted(u, labels) + 1, 0)
