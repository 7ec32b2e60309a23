"""numpy restatement of what the BOP toolkit computes per ground-truth instance and per model (bop_toolkit/scripts/calc_gt_info.py:131-185,
calc_gt_masks.py:107-126, calc_model_info.py:36-50, bop_toolkit_lib/misc.py depth_im_to_dist_im_fast :146-167, calc_2d_bbox :206-222,
calc_pts_diameter :289-303, visibility.py:34-38), the planted cases of the kernel tests, and the file format of
tools/gt_info_host_check.cpp.  tests/test_gt_info_cpu.py pins this file to tests/golden/gt_info.npz, which the reference's own functions
wrote (tools/gen_golden_gt_info.py); tests/test_gpu_gt_info.py compares the kernels with it, with ==.
"""
import json
import subprocess

import numpy as np

INFO_KEYS = ["px_count_all", "px_count_valid", "px_count_visib", "visib_fract", "bbox_obj", "bbox_visib"]     # calc_gt_info.py:176-185
MODEL_KEYS = ["min_x", "min_y", "min_z", "size_x", "size_y", "size_z", "diameter"]                              # calc_model_info.py:42-50
BOX_EMPTY = [2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31]
TILE = 1024                                                                                                      # gt_info.hip DM_TILE


# ---- per pixel ---------------------------------------------------------------------------------------------------------------------
def dist_im(depth, K):
    """depth (z) image -> distance-from-the-camera-centre image, float64: sqrt((u z)^2 + (v z)^2 + z^2) with u = (x - cx) / fx,
    v = (y - cy) / fy (what misc.depth_im_to_dist_im_fast returns)"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    H, W = depth.shape
    u = (np.arange(W, dtype=np.float64) - K[0, 2]) / K[0, 0]
    v = (np.arange(H, dtype=np.float64) - K[1, 2]) / K[1, 1]
    z = depth.astype(np.float64)
    a, b = u[None, :] * z, v[:, None] * z
    return np.sqrt(a * a + b * b + z * z)


def visib_mask(dist_test, dist_gt, delta):
    """visibility mode bop19 (what visibility.estimate_visib_mask_gt returns): on the render, and either not farther than delta behind
    the test surface — both distances cast to float32, the difference compared in float32 — or over missing test depth"""
    near = (dist_gt.astype(np.float32) - dist_test.astype(np.float32)) <= np.float32(delta)
    return (near | (dist_test == 0)) & (dist_gt > 0)


def box_of(xs, ys):
    """misc.calc_2d_bbox without clipping"""
    return [xs.min(), ys.min(), xs.max() - xs.min(), ys.max() - ys.min()]


def instance(canvas, depth_test, K, delta, ox, oy):
    """one instance in the order of calc_gt_info.py:125-185 -> (info dict, kernel row [12], mask u8, mask_visib u8)"""
    H, W = depth_test.shape
    depth_gt = canvas[oy:oy + H, ox:ox + W]
    dist_gt, dist_t = dist_im(depth_gt, K), dist_im(depth_test, K)
    visib = visib_mask(dist_t, dist_gt, delta)
    large, mask = canvas > 0, dist_gt > 0
    px_all, px_valid, px_visib = int(np.sum(large)), int(np.sum(dist_t[mask] > 0)), int(visib.sum())
    fract = px_visib / float(px_all) if px_all > 0 else 0.0
    bbox, bbox_visib = [-1, -1, -1, -1], [-1, -1, -1, -1]
    if px_visib > 0:
        ys, xs = large.nonzero()
        bbox = box_of(xs - ox, ys - oy)
        ys, xs = visib.nonzero()
        bbox_visib = box_of(xs, ys)
    info = {"px_count_all": px_all, "px_count_valid": px_valid, "px_count_visib": px_visib, "visib_fract": float(fract),
            "bbox_obj": [int(e) for e in bbox], "bbox_visib": [int(e) for e in bbox_visib]}
    row = [px_all, px_valid, px_visib, 0] + list(BOX_EMPTY) + list(BOX_EMPTY)
    if px_all:
        ys, xs = large.nonzero()
        row[4:8] = [int(xs.min()) - ox, int(ys.min()) - oy, int(xs.max()) - ox, int(ys.max()) - oy]
    if px_visib:
        ys, xs = visib.nonzero()
        row[8:12] = [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())]
    return info, row, (255 * mask.astype(np.uint8)), (255 * visib.astype(np.uint8))


def run_case(c):
    """a case of vis_cases() -> (infos, rows i64 [B,12], masks u8 [B,H,W], masks_visib u8 [B,H,W])"""
    infos, rows, masks, visibs = [], [], [], []
    ox, oy = c["window"]
    for b in range(len(c["depth_gt"])):
        i, r, m, v = instance(c["depth_gt"][b], c["depth_test"][c["img_idx"][b]], c["K"][b], c["delta"], ox, oy)
        infos.append(i), rows.append(r), masks.append(m), visibs.append(v)
    H, W = c["depth_test"].shape[1:]
    return (infos, np.array(rows, np.int64).reshape(-1, 12), np.array(masks, np.uint8).reshape(-1, H, W),
            np.array(visibs, np.uint8).reshape(-1, H, W))


def save_json_text(content):
    """inout.save_json for a dict: top-level keys sorted, one per line"""
    items = sorted(content.items(), key=lambda x: x[0])
    return "{\n" + ",\n".join('  "{}": {}'.format(k, json.dumps(v, sort_keys=True)) for k, v in items) + ("\n" if items else "") + "}"


# ---- per model ---------------------------------------------------------------------------------------------------------------------
def pair_d2(d):
    """(pts_diff * pts_diff).sum(axis=1) of rows d [...,3]: the three columns are added left to right"""
    s = d * d
    return (s[..., 0] + s[..., 1]) + s[..., 2]


def pair_d2_other(d):
    """the other association, dx^2 + (dy^2 + dz^2): NOT what numpy computes"""
    s = d * d
    return s[..., 0] + (s[..., 1] + s[..., 2])


def pts_diameter(pts, block=512, d2=pair_d2):
    """misc.calc_pts_diameter, blocked: the maximum of the squares, one square root (sqrt is monotone)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    best = -1.0
    for i0 in range(0, len(pts), block):
        a = pts[i0:i0 + block]
        for j0 in range(i0, len(pts), block):
            best = max(best, float(d2(a[:, None, :] - pts[None, j0:j0 + block, :]).max()))
    return float(np.sqrt(np.float64(best)))


def model_row(pts):
    """the row of fp_pts_diameter: {diameter, min x, y, z, size x, y, z, 0}"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    ref_pt = pts.min(axis=0)
    size = pts.max(axis=0) - ref_pt
    return np.array([pts_diameter(pts), *ref_pt, *size, 0.0], np.float64)


def model_info(pts):
    """calc_model_info.py:36-50 (with the Python 3 reading of its map() calls)"""
    r = model_row(pts)
    return {"min_x": float(r[1]), "min_y": float(r[2]), "min_z": float(r[3]), "size_x": float(r[4]), "size_y": float(r[5]),
            "size_z": float(r[6]), "diameter": float(r[0])}


# ---- planted cases -----------------------------------------------------------------------------------------------------------------
def _K(fx, fy, cx, cy):
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def _test_image(rng, H, W, holes=True):
    t = (1000.0 + 40.0 * rng.random((H, W))).astype(np.float32)
    if holes:
        t[rng.random((H, W)) < 0.08] = 0.0
    return t


def _blob(rng, canvas, test, ox, oy, x0, y0, x1, y1):
    """a silhouette over canvas[y0:y1, x0:x1]: depth = the test depth under it (1020 outside the image or over a hole) plus an offset in
    front of, inside or beyond the 15 mm band"""
    H, W = test.shape
    for y in range(max(y0, 0), min(y1, canvas.shape[0])):
        for x in range(max(x0, 0), min(x1, canvas.shape[1])):
            base = 1020.0
            if 0 <= y - oy < H and 0 <= x - ox < W and test[y - oy, x - ox] > 0:
                base = float(test[y - oy, x - ox])
            canvas[y, x] = np.float32(base + rng.choice([-40.0, -3.0, 5.0, 14.5, 40.0]))


def vis_cases():
    """name -> {depth_gt f32 [B,Hr,Wr], depth_test f32 [n_img,H,W], img_idx [B], K f64 [B,3,3], delta, window (ox, oy)}"""
    rng = np.random.default_rng(20241020)
    cases = {}
    # 1. truth table at image size: (d_gt, d_test) > 0 x {in front of, inside, beyond} the band; column = combination, every row the same
    W, H = 64, 48
    K = _K(70.0, 65.0, 31.5, 22.25)
    test, gt = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    combos = [(g, t, off) for g in (0, 1) for t in (0, 1) for off in (-40.0, 5.0, 40.0)]
    for k, (g, t, off) in enumerate(combos):
        test[:, 4 * k:4 * k + 4] = 1000.0 if t else 0.0
        gt[:, 4 * k:4 * k + 4] = (1000.0 + off) if g else 0.0
    cases["truth"] = dict(depth_gt=gt[None], depth_test=test[None], img_idx=[0], K=K[None], delta=15, window=(0, 0))
    # 2. float32 differences of exactly delta and one ulp either side, one pixel each at the integer principal point; 37 x 29 in 111 x 87:
    # nothing is a multiple of 4 (the scalar loop) and the window offset is odd
    W, H = 37, 29
    K = _K(50.0, 50.0, 18.0, 14.0)
    test = np.full((H, W), 1000.0, np.float32)
    gts = np.zeros((3, 3 * H, 3 * W), np.float32)
    for b, d in enumerate((np.float32(1015.0), np.nextafter(np.float32(1015.0), np.float32(2000.0)), np.nextafter(np.float32(1015.0), np.float32(0.0)))):
        gts[b, H + 14, W + 18] = d
    cases["ulp"] = dict(depth_gt=gts, depth_test=test[None], img_idx=[0, 0, 0], K=np.stack([K] * 3), delta=15, window=(W, H))
    # 3. the edge set on 64 x 48 in 192 x 144, three test images (1 = all zero), mixed indices
    W, H = 64, 48
    ox, oy = W, H
    tests = np.stack([_test_image(rng, H, W), np.zeros((H, W), np.float32), _test_image(rng, H, W)])
    K = _K(80.0, 82.0, 30.7, 25.2)
    gts = np.zeros((7, 3 * H, 3 * W), np.float32)
    idx = [0, 1, 2, 2, 0, 2, 0]
    _blob(rng, gts[0], tests[0], ox, oy, ox + 10, oy + 5, ox + 50, oy + 40)            # inside the image
    _blob(rng, gts[1], tests[1], ox, oy, ox - 20, oy + 10, ox + 30, oy + 60)           # test all zero: every silhouette pixel in the image is visible
    #     gts[2]: empty
    _blob(rng, gts[3], tests[2], ox, oy, 5, 7, 40, 30)                                 # only in the truncated ring
    gts[4, oy + 20, ox + 33] = np.float32(tests[0][20, 33] + 1.0 if tests[0][20, 33] > 0 else 1000.0)   # one visible pixel
    for (x, y) in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)):                    # the four image corners, visible (over a hole or in the band)
        gts[5, oy + y, ox + x] = np.float32(tests[2][y, x] + 2.0 if tests[2][y, x] > 0 else 990.0)
    _blob(rng, gts[6], tests[0], ox, oy, 0, 0, 3 * W, 3)                               # touching the canvas border: top row ...
    _blob(rng, gts[6], tests[0], ox, oy, 3 * W - 2, 0, 3 * W, 3 * H)                   # ... right column, through to the last pixel
    _blob(rng, gts[6], tests[0], ox, oy, 0, 3 * H - 1, 9, 3 * H)
    _blob(rng, gts[6], tests[0], ox, oy, ox + 60, oy + 40, ox + 70, oy + 50)           # and across the image's corner
    cases["edges"] = dict(depth_gt=gts, depth_test=tests, img_idx=idx, K=np.stack([K] * 7), delta=15, window=(ox, oy))
    # 4. odd sizes: canvas and image-size variants, per-instance intrinsics and a non-integer delta
    W, H = 37, 29
    tests = np.stack([_test_image(rng, H, W), _test_image(rng, H, W)])
    Ks = np.stack([_K(45.0, 47.0, 17.3, 15.1), _K(61.0, 59.0, 20.2, 11.9)])
    gts = np.zeros((2, 3 * H, 3 * W), np.float32)
    _blob(rng, gts[0], tests[1], W, H, W - 9, H + 3, W + 21, H + 40)
    _blob(rng, gts[1], tests[0], W, H, W + 30, H - 5, W + 50, H + 12)
    cases["odd_canvas"] = dict(depth_gt=gts, depth_test=tests, img_idx=[1, 0], K=Ks, delta=7.3, window=(W, H))
    cases["odd_image"] = dict(depth_gt=np.ascontiguousarray(gts[:, H:2 * H, W:2 * W]), depth_test=tests, img_idx=[1, 0], K=Ks, delta=7.3,
                              window=(0, 0))
    return cases


def big_case():
    """640 x 480 in 1920 x 1440: more pixel groups than the launch has lanes (the grid-stride loop), a silhouette across the image border"""
    rng = np.random.default_rng(7)
    W, H = 640, 480
    test = _test_image(rng, H, W)
    gt = np.zeros((3 * H, 3 * W), np.float32)
    yy, xx = np.mgrid[0:3 * H, 0:3 * W]
    inside = ((xx - (W + 600)) / 220.0) ** 2 + ((yy - (H + 130)) / 170.0) ** 2 < 1.0
    base = np.full((3 * H, 3 * W), 1020.0, np.float32)
    base[H:2 * H, W:2 * W] = np.where(test > 0, test, 1020.0)
    off = rng.choice(np.array([-40.0, -3.0, 5.0, 14.5, 40.0], np.float32), size=gt.shape)
    gt[inside] = (base + off)[inside]
    K = _K(1066.778, 1067.487, 312.9869, 241.3109)
    return dict(depth_gt=gt[None], depth_test=test[None], img_idx=[0], K=K[None], delta=15, window=(W, H))


def _planted(rng, n, scale, a, b):
    """n points within `scale` of the origin, rows a and b pushed apart to be the one farthest pair"""
    p = rng.normal(size=(n, 3))
    p *= scale / np.abs(p).max()
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    p[a], p[b] = 4.0 * scale * u + p[a] * 0.01, -4.0 * scale * u + p[b] * 0.01
    return p


def assoc_cloud():
    """a cloud on whose farthest pair (dx^2 + dy^2) + dz^2 and dx^2 + (dy^2 + dz^2) differ, and still differ after the square root"""
    for seed in range(1000):
        rng = np.random.default_rng(seed)
        p = rng.normal(size=(64, 3))
        d = p[:, None, :] - p[None, :, :]
        if np.sqrt(pair_d2(d).max()) != np.sqrt(pair_d2_other(d).max()):
            return p
    raise AssertionError("no such cloud")


def diam_cases(big=True):
    """name -> list of f64 [n,3] clouds handed to one call"""
    rng = np.random.default_rng(99)
    c = {}
    c["tiny"] = [rng.normal(size=(1, 3)), rng.normal(size=(2, 3)), rng.normal(size=(3, 3))]
    c["tiles"] = [_planted(rng, TILE - 1, 50.0, 0, TILE - 2), _planted(rng, TILE, 50.0, 5, 900), _planted(rng, TILE + 1, 50.0, 10, TILE),
                  _planted(rng, 2 * TILE + 5, 50.0, 10, 2 * TILE + 2), rng.normal(size=(2 * TILE + 5, 3))]
    one = rng.normal(size=(1, 3))
    c["dup"] = [np.repeat(one, 40, axis=0), np.concatenate([np.repeat(one, 7, axis=0), np.repeat(one + [3.0, -4.0, 12.0], 5, axis=0)])]
    c["scales"] = [rng.normal(size=(300, 3)) * s + 1.0e6 for s in (1e-3, 1.0, 1e3)]     # an fp32 or |a|^2 + |b|^2 - 2ab shortcut loses these
    c["assoc"] = [assoc_cloud()]
    if big:
        c["big"] = [np.asarray(rng.normal(size=(8192, 3)).astype(np.float32), np.float64) * 60.0]     # float32 vertices, as a PLY holds them
    return c


# ---- tools/gt_info_host_check.cpp ----------------------------------------------------------------------------------------------------
def host_visibility(exe, tmp, c, want_masks=True):
    """the serial host run of gt_info_core.h on one case -> (rows i32 [B,12], masks, masks_visib)"""
    gt, test = np.ascontiguousarray(c["depth_gt"], np.float32), np.ascontiguousarray(c["depth_test"], np.float32)
    B, Hr, Wr = gt.shape
    n_img, H, W = test.shape
    prm = np.zeros((B, 8))
    Kb = np.asarray(c["K"], np.float64)
    prm[:, 0], prm[:, 1], prm[:, 2], prm[:, 3], prm[:, 4] = Kb[:, 0, 0], Kb[:, 1, 1], Kb[:, 0, 2], Kb[:, 1, 2], c["delta"]
    head = np.array([B, Hr, Wr, c["window"][0], c["window"][1], n_img, H, W, int(want_masks)], np.int32)
    fin, fout = tmp / "vis_in.bin", tmp / "vis_out.bin"
    fin.write_bytes(head.tobytes() + np.asarray(c["img_idx"], np.int32).tobytes() + prm.tobytes() + gt.tobytes() + test.tobytes())
    r = subprocess.run([str(exe), "visibility", str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = fout.read_bytes()
    rows = np.frombuffer(raw[:B * 48], np.int32).reshape(B, 12)
    if not want_masks:
        assert len(raw) == B * 48
        return rows, None, None
    m = np.frombuffer(raw[B * 48:], np.uint8).reshape(2, B, H, W)
    return rows, m[0], m[1]


def host_diameter(exe, tmp, clouds, ranges=None):
    """-> f64 [M,8]; ranges overrides the {first, count} table (refusal checks)"""
    pts = np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds])
    if ranges is None:
        sizes = np.array([len(c) for c in clouds])
        ranges = np.stack([np.concatenate([[0], np.cumsum(sizes)[:-1]]), sizes], axis=1)
    ranges = np.asarray(ranges, np.int32).reshape(-1, 2)
    fin, fout = tmp / "diam_in.bin", tmp / "diam_out.bin"
    fin.write_bytes(np.array([len(pts), len(ranges)], np.int32).tobytes() + ranges.tobytes() + pts.tobytes())
    r = subprocess.run([str(exe), "diameter", str(fin), str(fout)], capture_output=True, text=True)
    if r.returncode == 3:
        return None                                    # refused
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return np.frombuffer(fout.read_bytes(), np.float64).reshape(len(ranges), 8)
