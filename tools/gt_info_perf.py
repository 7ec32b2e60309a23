"""Times the ground-truth info kernels on one MI355X and writes profiles/gt_info.md.

    python -m tools.gt_info_perf [--out profiles/gt_info.md] [--repeats 5] [--images 300]

What is timed:
  pts_diameter   `ops.pts_diameter` on one cloud of 8 192, 65 536 and 262 144 points already on the device, HIP events around the call (it
                 holds the two kernels, the upload of the 8-byte range table and the entry's read-back of it), median of the repeats; pairs
                 per second counts the n (n + 1) / 2 pairs the reference visits.
  restatement    tests/_gt_info_ref.pts_diameter (blocked numpy, 512 x 512 pairs per step) on the host of the same machine: in full at
                 8 192 points; above that a fixed number of block steps is timed and scaled by the step count (marked "scaled").
  toolkit loop   the structure of misc.calc_pts_diameter (one numpy difference of a point against the tail of the cloud per point) on
                 2 048 points, scaled by the pair count (marked "scaled"): the toolkit itself is not imported here.
  gt_info        `GtInfoCalculator.gt_info` on a stand-in scene of ycbv size: 640 x 480, `--images` images of five instances each, a
                 2 522-vertex model, 1920 x 1440 canvases; wall time split into the rasteriser calls, the fused pass (ops.gt_visibility,
                 with its uploads and the download of the counts) and everything else on the host, by synchronising around each call.
"""
import argparse
import datetime
import time

import numpy as np

from tests import _gt_info_ref as ref

SIZES = (8192, 65536, 262144)
IMAGES_PER_CALL = 32             # scripts/calc_gt_info.py IMAGES_PER_FLUSH
RESTATEMENT_STEPS = 136          # block steps timed above 8 192 points (8 192 points are 136 steps)


def toolkit_style_loop(pts):
    best = -1.0
    for i in range(len(pts)):
        d = pts[i] - pts[i:]
        best = max(best, float(np.sqrt((d * d).sum(axis=1).max())))
    return best


def restatement_time(pts, block=512):
    """seconds of ref.pts_diameter, measured in full or scaled from RESTATEMENT_STEPS block steps -> (seconds, scaled?)"""
    nb = -(-len(pts) // block)
    steps = nb * (nb + 1) // 2
    if steps <= RESTATEMENT_STEPS:
        t0 = time.perf_counter()
        ref.pts_diameter(pts, block)
        return time.perf_counter() - t0, False
    t0 = time.perf_counter()
    for k in range(RESTATEMENT_STEPS):
        a, b = pts[(k % nb) * block:(k % nb) * block + block], pts[((7 * k) % nb) * block:((7 * k) % nb) * block + block]
        ref.pair_d2(a[:, None, :] - b[None, :, :]).max()
    return (time.perf_counter() - t0) * steps / RESTATEMENT_STEPS, True


def sphere_mesh(nu=72, nv=36, radius=60.0):
    """a closed latitude / longitude sphere with a smooth bump pattern: 2 522 vertices, about the size of a ycbv object in mm"""
    v = [[0.0, 0.0, 1.0]]
    for j in range(1, nv):
        th = np.pi * j / nv
        v += [[np.sin(th) * np.cos(2 * np.pi * i / nu), np.sin(th) * np.sin(2 * np.pi * i / nu), np.cos(th)] for i in range(nu)]
    v = np.asarray(v + [[0.0, 0.0, -1.0]])
    ring = lambda j, i: 1 + (j - 1) * nu + i % nu   # noqa: E731
    f = [[0, ring(1, i), ring(1, i + 1)] for i in range(nu)]
    for j in range(1, nv - 1):
        for i in range(nu):
            f += [[ring(j, i), ring(j + 1, i), ring(j + 1, i + 1)], [ring(j, i), ring(j + 1, i + 1), ring(j, i + 1)]]
    f += [[len(v) - 1, ring(nv - 1, i + 1), ring(nv - 1, i)] for i in range(nu)]
    r = radius * (1.0 + 0.10 * np.sin(4 * v[:, 0]) * np.cos(3 * v[:, 1]) + 0.06 * v[:, 2] ** 2)
    return (v * r[:, None]).astype(np.float32), np.asarray(f, np.int32)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/gt_info.md")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=300)
    args = ap.parse_args(argv)
    import torch
    from freepose_amd import evaluation as ev, ops
    from freepose_amd.mesh_io import TriMesh
    rng = np.random.default_rng(5)
    lines = ["# Ground-truth info kernels (`csrc/gt_info.hip`)", "",
             f"Measured {datetime.date.today().isoformat()} on one MI355X with `python -m tools.gt_info_perf` (median of {args.repeats} after one warm-up call).",
             "", "## `pts_diameter`", "",
             "| points | pairs | device call, ms | pairs / s | numpy restatement on the host, s | toolkit-style loop, s |", "|---|---|---|---|---|---|"]
    small = rng.normal(size=(2048, 3)) * 60.0
    t0 = time.perf_counter()
    toolkit_style_loop(small)
    loop_2048 = time.perf_counter() - t0
    for n in SIZES:
        pts = rng.normal(size=(n, 3)) * 60.0
        d_pts = torch.from_numpy(pts).cuda()
        ops.pts_diameter([d_pts])
        ms = []
        for _ in range(args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = ops.pts_diameter([d_pts])
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        pairs = n * (n + 1) // 2
        med = float(np.median(ms))
        sec, scaled = restatement_time(pts)
        if not scaled:
            assert float(out[0, 0]) == ref.pts_diameter(pts)
        loop = loop_2048 * pairs / (2048 * 2049 // 2)
        lines.append(f"| {n} | {pairs:.3e} | {med:.3f} | {pairs / (med * 1e-3):.3e} | {sec:.2f}{' (scaled)' if scaled else ''} | {loop:.1f} (scaled from "
                     f"{loop_2048:.3f} s at 2 048 points) |")
        print(lines[-1], flush=True)
    # ---- gt_info on a stand-in scene ------------------------------------------------------------------------------------------------
    W, H, n_inst = 640, 480, 5
    K = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])
    v, f = sphere_mesh()
    calc = ev.GtInfoCalculator(W, H, 15)
    for o in range(1, n_inst + 1):
        calc.add_model(o, TriMesh(v, f))
    depth = (900.0 + 100.0 * rng.random((H, W))).astype(np.float32)
    depth[rng.random((H, W)) < 0.05] = 0.0
    inst, depths, Ks = [], {}, {}
    for im in range(args.images):
        depths[im], Ks[im] = depth, K
        for o in range(1, n_inst + 1):
            q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            inst.append((im, o, q * np.sign(np.linalg.det(q)), [rng.uniform(-250, 250), rng.uniform(-180, 180), rng.uniform(700, 1100)]))
    spent = {"render": 0.0, "pass": 0.0}
    raster, visib = ops.rasterize, ops.gt_visibility

    def timed(name, fn):
        def wrapper(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **kw)
            torch.cuda.synchronize()
            spent[name] += time.perf_counter() - t0
            return r
        return wrapper

    calc.gt_info(inst[:50], depths, Ks)                       # warm-up: model upload, workspaces
    ops.rasterize, ops.gt_visibility = timed("render", raster), timed("pass", visib)
    try:
        t0 = time.perf_counter()
        infos = []
        for i0 in range(0, len(inst), n_inst * IMAGES_PER_CALL):       # as the command does: 32 images per call
            part = inst[i0:i0 + n_inst * IMAGES_PER_CALL]
            infos += calc.gt_info(part, {i[0]: depths[i[0]] for i in part}, Ks)
        total = time.perf_counter() - t0
    finally:
        ops.rasterize, ops.gt_visibility = raster, visib
    visible = sum(i["px_count_visib"] > 0 for i in infos)
    lines += ["", "## `GtInfoCalculator.gt_info`", "",
              f"Stand-in scene: {W} x {H}, {args.images} images x {n_inst} instances = {len(inst)} instances ({visible} with a visible pixel), a "
              f"{len(v)}-vertex model, {3 * W} x {3 * H} canvases, {ev.GT_INFO_CANVAS_PIXELS_PER_BATCH // (9 * W * H)} canvases per batch, 32 images per call.  One run, "
              "after a warm-up of 50 instances; each part is synchronised, so the parts do not overlap.", "",
              "| part | s | ms per instance |", "|---|---|---|",
              f"| whole call | {total:.3f} | {1e3 * total / len(inst):.3f} |",
              f"| - rasteriser calls (`ops.rasterize`, one per object and batch) | {spent['render']:.3f} | {1e3 * spent['render'] / len(inst):.3f} |",
              f"| - fused pass (`ops.gt_visibility`: uploads, kernel, counts back) | {spent['pass']:.3f} | {1e3 * spent['pass'] / len(inst):.3f} |",
              f"| - host (test depth upload, pose packing, canvas gather, dicts) | {total - spent['render'] - spent['pass']:.3f} | "
              f"{1e3 * (total - spent['render'] - spent['pass']) / len(inst):.3f} |", "",
              "Not measured: the three commands on a real dataset (PNG decoding and writing included), `gt_masks`, and the kernels alone "
              "without their host calls.  The reference scripts were not run: they need an OpenGL renderer.", ""]
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines[-12:]))


if __name__ == "__main__":
    main()
