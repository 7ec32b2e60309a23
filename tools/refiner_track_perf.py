"""HIP-event times of one ops.pnp_epnp call (B = 12 frames, N = 600 points, 80 % visible, sigma = 0.5 px) and one ops.patch_points call
(S = 10 000 samples, C = 700 cells), inputs on the device: 3 warm-up calls, median / min / max of 20 (profiles/refiner_track.md).

    python tools/refiner_track_perf.py
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from freepose_amd import ops  # noqa: E402
from tests import _refiner_ref as ref  # noqa: E402

rng = np.random.default_rng(0)
N, B = 600, 12
p3 = rng.uniform(-1, 1, (N, 3)) * np.array([0.09, 0.06, 0.12])
p2 = []
for b in range(B):
    R = ref.rodrigues(rng.standard_normal(3), rng.uniform(0.2, 2.8))
    t = np.array([0.02, -0.01, 0.9])
    p2.append(ref._project_noisy(p3, R, t, 0.5, rng))
p3d, p2d, Kd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (p3, np.stack(p2), ref.K_TEST))
vis = torch.from_numpy((rng.random((B, N)) < 0.8).astype(np.uint8)).cuda()


def measure(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        tm = ops.Timer()
        tm.start()
        fn()
        tm.stop()
        ts.append(tm.elapsed_ms())
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


print("pnp_epnp B=12 N=600: median %.3f ms (min %.3f, max %.3f)" % measure(lambda: ops.pnp_epnp(p3d, p2d, Kd, vis)), flush=True)

d = rng.standard_normal((10000, 3))
samples = d / np.linalg.norm(d, axis=1, keepdims=True) * np.array([0.09, 0.05, 0.12])
K = np.array([[2100.0, 0, 259.0], [0, 2100.0, 259.0], [0, 0, 1]])
T = np.eye(4)
T[:3, :3] = ref.rodrigues([0.3, 1.0, 0.2], 0.8)
T[:3, 3] = [0, 0, 0.62]
occ = list(ref.cell_lists(samples, T, K))
cells = np.array((occ * 3)[:700], np.int32)
print("occupied cells", len(occ), flush=True)
s, Td, Kd2, cd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (samples, T[None], K[None], cells[None]))
print("patch_points S=10000 C=700: median %.3f ms (min %.3f, max %.3f)" % measure(lambda: ops.patch_points(s, Td, Kd2, cd)), flush=True)
