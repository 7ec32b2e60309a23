"""A point tracker for a synthetic clip whose ground truth is known (tests/test_gpu_refiner_track.py): each query pixel (t, x, y) is lifted
to the object's surface with the rasterised depth of frame t under the planted pose and projected with every frame's planted pose;
a point is visible in a frame where the frame's depth map agrees with the projected point's depth.  The frames it is handed are a slice
of the clip; it recognises them by their CRC.

    make(scene=".../scene.npz")   # vertices, faces, colors, K, poses [n,4,4], frames u8 [n,H,W,3]; the --tracker factory
"""
from __future__ import annotations

import time
import zlib

import numpy as np
import torch

DEPTH_TOL = 0.004       # metres: the object is 0.25 across


class SynthTracker:
    def __init__(self, vertices, faces, colors, K, poses, frames):
        from freepose_amd import ops
        self.K = np.asarray(K, dtype=np.float64)
        self.poses = np.asarray(poses, dtype=np.float64)
        H, W = frames.shape[1:3]
        mesh = ops.Mesh(vertices, faces, colors)
        _, depth = ops.rasterize(mesh, torch.from_numpy(self.poses.astype(np.float32)), 1.0, self.K[0, 0], self.K[1, 1], self.K[0, 2],
                                 self.K[1, 2], W, H)
        self.depth = depth.cpu().numpy().astype(np.float64)                    # [n,H,W], 0 = background
        self.index = {zlib.crc32(f.tobytes()): i for i, f in enumerate(frames)}
        assert len(self.index) == len(frames), "two frames of the clip are identical"
        self.seconds = 0.0
        self.calls = 0

    def _lookup(self, depth, uv):
        H, W = depth.shape
        x, y = np.rint(uv[:, 0]).astype(int), np.rint(uv[:, 1]).astype(int)
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        d = np.zeros(len(uv))
        d[ok] = depth[y[ok], x[ok]]
        return d

    def __call__(self, frames_u8, queries):
        t0 = time.perf_counter()
        ids = [self.index[zlib.crc32(np.ascontiguousarray(f).tobytes())] for f in frames_u8]
        queries = np.asarray(queries, dtype=np.float64)
        fx, fy, cx, cy = self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2]
        T, N = len(ids), len(queries)
        tracks = np.tile(queries[None, :, 1:], (T, 1, 1))
        vis = np.zeros((T, N), bool)
        for q_t in np.unique(queries[:, 0].astype(int)):
            sel = np.nonzero(queries[:, 0].astype(int) == q_t)[0]
            uv = queries[sel, 1:]
            z = self._lookup(self.depth[ids[q_t]], uv)
            hit = z > 0
            cam = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
            P = self.poses[ids[q_t]]
            obj = (cam - P[:3, 3]) @ P[:3, :3]                                  # R^T (x - t)
            for k, f in enumerate(ids):
                c = obj @ self.poses[f, :3, :3].T + self.poses[f, :3, 3]
                with np.errstate(all="ignore"):
                    p = np.stack([cx + fx * c[:, 0] / c[:, 2], cy + fy * c[:, 1] / c[:, 2]], 1)
                p[~hit] = uv[~hit]
                tracks[k, sel] = p
                vis[k, sel] = hit & (np.abs(self._lookup(self.depth[f], p) - c[:, 2]) < DEPTH_TOL)
        self.seconds += time.perf_counter() - t0
        self.calls += 1
        return tracks.astype(np.float32), vis


def make(scene: str):
    s = np.load(scene)
    return SynthTracker(s["vertices"], s["faces"], s["colors"], s["K"], s["poses"], s["frames"])
