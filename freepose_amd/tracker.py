"""The built-in point tracker: pyramidal Lucas-Kanade with a forward-backward check on the device (csrc/lk_track.hip).

    python -m scripts.smooth_poses_video ... --tracker freepose_amd.tracker:klt [--tracker_args '{"radius": 9}']
    TrackingRefiner(tracker=freepose_amd.tracker.klt())

What this is: a classical tracker (Bouguet's formulation of Lucas-Kanade; each point is followed frame to frame through a grey pyramid
and kept while the way there and back agree) that fills the `tracker` slot of TrackingRefiner so that the tracked-pose step runs as
shipped.  What it is not: a port of CoTracker, which the reference fetches from torch.hub and which INTEGRATION.md shows how to wrap.  It
sees one pair of frames at a time, knows nothing about occlusion beyond its own checks, and makes no parity claim against the
reference's tracks; it is not pinned to cv2.calcOpticalFlowPyrLK either.  It is pinned to the numpy restatement tests/_lk_ref.py and to
the planted truth of synthetic clips.
"""
from __future__ import annotations

import numpy as np
import torch

# thresholds on the two quality measures, from the sweep of profiles/klt_tracker.md
DEFAULT_MIN_EIG = 1.0            # smaller eigenvalue of the window's gradient matrix per pixel, grey levels^2 / px^2
DEFAULT_MAX_RESIDUAL = 12.0      # mean |A - B| over the window at the final position, grey levels


class LKTracker:
    """tracker(frames u8 [T,H,W,3], queries [N,3] = (t, x, y)) -> (tracks float32 [T,N,2], visibility bool [T,N]) as numpy arrays: the
    tracker contract of TrackingRefiner.  `last` keeps the diagnostics of the last call: dict(diag float32 [T,N,4] = forward-backward
    distance, eigenvalue, residual, flags (ops.LK_FLAG_*); sizes = the pyramid's level sizes)."""

    def __init__(self, levels: int = 4, radius: int = 7, iters: int = 10, fb_thresh: float = 1.0, min_eig: float = DEFAULT_MIN_EIG,
                 max_residual: float = DEFAULT_MAX_RESIDUAL):
        from . import ops
        if not 1 <= int(levels) <= ops.LK_MAX_LEVELS:
            raise ValueError(f"LKTracker: levels={levels} (1..{ops.LK_MAX_LEVELS})")
        if not 1 <= int(radius) <= ops.LK_MAX_RADIUS:
            raise ValueError(f"LKTracker: radius={radius} (1..{ops.LK_MAX_RADIUS})")
        if not 1 <= int(iters) <= ops.LK_MAX_ITERS:
            raise ValueError(f"LKTracker: iters={iters} (1..{ops.LK_MAX_ITERS})")
        self.levels, self.radius, self.iters = int(levels), int(radius), int(iters)
        self.fb_thresh, self.min_eig, self.max_residual = float(fb_thresh), float(min_eig), float(max_residual)
        self.last = None

    @staticmethod
    def check_inputs(frames, queries):
        """-> (frames as a tensor, queries float32 numpy [N,3]); ValueError for anything the tracker refuses"""
        f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
        if f.dtype != torch.uint8:
            raise ValueError(f"LKTracker: frames of dtype {f.dtype} (uint8 RGB expected)")
        if f.dim() != 4 or f.shape[3] != 3 or f.shape[0] < 1 or f.shape[1] < 1 or f.shape[2] < 1:
            raise ValueError(f"LKTracker: frames of shape {tuple(f.shape)} ([T,H,W,3] expected)")
        q = queries.detach().cpu().numpy() if isinstance(queries, torch.Tensor) else np.asarray(queries)
        if q.ndim != 2 or q.shape[1] != 3:
            raise ValueError(f"LKTracker: queries of shape {tuple(q.shape)} ([N,3] = (t, x, y) expected)")
        q = q.astype(np.float32)
        if not np.isfinite(q).all():
            raise ValueError("LKTracker: non-finite query")
        t = q[:, 0].astype(int)
        if ((t < 0) | (t >= f.shape[0])).any() or (q[:, 0] < 0).any():
            raise ValueError(f"LKTracker: query time outside [0, {f.shape[0]})")
        return f, q

    def __call__(self, frames, queries):
        from . import ops
        f, q = self.check_inputs(frames, queries)
        T, H, W = (int(v) for v in f.shape[:3])
        pyr = ops.lk_pyramid(f, self.levels, self.radius)
        tracks, vis, diag = ops.lk_track(pyr, T, H, W, q, self.levels, self.radius, self.iters, self.fb_thresh, self.min_eig,
                                         self.max_residual)
        self.last = dict(diag=diag.cpu().numpy(), sizes=ops.lk_layout(H, W, self.levels, self.radius))
        return tracks.cpu().numpy(), vis.cpu().numpy().astype(bool)


def klt(**params) -> LKTracker:
    """the --tracker factory: keyword arguments of LKTracker (levels, radius, iters, fb_thresh, min_eig, max_residual)"""
    return LKTracker(**params)
