"""Alias of freepose_amd.scripts.smooth_poses_video (reference module path: scripts/smooth_poses_video.py)."""
from freepose_amd.scripts.smooth_poses_video import *  # noqa: F401,F403
from freepose_amd.scripts.smooth_poses_video import build_parser, main, run

if __name__ == "__main__":
    run()
