"""Alias of freepose_amd.scripts.compute_scale_video (reference module path: scripts/compute_scale_video.py)."""
from freepose_amd.scripts.compute_scale_video import *  # noqa: F401,F403
from freepose_amd.scripts.compute_scale_video import build_parser, main, run

if __name__ == "__main__":
    run()
