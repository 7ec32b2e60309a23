"""Alias of freepose_amd.scripts.eval_videos (reference module path: scripts/eval_videos.py)."""
from freepose_amd.scripts.eval_videos import *  # noqa: F401,F403
from freepose_amd.scripts.eval_videos import build_parser, main, run

if __name__ == "__main__":
    run()
