"""Alias of freepose_amd.scripts.compute_scale (reference module path: scripts/compute_scale.py)."""
from freepose_amd.scripts.compute_scale import *  # noqa: F401,F403
from freepose_amd.scripts.compute_scale import build_parser, main, run

if __name__ == "__main__":
    run()
