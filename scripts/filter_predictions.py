"""Alias of freepose_amd.scripts.filter_predictions (reference module path: scripts/filter_predictions.py)."""
from freepose_amd.scripts.filter_predictions import *  # noqa: F401,F403
from freepose_amd.scripts.filter_predictions import build_parser, main, run

if __name__ == "__main__":
    run()
