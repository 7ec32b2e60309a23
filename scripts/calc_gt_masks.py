"""Alias of freepose_amd.scripts.calc_gt_masks (reference module path: bop_toolkit/scripts/calc_gt_masks.py)."""
from freepose_amd.scripts.calc_gt_masks import *  # noqa: F401,F403
from freepose_amd.scripts.calc_gt_masks import build_parser, run

if __name__ == "__main__":
    run()
