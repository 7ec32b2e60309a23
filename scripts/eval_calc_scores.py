"""Alias of freepose_amd.scripts.eval_calc_scores (reference module path: bop_toolkit/scripts/eval_calc_scores.py)."""
from freepose_amd.scripts.eval_calc_scores import *  # noqa: F401,F403
from freepose_amd.scripts.eval_calc_scores import build_parser, run

if __name__ == "__main__":
    run()
