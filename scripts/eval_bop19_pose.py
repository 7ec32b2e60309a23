"""Alias of freepose_amd.scripts.eval_bop19_pose (reference module path: bop_toolkit/scripts/eval_bop19_pose.py)."""
from freepose_amd.scripts.eval_bop19_pose import *  # noqa: F401,F403
from freepose_amd.scripts.eval_bop19_pose import build_parser, run

if __name__ == "__main__":
    run()
