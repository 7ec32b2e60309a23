"""Alias of freepose_amd.scripts.calc_model_info (reference module path: bop_toolkit/scripts/calc_model_info.py)."""
from freepose_amd.scripts.calc_model_info import *  # noqa: F401,F403
from freepose_amd.scripts.calc_model_info import build_parser, run

if __name__ == "__main__":
    run()
