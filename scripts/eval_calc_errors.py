"""Alias of freepose_amd.scripts.eval_calc_errors (reference module path: bop_toolkit/scripts/eval_calc_errors.py)."""
from freepose_amd.scripts.eval_calc_errors import *  # noqa: F401,F403
from freepose_amd.scripts.eval_calc_errors import run

if __name__ == "__main__":
    run()
