"""bench.py's measurement contract on one GPU at a small size: a plain run times the hot path only (the secondary legs are
--full's), --steps sets the number of timed steps, and --dump-outputs writes what the last timed step handed its caller — the
same arrays, bit for bit, from two runs on the same seeded inputs."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SMALL = ["--gpus", "1", "--warmup", "1", "--hyp", "24", "--bank", "2000", "--mesh-sub", "3", "--vit-batch", "8"]


def _bench(args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *SMALL, *args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, "stdout holds exactly the result line"
    return json.loads(lines[0])


def test_plain_run_steps_and_dumped_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    two = _bench(["--steps", "2", "--dump-outputs", str(a)])
    one = _bench(["--steps", "1", "--dump-outputs", str(b)])
    for out, n in ((two, 2), (one, 1)):
        assert out["steps"] == n and out["ms_per_step"] > 0 and out["unit"] == "proposals/s" and out["higher_is_better"] is True
        assert out["value"] == pytest.approx(1e3 / out["ms_per_step"], rel=1e-9)       # one proposal per step
        assert out["dtype"] == "bf16" and out["roofline"]["achieved"] > 0
        assert out["video_workload"] is None and out["configs"] is None and out["cpu_baseline"] is None
    assert two["roofline"]["launches"] == 2 * one["roofline"]["launches"] > 0          # the timed loop ran --steps times

    names = sorted(p.name for p in a.glob("*.npy"))
    assert names == sorted(p.name for p in b.glob("*.npy"))
    assert set(names) == {"topk_scores.npy", "topk_idx.npy", "hyp_scores.npy", "hyp_idx.npy", "TCO.npy", "result_rows.npy"}
    shapes = {"topk_scores.npy": (1, 100), "topk_idx.npy": (1, 100), "hyp_scores.npy": (1, 3), "hyp_idx.npy": (1, 3),
              "TCO.npy": (1, 3, 4, 4), "result_rows.npy": (1, 16)}
    for nm in names:
        x, y = np.load(a / nm), np.load(b / nm)
        assert x.dtype in (np.float32, np.float64) and x.shape == shapes[nm], (nm, x.dtype, x.shape)
        assert np.isfinite(x).all() and x.dtype == y.dtype and x.tobytes() == y.tobytes(), nm
    rows, tco = np.load(a / "result_rows.npy"), np.load(a / "TCO.npy")
    assert rows[0, 0] == np.load(a / "topk_idx.npy")[0, 0] and rows[0, 2] == np.load(a / "hyp_idx.npy")[0, 0]
    assert np.array_equal(rows[0, 4:13], tco[0, 0, :3, :3].ravel()) and np.array_equal(rows[0, 13:16], tco[0, 0, :3, 3])
