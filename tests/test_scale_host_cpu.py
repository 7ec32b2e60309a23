"""No-GPU checks of the depth-map scale: (1) tools/scale_host_check.cpp — the index arithmetic of csrc/scale_core.h run serially in the
kernels' phase order, built with -fsanitize=address,undefined — against scipy on the labelling and erosion fixtures; (2) the tests'
reference tests/_scale_ref.py against the production host function; (3) the new boundary: header / ctypes entries, estimator classes,
CLI flag."""
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest
from scipy import ndimage

from tests import _scale_cases as cases
from tests import _scale_ref as ref

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("scale_host") / "scale_host_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "freepose_amd" / "csrc"),
           str(ROOT / "tools" / "scale_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run(exe, tmp_path, masks, connectivity, min_vertices=25, radius=8.0):
    masks = np.ascontiguousarray(np.asarray(masks).astype(np.uint8))
    n, H, W = masks.shape
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    fin.write_bytes(struct.pack("<5id", n, H, W, connectivity, min_vertices, radius) + masks.tobytes())
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])       # a sanitizer report ends the program with a non-zero status
    blob, out, off = fout.read_bytes(), [], 0
    for _ in range(n):
        labels = np.frombuffer(blob, dtype="<i4", count=H * W, offset=off).reshape(H, W); off += 4 * H * W
        rec = np.frombuffer(blob, dtype="<i4", count=5, offset=off); off += 20
        cnt = np.frombuffer(blob, dtype="<i4", count=5, offset=off); off += 20
        d2 = np.frombuffer(blob, dtype=np.uint8, count=H * W, offset=off).reshape(H, W); off += H * W
        out.append(dict(labels=labels, root=int(rec[0]), area=int(rec[1]), steps=int(rec[2]), radius_index=int(rec[3]), survivors=int(rec[4]),
                        cnt=cnt, d2=d2))
    assert off == len(blob)
    return out


@pytest.mark.parametrize("shape", [(70, 90), (97, 131)])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_host_labelling_matches_scipy(host_check, tmp_path, shape, connectivity):
    fx = ref.label_masks(*shape)
    got = _run(host_check, tmp_path, list(fx.values()), connectivity)
    for (name, m), g in zip(fx.items(), got):
        want = ref.scipy_labels(m, connectivity)
        assert np.array_equal(ref.ranked(g["labels"]), want), name
        lab = g["labels"]
        u, first = np.unique(lab.ravel(), return_index=True)
        assert np.array_equal(u[u > 0] - 1, first[u > 0]), name          # label = 1 + raster index of the component's first pixel
        if want.max():
            area = np.bincount(want.ravel())[1:]
            assert g["area"] == area.max() and want.ravel()[g["root"]] == int(np.argmax(area)) + 1, name    # first maximum in scan order
        else:
            assert g["area"] == 0 and g["root"] == -1


def test_host_distance_and_chain_match_scipy(host_check, tmp_path):
    shapes = cases.erosion_shapes()
    got = _run(host_check, tmp_path, list(shapes.values()), 4)
    for (name, m), g in zip(shapes.items(), got):
        comp = ref.reference(np.ones(m.shape), np.eye(3), m)["component"]
        assert np.array_equal(g["d2"], ref.d2_capped(comp)), name        # the image border is not background
        d = ndimage.distance_transform_edt(comp)
        assert g["cnt"].tolist() == [int((d > r).sum()) for r in (8, 4, 2, 1, 0.5)], name
    c = cases.chain_case()
    got = _run(host_check, tmp_path, c["masks"], 4)
    assert [(g["radius_index"], g["survivors"]) for g in got] == cases.CHAIN_EXPECT
    assert all(g["steps"] == 5 for g in got)
    # other start radii: the chain stops after the first radius below 1
    for radius, steps in ((8.0, 5), (5.0, 4), (2.0, 3), (1.0, 2), (0.9, 1)):
        g = _run(host_check, tmp_path, c["masks"][:1], 4, radius=radius)[0]
        assert g["steps"] == steps
        r = ref.reference(c["depth"], c["K"], c["masks"][0], erosion_radius=radius)
        assert (g["radius_index"], g["survivors"]) == (r["radius_index"], r["survivors"]), radius


def _all_cases():
    out = dict(chain=cases.chain_case(), largest_tie=cases.largest_tie_case(), vga=cases.vga_case(), **cases.cut_cases())
    out.update({f"erosion_{r}": cases.erosion_case(r) for r in (8, 4, 2, 1, 0.5)})
    return out


def test_reference_is_the_production_host_function():
    """tests/_scale_ref.py returns exactly what scale_estimators.depthmap_scale returns on every fixture where no tie in |z - median|
    straddles the cut.  Two kinds of fixture are NOT of that kind (flag host_tie) and are compared by their sizes only: constant depth
    (the quirk keeps min_vertices of all-equal samples: which ones is the sort's choice) and the min_vertices clamp on quantised depth
    (n_keep cuts through samples at exactly the same distance).  There the reference pins (far, raster index); numpy's default argsort
    does not promise an order among equal keys.  The two-valued erosion fixtures carry the flag too: their ties lie inside the kept
    set, so the host keeps the same samples in another order and the scale agrees to the last places only."""
    from freepose_amd.src.pipeline.estimators import scale_estimators as se
    n_checked = 0
    for name, c in _all_cases().items():
        for i, m in enumerate(c["masks"]):
            r = ref.reference(c["depth"], c["K"], m, **c["kwargs"])
            pts = se.pointcloud_from_depth(c["depth"], c["K"], m, align=True, **c["kwargs"])
            assert pts.shape[0] == r["n_keep"], (name, i)
            assert ref.cut_is_clear(r), (name, i)
            if c["host_tie"]:
                far = np.sort(r["far"], kind="stable")
                if far[r["n_keep"] - 1] == far[r["n_keep"]]:       # a tie straddles the cut: the host's kept samples are the sort's choice
                    continue
                assert len(np.unique(far[:r["n_keep"]])) < r["n_keep"], (name, i)
                # ties inside the kept set only: the same samples in another order, i.e. the same sums in another order
                assert np.isclose(se.extent_scale(pts), r["scale"], rtol=1e-12, atol=0), (name, i)
                continue
            assert se.extent_scale(pts) == r["scale"], (name, i)
            n_checked += 1
            if c["scale"]:
                assert r["eig"][0] >= 2 * r["eig"][1] >= 4 * r["eig"][2] > 0, (name, i, r["eig"])
    assert n_checked >= 18
    assert [(ref.reference(c["depth"], c["K"], m)["radius_index"], ref.reference(c["depth"], c["K"], m)["survivors"])
            for c in [cases.chain_case()] for m in c["masks"]] == cases.CHAIN_EXPECT
    with pytest.raises(ValueError):
        ref.reference(np.ones((8, 8)), np.eye(3), np.zeros((8, 8), dtype=bool))


def test_erosion_fixture_keep_reveals_the_survivors():
    """what the GPU erosion test relies on: with the two-valued depth the kept set is the eroded mask minus the outlier pixels in it"""
    for radius in (8, 4, 2, 1, 0.5):
        c = cases.erosion_case(radius)
        for m in c["masks"]:
            r = ref.reference(c["depth"], c["K"], m, **c["kwargs"])
            assert r["survivors"] >= 2 and np.array_equal(r["keep"] | (r["survivor_mask"] & c["outliers"]), r["survivor_mask"])
            assert (r["survivor_mask"] & c["outliers"]).any()


def test_new_entry_points_are_declared_and_refuse_bad_arguments_without_a_gpu():
    import ctypes as C
    from freepose_amd import _lib
    lib = _lib.load()
    assert "fp_label_components" in _lib.SIGNATURES and "fp_depthmap_scale" in _lib.SIGNATURES
    assert lib.fp_label_components(None, None, 1, 4, 4, 4, None, None) == 1 and b"label_components" in lib.fp_last_error()
    assert lib.fp_depthmap_scale(None, None, None, 1, 4, 4, 1.0, 1.0, 0.0, 0.0, 8.0, 1.5, 25, 1, None, None, None, None) == 1
    assert b"depthmap_scale" in lib.fp_last_error()
    del C


def test_estimator_classes_and_cli_flag():
    import src.pipeline.estimators.scale_estimators as alias
    from freepose_amd.scripts import dino_inference as d
    from freepose_amd.src.pipeline.estimators import scale_estimators as se
    assert alias.MeanScaleEstimator is se.MeanScaleEstimator and alias.ConstantScaleEstimator is se.ConstantScaleEstimator
    assert alias.depthmap_scales is se.depthmap_scales
    assert se.ConstantScaleEstimator(0.3).estimate(None) == 0.3 and se.ConstantScaleEstimator(0.3).estimate(None, None, None) == 0.3
    e = se.MeanScaleEstimator(0.2)
    assert (e.mean_scale, e.svd) == (0.2, True) and se.MeanScaleEstimator(0.2, svd=False).svd is False
    ap = d.build_parser()
    assert ap.parse_args([]).scale_backend == "host" and ap.parse_args(["--scale_backend", "gpu"]).scale_backend == "gpu"
    with pytest.raises(SystemExit):
        ap.parse_args(["--scale_backend", "cpu"])
