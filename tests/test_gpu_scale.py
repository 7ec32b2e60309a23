"""Depth-map object scale on the device (csrc/scale.hip: fp_label_components, fp_depthmap_scale) against scipy and tests/_scale_ref.py.

Everything up to the kept pixel set is discrete and compared exactly: labels (ranked canonical labels == scipy.ndimage.label), the
chosen component, the index of the erosion radius, the survivor count, n_keep and the keep mask.  The capped d^2 image itself stays
inside the call; it is held through the survivor sets of every radius of the chain (the two-valued depth of _scale_cases.erosion_case
makes the keep mask reveal them) and, value by value, by the host program of tests/test_scale_host_cpu.py, which runs the same
recurrences.  Only the scale is floating point.

SCALE: largest relative difference |device - reference| / reference over the scale fixtures (odd, even, quantised, outlier at 70 x 90 and
the five 480 x 640 proposals, align on and off), measured on an MI355X: 7.9e-16 (odd, align on; 0 with align off: the
extent then involves no sum) — see SCALE_RTOL."""
import functools
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import _scale_cases as cases
from tests import _scale_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

SCALE_RTOL = 7.9e-15      # ten times the largest relative difference measured over the scale fixtures (module docstring)
SCALE_BUG = 1e-9          # a difference above this is a bug to find, whatever was measured


@functools.lru_cache(maxsize=None)
def _case(name):
    if name.startswith("erosion_"):
        return cases.erosion_case(float(name.split("_")[1]))
    table = dict(chain=cases.chain_case, largest_tie=cases.largest_tie_case, vga=cases.vga_case)
    return table[name]() if name in table else cases.cut_cases()[name]


@functools.lru_cache(maxsize=None)
def _refs(name, align=True):
    """the reference of every mask of a case, computed once and shared by the tests"""
    c = _case(name)
    return tuple(ref.reference(c["depth"], c["K"], m, align=align, **c["kwargs"]) for m in c["masks"])


def _device(name, align=True):
    from freepose_amd import ops
    c = _case(name)
    s, info, keep = ops.depthmap_scales(torch.from_numpy(c["depth"]), torch.from_numpy(c["masks"]), c["K"], align=align, return_keep=True,
                                        **c["kwargs"])
    return s.cpu().numpy(), info.cpu().numpy(), keep.cpu().numpy().astype(bool)


def _assert_discrete(name, info, keep):
    for i, r in enumerate(_refs(name)):
        assert ref.cut_is_clear(r), (name, i)       # no |z - median| within 1e-9 of the threshold: the last bit of sigma cannot move the count
        assert info[i].tolist() == [r["area"], r["radius_index"], r["survivors"], r["n_keep"]], (name, i, info[i])
        assert np.array_equal(keep[i], r["keep"]), (name, i)


# ---- labelling --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(70, 90), (97, 131)])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_labels_are_scipys(shape, connectivity):
    """empty, single pixel, full, checkerboard, diagonal chain, serpentine, spiral, blobs touching across a tile corner, random masks at
    densities 0.3 / 0.5 / 0.59: ranked canonical labels == scipy.ndimage.label, in one call of n = 7 and in calls of n = 1"""
    from freepose_amd import ops
    fx = ref.label_masks(*shape)
    names = list(fx)
    batch = ops.label_components(torch.from_numpy(np.stack([fx[k] for k in names[:7]])), connectivity).cpu().numpy()
    assert batch.shape == (7, *shape) and batch.dtype == np.int32
    singles = [ops.label_components(torch.from_numpy(fx[k]), connectivity).cpu().numpy() for k in names[7:]]      # [H,W] in, [H,W] out
    for name, got in zip(names, list(batch) + singles):
        want = ref.scipy_labels(fx[name], connectivity)
        assert np.array_equal(ref.ranked(got), want), name
        u, first = np.unique(got.ravel(), return_index=True)
        assert np.array_equal(u[u > 0] - 1, first[u > 0]), name          # label = 1 + raster index of the component's first pixel
    H, W = shape
    if connectivity == 4:
        assert ref.ranked(batch[names.index("checkerboard")]).max() == (H * W + 1) // 2      # every pixel its own component
    else:
        assert ref.ranked(batch[names.index("checkerboard")]).max() == 1
    again = ops.label_components(torch.from_numpy(np.stack([fx[k] for k in names[:7]])), connectivity).cpu().numpy()
    assert np.array_equal(again, batch)


def test_largest_component_ties_go_to_the_first_in_scan_order():
    s, info, keep = _device("largest_tie")
    _assert_discrete("largest_tie", info, keep)
    H, W = 70, 90
    first = [cases.rect(H, W, 5, 40, 6, 7), cases.rect(H, W, 36, 10, 6, 7), cases.rect(H, W, 20, 70, 6, 7)]
    for i in range(3):
        assert info[i, 0] == 42 and keep[i].any() and not (keep[i] & ~first[i]).any(), i      # the tie partner (another tile) is never touched


# ---- erosion ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [8, 4, 2, 1, 0.5])
def test_survivor_masks_are_the_distance_transform_threshold(radius):
    """a component on the image border and in its corner (the border is not background), one-pixel holes, a ring thinner than 16: with
    each radius of the chain as the first one, survivor count and survivor mask == distance_transform_edt > r"""
    name = f"erosion_{radius}"
    c = _case(name)
    s, info, keep = _device(name)
    _assert_discrete(name, info, keep)
    steps = {8: 5, 4: 4, 2: 3, 1: 2, 0.5: 1}[radius]                   # radii tried from this start: r, r / 2, ... down to the first below 1
    for i, r in enumerate(_refs(name)):
        k = int(info[i, 1])
        want = ndimage.distance_transform_edt(r["component"]) > radius / 2 ** k if k < steps else r["component"]
        assert np.array_equal(keep[i] | (want & c["outliers"]), want), (radius, i)
        assert info[i, 2] == int(want.sum()) and (want & c["outliers"]).any()


def test_every_step_of_the_fallback_chain():
    """exactly 25 survivors are not enough, 26 are; radius 8 -> 4 -> 2 -> 1 -> 0.5 -> the un-eroded component of 24 pixels (n_keep
    clipped to 24)"""
    s, info, keep = _device("chain")
    assert [tuple(x) for x in info[:, 1:3].tolist()] == cases.CHAIN_EXPECT
    assert info[5].tolist() == [24, 5, 24, 24] and np.array_equal(keep[5], _case("chain")["masks"][5])
    _assert_discrete("chain", info, keep)


# ---- cut --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["odd", "even", "quirk_constant", "quantised", "outlier", "clamp_ties"])
def test_cut_and_keep_mask(name):
    s, info, keep = _device(name)
    _assert_discrete(name, info, keep)
    r = _refs(name)[0]
    if name == "odd":
        assert r["survivors"] % 2 == 1
    if name == "even":
        assert r["survivors"] % 2 == 0
    if name == "quirk_constant":      # no sample beyond the threshold: argmax of all-False is 0 -> min_vertices samples, the first in raster order
        rows, cols = np.nonzero(r["survivor_mask"])
        want = np.zeros_like(keep[0])
        want[rows[:25], cols[:25]] = True
        assert info[0, 3] == 25 and np.array_equal(keep[0], want)
    if name == "quantised":           # ties in |z - median| on both sides of the median, all inside the cut
        c = _case(name)
        z = c["depth"][r["survivor_mask"]]
        med = np.median(z)
        far_lo, far_hi = np.abs(z[z < med] - med), np.abs(z[z > med] - med)
        assert len(np.intersect1d(far_lo, far_hi)) > 3
    if name == "outlier":
        assert not keep[0, 33, 47] and r["survivor_mask"][33, 47]
    if name == "clamp_ties":          # 23 within the threshold -> clamped to 25: the first two of the 17 tied samples in raster order
        c = _case(name)
        tied = np.abs(c["depth"] - 1.0) == 0.25
        rows, cols = np.nonzero(tied & r["survivor_mask"])
        assert info[0].tolist() == [40, 4, 40, 25] and len(rows) == 17
        assert (keep[0] & tied).sum() == 2 and keep[0, rows[0], cols[0]] and keep[0, rows[1], cols[1]]


# ---- scale ------------------------------------------------------------------------------------------------------------------------------
def test_scale_against_the_reference_and_bit_repeatable():
    """discrete outputs equal; the scale within SCALE_RTOL = 10 x the largest relative difference measured on an MI355X over exactly
    these fixtures (7.9e-16, with align on and off) and, as a condition of its own, within 1e-9; two calls return identical bits.  The
    fixtures keep the scatter matrix's eigenvalues apart by a ratio >= 2, so the difference measures arithmetic, not conditioning."""
    worst = 0.0
    for name in ("odd", "even", "quantised", "outlier", "vga"):
        assert _case(name)["scale"]
        for align in (True, False):
            s, info, keep = _device(name, align)
            s2, info2, keep2 = _device(name, align)
            assert s.tobytes() == s2.tobytes() and np.array_equal(info, info2) and np.array_equal(keep, keep2)
            _assert_discrete(name, info, keep)
            for i, r in enumerate(_refs(name, align)):
                if align:
                    assert r["eig"][0] >= 2 * r["eig"][1] >= 4 * r["eig"][2] > 0, (name, i, r["eig"])
                rel = abs(s[i] - r["scale"]) / r["scale"]
                print(f"scale {name}[{i}] align={int(align)} device={s[i]!r} reference={r['scale']!r} rel={rel:.3e}")
                worst = max(worst, rel)
    print(f"scale: largest relative difference {worst:.3e}")
    assert worst <= SCALE_BUG, worst
    assert worst <= SCALE_RTOL, worst


# ---- API --------------------------------------------------------------------------------------------------------------------------------
def test_mean_scale_estimator_is_its_definition():
    from freepose_amd.src.pipeline.estimators.scale_estimators import ConstantScaleEstimator, MeanScaleEstimator, depthmap_scales
    c = _case("vga")
    proposals = SimpleNamespace(masks=[torch.from_numpy(m) for m in c["masks"][:3]])
    for svd in (True, False):
        raw = np.array([r["scale"] for r in _refs("vga", svd)[:3]])
        want = raw * (0.2 / (2 * np.mean(raw)))                      # reference scale_estimators.py:25-32
        got = MeanScaleEstimator(0.2, svd=svd).estimate(proposals, c["depth"], c["K"])
        assert got.shape == (3,) and got.dtype == np.float64
        assert np.allclose(got, want, rtol=SCALE_RTOL, atol=0)
        assert np.isclose(2 * got.mean(), 0.2, rtol=1e-14)
    assert np.allclose(depthmap_scales(c["depth"], c["K"], c["masks"]), [r["scale"] for r in _refs("vga")], rtol=SCALE_RTOL, atol=0)
    assert ConstantScaleEstimator(0.3).estimate(proposals, c["depth"], c["K"]) == 0.3


def test_empty_mask_raises_value_error():
    from freepose_amd import ops
    c = _case("odd")
    masks = np.concatenate([c["masks"], np.zeros_like(c["masks"])])
    with pytest.raises(ValueError, match="empty proposal mask"):
        ops.depthmap_scales(torch.from_numpy(c["depth"]), torch.from_numpy(masks), c["K"])
    assert ops.label_components(torch.zeros((1, 33, 65), dtype=torch.uint8)).sum().item() == 0


def test_c_abi_refuses_bad_arguments():
    """connectivity not 4 or 8, H or W < 1, n < 0, a NULL required pointer: status 1 and a message; nothing is written"""
    from freepose_amd import _lib, ops
    lib, ctx, st = _lib.load(), ops.context(), _lib.current_stream()
    H, W = 8, 9
    m = torch.ones((2, H, W), dtype=torch.uint8, device="cuda")
    lab = torch.full((2, H, W), -7, dtype=torch.int32, device="cuda")
    p = _lib.ptr
    for args in ((ctx, p(m), 2, H, W, 6, p(lab), st), (ctx, p(m), 2, 0, W, 4, p(lab), st), (ctx, p(m), 2, H, 0, 8, p(lab), st),
                 (ctx, p(m), -1, H, W, 4, p(lab), st), (ctx, None, 2, H, W, 4, p(lab), st), (ctx, p(m), 2, H, W, 4, None, st),
                 (None, p(m), 2, H, W, 4, p(lab), st)):
        assert lib.fp_label_components(*args) == 1 and b"label_components" in lib.fp_last_error(), args[2:6]
    d = torch.ones((H, W), dtype=torch.float64, device="cuda")
    sc = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    info = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")
    good = [ctx, p(d), p(m), 2, H, W, 100.0, 100.0, 4.0, 4.0, 8.0, 1.5, 25, 1, p(sc), p(info), None, st]
    for pos, bad in ((0, None), (1, None), (2, None), (14, None), (15, None), (3, -1), (4, 0), (5, 0), (10, 0.0), (10, 9.0), (12, 0), (13, 2)):
        args = list(good)
        args[pos] = bad
        assert lib.fp_depthmap_scale(*args) == 1 and b"depthmap_scale" in lib.fp_last_error(), pos
    torch.cuda.synchronize()
    assert (lab == -7).all() and (sc == -7).all() and (info == -7).all()
    assert lib.fp_label_components(ctx, p(m), 0, H, W, 4, p(lab), st) == 0 and (lab == -7).all()       # n = 0: nothing to do


def test_dino_inference_scale_backend_gpu(tmp_path, monkeypatch):
    """`--depth_method depthmap --scale_backend gpu` on the synthetic BOP scene of the CLI end-to-end test: the same rows as the host
    backend, the scale column within SCALE_RTOL"""
    import pandas as pd
    from tests import _synth_scene as sc
    n_views, model = 64, "dinov2_vits14_reg"
    root = tmp_path
    sc.write_meshes(root)
    assert sc.render_shards(root, n_views).exists()
    frames, props, gts, K = sc.draw_frames(root, 2, n_views)
    sc.write_bop(root, "synth", frames, props, K, depths=sc.draw_frames.depths[:2])
    monkeypatch.chdir(root)
    monkeypatch.setenv("SLURM_ARRAY_TASK_ID", "0")
    from scripts import dino_inference
    argv = ["--dataset", "synth", "--proposals", "props.json", "--n_views", str(n_views), "--model", model, "--bbox_extend", "0.05",
            "--allow_random_weights", "--depth_method", "depthmap"]
    host = pd.read_csv(dino_inference.run(argv + ["--scale_backend", "host"]))
    text_default = pd.read_csv(dino_inference.run(argv)).to_csv(index=False)
    assert text_default == host.to_csv(index=False)                     # the default is the host backend
    gpu = pd.read_csv(dino_inference.run(argv + ["--scale_backend", "gpu"]))
    assert len(gpu) == len(host) == 4
    for col in ("scene_id", "im_id", "obj_id", "bbox_visib", "time"):
        assert gpu[col].tolist() == host[col].tolist(), col
    for a, b in zip(gpu.itertuples(), host.itertuples()):            # the poses follow the scale: equal to the places the scale is
        assert np.isclose(a.score, b.score, rtol=1e-5)
        for col in ("R", "t"):
            assert np.allclose([float(x) for x in getattr(a, col).split()], [float(x) for x in getattr(b, col).split()], rtol=1e-6, atol=1e-9)
    rel = np.abs(gpu["scale"].to_numpy() - host["scale"].to_numpy()) / host["scale"].to_numpy()
    print("dino_inference scale column, gpu against host, relative:", rel.tolist())
    assert (rel <= SCALE_RTOL).all(), rel
