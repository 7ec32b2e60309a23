"""Every dispatch and set-up branch of the rasteriser (csrc/raster.hip) on the device, one small constructed scene per branch
(tests/_raster_cases.py; tests/test_raster_cases_cpu.py shows without a GPU that each case reaches the branches it claims and that the
oracle equals the integer known answer).  Per case and per strategy it runs under: the library's own plan (fp_op_raster_plan) is the case's,
every output byte is written, depth bits and colours equal the oracle's, the integer known answer holds (coverage, owner and colour
exactly, depth within DEPTH_ULP), the fused extents equal the oracle's bit for bit with and without the depth image, and all strategies
return the same bytes."""
import numpy as np
import pytest
import torch

from tests import _raster_cases as rc

pytestmark = pytest.mark.gpu

POISON_RGB = 0xAB


def _poisoned(case, want_depth=True):
    Hn, H, W = case.Hn, case.H, case.W
    rgb = torch.full((Hn, H, W, 3), POISON_RGB, dtype=torch.uint8, device="cuda")
    depth = torch.full((Hn, H, W), float("nan"), dtype=torch.float32, device="cuda") if want_depth else None
    return rgb, depth


def _assert_plan(case, mode, ops):
    want = rc.plan(case.W, case.H, rc.n_faces(case), case.Hn, mode)
    got = ops.raster_plan(case.W, case.H, rc.n_faces(case), case.Hn)
    got.pop("text")
    assert got["constants"] == want["constants"], f"the case table is stale: the library was compiled with {got['constants']}, the table computed with {want['constants']}"
    assert got == want, f"the case table is stale: {case.name} under raster_tiled={mode}: the library plans {got}, the table {want}"
    assert rc.launch_labels(case.W, case.H, rc.n_faces(case), case.Hn, mode) <= rc.classify(case)


def _assert_written(rgb, depth, what):
    assert not torch.isnan(depth).any().item(), (what, "depth pixels left unwritten")
    # a colour byte may legitimately equal the poison value only where the known answer / the oracle says so: compared below, byte for byte


def _assert_known(case, rgb, depth, what):
    for view in range(case.Hn):
        covered, owner, d_known, _ = rc.known_answer(case, view)
        assert np.array_equal(depth[view] > 0, covered) and np.array_equal(depth[view] != 0, covered), (what, view, "coverage differs from the integer answer")
        assert np.array_equal(rgb[view], rc.expected_rgb(owner)), (what, view, "owner / colour differs from the integer answer")
        if covered.any():
            dev = int(rc.depth_ulps(depth[view], d_known)[covered].max())
            assert dev <= rc.DEPTH_ULP, (what, view, f"depth {dev} ulp from the plane depth")


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.id)
def test_raster_branch_case(case):
    from freepose_amd import ops
    from oracle import fp_oracle as fo
    v, f, c = rc.mesh(case)
    mesh = ops.Mesh(v, f, c).set_shading(0).set_ambient(1.0).set_cull(case.cull)
    poses = torch.from_numpy(rc.poses(case))
    K = rc.intrinsics(case)
    rgb_o, d_o = rc.oracle_render(case)
    ext_o = fo.depth_extents(d_o, *K) if case.extents else None
    results = {}
    for mode in case.modes:
        what = (case.name, f"raster_tiled={mode}")
        ops.set_option("raster_tiled", mode)
        try:
            _assert_plan(case, mode, ops)
            rgb_t, d_t = ops.rasterize(mesh, poses, 1.0, *K, case.W, case.H, out=_poisoned(case))
            _assert_written(rgb_t, d_t, what)
            rgb, depth = rgb_t.cpu().numpy(), d_t.cpu().numpy()
            assert np.array_equal(depth.view(np.uint32), d_o.view(np.uint32)), (what, "depth bits differ from the oracle")
            assert np.array_equal(rgb, rgb_o), (what, "colours differ from the oracle")
            if case.known:
                _assert_known(case, rgb, depth, what)
            results[mode] = (rgb, depth)
            if case.extents:
                for want_depth in (True, False):
                    out_rgb, out_d = _poisoned(case, want_depth)
                    ext_p = torch.full((case.Hn, 8), float("nan"), dtype=torch.float64, device="cuda")
                    box_p = torch.full((case.Hn, 4), -12345, dtype=torch.int32, device="cuda")
                    rgb_f, d_f, ext_f, box_f = ops.rasterize_extents(mesh, poses, 1.0, *K, case.W, case.H, want_depth=want_depth,
                                                                     out=(out_rgb, out_d, ext_p, box_p))
                    assert np.array_equal(rgb_f.cpu().numpy(), rgb_o), (what, want_depth, "fused: colours")
                    assert np.array_equal(ext_f.cpu().numpy().view(np.uint64), ext_o.view(np.uint64)), (what, want_depth, ext_f.cpu().numpy(), ext_o)
                    assert np.array_equal(box_f.cpu().numpy(), ext_o[:, :4].astype(np.int32)), (what, want_depth, "fused: boxes")
                    assert (d_f is None) == (not want_depth)
                    if want_depth:
                        assert np.array_equal(d_f.cpu().numpy().view(np.uint32), d_o.view(np.uint32)), (what, "fused: depth bits")
            if "views-groups+rem" in case.claims:                           # determinism: a second call returns the same bytes
                rgb_2, d_2 = ops.rasterize(mesh, poses, 1.0, *K, case.W, case.H, out=_poisoned(case))
                assert torch.equal(rgb_2, rgb_t) and torch.equal(d_2.view(torch.int32), d_t.view(torch.int32)), (what, "two calls differ")
        finally:
            ops.set_option("raster_tiled", -1)
    first = results[case.modes[0]]
    for mode in case.modes[1:]:
        assert np.array_equal(results[mode][0], first[0]) and np.array_equal(results[mode][1].view(np.uint32), first[1].view(np.uint32)), \
            (case.name, f"raster_tiled={mode} and {case.modes[0]} return different bytes")
