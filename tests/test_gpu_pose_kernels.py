"""Every dispatch branch of the pose-side kernels (csrc/pose.hip) against the C oracle, bit for bit: the ten crop instantiations and
their store paths, depth_extents' vector / scalar loads, its <100 px fallback and its LDS budget, and the chunk seams of the geodesic
compaction.  No tolerance appears in this file: f32 and fp64 results are compared as bit patterns, bf16 results against
fo.to_bf16_bits of the oracle's f32 result."""
import numpy as np
import pytest
import torch

from tests import _crop_cases as cc

pytestmark = pytest.mark.gpu

N = len(cc.BOXES)
GUARD = 64          # elements of poison kept on both sides of an output buffer (a multiple of 16 bytes in both output types)


def _bits(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy().view(np.uint32)


def _want_bits(o: np.ndarray, bf16: bool) -> np.ndarray:
    from oracle import fp_oracle as fo
    return fo.to_bf16_bits(o) if bf16 else np.ascontiguousarray(o).view(np.uint32)


def _crop_into_poisoned(img, boxes, target, ext, masks, mode, bf16, div):
    """fp_crop_resize_pad through the C ABI into the middle of a buffer filled with 0xFF bytes (a NaN in both output types, which no
    crop holds).  Returns (output, guards): an output element no store reached keeps the poison — so a dropped store cannot hide
    behind what an earlier call left in recycled memory — and a store outside the crop shows in the guards."""
    from freepose_amd import _lib, ops
    lib = _lib.load()
    img_d, bx_d = torch.from_numpy(img).cuda(), torch.from_numpy(boxes).cuda()
    m_d = torch.from_numpy(masks).cuda() if masks is not None else None
    if img.dtype == np.uint8:
        n_img, H, W, C = img.shape
        src = 2 if div else 1
    else:
        n_img, C, H, W = img.shape
        src = 0
    Co = 1 if mode == 2 else C
    n = len(boxes)
    dt = torch.bfloat16 if bf16 else torch.float32
    numel = n * Co * target * target
    raw = torch.full(((numel + 2 * GUARD) * dt.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
    buf = raw.view(dt)
    out = buf[GUARD:GUARD + numel]
    ops.check(lib.fp_crop_resize_pad(ops.context(), ops.ptr(img_d), src, n_img, Co, H, W, ops.ptr(bx_d), n, float(ext), int(target),
                                     ops.ptr(m_d), int(mode), ops.ptr(out), int(bf16), ops.current_stream()), "fp_crop_resize_pad")
    torch.cuda.synchronize()
    return out.reshape(n, Co, target, target), torch.cat([buf[:GUARD], buf[GUARD + numel:]])


def _poison_bits(bf16):
    return 0xFFFF if bf16 else 0xFFFFFFFF


# ---- 1. crop dispatch matrix ------------------------------------------------------------------------------------------------------
# source kinds: "f32" [1,3,H,W] float | "u8n" [n,H,W,3] one image per box | "u8s" [1,H,W,3] shared | "u8c1" [1,H,W,1] | "u8c4" [1,H,W,4]
#        id               source  div    target bf16   mask ext
CROP_CASES = [
    ("rgb11_split30",     "u8n",  False, 30,    True,  0,   0.0),
    ("rgb11_split98",     "u8n",  False, 98,    True,  0,   0.2),
    ("rgb11_shared34",    "u8s",  False, 34,    True,  0,   0.2),
    ("rgb11_aligned32",   "u8s",  False, 32,    True,  0,   0.0),
    ("rgb10_split34",     "u8n",  False, 34,    False, 0,   0.2),
    ("rgb10_shared98",    "u8s",  False, 98,    False, 0,   0.0),
    ("rgb10_aligned64",   "u8n",  False, 64,    False, 0,   0.2),
    ("rgb21_split98",     "u8n",  True,  98,    True,  0,   0.2),
    ("rgb21_aligned64",   "u8n",  True,  64,    True,  0,   0.0),
    ("rgb20_split30",     "u8n",  True,  30,    False, 0,   0.0),
    ("rgb20_shared64",    "u8s",  True,  64,    False, 0,   0.2),
    ("gen00_odd31",       "f32",  False, 31,    False, 0,   0.0),
    ("gen00_mask1_98",    "f32",  False, 98,    False, 1,   0.2),
    ("gen00_mask2_65",    "f32",  False, 65,    False, 2,   0.0),
    ("gen01_odd65",       "f32",  False, 65,    True,  1,   0.2),
    ("gen01_packed64",    "f32",  False, 64,    True,  0,   0.0),
    ("gen01_mask2_30",    "f32",  False, 30,    True,  2,   0.2),
    ("gen10_odd31",       "u8n",  False, 31,    False, 0,   0.0),
    ("gen10_mask1_32",    "u8n",  False, 32,    False, 1,   0.2),
    ("gen10_c1_32",       "u8c1", False, 32,    False, 0,   0.0),
    ("gen10_shared65",    "u8s",  False, 65,    False, 0,   0.2),
    ("gen11_odd65",       "u8n",  False, 65,    True,  0,   0.0),
    ("gen11_mask2_34",    "u8n",  False, 34,    True,  2,   0.2),
    ("gen11_c4_30",       "u8c4", False, 30,    True,  0,   0.0),
    ("gen20_mask1_98",    "u8n",  True,  98,    False, 1,   0.2),
    ("gen20_c4_65",       "u8c4", True,  65,    False, 0,   0.0),
    ("gen20_mask2_64",    "u8s",  True,  64,    False, 2,   0.0),
    ("gen21_odd31",       "u8n",  True,  31,    True,  0,   0.0),
    ("gen21_mask1_32",    "u8n",  True,  32,    True,  1,   0.2),
    ("gen21_mask2_64",    "u8n",  True,  64,    True,  2,   0.2),
    ("gen21_c1_34",       "u8c1", True,  34,    True,  0,   0.2),
]


@pytest.fixture(scope="module")
def sources():
    return {"f32": cc.float_image(), "u8n": cc.u8_images(N, 3, 21), "u8s": cc.u8_images(1, 3, 22), "u8c1": cc.u8_images(1, 1, 23),
            "u8c4": cc.u8_images(1, 4, 24), "masks": cc.masks(N)}


def _oracle_crop(sources, kind, div, target, mode, ext, boxes=cc.BOXES, sel=None):
    from oracle import fp_oracle as fo
    img, m = sources[kind], (sources["masks"] if mode else None)
    if sel is not None:                   # one box alone: its own image (per-box sources) and its own mask
        img = img[sel:sel + 1] if img.shape[0] > 1 else img
        m = m[sel:sel + 1] if m is not None else None
        boxes = boxes[sel:sel + 1]
    return img, boxes, m, fo.crop_resize_pad(img, boxes, target, ext, m, mode, u8_float_div=div)   # raises if a box does not resize


@pytest.mark.parametrize("case", CROP_CASES, ids=[c[0] for c in CROP_CASES])
def test_crop_dispatch_matrix(sources, case):
    """fp_crop_resize_pad_launch sends a call to crop_rgb_kernel<U,O> when the source is u8 with 3 channels, no mask mode, an even
    target <= 2048 and W <= 32767, else to crop_kernel<U,O>; U = 0 float source, 1 u8 as float(double/255), 2 u8 as float/255.f
    (u8_float_div); O = 1 bf16 output.  Case -> kernel / branch (check any row against that dispatch):

      rgb11_split30, rgb11_split98   crop_rgb_kernel<1,1>  target % 4 == 2: odd rows take the split 4-byte stores ((o & 3) != 0), the
                                                           last group of every row the nval == 2 tail; per-box images
      rgb11_shared34                 crop_rgb_kernel<1,1>  same two branches, one shared image (n_img == 1, n > 1)
      rgb11_aligned32                crop_rgb_kernel<1,1>  target % 4 == 0: only the aligned 8-byte store; shared image
      rgb10_split34                  crop_rgb_kernel<1,0>  f32 split float2 stores and the float2 tail
      rgb10_shared98                 crop_rgb_kernel<1,0>  same, shared image
      rgb10_aligned64                crop_rgb_kernel<1,0>  aligned float4 store only
      rgb21_split98, rgb21_aligned64 crop_rgb_kernel<2,1>  u8_float_div without masks: split + tail, then aligned
      rgb20_split30, rgb20_shared64  crop_rgb_kernel<2,0>  u8_float_div, f32; the second with a shared image
      gen00_odd31                    crop_kernel<0,0>      float source, odd target (the last pair of a row is a single pixel)
      gen00_mask1_98, gen00_mask2_65 crop_kernel<0,0>      mask modes 1 and 2 (mode 2: one output channel)
      gen01_odd65                    crop_kernel<0,1>      odd target: o is odd on every other row -> scalar bf16 fallback, and the
                                                           single-pixel tail; mask mode 1
      gen01_packed64                 crop_kernel<0,1>      even target: only the packed uint32 store
      gen01_mask2_30                 crop_kernel<0,1>      mask mode 2
      gen10_odd31                    crop_kernel<1,0>      u8 double/255 reaches the generic kernel by an odd target
      gen10_mask1_32                 crop_kernel<1,0>      ... by a mask mode
      gen10_c1_32                    crop_kernel<1,0>      ... by C != 3 (C = 1)
      gen10_shared65                 crop_kernel<1,0>      odd target, shared image
      gen11_odd65                    crop_kernel<1,1>      scalar bf16 fallback on a u8 source
      gen11_mask2_34, gen11_c4_30    crop_kernel<1,1>      mask mode 2; C = 4
      gen20_mask1_98, gen20_mask2_64 crop_kernel<2,0>      the detection path beyond 56 px: mask modes 1 (ext 0.2) and 2
      gen20_c4_65                    crop_kernel<2,0>      C = 4, odd target
      gen21_odd31                    crop_kernel<2,1>      bf16 output, scalar fallback
      gen21_mask1_32, gen21_mask2_64 crop_kernel<2,1>      bf16 output, ext 0.2 with mask modes 1 and 2
      gen21_c1_34                    crop_kernel<2,1>      C = 1

    Targets 64 and 65 lie on the two sides of nearest_src's h1 + w1 <= 128 switch.  Both u8 conversions are exercised, but they cannot
    be told apart by value: float(double(b)/255) == float(b)/255.f for all 256 bytes (tests/test_crop_vs_torch_cpu.py pins that), so
    the assertion that the two expected outputs differ is not made."""
    from freepose_amd import ops
    _, kind, div, target, bf16, mode, ext = case
    img, boxes, m, want = _oracle_crop(sources, kind, div, target, mode, ext)
    if img.dtype == np.uint8:
        assert all(len(np.unique(im)) == 256 for im in img)
    want = _want_bits(want, bf16)
    got = ops.crop_resize_pad(torch.from_numpy(img), torch.from_numpy(boxes), target, ext, torch.from_numpy(m) if m is not None else None,
                              mode, out_bf16=bf16, u8_float_div=div)
    assert got.dtype == (torch.bfloat16 if bf16 else torch.float32) and tuple(got.shape) == want.shape
    assert np.array_equal(_bits(got), want), f"{case[0]}: boxes {np.unique(np.nonzero(_bits(got) != want)[0]).tolist()} differ"
    # the same call into a poisoned buffer: every element written (no poison left), nothing written around it
    out, guards = _crop_into_poisoned(img, boxes, target, ext, m, mode, bf16, div)
    gb = _bits(out)
    assert not (gb == _poison_bits(bf16)).any(), f"{case[0]}: {(gb == _poison_bits(bf16)).sum()} output elements were never stored"
    assert np.array_equal(gb, want)
    assert (_bits(guards) == _poison_bits(bf16)).all(), f"{case[0]}: a store landed outside the output"


ALONE_CASES = [c for c in CROP_CASES if c[0] in ("rgb11_split30", "rgb10_split34", "gen01_odd65", "gen10_odd31")]


@pytest.mark.parametrize("case", ALONE_CASES, ids=[c[0] for c in ALONE_CASES])
def test_crop_alone_equals_crop_in_batch(sources, case):
    """the vector stores of one crop write nothing into its neighbours: each box cropped alone (n = 1) equals its slice of the batch and
    the oracle's crop of that box — both output types of both kernels, at the targets whose rows are misaligned"""
    from freepose_amd import ops
    _, kind, div, target, bf16, mode, ext = case
    img, boxes, m, _ = _oracle_crop(sources, kind, div, target, mode, ext)
    batch = _bits(ops.crop_resize_pad(torch.from_numpy(img), torch.from_numpy(boxes), target, ext,
                                      torch.from_numpy(m) if m is not None else None, mode, out_bf16=bf16, u8_float_div=div))
    for i in range(N):
        img1, box1, m1, want1 = _oracle_crop(sources, kind, div, target, mode, ext, sel=i)
        one = _bits(ops.crop_resize_pad(torch.from_numpy(img1), torch.from_numpy(box1), target, ext,
                                        torch.from_numpy(m1) if m1 is not None else None, mode, out_bf16=bf16, u8_float_div=div))
        assert np.array_equal(one[0], batch[i]) and np.array_equal(one[0], _want_bits(want1, bf16)[0]), (case[0], i)


# ---- the two guards that keep a 3-channel u8 crop out of crop_rgb_kernel -----------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_crop_wide_image_takes_the_generic_kernel(bf16):
    """W = 32770 > 32767: crop_rgb_kernel tabulates source columns as `short`, so the dispatch must send this 3-channel u8 crop to
    crop_kernel<1,*>; boxes lie below, across and above column 32767 (x0 > 32767 included)"""
    from freepose_amd import ops
    from oracle import fp_oracle as fo
    Wb = 32770
    img = cc.rng(31).integers(0, 256, size=(1, 2, Wb, 3), dtype=np.uint8)
    boxes = np.array([[32740, 0, 32770, 2], [32768, 0, 32770, 2], [32750, 0, 32790, 2], [32760, 0, 32769, 1], [0, 0, 50, 2],
                      [32700, 0, 32760, 2], [32766, 0, 32769, 2]], dtype=np.int32)
    want = _want_bits(fo.crop_resize_pad(img, boxes, 32, 0.0), bf16)
    got = ops.crop_resize_pad(torch.from_numpy(img), torch.from_numpy(boxes), 32, 0.0, out_bf16=bf16)
    assert np.array_equal(_bits(got), want)
    out, guards = _crop_into_poisoned(img, boxes, 32, 0.0, None, 0, bf16, False)
    assert np.array_equal(_bits(out), want) and (_bits(guards) == _poison_bits(bf16)).all()


def test_crop_target_above_2048_takes_the_generic_kernel(sources):
    """target 2050 is even but crop_rgb_kernel's column table holds 2048 entries: the dispatch must fall back to crop_kernel<1,0>
    (one box, 50 MB of f32 output; the oracle needs about 0.2 s for it)"""
    from freepose_amd import ops
    from oracle import fp_oracle as fo
    img, box = sources["u8s"], cc.BOXES[:1]
    want = fo.crop_resize_pad(img, box, 2050, 0.0)
    got = ops.crop_resize_pad(torch.from_numpy(img), torch.from_numpy(box), 2050, 0.0)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---- 3. depth extents ----------------------------------------------------------------------------------------------------------------
EXT_SHAPES = [(5, 4), (7, 8), (33, 36), (3, 1028), (421, 420), (100, 7), (320, 316), (104, 104)]


def _first_pixels(Hh, W, k):
    """the first k pixels, row by row, of a window that starts at column 1, is at most 40 wide and leaves the last column free: their
    bounding box never reaches the fallback square's far corner (min(315, W) - 1, min(315, H) - 1), so the fallback changes it"""
    rw = max(1, min(W - 2, 40))
    assert k <= rw * Hh
    return np.arange(k) // rw, 1 + np.arange(k) % rw


def _extent_views(Hh, W, seed):
    """views of one shape and the expected count of each: 0 and 1 positive pixels, 99 / 100 / 101 where the shape holds them, and one
    dense view that also holds negative depths and -0.0f outside the positive region (4 views below 101 px, else 6)"""
    g = cc.rng(seed)
    counts = [0, 1] + ([99, 100, 101] if (max(1, min(W - 2, 40))) * Hh >= 101 else [])
    views = np.zeros((len(counts) + 1, Hh, W), dtype=np.float32)
    for v, k in enumerate(counts):
        ys, xs = _first_pixels(Hh, W, k)
        views[v, ys, xs] = g.uniform(0.3, 2.0, size=k).astype(np.float32)
    # dense + signed: positive in the left part, negatives and -0.0f in the rest, a few exact zeros everywhere
    d = g.uniform(0.3, 2.0, size=(Hh, W)).astype(np.float32)
    split = max(1, (2 * W) // 3)
    right = d[:, split:]
    right *= -1.0
    right[g.random(right.shape) < 0.4] = -0.0
    d[g.random((Hh, W)) < 0.1] = 0.0
    if W - split > 0:
        d[Hh - 1, W - 1] = -1.5                      # a negative corner: inside the extents, outside the box
    d[0, 0] = 0.7
    views[-1] = d
    return views, counts + [int((d > 0).sum())]


@pytest.mark.parametrize("Hh,W", EXT_SHAPES, ids=[f"{h}x{w}" for h, w in EXT_SHAPES])
def test_depth_extents_paths_and_fallback(Hh, W):
    """depth_extents_kernel reads float4s when W % 4 == 0 (5x4, 7x8, 33x36, 3x1028, 421x420, 320x316, 104x104) and scalars otherwise
    (100x7); 5x4 and 7x8 hold fewer pixels than the block has threads, no H*W here is a multiple of the block's 1024, and all but
    421x420 and 320x316 are smaller than the 105..314 fallback square in at least one direction.  The fallback square applies below
    100 positive pixels and not at 100; z != 0 (negatives too) enters the extents, only z > 0 the count and the box; -0.0f is empty."""
    from freepose_amd import ops
    from oracle import fp_oracle as fo
    views, counts = _extent_views(Hh, W, 100 + Hh)
    fx, fy, cx, cy = 600.5, 590.25, W / 2 + 0.375, Hh / 2 - 0.25      # all exact in float32 (the C ABI's type); cx, cy are no integers
    assert cx != int(cx) and cy != int(cy) and np.float32(cx) == cx and np.float32(cy) == cy and (Hh * W) % 1024 != 0
    e_o = fo.depth_extents(views, fx, fy, cx, cy)
    # the oracle's own result has the properties the inputs were built for
    assert e_o[:, 6].astype(int).tolist() == counts
    assert np.signbit(views).any() and (views[-1] < 0).any() and ((views[-1] == 0) & np.signbit(views[-1])).any()
    for v, k in enumerate(counts[:-1]):
        if k == 0:
            continue
        ys, xs = _first_pixels(Hh, W, k)
        tight = [xs.min(), ys.min(), xs.max(), ys.max()]
        assert (e_o[v, :4].tolist() != tight) == (k < 100), (k, e_o[v, :4], tight)
    pos = np.argwhere(views[-1] > 0)
    nz = np.argwhere(views[-1] != 0)
    if counts[-1] >= 100:
        assert e_o[-1, 2] == pos[:, 1].max() < nz[:, 1].max()          # the box stops at the last positive column, the negatives lie beyond
    assert e_o[-1, 4] > 0 and e_o[-1, 5] > 0
    e_g = ops.depth_extents(torch.from_numpy(views), fx, fy, cx, cy).cpu().numpy()
    assert np.array_equal(e_g.view(np.uint64), e_o.view(np.uint64)), (Hh, W, e_g, e_o)


def test_depth_extents_full_hd_frame():
    """1080 x 1920: H + W = 3000 > 1536.  The kernel's reduction keeps one partial per wave (under 1 KB of static LDS), so the
    [W] + [H] fp64 tables — 23.4 KB here — are all the LDS a launch needs and fit the 64 KB available without an opt-in."""
    from freepose_amd import ops
    from oracle import fp_oracle as fo
    g = cc.rng(41)
    d = np.zeros((1, 1080, 1920), dtype=np.float32)
    ys, xs = g.integers(300, 700, size=400), g.integers(1000, 1900, size=400)      # a sparse object right of and below the fallback square
    d[0, ys, xs] = g.uniform(0.4, 3.0, size=400).astype(np.float32)
    d[0, 1079, 1919] = 0.9
    d[0, 5, 1500] = -1.25
    e_o = fo.depth_extents(d, 1400.5, 1390.25, 960.375, 539.75)
    e_g = ops.depth_extents(torch.from_numpy(d), 1400.5, 1390.25, 960.375, 539.75).cpu().numpy()
    assert e_o[0, 6] >= 100 and e_o[0, 2] == 1919 and e_o[0, 3] == 1079
    assert np.array_equal(e_g.view(np.uint64), e_o.view(np.uint64)), (e_g, e_o)


def test_depth_extents_refuses_a_frame_beyond_its_lds_tables():
    """H + W > 8064 would need more than the 63 KB of dynamic LDS the host check allows: refused on the host, nothing is launched"""
    from freepose_amd import ops
    with pytest.raises(RuntimeError, match="depth_extents"):
        ops.depth_extents(torch.zeros((1, 1, 8100)), 600.0, 600.0, 4050.5, 0.5)
    ok = ops.depth_extents(torch.zeros((1, 1, 8063)), 600.0, 600.0, 4031.5, 0.5).cpu().numpy()       # the largest that fits: H + W = 8064
    assert ok[0, 6] == 0 and ok[0, 4] == 0


# ---- 4. geodesic compaction seams ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rotation_grids():
    from oracle import fp_oracle as fo
    return {G: fo.generate_rotations(G) for G in (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049)}


@pytest.mark.parametrize("thresh", [181.0, 0.0, 75.0], ids=["all", "none", "mid"])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049])
def test_geodesic_compaction_seams(rotation_grids, G, thresh):
    """compact_flags_kernel scans 1024 flags per pass (16 waves of 64) and carries the count: grid sizes around one wave, one pass and
    two passes; 181 degrees selects every index (each pass's carry is full), 0 none, 75 a scattered subset"""
    from freepose_amd import ops
    from oracle import fp_oracle as fo
    grid = rotation_grids[G]
    Rp = grid[G // 2]
    idx_o = fo.geodesic_select(grid, Rp, thresh)
    idx_g = ops.geodesic_select(torch.from_numpy(grid).cuda(), Rp, thresh)
    if thresh == 181.0:
        assert np.array_equal(idx_o, np.arange(G))
    elif thresh == 0.0:
        assert len(idx_o) == 0
    elif G >= 63:
        assert 0 < len(idx_o) < G
    assert idx_g.dtype == idx_o.dtype and np.array_equal(idx_g, idx_o)
