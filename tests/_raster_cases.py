"""Constructed scenes for the rasteriser (csrc/raster.hip): one small scene per dispatch and set-up branch, each with an answer written in
integer arithmetic, and a classifier that says which branches a scene really reaches.  Importable without a GPU.

Construction.  Identity rotation, t = (k / 256, 0, 1), scale 1, fx = fy = 256, integer principal point (cx, cy).  A vertex that should land
on fixed-point window coordinate (xi, yi) (1/256 px) at camera depth zc (a power of two) is stored as
    ((xi - 256 cx) / 65536 * zc, (yi - 256 cy) / 65536 * zc, zc - 1):
every step of the vertex stage is then exact in float32 and fp_project_vertices returns (xi + 256 k / zc, yi) — tests/test_raster_cases_cpu.py
asserts it for every case and view.  Colours are flat per triangle (three private vertices) and encode face id + 1 in their three bytes;
with set_shading(0) and set_ambient(1.0) the output byte is the colour byte.

Known answer (known_answer): pixel centre (256 px + 128, 256 py + 128), the three edge functions in integers after the orientation swap,
the top-left rule on zeros, the nearest plane wins, equal planes go to the lower face id.  It never calls the oracle and shares no code with
it.  Near-plane straddlers have no integer answer; the cases that hold them are compared with the oracle only (Case.known False).

classify() restates tri_setup_v (csrc/raster_core.h) on the integers for every triangle and view and, with plan() — the mirror of
csrc/raster_plan.h make_plan — gives the set of branch LABELS a case reaches.  The thresholds are read from raster_plan.h itself
(CONSTANTS), never copied: the GPU test holds them to the ones the library was compiled with (ops.raster_plan)."""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass
from fractions import Fraction
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def _read_constants():
    """every `constexpr int|float NAME = <arithmetic>;` of csrc/raster_plan.h"""
    text = (ROOT / "freepose_amd" / "csrc" / "raster_plan.h").read_text()
    out = {}
    for kind, name, expr in re.findall(r"^constexpr\s+(int|float)\s+(\w+)\s*=\s*([^;]+);", text, flags=re.M):
        expr = expr.strip()
        assert re.fullmatch(r"[0-9\s*+\-.f]+", expr), (name, expr)
        val = eval(re.sub(r"(?<=[0-9.])f", "", expr), {"__builtins__": {}})   # digits and operators only (asserted above)
        out[name] = float(np.float32(val)) if kind == "float" else int(val)
    return out


CONSTANTS = _read_constants()
ZNEAR, CLAMP_PX, SMALL_SPAN = CONSTANTS["ZNEAR"], int(CONSTANTS["CLAMP_PX"]), CONSTANTS["SMALL_SPAN"]
BIG_AREA, BIG_TILE_AREA = CONSTANTS["BIG_AREA"], CONSTANTS["BIG_TILE_AREA"]
BIN_CHUNK, BIN_WAVES, HITS_ROUND = CONSTANTS["BIN_CHUNK"], CONSTANTS["BIN_WAVES"], CONSTANTS["HITS_ROUND"]
TILE_MIN, TILE_MAX, TILES_SIDE, TILED_MAX_TRIS = CONSTANTS["TILE_MIN"], CONSTANTS["TILE_MAX"], CONSTANTS["TILES_SIDE"], CONSTANTS["TILED_MAX_TRIS"]
# the constants fp_op_raster_plan reports, under the names it reports them by
REPORTED = {"big_area": BIG_AREA, "big_tile_area": BIG_TILE_AREA, "chunk": BIN_CHUNK, "hits_round": HITS_ROUND, "small_span": SMALL_SPAN,
            "max_tris": TILED_MAX_TRIS, "max_tile": TILE_MAX, "clamp": CLAMP_PX, "znear": float(f"{ZNEAR:g}")}   # (znear as "%g" prints it)

# Largest deviation, in float32 units in the last place, of the ORACLE's depth from the integer answer's plane depth over the case table
# (measured and asserted by tests/test_raster_cases_cpu.py; it must not exceed 4: three correctly rounded quotients that sum to 1 within
# 1.5 ulp, one fma chain, one reciprocal).  Measured: 2 (the backdrops of the seam scenes, the sloped planes).  The GPU test allows the
# kernels the same.
DEPTH_ULP = 2

FX = 256.0
IZS = 64          # 1 / zc in units of 1 / IZS: zc is a power of two in [1 / 16, 64]


def cdiv(a, b):
    return -(-a // b)


# ---- the launch plan: mirror of csrc/raster_plan.h make_plan (held to the header by tools/raster_plan_host_check.cpp in the CPU test)
def plan(W, H, F, Hn, mode):
    side = max(W, H)
    T = TILE_MIN if side <= TILE_MIN * TILES_SIDE else (cdiv(side, TILES_SIDE) + 7) // 8 * 8
    tiled = T <= TILE_MAX and (mode == 1 or (mode != 0 and F <= TILED_MAX_TRIS))
    p = {"path": "tiled" if tiled else "global", "T": T, "tiles": (0, 0), "chunks": 0, "rounds": 0, "bin": 0, "views": (Hn >> 3, Hn & 7),
         "flush": "none", "lds": 0, "constants": dict(REPORTED)}
    if tiled:
        nchunk = cdiv(F, BIN_CHUNK)
        p.update(tiles=(cdiv(W, T), cdiv(H, T)), chunks=nchunk, rounds=cdiv(nchunk, HITS_ROUND), bin=cdiv(nchunk, BIN_WAVES),
                 flush="dword" if W % 4 == 0 else "bytes", lds=T * T * 8 + 2048 + HITS_ROUND * 2 + 2 * T * 8)
    return p


def parse_plan(text):
    """the dict of plan() from one line of fp_op_raster_plan / tools/raster_plan_host_check.cpp"""
    path, *fields = text.split()
    kv = dict(f.split("=") for f in fields)
    p = {"path": path, "T": int(kv.pop("T")), "tiles": tuple(int(v) for v in kv.pop("tiles").split("x")), "chunks": int(kv.pop("chunks")),
         "rounds": int(kv.pop("rounds")), "bin": int(kv.pop("bin")), "views": tuple(int(v) for v in kv.pop("views").split("+")),
         "flush": kv.pop("flush"), "lds": int(kv.pop("lds"))}
    p["constants"] = {k: (float(v) if k == "znear" else int(v)) for k, v in kv.items()}
    return p


def launch_labels(W, H, F, Hn, mode):
    p = plan(W, H, F, Hn, mode)
    out = set()
    if p["path"] == "tiled":
        T, (ntx, nty) = p["T"], p["tiles"]
        out.add(f"tiled-T{T}")
        out.add("tiles-exact-x" if W % T == 0 else "tiles-partial-x")
        out.add("tiles-exact-y" if H % T == 0 else "tiles-partial-y")
        out.add("flush-dword" if p["flush"] == "dword" else f"flush-bytes-w{W % 4}")
        if mode < 0 and F == TILED_MAX_TRIS:
            out.add("tiled-at-count-limit")
        out.add("chunks-1-partial" if F < BIN_CHUNK else "chunks-exact" if F % BIN_CHUNK == 0 else "chunks-tail")
        if p["chunks"] % BIN_WAVES:
            out.add("bin-grid-tail")
        if p["chunks"] == HITS_ROUND:
            out.add("rounds-1-full")
        if p["rounds"] >= 2:
            out.add("rounds-2")
        if p["bin"] > 1 and p["views"][0] > 0 and p["views"][1] > 0:
            out.add("views-bin-grid")                                  # the bin kernel's own view-major walk over more than one workgroup per view
    else:
        if p["T"] > TILE_MAX:
            out.add("global-by-size")
        elif mode == 0:
            out.add("global-forced")
        else:
            out.add("global-by-count")
    g, r = p["views"]
    out.add("views-lt8" if g == 0 else "views-groups-only" if r == 0 else "views-groups+rem")
    if g:
        out.add(f"views-{Hn}")
    return out


# ---- tri_setup_v on integers, vectorised over triangles (held to csrc/raster_core.h by tools/raster_core_host_check.cpp in the CPU test) -------
@dataclass
class Setup:
    W: int
    H: int
    nfront: np.ndarray
    strad: np.ndarray
    ok: np.ndarray
    swapped: np.ndarray
    area2: np.ndarray
    x: np.ndarray          # [F,3] after the orientation swap
    y: np.ndarray
    k: np.ndarray          # [F,3] which original corner sits at each place after the swap
    bbox: np.ndarray       # [F,4] bx0, by0, bx1, by1 (clipped, inclusive)
    ubox: np.ndarray       # [F,4] the same before clipping to the frame
    small: np.ndarray
    span: np.ndarray       # max of the x and y vertex spans (subpixels)
    culled: np.ndarray     # back face under cull = 1 (straddlers: never judged here)


def setup(xi, yi, zc, W, H, cull=0):
    """xi, yi int [F,3] (fixed-point window coordinates, already clamped), zc float [F,3] -> Setup (raster_core.h tri_setup_v)"""
    xi, yi = np.asarray(xi, np.int64), np.asarray(yi, np.int64)
    front = np.asarray(zc, np.float32) > np.float32(ZNEAR)
    nfront = front.sum(1)
    strad = (nfront == 1) | (nfront == 2)
    area2 = (xi[:, 1] - xi[:, 0]) * (yi[:, 2] - yi[:, 0]) - (yi[:, 1] - yi[:, 0]) * (xi[:, 2] - xi[:, 0])
    swapped = (area2 < 0) & ~strad
    k = np.tile(np.array([0, 1, 2]), (xi.shape[0], 1))
    k[swapped] = [0, 2, 1]
    x, y = np.take_along_axis(xi, k, 1), np.take_along_axis(yi, k, 1)
    mnx, mxx, mny, mxy = xi.min(1), xi.max(1), yi.min(1), yi.max(1)
    ubox = np.stack([(mnx - 128 + 255) >> 8, (mny - 128 + 255) >> 8, (mxx - 128) >> 8, (mxy - 128) >> 8], 1)
    bbox = np.stack([np.maximum(0, ubox[:, 0]), np.maximum(0, ubox[:, 1]), np.minimum(W - 1, ubox[:, 2]), np.minimum(H - 1, ubox[:, 3])], 1)
    ok = (nfront == 3) & (area2 != 0) & (bbox[:, 2] >= bbox[:, 0]) & (bbox[:, 3] >= bbox[:, 1])
    small = ((mxx - mnx) < SMALL_SPAN) & ((mxy - mny) < SMALL_SPAN) & ~strad
    full = np.array([0, 0, W - 1, H - 1])
    bbox[strad] = full
    ok = ok | strad
    culled = ok & ~strad & ~swapped if cull else np.zeros_like(ok)
    return Setup(W, H, nfront, strad, ok, swapped, np.abs(area2), x, y, k, bbox, ubox, small, np.maximum(mxx - mnx, mxy - mny), culled)


def _topleft(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


def _edges(s: Setup, ids, px, py):
    """edge functions of triangles `ids` at pixels (px, py) (arrays of the same length): w [n,3], covered [n], on_edge [n]"""
    sx, sy = px * 256 + 128, py * 256 + 128
    x, y = s.x[ids], s.y[ids]
    w, tl = [], []
    for a, b in ((1, 2), (2, 0), (0, 1)):                              # the edge opposite corner 0, 1, 2
        dx, dy = x[:, b] - x[:, a], y[:, b] - y[:, a]
        w.append(dx * (sy - y[:, a]) - dy * (sx - x[:, a]))
        tl.append(_topleft(dx, dy))
    w, tl = np.stack(w, 1), np.stack(tl, 1)
    inside = (w >= 0).all(1)
    return w, inside & ((w != 0) | tl).all(1), inside & (w == 0).any(1)


def fragments(s: Setup):
    """every (pixel, triangle) whose centre the triangle covers, straddlers and culled faces left out: dict of arrays pix (py * W + px),
    f, w [n,3], and edge_pix / edge_f: the (pixel, triangle) pairs with the centre exactly ON an edge (covered or not)"""
    ids = np.nonzero(s.ok & ~s.strad & ~s.culled)[0]
    bw = s.bbox[ids, 2] - s.bbox[ids, 0] + 1
    n = bw * (s.bbox[ids, 3] - s.bbox[ids, 1] + 1)
    acc = {"pix": [], "f": [], "w": [], "edge_pix": [], "edge_f": []}

    def take(t, px, py):
        w, cov, edge = _edges(s, t, px, py)
        acc["pix"].append((py * s.W + px)[cov]); acc["f"].append(t[cov]); acc["w"].append(w[cov])
        acc["edge_pix"].append((py * s.W + px)[edge]); acc["edge_f"].append(t[edge])

    few = n <= 16
    for j in range(16):                                                # the many triangles of a few candidates: candidate j of each at once
        m = few & (j < n)
        if m.any():
            take(ids[m], s.bbox[ids[m], 0] + j % bw[m], s.bbox[ids[m], 1] + j // bw[m])
    for t, b, c in zip(ids[~few], bw[~few], n[~few]):                  # the few triangles of many candidates: one at a time
        j = np.arange(c)
        take(np.full(c, t), s.bbox[t, 0] + j % b, s.bbox[t, 1] + j // b)
    return {k: (np.concatenate(v) if v else np.zeros((0, 3) if k == "w" else 0, np.int64)) for k, v in acc.items()}


# ---- cases ------------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    W: int
    H: int
    build: object                      # () -> (xs, ys, zc): int [F,3], int [F,3], float [F,3]
    claims: frozenset
    shifts: tuple = (0,)               # per view: translation in whole pixels (at zc = 1) along x
    modes: tuple = (1, 0)              # raster_tiled values the GPU test runs the case under
    cull: int = 0
    cx: int = 0
    cy: int = 0
    extents: bool = False              # also run rasterize_extents
    known: bool = True                 # the integer answer covers the case (False: near-plane straddlers)

    @property
    def id(self):
        return self.name

    @property
    def Hn(self):
        return len(self.shifts)


@functools.lru_cache(maxsize=None)
def geometry(case: Case):
    xs, ys, zc = case.build()
    xs, ys, zc = np.asarray(xs, np.int64).reshape(-1, 3), np.asarray(ys, np.int64).reshape(-1, 3), np.asarray(zc, np.float64).reshape(-1, 3)
    assert xs.shape == ys.shape == zc.shape
    return xs, ys, zc


def n_faces(case):
    return geometry(case)[0].shape[0]


def mesh(case):
    """(verts f32 [3F,3], faces i32 [F,3], colors u8 [3F,3]) — every arithmetic step exact (asserted)"""
    xs, ys, zc = geometry(case)
    F = xs.shape[0]
    v64 = np.stack([(xs - 256 * case.cx) / 65536.0 * zc, (ys - 256 * case.cy) / 65536.0 * zc, zc - 1.0], 2).reshape(-1, 3)
    v = v64.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), v64), case.name
    ident = np.arange(F, dtype=np.int64) + 1
    col = np.stack([ident & 255, (ident >> 8) & 255, (ident >> 16) & 255], 1).astype(np.uint8)
    return v, np.arange(3 * F, dtype=np.int32).reshape(F, 3), np.repeat(col, 3, axis=0)


def poses(case):
    p = np.tile(np.eye(4, dtype=np.float32), (case.Hn, 1, 1))
    p[:, 0, 3] = np.array(case.shifts, np.float32) / np.float32(256.0)
    p[:, 2, 3] = 1.0
    return p


def intrinsics(case):
    return FX, FX, float(case.cx), float(case.cy)


def shifted(case, view):
    """(xs, ys, zc) [F,3] of one view in exact integers BEFORE the clamp: the shift moves a vertex by 256 k / zc subpixels.  Vertices
    behind the near plane keep their nominal coordinates (set-up never reads them)."""
    xs, ys, zc = geometry(case)
    k = case.shifts[view]
    if k:
        assert all(Fraction(256 * k) / Fraction(float(z)) % 1 == 0 for z in np.unique(zc[zc > ZNEAR])), (case.name, "shift is no whole subpixel")
    dx = np.where(zc > ZNEAR, np.round(256 * k / np.where(zc > ZNEAR, zc, 1.0)), 0).astype(np.int64)
    return xs + dx, ys, zc


def projected(case, view):
    """what the vertex stage must produce: shifted(), clamped to +-CLAMP_PX px (raster_core.h project_vertex)"""
    xs, ys, zc = shifted(case, view)
    lim = CLAMP_PX * 256
    return np.clip(xs, -lim, lim), np.clip(ys, -lim, lim), zc


def case_setup(case, view):
    xi, yi, zc = projected(case, view)
    return setup(xi, yi, zc, case.W, case.H, case.cull)


def known_answer(case, view):
    """(covered bool [H,W], owner i32 [H,W] (-1 = background), depth f64 [H,W] (0 = background), info) in integer arithmetic; info holds
    per-pixel counts for the classifier: cover_n (triangles covering the centre), tie (two nearest fragments on equal planes), edge_n
    (triangles with the centre exactly on an edge) and those (pixel, triangle) pairs themselves, edge_pix / edge_f"""
    assert case.known, case.name
    s = case_setup(case, view)
    zc = np.take_along_axis(geometry(case)[2], s.k, 1)                 # per corner AFTER the orientation swap
    fr = fragments(s)
    W, H = case.W, case.H
    pix, f, w = fr["pix"], fr["f"], fr["w"]
    z = zc[f]
    flat = (z[:, 0] == z[:, 1]) & (z[:, 1] == z[:, 2])
    izn = np.round(IZS / z).astype(np.int64)
    assert np.array_equal(izn * z, np.full_like(z, IZS)), (case.name, "depths must be powers of two in [1/16, 64]")
    num = (w * izn).sum(1)                                             # 1 / depth = num / (area2 * IZS)
    d = np.where(flat, z[:, 0], s.area2[f].astype(np.float64) * IZS / np.where(num > 0, num, 1).astype(np.float64))
    order = np.lexsort((f, d, pix))                                    # per pixel: nearest plane first, then the lowest face id
    pix, f, d = pix[order], f[order], d[order]
    first = np.ones(len(pix), bool)
    first[1:] = pix[1:] != pix[:-1]
    owner = np.full(W * H, -1, np.int32)
    depth = np.zeros(W * H, np.float64)
    owner[pix[first]] = f[first]
    depth[pix[first]] = d[first]
    tie = np.zeros(W * H, bool)
    second = ~first
    second[1:] &= first[:-1]                                           # the runner-up of its pixel
    tie[pix[second]] = d[second] == d[np.nonzero(second)[0] - 1]
    info = {"cover_n": np.bincount(pix, minlength=W * H).reshape(H, W), "tie": tie.reshape(H, W),
            "edge_n": np.bincount(fr["edge_pix"], minlength=W * H).reshape(H, W), "edge_pix": fr["edge_pix"], "edge_f": fr["edge_f"]}
    owner = owner.reshape(H, W)
    return owner >= 0, owner, depth.reshape(H, W), info


def coverage_info(s: Setup):
    """(covered bool [H,W], info) of a set-up without depths (no tie information): what classify_setup takes as `cover` for scenes that are
    not constructed (the random soups of tests/test_gpu_fuzz.py); None when a straddler makes the integer coverage incomplete"""
    if s.strad.any():
        return None
    fr = fragments(s)
    n = s.W * s.H
    cover_n = np.bincount(fr["pix"], minlength=n).reshape(s.H, s.W)
    return cover_n > 0, {"cover_n": cover_n, "tie": np.zeros((s.H, s.W), bool), "edge_n": np.bincount(fr["edge_pix"], minlength=n).reshape(s.H, s.W),
                          "edge_pix": fr["edge_pix"], "edge_f": fr["edge_f"]}


def expected_rgb(owner):
    ident = (owner.astype(np.int64) + 1)
    return np.stack([ident & 255, (ident >> 8) & 255, (ident >> 16) & 255], -1).astype(np.uint8)


def depth_ulps(depth_f32, depth_known):
    """deviation of a float32 depth image from the known plane depth, in float32 units in the last place (bit distance to the rounded
    known value; both are positive wherever the answer is covered)"""
    a = np.ascontiguousarray(depth_f32, np.float32).view(np.int32).astype(np.int64)
    b = depth_known.astype(np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


@functools.lru_cache(maxsize=None)
def oracle_render(case):
    """(rgb u8 [Hn,H,W,3], depth f32 [Hn,H,W]) of oracle/fp_oracle.c, computed once per process and shared (treat as read-only)"""
    from oracle import fp_oracle as fo
    v, f, c = mesh(case)
    rgb, depth = fo.rasterize(v, f, c, poses(case), 1.0, *intrinsics(case), case.W, case.H, ambient=1.0, shade=0, cull=case.cull)
    rgb.setflags(write=False); depth.setflags(write=False)
    return rgb, depth


# ---- the classifier -----------------------------------------------------------------------------------------------------------------------------
TILE_WIDTHS = (1, 3, 7, 32)


def classify_setup(s: Setup, modes, F, Hn, raw=None, zc=None, cover=None):
    """branch labels one view's set-up reaches under the given raster_tiled modes.  raw = (xs, ys) before the clamp; cover = the known
    answer's (covered, info) or None where there is none (straddlers)"""
    out = set()
    W, H = s.W, s.H
    live = s.ok & ~s.culled
    plain = s.ok & ~s.strad
    if (s.nfront == 0).any():
        out.add("drop-behind")
    all_front = s.nfront == 3
    if (all_front & (s.area2 == 0)).any():
        out.add("drop-zero-area")
    nonzero = all_front & (s.area2 != 0)
    no_centre = (s.ubox[:, 2] < s.ubox[:, 0]) | (s.ubox[:, 3] < s.ubox[:, 1])
    if (nonzero & no_centre).any():
        out.add("drop-no-centre")
    if (nonzero & ~no_centre & ~s.ok).any():
        out.add("drop-offscreen")
    if (plain & s.swapped).any():
        out.add("swapped")
    if (plain & ~s.swapped).any():
        out.add("unswapped")
    if s.culled.any():
        out.add("cull-back")
    if (plain & ~s.culled & s.swapped).any() and s.culled.any():
        out.add("cull-front")
    if (s.strad & (s.nfront == 1)).any():
        out.add("straddler-1front")
    if (s.strad & (s.nfront == 2)).any():
        out.add("straddler-2front")
    if (plain & live & (s.span == SMALL_SPAN - 1)).any():
        out.add(f"small-{SMALL_SPAN - 1}")
    if (plain & live & (s.span == SMALL_SPAN)).any():
        out.add(f"wide-{SMALL_SPAN}")
    if raw is not None:
        lim = CLAMP_PX * 256
        clamped = ((np.abs(raw[0]) > lim) | (np.abs(raw[1]) > lim)) & (np.asarray(zc, np.float32) > np.float32(ZNEAR))
        if (clamped.any(1) & plain & live).any():
            out.add(f"clamp-{CLAMP_PX}")
    if zc is not None and (plain & live & ((zc.max(1) != zc.min(1)))).any():
        out.add("depth-sloped")
    area = (s.bbox[:, 2] - s.bbox[:, 0] + 1) * (s.bbox[:, 3] - s.bbox[:, 1] + 1)
    for mode in modes:
        p = plan(W, H, F, Hn, mode)
        if p["path"] == "global":
            if (plain & live & (area == BIG_AREA)).any():
                out.add(f"global-own-{BIG_AREA}")
            if (plain & live & (area == BIG_AREA + 1)).any():
                out.add(f"global-queue-{BIG_AREA + 1}")
            continue
        T, (ntx, nty) = p["T"], p["tiles"]
        t0x, t0y, t1x, t1y = (s.bbox[:, k] // T for k in range(4))
        if (live & (t1x - t0x == 1) & (t1y - t0y == 1)).any():
            out.add("spans-2x2-tiles")
        if ntx * nty > 1 and (live & ~s.strad & (t0x == 0) & (t0y == 0) & (t1x == ntx - 1) & (t1y == nty - 1)).any():
            out.add("spans-all-tiles")
        hit_any, untouched, hit_empty = False, False, False
        for ty in range(nty):
            for tx in range(ntx):
                X0, Y0, X1, Y1 = tx * T, ty * T, min(W, tx * T + T) - 1, min(H, ty * T + T) - 1
                inr = live & (t0x <= tx) & (tx <= t1x) & (t0y <= ty) & (ty <= t1y)
                x0, y0 = np.maximum(s.bbox[:, 0], X0), np.maximum(s.bbox[:, 1], Y0)
                x1, y1 = np.minimum(s.bbox[:, 2], X1), np.minimum(s.bbox[:, 3], Y1)
                bw, n = x1 - x0 + 1, (x1 - x0 + 1) * (y1 - y0 + 1)
                mine = inr & (x0 <= x1) & (y0 <= y1)
                lane = mine & s.small & ~s.strad & (n <= BIG_TILE_AREA)
                wave = mine & s.small & ~s.strad & (n > BIG_TILE_AREA)
                if (lane & (n == BIG_TILE_AREA)).any():
                    out.add(f"tile-lane-{BIG_TILE_AREA}")
                if (wave & (n == BIG_TILE_AREA + 1)).any():
                    out.add(f"tile-wave-{BIG_TILE_AREA + 1}")
                for b in TILE_WIDTHS:                                  # the last lane shape and the first wave shape of each bbox width
                    if (lane & (bw == b) & (n + b > BIG_TILE_AREA)).any():
                        out.add(f"tile-lane-w{b}")
                    if (wave & (bw == b) & (n - b <= BIG_TILE_AREA)).any():
                        out.add(f"tile-wave-w{b}")
                wide = mine & ~s.small & ~s.strad
                if wide.any():
                    out.add("tile-wave-wide")
                if cover is not None and len(cover[1]["edge_f"]):         # which of the three coverage routines meets a centre ON an edge here
                    ex, ey = cover[1]["edge_pix"] % W, cover[1]["edge_pix"] // W
                    ef = cover[1]["edge_f"][(ex >= X0) & (ex <= X1) & (ey >= Y0) & (ey <= Y1)]
                    for name, who in (("lane", lane), ("wave32", wave), ("wide", wide)):
                        if who[ef].any():
                            out.add(f"edge-centres-{name}")
                if inr.any():
                    hit_any = True
                    if cover is not None and not cover[0][Y0:Y1 + 1, X0:X1 + 1].any():
                        hit_empty = True
                else:
                    untouched = True
        if hit_any and untouched:
            out.add("tile-untouched")
        if hit_empty:
            out.add("tile-hit-but-empty")
    if cover is not None:
        covered, info = cover
        if (info["edge_n"] > 0).any():
            out.add("edge-through-centres")
        if ((info["edge_n"] >= 2) & (info["cover_n"] == 1)).any():
            out.add("shared-edge-watertight")
        if info["tie"].any():
            out.add("tie-lowest-id")
    return out


def extents_labels(case, count):
    width = "wide" if case.W >= 106 else "narrow"
    out = {f"box-{'0px' if count == 0 else '1..99px' if count < 100 else 'ge100px'}-{width}"}
    if count in (99, 100):
        out.add(f"box-{count}px")                                      # either side of the fallback's threshold
    return out


@functools.lru_cache(maxsize=None)
def classify(case: Case):
    """the set of branch labels the case reaches (launch labels of every mode it runs under, triangle labels of every view)"""
    F = n_faces(case)
    out = set()
    for mode in case.modes:
        out |= launch_labels(case.W, case.H, F, case.Hn, mode)
    seen = {}
    for view in range(case.Hn):
        s = case_setup(case, view)
        cover = None
        if case.known:
            covered, _, _, info = known_answer(case, view)
            cover = (covered, info)
            if case.extents:
                out |= extents_labels(case, int(covered.sum()))
                if case.cx > 0 and covered[:, :case.cx].any():
                    out.add("ext-negative-X")
        k = case.shifts[view]
        if k not in seen:                                              # (the views of a view-count case repeat a few shifts' set-ups)
            xs, ys, zc = shifted(case, view)
            seen[k] = classify_setup(s, case.modes, F, case.Hn, raw=(xs, ys), zc=zc, cover=cover)
        out |= seen[k]
    return frozenset(out)


# ---- scene builders (coordinates in subpixels; px(p) = the centre of pixel p) -------------------------------------------------------------------
def px(p):
    return 256 * p + 128


def _tris(rows):
    """rows of ((x, y) * 3, zc | (zc, zc, zc)) -> (xs, ys, zc)"""
    xs = [[c[0] for c in r[:3]] for r in rows]
    ys = [[c[1] for c in r[:3]] for r in rows]
    zc = [list(r[3]) if isinstance(r[3], (tuple, list)) else [r[3]] * 3 for r in rows]
    return np.array(xs, np.int64), np.array(ys, np.int64), np.array(zc, np.float64)


def pixel_tri(pxl, pyl, zc=1.0):
    """a triangle that owns exactly pixel (pxl, pyl): corners (c - 64, c - 64), (c + 128, c - 64), (c - 64, c + 128)"""
    cx_, cy_ = px(pxl), px(pyl)
    return ((cx_ - 64, cy_ - 64), (cx_ + 128, cy_ - 64), (cx_ - 64, cy_ + 128), zc)


def box_tri(x0, y0, bw, bh, zc=1.0, flip=False):
    """a triangle whose candidate box is exactly pixels [x0, x0 + bw) x [y0, y0 + bh).  One pixel wide or high: a sliver symmetric about
    the centre line that covers EVERY candidate.  Otherwise a right triangle that covers the box's LAST candidate: legs along the top and
    right sides of a wide box (the last column: candidates b r + b - 1), the left and bottom sides of a tall one (the first column:
    candidates b r) — the two places where a row / column split of the candidate index by a float reciprocal could go wrong"""
    xl, xr, yt, yb = px(x0) - 64, px(x0 + bw - 1) + 64, px(y0) - 64, px(y0 + bh - 1) + 64
    if bw == 1:
        a, b, c = (xl, yt), (xr, yt), (px(x0), yb)
    elif bh == 1:
        a, b, c = (xl, yt), (xr, px(y0)), (xl, yb)
    else:
        a, c = (xl, yt), (xr, yb)
        b = (xr, yt) if xr - xl >= yb - yt else (xl, yb)
    return (a, c, b, zc) if flip else (a, b, c, zc)


def rect(x0, y0, x1, y1, zc=1.0):
    """two triangles over the pixel-boundary rectangle [x0, x1) x [y0, y1) px, split by the diagonal from its top-left corner; the second is
    wound so that set-up swaps it"""
    A, B, C, D = (256 * x0, 256 * y0), (256 * x1, 256 * y0), (256 * x1, 256 * y1), (256 * x0, 256 * y1)
    return [(A, B, C, zc), (A, D, C, zc)]


def pixel_grid(W, n, extra=()):
    """one pixel_tri per pixel for the first n pixels of a W-wide frame in raster order (vectorised), then the extra triangles"""
    def build():
        i = np.arange(n, dtype=np.int64)
        cxs, cys = px(i % W), px(i // W)
        xs = np.stack([cxs - 64, cxs + 128, cxs - 64], 1)
        ys = np.stack([cys - 64, cys - 64, cys + 128], 1)
        zc = np.ones((n, 3))
        if extra:
            ex, ey, ez = _tris(list(extra))
            xs, ys, zc = np.concatenate([xs, ex]), np.concatenate([ys, ey]), np.concatenate([zc, ez])
        return xs, ys, zc
    return build


def seam_scene(W, H, T):
    """a backdrop over the whole frame at depth 4, a 6 x 6-px box triangle across every vertical tile seam (18 candidates on either side),
    one across the horizontal seam if there is one, and single-pixel triangles in the frame's four corners"""
    def build():
        rows = [((-256, -256), (256 * (2 * W + 2), -256), (-256, 256 * (2 * H + 2)), 4.0)]
        for i in range(1, cdiv(W, T)):
            rows.append(box_tri(i * T - 3, min(3 + 2 * i, H - 6), 6, 6, 1.0, flip=bool(i & 1)))
        if H > T:
            rows.append(box_tri(5, T - 3, 6, 6, 1.0))
        rows += [pixel_tri(0, 0), pixel_tri(W - 1, 0), pixel_tri(0, H - 1), pixel_tri(W - 1, H - 1), pixel_tri(W - 2, H - 1, 2.0)]
        return _tris(rows)
    return build


def centre_rect(x0, y0, x1, y1, zc=1.0):
    """two triangles over the rectangle whose corners are the CENTRES of pixels (x0, y0) and (x1, y1): all four sides and (for a square) the
    shared diagonal run through pixel centres, so the top-left rule decides every border pixel"""
    A, B, C, D = (px(x0), px(y0)), (px(x1), px(y0)), (px(x1), px(y1)), (px(x0), px(y1))
    return [(A, B, C, zc), (A, D, C, zc)]


def _edge_lane():
    return _tris(centre_rect(10, 10, 14, 14) + centre_rect(61, 30, 66, 33) + centre_rect(20, 62, 23, 66, 2.0))   # 25 candidates; across either seam


def _edge_wide():
    assert 128 * 256 == SMALL_SPAN
    return _tris(centre_rect(1, 2, 129, 40) + centre_rect(3, 50, 130, 60, 2.0))     # spans 32 768 and 32 512 subpixels


def _quad_diagonal():
    return _tris(rect(30, 30, 70, 70))                                 # 40 x 40 px across all four tiles of 96 x 80; the diagonal runs through 40 centres


def _spans():
    rows = [((-256, -256), (256 * 300, -256), (-256, 256 * 300), 2.0),                 # behind everything, every tile
            box_tri(60, 60, 8, 8, 1.0), box_tri(120, 2, 8, 3, 1.0)]                    # 2 x 2 tiles; the partial last column
    return _tris(rows)


def _one_small():
    return _tris([box_tri(5, 5, 4, 4), pixel_tri(20, 9)])


def _hit_but_empty():
    # the sliver's box reaches pixels 64, 65 of tile 1, but it covers centres up to x = 61.5 only; tile 1 of 128 x 64 stays background
    return _tris([((256 * 50, 256 * 10), (256 * 66, 256 * 10), (256 * 50, 256 * 12), 1.0), box_tri(3, 3, 5, 5)])


def _drops():
    behind = 1.0 / 32                                                  # 0.03125 <= ZNEAR
    rows = [box_tri(10, 10, 6, 6),                                                                      # visible
            (( px(20), px(20)), (px(30), px(20)), (px(25), px(30)), behind),                            # all three behind the near plane
            ((px(20), px(40)), (px(30), px(50)), (px(40), px(60)), 1.0),                                # collinear
            ((px(50), px(10)), (px(50), px(10)), (px(60), px(20)), 1.0),                                # a repeated corner
            ((px(40) + 10, px(40) + 10), (px(40) + 200, px(40) + 20), (px(40) + 20, px(40) + 200), 1.0),   # between four centres
            ((-256 * 40, 256 * 10), (-256 * 20, 256 * 10), (-256 * 30, 256 * 30), 1.0),                 # left of the frame
            ((256 * 100, 256 * 10), (256 * 130, 256 * 10), (256 * 110, 256 * 30), 1.0),                 # right of it
            ((256 * 10, 256 * 90), (256 * 40, 256 * 90), (256 * 20, 256 * 120), 1.0)]                   # below it
    return _tris(rows)


def _cull():
    return _tris([box_tri(5, 5, 12, 9, 1.0), box_tri(30, 5, 12, 9, 1.0, flip=True), box_tri(8, 8, 30, 4, 2.0), box_tri(8, 20, 5, 30, 2.0, flip=True)])


def _span_threshold():
    y = 256 * 5
    rows = [((256, y), (256 + SMALL_SPAN - 1, y), (256, y + 256 * 20), 1.0),                # spans 32 767 subpixels: 32-bit edge functions
            ((256, y + 256 * 8), (256 + SMALL_SPAN, y + 256 * 8), (256, y + 256 * 40), 2.0),   # spans 32 768: 64-bit, one plane behind
            ((256, y + 256 * 8), (256 + SMALL_SPAN, y + 256 * 8), (256, y + 256 * 40), 2.0),   # its coplanar duplicate: loses every pixel
            # 32 767 again, wound the other way, and its mirror-wound duplicate.  (Below the others: two DIFFERENT triangles on one plane may
            # differ in the last bit of their float depths, so only exact duplicates tie.)
            ((256, y + 256 * 46), (256, y + 256 * 60), (256 + SMALL_SPAN - 1, y + 256 * 46), 2.0),
            ((256, y + 256 * 46), (256 + SMALL_SPAN - 1, y + 256 * 46), (256, y + 256 * 60), 2.0)]
    return _tris(rows)


def _global_area():
    side = int(round(BIG_AREA ** 0.5))
    assert side * side == BIG_AREA
    rows = [box_tri(3, 3, side, side, 1.0), box_tri(30, 2, BIG_AREA, 1, 1.0), box_tri(30, 6, BIG_AREA + 1, 1, 1.0),
            box_tri(320, 1, 1, 18, 1.0), box_tri(330, 2, side, side + 1, 2.0)]
    return _tris(rows)


def _tile_candidates():
    """per bbox width b in 1, 3, 7, 32: the tallest box of at most BIG_TILE_AREA candidates (one lane, reciprocal divide by b) and the
    shortest above it (whole wave), all inside tile (0, 0) of a 96 x 80 frame, plus boxes that only the tile seam cuts down to a lane's"""
    rows, x = [], 1
    for b in (1, 3, 7):
        h = BIG_TILE_AREA // b
        rows += [box_tri(x, 1, b, h, 1.0), box_tri(x + b + 1, 1, b, h + 1, 1.0, flip=True)]
        x += 2 * b + 2
    rows += [box_tri(1, 40, 32, 1, 1.0), box_tri(1, 42, 32, 2, 1.0), box_tri(1, 46, BIG_TILE_AREA + 1, 1, 1.0, flip=True)]
    rows += [box_tri(60, 60, 8, 8, 1.0), box_tri(40, 50, 48, 1, 1.0)]          # 64 candidates: 16 per tile; 48 x 1: 24 | 24
    return _tris(rows)


def _clamp():
    far = 9_000_000                                                    # 35 156 px: clamped to 30 000 px
    assert far > CLAMP_PX * 256 and far < 2 ** 24
    return _tris([((-far, 256 * 10), (far, 256 * 10), (0, 256 * 60), 2.0), ((256 * 20, 256 * 20), (far, 256 * 30), (256 * 20, 256 * 40), 1.0),
                  box_tri(70, 50, 5, 5, 1.0)])


def _straddlers():
    behind = 1.0 / 32
    rows = [((px(10), px(10)), (px(60), px(20)), (px(30), px(70)), (1.0, behind, behind)),       # one corner in front
            ((px(40), px(5)), (px(90), px(10)), (px(70), px(60)), (1.0, 2.0, -1.0)),             # two in front, one behind the camera
            box_tri(5, 60, 20, 10, 1.0), box_tri(50, 40, 30, 30, 4.0)]
    return _tris(rows)


def _sloped():
    rows = [((256 * 5, 256 * 5), (256 * 85, 256 * 10), (256 * 20, 256 * 70), (1.0, 2.0, 4.0)),
            ((256 * 10, 256 * 60), (256 * 90, 256 * 75), (256 * 60, 256 * 3), (4.0, 0.5, 1.0)),
            ((256 * 2, 256 * 2), (256 * 94, 256 * 2), (256 * 2, 256 * 78), (8.0, 8.0, 16.0))]
    return _tris(rows)


def _view_scene():
    return _tris([box_tri(2, 4, 5, 9, 1.0), box_tri(9, 2, 7, 3, 1.0, flip=True), pixel_tri(4, 20), pixel_tri(12, 30), box_tri(3, 40, 12, 12, 1.0)])


def _ext_scene():
    return _tris(rect(4, 6, 16, 18) + [pixel_tri(2, 30)])              # 144 px + 1 px at the left of the frame


def _ext_boundary():
    return _tris(rect(110, 20, 120, 30) + rect(10, 5, 19, 16, 2.0))     # 100 px in the frame; 99 px that only the third view brings in alone


def _c(name, W, H, build, claims, **kw):
    return Case(name, W, H, build, frozenset(claims), **kw)


ALL_MODES = (1, 0, -1)
assert TILED_MAX_TRIS == 512 * 256, "the count-limit cases are built for a 512 x 256 frame of one triangle per pixel"
CASES = [
    _c("quad-diagonal-96x80", 96, 80, _quad_diagonal, {"tiled-T64", "global-forced", "tiles-partial-x", "tiles-partial-y", "flush-dword", "views-lt8",
       "chunks-1-partial", "bin-grid-tail", "edge-through-centres", "edge-centres-wave32", "shared-edge-watertight", "swapped", "unswapped",
       "spans-2x2-tiles", "box-ge100px-narrow"}, modes=ALL_MODES, extents=True),
    _c("edge-lane-96x80", 96, 80, _edge_lane, {"edge-through-centres", "edge-centres-lane", "shared-edge-watertight"}),
    _c("edge-wide-131x70", 131, 70, _edge_wide, {"edge-through-centres", "edge-centres-wide", "edge-centres-wave32", f"wide-{SMALL_SPAN}", "shared-edge-watertight"}),
    _c("spans-131x70", 131, 70, _spans, {"spans-all-tiles", "spans-2x2-tiles", "flush-bytes-w3", "tile-wave-wide", "box-ge100px-wide"}, extents=True),
    _c("one-small-131x70", 131, 70, _one_small, {"tile-untouched", "tiled-T64", "box-1..99px-wide"}, extents=True),
    _c("hit-but-empty-128x64", 128, 64, _hit_but_empty, {"tile-hit-but-empty", "tiles-exact-x", "tiles-exact-y", "flush-dword"}),
    _c("drops-96x80", 96, 80, _drops, {"drop-behind", "drop-zero-area", "drop-no-centre", "drop-offscreen"}),
    _c("cull-96x80", 96, 80, _cull, {"cull-front", "cull-back", "tiled-T64", "global-forced"}, cull=1),
    _c("span-threshold-131x70", 131, 70, _span_threshold, {f"small-{SMALL_SPAN - 1}", f"wide-{SMALL_SPAN}", "tie-lowest-id", "swapped", "unswapped"}),
    _c("global-area-520x24", 520, 24, _global_area, {f"global-own-{BIG_AREA}", f"global-queue-{BIG_AREA + 1}", "tiled-T72", "tiles-partial-x"}),
    _c("tile-candidates-96x80", 96, 80, _tile_candidates, {f"tile-lane-{BIG_TILE_AREA}", f"tile-wave-{BIG_TILE_AREA + 1}"} |
       {f"tile-{k}-w{b}" for k in ("lane", "wave") for b in TILE_WIDTHS}),
    _c("clamp-96x80", 96, 80, _clamp, {f"clamp-{CLAMP_PX}", "tile-wave-wide"}),
    _c("straddlers-96x80", 96, 80, _straddlers, {"straddler-1front", "straddler-2front"}, known=False),
    _c("sloped-96x80", 96, 80, _sloped, {"depth-sloped"}),
    # ---- tile edges 72, 80, 88 and the frame that is too wide: seams, partial last tiles, every flush form
    _c("seams-520x24", 520, 24, seam_scene(520, 24, 72), {"tiled-T72", "tiles-partial-x", "flush-dword", "spans-all-tiles"}, modes=ALL_MODES),
    _c("seams-576x16", 576, 16, seam_scene(576, 16, 72), {"tiled-T72", "tiles-exact-x", "tiles-partial-y"}),
    _c("seams-580x24", 580, 24, seam_scene(580, 24, 80), {"tiled-T80", "tiles-partial-x", "flush-dword"}),
    _c("seams-581x24", 581, 24, seam_scene(581, 24, 80), {"tiled-T80", "flush-bytes-w1"}),
    _c("seams-640x48", 640, 48, seam_scene(640, 48, 80), {"tiled-T80", "tiles-exact-x", "flush-dword"}, modes=ALL_MODES),
    _c("seams-650x24", 650, 24, seam_scene(650, 24, 88), {"tiled-T88", "flush-bytes-w2", "tiles-partial-x"}),
    _c("seams-704x16", 704, 16, seam_scene(704, 16, 88), {"tiled-T88", "tiles-exact-x"}, modes=ALL_MODES),
    _c("seams-708x24", 708, 24, seam_scene(708, 24, 96), {"global-by-size"}, modes=(-1, 1)),
    _c("seams-131x70", 131, 70, seam_scene(131, 70, 64), {"tiled-T64", "flush-bytes-w3", "spans-all-tiles"}),
    # ---- view counts: one scene under N poses, view h shifted by 3 h px (a view in another view's slot is a shifted image)
    _c("views-8-96x80", 96, 80, _view_scene, {"views-groups-only", "views-8"}, shifts=tuple(3 * h for h in range(8))),
    _c("views-16-128x64", 128, 64, _view_scene, {"views-groups-only", "views-16"}, shifts=tuple(3 * h for h in range(16))),
    _c("views-11-131x70", 131, 70, _view_scene, {"views-groups+rem", "views-11"}, shifts=tuple(3 * h for h in range(11))),
    _c("views-19-580x24", 580, 24, seam_scene(580, 24, 80), {"views-groups+rem", "views-19", "tiled-T80"}, shifts=tuple(2 * h for h in range(19))),
    _c("views-11-chunks-131x70", 131, 70, pixel_grid(131, 600), {"views-groups+rem", "views-11", "views-bin-grid", "bin-grid-tail", "chunks-tail"},
       shifts=tuple(3 * h for h in range(11))),
    # ---- extents: a view of >= 100 mask pixels, one of 1 .. 99, an empty one; wide and narrow frames; a cloud left of the principal point
    _c("extents-96x80", 96, 80, _ext_scene, {"box-ge100px-narrow", "box-1..99px-narrow", "box-0px-narrow", "ext-negative-X"},
       shifts=(0, -10, -40), cx=40, cy=30, extents=True),
    _c("extents-131x70", 131, 70, _ext_scene, {"box-ge100px-wide", "box-1..99px-wide", "box-0px-wide", "ext-negative-X"},
       shifts=(0, -10, -40), cx=40, cy=30, extents=True),
    _c("extents-boundary-131x70", 131, 70, _ext_boundary, {"box-100px", "box-99px", "box-ge100px-wide", "box-1..99px-wide"},
       shifts=(-40, 40), extents=True),
    # ---- chunks and rounds: one triangle per pixel, so a lost chunk is a background pixel in a known place
    _c("chunks-64-96x80", 96, 80, pixel_grid(96, 64), {"chunks-exact", "bin-grid-tail"}),
    _c("chunks-65-96x80", 96, 80, pixel_grid(96, 65), {"chunks-tail", "bin-grid-tail"}),
    _c("chunks-256-96x80", 96, 80, pixel_grid(96, 256), {"chunks-exact"}),
    _c("round-full-512x256", 512, 256, pixel_grid(512, 512 * 256), {"rounds-1-full", "tiled-at-count-limit", "chunks-exact", "global-forced"},
       modes=ALL_MODES),
    _c("count-limit+1-512x256", 512, 256, pixel_grid(512, 512 * 256, extra=(box_tri(100, 100, 9, 9, 2.0),)), {"global-by-count", "rounds-2", "chunks-tail"},
       modes=ALL_MODES),
    _c("rounds-2-384x352", 384, 352, pixel_grid(384, 384 * 352), {"rounds-2", "chunks-exact", "global-by-count"}, modes=ALL_MODES),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# every label of the issue, and the extra ones this table adds
LABELS = (
    ["tiled-T64", "tiled-T72", "tiled-T80", "tiled-T88", "global-forced", "global-by-size", "global-by-count", "tiled-at-count-limit",
     "tiles-exact-x", "tiles-partial-x", "tiles-exact-y", "tiles-partial-y", "flush-dword", "flush-bytes-w1", "flush-bytes-w2", "flush-bytes-w3",
     "views-lt8", "views-groups-only", "views-8", "views-16", "views-groups+rem", "views-11", "views-19",
     "chunks-1-partial", "chunks-exact", "chunks-tail", "bin-grid-tail", "rounds-1-full", "rounds-2", "tile-untouched", "tile-hit-but-empty",
     "drop-behind", "drop-zero-area", "drop-no-centre", "drop-offscreen", "swapped", "unswapped", "cull-front", "cull-back",
     f"small-{SMALL_SPAN - 1}", f"wide-{SMALL_SPAN}", f"global-own-{BIG_AREA}", f"global-queue-{BIG_AREA + 1}",
     f"tile-lane-{BIG_TILE_AREA}", f"tile-wave-{BIG_TILE_AREA + 1}"]
    + [f"tile-{k}-w{b}" for k in ("lane", "wave") for b in TILE_WIDTHS]
    + ["spans-2x2-tiles", "spans-all-tiles", f"clamp-{CLAMP_PX}", "straddler-1front", "straddler-2front", "edge-through-centres",
       "shared-edge-watertight", "tie-lowest-id"]
    + [f"box-{n}-{w}" for n in ("0px", "1..99px", "ge100px") for w in ("wide", "narrow")] + ["ext-negative-X"]
    + ["tile-wave-wide", "depth-sloped", "edge-centres-lane", "edge-centres-wave32", "edge-centres-wide", "views-bin-grid", "box-99px", "box-100px"])
