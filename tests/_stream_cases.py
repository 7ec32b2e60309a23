"""The case table of the stream contract (include/freepose_hip.h: every call enqueues all of its device work on the stream it is given).
tests/test_stream_cases_cpu.py holds the table to the header (every entry with a `void* stream` parameter is named by a case or by
EXCLUDED) and checks the inputs on the host; tests/test_gpu_streams.py runs every case with late inputs on a side stream, hands the
stateful objects from stream to stream, and checks that no steady-state call drains the device.

Importing this module needs no GPU and does not load the library.  A case is
  name      the test id
  entries   the C entries whose launches, memsets and copies the case's result depends on
  build     build(which, n=None) -> {name: CPU tensor}: the DEVICE-RESIDENT inputs of set "A" or "B" — the same shapes and dtypes, other
            seeds, both valid (indices, counts, ranges, masks and tables in range; no NaN fill).  n = another batch size (cases with `batches`)
  call      call(x) -> tuple of tensors, x = the inputs as device tensors; enqueues on torch's current stream, through the public wrapper
            where it takes device tensors, through _lib with device tables where the wrapper would upload host arrays itself
  late      the inputs that are copied in behind the delay (default: all of them)
  waits     the entry is documented to wait on its own stream (it may block the host; it must still not drain the device)
  check     host check of the index-like inputs of a built set (the wrapper's own where it has one); raises on a bad table
  mutant    one of the five value-only entries the mutant control reruns with the launch stream swapped for the default one
  batches   (first, side, last) batch sizes of the hand-over test (stateful objects, ffa, the mesh)
"""
import ctypes as C
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

EXCLUDED = {}            # entry -> one-line reason naming what it does with its stream (at most 8; empty: every entry has a case)
MAX_EXCLUDED = 8
DRAINS_DEVICE = {}       # case name -> reason: entries whose steady-state call drains the device by design (none)

QSCALE = 1.4426950408889634 / 8.0
SPLIT_M, SPLIT_N = 8193, 1024      # the smallest M the planner labels split_* at N = 1024 on 256 CUs (8192 rows in front, 1 behind): two launches


@dataclass
class Case:
    name: str
    entries: tuple
    build: Callable
    call: Callable
    late: Optional[tuple] = None
    waits: bool = False
    check: Optional[Callable] = None
    mutant: bool = False
    batches: Optional[tuple] = None
    plan: Optional[tuple] = None      # GEMM cases: (M, N, K, epi, ln_part, label prefix the planner gives)


CASES = []


def _add(name, entries, build, call, **kw):
    CASES.append(Case(name, (entries,) if isinstance(entries, str) else tuple(entries), build, call, **kw))


def by_name(name):
    return next(c for c in CASES if c.name == name)


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------
def _seed(which, base):
    assert which in ("A", "B")
    return np.random.default_rng(base + (0 if which == "A" else 1000))


def _bf(rng, shape, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32)).to(torch.bfloat16)


def _f32(rng, shape, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32))


def _f64(rng, shape, scale=1.0):
    return torch.from_numpy(scale * rng.standard_normal(shape))


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


def _ops():
    from freepose_amd import ops
    return ops


def _lib():
    from freepose_amd import _lib as L
    return L


def _rodrigues(v):
    """rotation matrix of the rotation vector v (numpy float64)"""
    th = float(np.linalg.norm(v))
    if th < 1e-12:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def same_bits(a, b):
    """two tensors (or tuples of tensors) of equal shapes and dtypes with the same bytes"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu().contiguous().reshape(-1), b.detach().cpu().contiguous().reshape(-1)
    return bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))


# stateful objects, one per (case, context): a hand-over test runs under a fresh context and so gets fresh objects
_OBJECTS = {}


def _obj(key, make):
    ops = _ops()
    k = (key, ops.context().value)
    if k not in _OBJECTS:
        _OBJECTS[k] = make()
    return _OBJECTS[k]


def drop_objects(ctx_value=None):
    """forget the objects of one context (None: of all)"""
    for k in [k for k in _OBJECTS if ctx_value is None or k[1] == ctx_value]:
        del _OBJECTS[k]


# ---- the GEMM family ----------------------------------------------------------------------------------------------------------------------
BIAS, LS_RES_STATS, LN_BIAS, VT, PATCH = 0, 8, 5, 4, 3            # FpGemmEpi (tests/_gemm_cases.py)
GEMM_SHAPES = {"tiny64": (65, 144, 64), "small128": (2049, 1936, 64), "split": (SPLIT_M, SPLIT_N, 64)}
STATS_SHAPES = {"tiny64": (65, 192, 64), "small128": (2049, 1984, 64), "split": (SPLIT_M, SPLIT_N, 64)}
LN_SHAPES = {"tiny64": (65, 192, 128), "small128": (2049, 1984, 128), "split": (SPLIT_M, SPLIT_N, 128)}
VT_SHAPES = {"tiny64": (3, 16, 6, 64), "small128": (12, 912, 6, 64)}                     # B, npad, heads, K
PATCH_SHAPES = {"tiny64": (3, 35, 48, 1, 64, 64), "small128": (3, 1369, 1376, 5, 1024, 64)}   # B, P, npad, tok_off, N, K
CHAIN_SHAPES = {"tiny64": (160, 384, 1536), "small128": (2048, 256, 2048), "split": (SPLIT_M, 256, SPLIT_N)}   # M, D, N2 (K1 = 64)


def _label(tier):
    return "split_" if tier == "split" else tier


def _gemm_cases():
    for tier, (M, N, K) in GEMM_SHAPES.items():
        def build(which, n=None, M=M, N=N, K=K):
            r = _seed(which, 100 + M)
            return dict(x=_bf(r, (M, K)), w=_bf(r, (N, K), 0.05), bias=_bf(r, (N,), 0.1))
        _add(f"gemm_{tier}", "fp_op_gemm", build, lambda x: (_ops().gemm(x["x"], x["w"], x["bias"]),), mutant=tier == "tiny64",
             plan=(M, N, K, BIAS, False, _label(tier)))
    for tier, (M, N, K) in STATS_SHAPES.items():
        def build(which, n=None, M=M, N=N, K=K):
            r = _seed(which, 200 + M)
            return dict(x=_bf(r, (M, K)), w=_bf(r, (N, K), 0.05), bias=_bf(r, (N,), 0.1), gamma=_bf(r, (N,), 0.5), resid=_bf(r, (M, N)))
        _add(f"gemm_stats_{tier}", "fp_op_gemm_stats", build,
             lambda x: _ops().gemm_stats(x["x"], x["w"], x["bias"], x["gamma"], x["resid"]), plan=(M, N, K, LS_RES_STATS, False, _label(tier)))
    for tier, (M, N, K) in LN_SHAPES.items():
        def build(which, n=None, M=M, N=N, K=K):
            r = _seed(which, 300 + M)
            return dict(x=_bf(r, (M, K)), g=_bf(r, (K,), 0.5), b=_bf(r, (K,), 0.1), w=_bf(r, (N, K), 0.05), bias=_bf(r, (N,), 0.1))
        _add(f"ln_linear_{tier}", "fp_op_ln_linear", build,
             lambda x: (_ops().ln_linear(x["x"], x["g"], x["b"], x["w"], x["bias"], mode=0, n_scaled=64, row_scale=QSCALE),),
             plan=(M, N, K, LN_BIAS, False, _label(tier)))

        def consume(x):
            ops = _ops()
            rec, rstd = ops.row_stats(x["x"])
            return (ops.ln_consume(x["x"], rec, rstd, x["g"], x["b"], x["w"], x["bias"], mode=0), rec, rstd)
        _add(f"ln_consume_{tier}", ("fp_op_ln_consume", "fp_op_row_stats"), build, consume, plan=(M, N, K, LN_BIAS, False, _label(tier)))
    for tier, (B, npad, heads, K) in VT_SHAPES.items():
        def build(which, n=None, B=B, npad=npad, heads=heads, K=K):
            r = _seed(which, 400 + npad)
            return dict(x=_bf(r, (B * npad, K)), w=_bf(r, (heads * 64, K), 0.05), bias=_bf(r, (heads * 64,), 0.1))
        _add(f"gemm_vt_{tier}", "fp_op_gemm_vt", build,
             lambda x, npad=npad, heads=heads: (_ops().gemm_vt(x["x"], x["w"], x["bias"], npad, heads),),
             plan=(B * npad, heads * 64, K, VT, False, tier))
    for tier, (B, P, npad, off, N, K) in PATCH_SHAPES.items():
        def build(which, n=None, B=B, P=P, npad=npad, N=N, K=K):
            r = _seed(which, 500 + P)
            return dict(x=_bf(r, (B * P, K)), w=_bf(r, (N, K), 0.05), bias=_bf(r, (N,), 0.1), pos=_bf(r, (P, N), 0.1), tokens=_bf(r, (B, npad, N)))
        _add(f"gemm_patch_{tier}", "fp_op_gemm_patch", build,
             lambda x, off=off: (_ops().gemm_patch(x["x"], x["w"], x["bias"], x["pos"], x["tokens"].clone(), off),),
             plan=(B * P, N, K, PATCH, False, tier))
    for tier, (M, D, N2) in CHAIN_SHAPES.items():
        def build(which, n=None, M=M, D=D, N2=N2):
            r = _seed(which, 600 + M)
            return dict(x1=_bf(r, (M, 64)), w1=_bf(r, (D, 64), 0.05), b1=_bf(r, (D,), 0.1), gamma=_bf(r, (D,), 0.5), resid=_bf(r, (M, D)),
                        g=_bf(r, (D,), 0.5), b=_bf(r, (D,), 0.1), w2=_bf(r, (N2, D), 0.05), b2=_bf(r, (N2,), 0.1))
        _add(f"ln_chain_{tier}", "fp_op_ln_chain", build,
             lambda x: _ops().ln_chain(x["x1"], x["w1"], x["b1"], x["gamma"], x["resid"], x["g"], x["b"], x["w2"], x["b2"], mode=0, route=1),
             plan=(M, N2, D, LN_BIAS, True, _label(tier)))
    _add("gelu_direct", "fp_op_gelu", lambda which, n=None: dict(x=_bf(_seed(which, 700), (1000,), 2.0)), lambda x: (_ops().gelu_direct(x["x"]),))


_gemm_cases()


# ---- attention --------------------------------------------------------------------------------------------------------------------------------
def _attention_cases():
    def build_qk(which, n=None):
        r = _seed(which, 800)
        return dict(qk=_bf(r, (80, 128)), vt=_bf(r, (1, 1, 64, 80)))
    _add("attention", "fp_op_attention", build_qk, lambda x: (_ops().attention(x["qk"], x["vt"], 65),))          # B=1, H=1, n_tok=65 in 80 rows
    _add("attention_hd", "fp_op_attention_hd", lambda which, n=None: dict(qkv=_bf(_seed(which, 810), (1, 80, 3 * 104))),
         lambda x: (_ops().attention_hd(x["qkv"], 1, 65),), mutant=True)                                         # hd=104, n_tok=65
    _add("attention_causal", "fp_op_attention_causal", lambda which, n=None: dict(qkv=_bf(_seed(which, 820), (1, 80, 3 * 64))),
         lambda x: (_ops().attention_causal(x["qkv"], 1, 77),))                                                  # hd=64, n_tok=77


_attention_cases()


# ---- the ViT helper kernels -------------------------------------------------------------------------------------------------------------------
def _vit_helper_cases():
    def img(which, n=None):
        return dict(images=torch.from_numpy(_seed(which, 900).random((2, 3, 28, 42), dtype=np.float32)).to(torch.bfloat16))
    _add("im2col_norm", "fp_op_im2col_norm", img, lambda x: (_ops().im2col_norm(x["images"]),))

    def tok(which, n=None):
        r = _seed(which, 910)
        return dict(x=_bf(r, (2, 48, 64)), cls=_bf(r, (64,)), pos0=_bf(r, (64,)), reg=_bf(r, (4, 64)))
    _add("token_init", "fp_op_token_init", tok, lambda x: (_ops().token_init(x["x"].clone(), x["cls"], x["pos0"], x["reg"], 40),))

    def ln(which, n=None, rows=37):
        r = _seed(which, 920 + rows)
        return dict(x=_bf(r, (rows, 384)), gamma=_bf(r, (384,), 0.5), beta=_bf(r, (384,), 0.1))
    _add("layernorm", "fp_op_layernorm", ln, lambda x: (_ops().layernorm(x["x"], x["gamma"], x["beta"]),), mutant=True)
    _add("layernorm_rows", "fp_op_layernorm_rows", lambda which, n=None: ln(which, rows=96),
         lambda x: (_ops().layernorm_rows(x["x"], x["gamma"], x["beta"], rows=70, rows_per_b=35, in_stride_b=48, in_off=5, l2_normalize=True),))
    _add("posembed_aa", "fp_op_posembed_aa", lambda which, n=None: dict(grid=_bf(_seed(which, 930), (37 * 37, 64))),
         lambda x: (_ops().posembed_aa(x["grid"], 20, 30),))
    _add("row_stats", "fp_op_row_stats", lambda which, n=None: dict(x=_bf(_seed(which, 940), (37, 384))), lambda x: _ops().row_stats(x["x"]))

    def part(which, n=None):
        x = _seed(which, 950).standard_normal((6, 40, 64))             # the sums of real rows: sum x^2 >= (sum x)^2 / 64, a valid variance
        return dict(part=_t(np.stack([x.sum(-1), (x * x).sum(-1)], -1).astype(np.float32)))
    _add("stats_finalize", "fp_op_stats_finalize", part, lambda x: _ops().stats_finalize(x["part"], 37))

    def fold(which, n=None):
        r = _seed(which, 960)
        return dict(w=_bf(r, (130, 128), 0.05), gamma=_bf(r, (128,), 0.5), beta=_bf(r, (128,), 0.1), bias=_bf(r, (130,), 0.1))
    _add("ln_fold", "fp_op_ln_fold", fold, lambda x: _ops().ln_fold(x["w"], x["gamma"], x["beta"], x["bias"], n_scaled=64, row_scale=QSCALE))
    _add("transpose", "fp_op_transpose", lambda which, n=None: dict(x=_bf(_seed(which, 970), (37, 72))), lambda x: (_ops().transpose(x["x"]),),
         mutant=True)
    _add("l2_normalize", "fp_l2_normalize", lambda which, n=None: dict(x=_bf(_seed(which, 980), (37, 384))),
         lambda x: (_ops().l2_normalize(x["x"]),), mutant=True)                                                  # the vector kernel
    _add("l2_normalize_scalar", "fp_l2_normalize", lambda which, n=None: dict(x=_bf(_seed(which, 990), (5, 2048))),
         lambda x: (_ops().l2_normalize(x["x"]),))                                                               # D > 1536: the row kernel


_vit_helper_cases()


# ---- FFA --------------------------------------------------------------------------------------------------------------------------------------
def _ffa_inputs(which, B, gh, gw, cell, D=384):
    r = _seed(which, 1000 + B + cell)
    m = (r.random((B, gh * cell, gw * cell)) < 0.5).astype(np.uint8)
    m[:, 0, 0] = 1                                                    # no empty mask: the mean has a denominator
    return dict(feats=_bf(r, (B, gh * gw, D)), masks=_t(m))


def _ffa_cases():
    def call1(x):
        m = x["masks"]
        return (_ops().ffa(x["feats"], m.reshape(m.shape[0], -1), cell=1, normalize=True),)
    _add("ffa_fused_B2", "fp_ffa", lambda which, n=None: _ffa_inputs(which, n or 2, 5, 7, 1), call1, batches=(2, 5, 3))     # arrival counters
    _add("ffa_rows_B17", "fp_ffa", lambda which, n=None: _ffa_inputs(which, 17, 5, 7, 1), call1)                             # row-kernel tail
    _add("ffa_cell14", "fp_ffa", lambda which, n=None: _ffa_inputs(which, 2, 2, 3, 14),
         lambda x: (_ops().ffa(x["feats"], x["masks"], cell=14, normalize=True),))                                           # cell-mask pass


_ffa_cases()


# ---- retrieval --------------------------------------------------------------------------------------------------------------------------------
def _unit_bf16(r, shape):
    x = r.standard_normal(shape)
    return torch.from_numpy((x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)).to(torch.bfloat16)


RERANK = dict(n_mesh=5, views=6, Q=2, C=3, D=64, k=4)


def _rerank_check(x):
    off, cand = x["offsets"].numpy(), x["cand"].numpy()
    assert off[0] == 0 and (np.diff(off) >= RERANK["k"]).all() and off[-1] == x["views"].shape[0], "rerank offsets"
    assert cand.min() >= 0 and cand.max() < len(off) - 1, "rerank candidates outside the mesh list"


def _retrieval_cases():
    _add("bank_prepare", "fp_bank_prepare", lambda which, n=None: dict(bank=_f32(_seed(which, 1100), (300, 384))),
         lambda x: (_ops().bank_prepare(x["bank"]),))
    _add("bank_topk", "fp_bank_topk", lambda which, n=None: dict(bank=_unit_bf16(_seed(which, 1110), (300, 384)), q=_unit_bf16(_seed(which, 1111), (3, 384))),
         lambda x: _ops().bank_topk(x["bank"], x["q"], k=10))

    def merge(which, n=None):
        r = _seed(which, 1120)
        return dict(s=_f32(r, (3, 32)), i=_t(np.stack([r.permutation(1000)[:32] for _ in range(3)]).astype(np.int32)))
    _add("topk_merge", "fp_topk_merge", merge, lambda x: _ops().topk_merge(x["s"], x["i"], 8))

    def rerank(which, n=None):
        r, c = _seed(which, 1130), RERANK
        return dict(views=_bf(r, (c["n_mesh"] * c["views"], c["D"])), offsets=_t(np.arange(c["n_mesh"] + 1, dtype=np.int32) * c["views"]),
                    cand=_t(np.stack([r.permutation(c["n_mesh"])[:c["C"]] for _ in range(c["Q"])]).astype(np.int32)), q=_bf(r, (c["Q"], c["D"])))
    _add("rerank_views", "fp_rerank_views", rerank, lambda x: (_ops().rerank_views(x["views"], x["offsets"], x["cand"], x["q"], RERANK["k"]),),
         check=_rerank_check)

    def tmpl(which, n=None):
        r = _seed(which, 1140)
        return dict(tmpl=_bf(r, (4, 35, 64)), q=_bf(r, (35, 64)), w=torch.from_numpy(r.random((4, 35), dtype=np.float32)))
    _add("template_score", "fp_template_score", tmpl, lambda x: (_ops().template_score(x["tmpl"], x["q"], x["w"]),))
    _add("template_score_normed", "fp_template_score_normed",
         lambda which, n=None: dict(tmpl=_unit_bf16(_seed(which, 1150), (4, 35, 64)), q=_unit_bf16(_seed(which, 1151), (35, 64))),
         lambda x: (_ops().template_score(x["tmpl"], x["q"], normalized=True),))
    _add("knn_l2", "fp_knn_l2", lambda which, n=None: dict(table=_f32(_seed(which, 1160), (12, 64)), q=_f32(_seed(which, 1161), (2, 64))),
         lambda x: _ops().knn_l2(x["table"], x["q"], 3))


_retrieval_cases()


# ---- pose -------------------------------------------------------------------------------------------------------------------------------------
CROP_HW = (40, 50)


def _boxes(r, n, H, W):
    x0, y0 = r.integers(0, W - 12, n), r.integers(0, H - 12, n)
    return np.stack([x0, y0, x0 + r.integers(6, 12, n), y0 + r.integers(6, 12, n)], 1).astype(np.int32)


def _boxes_check(x):
    b, (H, W) = x["boxes"].numpy(), CROP_HW
    assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] <= W).all() and (b[:, 3] <= H).all() and (b[:, 2] > b[:, 0]).all() and \
        (b[:, 3] > b[:, 1]).all(), "crop boxes"


def _rois_check(x):
    r = x["rois"].numpy()
    assert set(r[:, 0].tolist()) <= {0.0, 1.0} and (r[:, 1:] >= 0).all() and (r[:, 3] > r[:, 1]).all() and (r[:, 4] > r[:, 2]).all(), "rois"


GEO_G, GEO_RPREV = 1025, _rodrigues(np.array([0.3, -0.2, 0.5]))


def _pose_cases():
    H, W = CROP_HW
    _add("crop_u8_rgb", "fp_crop_resize_pad",
         lambda which, n=None: dict(images=_t(_seed(which, 1200).integers(0, 256, (1, H, W, 3)).astype(np.uint8)), boxes=_t(_boxes(_seed(which, 1201), 3, H, W))),
         lambda x: (_ops().crop_resize_pad(x["images"], x["boxes"], 16, bbox_extend=0.1),), check=_boxes_check)      # u8, C=3, even target: the RGB kernel

    def generic(which, n=None):
        r = _seed(which, 1210)
        return dict(images=torch.from_numpy(r.random((1, 3, H, W), dtype=np.float32)), boxes=_t(_boxes(r, 3, H, W)),
                    masks=_t((r.random((3, H, W)) < 0.7).astype(np.uint8)))
    _add("crop_generic", "fp_crop_resize_pad", generic,
         lambda x: (_ops().crop_resize_pad(x["images"], x["boxes"], 15, masks=x["masks"], mask_mode=1),), check=_boxes_check)

    def rois(which, n=None):
        r = _seed(which, 1220)
        x1, y1 = r.uniform(0, 10, 3), r.uniform(0, 8, 3)
        rr = np.stack([np.array([0, 1, 0]), x1, y1, x1 + r.uniform(3, 12, 3), y1 + r.uniform(3, 10, 3)], 1).astype(np.float32)
        return dict(images=_f32(r, (2, 3, 20, 24)), rois=_t(rr))
    _add("roi_align", "fp_roi_align", rois, lambda x: (_ops().roi_align(x["images"], x["rois"], 7, sampling_ratio=2),), check=_rois_check)

    def grid(which, n=None):
        g = _ops().generate_rotations(GEO_G)                             # host-only entry
        return dict(grid=_t(g if which == "A" else g[np.random.default_rng(5).permutation(GEO_G)]))

    def geo(x):
        idx = _ops().geodesic_select(x["grid"], GEO_RPREV, 40.0)
        out = torch.full((GEO_G + 1,), -1, dtype=torch.int64)
        out[0] = len(idx)
        out[1:1 + len(idx)] = torch.from_numpy(idx)
        return (out,)
    _add("geodesic_select", "fp_geodesic_select", grid, geo, waits=True)

    def depth(which, Hh, Ww):
        r = _seed(which, 1230 + Ww)
        d = np.zeros((3, Hh, Ww), np.float32)
        for i in range(3):
            y0, x0 = r.integers(2, 12, 2)
            d[i, y0:y0 + 20 + i, x0:x0 + 25 + i] = (0.8 + 0.2 * r.random((20 + i, 25 + i))).astype(np.float32)
        return dict(depth=_t(d))
    _add("depth_extents_vec", "fp_depth_extents", lambda which, n=None: depth(which, 48, 64),
         lambda x: (_ops().depth_extents(x["depth"], 80.0, 81.0, 31.5, 23.5),))
    _add("depth_extents_scalar", "fp_depth_extents", lambda which, n=None: depth(which, 47, 63),
         lambda x: (_ops().depth_extents(x["depth"], 80.0, 81.0, 31.5, 23.5),))


_pose_cases()


# ---- rasteriser -------------------------------------------------------------------------------------------------------------------------------
RASTER = dict(scale=0.25, fx=80.0, fy=80.0, cx=32.0, cy=32.0, W=64, H=64)


def _poses(which, n):
    r = _seed(which, 1300 + n)
    p = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    for i in range(n):
        p[i, :3, :3] = _rodrigues(r.uniform(-1.0, 1.0, 3))
        p[i, :3, 3] = (r.uniform(-0.05, 0.05), r.uniform(-0.05, 0.05), r.uniform(0.9, 1.1))
    return dict(poses=_t(p))


def _mesh():
    import bench
    return _obj("mesh", lambda: _ops().Mesh(*bench.synthetic_mesh(2)))


def _raster_cases():
    c = RASTER

    def with_tiled(tiled, fn):
        def call(x):
            ops = _ops()
            ops.set_option("raster_tiled", tiled)
            try:
                return fn(ops, x)
            finally:
                ops.set_option("raster_tiled", -1)
        return call
    for tiled in (0, 1):
        _add(f"rasterize_tiled{tiled}", "fp_rasterize", lambda which, n=None: _poses(which, n or 3),
             with_tiled(tiled, lambda ops, x: ops.rasterize(_mesh(), x["poses"], c["scale"], c["fx"], c["fy"], c["cx"], c["cy"], c["W"], c["H"])),
             batches=(3, 5, 2) if tiled else None)
        _add(f"rasterize_extents_tiled{tiled}", "fp_rasterize_extents", lambda which, n=None: _poses(which, 3),
             with_tiled(tiled, lambda ops, x: ops.rasterize_extents(_mesh(), x["poses"], c["scale"], c["fx"], c["fy"], c["cx"], c["cy"], c["W"], c["H"],
                                                                    want_depth=True)))
        _add(f"project_vertices_tiled{tiled}", "fp_project_vertices", lambda which, n=None: _poses(which, 3),
             with_tiled(tiled, lambda ops, x: ops.project_vertices(_mesh(), x["poses"], c["scale"], c["fx"], c["fy"], c["cx"], c["cy"])))


_raster_cases()


# ---- depth-map scale --------------------------------------------------------------------------------------------------------------------------
def _scale_cases_():
    from tests import _scale_cases as sc

    def chain(which):
        c = sc.chain_case()
        depth = c["depth"] if which == "A" else np.ascontiguousarray(sc.plane(70, 90, seed=11), dtype=np.float64)
        return c, depth
    _add("label_components", "fp_label_components",
         lambda which, n=None: dict(masks=_t((chain(which)[0]["masks"] if which == "A" else chain(which)[0]["masks"][:, :, ::-1]).astype(np.uint8))),
         lambda x: (_ops().label_components(x["masks"], 4),))

    def build(which, n=None):
        c, depth = chain(which)
        return dict(depth=_t(depth), masks=_t(c["masks"].astype(np.uint8)))

    def call(x):                                                        # the wrapper reads `info` back to refuse empty masks: the C entry directly
        L, ops = _lib(), _ops()
        K = sc.intrinsics(70, 90)
        d, m = x["depth"], x["masks"]
        n, H, W = m.shape
        scales = torch.empty((n,), dtype=torch.float64, device=d.device)
        info = torch.zeros((n, 4), dtype=torch.int32, device=d.device)
        keep = torch.empty((n, H, W), dtype=torch.uint8, device=d.device)
        L.check(L.load().fp_depthmap_scale(ops.context(), L.ptr(d), L.ptr(m), n, H, W, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
                                           8.0, 1.5, 25, 1, L.ptr(scales), L.ptr(info), L.ptr(keep), L.current_stream()), "fp_depthmap_scale")
        return scales, info, keep
    _add("depthmap_scales", "fp_depthmap_scale", build, call, check=lambda x: _assert(bool((x["masks"].reshape(6, -1).sum(1) > 0).all()), "empty mask"))


def _assert(ok, what):
    assert ok, what


_scale_cases_()


# ---- refiner ----------------------------------------------------------------------------------------------------------------------------------
REFINE_K = np.array([[600.0, 0.0, 320.0], [0.0, 600.0, 240.0], [0.0, 0.0, 1.0]])


def _refiner_cases():
    def pp(which, n=None):
        r = _seed(which, 1500)
        T = np.tile(np.eye(4), (3, 1, 1))
        for i in range(3):
            T[i, :3, :3] = _rodrigues(r.uniform(-0.5, 0.5, 3))
            T[i, :3, 3] = (r.uniform(-0.02, 0.02), r.uniform(-0.02, 0.02), r.uniform(0.9, 1.1))
        cells = np.stack([r.integers(18, 28, (3, 16)), r.integers(13, 22, (3, 16))], -1).astype(np.int32)       # around the projected object
        return dict(samples=_t(r.uniform(-0.1, 0.1, (256, 3))), T=_t(T), K=_t(np.tile(REFINE_K, (3, 1, 1))), cells=_t(cells),
                    ncells=_t(np.array([16, 9, 12], np.int32)))
    _add("patch_points", "fp_patch_points", pp, lambda x: (_ops().patch_points(x["samples"], x["T"], x["K"], x["cells"], x["ncells"]),),
         check=lambda x: _assert(int(x["ncells"].min()) >= 0 and int(x["ncells"].max()) <= x["cells"].shape[1], "ncells"))

    def pnp(which, n=None):
        r = _seed(which, 1510)
        p3 = r.uniform(-0.1, 0.1, (65, 3))
        p2 = np.zeros((3, 65, 2))
        for i in range(3):
            Xc = p3 @ _rodrigues(r.uniform(-0.5, 0.5, 3)).T + np.array([r.uniform(-0.02, 0.02), r.uniform(-0.02, 0.02), r.uniform(0.9, 1.1)])
            uvw = Xc @ REFINE_K.T
            p2[i] = uvw[:, :2] / uvw[:, 2:] + 0.3 * r.standard_normal((65, 2))
        vis = (r.random((3, 65)) < 0.8).astype(np.uint8)
        vis[:, :8] = 1
        return dict(p3=_t(p3), p2=_t(p2), K=_t(REFINE_K.copy()), vis=_t(vis))
    _add("pnp_epnp", "fp_pnp_epnp", pnp, lambda x: (_ops().pnp_epnp(x["p3"], x["p2"], x["K"], x["vis"]),))


_refiner_cases()


# ---- tracker ----------------------------------------------------------------------------------------------------------------------------------
LK_T, LK_H, LK_W = 3, 72, 88                                          # the edge_clip of tests/test_gpu_lk_tracker.py


def _tracker_cases():
    def frames(which):
        from tests import _lk_ref as ref
        return ref.render(ref.Texture(7 if which == "A" else 8), ref.Translation(0.9, -0.6), LK_T, LK_H, LK_W)

    def queries(which):
        r = _seed(which, 1600)
        return np.stack([np.arange(5) % 3, r.uniform(16, LK_W - 17, 5), r.uniform(16, LK_H - 17, 5)], 1).astype(np.float32)

    def params():
        from tests import _lk_ref as ref
        return dict(ref.PARAMS)
    _add("lk_pyramid", "fp_lk_pyramid", lambda which, n=None: dict(frames=_t(frames(which))),
         lambda x: (_ops().lk_pyramid(x["frames"], params()["levels"], params()["radius"]),))

    def track(x):
        ops, p = _ops(), params()
        pyr = ops.lk_pyramid(x["frames"], p["levels"], p["radius"])
        return ops.lk_track(pyr, LK_T, LK_H, LK_W, x["queries"], **p)
    _add("lk_track", ("fp_lk_track", "fp_lk_pyramid"), lambda which, n=None: dict(frames=_t(frames(which)), queries=_t(queries(which))), track)


_tracker_cases()


# ---- evaluation -------------------------------------------------------------------------------------------------------------------------------
CHAMFER_SIZES = (20, 30)
EVAL_K = np.array([[572.4, 0.0, 325.3], [0.0, 573.6, 242.0], [0.0, 0.0, 1.0]])


def _chamfer_tables(which, projected):
    """what ops._chamfer packs on the host for two pairs (cloud 0 against cloud 1, cloud 1 against itself), as device inputs"""
    r = _seed(which, 1700)
    clouds = [r.uniform(-50.0, 50.0, (n, 3)) for n in CHAMFER_SIZES]
    pts = np.concatenate(clouds)
    starts = np.concatenate([[0], np.cumsum(CHAMFER_SIZES)])
    pairs = np.array([[0, 1], [1, 1]])
    n_e, n_g = np.array(CHAMFER_SIZES)[pairs[:, 0]], np.array(CHAMFER_SIZES)[pairs[:, 1]]
    table = np.zeros((2, 8), np.int32)
    table[:, 0], table[:, 1], table[:, 2], table[:, 3] = starts[pairs[:, 0]], n_e, starts[pairs[:, 1]], n_g
    slot = np.concatenate([[0], np.cumsum(n_e + n_g)])
    table[:, 4], table[:, 5] = slot[:-1], slot[:-1] + n_e
    xf = np.zeros((2, 40))
    for b in range(2):
        xf[b, 0] = r.uniform(0.9, 1.1)
        xf[b, 1:10] = _rodrigues(r.uniform(-1, 1, 3)).ravel()
        xf[b, 10:13] = (r.uniform(-20, 20), r.uniform(-20, 20), r.uniform(900, 1100))
        xf[b, 13:22] = _rodrigues(r.uniform(-1, 1, 3)).ravel()
        xf[b, 22:25] = (r.uniform(-20, 20), r.uniform(-20, 20), r.uniform(900, 1100))
        xf[b, 25:28] = clouds[pairs[b, 1]].mean(0)
        if projected:
            xf[b, 28:37] = EVAL_K.ravel()
    return dict(pts=_t(pts), table=_t(table), xf=_t(xf))


def _chamfer_check(x):
    t, n_pts = x["table"].numpy().astype(np.int64), x["pts"].shape[0]
    ws = int((t[:, 1] + t[:, 3]).sum())
    assert (t[:, [1, 3]] > 0).all() and (t[:, 0] >= 0).all() and (t[:, 0] + t[:, 1] <= n_pts).all() and (t[:, 2] + t[:, 3] <= n_pts).all(), "chamfer clouds"
    assert (t[:, 4] >= 0).all() and (t[:, 5] == t[:, 4] + t[:, 1]).all() and (t[:, 5] + t[:, 3] <= ws).all(), "chamfer workspace slots"


def _chamfer_call(projected):
    def call(x):
        L, ops = _lib(), _ops()
        out = torch.empty((2,), dtype=torch.float64, device=x["pts"].device)
        L.check(L.load().fp_chamfer(ops.context(), L.ptr(x["pts"]), int(x["pts"].shape[0]), L.ptr(x["table"]), L.ptr(x["xf"]), 2, max(CHAMFER_SIZES),
                                    2 * CHAMFER_SIZES[1] + sum(CHAMFER_SIZES), projected, L.ptr(out), L.current_stream()), "fp_chamfer")
        return (out,)
    return call


def _gt_edges(which):
    from tests import _gt_info_ref as ref
    c = ref.vis_cases()["edges"]
    gt, test = c["depth_gt"], c["depth_test"]
    if which == "B":                                                    # other depths under the same silhouettes: still positive, still millimetres
        gt, test = np.where(gt > 0, gt + np.float32(9.0), gt), np.where(test > 0, test + np.float32(4.0), test)
    return c, np.ascontiguousarray(gt, np.float32), np.ascontiguousarray(test, np.float32)


BOP = dict(P=9, Gr=3, R=5, T=2, n_obj=2, n_scene=2, n_top=0)


def _bop_tables(which):
    r = _seed(which, 1800)
    groups = np.array([[0, 2, 2, 0], [4, 3, 1, 2], [7, 1, 2, 3]], np.int32)          # {err_offset, E, G, first_gt_row}
    return dict(err=_t(r.uniform(0.0, 1.0, BOP["P"])), groups=_t(groups), valid=_t(np.array([1, 1, 1, 0, 1], np.uint8)),
                obj=_t(np.array([0, 0, 1, 1, 1], np.int32)), scene=_t(np.array([0, 0, 0, 1, 1], np.int32)), th=_t(np.array([0.3, 0.6])))


def _bop_check(x):
    _ops().bop_tables_check(x["err"].numpy(), x["groups"].numpy(), x["valid"].numpy(), x["obj"].numpy(), x["scene"].numpy(), x["th"].numpy(),
                            BOP["n_obj"], BOP["n_scene"])


def _eval_cases():
    _add("chamfer", "fp_chamfer", lambda which, n=None: _chamfer_tables(which, 0), _chamfer_call(0), check=_chamfer_check)
    _add("chamfer_proj", "fp_chamfer", lambda which, n=None: _chamfer_tables(which, 1), _chamfer_call(1), check=_chamfer_check)

    def dc(which, n=None):
        r = _seed(which, 1710)
        def stack(k):
            d = (1000.0 + 40.0 * r.random((k, 10, 12))).astype(np.float32)
            d[r.random((k, 10, 12)) < 0.3] = 0.0
            return d
        prm = np.zeros((2, 8))
        prm[:] = [80.0, 82.0, 5.5, 4.5, 15.0, 100.0, 0.0, 0.0]
        return dict(est=_t(stack(2)), gt=_t(stack(2)), test=_t(stack(2)), idx=_t(np.array([1, 0], np.int32)), prm=_t(prm), taus=_t(np.array([0.05, 0.2, 0.5])))

    def dc_call(x):                                                     # the wrapper uploads idx / params / taus itself: the C entry directly
        L, ops = _lib(), _ops()
        out = torch.empty((2, 7), dtype=torch.int32, device=x["est"].device)
        L.check(L.load().fp_depth_compare(ops.context(), L.ptr(x["est"]), L.ptr(x["gt"]), 2, 10, 12, L.ptr(x["test"]), 2, L.ptr(x["idx"]), L.ptr(x["prm"]),
                                          L.ptr(x["taus"]), 3, L.ptr(out), L.current_stream()), "fp_depth_compare")
        return (out,)
    _add("depth_compare", "fp_depth_compare", dc, dc_call,
         check=lambda x: _assert(int(x["idx"].min()) >= 0 and int(x["idx"].max()) < x["test"].shape[0], "depth_compare img_idx"))

    def vis(which, n=None):
        _, gt, test = _gt_edges(which)
        return dict(depth_gt=_t(gt), depth_test=_t(test))

    def vis_call(x):
        c = _gt_edges("A")[0]
        return _ops().gt_visibility(x["depth_gt"], x["depth_test"], c["img_idx"], c["K"], c["delta"], window=c["window"])

    def vis_check(x):
        c = _gt_edges("A")[0]
        assert min(c["img_idx"]) >= 0 and max(c["img_idx"]) < x["depth_test"].shape[0] and len(c["img_idx"]) == x["depth_gt"].shape[0], "gt_visibility img_idx"
    _add("gt_visibility", "fp_gt_visibility", vis, vis_call, waits=True, check=vis_check)

    def clouds(which, n=None):
        from tests import _gt_info_ref as ref
        if which == "A":
            cl = ref.diam_cases(big=False)["tiny"] + [ref.diam_cases(big=False)["tiles"][2]]                       # 1, 2, 3 and TILE + 1 points
        else:
            r = _seed(which, 1720)
            cl = [r.normal(size=(k, 3)) for k in (1, 2, 3)] + [50.0 * r.normal(size=(ref.TILE + 1, 3))]
        assert [len(c) for c in cl] == [1, 2, 3, ref.TILE + 1]
        return {f"c{i}": _t(np.ascontiguousarray(c, np.float64)) for i, c in enumerate(cl)}
    _add("pts_diameter", "fp_pts_diameter", clouds, lambda x: (_ops().pts_diameter([x[f"c{i}"] for i in range(4)]),), waits=True)

    def tracks(which, n=None):
        r = _seed(which, 1730)
        def traj():
            out, R, t = np.zeros((21, 12)), _rodrigues(r.uniform(-1, 1, 3)), np.array([r.uniform(-0.1, 0.1), r.uniform(-0.1, 0.1), r.uniform(0.8, 1.2)])
            for k in range(21):
                R, t = _rodrigues(r.uniform(-0.05, 0.05, 3)) @ R, t + r.uniform(-0.01, 0.01, 3)
                out[k, :9], out[k, 9:] = R.ravel(), t
            return out
        return dict(est=_t(np.stack([traj(), traj()])), gt=_t(np.stack([traj(), traj()])))
    _add("video_errors", "fp_video_errors", tracks,
         lambda x: _ops().video_errors(x["est"], x["gt"], [1, 2, 5], 0.1, 0.11, 640, 480, sym_axis=[0.0, 0.0, 1.0], n_sym=11), waits=True)

    def bop_call(x):                                                    # the wrapper uploads its host tables itself: the C entry directly
        L, ops, b = _lib(), _ops(), BOP
        dev = x["err"].device
        match = torch.empty((b["T"], b["R"]), dtype=torch.int32, device=dev)
        tp_obj, tp_scene = torch.empty((b["T"], b["n_obj"]), dtype=torch.int32, device=dev), torch.empty((b["T"], b["n_scene"]), dtype=torch.int32, device=dev)
        tar_obj, tar_scene = torch.empty((b["n_obj"],), dtype=torch.int32, device=dev), torch.empty((b["n_scene"],), dtype=torch.int32, device=dev)
        L.check(L.load().fp_bop_scores(ops.context(), L.ptr(x["err"]), L.ptr(x["groups"]), L.ptr(x["valid"]), L.ptr(x["obj"]), L.ptr(x["scene"]), L.ptr(x["th"]),
                                       b["P"], b["Gr"], b["R"], b["T"], b["n_obj"], b["n_scene"], b["n_top"], L.ptr(match), L.ptr(tp_obj), L.ptr(tp_scene),
                                       L.ptr(tar_obj), L.ptr(tar_scene), L.current_stream()), "fp_bop_scores")
        return match, tp_obj, tp_scene, tar_obj, tar_scene
    _add("bop_scores", "fp_bop_scores", lambda which, n=None: _bop_tables(which), bop_call, check=_bop_check)


_eval_cases()


# ---- the gathers of comm.hip on one rank, no communicator ---------------------------------------------------------------------------------------
def _comm_cases():
    def bytes_call(x):
        L, ops = _lib(), _ops()
        out = torch.empty_like(x["send"])
        L.check(L.load().fp_allgather_bytes(ops.context(), L.ptr(x["send"]), x["send"].numel(), L.ptr(out), L.current_stream()), "fp_allgather_bytes")
        return (out,)
    _add("allgather_bytes", "fp_allgather_bytes", lambda which, n=None: dict(send=_t(_seed(which, 1900).integers(0, 256, 1000).astype(np.uint8))), bytes_call)

    def poses_call(x):
        L, ops = _lib(), _ops()
        out = torch.empty_like(x["rows"])
        L.check(L.load().fp_allgather_poses(ops.context(), L.ptr(x["rows"]), 2, 19, L.ptr(out), L.current_stream()), "fp_allgather_poses")
        return (out,)
    _add("allgather_poses", "fp_allgather_poses", lambda which, n=None: dict(rows=_f64(_seed(which, 1910), (2, 19))), poses_call)

    def topk(which, n=None):
        r = _seed(which, 1920)
        return dict(s=_t(np.sort(r.random((3, 16)).astype(np.float32), axis=1)[:, ::-1].copy()), i=_t(r.permutation(48).reshape(3, 16).astype(np.int32)))

    def topk_call(x):
        L, ops = _lib(), _ops()
        os_, oi = torch.empty((3, 8), dtype=torch.float32, device=x["s"].device), torch.empty((3, 8), dtype=torch.int32, device=x["s"].device)
        L.check(L.load().fp_allgather_topk(ops.context(), L.ptr(x["s"]), L.ptr(x["i"]), 3, 16, 8, L.ptr(os_), L.ptr(oi), L.current_stream()), "fp_allgather_topk")
        return os_, oi
    _add("allgather_topk", "fp_allgather_topk", topk, topk_call)


_comm_cases()


# ---- stateful objects -------------------------------------------------------------------------------------------------------------------------
VIT_NAME, CLIP_NAME, TEXT_NAME = "dinov2_vits14_reg", "tiny-64-s56", "tiny-64-c17"


def _images(which, n, H, W, base):
    return dict(images=torch.from_numpy(_seed(which, base + n).random((n, 3, H, W), dtype=np.float32)).to(torch.bfloat16))


def _vit(key):
    return _obj(key, lambda: _ops().ViT(VIT_NAME, _ops().random_state_dict(VIT_NAME, seed=2)))


def _text_ids(which, n):
    ops = _ops()
    vocab, ctx = ops.CLIP_TEXT_ARCHS[TEXT_NAME][4], ops.CLIP_TEXT_ARCHS[TEXT_NAME][5]
    ids = _seed(which, 2100 + n).integers(1, vocab - 1, (n, ctx)).astype(np.int32)
    ids[:, -3:] = 0
    ids[np.arange(n), ctx - 4 - np.arange(n) % 5] = vocab - 1           # the end-of-text token: the one largest id of each prompt
    return dict(ids=_t(ids))


def _ids_check(x):
    vocab = _ops().CLIP_TEXT_ARCHS[TEXT_NAME][4]
    assert int(x["ids"].min()) >= 0 and int(x["ids"].max()) < vocab, "token ids outside the vocabulary"


def _stateful_cases():
    def vit_call(key, fused):
        def call(x):
            ops = _ops()
            v = _vit(key)
            ops.set_option("ln_fused", fused)
            try:
                return (v(x["images"], layer=2, feature_type="patch"),)
            finally:
                ops.set_option("ln_fused", -1)
        return call
    for fused in (1, 0):
        tag = "fused" if fused else "unfused"
        _add(f"vit_28x42_{tag}", "fp_vit_forward", lambda which, n=None: _images(which, n or 2, 28, 42, 2000), vit_call(f"vit_28x42_{tag}", fused),
             batches=(2, 5, 3))                                         # resized position rows
        _add(f"vit_native_{tag}", "fp_vit_forward", lambda which, n=None: _images(which, n or 1, 518, 518, 2010), vit_call(f"vit_native_{tag}", fused),
             batches=(1, 2, 1))                                         # the 37 x 37 grid: no resize
    _add("clip_visual", "fp_clip_encode_image", lambda which, n=None: _images(which, n or 2, 56, 56, 2020),
         lambda x: (_obj("clip_visual", lambda: _ops().ClipVisual(CLIP_NAME, _ops().random_clip_state_dict(CLIP_NAME, seed=4)))(x["images"]),),
         batches=(2, 5, 3))
    _add("clip_text", "fp_clip_text_encode", lambda which, n=None: _text_ids(which, n or 3),
         lambda x: (_obj("clip_text", lambda: _ops().ClipText(TEXT_NAME, _ops().random_clip_text_state_dict(TEXT_NAME, seed=6)))(x["ids"]),),
         waits=True, check=_ids_check, batches=(3, 5, 2))

    # the weight setters that copy: the patch / projection weights are repacked on the setter's stream
    def w_build(shape, base, images):
        def build(which, n=None):
            d = dict(w=_bf(_seed(which, base), shape, 0.02))
            d.update(images("A"))
            return d
        return build

    def vit_set(x):
        ops = _ops()
        v = _vit("vit_set_weight")                                      # never runs folded: replacing a weight asks for no re-fold
        ops.set_option("ln_fused", 0)
        try:
            ops.check(v.lib.fp_vit_set_weight(v.handle, b"patch_embed.proj.weight", ops.ptr(x["w"]), x["w"].numel(), _lib().current_stream()), "fp_vit_set_weight")
            return (v(x["images"], layer=1, feature_type="patch"),)
        finally:
            ops.set_option("ln_fused", -1)
    _add("vit_set_weight", ("fp_vit_set_weight", "fp_vit_forward"), w_build((384, 3, 14, 14), 2200, lambda w: _images(w, 2, 28, 42, 2000)), vit_set, late=("w",))

    def clip_set(x):
        ops = _ops()
        v = _obj("clip_set_weight", lambda: ops.ClipVisual(CLIP_NAME, ops.random_clip_state_dict(CLIP_NAME, seed=4)))
        ops.check(v.lib.fp_clip_set_weight(v.handle, b"conv1.weight", ops.ptr(x["w"]), x["w"].numel(), _lib().current_stream()), "fp_clip_set_weight")
        ops.check(v.lib.fp_clip_set_weight(v.handle, b"proj", ops.ptr(x["proj"]), x["proj"].numel(), _lib().current_stream()), "fp_clip_set_weight")
        return (v(x["images"]),)

    def clip_w(which, n=None):
        d = w_build((128, 3, 14, 14), 2210, lambda w: _images(w, 2, 56, 56, 2020))(which)
        d["proj"] = _bf(_seed(which, 2211), (128, 64), 128 ** -0.5)
        return d
    _add("clip_set_weight", ("fp_clip_set_weight", "fp_clip_encode_image"), clip_w, clip_set, late=("w", "proj"))

    def text_set(x):
        ops = _ops()
        v = _obj("clip_text_set_weight", lambda: ops.ClipText(TEXT_NAME, ops.random_clip_text_state_dict(TEXT_NAME, seed=6)))
        ops.check(v.lib.fp_clip_text_set_weight(v.handle, b"text_projection", ops.ptr(x["w"]), x["w"].numel(), _lib().current_stream()), "fp_clip_text_set_weight")
        return (v(x["ids"]),)

    def text_w(which, n=None):
        d = dict(w=_bf(_seed(which, 2220), (128, 64), 128 ** -0.5))
        d.update(_text_ids("A", 3))
        return d
    _add("clip_text_set_weight", ("fp_clip_text_set_weight", "fp_clip_text_encode"), text_w, text_set, late=("w",), waits=True, check=_ids_check)


_stateful_cases()


# ---- the event timer of bench.py ------------------------------------------------------------------------------------------------------------------
_TIMER = []


def timer():
    """the one fp_timer of the process (its events are re-recorded by every use; never destroyed while a record may be pending)"""
    if not _TIMER:
        L, t = _lib(), C.c_void_p()
        L.check(L.load().fp_timer_create(C.byref(t)), "fp_timer_create")
        _TIMER.append(t)
    return _TIMER[0]


def _timer_cases():
    def call(x):
        L, ops = _lib(), _ops()
        lib, t = L.load(), timer()
        L.check(lib.fp_timer_start(t, L.current_stream()), "fp_timer_start")
        y = ops.l2_normalize(x["x"])
        L.check(lib.fp_timer_stop(t, L.current_stream()), "fp_timer_stop")
        return (y,)
    # the events themselves are held to their stream by tests/test_gpu_streams.py::test_timer_events_are_recorded_on_the_given_stream
    _add("timer", ("fp_timer_start", "fp_timer_stop", "fp_l2_normalize"), lambda which, n=None: dict(x=_bf(_seed(which, 2300), (37, 384))), call)


_timer_cases()

MUTANTS = tuple(c.name for c in CASES if c.mutant)
HANDOVER = tuple(c.name for c in CASES if c.batches)
