"""The harness and the case table of the buffer contract (include/freepose_hip.h states the shape of every output): a call writes every
documented byte of its outputs, nothing outside them — not past the end, not into the gap between the rows of a strided output — and its
result depends on nothing outside the documented extent of its inputs.  tests/test_extent_cases_cpu.py holds the table to the header and
proves the harness on the host with numpy writers; tests/test_gpu_extents.py runs every case on the device.

Importing this module needs no GPU and does not load the library.

  Region   one device buffer of a call: name, dtype, shape, ld (row stride in elements where the entry takes one), role in | out | inout;
           `data` the CPU tensor an in / inout region holds, `index_like` (tables, ranges, ids, counts: their guards hold zeros, a valid
           index), `shift` elements between a 16-byte boundary and the start of the extent (the three alignment placements only), `quote`
           the header text that states the shape and dtype of an output and `dims` the values of the names in it
  embed    one flat uint8 buffer per region, guard | extent | guard: 4096-byte guards, the extent on a 256-byte boundary, stride gaps
           count as guard, everything but the data of in / inout regions filled with one byte
  run      four calls of the entry: twice into exact-fit tensors (bit-identical, or the entry is not repeatable), once embedded under the
           fill 0xFF (NaN in every float type, -1 in every integer type) and once under 0x5A (finite and non-zero in every type); then
           every NEVER byte still holds what it held, the MUST bytes of the two embedded runs are equal (written) and equal to the exact-fit
           run (nothing outside the documented inputs reached them), and — where the public wrapper hands back the entry's own buffer — equal
           to what the stream table's `call` returns for the same inputs

A case is
  name      the test id
  entries   the C entries the call runs
  inputs    () -> {name: CPU tensor}: set "A" of the stream table (tests/_stream_cases.py), or a second shape where that one hides a tail
  regions   (x) -> [Region]: every device buffer handed to the entry
  call      (P, x) -> {name: host value} | None; P[name] is the Placed buffer of a region (P[name].ptr, P[name].ld); enqueues on torch's
            current stream through freepose_amd._lib
  mask      (x, host) -> {region: uint8 array of the region's shape with MUST / NEVER / FREE per element}; regions it leaves out are all MUST
  free      {region: the sentence of the header behind its FREE bytes}
  wrapper   (stream case, {region: index into what its `call` returns}): outputs the public wrapper hands back unchanged
  host_example   the host values `mask` is given by the CPU test (cases whose mask depends on a count the call returns)
"""
import ctypes as C
import re
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import torch

from tests import _stream_cases as sc

NEVER, MUST, FREE = 0, 1, 2
GUARD, ALIGN = 4096, 256
FILLS = (0xFF, 0x5A)
MAX_PINNED, MAX_FREE_CASES = 16, 6

# entry -> "tests/file.py::test_name": a test that already pre-fills the entry's output and asserts the guard rows and columns around it
PINNED_ELSEWHERE = {
    "fp_op_gemm": "tests/test_gpu_gemm_branches.py::test_tiny",
    "fp_op_gemm_vt": "tests/test_gpu_gemm_branches.py::test_vt",
    "fp_op_gemm_patch": "tests/test_gpu_gemm_branches.py::test_patch",
    "fp_op_ln_chain": "tests/test_gpu_gemm_branches.py::test_ln_chain",
    "fp_op_attention": "tests/test_gpu_attention_exact.py::test_attention_exact",
    "fp_op_attention_hd": "tests/test_gpu_attention_hd.py::test_attention_hd",
    "fp_op_attention_causal": "tests/test_gpu_attention_causal.py::test_attention_causal",
    "fp_crop_resize_pad": "tests/test_gpu_pose_kernels.py::test_crop_dispatch_matrix",
    "fp_bank_topk": "tests/test_gpu_retrieval_branches.py::test_select_matrix",
    "fp_topk_merge": "tests/test_gpu_retrieval_branches.py::test_topk_merge",
}

DTYPES = {"f64": torch.float64, "f32": torch.float32, "i32": torch.int32, "u32": torch.int32, "u8": torch.uint8, "bf16": torch.bfloat16}


# ---- regions and their placement --------------------------------------------------------------------------------------------------------------
@dataclass
class Region:
    name: str
    dtype: torch.dtype
    shape: tuple
    ld: Optional[int] = None
    role: str = "out"
    data: Optional[torch.Tensor] = None
    index_like: bool = False
    shift: int = 0
    quote: tuple = ()
    dims: dict = field(default_factory=dict)

    def __post_init__(self):
        self.shape = tuple(int(v) for v in self.shape)
        assert self.role in ("in", "out", "inout") and len(self.shape) >= 1 and min(self.shape) >= 1, (self.name, self.role, self.shape)
        assert (self.data is not None) == (self.role != "out"), f"{self.name}: in / inout regions hold data, out regions do not"
        if self.data is not None:
            assert tuple(self.data.shape) == self.shape and self.data.dtype == self.dtype and not self.data.is_cuda, self.name
        assert self.ld is None or self.ld >= self.cols, self.name
        if isinstance(self.quote, str):
            self.quote = (self.quote,)

    @property
    def itemsize(self):
        return torch.empty((), dtype=self.dtype).element_size()

    @property
    def cols(self):
        return self.shape[-1]

    @property
    def rows(self):
        return int(np.prod(self.shape[:-1], dtype=np.int64))

    def stride(self, tight=False):
        return self.cols if tight or self.ld is None else self.ld

    def extent_bytes(self, tight=False):
        return ((self.rows - 1) * self.stride(tight) + self.cols) * self.itemsize

    def data_bytes(self):
        """the data of an in / inout region as uint8 [rows, cols * itemsize]"""
        return self.data.contiguous().reshape(-1).view(torch.uint8).reshape(self.rows, self.cols * self.itemsize)


class Placed:
    """a region inside its flat uint8 buffer: the extent starts `start` bytes in, rows are `ld` elements apart"""

    def __init__(self, region, buf, start, ld):
        self.region, self.buf, self.start, self.ld = region, buf, start, ld

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.start)

    @property
    def nbytes(self):
        r = self.region
        return ((r.rows - 1) * self.ld + r.cols) * r.itemsize

    def rows_u8(self):
        """the rows of the extent as a uint8 view [rows, cols * itemsize] of the buffer (no gaps)"""
        r = self.region
        return torch.as_strided(self.buf, (r.rows, r.cols * r.itemsize), (self.ld * r.itemsize, 1), self.buf.storage_offset() + self.start)

    def typed(self):
        """the rows as a typed view [rows, cols] of the buffer"""
        r = self.region
        flat = self.buf[self.start:self.start + self.nbytes].view(r.dtype)
        return torch.as_strided(flat, (r.rows, r.cols), (self.ld, 1))

    def element(self, index):
        """the element `index` elements from the start of the extent, inside it or in a guard (host writers); None outside the buffer"""
        r = self.region
        o = self.start + index * r.itemsize
        if o < 0 or o + r.itemsize > self.buf.numel():
            return None
        return self.buf[o:o + r.itemsize].view(r.dtype)


def _aligned_bytes(nbytes, device):
    raw = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=device)
    off = (-raw.data_ptr()) % ALIGN
    return raw[off:off + nbytes]


def embed(regions, fill, device="cuda", tight=False):
    """{name: Placed}.  tight: exact-fit, tightly packed, no guards, zero-filled outputs.  Otherwise guard | extent | guard with GUARD bytes
    either side (GUARD + shift elements in front of a shifted extent), rows `ld` apart, and every byte that is not data of an in / inout
    region set to `fill` — zero in the guards and gaps of index-like inputs."""
    out = {}
    for r in regions:
        if tight:
            buf = _aligned_bytes(r.extent_bytes(True), device)
            buf.zero_()
            p = Placed(r, buf, 0, r.cols)
        else:
            start = GUARD + r.shift * r.itemsize
            buf = _aligned_bytes(start + r.extent_bytes() + GUARD, device)
            buf.fill_(0 if (r.role == "in" and r.index_like) else fill)
            p = Placed(r, buf, start, r.stride())
            assert (buf.data_ptr() + GUARD) % ALIGN == 0
        if r.data is not None:
            p.rows_u8().copy_(r.data_bytes())
        out[r.name] = p
    return out


def byte_mask(region, elem_mask, placed):
    """the mask of every byte of a placed region's buffer: guards and gaps NEVER, the extent from the per-element mask"""
    m = np.full(placed.buf.numel(), NEVER, np.uint8)
    em = np.full(region.shape, MUST, np.uint8) if elem_mask is None else np.asarray(elem_mask, np.uint8)
    assert em.shape == region.shape, (region.name, em.shape, region.shape)
    rows = np.repeat(em.reshape(region.rows, region.cols), region.itemsize, axis=1)
    view = np.lib.stride_tricks.as_strided(m[placed.start:], (region.rows, region.cols * region.itemsize), (placed.ld * region.itemsize, 1))
    view[:] = rows
    return m


class ExtentError(AssertionError):
    def __init__(self, case, kind, region, offset, row, col, text):
        self.case, self.kind, self.region, self.offset, self.row, self.col = case, kind, region, offset, row, col
        super().__init__(f"{case}: region {region}: {text} — first at byte offset {offset} of the extent (row {row}, column {col})")


class NotRepeatable(AssertionError):
    """two calls into exact-fit tensors differ: a finding of its own, not a footprint failure"""


def _where(placed, first):
    """(byte offset from the start of the extent, row, column) of byte `first` of the buffer"""
    r = placed.region
    off = int(first) - placed.start
    el = off // r.itemsize
    return off, el // placed.ld, el % placed.ld


def _fail(case, kind, placed, bad, text):
    off, row, col = _where(placed, np.flatnonzero(bad)[0])
    raise ExtentError(case.name, kind, placed.region.name, off, row, col, text)


@dataclass
class ExtentCase:
    name: str
    entries: tuple
    inputs: Callable
    regions: Callable
    call: Callable
    mask: Optional[Callable] = None
    free: dict = field(default_factory=dict)
    wrapper: Optional[tuple] = None
    host_example: Optional[dict] = None


def element_masks(case, x, regions, host):
    got = case.mask(x, host) if case.mask else {}
    names = {r.name for r in regions if r.role != "in"}
    assert set(got) <= names, (case.name, sorted(set(got) - names))
    return got


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _host_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return set(a) == set(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def run(case, device="cuda", entry=None):
    """the four calls and the assertions; `entry` replaces case.call (the host writers of the CPU test)"""
    call = entry or case.call
    x = case.inputs()
    regions = case.regions(x)
    assert len({r.name for r in regions}) == len(regions)
    written = [r for r in regions if r.role != "in"]

    def once(fill, tight):
        P = embed(regions, fill, device, tight)
        before = {n: p.buf.cpu().numpy().copy() for n, p in P.items()}
        host = call(P, x)
        _sync(device)
        return P, before, {n: p.buf.cpu().numpy() for n, p in P.items()}, host

    P1, _, got1, host1 = once(0, True)
    P1b, _, got1b, host1b = once(0, True)
    elem = element_masks(case, x, regions, host1)
    for r in written:
        m = byte_mask(r, elem.get(r.name), P1[r.name]) == MUST
        if not np.array_equal(got1[r.name][m], got1b[r.name][m]):
            raise NotRepeatable(f"{case.name}: region {r.name}: two calls into exact-fit tensors differ — {', '.join(case.entries)} is not repeatable")
    if not _host_equal(host1, host1b):
        raise NotRepeatable(f"{case.name}: the host outputs of two calls differ: {host1} / {host1b}")
    runs = [once(fill, False) for fill in FILLS]
    for (P, before, got, host), fill in zip(runs, FILLS):
        assert _host_equal(host, host1), f"{case.name}: host outputs under fill 0x{fill:02X}: {host}, exact-fit run: {host1}"
        for r in regions:
            p = P[r.name]
            m = byte_mask(r, elem.get(r.name) if r.role != "in" else np.full(r.shape, NEVER, np.uint8), p)
            if r.role != "in":
                free = int((m == FREE).sum())
                assert free == 0 or r.name in case.free, f"{case.name}: region {r.name} has FREE bytes and no sentence of the header behind them"
                assert 2 * free <= r.extent_bytes(True), f"{case.name}: FREE covers more than half of region {r.name}"
            bad = (m == NEVER) & (got[r.name] != before[r.name])
            if bad.any():
                what = "an input was written" if r.role == "in" else "a byte outside the documented extent was written (guard, stride gap or a byte the header says is left alone)"
                _fail(case, "never", p, bad, f"{what}, fill 0x{fill:02X}")
    (Pa, _, ga, _), (Pb, _, gb, _) = runs
    for r in written:
        pa = Pa[r.name]
        m = byte_mask(r, elem.get(r.name), pa) == MUST
        bad = m & (ga[r.name] != gb[r.name])
        if bad.any():
            _fail(case, "unwritten", pa, bad, "a documented byte differs under the two fills: it was never written, or holds a value read from outside an input")
        tight = byte_mask(r, elem.get(r.name), P1[r.name]) == MUST
        if not np.array_equal(ga[r.name][m], got1[r.name][tight]):
            bad = np.zeros_like(m)
            bad[np.flatnonzero(m)[ga[r.name][m] != got1[r.name][tight]]] = True
            _fail(case, "leak", pa, bad, "the embedded result differs from the exact-fit result: something outside the documented inputs reached it")
    if case.wrapper and entry is None:
        name, outs = case.wrapper
        want = sc.by_name(name).call({k: v.cuda() for k, v in sc.by_name(name).build("A").items()})
        torch.cuda.synchronize()
        for rname, i in outs.items():
            r = next(r for r in written if r.name == rname)
            w = want[i].detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy()
            assert w.size == r.extent_bytes(True), (case.name, rname, w.size, r.extent_bytes(True))
            tight = byte_mask(r, elem.get(rname), P1[rname]) == MUST
            bad = tight & (got1[rname] != w)
            if bad.any():
                _fail(case, "wrapper", P1[rname], bad, f"the direct call differs from output {i} of the public wrapper (stream case {name})")
    return host1


# ---- the header ------------------------------------------------------------------------------------------------------------------------------
def header_text(path):
    """the header with comment line prefixes and line breaks folded away, so that a quote may run over a line end"""
    t = path.read_text()
    t = re.sub(r"\n\s*\*\s?", " ", t)
    return re.sub(r"\s+", " ", t)


def parse_quote(quote, dims):
    """(dtype or None, shape) a tuple of header fragments states: the shape is the last [...] of the first fragment, the dtype the first
    type token (f64 f32 i32 u32 u8 bf16, free-standing or as the tail of a pointer's name) of any fragment"""
    text = quote[0]
    inner = text[text.rindex("[") + 1:text.rindex("]")]
    parts, depth, cur = [], 0, ""
    for ch in inner:
        depth += ch == "("
        depth -= ch == ")"
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    parts.append(cur)
    shape = tuple(int(eval(p.strip().replace("/", "//"), {"__builtins__": {}}, dict(dims))) for p in parts)
    dtype = None
    for q in quote:
        m = re.search(r"(?:\b|_)(f64|f32|i32|u32|u8|bf16)\b", q)
        if m:
            dtype = DTYPES[m.group(1)]
            break
    return dtype, shape


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------
CASES = []


def _add(name, entries, inputs, regions, call, **kw):
    CASES.append(ExtentCase(name, (entries,) if isinstance(entries, str) else tuple(entries), inputs, regions, call, **kw))


def by_name(name):
    return next(c for c in CASES if c.name == name)


def _A(name):
    return lambda: sc.by_name(name).build("A")


def _ins(inputs, /, index_like=(), only=None, **kw):
    """the inputs of a case as `in` regions; kw: per-input Region fields (ld, shift)"""
    return [Region(k, v.dtype, tuple(v.shape), role="in", data=v, index_like=k in index_like, **kw.get(k, {})) for k, v in inputs.items()
            if only is None or k in only]


def _in(name, t, index_like=False, **kw):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return Region(name, t.dtype, tuple(t.shape), role="in", data=t.contiguous(), index_like=index_like, **kw)


def _out(name, quote, dtype=None, **dims):
    ld, shift = dims.pop("ld", None), dims.pop("shift", 0)
    q = (quote,) if isinstance(quote, str) else tuple(quote)
    dt, shape = parse_quote(q, dims)
    return Region(name, dtype or dt, shape, ld=ld, shift=shift, quote=q, dims=dims)


def _api():
    from freepose_amd import _lib, ops
    return _lib, ops, _lib.load(), ops.context(), _lib.current_stream()


def _chk(rc, what):
    from freepose_amd import _lib
    _lib.check(rc, what)


BF16_HELPERS = "All tensors bf16 unless said otherwise"


# ---- the three tower drivers -------------------------------------------------------------------------------------------------------------------
def _tower_cases():
    for fused in (1, 0):
        tag = "fused" if fused else "unfused"

        def call(P, x, fused=fused, tag=tag):
            L, ops, lib, ctx, s = _api()
            v = sc._vit(f"vit_28x42_{tag}")
            ops.set_option("ln_fused", fused)
            try:
                _chk(lib.fp_vit_forward(v.handle, P["images"].ptr, 2, 28, 42, 2, 2, P["out"].ptr, s), "fp_vit_forward")
            finally:
                ops.set_option("ln_fused", -1)
        _add(f"vit_28x42_{tag}", "fp_vit_forward", _A(f"vit_28x42_{tag}"),
             lambda x: _ins(x) + [_out("out", ("2 = patch [B,P,dim]", "void* d_out_bf16"), B=2, P=6, dim=384)], call,
             wrapper=(f"vit_28x42_{tag}", {"out": 0}))

    def clip(P, x):
        L, ops, lib, ctx, s = _api()
        v = sc._obj("clip_visual", lambda: ops.ClipVisual(sc.CLIP_NAME, ops.random_clip_state_dict(sc.CLIP_NAME, seed=4)))
        _chk(lib.fp_clip_encode_image(v.handle, P["images"].ptr, 2, 56, P["out"].ptr, s), "fp_clip_encode_image")
    _add("clip_visual", "fp_clip_encode_image", _A("clip_visual"), lambda x: _ins(x) + [_out("out", "d_out bf16 [B, embed_dim]", B=2, embed_dim=64)],
         clip, wrapper=("clip_visual", {"out": 0}))

    def text(P, x):
        L, ops, lib, ctx, s = _api()
        v = sc._obj("clip_text", lambda: ops.ClipText(sc.TEXT_NAME, ops.random_clip_text_state_dict(sc.TEXT_NAME, seed=6)))
        _chk(lib.fp_clip_text_encode(v.handle, P["ids"].ptr, 3, P["out"].ptr, s), "fp_clip_text_encode")
    _add("clip_text", "fp_clip_text_encode", _A("clip_text"),
         lambda x: _ins(x, index_like=("ids",)) + [_out("out", "-> d_out bf16 [B, embed_dim]: token + positional embedding", B=3, embed_dim=64)], text,
         wrapper=("clip_text", {"out": 0}))


_tower_cases()


# ---- FFA -----------------------------------------------------------------------------------------------------------------------------------------
def _ffa_cases():
    def regions(B, shift=0, f32=False):
        def make(x):
            r = _ins(x) + [_out("out", "d_out_bf16 [B,D] (may be NULL)", B=B, D=384, shift=shift)]
            return r + ([_out("out_f32", "d_out_f32 [B,D] (bf16 values widened, may be NULL)", B=B, D=384)] if f32 else [])
        return make

    def call(B, gh, gw, cell, normalize):
        def fn(P, x):
            L, ops, lib, ctx, s = _api()
            _chk(lib.fp_ffa(ctx, P["feats"].ptr, P["masks"].ptr, B, gh, gw, 384, cell, normalize, P["out"].ptr,
                            P["out_f32"].ptr if "out_f32" in P else None, s), "fp_ffa")
        return fn
    _add("ffa_fused_B2", "fp_ffa", _A("ffa_fused_B2"), regions(2), call(2, 1, 35, 1, 1), wrapper=("ffa_fused_B2", {"out": 0}))      # B <= 16: the fused path
    _add("ffa_rows_B17", "fp_ffa", _A("ffa_rows_B17"), regions(17), call(17, 1, 35, 1, 1), wrapper=("ffa_rows_B17", {"out": 0}))    # the row-kernel path
    _add("ffa_cell14", "fp_ffa", _A("ffa_cell14"), regions(2), call(2, 2, 3, 14, 1), wrapper=("ffa_cell14", {"out": 0}))
    _add("ffa_cell14_raw_both_outputs", "fp_ffa", _A("ffa_cell14"), regions(2, f32=True), call(2, 2, 3, 14, 0))                      # not normalised: both outputs
    # the alignment test of the launcher (csrc/capi.hip fp_ffa): a bf16 output one element past a 16-byte boundary takes the row kernel
    _add("ffa_fused_B2_out_misaligned", "fp_ffa", _A("ffa_fused_B2"), regions(2, shift=1), call(2, 1, 35, 1, 1))


_ffa_cases()


# ---- retrieval -------------------------------------------------------------------------------------------------------------------------------------
def _retrieval_cases():
    def prepare(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_bank_prepare(ctx, P["bank"].ptr, 300, 384, P["out"].ptr, s), "fp_bank_prepare")
    _add("bank_prepare", "fp_bank_prepare", _A("bank_prepare"), lambda x: _ins(x) + [_out("out", "d_bank_bf16 out [N,D]", N=300, D=384)], prepare,
         wrapper=("bank_prepare", {"out": 0}))

    for name in ("l2_normalize", "l2_normalize_scalar"):
        def l2(P, x):
            L, ops, lib, ctx, s = _api()
            rows, D = x["x"].shape
            _chk(lib.fp_l2_normalize(ctx, P["x"].ptr, rows, D, P["y"].ptr, s), "fp_l2_normalize")
        _add(name, "fp_l2_normalize", _A(name),
             lambda x: _ins(x) + [_out("y", "d_x_bf16 and d_y_bf16 bf16 [rows,D]", rows=x["x"].shape[0], D=x["x"].shape[1])], l2,
             wrapper=(name, {"y": 0}))

    c = sc.RERANK

    def rerank(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_rerank_views(ctx, P["views"].ptr, P["offsets"].ptr, P["cand"].ptr, P["q"].ptr, c["Q"], c["C"], c["D"], c["k"], P["out"].ptr, s),
             "fp_rerank_views")

    def rerank_regions(shift):
        return lambda x: _ins(x, index_like=("offsets", "cand"), q=dict(shift=shift)) + [_out("out", "d_out f32 [Q,C]", Q=c["Q"], C=c["C"])]
    _add("rerank_views", "fp_rerank_views", _A("rerank_views"), rerank_regions(0), rerank, wrapper=("rerank_views", {"out": 0}))
    # the element-wise query load (csrc/retrieval.hip rerank_views_kernel): every query row one element past a 16-byte boundary
    _add("rerank_views_query_misaligned", "fp_rerank_views", _A("rerank_views"), rerank_regions(1), rerank)

    def tmpl(entry, T):
        def fn(P, x):
            L, ops, lib, ctx, s = _api()
            _chk(getattr(lib, entry)(ctx, P["tmpl"].ptr, P["q"].ptr, P["w"].ptr if "w" in P else None, T, 35, 64, P["out"].ptr, s), entry)
        return fn
    score = lambda T: (lambda x: _ins(x) + [_out("out", "d_scores f32 [T]", T=T)])      # noqa: E731
    _add("template_score", "fp_template_score", _A("template_score"), score(4), tmpl("fp_template_score", 4), wrapper=("template_score", {"out": 0}))
    _add("template_score_normed", "fp_template_score_normed", _A("template_score_normed"), score(4), tmpl("fp_template_score_normed", 4),
         wrapper=("template_score_normed", {"out": 0}))                                   # T = 4 below ceil(4096 / P) = 118 slices: every slice one template

    def normed_T130():
        # T = 130 over TS = 118 slices: slices 0..11 walk two templates, the rest one; T is no multiple of 3 TS, so the rotation of the three
        # register buffers ends inside its first round and the two rows requested ahead lie past the last template
        return dict(tmpl=sc._unit_bf16(sc._seed("A", 3150), (130, 35, 64)), q=sc._unit_bf16(sc._seed("A", 3151), (35, 64)))
    _add("template_score_normed_T130", "fp_template_score_normed", normed_T130, score(130), tmpl("fp_template_score_normed", 130))

    def knn(N, E, Q, k):
        def fn(P, x):
            L, ops, lib, ctx, s = _api()
            _chk(lib.fp_knn_l2(ctx, P["table"].ptr, N, E, P["q"].ptr, Q, k, P["idx"].ptr, P["d2"].ptr, s), "fp_knn_l2")
        return fn
    knn_regions = lambda Q, k: (lambda x: _ins(x) + [_out("idx", "d_out_idx i32 [Q,k]", Q=Q, k=k), _out("d2", "d_out_d2 f32 [Q,k]", Q=Q, k=k)])   # noqa: E731
    _add("knn_l2", "fp_knn_l2", _A("knn_l2"), knn_regions(2, 3), knn(12, 64, 2, 3), wrapper=("knn_l2", {"idx": 0, "d2": 1}))
    # E = 100 is no multiple of the 64 lanes, N = 13 no multiple of the 4 rows of a workgroup, k = N selects every row
    _add("knn_l2_E100_N13_kN", "fp_knn_l2", lambda: dict(table=sc._f32(sc._seed("A", 3160), (13, 100)), q=sc._f32(sc._seed("A", 3161), (2, 100))),
         knn_regions(2, 13), knn(13, 100, 2, 13))


_retrieval_cases()


# ---- pose ------------------------------------------------------------------------------------------------------------------------------------------
GEO_THRESH = 150.0        # degrees: about two thirds of a uniform grid lie within it, so the FREE tail of d_out_idx stays below half of it


def _pose_cases():
    def roi(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_roi_align(ctx, P["images"].ptr, 2, 3, 20, 24, P["rois"].ptr, 3, 7, 7, 2, 1.0, P["out"].ptr, s), "fp_roi_align")
    _add("roi_align", "fp_roi_align", _A("roi_align"),
         lambda x: _ins(x, index_like=("rois",)) + [_out("out", "d_out f32 [n,C,pooled_h,pooled_w]", n=3, C=3, pooled_h=7, pooled_w=7)], roi,
         wrapper=("roi_align", {"out": 0}))

    def geo(P, x):
        L, ops, lib, ctx, s = _api()
        Rp, n = np.ascontiguousarray(sc.GEO_RPREV, np.float64), C.c_int(0)
        _chk(lib.fp_geodesic_select(ctx, P["grid"].ptr, sc.GEO_G, L.ptr(Rp), GEO_THRESH, P["idx"].ptr, C.byref(n), s), "fp_geodesic_select")
        return dict(n=n.value)

    def geo_mask(x, host):
        m = np.full((sc.GEO_G,), FREE, np.uint8)
        m[:host["n"]] = MUST
        return dict(idx=m)
    _add("geodesic_select", "fp_geodesic_select", _A("geodesic_select"),
         lambda x: _ins(x) + [_out("idx", "d_out_idx i32 [G]: the first *h_n entries are written", G=sc.GEO_G)], geo, mask=geo_mask,
         free=dict(idx="the first *h_n entries are written, in ascending order (np.where order); the entries behind them are unspecified"),
         host_example=dict(n=690))

    for name, (Hh, W) in (("depth_extents_vec", (48, 64)), ("depth_extents_scalar", (47, 63))):
        def ext(P, x, Hh=Hh, W=W):
            L, ops, lib, ctx, s = _api()
            _chk(lib.fp_depth_extents(ctx, P["depth"].ptr, 3, Hh, W, 80.0, 81.0, 31.5, 23.5, P["out"].ptr, s), "fp_depth_extents")
        _add(name, "fp_depth_extents", _A(name), lambda x: _ins(x) + [_out("out", "out f64 [Hn,8]", Hn=3)], ext, wrapper=(name, {"out": 0}))


_pose_cases()


# ---- rasteriser ------------------------------------------------------------------------------------------------------------------------------------
def _mesh_V():
    import bench
    return int(bench.synthetic_mesh(2)[0].shape[0])


def _raster_cases():
    c = sc.RASTER
    Hn, W, H = 3, c["W"], c["H"]

    def tiled(mode, fn):
        def call(P, x):
            L, ops, lib, ctx, s = _api()
            ops.set_option("raster_tiled", mode)
            try:
                fn(P, lib, ctx, s, sc._mesh())
            finally:
                ops.set_option("raster_tiled", -1)
        return call
    cam = (float(c["scale"]), float(c["fx"]), float(c["fy"]), float(c["cx"]), float(c["cy"]))
    rgb = lambda: _out("rgb", "rgb u8 [Hn,Hh,W,3]", Hn=Hn, Hh=H, W=W)                    # noqa: E731
    depth = lambda: _out("depth", "depth f32 [Hn,Hh,W]", Hn=Hn, Hh=H, W=W)               # noqa: E731

    def project(P, lib, ctx, s, mesh):
        _chk(lib.fp_project_vertices(ctx, mesh.handle, P["poses"].ptr, Hn, *cam, P["xy"].ptr, P["zc"].ptr, s), "fp_project_vertices")

    def raster(P, lib, ctx, s, mesh):
        _chk(lib.fp_rasterize(ctx, mesh.handle, P["poses"].ptr, Hn, *cam, W, H, P["rgb"].ptr, P["depth"].ptr, s), "fp_rasterize")

    def fused(P, lib, ctx, s, mesh):
        _chk(lib.fp_rasterize_extents(ctx, mesh.handle, P["poses"].ptr, Hn, *cam, W, H, P["rgb"].ptr, P["depth"].ptr if "depth" in P else None,
                                      P["ext"].ptr, P["boxes"].ptr, s), "fp_rasterize_extents")
    ext = lambda: [_out("ext", "d_ext f64 [Hn,8]", Hn=Hn), _out("boxes", "d_boxes i32 [Hn,4]", Hn=Hn)]      # noqa: E731
    _add("project_vertices", "fp_project_vertices", _A("project_vertices_tiled1"),
         lambda x: _ins(x) + [_out("xy", "d_xy i32 [Hn,V,2]", Hn=Hn, V=_mesh_V()), _out("zc", "d_zc f32 [Hn,V]", Hn=Hn, V=_mesh_V())],
         tiled(1, project), wrapper=("project_vertices_tiled1", {"xy": 0, "zc": 1}))
    for mode in (0, 1):
        _add(f"rasterize_tiled{mode}", "fp_rasterize", _A(f"rasterize_tiled{mode}"), lambda x: _ins(x) + [rgb(), depth()], tiled(mode, raster),
             wrapper=(f"rasterize_tiled{mode}", {"rgb": 0, "depth": 1}))
        _add(f"rasterize_extents_tiled{mode}", "fp_rasterize_extents", _A(f"rasterize_extents_tiled{mode}"),
             lambda x: _ins(x) + [rgb(), depth()] + ext(), tiled(mode, fused),
             wrapper=(f"rasterize_extents_tiled{mode}", {"rgb": 0, "depth": 1, "ext": 2, "boxes": 3}))
    _add("rasterize_extents_no_depth", "fp_rasterize_extents", _A("rasterize_extents_tiled1"), lambda x: _ins(x) + [rgb()] + ext(), tiled(1, fused))


_raster_cases()


# ---- depth-map scale -----------------------------------------------------------------------------------------------------------------------------------
def _scale_cases():
    def label(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_label_components(ctx, P["masks"].ptr, 6, 70, 90, 4, P["labels"].ptr, s), "fp_label_components")
    _add("label_components", "fp_label_components", _A("label_components"), lambda x: _ins(x) + [_out("labels", "d_labels i32 [n,H,W]", n=6, H=70, W=90)],
         label, wrapper=("label_components", {"labels": 0}))

    def scale(P, x):
        from tests import _scale_cases as ssc
        L, ops, lib, ctx, s = _api()
        K = ssc.intrinsics(70, 90)
        _chk(lib.fp_depthmap_scale(ctx, P["depth"].ptr, P["masks"].ptr, 6, 70, 90, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), 8.0, 1.5,
                                   25, 1, P["scale"].ptr, P["info"].ptr, P["keep"].ptr if "keep" in P else None, s), "fp_depthmap_scale")

    def regions(keep):
        def make(x):
            r = _ins(x) + [_out("scale", "d_scale f64 [n]", n=6), _out("info", "d_info i32 [n,4]", n=6)]
            return r + ([_out("keep", "d_keep u8 [n,H,W] or NULL", n=6, H=70, W=90)] if keep else [])
        return make
    _add("depthmap_scales", "fp_depthmap_scale", _A("depthmap_scales"), regions(True), scale, wrapper=("depthmap_scales", {"scale": 0, "info": 1, "keep": 2}))
    _add("depthmap_scales_no_keep", "fp_depthmap_scale", _A("depthmap_scales"), regions(False), scale)


_scale_cases()


# ---- refiner and tracker ---------------------------------------------------------------------------------------------------------------------------------
def _refiner_cases():
    def pp(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_patch_points(ctx, P["samples"].ptr, 256, P["T"].ptr, P["K"].ptr, P["cells"].ptr, P["ncells"].ptr, 3, 16, 14.0, P["out"].ptr, s),
             "fp_patch_points")
    pp_regions = lambda x: _ins(x, index_like=("cells", "ncells")) + [_out("out", "d_out i32 [B,C]", B=3, C=16)]      # noqa: E731
    _add("patch_points", "fp_patch_points", _A("patch_points"), pp_regions, pp, wrapper=("patch_points", {"out": 0}))

    def fewer():                                                        # C = 16 above every d_ncells[b]: each item has a tail of -1 slots
        x = sc.by_name("patch_points").build("A")
        x["ncells"] = torch.tensor([9, 12, 7], dtype=torch.int32)
        return x
    _add("patch_points_C_above_ncells", "fp_patch_points", fewer, pp_regions, pp)

    def pnp(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_pnp_epnp(ctx, P["p3"].ptr, P["p2"].ptr, P["vis"].ptr, P["K"].ptr, 3, 65, P["out"].ptr, s), "fp_pnp_epnp")
    _add("pnp_epnp", "fp_pnp_epnp", _A("pnp_epnp"), lambda x: _ins(x) + [_out("out", "d_out f64 [B,16]", B=3)], pnp, wrapper=("pnp_epnp", {"out": 0}))

    def lk_floats():
        from freepose_amd import ops
        from tests import _lk_ref as ref
        return sum(sc.LK_T * h * w for h, w in ops.lk_layout(sc.LK_H, sc.LK_W, ref.PARAMS["levels"], ref.PARAMS["radius"]))

    def pyr_region():
        return _out("pyramid", "d_pyramid f32 [n_floats], the levels back to back", n_floats=lk_floats())

    def pyramid(P, x):
        from tests import _lk_ref as ref
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_lk_pyramid(ctx, P["frames"].ptr, sc.LK_T, sc.LK_H, sc.LK_W, ref.PARAMS["levels"], ref.PARAMS["radius"], P["pyramid"].ptr, s), "fp_lk_pyramid")
    _add("lk_pyramid", "fp_lk_pyramid", _A("lk_pyramid"), lambda x: _ins(x) + [pyr_region()], pyramid, wrapper=("lk_pyramid", {"pyramid": 0}))

    def track(P, x):
        from tests import _lk_ref as ref
        L, ops, lib, ctx, s = _api()
        p, N = ref.PARAMS, x["queries"].shape[0]
        pyramid(P, x)
        _chk(lib.fp_lk_track(ctx, P["pyramid"].ptr, sc.LK_T, sc.LK_H, sc.LK_W, p["levels"], P["queries"].ptr, N, p["radius"], p["iters"], p["fb_thresh"],
                             p["min_eig"], p["max_residual"], P["tracks"].ptr, P["vis"].ptr, P["diag"].ptr, s), "fp_lk_track")

    def track_regions(x):
        N = x["queries"].shape[0]
        return _ins(x) + [pyr_region(), _out("tracks", "d_tracks f32 [T,N,2]", T=sc.LK_T, N=N), _out("vis", "d_vis u8 [T,N]", T=sc.LK_T, N=N),
                          _out("diag", "d_diag f32 [T,N,4]", T=sc.LK_T, N=N)]
    _add("lk_track", ("fp_lk_track", "fp_lk_pyramid"), _A("lk_track"), track_regions, track, wrapper=("lk_track", {"tracks": 0, "vis": 1, "diag": 2}))

    def ends():                                                         # queries on the first and on the last frame only: one chain direction has nothing to do
        x = sc.by_name("lk_track").build("A")
        q = x["queries"][:3].clone()
        q[:, 0] = torch.tensor([0.0, sc.LK_T - 1.0, 0.0])
        x["queries"] = q
        return x
    _add("lk_track_first_and_last_frame", ("fp_lk_track", "fp_lk_pyramid"), ends, track_regions, track)


_refiner_cases()


# ---- evaluation ------------------------------------------------------------------------------------------------------------------------------------------
def _video_tables(M, Nmax, n_frames, n_sym, dts):
    from freepose_amd import ops
    meta, params = np.zeros((M, ops.VIDEO_META_LD), np.int32), np.zeros((M, ops.VIDEO_PARAM_LD), np.float64)
    meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3] = np.arange(M), n_frames, n_sym, ops.VIDEO_HAS_AXIS
    meta[:, 4:4 + len(dts)] = dts
    params[:, :4] = [0.1, 0.11, 640.0, 480.0]
    params[:, 4:7] = [0.0, 0.0, 1.0]
    return meta, params


def _eval_cases():
    for name, projected in (("chamfer", 0), ("chamfer_proj", 1)):
        def call(P, x, projected=projected):
            L, ops, lib, ctx, s = _api()
            n = sc.CHAMFER_SIZES
            _chk(lib.fp_chamfer(ctx, P["pts"].ptr, sum(n), P["table"].ptr, P["xf"].ptr, 2, max(n), 2 * n[1] + sum(n), projected, P["out"].ptr, s), "fp_chamfer")
        _add(name, "fp_chamfer", _A(name), lambda x: _ins(x, index_like=("table",)) + [_out("out", "d_out f64 [B]", B=2)], call,
             wrapper=(name, {"out": 0}))

    def dc(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_depth_compare(ctx, P["est"].ptr, P["gt"].ptr, 2, 10, 12, P["test"].ptr, 2, P["idx"].ptr, P["prm"].ptr, P["taus"].ptr, 3, P["out"].ptr, s),
             "fp_depth_compare")
    _add("depth_compare", "fp_depth_compare", _A("depth_compare"),
         lambda x: _ins(x, index_like=("idx",)) + [_out("out", "d_out i32 [B,4+n_tau]", B=2, n_tau=3)], dc, wrapper=("depth_compare", {"out": 0}))

    def dc_cus(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_depth_compare(ctx, P["est"].ptr, P["gt"].ptr, 2, 10, 12, None, 0, None, None, None, 0, P["out"].ptr, s), "fp_depth_compare")
    _add("depth_compare_no_test", "fp_depth_compare", _A("depth_compare"),
         lambda x: _ins(x, only=("est", "gt")) + [_out("out", "Without d_depth_test: d_out i32 [B,4]", B=2)], dc_cus)

    # ground-truth visibility: 64 x 48 windows at (64, 48) of 192 x 144 canvases, 7 instances, 3 test images
    def vis_inputs():
        x = sc.by_name("gt_visibility").build("A")
        c = sc._gt_edges("A")[0]
        K = np.asarray(c["K"], np.float64)
        prm = np.zeros((len(K), 8))
        prm[:, 0], prm[:, 1], prm[:, 2], prm[:, 3], prm[:, 4] = K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], float(c["delta"])
        x["idx"], x["prm"] = torch.from_numpy(np.asarray(c["img_idx"], np.int32)), torch.from_numpy(prm)
        return x

    def vis(P, x):
        L, ops, lib, ctx, s = _api()
        B, Hr, Wr = x["depth_gt"].shape
        n_img, H, W = x["depth_test"].shape
        ox, oy = sc._gt_edges("A")[0]["window"]
        _chk(lib.fp_gt_visibility(ctx, P["depth_gt"].ptr, B, Hr, Wr, int(ox), int(oy), P["depth_test"].ptr, n_img, H, W, P["idx"].ptr, P["prm"].ptr,
                                  P["mask"].ptr if "mask" in P else None, P["visib"].ptr if "visib" in P else None, P["out"].ptr, s), "fp_gt_visibility")

    def vis_regions(masks, shift=0):
        def make(x):
            B, (n_img, H, W) = x["depth_gt"].shape[0], x["depth_test"].shape
            r = _ins(x, index_like=("idx",), depth_gt=dict(shift=shift)) + [_out("out", "d_out i32 [B,12]", B=B)]
            if "mask" in masks:
                r.append(_out("mask", "d_mask u8 [B,H,W] | NULL", B=B, H=H, W=W))
            if "visib" in masks:
                r.append(_out("visib", "d_mask_visib u8 [B,H,W] | NULL", B=B, H=H, W=W))
            return r
        return make
    _add("gt_visibility", "fp_gt_visibility", vis_inputs, vis_regions(("mask", "visib")), vis, wrapper=("gt_visibility", {"out": 0, "mask": 1, "visib": 2}))
    _add("gt_visibility_no_masks", "fp_gt_visibility", vis_inputs, vis_regions(()), vis)
    _add("gt_visibility_mask_only", "fp_gt_visibility", vis_inputs, vis_regions(("mask",)), vis)
    _add("gt_visibility_visib_only", "fp_gt_visibility", vis_inputs, vis_regions(("visib",)), vis)
    # the alignment test of the launcher (csrc/gt_info.hip fp_gt_visibility_launch): the canvases one float past a 16-byte boundary
    _add("gt_visibility_canvas_misaligned", "fp_gt_visibility", vis_inputs, vis_regions(("mask", "visib"), shift=1), vis)

    # model diameters: 1, 2, 3 and tile + 1 points in one call
    def diam_inputs():
        x = sc.by_name("pts_diameter").build("A")
        sizes = [x[f"c{i}"].shape[0] for i in range(4)]
        starts = np.concatenate([[0], np.cumsum(sizes)])[:-1]
        return dict(pts=torch.cat([x[f"c{i}"] for i in range(4)]), ranges=torch.from_numpy(np.stack([starts, sizes], 1).astype(np.int32)))

    def diam(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_pts_diameter(ctx, P["pts"].ptr, x["pts"].shape[0], P["ranges"].ptr, 4, P["out"].ptr, s), "fp_pts_diameter")
    _add("pts_diameter", "fp_pts_diameter", diam_inputs, lambda x: _ins(x, index_like=("ranges",)) + [_out("out", "d_out f64 [M,8]", M=4)], diam,
         wrapper=("pts_diameter", {"out": 0}))

    # video errors: M = 2 tracks of Nmax = 21 frames, D = 3 offsets
    DTS = (1, 2, 5)

    def video(n_frames, n_sym, extras):
        def call(P, x):
            L, ops, lib, ctx, s = _api()
            meta, params = _video_tables(2, 21, n_frames, n_sym, DTS)
            _chk(lib.fp_video_errors(ctx, P["est"].ptr, P["gt"].ptr, L.ptr(meta), L.ptr(params), 2, 2, 21, 3, P["per"].ptr, P["fin"].ptr,
                                     P["aligned"].ptr if extras else None, P["pairs"].ptr if extras else None, s), "fp_video_errors")

        def regions(x):
            r = _ins(x) + [_out("per", "d_per_offset f64 [M,D,3]", M=2, D=3), _out("fin", "d_final f64 [M,3]", M=2)]
            if extras:
                r += [_out("aligned", "d_aligned f64 [M,Nmax,3]", M=2, Nmax=21), _out("pairs", "d_pairs f64 [M,D,Nmax,3]", M=2, D=3, Nmax=21)]
            return r

        def mask(x, host):
            if not extras:
                return {}
            a, p = np.full((2, 21, 3), NEVER, np.uint8), np.full((2, 3, 21, 3), NEVER, np.uint8)
            for m, N in enumerate(n_frames):
                a[m, :N] = MUST                                         # rows past a track's own length are left as they are
                for d, dt in enumerate(DTS):
                    p[m, d, :N - dt] = MUST                             # rows t1 >= N - dt are left as they are
            return dict(aligned=a, pairs=p)
        return call, regions, mask
    call, regions, mask = video((21, 21), 11, False)
    _add("video_errors", "fp_video_errors", _A("video_errors"), regions, call, mask=mask, wrapper=("video_errors", {"per": 0, "fin": 1}))
    call, regions, mask = video((21, 15), 101, True)                    # a track shorter than Nmax, d_aligned and d_pairs wanted, 101 symmetries
    _add("video_errors_pairs_aligned_short_track", "fp_video_errors", _A("video_errors"), regions, call, mask=mask)

    def bop(P, x):
        L, ops, lib, ctx, s = _api()
        b = sc.BOP
        _chk(lib.fp_bop_scores(ctx, P["err"].ptr, P["groups"].ptr, P["valid"].ptr, P["obj"].ptr, P["scene"].ptr, P["th"].ptr, b["P"], b["Gr"], b["R"], b["T"],
                               b["n_obj"], b["n_scene"], b["n_top"], P["match"].ptr, P["tp_obj"].ptr, P["tp_scene"].ptr, P["tar_obj"].ptr, P["tar_scene"].ptr,
                               s), "fp_bop_scores")

    def bop_regions(x):
        b = sc.BOP
        return _ins(x, index_like=("groups", "valid", "obj", "scene")) + [
            _out("match", "d_match i32 [T,R]", T=b["T"], R=b["R"]), _out("tp_obj", "d_tp_obj i32 [T,n_obj]", T=b["T"], n_obj=b["n_obj"]),
            _out("tp_scene", "d_tp_scene i32 [T,n_scene]", T=b["T"], n_scene=b["n_scene"]), _out("tar_obj", "d_tar_obj i32 [n_obj]", n_obj=b["n_obj"]),
            _out("tar_scene", "d_tar_scene i32 [n_scene]", n_scene=b["n_scene"])]
    _add("bop_scores", "fp_bop_scores", _A("bop_scores"), bop_regions, bop,
         wrapper=("bop_scores", {"match": 0, "tp_obj": 1, "tp_scene": 2, "tar_obj": 3, "tar_scene": 4}))


_eval_cases()


# ---- the gathers on one rank, no communicator ----------------------------------------------------------------------------------------------------------------
def _comm_cases():
    def gather_bytes(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_allgather_bytes(ctx, P["send"].ptr, 1000, P["recv"].ptr, s), "fp_allgather_bytes")
    _add("allgather_bytes", "fp_allgather_bytes", _A("allgather_bytes"),
         lambda x: _ins(x) + [_out("recv", "d_recv [nranks * bytes]", dtype=torch.uint8, nranks=1, bytes=1000)], gather_bytes,
         wrapper=("allgather_bytes", {"recv": 0}))

    def poses(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_allgather_poses(ctx, P["rows"].ptr, 2, 19, P["out"].ptr, s), "fp_allgather_poses")
    _add("allgather_poses", "fp_allgather_poses", _A("allgather_poses"),
         lambda x: _ins(x) + [_out("out", ("d_out [nranks * n_rows, row_len]", "fixed-length f64 result rows"), nranks=1, n_rows=2, row_len=19)], poses,
         wrapper=("allgather_poses", {"out": 0}))

    def topk(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_allgather_topk(ctx, P["s"].ptr, P["i"].ptr, 3, 16, 8, P["os"].ptr, P["oi"].ptr, s), "fp_allgather_topk")
    _add("allgather_topk", "fp_allgather_topk", _A("allgather_topk"),
         lambda x: _ins(x) + [_out("os", ("identical [Q,k_out] on every rank", "d_out_scores f32"), Q=3, k_out=8),
                              _out("oi", ("identical [Q,k_out] on every rank", "d_out_idx i32"), Q=3, k_out=8)], topk,
         wrapper=("allgather_topk", {"os": 0, "oi": 1}))


_comm_cases()


# ---- the GEMM entries that no guard-band test names, with ld > row length wherever the entry takes one --------------------------------------------------------
def _gemm_cases():
    M, N, K = sc.STATS_SHAPES["tiny64"]
    PAD = 8                                                             # leading dimensions are multiples of 8

    def stats(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_gemm_stats(ctx, P["x"].ptr, P["x"].ld, P["w"].ptr, P["w"].ld, P["C"].ptr, P["C"].ld, P["bias"].ptr, P["gamma"].ptr, P["resid"].ptr,
                                  P["resid"].ld, M, N, K, 1e-6, P["stat"].ptr, s), "fp_op_gemm_stats")

    def stats_mask(x, host):
        m = np.full((M, 6), MUST, np.uint8)
        m[:, 5] = NEVER                                                 # "word 5 unused (never written)"
        return dict(stat=m)
    _add("gemm_stats_tiny64", "fp_op_gemm_stats", _A("gemm_stats_tiny64"),
         lambda x: _ins(x, x=dict(ld=K + PAD), w=dict(ld=K + PAD), resid=dict(ld=N + PAD)) + [
             _out("C", ("C[M,N] = epi(", "bf16, ld* in elements"), M=M, N=N, ld=N + PAD), _out("stat", "d_stat u32/f32 [M,6]", M=M)], stats, mask=stats_mask, wrapper=("gemm_stats_tiny64", {"C": 0}))

    M2, N2, K2 = sc.LN_SHAPES["tiny64"]

    def ln_linear(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_ln_linear(ctx, P["x"].ptr, M2, K2, P["g"].ptr, P["b"].ptr, 1e-6, P["w"].ptr, N2, P["bias"].ptr, 0, 0, 0, 64, sc.QSCALE, P["out"].ptr, s),
             "fp_op_ln_linear")
    _add("ln_linear_tiny64", "fp_op_ln_linear", _A("ln_linear_tiny64"), lambda x: _ins(x) + [_out("out", "mode 0: d_out bf16 [M,N]", M=M2, N=N2)], ln_linear,
         wrapper=("ln_linear_tiny64", {"out": 0}))

    def consume(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_row_stats(P["x"].ptr, M2, K2, 1e-6, P["rec"].ptr, P["rstd"].ptr, s), "fp_op_row_stats")
        _chk(lib.fp_op_ln_consume(ctx, P["x"].ptr, M2, K2, P["g"].ptr, P["b"].ptr, P["w"].ptr, N2, P["bias"].ptr, 0, 0, 0, 0, 1.0, P["rec"].ptr, P["rstd"].ptr,
                                  P["out"].ptr, P["out"].ld, s), "fp_op_ln_consume")
    _add("ln_consume_tiny64", ("fp_op_ln_consume", "fp_op_row_stats"), _A("ln_consume_tiny64"),
         lambda x: _ins(x) + [_out("out", "d_out: bf16 [M,N] with ldo elements per row", M=M2, N=N2, ld=N2 + PAD),
                              _out("rec", "d_rec u32 [rows,4]", rows=M2), _out("rstd", "d_rstd f32 [rows]", rows=M2)], consume,
         wrapper=("ln_consume_tiny64", {"out": 0, "rec": 1, "rstd": 2}))


_gemm_cases()


# ---- the ViT helper entries --------------------------------------------------------------------------------------------------------------------------------
def _helper_cases():
    def gelu(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_gelu(P["x"].ptr, P["y"].ptr, 1000, s), "fp_op_gelu")
    _add("gelu_direct", "fp_op_gelu", _A("gelu_direct"), lambda x: _ins(x) + [_out("y", "d_x and d_y bf16 [n]", n=1000)], gelu, wrapper=("gelu_direct", {"y": 0}))

    def im2col(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_im2col_norm(P["images"].ptr, P["A"].ptr, 2, 28, 42, 14, 640, s), "fp_op_im2col_norm")
    _add("im2col_norm", "fp_op_im2col_norm", _A("im2col_norm"),
         lambda x: _ins(x) + [_out("A", ("the patch-embed GEMM's A operand [B*(H/ps)*(W/ps), KP]", "unfold of bf16 crops"), B=2, H=28, W=42, ps=14, KP=640)],
         im2col, wrapper=("im2col_norm", {"A": 0}))

    def token_init(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_token_init(P["x"].ptr, P["cls"].ptr, P["pos0"].ptr, P["reg"].ptr, 4, 2, 40, 48, 64, s), "fp_op_token_init")

    def token_regions(x):
        quote = ("the token buffer d_X [B, npad, D]", BF16_HELPERS)
        dt, shape = parse_quote(quote, dict(B=2, npad=48, D=64))
        return _ins(x, only=("cls", "pos0", "reg")) + [Region("x", dt, shape, role="inout", data=x["x"], quote=quote, dims=dict(B=2, npad=48, D=64))]

    def token_mask(x, host):
        m = np.full((2, 48, 64), NEVER, np.uint8)                      # "Rows 1 + nreg .. n_tok - 1 are not touched"
        m[:, :5] = MUST
        m[:, 40:] = MUST
        return dict(x=m)
    _add("token_init", "fp_op_token_init", _A("token_init"), token_regions, token_init, mask=token_mask, wrapper=("token_init", {"x": 0}))

    def layernorm(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_layernorm(P["x"].ptr, P["y"].ptr, P["gamma"].ptr, P["beta"].ptr, 37, 384, 1e-6, s), "fp_op_layernorm")
    _add("layernorm", "fp_op_layernorm", _A("layernorm"), lambda x: _ins(x) + [_out("y", "d_X and d_Y bf16 [rows,D]", rows=37, D=384)], layernorm,
         wrapper=("layernorm", {"y": 0}))

    def layernorm_rows(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_layernorm_rows(P["x"].ptr, P["y"].ptr, P["gamma"].ptr, P["beta"].ptr, 70, 384, 1e-6, 35, 48, 5, 1, s), "fp_op_layernorm_rows")
    _add("layernorm_rows", "fp_op_layernorm_rows", _A("layernorm_rows"),
         lambda x: _ins(x) + [_out("y", ("d_Y [rows,D]: output row r reads input row", BF16_HELPERS), rows=70, D=384)], layernorm_rows,
         wrapper=("layernorm_rows", {"y": 0}))

    def posembed(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_posembed_aa(P["grid"].ptr, P["dst"].ptr, 37, 20, 30, 64, s), "fp_op_posembed_aa")
    _add("posembed_aa", "fp_op_posembed_aa", _A("posembed_aa"), lambda x: _ins(x) + [_out("dst", ("d_dst [gh*gw, D]", BF16_HELPERS), gh=20, gw=30, D=64)],
         posembed, wrapper=("posembed_aa", {"dst": 0}))

    def row_stats(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_row_stats(P["x"].ptr, 37, 384, 1e-6, P["rec"].ptr, P["rstd"].ptr, s), "fp_op_row_stats")
    recs = lambda: [_out("rec", "d_rec u32 [rows,4]", rows=37), _out("rstd", "d_rstd f32 [rows]", rows=37)]      # noqa: E731
    _add("row_stats", "fp_op_row_stats", _A("row_stats"), lambda x: _ins(x) + recs(), row_stats, wrapper=("row_stats", {"rec": 0, "rstd": 1}))

    def finalize(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_stats_finalize(P["part"].ptr, 37, 384, 1e-6, 40, P["rec"].ptr, P["rstd"].ptr, s), "fp_op_stats_finalize")
    _add("stats_finalize", "fp_op_stats_finalize", _A("stats_finalize"), lambda x: _ins(x) + recs(), finalize, wrapper=("stats_finalize", {"rec": 0, "rstd": 1}))

    def fold(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_ln_fold(P["w"].ptr, P["gamma"].ptr, P["beta"].ptr, P["bias"].ptr, 130, 128, 64, sc.QSCALE, P["wf"].ptr, P["cb"].ptr, s), "fp_op_ln_fold")
    _add("ln_fold", "fp_op_ln_fold", _A("ln_fold"),
         lambda x: _ins(x) + [_out("wf", ("d_Wf [N,K] = bf16(", BF16_HELPERS), N=130, K=128), _out("cb", "d_cb u32 [N,4]", N=130)], fold,
         wrapper=("ln_fold", {"wf": 0, "cb": 1}))

    def transpose(P, x):
        L, ops, lib, ctx, s = _api()
        _chk(lib.fp_op_transpose(P["x"].ptr, P["dst"].ptr, 37, 72, s), "fp_op_transpose")
    _add("transpose", "fp_op_transpose", _A("transpose"), lambda x: _ins(x) + [_out("dst", ("d_dst [cols, rows]", BF16_HELPERS), rows=37, cols=72)], transpose,
         wrapper=("transpose", {"dst": 0}))


_helper_cases()

# the three launchers that choose a kernel by pointer alignment: the case whose extent starts one element past a 16-byte boundary
MISALIGNED = {"fp_gt_visibility": "gt_visibility_canvas_misaligned", "fp_ffa": "ffa_fused_B2_out_misaligned", "fp_rerank_views": "rerank_views_query_misaligned"}
