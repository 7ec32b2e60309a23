"""Tensor-level wrappers over the C ABI: torch provides device memory and the stream, libfreepose_hip.so does
the work.  Every function raises if the library is missing or a call fails (no CPU fallback)."""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, ptr

_ctx = {}


def context(device: Optional[int] = None):
    """One fp_ctx per (process, device)."""
    if device is None:
        device = torch.cuda.current_device()
    h = _ctx.get(device)
    if h is None:
        lib = _lib.load()
        out = C.c_void_p()
        check(lib.fp_ctx_create(int(device), C.byref(out)), "fp_ctx_create")
        h = _ctx[device] = out
    return h


CTX_OPTIONS = ("ln_fused", "raster_tiled", "gemm_row_split")
BANK_QUERIES_PER_PASS = 4      # bank_scan_kernel: up to 4 queries share one pass over the bank (retrieval.hip fp_bank_scan)


def set_option(name: str, value: int, device: Optional[int] = None):
    """Run-time option of this process's context on `device` (fp_ctx_set_option): 'ln_fused', 'raster_tiled', 'gemm_row_split';
    value < 0 restores the default.  Any other name is a measurement toggle of the LAB build ('gemm_variant', 'gemm_dbg',
    'attn_slots', 'attn_variant', 'topk_select': tools/ call _lib.use_lab() first) and raises on the product library."""
    lib = _lib.load()
    if name in CTX_OPTIONS:
        check(lib.fp_ctx_set_option(context(device), name.encode(), int(value)), "fp_ctx_set_option")
    elif hasattr(lib, "fp_lab_set_option"):
        check(lib.fp_lab_set_option(name.encode(), int(value)), "fp_lab_set_option")
    else:
        raise RuntimeError(f"option '{name}' exists only in the lab build (python -m freepose_amd.build --lab; _lib.use_lab())")


def _dev(t: torch.Tensor, dtype=None) -> torch.Tensor:
    if not t.is_cuda:
        t = t.to("cuda", non_blocking=False)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


# ------------------------------------------------------------------------------------------------
VIT_ARCHS = {
    # name: (dim, depth, heads, n_reg).  Only the *_reg hub models: they interpolate the position embedding with
    # antialias=True, offset 0 (what fp_vit_forward implements); the non-reg hub entries use antialias=False and
    # interpolate_offset=0.1 and are not used by the reference (dino.py:8, tracking_refiner.py:23).
    "dinov2_vits14_reg": (384, 12, 6, 4), "dinov2_vitb14_reg": (768, 12, 12, 4), "dinov2_vitl14_reg": (1024, 24, 16, 4),
}
# "patch_normalized": patch features with every row F.normalize()d by the final-norm kernel itself (== l2_normalize(patch features), bit
# for bit) — what the estimators score hypotheses with (pose_estimator.py:85-88): no separate normalisation pass over 1.6 GB
FEATURE_TYPES = {"cls": 0, "reg": 1, "patch": 2, "patch_normalized": 3}


class ViT:
    """Device-resident DINOv2 ViT (hub state-dict layout) driving fp_vit_forward."""

    def __init__(self, model_name: str = "dinov2_vitl14_reg", state_dict: Optional[dict] = None, seed: int = 0,
                 device: Optional[int] = None):
        if model_name not in VIT_ARCHS:
            raise ValueError(f"unknown DINOv2 model {model_name}")
        dim, depth, heads, n_reg = VIT_ARCHS[model_name]
        self.dim, self.depth, self.heads, self.n_reg, self.patch, self.pos_grid = dim, depth, heads, n_reg, 14, 37
        self.lib = _lib.load()
        self.ctx = context(device)
        arch = _lib.VitArch(dim, depth, heads, 4 * dim, 14, n_reg, 37, 1e-6)
        h = C.c_void_p()
        check(self.lib.fp_vit_create(self.ctx, C.byref(arch), C.byref(h)), "fp_vit_create")
        self.handle = h
        self.weights = {}
        if state_dict is None:
            state_dict = random_state_dict(model_name, seed)
        self.load_state_dict(state_dict)

    def load_state_dict(self, sd: dict):
        s = current_stream()
        for name, t in sd.items():
            if name == "mask_token":
                continue
            w = _dev(torch.as_tensor(t), torch.bfloat16)
            self.weights[name] = w  # keep alive: the library stores raw pointers
            check(self.lib.fp_vit_set_weight(self.handle, name.encode(), ptr(w), w.numel(), s), f"set_weight({name})")
        torch.cuda.synchronize()

    def forward(self, images: torch.Tensor, layer: int = 22, feature_type: str = "cls",
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """`out`: optional preallocated contiguous bf16 tensor of the result shape (e.g. a slice along dim 0 of a larger
        buffer, so chunked calls need no concatenation)"""
        x = _dev(images, torch.bfloat16)
        B, Cc, H, W = x.shape
        assert Cc == 3
        P = (H // self.patch) * (W // self.patch)
        ft = FEATURE_TYPES[feature_type]
        shape = {0: (B, self.dim), 1: (B, self.n_reg, self.dim), 2: (B, P, self.dim), 3: (B, P, self.dim)}[ft]
        if out is None:
            out = torch.empty(shape, dtype=torch.bfloat16, device=x.device)
        else:
            assert tuple(out.shape) == shape and out.dtype == torch.bfloat16 and out.is_contiguous() and out.device == x.device
        if B > 0:
            check(self.lib.fp_vit_forward(self.handle, ptr(x), B, H, W, int(layer), ft, ptr(out), current_stream()),
                  "fp_vit_forward")
        return out

    __call__ = forward

    def flops(self, B, H, W, layer=22) -> float:
        return float(self.lib.fp_vit_flops(self.handle, B, H, W, layer))

    def profile(self, enable: bool):
        check(self.lib.fp_vit_profile(self.handle, int(enable)))

    def profile_read(self):
        g, a, o, f = C.c_float(), C.c_float(), C.c_float(), C.c_double()
        check(self.lib.fp_vit_profile_read(self.handle, C.byref(g), C.byref(a), C.byref(o), C.byref(f)))
        return {"ms_gemm": g.value, "ms_attn": a.value, "ms_other": o.value, "gemm_flops": f.value,
                "gemm_launches": int(self.lib.fp_vit_profile_gemm_launches(self.handle))}

    def __del__(self):
        try:
            self.lib.fp_vit_destroy(self.handle)
        except Exception:
            pass


def random_state_dict(model_name: str, seed: int = 0) -> dict:
    """Seeded random-init weights with the hub DINOv2 state-dict names/shapes (no checkpoints offline).
    trunc-normal(0.02) linears, LayerScale gamma 1.0, LayerNorm (1, 0) — SURVEY.md §8d C2."""
    dim, depth, heads, n_reg = VIT_ARCHS[model_name]
    g = torch.Generator().manual_seed(seed)

    def tn(*shape, std=0.02):
        return torch.nn.init.trunc_normal_(torch.empty(*shape), std=std, a=-2 * std, b=2 * std, generator=g)

    sd = {"cls_token": tn(1, 1, dim, std=1e-6) + 0.0, "pos_embed": tn(1, 1 + 37 * 37, dim),
          "patch_embed.proj.weight": tn(dim, 3, 14, 14), "patch_embed.proj.bias": tn(dim),
          "norm.weight": torch.ones(dim), "norm.bias": torch.zeros(dim)}
    sd["cls_token"] = tn(1, 1, dim)
    if n_reg:
        sd["register_tokens"] = tn(1, n_reg, dim)
    for i in range(depth):
        p = f"blocks.{i}."
        sd[p + "norm1.weight"] = torch.ones(dim) + tn(dim, std=0.05)
        sd[p + "norm1.bias"] = tn(dim)
        sd[p + "attn.qkv.weight"] = tn(3 * dim, dim)
        sd[p + "attn.qkv.bias"] = tn(3 * dim)
        sd[p + "attn.proj.weight"] = tn(dim, dim)
        sd[p + "attn.proj.bias"] = tn(dim)
        sd[p + "ls1.gamma"] = torch.ones(dim)
        sd[p + "norm2.weight"] = torch.ones(dim) + tn(dim, std=0.05)
        sd[p + "norm2.bias"] = tn(dim)
        sd[p + "mlp.fc1.weight"] = tn(4 * dim, dim)
        sd[p + "mlp.fc1.bias"] = tn(4 * dim)
        sd[p + "mlp.fc2.weight"] = tn(dim, 4 * dim)
        sd[p + "mlp.fc2.bias"] = tn(dim)
        sd[p + "ls2.gamma"] = torch.ones(dim)
    return {k: v.to(torch.bfloat16) for k, v in sd.items()}


# ------------------------------------------------------------------------------------------------
def ffa(feats: torch.Tensor, masks: torch.Tensor, cell: int = 14, normalize: bool = False, out_f32: bool = False):
    """FFA descriptor.  feats bf16 [B,P,D]; masks bool/u8 [B,gh*cell,gw*cell] (or [B,P] with cell=1)."""
    lib = _lib.load()
    f = _dev(feats, torch.bfloat16)
    B, Pn, D = f.shape
    m = _dev(masks)
    m = (m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)).contiguous()   # (a bool tensor IS 0 / 1 bytes: no copy kernel)
    if cell == 1:
        gh, gw = 1, Pn
        m = m.reshape(B, 1, Pn)
    else:
        gh, gw = m.shape[1] // cell, m.shape[2] // cell
        if m.shape[1] != gh * cell or m.shape[2] != gw * cell:
            m = m[:, :gh * cell, :gw * cell].contiguous()
    assert gh * gw == Pn, f"mask grid {gh}x{gw} != {Pn} patches"
    ob = torch.empty((B, D), dtype=torch.bfloat16, device=f.device)
    of = torch.empty((B, D), dtype=torch.float32, device=f.device) if out_f32 else None
    if B:
        check(lib.fp_ffa(context(), ptr(f), ptr(m), B, gh, gw, D, cell, int(normalize), ptr(ob), ptr(of), current_stream()),
              "fp_ffa")
    return of if out_f32 else ob


def l2_normalize(x: torch.Tensor, inplace: bool = False) -> torch.Tensor:
    """F.normalize(x, dim=-1) with the reference's bf16 rounding points; `inplace` overwrites a contiguous bf16 device tensor"""
    lib = _lib.load()
    xb = _dev(x, torch.bfloat16)
    D = xb.shape[-1]
    rows = xb.numel() // D
    y = xb if inplace else torch.empty_like(xb)
    if rows:
        check(lib.fp_l2_normalize(context(), ptr(xb), rows, D, ptr(y), current_stream()), "fp_l2_normalize")
    return y


def bank_prepare(bank_f32: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    b = _dev(bank_f32, torch.float32)
    N, D = b.shape
    out = torch.empty((N, D), dtype=torch.bfloat16, device=b.device)
    check(lib.fp_bank_prepare(context(), ptr(b), N, D, ptr(out), current_stream()), "fp_bank_prepare")
    return out


def bank_topk(bank_bf16: torch.Tensor, queries: torch.Tensor, k: int = 100, idx_offset: int = 0):
    """(scores f32 [Q,k], idx i32 [Q,k]) ordered by (score desc, index asc)."""
    lib = _lib.load()
    b = _dev(bank_bf16, torch.bfloat16)
    q = _dev(queries, torch.bfloat16)
    if q.dim() == 1:
        q = q[None]
    N, D = b.shape
    Q = q.shape[0]
    s = torch.empty((Q, k), dtype=torch.float32, device=b.device)
    i = torch.empty((Q, k), dtype=torch.int32, device=b.device)
    if Q:
        check(lib.fp_bank_topk(context(), ptr(b), N, D, ptr(q), Q, k, idx_offset, ptr(s), ptr(i), current_stream()),
              "fp_bank_topk")
    return s, i


def topk_merge(cand_scores: torch.Tensor, cand_idx: torch.Tensor, k: int):
    lib = _lib.load()
    cs = _dev(cand_scores, torch.float32)
    ci = _dev(cand_idx, torch.int32)
    Q, Cn = cs.shape
    s = torch.empty((Q, k), dtype=torch.float32, device=cs.device)
    i = torch.empty((Q, k), dtype=torch.int32, device=cs.device)
    if Q:
        check(lib.fp_topk_merge(context(), ptr(cs), ptr(ci), Q, Cn, k, ptr(s), ptr(i), current_stream()), "fp_topk_merge")
    return s, i


def rerank_views(views_bf16: torch.Tensor, offsets: torch.Tensor, cand_idx: torch.Tensor, queries: torch.Tensor, k: int) -> torch.Tensor:
    """per-view fine re-rank scores f32 [Q,C] (numpy-mean of the top-k per-view scores of each candidate mesh)"""
    lib = _lib.load()
    v = _dev(views_bf16, torch.bfloat16)
    off = _dev(offsets).to(torch.int32).contiguous()
    cd = _dev(cand_idx).to(torch.int32).contiguous()
    q = _dev(queries, torch.bfloat16).reshape(cd.shape[0], v.shape[1])
    out = torch.empty(cd.shape, dtype=torch.float32, device=v.device)
    if cd.numel():
        check(lib.fp_rerank_views(context(), ptr(v), ptr(off), ptr(cd), ptr(q), cd.shape[0], cd.shape[1], v.shape[1], int(k),
                                  ptr(out), current_stream()), "fp_rerank_views")
    return out


def template_score(tmpl: torch.Tensor, query: torch.Tensor, weights: Optional[torch.Tensor] = None,
                   normalized: bool = False) -> torch.Tensor:
    """tmpl bf16 [T,P,D] raw — or, with normalized=True, already l2_normalize()d rows (the pre-normalised feature store; same
    bits out, one streaming pass) —, query bf16 [P,D] used as given -> scores f32 [T] (bf16-valued unless weighted)."""
    lib = _lib.load()
    t = _dev(tmpl, torch.bfloat16)
    q = _dev(query, torch.bfloat16).reshape(-1, t.shape[-1])
    T, Pn, D = t.shape
    assert q.shape[0] == Pn
    w = _dev(weights, torch.float32) if weights is not None else None
    out = torch.empty((T,), dtype=torch.float32, device=t.device)
    if T:
        fn = lib.fp_template_score_normed if normalized else lib.fp_template_score
        check(fn(context(), ptr(t), ptr(q), ptr(w), T, Pn, D, ptr(out), current_stream()), "fp_template_score")
    return out


def crop_resize_pad(images: torch.Tensor, boxes: torch.Tensor, target: int, bbox_extend: float = 0.0,
                    masks: Optional[torch.Tensor] = None, mask_mode: int = 0, out_bf16: bool = False,
                    u8_float_div: bool = False) -> torch.Tensor:
    """images f32 [n_img,C,H,W] or u8 [n_img,H,W,C]; boxes int [n,4] xyxy.  u8 pixels become
    float(double(x)/255) (renderer.py:121) or, with u8_float_div, float(x)/255.f (utils.py:20)."""
    lib = _lib.load()
    if images.dtype == torch.uint8:
        img = _dev(images)
        n_img, H, W, Cc = img.shape
        src = 2 if u8_float_div else 1
    else:
        img = _dev(images, torch.float32)
        n_img, Cc, H, W = img.shape
        src = 0
    bx = _dev(boxes).to(torch.int32).contiguous()
    n = bx.shape[0]
    m = _dev(masks).to(torch.uint8).contiguous() if masks is not None else None
    if mask_mode == 2:
        Cc_out = 1
    else:
        Cc_out = Cc
    out = torch.empty((n, Cc_out, target, target), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=img.device)
    if n:
        check(lib.fp_crop_resize_pad(context(), ptr(img), src, n_img, Cc_out if mask_mode == 2 else Cc, H, W, ptr(bx), n,
                                     float(bbox_extend), int(target), ptr(m), int(mask_mode), ptr(out), int(out_bf16),
                                     current_stream()), "fp_crop_resize_pad")
    return out


def roi_align(images: torch.Tensor, rois: torch.Tensor, output_size, sampling_ratio: int = 2,
              spatial_scale: float = 1.0) -> torch.Tensor:
    """torchvision.ops.roi_align(images, rois, output_size, spatial_scale, sampling_ratio, aligned=False):
    images f32 [N,C,H,W], rois f32 [n,5] (image index, x1, y1, x2, y2) -> f32 [n,C,ph,pw]"""
    lib = _lib.load()
    img = _dev(images, torch.float32)
    r = _dev(rois, torch.float32).reshape(-1, 5).contiguous()
    ph, pw = (output_size, output_size) if isinstance(output_size, int) else output_size
    N, Cc, H, W = img.shape
    n = r.shape[0]
    out = torch.empty((n, Cc, ph, pw), dtype=torch.float32, device=img.device)
    if n:
        check(lib.fp_roi_align(context(), ptr(img), N, Cc, H, W, ptr(r), n, int(ph), int(pw), int(sampling_ratio),
                               float(spatial_scale), ptr(out), current_stream()), "fp_roi_align")
    return out


def generate_rotations(n: int) -> np.ndarray:
    lib = _lib.load()
    out = np.empty((n, 3, 3), dtype=np.float64)
    check(lib.fp_generate_rotations(n, ptr(out)), "fp_generate_rotations")
    return out


def geodesic_select(grid_f64: torch.Tensor, R_prev: np.ndarray, thresh_deg: float) -> np.ndarray:
    lib = _lib.load()
    g = _dev(grid_f64, torch.float64)
    G = g.shape[0]
    idx = torch.empty((G,), dtype=torch.int32, device=g.device)
    Rp = np.ascontiguousarray(np.asarray(R_prev, dtype=np.float64)[:3, :3])
    n = C.c_int(0)
    check(lib.fp_geodesic_select(context(), ptr(g), G, ptr(Rp), float(thresh_deg), ptr(idx), C.byref(n), current_stream()),
          "fp_geodesic_select")
    return idx[: n.value].cpu().numpy().astype(np.int64)


class Mesh:
    """device copy of a triangle mesh.  `colors` u8 [V,3] selects vertex colours; `uv` f32 [F,3,2] + `texture` u8 [th,tw,3]
    (+ optional diffuse factor `kd` [3]) select per-fragment texture sampling; neither = white."""

    def __init__(self, vertices: np.ndarray, faces: np.ndarray, colors: Optional[np.ndarray] = None, uv: Optional[np.ndarray] = None,
                 texture: Optional[np.ndarray] = None, kd=None):
        self.lib = _lib.load()
        v = np.ascontiguousarray(vertices, dtype=np.float32)
        f = np.ascontiguousarray(faces, dtype=np.int32)
        h = C.c_void_p()
        if uv is not None and texture is not None:
            t = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 3, 2)
            if t.shape[0] != f.shape[0]:
                raise ValueError(f"uv must be per-corner [F,3,2]; got {t.shape} for {f.shape[0]} faces")
            x = np.ascontiguousarray(np.asarray(texture)[:, :, :3], dtype=np.uint8)
            k = None if kd is None else np.ascontiguousarray(kd, dtype=np.float32).reshape(3)
            check(self.lib.fp_mesh_upload_textured(context(), ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(t), ptr(x), x.shape[0],
                                                   x.shape[1], ptr(k), C.byref(h)), "fp_mesh_upload_textured")
        else:
            c = np.ascontiguousarray(colors[:, :3], dtype=np.uint8) if colors is not None else None
            check(self.lib.fp_mesh_upload(context(), ptr(v), v.shape[0], ptr(f), f.shape[0], ptr(c), C.byref(h)), "fp_mesh_upload")
        self.handle, self.V, self.F = h, v.shape[0], f.shape[0]

    def set_filter(self, mode: int):
        """texture minification: 1 = trilinear mip-maps (default), 0 = bilinear level 0 (csrc/raster.hip header)"""
        check(self.lib.fp_mesh_set_filter(self.handle, int(mode)), "fp_mesh_set_filter")
        return self

    def set_cull(self, mode: int):
        """back-face culling: 0 = both sides (default; the reference's callers), 1 = pyrender's default culling (cull_faces=True)"""
        check(self.lib.fp_mesh_set_cull(self.handle, int(mode)), "fp_mesh_set_cull")
        self.cull = int(mode)
        return self

    def set_shading(self, mode: int):
        """1 = gamma output rule (default), 0 = linear (csrc/raster.hip header)"""
        check(self.lib.fp_mesh_set_shading(self.handle, int(mode)), "fp_mesh_set_shading")
        return self

    def set_ambient(self, ambient: float):
        """scene ambient light factor (2 = MeshRenderer's scenes, 5 = TrackingRefiner's)"""
        check(self.lib.fp_mesh_set_ambient(self.handle, float(ambient)), "fp_mesh_set_ambient")
        return self

    def __del__(self):
        try:
            self.lib.fp_mesh_destroy(self.handle)
        except Exception:
            pass


def _raster_out(out, n, shapes, dtypes, device):
    """the output tensors of a rasteriser call: fresh ones, or the caller's (`out`: contiguous device tensors of these shapes and types;
    None entries are passed on as "not wanted")"""
    if out is None:
        return [torch.empty(s, dtype=d, device=device) for s, d in zip(shapes, dtypes)]
    assert len(out) == n
    for t, s, d in zip(out, shapes, dtypes):
        assert t is None or (t.is_cuda and t.is_contiguous() and tuple(t.shape) == tuple(s) and t.dtype == d), (s, d)
    return list(out)


def rasterize(mesh: Mesh, poses: torch.Tensor, scale: float, fx: float, fy: float, cx: float, cy: float, W: int, H: int, out=None):
    """poses [Hn,4,4] object->camera (OpenCV).  Returns (rgb u8 [Hn,H,W,3], depth f32 [Hn,H,W]) on device; `out` = (rgb, depth) to
    write into (every element is written)."""
    lib = _lib.load()
    p = _dev(torch.as_tensor(poses), torch.float32)
    Hn = p.shape[0]
    rgb, depth = _raster_out(out, 2, [(Hn, H, W, 3), (Hn, H, W)], [torch.uint8, torch.float32], p.device)
    if Hn:
        check(lib.fp_rasterize(context(), mesh.handle, ptr(p), Hn, float(scale), float(fx), float(fy), float(cx), float(cy),
                               int(W), int(H), ptr(rgb), ptr(depth), current_stream()), "fp_rasterize")
    return rgb, depth


def rasterize_extents(mesh: Mesh, poses: torch.Tensor, scale: float, fx: float, fy: float, cx: float, cy: float, W: int, H: int,
                      want_depth: bool = False, out=None):
    """rasterize() with the depth image's consumers fused into the tile epilogue: returns (rgb u8 [Hn,H,W,3], depth f32 [Hn,H,W] or
    None, ext f64 [Hn,8] == depth_extents(depth), boxes i32 [Hn,4] == ext[:, :4]).  Without `want_depth` the depth image is never
    written (the pose hot path needs only the extents).  `out` = (rgb, depth | None, ext, boxes) to write into."""
    lib = _lib.load()
    p = _dev(torch.as_tensor(poses), torch.float32)
    Hn = p.shape[0]
    if out is None:
        out = (torch.empty((Hn, H, W, 3), dtype=torch.uint8, device=p.device),
               torch.empty((Hn, H, W), dtype=torch.float32, device=p.device) if want_depth else None,
               torch.empty((Hn, 8), dtype=torch.float64, device=p.device), torch.empty((Hn, 4), dtype=torch.int32, device=p.device))
    assert (out[1] is not None) == bool(want_depth)
    rgb, depth, ext, boxes = _raster_out(out, 4, [(Hn, H, W, 3), (Hn, H, W), (Hn, 8), (Hn, 4)],
                                         [torch.uint8, torch.float32, torch.float64, torch.int32], p.device)
    if Hn:
        check(lib.fp_rasterize_extents(context(), mesh.handle, ptr(p), Hn, float(scale), float(fx), float(fy), float(cx), float(cy),
                                       int(W), int(H), ptr(rgb), ptr(depth), ptr(ext), ptr(boxes), current_stream()), "fp_rasterize_extents")
    return rgb, depth, ext, boxes


def project_vertices(mesh: Mesh, poses: torch.Tensor, scale: float, fx: float, fy: float, cx: float, cy: float):
    """vertex stage of the rasteriser: (xy i32 [Hn,V,2] window coordinates in 1/256 px, zc f32 [Hn,V]) on device"""
    lib = _lib.load()
    p = _dev(torch.as_tensor(poses), torch.float32)
    Hn = p.shape[0]
    xy = torch.zeros((Hn, mesh.V, 2), dtype=torch.int32, device=p.device)
    zc = torch.zeros((Hn, mesh.V), dtype=torch.float32, device=p.device)
    if Hn:
        check(lib.fp_project_vertices(context(), mesh.handle, ptr(p), Hn, float(scale), float(fx), float(fy), float(cx), float(cy),
                                      ptr(xy), ptr(zc), current_stream()), "fp_project_vertices")
    return xy, zc


def depth_extents(depth: torch.Tensor, fx: float, fy: float, cx: float, cy: float) -> torch.Tensor:
    """[Hn,8] = xmin,ymin,xmax,ymax (mask bbox incl. <100 px fallback), dx, dy (m), count, 0"""
    lib = _lib.load()
    d = _dev(depth, torch.float32)
    Hn, H, W = d.shape
    out = torch.empty((Hn, 8), dtype=torch.float64, device=d.device)
    if Hn:
        check(lib.fp_depth_extents(context(), ptr(d), Hn, H, W, float(fx), float(fy), float(cx), float(cy), ptr(out),
                                   current_stream()), "fp_depth_extents")
    return out


# ---- depth-map object scale (csrc/scale.hip) --------------------------------------------------------
def label_components(masks: torch.Tensor, connectivity: int = 4) -> torch.Tensor:
    """connected components of binary masks [n,H,W] (or [H,W]) -> int32 labels of the same shape: 0 = background, else 1 + raster
    index of the component's first pixel; ranked, that is scipy.ndimage.label's numbering (src/pipeline/utils.py:71-84)"""
    lib = _lib.load()
    m = _dev(masks)
    single = m.dim() == 2
    m = _dev((m[None] if single else m) != 0, torch.uint8)
    if m.dim() != 3:
        raise ValueError(f"label_components: masks of shape {tuple(masks.shape)} ([n,H,W] or [H,W])")
    n, H, W = m.shape
    out = torch.empty((n, H, W), dtype=torch.int32, device=m.device)
    check(lib.fp_label_components(context(), ptr(m), n, H, W, int(connectivity), ptr(out), current_stream()), "fp_label_components")
    return out[0] if single else out


def depthmap_scales(depth, masks, K, erosion_radius: float = 8, std_factor: float = 1.5, min_vertices: int = 25, align: bool = True,
                    return_keep: bool = False):
    """object scale under each of the n proposal masks [n,H,W] of one image from its float64 depth map [H,W] and intrinsics K [3,3]
    (reference scale_estimators.py:117-187, one call instead of a host loop) -> (scales f64 [n], info i32 [n,4] = component area,
    index of the erosion radius used (5 = un-eroded for radius 8), survivor count, points kept) and, with return_keep, the u8 mask
    [n,H,W] of the pixels whose points entered the extent.  Raises ValueError on an empty mask, like the host function."""
    lib = _lib.load()
    d = _dev(torch.as_tensor(depth), torch.float64)
    m = _dev(torch.as_tensor(masks))
    m = _dev(m != 0, torch.uint8)
    if d.dim() != 2 or m.dim() != 3 or tuple(m.shape[1:]) != tuple(d.shape):
        raise ValueError(f"depthmap_scales: depth {tuple(d.shape)} and masks {tuple(m.shape)} ([H,W] and [n,H,W])")
    Kn = np.asarray(K.detach().cpu() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    n, H, W = m.shape
    scales = torch.empty((n,), dtype=torch.float64, device=d.device)
    info = torch.zeros((n, 4), dtype=torch.int32, device=d.device)
    keep = torch.empty((n, H, W), dtype=torch.uint8, device=d.device) if return_keep else None
    check(lib.fp_depthmap_scale(context(), ptr(d), ptr(m), n, H, W, float(Kn[0, 0]), float(Kn[1, 1]), float(Kn[0, 2]), float(Kn[1, 2]),
                                float(erosion_radius), float(std_factor), int(min_vertices), int(bool(align)), ptr(scales), ptr(info),
                                ptr(keep), current_stream()), "fp_depthmap_scale")
    empty = (info[:, 0] == 0).nonzero().flatten().tolist()
    if empty:
        raise ValueError(f"depthmap scale: empty proposal mask (mask {empty[0]} of {n})")
    return (scales, info, keep) if return_keep else (scales, info)


# ---- TrackingRefiner correspondences and pose from tracks (csrc/refine.hip) ------------------------------
PNP_MIN_POINTS, PNP_MAX_POINTS = 4, 4096                   # csrc/pnp_core.h FP_PNP_MIN_N / FP_PNP_MAX_N
PNP_OK, PNP_FEW, PNP_SINGULAR = 0, 1, 2


def patch_points(samples, transforms, Ks, cells, ncells=None, patch: float = 14.0) -> torch.Tensor:
    """TrackingRefiner._compute_3d_points (reference tracking_refiner.py:102-130) for B items in one call: samples f64 [S,3] (object frame,
    shared), transforms f64 [B,4,4] object -> camera, Ks f64 [B,3,3] (or one [3,3] for all), cells i32 [B,C,2] (x, y) patch cells,
    ncells i32 [B] real slots per item (default: all C) -> i32 [B,C] on the device: index of the sample chosen for each cell, -1 for a
    cell no sample projects into and for slots >= ncells[b]."""
    lib = _lib.load()
    s = _dev(torch.as_tensor(samples), torch.float64)
    T = _dev(torch.as_tensor(transforms), torch.float64)
    K = _dev(torch.as_tensor(Ks), torch.float64)
    c = _dev(torch.as_tensor(cells), torch.int32)
    if s.dim() != 2 or s.shape[1] != 3 or s.shape[0] < 1:
        raise ValueError(f"patch_points: samples {tuple(s.shape)} ([S,3], S >= 1)")
    if T.dim() != 3 or tuple(T.shape[1:]) != (4, 4):
        raise ValueError(f"patch_points: transforms {tuple(T.shape)} ([B,4,4])")
    B = T.shape[0]
    if K.dim() == 2:
        K = K.unsqueeze(0).expand(B, 3, 3).contiguous()
    if tuple(K.shape) != (B, 3, 3) or c.dim() != 3 or c.shape[0] != B or c.shape[2] != 2:
        raise ValueError(f"patch_points: Ks {tuple(K.shape)} / cells {tuple(c.shape)} for B = {B} ([B,3,3] and [B,C,2])")
    Cn = c.shape[1]
    n = torch.full((B,), Cn, dtype=torch.int32, device=s.device) if ncells is None else _dev(torch.as_tensor(ncells), torch.int32)
    if tuple(n.shape) != (B,):
        raise ValueError(f"patch_points: ncells {tuple(n.shape)} ([B])")
    out = torch.empty((B, Cn), dtype=torch.int32, device=s.device)
    if B == 0 or Cn == 0:                                  # nothing to answer: an empty tensor has no address to pass
        return out
    check(lib.fp_patch_points(context(), ptr(s), s.shape[0], ptr(T), ptr(K), ptr(c), ptr(n), B, Cn, float(patch), ptr(out),
                              current_stream()), "fp_patch_points")
    return out


def pnp_epnp(pts3d, pts2d, K, vis=None) -> torch.Tensor:
    """cv2.solvePnP(..., flags=SOLVEPNP_EPNP) (reference tracking_refiner.py:173, smooth_poses_video.py:182) for the B frames of an
    interval in one call: pts3d f64 [N,3] shared, pts2d f64 [B,N,2] (the tracker's pred_tracks), K [3,3], vis bool / u8 [B,N] or None
    (all points used) -> f64 [B,16] on the device = R[9] row-major, t[3], mean reprojection error (px), used points, status (PNP_OK,
    PNP_FEW: fewer than 4 used points, PNP_SINGULAR: coplanar or coincident points), 0.  R, t are NaN where the status is not 0."""
    lib = _lib.load()
    p3 = _dev(torch.as_tensor(pts3d), torch.float64)
    p2 = _dev(torch.as_tensor(pts2d), torch.float64)
    Kd = _dev(torch.as_tensor(K), torch.float64)
    if p3.dim() != 2 or p3.shape[1] != 3 or p2.dim() != 3 or tuple(p2.shape[1:]) != (p3.shape[0], 2) or Kd.numel() != 9:
        raise ValueError(f"pnp_epnp: pts3d {tuple(p3.shape)}, pts2d {tuple(p2.shape)}, K {tuple(Kd.shape)} ([N,3], [B,N,2], [3,3])")
    B, N = p2.shape[0], p3.shape[0]
    v = None
    if vis is not None:
        v = _dev(torch.as_tensor(vis))
        v = _dev(v != 0, torch.uint8)
        if tuple(v.shape) != (B, N):
            raise ValueError(f"pnp_epnp: vis {tuple(v.shape)} ([B,N] = {(B, N)})")
    out = torch.empty((B, 16), dtype=torch.float64, device=p3.device)
    if B == 0:                                             # no problem: an empty tensor has no address to pass
        return out
    check(lib.fp_pnp_epnp(context(), ptr(p3), ptr(p2), ptr(v), ptr(Kd), B, N, ptr(out), current_stream()), "fp_pnp_epnp")
    return out


# ---- the built-in point tracker: pyramidal Lucas-Kanade (csrc/lk_track.hip) -------------------------
LK_MAX_LEVELS, LK_MAX_RADIUS, LK_MAX_ITERS = 8, 15, 64     # csrc/lk_core.h
LK_FLAG_FB, LK_FLAG_EIG, LK_FLAG_RESIDUAL, LK_FLAG_OUTSIDE, LK_FLAG_LOST_BEFORE = 1, 2, 4, 8, 16


def lk_layout(H: int, W: int, levels: int, radius: int):
    """[(h_l, w_l)] of the levels fp_lk_pyramid keeps (csrc/lk_core.h lk_pyramid_layout): h_l = (h_{l-1} + 1) // 2, a level whose smaller
    side is below 2 radius + 1 is dropped with all coarser ones, level 0 always stays"""
    sizes = [(int(H), int(W))]
    for _ in range(1, int(levels)):
        h, w = (sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2
        if min(h, w) < 2 * int(radius) + 1:
            break
        sizes.append((h, w))
    return sizes


def lk_pyramid(frames, levels: int = 4, radius: int = 7) -> torch.Tensor:
    """frames u8 [T,H,W,3] (RGB) -> the grey pyramid as one f32 device tensor, the levels of lk_layout back to back, each [T,h_l,w_l]
    (fp_lk_pyramid; split it with lk_levels)"""
    lib = _lib.load()
    f = _dev(torch.as_tensor(frames))
    if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3:
        raise ValueError(f"lk_pyramid: frames {f.dtype} {tuple(f.shape)} (uint8 [T,H,W,3])")
    T, H, W = (int(v) for v in f.shape[:3])
    n = sum(T * h * w for h, w in lk_layout(H, W, levels, radius)) if 1 <= int(levels) <= LK_MAX_LEVELS and 1 <= int(radius) <= LK_MAX_RADIUS else 1
    out = torch.empty(max(n, 1), dtype=torch.float32, device=f.device)
    check(lib.fp_lk_pyramid(context(), ptr(f) if f.numel() else None, T, H, W, int(levels), int(radius), ptr(out), current_stream()),
          "fp_lk_pyramid")
    return out


def lk_levels(pyramid: torch.Tensor, T: int, H: int, W: int, levels: int, radius: int):
    """views [T,h_l,w_l] of the levels of an lk_pyramid tensor"""
    out, off = [], 0
    for h, w in lk_layout(H, W, levels, radius):
        out.append(pyramid[off:off + T * h * w].view(T, h, w))
        off += T * h * w
    return out


def lk_track(pyramid: torch.Tensor, T: int, H: int, W: int, queries, levels: int = 4, radius: int = 7, iters: int = 10,
             fb_thresh: float = 1.0, min_eig: float = 0.0, max_residual: float = 255.0):
    """fp_lk_track: pyramid from lk_pyramid(frames, levels, radius) of T frames of H x W, queries f32 [N,3] = (t, x, y) ->
    (tracks f32 [T,N,2], visibility u8 [T,N], diagnostics f32 [T,N,4] = forward-backward distance, eigenvalue, residual, flags), all on
    the device; nothing is synchronised.  The algorithm: include/freepose_hip.h, DESIGN.md §18."""
    lib = _lib.load()
    q = _dev(torch.as_tensor(queries), torch.float32)
    if q.dim() != 2 or q.shape[1] != 3:
        raise ValueError(f"lk_track: queries {tuple(q.shape)} ([N,3] = (t, x, y))")
    if not (pyramid.is_cuda and pyramid.dtype == torch.float32 and pyramid.is_contiguous()):
        raise ValueError("lk_track: the pyramid is the float32 device tensor lk_pyramid returns")
    if 1 <= int(levels) <= LK_MAX_LEVELS and 1 <= int(radius) <= LK_MAX_RADIUS and T >= 1 and H >= 1 and W >= 1:
        need = sum(T * h * w for h, w in lk_layout(H, W, levels, radius))
        if pyramid.numel() < need:
            raise ValueError(f"lk_track: pyramid of {pyramid.numel()} floats, {need} needed for T={T}, {H} x {W}, levels={levels}, radius={radius}")
    N = int(q.shape[0])
    Tn = max(int(T), 0)
    tracks = torch.empty((Tn, N, 2), dtype=torch.float32, device=q.device)
    vis = torch.empty((Tn, N), dtype=torch.uint8, device=q.device)
    diag = torch.empty((Tn, N, 4), dtype=torch.float32, device=q.device)
    check(lib.fp_lk_track(context(), ptr(pyramid), int(T), int(H), int(W), int(levels), ptr(q) if N else None, N, int(radius), int(iters),
                          float(fb_thresh), float(min_eig), float(max_residual), ptr(tracks) if N else None, ptr(vis) if N else None,
                          ptr(diag) if N else None, current_stream()), "fp_lk_track")
    return tracks, vis, diag


# ---- video velocity errors (csrc/video_eval.hip) ----------------------------------------------------
VIDEO_META_LD, VIDEO_PARAM_LD = 20, 16                     # csrc/video_eval_core.h FP_VE_META_LD / FP_VE_PARAM_LD
VIDEO_MAX_OFFSETS, VIDEO_MAX_SYM, VIDEO_MAX_TRACKS = 16, 1024, 65535
VIDEO_HAS_AXIS, VIDEO_HAS_K, VIDEO_NO_ALIGN = 1, 2, 4


def _pose_rows(x, what) -> torch.Tensor:
    """[B,N,4,4] poses (or [B,N,12] = R[9] row-major, t[3]) -> f64 [B,N,12] on the device"""
    p = _dev(torch.as_tensor(x), torch.float64)
    if p.dim() == 4 and tuple(p.shape[2:]) == (4, 4):
        p = torch.cat([p[:, :, :3, :3].reshape(p.shape[0], p.shape[1], 9), p[:, :, :3, 3]], dim=2).contiguous()
    if p.dim() != 3 or p.shape[2] != 12:
        raise ValueError(f"video_errors: {what} {tuple(p.shape)} ([B,N,4,4] or [B,N,12])")
    return p


def _per_track(x, M, what, dtype, tail=()):
    a = np.asarray(x, dtype=dtype)
    if a.shape == tuple(tail):
        a = np.broadcast_to(a, (M,) + tuple(tail))
    if a.shape != (M,) + tuple(tail):
        raise ValueError(f"video_errors: {what} {a.shape} (one per track: {(M,) + tuple(tail)})")
    return a


def video_errors(est, gt, dts, est_scale, gt_scale, w, h, video=None, n_frames=None, sym_axis=None, n_sym=101, K=None,
                 align: bool = True, return_aligned: bool = False, return_pairs: bool = False):
    """The velocity errors of the reference's src/utils/video_evaluation.py (get_average_rot / proj / depth_errors_dt :4-34 with
    get_rot_errors :37-63, get_translation_errors_depth / _proj :66-109, align_object_origins :112-155) for M tracks against V ground-truth
    trajectories in one call: est f64 [M,Nmax,4,4] (or [M,Nmax,12] = R[9] row-major, t[3]) estimated poses, gt [V,Nmax,4,4] likewise, dts
    int [M,D] time offsets (D <= 16, 1 <= dt <= N - 1), est_scale / gt_scale / w / h one number or [M], video int [M] row of gt a track
    is scored against (default: its own index, V == M), n_frames int [M] length N >= 2 of each track (default Nmax; rows past it are
    padding), sym_axis None, one 3-vector for all, or M entries of None / 3-vector (used as given, not normalised), n_sym the symmetry
    grid linspace(-pi, pi, n_sym), 1..1024, K None, one [3,3], or M entries of None / [3,3] (None: f = sqrt(w^2 + h^2), c = (w/2, h/2))
    -> (per_offset f64 [M,D,3], final f64 [M,3]) on the device: per offset the mean over the N - dt pairs / dt of (rot, proj, depth);
    final = mean over the offsets with rot in degrees and proj / sqrt(w^2 + h^2) * 100 (eval_videos.py:195-205).  align=False scores
    the translations as given (no origin alignment: get_translation_errors_* called on their own).  return_aligned adds
    f64 [M,Nmax,3], the estimates' translations at the aligned object origin; return_pairs adds f64 [M,D,Nmax,3], the per-pair errors
    (NaN at t1 >= N - dt).  Fixed summation order, no atomics: two calls give the same bits."""
    lib = _lib.load()
    e, g = _pose_rows(est, "est"), _pose_rows(gt, "gt")
    M, Nmax, V = e.shape[0], e.shape[1], g.shape[0]
    if g.shape[1] != Nmax:
        raise ValueError(f"video_errors: gt {tuple(g.shape)} for est {tuple(e.shape)} (the same Nmax)")
    d = np.asarray(dts)
    if d.ndim == 1:
        d = np.broadcast_to(d, (M, len(d)))
    if d.ndim != 2 or d.shape[0] != M or not 1 <= d.shape[1] <= VIDEO_MAX_OFFSETS or not np.issubdtype(d.dtype, np.integer):
        raise ValueError(f"video_errors: dts {d.shape} {d.dtype} (int [M,D] = [{M}, 1..{VIDEO_MAX_OFFSETS}])")
    D = d.shape[1]
    if video is None and V != M:
        raise ValueError(f"video_errors: {M} tracks, {V} ground-truth trajectories and no `video`")
    meta = np.zeros((M, VIDEO_META_LD), np.int32)
    params = np.zeros((M, VIDEO_PARAM_LD), np.float64)
    meta[:, 0] = np.arange(M) if video is None else _per_track(video, M, "video", np.int64)
    meta[:, 1] = Nmax if n_frames is None else _per_track(n_frames, M, "n_frames", np.int64)
    meta[:, 2] = _per_track(n_sym, M, "n_sym", np.int64)
    meta[:, 4:4 + D] = d
    meta[:, 3] = 0 if align else VIDEO_NO_ALIGN
    for col, (x, what) in enumerate(((est_scale, "est_scale"), (gt_scale, "gt_scale"), (w, "w"), (h, "h"))):
        params[:, col] = _per_track(x, M, what, np.float64)
    def entries(x, shape):                                 # None, one value for all, or one (None or value) per track
        if x is None:
            return [None] * M
        if not any(v is None for v in x) and np.shape(x) == shape:
            return [x] * M
        return list(x)
    axes, Ks = entries(sym_axis, (3,)), entries(K, (3, 3))
    if len(axes) != M or len(Ks) != M:
        raise ValueError(f"video_errors: {len(axes)} sym_axis / {len(Ks)} K entries for {M} tracks")
    for m in range(M):
        if axes[m] is not None:
            a = np.asarray(axes[m], dtype=np.float64)
            if a.shape != (3,):
                raise ValueError(f"video_errors: sym_axis of track {m} {a.shape} ([3])")
            meta[m, 3] |= VIDEO_HAS_AXIS
            params[m, 4:7] = a
        if Ks[m] is not None:
            k = np.asarray(Ks[m], dtype=np.float64)
            if k.shape != (3, 3):
                raise ValueError(f"video_errors: K of track {m} {k.shape} ([3,3])")
            meta[m, 3] |= VIDEO_HAS_K
            params[m, 7:16] = k.ravel()
    if M > VIDEO_MAX_TRACKS:
        raise ValueError(f"video_errors: {M} tracks (at most {VIDEO_MAX_TRACKS} per call)")
    per = torch.empty((M, D, 3), dtype=torch.float64, device=e.device)
    fin = torch.empty((M, 3), dtype=torch.float64, device=e.device)
    aligned = torch.zeros((M, Nmax, 3), dtype=torch.float64, device=e.device) if return_aligned else None
    pairs = torch.full((M, D, Nmax, 3), float("nan"), dtype=torch.float64, device=e.device) if return_pairs else None
    if M > 0:                                              # no track: an empty tensor has no address to pass
        check(lib.fp_video_errors(context(), ptr(e), ptr(g), ptr(meta), ptr(params), M, V, Nmax, D, ptr(per), ptr(fin), ptr(aligned),
                                  ptr(pairs), current_stream()), "fp_video_errors")
    out = (per, fin)
    if return_aligned:
        out += (aligned,)
    if return_pairs:
        out += (pairs,)
    return out


# ---- BOP scores: pose matching and recall counts (csrc/bop_score.hip) -------------------------------
BOP_GROUP_LD = 4                                           # csrc/bop_score_core.h FP_BS_GROUP_LD: {err_offset, E, G, first_gt_row}
BOP_MAX_THRESHOLDS = 65536


def bop_tables_check(err, groups, gt_valid, gt_obj, gt_scene, th, n_obj, n_scene):
    """The limits of fp_bop_scores on the host twins of its tables (numpy only, no device): returns them as contiguous arrays of the
    entry's types, or raises ValueError with the offending group."""
    err = np.ascontiguousarray(err, dtype=np.float64).reshape(-1)
    groups = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1, BOP_GROUP_LD)
    gt_valid = np.ascontiguousarray(gt_valid, dtype=np.uint8).reshape(-1)
    gt_obj = np.ascontiguousarray(gt_obj, dtype=np.int32).reshape(-1)
    gt_scene = np.ascontiguousarray(gt_scene, dtype=np.int32).reshape(-1)
    th = np.ascontiguousarray(th, dtype=np.float64).reshape(-1)
    P, Gr, R, T = len(err), len(groups), len(gt_valid), len(th)
    if not 1 <= T <= BOP_MAX_THRESHOLDS:
        raise ValueError(f"bop_scores: T={T} thresholds (1..{BOP_MAX_THRESHOLDS})")
    if int(n_obj) < 1 or int(n_scene) < 1:
        raise ValueError(f"bop_scores: n_obj={n_obj}, n_scene={n_scene} (>= 1)")
    if len(gt_obj) != R or len(gt_scene) != R:
        raise ValueError(f"bop_scores: gt_valid [{R}], gt_obj [{len(gt_obj)}], gt_scene [{len(gt_scene)}] (one row per ground truth)")
    if max(Gr, R, int(n_obj), int(n_scene)) * T >= 2 ** 31 or P >= 2 ** 31:
        raise ValueError(f"bop_scores: Gr={Gr}, R={R}, n_obj={n_obj}, n_scene={n_scene} times T={T}, and P={P} (each below 2^31)")
    g = groups.astype(np.int64)
    off, E, G, first = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    bad = np.flatnonzero((off < 0) | (E < 0) | (G < 0) | (first < 0) | (off + E * G > P) | (first + G > R))
    if len(bad):
        i = int(bad[0])
        raise ValueError(f"bop_scores: group {i} = {groups[i].tolist()} reaches outside P={P} errors or R={R} ground truths")
    rows = np.flatnonzero(G > 0)
    rows = rows[np.argsort(first[rows], kind="stable")]
    over = np.flatnonzero(first[rows][:-1] + G[rows][:-1] > first[rows][1:])
    if len(over):
        a, b = int(rows[over[0]]), int(rows[over[0] + 1])
        raise ValueError(f"bop_scores: groups {a} and {b} share ground-truth rows ({groups[a].tolist()}, {groups[b].tolist()})")
    if len(rows):
        Gs, fs = G[rows], first[rows]
        idx = np.repeat(fs, Gs) + (np.arange(int(Gs.sum())) - np.repeat(np.cumsum(Gs) - Gs, Gs))
        for name, col, n in (("gt_obj", gt_obj, int(n_obj)), ("gt_scene", gt_scene, int(n_scene))):
            head = np.repeat(col[fs], Gs)
            wrong = np.flatnonzero((col[idx] != head) | (head < 0) | (head >= n))
            if len(wrong):
                r = int(idx[wrong[0]])
                raise ValueError(f"bop_scores: {name}[{r}] = {int(col[r])} (one index in 0..{n - 1} for all rows of a group)")
    return err, groups, gt_valid, gt_obj, gt_scene, th


def bop_scores(err, groups, gt_valid, gt_obj, gt_scene, th, n_obj: int, n_scene: int, n_top: int = 0):
    """Pose matching and recall counts of the BOP toolkit (pose_matching.py match_poses :39-87, score.py :77-109) for every group and all
    T thresholds in one launch.  Host tables (numpy): err f64 [P] (per group a row-major [E,G] block, estimates in matching order and cut to
    n_top, ground truths in visiting order, already normalised), groups i32 [Gr,4] = {err_offset, E, G, first_gt_row}, gt_valid u8 [R],
    gt_obj / gt_scene i32 [R] indices into the object / scene lists, th f64 [T]; n_top > 0 caps the targets of a group.  The tables are
    checked (bop_tables_check: ValueError with a message, nothing is launched) and uploaded.
    -> device tensors (match i32 [T,R]: row of the matched estimate within its group or -1, tp_obj i32 [T,n_obj], tp_scene i32 [T,n_scene],
    tar_obj i32 [n_obj], tar_scene i32 [n_scene]).  Comparisons and integer sums only: exact, and two calls give the same bits."""
    err, groups, gt_valid, gt_obj, gt_scene, th = bop_tables_check(err, groups, gt_valid, gt_obj, gt_scene, th, n_obj, n_scene)
    lib = _lib.load()
    P, Gr, R, T = len(err), len(groups), len(gt_valid), len(th)
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda a: torch.from_numpy(a).to(dev) if a.size else None   # noqa: E731  (an empty tensor has no address to pass)
    d_err, d_groups, d_valid, d_obj, d_scene, d_th = up(err), up(groups), up(gt_valid), up(gt_obj), up(gt_scene), up(th)
    match = torch.empty((T, R), dtype=torch.int32, device=dev)
    tp_obj = torch.empty((T, int(n_obj)), dtype=torch.int32, device=dev)
    tp_scene = torch.empty((T, int(n_scene)), dtype=torch.int32, device=dev)
    tar_obj = torch.empty((int(n_obj),), dtype=torch.int32, device=dev)
    tar_scene = torch.empty((int(n_scene),), dtype=torch.int32, device=dev)
    check(lib.fp_bop_scores(context(), ptr(d_err), ptr(d_groups), ptr(d_valid), ptr(d_obj), ptr(d_scene), ptr(d_th), P, Gr, R, T, int(n_obj),
                            int(n_scene), int(n_top), ptr(match) if R else None, ptr(tp_obj), ptr(tp_scene), ptr(tar_obj), ptr(tar_scene),
                            current_stream()), "fp_bop_scores")
    return match, tp_obj, tp_scene, tar_obj, tar_scene


# ---- pose-error evaluation (csrc/eval.hip) ----------------------------------------------------------
EVAL_XF_LD, EVAL_TABLE_LD, EVAL_MAX_TAUS = 40, 8, 16      # csrc/internal.h FP_EVAL_*
EVAL_MAX_PAIRS = 65535                                     # pairs per launch (grid z / y)
EVAL_MAX_WS_POINTS = 32 << 20                              # centred points held in the context's workspace per launch (12 bytes each)


def _per_pair(x, B, shape, what):
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)
    if a.size == int(np.prod(shape)):
        a = np.broadcast_to(a.reshape(shape), (B,) + tuple(shape))
    if a.size != B * int(np.prod(shape)):
        raise ValueError(f"{what}: expected {tuple(shape)} or {(B,) + tuple(shape)}, got {a.shape}")
    return a.reshape((B,) + tuple(shape))


def _chamfer(clouds, pairs, s_e, R_e, t_e, R_g, t_g, K):
    lib = _lib.load()
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    B = pairs.shape[0]
    dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((B,), dtype=torch.float64, device=dev)
    if B == 0:
        return out
    cl = [_dev(torch.as_tensor(c), torch.float64).reshape(-1, 3) for c in clouds]
    sizes = np.array([c.shape[0] for c in cl], dtype=np.int64)
    if (sizes <= 0).any():
        raise ValueError("chamfer: empty vertex cloud")
    if pairs.min() < 0 or pairs.max() >= len(cl):
        raise ValueError("chamfer: pair refers to a cloud that was not given")
    starts = np.concatenate([[0], np.cumsum(sizes)])
    if starts[-1] >= 1 << 31:
        raise ValueError("chamfer: more than 2^31 vertices in one call")
    pts = cl[0] if len(cl) == 1 else torch.cat(cl, dim=0)
    centroid = {}
    for g in np.unique(pairs[:, 1]):                       # origin of the centred clouds: any point near the object does
        centroid[int(g)] = cl[int(g)].mean(dim=0).cpu().numpy()
    xf = np.zeros((B, EVAL_XF_LD), dtype=np.float64)
    xf[:, 0] = _per_pair(s_e, B, (), "s_e")
    xf[:, 1:10] = _per_pair(R_e, B, (3, 3), "R_e").reshape(B, 9)
    xf[:, 10:13] = _per_pair(t_e, B, (3,), "t_e")
    xf[:, 13:22] = _per_pair(R_g, B, (3, 3), "R_g").reshape(B, 9)
    xf[:, 22:25] = _per_pair(t_g, B, (3,), "t_g")
    xf[:, 25:28] = np.stack([centroid[int(g)] for g in pairs[:, 1]])
    if K is not None:
        xf[:, 28:37] = _per_pair(K, B, (3, 3), "K").reshape(B, 9)
    n_e, n_g = sizes[pairs[:, 0]], sizes[pairs[:, 1]]
    b0 = 0
    while b0 < B:                                          # launches bounded by the pair count and by the workspace
        b1, ws = b0, 0
        while b1 < B and b1 - b0 < EVAL_MAX_PAIRS and (b1 == b0 or ws + n_e[b1] + n_g[b1] <= EVAL_MAX_WS_POINTS):
            ws += int(n_e[b1] + n_g[b1])
            b1 += 1
        if ws >= 1 << 31:
            raise ValueError("chamfer: one pair of clouds exceeds the workspace index range")
        nb = b1 - b0
        table = np.zeros((nb, EVAL_TABLE_LD), dtype=np.int32)
        table[:, 0], table[:, 1] = starts[pairs[b0:b1, 0]], n_e[b0:b1]
        table[:, 2], table[:, 3] = starts[pairs[b0:b1, 1]], n_g[b0:b1]
        slot = np.concatenate([[0], np.cumsum(n_e[b0:b1] + n_g[b0:b1])])
        table[:, 4], table[:, 5] = slot[:-1], slot[:-1] + n_e[b0:b1]
        d_table = torch.from_numpy(table).to(dev)
        d_xf = torch.from_numpy(xf[b0:b1].copy()).to(dev)
        max_n = int(max(n_e[b0:b1].max(), n_g[b0:b1].max()))
        check(lib.fp_chamfer(context(), ptr(pts), int(starts[-1]), ptr(d_table), ptr(d_xf), nb, max_n, int(ws), int(K is not None),
                             C.c_void_p(out.data_ptr() + 8 * b0), current_stream()), "fp_chamfer")
        b0 = b1
    return out


def chamfer(clouds, pairs, s_e, R_e, t_e, R_g, t_g) -> torch.Tensor:
    """bidirectional chamfer distance of posed vertex clouds (bop_toolkit pose_error.chamfer) for B pairs at once -> f64 [B] on device.
    clouds: list of [N_i,3] float64 vertex arrays (numpy or device tensors); pairs int [B,2] = (cloud of the mesh used at inference,
    cloud of the ground-truth model); s_e [B] scales the inference cloud first; R_* [B,3,3], t_* [B,3] (or one for all pairs)."""
    return _chamfer(clouds, pairs, s_e, R_e, t_e, R_g, t_g, None)


def chamfer_proj(clouds, pairs, s_e, R_e, t_e, R_g, t_g, K) -> torch.Tensor:
    """chamfer() of the clouds projected by K [3,3] (or [B,3,3]) into the image, in pixels (pose_error.chamfer_proj)"""
    return _chamfer(clouds, pairs, s_e, R_e, t_e, R_g, t_g, K)


def depth_compare(depth_est: torch.Tensor, depth_gt: torch.Tensor, depth_test: Optional[torch.Tensor] = None, img_idx=None, K=None,
                  delta=None, taus=None, divisor=1.0) -> torch.Tensor:
    """pixel counts of B pairs of rendered depth images f32 [B,H,W] -> i32 [B,4] = (inter, union of depth > 0, 0, 0): pose_error.cus.
    With depth_test f32 [n_img,H,W] (+ img_idx [B], K [3,3] | [B,3,3], delta, taus [n_tau], divisor = diameter or 1 per pair):
    i32 [B, 4 + n_tau] = (inter, union, visib_inter, visib_union, cost-1 pixels per tau): pose_error.vsd."""
    lib = _lib.load()
    de, dg = _dev(depth_est, torch.float32), _dev(depth_gt, torch.float32)
    if de.dim() != 3 or de.shape != dg.shape:
        raise ValueError(f"depth_compare: depth stacks {tuple(de.shape)} and {tuple(dg.shape)}")
    B, H, W = de.shape
    if depth_test is None:
        out = torch.zeros((B, 4), dtype=torch.int32, device=de.device)
        for b0 in range(0, B, EVAL_MAX_PAIRS):
            nb = min(EVAL_MAX_PAIRS, B - b0)
            check(lib.fp_depth_compare(context(), ptr(de[b0:]), ptr(dg[b0:]), nb, H, W, None, 0, None, None, None, 0, ptr(out[b0:]),
                                       current_stream()), "fp_depth_compare")
        return out
    dt = _dev(depth_test, torch.float32)
    if dt.dim() == 2:
        dt = dt[None]
    if tuple(dt.shape[1:]) != (H, W):
        raise ValueError(f"depth_compare: test depth {tuple(dt.shape)} for renders of {H} x {W}")
    tau = np.asarray(taus, dtype=np.float64).reshape(-1)
    if not 0 < tau.size <= EVAL_MAX_TAUS:
        raise ValueError(f"depth_compare: {tau.size} taus (1..{EVAL_MAX_TAUS})")
    idx = np.zeros(B, np.int32) if img_idx is None else np.asarray(img_idx, dtype=np.int32).reshape(B)
    if B and (idx.min() < 0 or idx.max() >= dt.shape[0]):
        raise ValueError("depth_compare: img_idx outside the test depth stack")
    Kb = _per_pair(K, B, (3, 3), "K")
    prm = np.zeros((B, 8), dtype=np.float64)
    prm[:, 0], prm[:, 1], prm[:, 2], prm[:, 3] = Kb[:, 0, 0], Kb[:, 1, 1], Kb[:, 0, 2], Kb[:, 1, 2]
    prm[:, 4] = _per_pair(delta, B, (), "delta")
    prm[:, 5] = _per_pair(divisor, B, (), "divisor")
    d_prm, d_idx, d_tau = torch.from_numpy(prm).to(de.device), torch.from_numpy(idx).to(de.device), torch.from_numpy(tau).to(de.device)
    out = torch.zeros((B, 4 + tau.size), dtype=torch.int32, device=de.device)
    for b0 in range(0, B, EVAL_MAX_PAIRS):
        nb = min(EVAL_MAX_PAIRS, B - b0)
        check(lib.fp_depth_compare(context(), ptr(de[b0:]), ptr(dg[b0:]), nb, H, W, ptr(dt), int(dt.shape[0]), ptr(d_idx[b0:]),
                                   ptr(d_prm[b0:]), ptr(d_tau), int(tau.size), ptr(out[b0:]), current_stream()), "fp_depth_compare")
    return out


# ---- ground-truth info (csrc/gt_info.hip) -----------------------------------------------------------
GT_INFO_OUT_LD = 12                                        # csrc/gt_info_core.h FP_GI_OUT_LD
GT_INFO_MAX_BATCH = 65535                                  # instances per launch (grid y); tests lower it
GT_INFO_BOX_EMPTY = (2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31)   # the box no pixel has touched
DIAMETER_TILE = 1024                                       # csrc/gt_info.hip DM_TILE
DIAMETER_MAX_POINTS = 1 << 21                              # csrc/internal.h FP_DIAM_MAX_POINTS
DIAMETER_MAX_MODELS = 65535                                # models per launch (grid y); tests lower it
DIAMETER_MAX_SLOTS = 1 << 24                               # per-block maxima per launch (128 MiB of workspace; the entry takes up to 2^26)


def gt_visibility(depth_gt, depth_test, img_idx, K, delta, window=None, want_masks: bool = True):
    """calc_gt_info.py:131-173 / calc_gt_masks.py:107-126 for B ground-truth instances in one fused pass each (fp_gt_visibility).
    depth_gt f32 [B,Hr,Wr] rendered canvases; depth_test f32 [n_img,H,W] (or [H,W]) test depth in the unit of the renders; img_idx [B]
    the image of each instance (None: image 0); K [3,3] | [B,3,3] the IMAGE's intrinsics; delta one value or [B]; window = (ox, oy): the
    image is canvas[oy:oy+H, ox:ox+W] (None: the canvases have the image's size).
    -> (counts i32 [B,12] = {px_count_all, px_count_valid, px_count_visib, 0, box of the silhouette: min x, min y, max x, max y relative to
    the window, box of the visible mask}, mask u8 [B,H,W], mask_visib u8 [B,H,W]) on the device; the masks are None without want_masks.
    An untouched box is GT_INFO_BOX_EMPTY.  ValueError for what the C entry would refuse."""
    lib = _lib.load()
    dg, dt = _dev(torch.as_tensor(depth_gt), torch.float32), _dev(torch.as_tensor(depth_test), torch.float32)
    if dt.dim() == 2:
        dt = dt[None]
    if dg.dim() != 3 or dt.dim() != 3:
        raise ValueError(f"gt_visibility: depth stacks {tuple(dg.shape)} and {tuple(dt.shape)} ([B,Hr,Wr] and [n_img,H,W])")
    B, Hr, Wr = dg.shape
    n_img, H, W = dt.shape
    if window is None:
        if (Hr, Wr) != (H, W):
            raise ValueError(f"gt_visibility: canvases of {Wr} x {Hr} for images of {W} x {H} need a window")
        ox, oy = 0, 0
    else:
        ox, oy = int(window[0]), int(window[1])
    if n_img < 1 or H < 1 or W < 1 or Hr * Wr > 1 << 30:
        raise ValueError(f"gt_visibility: {n_img} test images of {W} x {H}, canvas {Wr} x {Hr}")
    if ox < 0 or oy < 0 or ox + W > Wr or oy + H > Hr:
        raise ValueError(f"gt_visibility: window {W} x {H} at ({ox}, {oy}) leaves the canvas {Wr} x {Hr}")
    idx = np.zeros(B, np.int32) if img_idx is None else np.asarray(img_idx, dtype=np.int64).reshape(-1)
    if idx.size != B:
        raise ValueError(f"gt_visibility: {idx.size} image indices for {B} instances")
    if B and (idx.min() < 0 or idx.max() >= n_img):
        raise ValueError(f"gt_visibility: img_idx outside [0, {n_img})")
    Kb = _per_pair(K, B, (3, 3), "K")
    prm = np.zeros((B, 8), dtype=np.float64)
    prm[:, 0], prm[:, 1], prm[:, 2], prm[:, 3] = Kb[:, 0, 0], Kb[:, 1, 1], Kb[:, 0, 2], Kb[:, 1, 2]
    prm[:, 4] = _per_pair(delta, B, (), "delta")
    out = torch.empty((B, GT_INFO_OUT_LD), dtype=torch.int32, device=dg.device)
    mask = torch.empty((B, H, W), dtype=torch.uint8, device=dg.device) if want_masks else None
    visib = torch.empty((B, H, W), dtype=torch.uint8, device=dg.device) if want_masks else None
    if B == 0:
        return out, mask, visib
    d_prm, d_idx = torch.from_numpy(prm).to(dg.device), torch.from_numpy(idx.astype(np.int32)).to(dg.device)
    for b0 in range(0, B, GT_INFO_MAX_BATCH):
        nb = min(GT_INFO_MAX_BATCH, B - b0)
        check(lib.fp_gt_visibility(context(), ptr(dg[b0:]), nb, Hr, Wr, ox, oy, ptr(dt), n_img, H, W, ptr(d_idx[b0:]), ptr(d_prm[b0:]),
                                   ptr(mask[b0:]) if want_masks else None, ptr(visib[b0:]) if want_masks else None, ptr(out[b0:]),
                                   current_stream()), "fp_gt_visibility")
    return out, mask, visib


def pts_diameter(clouds) -> torch.Tensor:
    """misc.calc_pts_diameter (misc.py:289-303) and the box of calc_model_info.py:36-37 for M vertex clouds at once (fp_pts_diameter).
    clouds: list of [N_i,3] float64 arrays (numpy or tensors) -> f64 [M,8] on the device = {diameter, min x, y, z, size x, y, z, 0},
    bit for bit the reference's float64 values.  Launches are split by model count and by the workspace of per-block maxima.
    ValueError for an empty cloud or one above DIAMETER_MAX_POINTS points."""
    lib = _lib.load()
    cl = [_dev(torch.as_tensor(c), torch.float64).reshape(-1, 3) for c in clouds]
    M = len(cl)
    dev = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((M, 8), dtype=torch.float64, device=dev)
    if M == 0:
        return out
    sizes = np.array([c.shape[0] for c in cl], dtype=np.int64)
    if (sizes <= 0).any():
        raise ValueError(f"pts_diameter: cloud {int(np.flatnonzero(sizes <= 0)[0])} is empty")
    if sizes.max() > DIAMETER_MAX_POINTS:
        raise ValueError(f"pts_diameter: a cloud of {int(sizes.max())} points (at most {DIAMETER_MAX_POINTS})")
    starts = np.concatenate([[0], np.cumsum(sizes)])
    if starts[-1] >= 1 << 31:
        raise ValueError("pts_diameter: more than 2^31 points in one call")
    pts = cl[0] if M == 1 else torch.cat(cl, dim=0)
    tiles = -(-sizes // DIAMETER_TILE)
    pairs = tiles * (tiles + 1) // 2
    if pairs.max() > DIAMETER_MAX_SLOTS:
        raise ValueError(f"pts_diameter: a cloud of {int(sizes.max())} points needs {int(pairs.max())} slots (limit {DIAMETER_MAX_SLOTS})")
    m0 = 0
    while m0 < M:                                          # a launch: at most DIAMETER_MAX_MODELS models, models x slots of the largest within the limit
        m1, most = m0, 0
        while m1 < M and m1 - m0 < DIAMETER_MAX_MODELS and (m1 == m0 or max(most, int(pairs[m1])) * (m1 - m0 + 1) <= DIAMETER_MAX_SLOTS):
            most = max(most, int(pairs[m1]))
            m1 += 1
        rg = np.stack([starts[m0:m1], sizes[m0:m1]], axis=1).astype(np.int32)
        d_rg = torch.from_numpy(rg).to(dev)
        check(lib.fp_pts_diameter(context(), ptr(pts), int(starts[-1]), ptr(d_rg), m1 - m0, ptr(out[m0:]), current_stream()), "fp_pts_diameter")
        m0 = m1
    return out


# ---- kernel-level ops (unit tests / microbenchmarks) ------------------------------------------------
def gemm(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, epi: int = 0, gamma=None, resid=None,
         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """epi 0: x w^T + b ; 1: gelu(.) ; 2: resid + gamma*(.)   (all bf16, fp32 accumulate)"""
    lib = _lib.load()
    x, w, bias = _dev(x, torch.bfloat16), _dev(w, torch.bfloat16), _dev(bias, torch.bfloat16)
    M, K = x.shape
    N = w.shape[0]
    g = _dev(gamma, torch.bfloat16) if gamma is not None else None
    r = _dev(resid, torch.bfloat16) if resid is not None else None
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    check(lib.fp_op_gemm(context(), ptr(x), K, ptr(w), K, ptr(out), N, ptr(bias), ptr(g), ptr(r), N, M, N, K, epi, current_stream()),
          "fp_op_gemm")
    return out


def gelu_direct(x: torch.Tensor) -> torch.Tensor:
    """bf16(0.5 x (1 + erf(x / sqrt 2))) elementwise, the direct fp32 expression the fc1 epilogue's GELU table is filled from"""
    x = _dev(x, torch.bfloat16)
    y = torch.empty_like(x)
    check(_lib.load().fp_op_gelu(ptr(x), ptr(y), x.numel(), current_stream()), "fp_op_gelu")
    return y


def gemm_vt(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, npad: int, heads: int,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    x, w, bias = _dev(x, torch.bfloat16), _dev(w, torch.bfloat16), _dev(bias, torch.bfloat16)
    M, K = x.shape
    N = w.shape[0]
    B = M // npad
    vt = out if out is not None else torch.zeros((B, heads, 64, npad), dtype=torch.bfloat16, device=x.device)
    check(lib.fp_op_gemm_vt(context(), ptr(x), K, ptr(w), K, ptr(vt), ptr(bias), M, N, K, npad, heads, current_stream()), "fp_op_gemm_vt")
    return vt


def ln_linear(x: torch.Tensor, g_ln: torch.Tensor, b_ln: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, mode: int = 0,
              npad: int = 0, heads: int = 0, eps: float = 1e-6, n_scaled: int = 0, row_scale: float = 1.0) -> torch.Tensor:
    """LayerNorm folded into the consuming linear layer (fp_op_ln_linear): mode 0 LN(x) w^T + b, 1 gelu(.), 2 transposed V store.
    Output features below n_scaled are multiplied by row_scale inside the fold (the ViT's q rows: ATTN_QSCALE)"""
    lib = _lib.load()
    x, w, bias = _dev(x, torch.bfloat16), _dev(w, torch.bfloat16), _dev(bias, torch.bfloat16)
    g_ln, b_ln = _dev(g_ln, torch.bfloat16), _dev(b_ln, torch.bfloat16)
    M, K = x.shape
    N = w.shape[0]
    if mode == 2:
        out = torch.zeros((M // npad, heads, 64, npad), dtype=torch.bfloat16, device=x.device)
    else:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    check(lib.fp_op_ln_linear(context(), ptr(x), M, K, ptr(g_ln), ptr(b_ln), float(eps), ptr(w), N, ptr(bias), int(mode), int(npad),
                              int(heads), int(n_scaled), float(row_scale), ptr(out), current_stream()), "fp_op_ln_linear")
    return out


def gemm_stats(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, gamma: torch.Tensor, resid: torch.Tensor, eps: float = 1e-6):
    """resid + gamma * (x w^T + b) plus the row statistics from the epilogue's partial sums (fp_op_gemm_stats): returns (out,
    stat f32 [M,3] = (mean, sigma, rstd)) — mean and sigma decoded from the two-piece bf16 splits the consuming GEMM reads"""
    lib = _lib.load()
    x, w, bias = _dev(x, torch.bfloat16), _dev(w, torch.bfloat16), _dev(bias, torch.bfloat16)
    g, r = _dev(gamma, torch.bfloat16), _dev(resid, torch.bfloat16)
    M, K = x.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    raw = torch.zeros((M, 6), dtype=torch.float32, device=x.device)
    check(lib.fp_op_gemm_stats(context(), ptr(x), K, ptr(w), K, ptr(out), N, ptr(bias), ptr(g), ptr(r), N, M, N, K, float(eps), ptr(raw),
                               current_stream()), "fp_op_gemm_stats")
    rec = raw[:, :4].contiguous().view(torch.bfloat16).float()          # [M, 8]: sh, sl, sh, -mh, -ml, -mh, 0, 0
    stat = torch.stack([-(rec[:, 3] + rec[:, 4]), rec[:, 0] + rec[:, 1], raw[:, 4]], dim=1)
    return out, stat


def gemm_patch(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, pos: torch.Tensor, tokens: torch.Tensor, tok_off: int) -> torch.Tensor:
    """the patch-embed GEMM (fp_op_gemm_patch), in place on the token buffer tokens bf16 [B, npad, D]: row b * P + p of x [B * P, K] lands
    in tokens[b, tok_off + p] as bf16(bf16(x w^T + bias) + pos[p]), pos bf16 [P, D]; the other rows are not touched"""
    lib = _lib.load()
    x, w, bias, pos = _dev(x, torch.bfloat16), _dev(w, torch.bfloat16), _dev(bias, torch.bfloat16), _dev(pos, torch.bfloat16)
    assert tokens.is_cuda and tokens.dtype == torch.bfloat16 and tokens.is_contiguous() and tokens.dim() == 3
    B, npad, D = tokens.shape
    M, K = x.shape
    P = pos.shape[0]
    assert tuple(w.shape) == (D, K) and tuple(pos.shape) == (P, D) and bias.numel() == D and M == B * P
    check(lib.fp_op_gemm_patch(context(), ptr(x), K, ptr(w), K, ptr(tokens), D, ptr(bias), ptr(pos), M, D, K, P, npad, int(tok_off),
                               current_stream()), "fp_op_gemm_patch")
    return tokens


def ln_chain(x1: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, gamma: torch.Tensor, resid: torch.Tensor, g_ln: torch.Tensor,
             b_ln: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, mode: int = 0, route: int = 0, eps: float = 1e-6, n_scaled: int = 0,
             row_scale: float = 1.0):
    """producer -> consumer pair of the folded LayerNorm (fp_op_ln_chain): y = resid + gamma * (x1 w1^T + b1) with the row sums of y from
    the epilogue, out = LN(y) w2^T + b2 (mode 0) or its GELU (mode 1).  route 0: the sums are finalised by their own kernel, 1: the
    consumer launch takes them along.  Returns (y, out, records i32 [M, 4], rstd f32 [M])"""
    lib = _lib.load()
    x1, w1, b1 = _dev(x1, torch.bfloat16), _dev(w1, torch.bfloat16), _dev(b1, torch.bfloat16)
    gamma, resid = _dev(gamma, torch.bfloat16), _dev(resid, torch.bfloat16)
    g_ln, b_ln, w2, b2 = _dev(g_ln, torch.bfloat16), _dev(b_ln, torch.bfloat16), _dev(w2, torch.bfloat16), _dev(b2, torch.bfloat16)
    M, K1 = x1.shape
    D, N2 = w1.shape[0], w2.shape[0]
    assert tuple(w1.shape) == (D, K1) and tuple(resid.shape) == (M, D) and tuple(w2.shape) == (N2, D)
    assert b1.numel() == D and gamma.numel() == D and g_ln.numel() == D and b_ln.numel() == D and b2.numel() == N2
    y = torch.empty((M, D), dtype=torch.bfloat16, device=x1.device)
    out = torch.empty((M, N2), dtype=torch.bfloat16, device=x1.device)
    rec = torch.empty((M, 4), dtype=torch.int32, device=x1.device)
    rstd = torch.empty((M,), dtype=torch.float32, device=x1.device)
    check(lib.fp_op_ln_chain(context(), ptr(x1), K1, ptr(w1), ptr(b1), ptr(gamma), ptr(resid), ptr(y), M, D, ptr(g_ln), ptr(b_ln), float(eps),
                             ptr(w2), N2, ptr(b2), int(mode), int(n_scaled), float(row_scale), int(route), ptr(out), N2, ptr(rec), ptr(rstd),
                             current_stream()), "fp_op_ln_chain")
    return y, out, rec, rstd


def ln_consume(x: torch.Tensor, rec: torch.Tensor, rstd: torch.Tensor, g_ln: torch.Tensor, b_ln: torch.Tensor, w: torch.Tensor,
               bias: torch.Tensor, mode: int = 0, npad: int = 0, heads: int = 0, n_scaled: int = 0, row_scale: float = 1.0) -> torch.Tensor:
    """ln_linear on row records the caller supplies (fp_op_ln_consume): rec i32 [M, 4], rstd f32 [M] as ln_chain, row_stats or
    stats_finalize return them — a further consumer of the same rows, e.g. the ViT's transposed-V launch (mode 2) behind its qk launch"""
    lib = _lib.load()
    x, w, bias = _dev(x, torch.bfloat16), _dev(w, torch.bfloat16), _dev(bias, torch.bfloat16)
    g_ln, b_ln = _dev(g_ln, torch.bfloat16), _dev(b_ln, torch.bfloat16)
    rec, rstd = _dev(rec, torch.int32), _dev(rstd, torch.float32)
    M, K = x.shape
    N = w.shape[0]
    assert tuple(rec.shape) == (M, 4) and tuple(rstd.shape) == (M,) and w.shape[1] == K and bias.numel() == N
    if mode == 2:
        out = torch.zeros((M // npad, heads, 64, npad), dtype=torch.bfloat16, device=x.device)
    else:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    check(lib.fp_op_ln_consume(context(), ptr(x), M, K, ptr(g_ln), ptr(b_ln), ptr(w), N, ptr(bias), int(mode), int(npad), int(heads),
                               int(n_scaled), float(row_scale), ptr(rec), ptr(rstd), ptr(out), N, current_stream()), "fp_op_ln_consume")
    return out


def gemm_plan(M: int, N: int, K: int, epi: int, ldx: Optional[int] = None, ldw: Optional[int] = None, ln_part: bool = False,
              device: Optional[int] = None) -> dict:
    """the plan the library's GEMM dispatch would execute on this device for such a launch, under the context's gemm_row_split
    (fp_op_gemm_plan; nothing is launched): {"label": tiny64 | small128 | big_hip | big_hip_stream | big_asm | split_big+<tier> |
    split_mid+<tier> | finalize_then_<label>, "row0": first row of the second part (0 = no split), "ring": K-tile ring depth of each part
    (0: not on the 64x64 tier), "grid": workgroups of each part, "text": the entry's own line}"""
    import ctypes
    buf = ctypes.create_string_buffer(160)
    check(_lib.load().fp_op_gemm_plan(context(device), int(M), int(N), int(K), int(epi), int(K if ldx is None else ldx), int(K if ldw is None else ldw),
                                      int(bool(ln_part)), buf, len(buf)), "fp_op_gemm_plan")
    text = buf.value.decode()
    label, *fields = text.split()
    kv = dict(f.split("=") for f in fields)
    return {"label": label, "row0": int(kv["row0"]), "ring": tuple(int(v) for v in kv["ring"].split(",")),
            "grid": tuple(int(v) for v in kv["grid"].split(",")), "text": text}


def raster_plan(W: int, H: int, F: int, Hn: int, device: Optional[int] = None) -> dict:
    """how rasterize() / rasterize_extents() would launch F triangles under Hn poses on a W x H frame, under the context's raster_tiled
    (fp_op_raster_plan; nothing is launched): {"path": "tiled" | "global", "T": tile edge, "tiles": (ntx, nty), "chunks", "rounds", "bin":
    bin workgroups per view, "views": (groups of 8, rest), "flush": "dword" | "bytes" | "none", "lds": bytes, "constants": {big_area,
    big_tile_area, chunk, hits_round, small_span, max_tris, max_tile, clamp, znear: the thresholds the kernels were compiled with},
    "text": the entry's own line}"""
    import ctypes
    buf = ctypes.create_string_buffer(384)
    check(_lib.load().fp_op_raster_plan(context(device), int(W), int(H), int(F), int(Hn), buf, len(buf)), "fp_op_raster_plan")
    return parse_raster_plan(buf.value.decode())


def parse_raster_plan(text: str) -> dict:
    """the dict of raster_plan() from the one-line text of fp_op_raster_plan / csrc/raster_plan.h plan_text"""
    path, *fields = text.split()
    kv = dict(f.split("=") for f in fields)
    plan = {"path": path, "T": int(kv.pop("T")), "tiles": tuple(int(v) for v in kv.pop("tiles").split("x")), "chunks": int(kv.pop("chunks")),
            "rounds": int(kv.pop("rounds")), "bin": int(kv.pop("bin")), "views": tuple(int(v) for v in kv.pop("views").split("+")),
            "flush": kv.pop("flush"), "lds": int(kv.pop("lds"))}
    plan["constants"] = {k: (float(v) if k == "znear" else int(v)) for k, v in kv.items()}
    plan["text"] = text
    return plan


def workspace_read(name: str, shape, dtype=torch.bfloat16, device: Optional[int] = None) -> torch.Tensor:
    """the head of the context workspace `name` ("vit.x", "clip.qkv", ...: what the last tower forward left there) as a host tensor of
    `shape` and `dtype` (fp_op_workspace_read); raises when the context has no such workspace or it is shorter"""
    out = torch.empty(tuple(int(v) for v in shape), dtype=dtype)
    if out.numel():
        check(_lib.load().fp_op_workspace_read(context(device), name.encode(), ptr(out), out.numel() * out.element_size()), "fp_op_workspace_read")
    return out


ATTN_QSCALE = 1.4426950408889634 / 8.0   # log2(e) / sqrt(64): what q_prescaled=True expects the q columns to carry


def attention(qk: torch.Tensor, vt: torch.Tensor, n_tok: int, out: Optional[torch.Tensor] = None, q_prescaled: bool = False) -> torch.Tensor:
    """qk bf16 [B*npad, 2*H*64], vt bf16 [B,H,64,npad] -> o bf16 [B*npad, H*64].  q_prescaled: the q columns already hold
    q * ATTN_QSCALE (what the ViT's LayerNorm-folded qkv layer produces)"""
    lib = _lib.load()
    qk, vt = _dev(qk, torch.bfloat16), _dev(vt, torch.bfloat16)
    B, H, _, npad = vt.shape
    if out is None:
        out = torch.zeros((B * npad, H * 64), dtype=torch.bfloat16, device=qk.device)
    check(lib.fp_op_attention(ptr(qk), 2 * H * 64, ptr(vt), ptr(out), H * 64, B, H, n_tok, npad, int(bool(q_prescaled)), current_stream()),
          "fp_op_attention")
    return out


def _attention_qkv(entry_name: str, qkv: torch.Tensor, heads: int, n_tok: int, scale: Optional[float], out: Optional[torch.Tensor]) -> torch.Tensor:
    """attention_hd / attention_causal: the C entry fp_op_<entry_name> on the [q | k | v] rows"""
    lib = _lib.load()
    qkv = _dev(qkv, torch.bfloat16)
    if qkv.dim() != 3 or qkv.shape[2] % (3 * heads) != 0:
        raise ValueError(f"{entry_name}: qkv of shape {tuple(qkv.shape)} ([B, npad, 3*heads*hd]) with heads={heads}")
    B, npad, w3 = qkv.shape
    width = w3 // 3
    hd = width // heads
    if out is None:
        out = torch.zeros((B, npad, width), dtype=torch.bfloat16, device=qkv.device)
    else:
        assert out.dtype == torch.bfloat16 and out.is_cuda and tuple(out.shape) == (B, npad, width)
        assert out.stride(2) == 1 and out.stride(0) == npad * out.stride(1)
    sc = float(scale) if scale is not None else 1.0 / float(np.sqrt(hd))
    entry = "fp_op_" + entry_name
    check(getattr(lib, entry)(ptr(qkv), w3, ptr(out), int(out.stride(1)), B, heads, hd, int(n_tok), npad, sc, current_stream()), entry)
    return out


def attention_hd(qkv: torch.Tensor, heads: int, n_tok: int, scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attention for any head dimension (a multiple of 8 up to 128) on the plain output of one bias GEMM (fp_op_attention_hd):
    qkv bf16 [B, npad, 3*heads*hd], columns [q | k | v] (nn.MultiheadAttention's in_proj order) -> o bf16 [B, npad, heads*hd], the
    softmax running over the first n_tok tokens of each crop.  scale defaults to 1/sqrt(hd).  `out`: optional bf16 [B, npad, width]
    whose rows are contiguous B*npad and whose row stride may exceed the width (a column slice of a wider buffer)."""
    return _attention_qkv("attention_hd", qkv, heads, n_tok, scale, out)


def attention_causal(qkv: torch.Tensor, heads: int, n_tok: int, scale: Optional[float] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attention_hd under a causal mask (fp_op_attention_causal, the attention of the CLIP text tower): the same arguments and layout;
    token t attends to the tokens 0 .. t of its prompt."""
    return _attention_qkv("attention_causal", qkv, heads, n_tok, scale, out)


def knn_l2(table: torch.Tensor, queries: torch.Tensor, k: int):
    """exact k nearest rows of `table` f32 [N,E] for each row of `queries` f32 [Q,E] in Euclidean distance (fp_knn_l2; the brute-force
    form of scipy.spatial.KDTree(table).query(queries, k)) -> (idx i32 [Q,k], squared distances f32 [Q,k]) ordered by (distance
    ascending, row index ascending)"""
    lib = _lib.load()
    t, q = _dev(torch.as_tensor(table), torch.float32), _dev(torch.as_tensor(queries), torch.float32)
    if t.dim() != 2 or q.dim() != 2 or t.shape[1] != q.shape[1]:
        raise ValueError(f"knn_l2: table {tuple(t.shape)} and queries {tuple(q.shape)} ([N,E] and [Q,E])")
    N, E = t.shape
    Q = q.shape[0]
    idx = torch.empty((Q, int(k)), dtype=torch.int32, device=t.device)
    d2 = torch.empty((Q, int(k)), dtype=torch.float32, device=t.device)
    if Q > 0:
        check(lib.fp_knn_l2(context(), ptr(t), N, E, ptr(q), Q, int(k), ptr(idx), ptr(d2), current_stream()), "fp_knn_l2")
    return idx, d2


# ---- CLIP image tower (csrc/clip.hip) -----------------------------------------------------------------
CLIP_ARCHS = {
    # name: (width, depth, heads, mlp_dim, embed_dim, patch, grid) — open_clip's model configs (public); all use the exact-erf GELU
    "ViT-bigG-14": (1664, 48, 16, 8192, 1280, 14, 16),
    "ViT-H-14": (1280, 32, 16, 5120, 1024, 14, 16),
    "ViT-L-14": (1024, 24, 16, 4096, 768, 14, 16),
    # test towers: depth 2, head dimensions 64 / 80 / 104, at 224^2 (257 tokens) and 56^2 (17 tokens); one bigG-wide block
    "tiny-64": (128, 2, 2, 512, 64, 14, 16), "tiny-80": (320, 2, 4, 640, 64, 14, 16), "tiny-104": (832, 2, 8, 1024, 64, 14, 16),
    "tiny-64-s56": (128, 2, 2, 512, 64, 14, 4), "tiny-80-s56": (320, 2, 4, 640, 64, 14, 4), "tiny-104-s56": (832, 2, 8, 1024, 64, 14, 4),
    "tiny-bigG-wide": (1664, 1, 16, 128, 1280, 14, 4),
}


def _resblock_names(width: int, mlp: int, depth: int) -> dict:
    """open_clip's transformer.resblocks.<i>.* name -> shape, block by block (both towers; the order is the one the seeded random
    state dicts draw in)"""
    names = {}
    for i in range(depth):
        p = f"transformer.resblocks.{i}."
        names.update({p + "ln_1.weight": (width,), p + "ln_1.bias": (width,), p + "attn.in_proj_weight": (3 * width, width),
                      p + "attn.in_proj_bias": (3 * width,), p + "attn.out_proj.weight": (width, width), p + "attn.out_proj.bias": (width,),
                      p + "ln_2.weight": (width,), p + "ln_2.bias": (width,), p + "mlp.c_fc.weight": (mlp, width), p + "mlp.c_fc.bias": (mlp,),
                      p + "mlp.c_proj.weight": (width, mlp), p + "mlp.c_proj.bias": (width,)})
    return names


class _ClipTower:
    """what ClipVisual and ClipText share: registering a state dict with the library and releasing the handle.  A subclass names its
    tower (_WHAT, in the error text), its name table (_names) and its C entries (_SET_WEIGHT, _DESTROY)"""

    def load_state_dict(self, sd: dict):
        s = current_stream()
        want = self._names(self.model_name)
        missing = sorted(set(want) - set(sd))
        if missing:
            raise KeyError(f"{self._WHAT} state dict lacks {len(missing)} tensors, e.g. {missing[:3]}")
        set_weight = getattr(self.lib, self._SET_WEIGHT)
        for name in want:
            w = _dev(torch.as_tensor(sd[name]), torch.bfloat16)
            self.weights[name] = w  # keep alive: the library stores raw pointers
            check(set_weight(self.handle, name.encode(), ptr(w), w.numel(), s), f"set_weight({name})")
        torch.cuda.synchronize()

    def __del__(self):
        try:
            getattr(self.lib, self._DESTROY)(self.handle)
        except Exception:
            pass


def clip_state_dict_names(model_name: str) -> dict:
    """open_clip visual state-dict name -> shape"""
    width, depth, heads, mlp, embed, patch, grid = CLIP_ARCHS[model_name]
    names = {"conv1.weight": (width, 3, patch, patch), "class_embedding": (width,), "positional_embedding": (1 + grid * grid, width),
             "ln_pre.weight": (width,), "ln_pre.bias": (width,), "ln_post.weight": (width,), "ln_post.bias": (width,), "proj": (width, embed)}
    names.update(_resblock_names(width, mlp, depth))
    return names


def random_clip_state_dict(model_name: str, seed: int = 0) -> dict:
    """seeded random-init weights under open_clip's visual state-dict names (no checkpoint offline): trunc-normal linears,
    LayerNorm (1 + noise, noise)"""
    width = CLIP_ARCHS[model_name][0]
    g = torch.Generator().manual_seed(seed)

    def tn(shape, std=0.02):
        return torch.nn.init.trunc_normal_(torch.empty(*shape), std=std, a=-2 * std, b=2 * std, generator=g)

    sd = {}
    for name, shape in clip_state_dict_names(model_name).items():
        if name.endswith(("ln_pre.weight", "ln_post.weight", "ln_1.weight", "ln_2.weight")):
            sd[name] = torch.ones(shape) + tn(shape, std=0.05)
        elif name == "proj":
            sd[name] = tn(shape, std=width ** -0.5)
        else:
            sd[name] = tn(shape)
    return {k: v.to(torch.bfloat16) for k, v in sd.items()}


class ClipVisual(_ClipTower):
    """Device-resident CLIP image tower (open_clip visual state-dict layout) driving fp_clip_encode_image."""
    _WHAT, _names, _SET_WEIGHT, _DESTROY = "CLIP", staticmethod(clip_state_dict_names), "fp_clip_set_weight", "fp_clip_destroy"

    def __init__(self, model_name: str = "ViT-bigG-14", state_dict: Optional[dict] = None, seed: int = 0, device: Optional[int] = None,
                 quick_gelu: bool = False):
        if model_name not in CLIP_ARCHS:
            raise ValueError(f"unknown CLIP model {model_name}")
        self.width, self.depth, self.heads, self.mlp_dim, self.embed_dim, self.patch, self.grid = CLIP_ARCHS[model_name]
        self.model_name = model_name
        self.image_size = self.patch * self.grid
        self.lib = _lib.load()
        self.ctx = context(device)
        arch = _lib.ClipArch(self.width, self.depth, self.heads, self.mlp_dim, self.patch, self.grid, self.embed_dim, 1e-5, int(bool(quick_gelu)))
        h = C.c_void_p()
        check(self.lib.fp_clip_create(self.ctx, C.byref(arch), C.byref(h)), "fp_clip_create")
        self.handle = h
        self.weights = {}
        self.load_state_dict(state_dict if state_dict is not None else random_clip_state_dict(model_name, seed))

    def encode_image(self, images: torch.Tensor) -> torch.Tensor:
        """bf16 [B,3,S,S] in [0,1] -> bf16 [B, embed_dim]"""
        x = _dev(images, torch.bfloat16)
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise ValueError(f"CLIP images of shape {tuple(x.shape)} ([B,3,S,S])")
        B, S = x.shape[0], x.shape[2]
        out = torch.empty((B, self.embed_dim), dtype=torch.bfloat16, device=x.device)
        if B > 0:
            check(self.lib.fp_clip_encode_image(self.handle, ptr(x), B, S, ptr(out), current_stream()), "fp_clip_encode_image")
        return out

    __call__ = encode_image

    def flops(self, B: int) -> float:
        return float(self.lib.fp_clip_flops(self.handle, int(B)))


# ---- CLIP text tower (csrc/clip_text.hip) -------------------------------------------------------------
CLIP_TEXT_ARCHS = {
    # name: (width, depth, heads, mlp_dim, vocab, ctx, embed_dim) — the text half of open_clip's model configs (public); keyed by the
    # name of the image tower it belongs to, head dimension 64 throughout
    "ViT-bigG-14": (1280, 32, 20, 5120, 49408, 77, 1280),
    "ViT-H-14": (1024, 24, 16, 4096, 49408, 77, 1024),
    "ViT-L-14": (768, 12, 12, 3072, 49408, 77, 768),
    # test towers: one per tiny image tower (its width, heads and embedding size; depth 2, 1024 tokens, 77 positions) ...
    "tiny-64": (128, 2, 2, 512, 1024, 77, 64), "tiny-80": (320, 2, 4, 640, 1024, 77, 64), "tiny-104": (832, 2, 8, 1024, 1024, 77, 64),
    "tiny-64-s56": (128, 2, 2, 512, 1024, 77, 64), "tiny-80-s56": (320, 2, 4, 640, 1024, 77, 64), "tiny-104-s56": (832, 2, 8, 1024, 1024, 77, 64),
    "tiny-bigG-wide": (1280, 2, 20, 256, 1024, 77, 1280),
    # ... a 17-position one (padded to 32 rows) and one block at ViT-bigG/14's text width
    "tiny-64-c17": (128, 2, 2, 512, 1024, 17, 64),
    "tiny-bigG-text": (1280, 1, 20, 256, 1024, 77, 1280),
}


def clip_text_state_dict_names(model_name: str) -> dict:
    """open_clip text state-dict name -> shape (the top-level names of a CLIP checkpoint)"""
    width, depth, heads, mlp, vocab, ctx, embed = CLIP_TEXT_ARCHS[model_name]
    names = {"token_embedding.weight": (vocab, width), "positional_embedding": (ctx, width), "ln_final.weight": (width,),
             "ln_final.bias": (width,), "text_projection": (width, embed)}
    names.update(_resblock_names(width, mlp, depth))
    return names


def random_clip_text_state_dict(model_name: str, seed: int = 0) -> dict:
    """seeded random-init weights under open_clip's text state-dict names (no checkpoint offline): trunc-normal linears and embeddings,
    LayerNorm (1 + noise, noise)"""
    width = CLIP_TEXT_ARCHS[model_name][0]
    g = torch.Generator().manual_seed(seed)

    def tn(shape, std=0.02):
        return torch.nn.init.trunc_normal_(torch.empty(*shape), std=std, a=-2 * std, b=2 * std, generator=g)

    sd = {}
    for name, shape in clip_text_state_dict_names(model_name).items():
        if name.endswith(("ln_final.weight", "ln_1.weight", "ln_2.weight")):
            sd[name] = torch.ones(shape) + tn(shape, std=0.05)
        elif name == "text_projection":
            sd[name] = tn(shape, std=width ** -0.5)
        elif name == "positional_embedding":
            sd[name] = tn(shape, std=0.01)
        else:
            sd[name] = tn(shape)
    return {k: v.to(torch.bfloat16) for k, v in sd.items()}


class ClipText(_ClipTower):
    """Device-resident CLIP text tower (open_clip state-dict names) driving fp_clip_text_encode."""
    _WHAT, _names, _SET_WEIGHT, _DESTROY = "CLIP text", staticmethod(clip_text_state_dict_names), "fp_clip_text_set_weight", "fp_clip_text_destroy"

    def __init__(self, model_name: str = "ViT-bigG-14", state_dict: Optional[dict] = None, seed: int = 0, device: Optional[int] = None,
                 chunk: int = 256):
        if model_name not in CLIP_TEXT_ARCHS:
            raise ValueError(f"unknown CLIP text model {model_name}")
        self.width, self.depth, self.heads, self.mlp_dim, self.vocab, self.ctx, self.embed_dim = CLIP_TEXT_ARCHS[model_name]
        self.model_name = model_name
        self.chunk = int(chunk)
        self.lib = _lib.load()
        self.ctx_handle = context(device)
        arch = _lib.ClipTextArch(self.width, self.depth, self.heads, self.mlp_dim, self.vocab, self.ctx, self.embed_dim, 1e-5)
        h = C.c_void_p()
        check(self.lib.fp_clip_text_create(self.ctx_handle, C.byref(arch), C.byref(h)), "fp_clip_text_create")
        self.handle = h
        self.weights = {}
        self.load_state_dict(state_dict if state_dict is not None else random_clip_text_state_dict(model_name, seed))

    def encode_text(self, ids: torch.Tensor, chunk: Optional[int] = None) -> torch.Tensor:
        """token ids [N, ctx] (any integer dtype) -> bf16 [N, embed_dim], `chunk` prompts per tower call (bounded workspaces; a prompt's
        embedding does not depend on the chunk it rides in).  An id outside [0, vocab) is an error."""
        ids = torch.as_tensor(ids)
        if ids.dim() != 2 or ids.shape[1] != self.ctx or ids.is_floating_point():
            raise ValueError(f"CLIP text ids of shape {tuple(ids.shape)} {ids.dtype} (integer [N, {self.ctx}])")
        x = ids.to("cuda", dtype=torch.int32).contiguous()
        step = max(1, int(chunk or self.chunk))
        out = torch.empty((x.shape[0], self.embed_dim), dtype=torch.bfloat16, device=x.device)
        for i in range(0, x.shape[0], step):
            part, dst = x[i:i + step], out[i:i + step]
            check(self.lib.fp_clip_text_encode(self.handle, ptr(part), part.shape[0], ptr(dst), current_stream()), "fp_clip_text_encode")
        return out

    __call__ = encode_text

    def flops(self, B: int) -> float:
        return float(self.lib.fp_clip_text_flops(self.handle, int(B)))


def im2col_norm(images: torch.Tensor, ps: int = 14, kp: Optional[int] = None) -> torch.Tensor:
    """bf16 crops [B,3,H,W] in [0,1] -> normalised patch rows [B*(H/ps)*(W/ps), kp] (fp_op_im2col_norm; kp defaults to 3*ps*ps rounded
    up to a multiple of 64, what fp_vit_forward uses)"""
    lib = _lib.load()
    images = _dev(images, torch.bfloat16)
    B, _, H, W = images.shape
    kp = kp or (3 * ps * ps + 63) // 64 * 64
    out = torch.empty((B * (H // ps) * (W // ps), kp), dtype=torch.bfloat16, device=images.device)
    check(lib.fp_op_im2col_norm(ptr(images), ptr(out), B, H, W, ps, kp, current_stream()), "fp_op_im2col_norm")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    lib = _lib.load()
    x, gamma, beta = _dev(x, torch.bfloat16), _dev(gamma, torch.bfloat16), _dev(beta, torch.bfloat16)
    rows, D = x.shape
    y = torch.empty_like(x)
    check(lib.fp_op_layernorm(ptr(x), ptr(y), ptr(gamma), ptr(beta), rows, D, float(eps), current_stream()), "fp_op_layernorm")
    return y


def layernorm_rows(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-6, rows: Optional[int] = None,
                   rows_per_b: int = 0, in_stride_b: int = 0, in_off: int = 0, l2_normalize: bool = False) -> torch.Tensor:
    """fp_op_layernorm_rows on x bf16 [n, D]: `rows` output rows (default n), output row r from input row
    (r // rows_per_b) * in_stride_b + in_off + r % rows_per_b (rows_per_b 0: row r); l2_normalize: every row F.normalize()d"""
    lib = _lib.load()
    x, gamma, beta = _dev(x, torch.bfloat16), _dev(gamma, torch.bfloat16), _dev(beta, torch.bfloat16)
    n, D = x.shape
    rows = n if rows is None else int(rows)
    if rows_per_b > 0 and rows > 0:
        nb = (rows - 1) // rows_per_b                      # the last, possibly partial, batch; the one before it is whole
        last = nb * in_stride_b + in_off + (rows - 1) % rows_per_b
        whole = (nb - 1) * in_stride_b + in_off + rows_per_b - 1 if nb else 0
        assert min(in_stride_b, in_off) >= 0 and max(last, whole) < n, f"layernorm_rows: the gather reads past row {n - 1}"
    else:
        assert rows <= n
    context()
    y = torch.empty((rows, D), dtype=torch.bfloat16, device=x.device)
    check(lib.fp_op_layernorm_rows(ptr(x), ptr(y), ptr(gamma), ptr(beta), rows, D, float(eps), int(rows_per_b), int(in_stride_b), int(in_off),
                                   int(bool(l2_normalize)), current_stream()), "fp_op_layernorm_rows")
    return y


def posembed_aa(grid: torch.Tensor, gh: int, gw: int) -> torch.Tensor:
    """grid bf16 [G*G, D] -> [gh*gw, D]: the bicubic antialiased resize of the ViT's position embedding (fp_op_posembed_aa)"""
    lib = _lib.load()
    grid = _dev(grid, torch.bfloat16)
    n, D = grid.shape
    G = int(round(n ** 0.5))
    assert G * G == n, f"posembed_aa: {n} rows are no square grid"
    context()
    out = torch.empty((gh * gw, D), dtype=torch.bfloat16, device=grid.device)
    check(lib.fp_op_posembed_aa(ptr(grid), ptr(out), G, int(gh), int(gw), D, current_stream()), "fp_op_posembed_aa")
    return out


def token_init(x: torch.Tensor, cls: torch.Tensor, pos0: torch.Tensor, reg: Optional[torch.Tensor], n_tok: int) -> torch.Tensor:
    """in place on the token buffer x bf16 [B, npad, D] (contiguous, on the device): row 0 = cls + pos0, rows 1..nreg = reg [nreg, D],
    rows [n_tok, npad) = 0 (fp_op_token_init)"""
    lib = _lib.load()
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 3
    B, npad, D = x.shape
    cls, pos0 = _dev(cls, torch.bfloat16).reshape(-1), _dev(pos0, torch.bfloat16).reshape(-1)
    nreg = 0 if reg is None else int(reg.shape[0])
    reg = _dev(reg, torch.bfloat16) if nreg else None
    assert cls.numel() == D and pos0.numel() == D and (reg is None or tuple(reg.shape) == (nreg, D))
    context()
    check(lib.fp_op_token_init(ptr(x), ptr(cls), ptr(pos0), ptr(reg), nreg, B, int(n_tok), npad, D, current_stream()), "fp_op_token_init")
    return x


def row_stats(x: torch.Tensor, eps: float = 1e-6):
    """statistics of the folded LayerNorm from the rows x bf16 [rows, D] (fp_op_row_stats): (records i32 [rows, 4], rstd f32 [rows]);
    a record is bf16 {sh, sl, sh, -mh, -ml, -mh, 0, 0}: sigma = sh + sl, mean = -(mh + ml)"""
    lib = _lib.load()
    x = _dev(x, torch.bfloat16)
    rows, D = x.shape
    context()
    rec = torch.empty((rows, 4), dtype=torch.int32, device=x.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device)
    check(lib.fp_op_row_stats(ptr(x), rows, D, float(eps), ptr(rec), ptr(rstd), current_stream()), "fp_op_row_stats")
    return rec, rstd


def stats_finalize(part: torch.Tensor, rows: int, eps: float = 1e-6):
    """the same from partial sums part f32 [D / 64, part_ld, 2] = (sum x, sum x^2) per 64-column block, part_ld >= rows
    (fp_op_stats_finalize): (records i32 [rows, 4], rstd f32 [rows])"""
    lib = _lib.load()
    part = _dev(part, torch.float32)
    nb, part_ld, two = part.shape
    assert two == 2 and part_ld >= rows
    context()
    rec = torch.empty((rows, 4), dtype=torch.int32, device=part.device)
    rstd = torch.empty((rows,), dtype=torch.float32, device=part.device)
    check(lib.fp_op_stats_finalize(ptr(part), int(rows), nb * 64, float(eps), part_ld, ptr(rec), ptr(rstd), current_stream()),
          "fp_op_stats_finalize")
    return rec, rstd


def ln_fold(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: torch.Tensor, n_scaled: int = 0, row_scale: float = 1.0):
    """the weight side of the folded LayerNorm (fp_op_ln_fold): (Wf bf16 [N, K], records i32 [N, 4] = bf16 {b'h, b'h, b'l, ch, ch, cl, 0, 0})"""
    lib = _lib.load()
    w, bias = _dev(w, torch.bfloat16), _dev(bias, torch.bfloat16)
    gamma, beta = _dev(gamma, torch.bfloat16), _dev(beta, torch.bfloat16)
    N, K = w.shape
    assert gamma.numel() == K and beta.numel() == K and bias.numel() == N
    context()
    wf = torch.empty_like(w)
    cb = torch.empty((N, 4), dtype=torch.int32, device=w.device)
    check(lib.fp_op_ln_fold(ptr(w), ptr(gamma), ptr(beta), ptr(bias), N, K, int(n_scaled), float(row_scale), ptr(wf), ptr(cb),
                            current_stream()), "fp_op_ln_fold")
    return wf, cb


def transpose(x: torch.Tensor) -> torch.Tensor:
    """x bf16 [rows, cols] -> [cols, rows] (fp_op_transpose)"""
    lib = _lib.load()
    x = _dev(x, torch.bfloat16)
    rows, cols = x.shape
    context()
    out = torch.empty((cols, rows), dtype=torch.bfloat16, device=x.device)
    check(lib.fp_op_transpose(ptr(x), ptr(out), rows, cols, current_stream()), "fp_op_transpose")
    return out


def plan_vit_batches(n: int, n_tok: int, max_batch: int = 192, n_cu: int = 256) -> list:
    return list(_plan_vit_batches(int(n), int(n_tok), int(max_batch), int(n_cu)))


@functools.lru_cache(maxsize=256)
def _plan_vit_batches(n: int, n_tok: int, max_batch: int, n_cu: int) -> tuple:
    """Split n crops into ViT batches whose GEMM grids fill whole rounds of the resident (one workgroup per CU) grid.

    The persistent GEMM walks 256x256 tiles with one workgroup per CU; a batch of b crops has ceil(b*npad/256) tile rows,
    and the narrowest linear layers (N = 1024: 4 tile columns) are the ones whose last partial round costs the most.
    Dynamic programme over batch sizes in [max_batch/2, max_batch + max_batch/8]: minimise the total number of rounds,
    then the number of batches.  Host-side policy only — results do not depend on the split.
    """
    if n <= 0:
        return ()
    npad = (n_tok + 15) // 16 * 16
    lo, hi = max(1, max_batch // 2), max_batch + max(1, max_batch // 8)

    def rounds(b):
        return -(-(-(-b * npad // 256) * 4) // n_cu)

    if n <= hi:
        return (n,)
    INF = (1 << 60, 1 << 60)
    best = [INF] * (n + 1)
    back = [0] * (n + 1)
    best[0] = (0, 0)
    for m in range(1, n + 1):
        for b in range(lo, min(hi, m) + 1):
            prev = best[m - b]
            if prev == INF:
                continue
            cand = (prev[0] + rounds(b), prev[1] + 1)
            if cand < best[m]:
                best[m], back[m] = cand, b
    if best[n] == INF:            # n below 2*lo: one batch or an even split
        return (n,) if n <= hi else (n // 2, n - n // 2)
    out, m = [], n
    while m > 0:
        out.append(back[m])
        m -= back[m]
    return tuple(sorted(out, reverse=True))


class Timer:
    """HIP-event timer on the current stream (bench.py)."""

    def __init__(self):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.fp_timer_create(C.byref(h)))
        self.h = h

    def start(self):
        check(self.lib.fp_timer_start(self.h, current_stream()))

    def stop(self):
        check(self.lib.fp_timer_stop(self.h, current_stream()))

    def elapsed_ms(self) -> float:
        ms = C.c_float()
        check(self.lib.fp_timer_elapsed_ms(self.h, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            self.lib.fp_timer_destroy(self.h)
        except Exception:
            pass
