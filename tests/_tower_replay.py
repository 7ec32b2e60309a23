"""The three transformer forwards replayed one kernel-level op at a time (not a test module).

Each replay is written from the MODEL definition — oracle/vit_ref.py (hub DINOv2 with registers), tests/_clip_ref.py and
tests/_clip_text_ref.py (open_clip's image and text transformers) — on the layouts the kernels work in: token buffers of npad = 16 *
ceil(n_tok / 16) rows per crop, the q | k columns and the per-head transposed V of the ViT's attention, the [q | k | v] rows of the CLIP
attention.  Every arithmetic step is one op of freepose_amd.ops (each has exact-answer tests of its own); plain torch only moves bf16
values (zero-padding, slicing, picking rows), adds two bf16 tensors, or applies torchvision's Normalize to a bf16 image.  The drivers
(fp_vit_forward, fp_clip_encode_image, fp_clip_text_encode) are held to these replays bit for bit by tests/test_gpu_tower_replay.py.

  replay_vit / replay_clip_visual / replay_clip_text   -> (output, {workspace name of the driver: buffer after the last block})
  massive_state_dict                                   ViT weights under which every parameter is observable
  fault=                                               ONE wiring fault injected into the replay (FAULTS_*): the self-test of the inputs
"""
from __future__ import annotations

import numpy as np
import torch

LN_EPS_VIT = 1e-6
LN_EPS_CLIP = 1e-5
BIG_MIN_TILES = 192      # csrc/gemm_plan.h: fewer 256 x 256 tiles than this never run on the big tile tier

FAULTS_VIT = ("ls_swapped", "ls_ignored", "ln_eps_1e-5", "pos_shifted", "grid_transposed", "tok_off_no_registers", "ln1_records_stale",
              "last_block_sums_stale", "vt_records_from_rows", "q_scaled_twice")
FAULTS_CLIP = ("ln_pre_post_swapped",)
FAULTS_TEXT = ("pool_last_maximum",)


def cdiv(a, b):
    return -(-a // b)


def sums_stay_pending(M: int, N: int) -> bool:
    """the driver's rule for a consumer of width N on M rows: the producer's partial sums ride along with the consumer launch (the small
    tile tiers finalise them in their prologue) iff the launch cannot reach the big tier; otherwise their own kernel runs first"""
    return cdiv(M, 256) * cdiv(N, 256) < BIG_MIN_TILES


def massive_state_dict(model, seed):
    """random-init weights bent towards what trained DINOv2-reg checkpoints look like (parity caveat i): a few residual
    channels carry activations hundreds of times the typical magnitude at the CLS / register tokens and at a handful of patch
    positions, LayerNorm gains span an order of magnitude with non-zero shifts, LayerScale gammas are small and uneven."""
    from freepose_amd import ops
    sd = {k: v.float() for k, v in ops.random_state_dict(model, seed=seed).items()}
    g = torch.Generator().manual_seed(seed + 100)
    dim = sd["norm.weight"].numel()
    big = [5, dim // 3, dim - 7]
    sd["cls_token"][..., big[0]] += 90.0
    if "register_tokens" in sd:
        sd["register_tokens"][..., big[1]] += 160.0
        sd["register_tokens"][:, :2, big[2]] -= 70.0
    sd["pos_embed"][:, 40:44, big[1]] += 220.0            # a few patch tokens with a massive channel
    sd["pos_embed"][:, 300:302, big[0]] -= 130.0
    for k in list(sd):
        if k.endswith("norm1.weight") or k.endswith("norm2.weight") or k == "norm.weight":
            sd[k] = torch.exp(torch.empty(dim).uniform_(-1.2, 1.0, generator=g))
        elif k.endswith("norm1.bias") or k.endswith("norm2.bias") or k == "norm.bias":
            sd[k] = torch.empty(dim).uniform_(-0.5, 0.5, generator=g)
        elif k.endswith("gamma"):
            sd[k] = torch.exp(torch.empty(dim).uniform_(-4.0, 0.0, generator=g))
    return {k: v.to(torch.bfloat16) for k, v in sd.items()}


def smooth_images(B, H, W, seed):
    """smooth-ish synthetic crops in [0,1] (pure white noise would be a degenerate ViT input), bf16 [B,3,H,W]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    low = rng.random((B, 3, max(H // 14, 1), max(W // 14, 1))).astype(np.float32)
    img = torch.nn.functional.interpolate(torch.from_numpy(low), size=(H, W), mode="bilinear")
    img = 0.8 * img + 0.2 * torch.from_numpy(rng.random((B, 3, H, W)).astype(np.float32))
    return img.to(torch.bfloat16)


def _dev(t, dtype=torch.bfloat16):
    return torch.as_tensor(t).to("cuda", dtype=dtype).contiguous()


def _unfold(x, ps, kp):
    """normalised images bf16 [B,3,H,W] -> the patch GEMM's A operand [B * gh * gw, kp], k = c * ps^2 + dy * ps + dx, zero columns behind"""
    B, _, H, W = x.shape
    p = x.unfold(2, ps, ps).unfold(3, ps, ps).permute(0, 2, 3, 1, 4, 5).reshape(B * (H // ps) * (W // ps), 3 * ps * ps)
    out = torch.zeros((p.shape[0], kp), dtype=torch.bfloat16, device=x.device)
    out[:, :3 * ps * ps] = p
    return out


def _pad_patch_weight(w, kp):
    """Conv2d weight [D,3,ps,ps] -> the zero-padded [D, kp] matrix of the patch GEMM"""
    D = w.shape[0]
    out = torch.zeros((D, kp), dtype=torch.bfloat16, device=w.device)
    out[:, :w[0].numel()] = w.reshape(D, -1)
    return out


# ---- DINOv2 ViT ------------------------------------------------------------------------------------------------------------------------
def replay_vit(sd, images, layer, feature_type, ln_fused, route=None, fault=None):
    """hub DINOv2-reg forward (oracle/vit_ref.vit_forward) on kernel-level ops.  ln_fused: LayerNorm 1 / 2 folded into the qkv / fc1
    GEMMs (statistics handed from the producing GEMM's epilogue to the consumer) or the separate LayerNorm kernel.  route: None = per
    consumer by sums_stay_pending, 0 / 1 = fp_op_ln_chain's route for every chain.  Returns (features, buffers)."""
    from freepose_amd import ops
    assert fault is None or fault in FAULTS_VIT, fault
    w = {k: _dev(v) for k, v in sd.items() if k != "mask_token"}
    img = _dev(images)
    D = w["cls_token"].shape[-1]
    heads, ps = D // 64, w["patch_embed.proj.weight"].shape[-1]
    n_reg = w["register_tokens"].shape[1] if "register_tokens" in w else 0
    depth = 1 + max(int(k.split(".")[1]) for k in w if k.startswith("blocks."))
    G = int(round((w["pos_embed"].shape[1] - 1) ** 0.5))
    B, _, H, W = img.shape
    gh, gw = H // ps, W // ps
    P, n_tok = gh * gw, gh * gw + 1 + n_reg
    npad = cdiv(n_tok, 16) * 16
    M = B * npad
    L = layer if 1 <= layer <= depth else depth      # dino.py:18-21: the break never fires for a layer outside [1, depth]
    eps = 1e-5 if fault == "ln_eps_1e-5" else LN_EPS_VIT
    kp = cdiv(3 * ps * ps, 64) * 64
    bufs = {}

    # ---- prepare_tokens_with_masks: [cls + pos0 | registers | patches + pos] ---------------------------------------------------------
    pos = w["pos_embed"][0]
    if gh == G and gw == G:
        pos_patch = pos[1:].contiguous()
    elif fault == "grid_transposed":
        pos_patch = ops.posembed_aa(pos[1:], gw, gh)
    else:
        pos_patch = ops.posembed_aa(pos[1:], gh, gw)
    if fault == "pos_shifted":
        pos_patch = torch.roll(pos_patch, 1, dims=0).contiguous()
    a0 = bufs["im2col"] = ops.im2col_norm(img, ps, kp)
    x = torch.zeros((B, npad, D), dtype=torch.bfloat16, device="cuda")
    ops.token_init(x, w["cls_token"], pos[0], w["register_tokens"][0] if n_reg else None, n_tok)
    ops.gemm_patch(a0, _pad_patch_weight(w["patch_embed.proj.weight"], kp), w["patch_embed.proj.bias"], pos_patch, x,
                   1 if fault == "tok_off_no_registers" else 1 + n_reg)
    x = x.view(M, D)

    def blk(i, name):
        return w[f"blocks.{i}.{name}"]

    def ls(i, which):
        if fault == "ls_ignored":
            return torch.ones(D, dtype=torch.bfloat16, device="cuda")
        if fault == "ls_swapped":
            which = {"ls1": "ls2", "ls2": "ls1"}[which]
        return blk(i, which + ".gamma")

    def qk_w(i):
        return blk(i, "attn.qkv.weight")[:2 * D].contiguous(), blk(i, "attn.qkv.bias")[:2 * D].contiguous()

    def v_w(i):
        return blk(i, "attn.qkv.weight")[2 * D:].contiguous(), blk(i, "attn.qkv.bias")[2 * D:].contiguous()

    def rt(N):
        return int(sums_stay_pending(M, N)) if route is None else int(route)

    if ln_fused:
        # q rows of the folded weights carry log2(e) / sqrt(64): the attention kernel then takes exp2 of q.k directly
        qscale = dict(n_scaled=D, row_scale=ops.ATTN_QSCALE)
        rec, rstd = ops.row_stats(x, eps)                          # block 0: no producer ran, the statistics come from the rows
        n1 = (blk(0, "norm1.weight"), blk(0, "norm1.bias"))
        qk = ops.ln_consume(x, rec, rstd, *n1, *qk_w(0), mode=0, **qscale)
        vt = ops.ln_consume(x, rec, rstd, *n1, *v_w(0), mode=2, npad=npad, heads=heads)
        for i in range(L):
            ao = ops.attention(qk, vt, n_tok, q_prescaled=fault != "q_scaled_twice")
            # x += ls1 * proj(attn); its row sums feed LN2 inside fc1
            x, h1, rec2, rstd2 = ops.ln_chain(ao, blk(i, "attn.proj.weight"), blk(i, "attn.proj.bias"), ls(i, "ls1"), x, blk(i, "norm2.weight"),
                                              blk(i, "norm2.bias"), blk(i, "mlp.fc1.weight"), blk(i, "mlp.fc1.bias"), mode=1, route=rt(4 * D), eps=eps)
            bufs.update(qk=qk, vt=vt, ao=ao, h1=h1)
            if i + 1 == L:
                # nothing normalises the last block's output row by row inside a GEMM: a plain LayerScale + residual layer
                x = ops.gemm(h1, blk(i, "mlp.fc2.weight"), blk(i, "mlp.fc2.bias"), 2, ls(i, "ls2"), x)
                break
            # x += ls2 * fc2(h1); its row sums feed LN1 of the next block inside the qk layer, whose records V^T reads
            n1 = (blk(i + 1, "norm1.weight"), blk(i + 1, "norm1.bias"))
            prev = (rec, rstd)
            x, qk, rec, rstd = ops.ln_chain(h1, blk(i, "mlp.fc2.weight"), blk(i, "mlp.fc2.bias"), ls(i, "ls2"), x, *n1, *qk_w(i + 1), mode=0,
                                            route=rt(2 * D), eps=eps, **qscale)
            if fault == "ln1_records_stale":                       # block i + 1 normalises with the records of block i's input
                rec, rstd = prev
                qk = ops.ln_consume(x, rec, rstd, *n1, *qk_w(i + 1), mode=0, **qscale)
            if fault == "last_block_sums_stale" and i + 2 == L:    # fc2 in front of the last block emitted nothing: proj's sums are read
                rec, rstd = rec2, rstd2
                qk = ops.ln_consume(x, rec, rstd, *n1, *qk_w(i + 1), mode=0, **qscale)
            if fault == "vt_records_from_rows":
                vt = ops.ln_linear(x, *n1, *v_w(i + 1), mode=2, npad=npad, heads=heads, eps=eps)
            else:
                vt = ops.ln_consume(x, rec, rstd, *n1, *v_w(i + 1), mode=2, npad=npad, heads=heads)
    else:
        for i in range(L):
            y = ops.layernorm(x, blk(i, "norm1.weight"), blk(i, "norm1.bias"), eps)
            qk = ops.gemm(y, *qk_w(i))
            vt = ops.gemm_vt(y, *v_w(i), npad, heads)
            ao = ops.attention(qk, vt, n_tok, q_prescaled=False)
            x = ops.gemm(ao, blk(i, "attn.proj.weight"), blk(i, "attn.proj.bias"), 2, ls(i, "ls1"), x)
            y = ops.layernorm(x, blk(i, "norm2.weight"), blk(i, "norm2.bias"), eps)
            h1 = ops.gemm(y, blk(i, "mlp.fc1.weight"), blk(i, "mlp.fc1.bias"), 1)
            x = ops.gemm(h1, blk(i, "mlp.fc2.weight"), blk(i, "mlp.fc2.bias"), 2, ls(i, "ls2"), x)
            bufs.update(qk=qk, vt=vt, ao=ao, y=y, h1=h1)
    bufs["x"] = x

    # ---- final norm, then the slice of the token axis (dino.py:23-30) ------------------------------------------------------------------
    per, first = {"cls": (1, 0), "reg": (n_reg, 1), "patch": (P, 1 + n_reg), "patch_normalized": (P, 1 + n_reg)}[feature_type]
    out = ops.layernorm_rows(x, w["norm.weight"], w["norm.bias"], eps, rows=B * per, rows_per_b=per, in_stride_b=npad, in_off=first,
                             l2_normalize=feature_type == "patch_normalized")
    out = out.view(B, D) if feature_type == "cls" else out.view(B, per, D)
    torch.cuda.synchronize()
    return out, bufs


VIT_ORDER = ("im2col", "qk", "vt", "ao", "y", "h1", "x")       # forward order of the buffers a block leaves behind (y: unfused only)


# ---- CLIP towers: open_clip's resblocks ------------------------------------------------------------------------------------------------
def _resblocks(w, x, B, npad, n_tok, depth, heads, attention, bufs):
    """depth x { x += out_proj(attn(ln_1 x)); x += c_proj(gelu(c_fc(ln_2 x))) } on x bf16 [B * npad, D]; the last LayerNorm output, qkv,
    attention output and c_fc output go to bufs under ln / qkv / ao / h1"""
    from freepose_amd import ops
    D = x.shape[1]
    hd = D // heads
    scale = float(np.float32(1.0) / np.sqrt(np.float32(hd)))       # 1 / sqrt(head_dim) in single precision, as a C float expression gives it
    ones = torch.ones(D, dtype=torch.bfloat16, device="cuda")      # no LayerScale in CLIP
    for i in range(depth):
        p = f"transformer.resblocks.{i}."
        t = ops.layernorm(x, w[p + "ln_1.weight"], w[p + "ln_1.bias"], LN_EPS_CLIP)
        qkv = ops.gemm(t, w[p + "attn.in_proj_weight"], w[p + "attn.in_proj_bias"])
        ao = attention(qkv.view(B, npad, 3 * D), heads, n_tok, scale).view(B * npad, D)
        x = ops.gemm(ao, w[p + "attn.out_proj.weight"], w[p + "attn.out_proj.bias"], 2, ones, x)
        t = ops.layernorm(x, w[p + "ln_2.weight"], w[p + "ln_2.bias"], LN_EPS_CLIP)
        h1 = ops.gemm(t, w[p + "mlp.c_fc.weight"], w[p + "mlp.c_fc.bias"], 1)
        x = ops.gemm(h1, w[p + "mlp.c_proj.weight"], w[p + "mlp.c_proj.bias"], 2, ones, x)
        bufs.update(qkv=qkv, ao=ao, ln=t, h1=h1)
    return x


def clip_normalize(images):
    """torchvision Normalize with CLIP's constants on a bf16 tensor (clip.py:12,17): bf16 mean / std, subtract (rounded), divide (rounded)"""
    from tests._clip_ref import CLIP_MEAN, CLIP_STD
    x = images.to(torch.bfloat16)
    mean = torch.tensor(CLIP_MEAN).to(torch.bfloat16).to(x.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD).to(torch.bfloat16).to(x.device).view(1, 3, 1, 1)
    return (x - mean) / std


def replay_clip_visual(name, sd, images, fault=None):
    """open_clip VisionTransformer.forward (tests/_clip_ref.clip_forward) on kernel-level ops.  The image tower keeps its residual stream
    in the workspace `clip.y` and its LayerNorm outputs in `clip.x` (the patch GEMM fills x, ln_pre moves the stream to y)."""
    from freepose_amd import ops
    assert fault is None or fault in FAULTS_CLIP, fault
    D, depth, heads, mlp, E, ps, grid = ops.CLIP_ARCHS[name]
    w = {k: _dev(v) for k, v in sd.items()}
    img = _dev(images)
    B = img.shape[0]
    P, n_tok = grid * grid, grid * grid + 1
    npad = cdiv(n_tok, 16) * 16
    kp = cdiv(3 * ps * ps, 64) * 64
    bufs = {}
    # no kernel-level entry normalises with CLIP's constants: the two bf16 operations in torch (the test compares the driver's buffer)
    a0 = bufs["im2col"] = _unfold(clip_normalize(img), ps, kp)
    x = torch.zeros((B, npad, D), dtype=torch.bfloat16, device="cuda")
    pos = w["positional_embedding"]
    ops.token_init(x, w["class_embedding"], pos[0], None, n_tok)
    ops.gemm_patch(a0, _pad_patch_weight(w["conv1.weight"], kp), torch.zeros(D, dtype=torch.bfloat16, device="cuda"), pos[1:].contiguous(), x, 1)
    pre, post = ("ln_post", "ln_pre") if fault == "ln_pre_post_swapped" else ("ln_pre", "ln_post")
    x = ops.layernorm(x.view(B * npad, D), w[pre + ".weight"], w[pre + ".bias"], LN_EPS_CLIP)
    x = _resblocks(w, x, B, npad, n_tok, depth, heads, lambda q, h, n, s: ops.attention_hd(q, h, n, s), bufs)
    bufs["x"], bufs["y"] = bufs.pop("ln"), x
    pool = bufs["pool"] = ops.layernorm_rows(x, w[post + ".weight"], w[post + ".bias"], LN_EPS_CLIP, rows=B, rows_per_b=1, in_stride_b=npad, in_off=0)
    out = ops.gemm(pool, ops.transpose(w["proj"]), torch.zeros(E, dtype=torch.bfloat16, device="cuda"))
    torch.cuda.synchronize()
    return out, bufs


CLIP_ORDER = ("im2col", "qkv", "ao", "x", "h1", "y", "pool")


def first_maximum(ids):
    """position of the first largest id of every prompt (open_clip: text.argmax(dim=-1)), spelled out"""
    rows = torch.as_tensor(ids).tolist()
    return [r.index(max(r)) for r in rows]


def replay_clip_text(name, sd, ids, fault=None):
    """open_clip's encode_text (tests/_clip_text_ref.clip_text_forward) on kernel-level ops; buffers additionally hold `pool_at`, the pooled
    position of every prompt"""
    from freepose_amd import ops
    assert fault is None or fault in FAULTS_TEXT, fault
    D, depth, heads, mlp, vocab, ctx, E = ops.CLIP_TEXT_ARCHS[name]
    w = {k: _dev(v) for k, v in sd.items()}
    ids = torch.as_tensor(ids).long()
    B = ids.shape[0]
    assert ids.shape[1] == ctx and int(ids.min()) >= 0 and int(ids.max()) < vocab
    npad = cdiv(ctx, 16) * 16
    bufs = {}
    x = torch.zeros((B, npad, D), dtype=torch.bfloat16, device="cuda")
    x[:, :ctx] = w["token_embedding.weight"][ids.cuda()] + w["positional_embedding"][:ctx]       # one bf16 addition
    x = _resblocks(w, x.view(B * npad, D), B, npad, ctx, depth, heads, lambda q, h, n, s: ops.attention_causal(q, h, n, s), bufs)
    bufs["x"], bufs["y"] = x, bufs.pop("ln")
    at = first_maximum(ids)
    if fault == "pool_last_maximum":
        at = [ctx - 1 - r[::-1].index(max(r)) for r in ids.tolist()]
    bufs["pool_at"] = at
    pool = bufs["pool"] = x.view(B, npad, D)[torch.arange(B), torch.tensor(at)].contiguous()
    pooln = bufs["pooln"] = ops.layernorm(pool, w["ln_final.weight"], w["ln_final.bias"], LN_EPS_CLIP)
    out = ops.gemm(pooln, ops.transpose(w["text_projection"]), torch.zeros(E, dtype=torch.bfloat16, device="cuda"))
    torch.cuda.synchronize()
    return out, bufs


TEXT_ORDER = ("qkv", "ao", "y", "h1", "x", "pool", "pooln")


# ---- comparing a driver's buffers with a replay's -------------------------------------------------------------------------------------------
def first_difference(got, want):
    """None when the two bf16 tensors carry the same bits, else a description of the first differing row (2-D view: rows of the last axis)"""
    g, t = got.contiguous().view(torch.int16).cpu(), want.contiguous().view(torch.int16).cpu()
    if g.shape != t.shape:
        return f"shape {tuple(g.shape)} against {tuple(t.shape)}"
    if torch.equal(g, t):
        return None
    g2, t2 = g.reshape(-1, g.shape[-1]), t.reshape(-1, t.shape[-1])
    rows = (g2 != t2).any(dim=1).nonzero().flatten()
    r = int(rows[0])
    c = int((g2[r] != t2[r]).nonzero()[0])
    return (f"{len(rows)} of {g2.shape[0]} rows differ; first row {r}, col {c}: driver 0x{int(g2[r, c]) & 0xFFFF:04x}, "
            f"replay 0x{int(t2[r, c]) & 0xFFFF:04x}")
