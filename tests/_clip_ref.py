"""References of the CLIP image tower and of GPT4ScaleEstimator for the tests (not a test module).

  clip_forward        the tower restated in torch (fp32 or fp64) from open_clip's public VisionTransformer structure; `rnd` is applied at
                      every module boundary (identity: the exact forward; `bf16_round`: the rounding points of a module cast to bf16)
  hf_name_map / to_hf open_clip visual names -> transformers.CLIPVisionModelWithProjection names (the fused in_proj splits into q, k, v)
  hf_model            a CLIPVisionModelWithProjection (hidden_act='gelu') carrying an open_clip-named state dict
  gpt4_scale_ref      float64 restatement of GPT4ScaleEstimator.estimate (reference scale_estimators.py:50-80) from the embeddings on
"""
from __future__ import annotations

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def normalize_bf16(images: torch.Tensor) -> torch.Tensor:
    """torchvision Normalize on a bf16 tensor (clip.py:12,17): bf16 mean / std, subtract (rounded), divide (rounded)"""
    x = images.to(torch.bfloat16)
    mean = torch.tensor(CLIP_MEAN).to(torch.bfloat16).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD).to(torch.bfloat16).view(1, 3, 1, 1)
    return (x - mean) / std


def clip_forward(sd: dict, x_norm: torch.Tensor, heads: int, eps: float = 1e-5, rnd=lambda t: t, dtype=torch.float32) -> torch.Tensor:
    """sd: open_clip visual names; x_norm: normalised images [B,3,S,S] -> [B, embed_dim]"""
    F = torch.nn.functional
    w = {k: v.to(dtype) for k, v in sd.items()}
    x = x_norm.to(dtype)
    width = w["class_embedding"].numel()
    ps = w["conv1.weight"].shape[-1]
    depth = 1 + max(int(k.split(".")[2]) for k in w if k.startswith("transformer.resblocks."))
    x = rnd(F.conv2d(x, w["conv1.weight"], stride=ps))                       # [B, width, g, g]
    B = x.shape[0]
    x = x.reshape(B, width, -1).permute(0, 2, 1)
    x = torch.cat([w["class_embedding"].view(1, 1, width).expand(B, -1, -1), x], dim=1)
    x = rnd(x + w["positional_embedding"])
    x = rnd(F.layer_norm(x, (width,), w["ln_pre.weight"], w["ln_pre.bias"], eps))
    hd = width // heads
    for i in range(depth):
        p = f"transformer.resblocks.{i}."
        y = rnd(F.layer_norm(x, (width,), w[p + "ln_1.weight"], w[p + "ln_1.bias"], eps))
        qkv = rnd(y @ w[p + "attn.in_proj_weight"].t() + w[p + "attn.in_proj_bias"])
        q, k, v = (t.reshape(B, -1, heads, hd).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
        a = torch.softmax(q @ k.transpose(-1, -2) / float(np.sqrt(hd)), dim=-1) @ v
        a = rnd(a.permute(0, 2, 1, 3).reshape(B, -1, width))
        x = rnd(x + rnd(a @ w[p + "attn.out_proj.weight"].t() + w[p + "attn.out_proj.bias"]))
        y = rnd(F.layer_norm(x, (width,), w[p + "ln_2.weight"], w[p + "ln_2.bias"], eps))
        hmid = rnd(F.gelu(rnd(y @ w[p + "mlp.c_fc.weight"].t() + w[p + "mlp.c_fc.bias"])))
        x = rnd(x + rnd(hmid @ w[p + "mlp.c_proj.weight"].t() + w[p + "mlp.c_proj.bias"]))
    pooled = rnd(F.layer_norm(x[:, 0], (width,), w["ln_post.weight"], w["ln_post.bias"], eps))
    return rnd(pooled @ w["proj"])


def hf_name_map(depth: int) -> dict:
    """open_clip visual name -> list of (HF name, row slice index or None, transposed)"""
    v = "vision_model."
    m = {"conv1.weight": [(v + "embeddings.patch_embedding.weight", None, False)],
         "class_embedding": [(v + "embeddings.class_embedding", None, False)],
         "positional_embedding": [(v + "embeddings.position_embedding.weight", None, False)],
         "ln_pre.weight": [(v + "pre_layrnorm.weight", None, False)], "ln_pre.bias": [(v + "pre_layrnorm.bias", None, False)],
         "ln_post.weight": [(v + "post_layernorm.weight", None, False)], "ln_post.bias": [(v + "post_layernorm.bias", None, False)],
         "proj": [("visual_projection.weight", None, True)]}
    for i in range(depth):
        o, h = f"transformer.resblocks.{i}.", f"{v}encoder.layers.{i}."
        for s in ("weight", "bias"):
            m[o + f"ln_1.{s}"] = [(h + f"layer_norm1.{s}", None, False)]
            m[o + f"ln_2.{s}"] = [(h + f"layer_norm2.{s}", None, False)]
            m[o + f"attn.in_proj_{s}"] = [(h + f"self_attn.{n}_proj.{s}", j, False) for j, n in enumerate("qkv")]
            m[o + f"attn.out_proj.{s}"] = [(h + f"self_attn.out_proj.{s}", None, False)]
            m[o + f"mlp.c_fc.{s}"] = [(h + f"mlp.fc1.{s}", None, False)]
            m[o + f"mlp.c_proj.{s}"] = [(h + f"mlp.fc2.{s}", None, False)]
    return m


def to_hf(sd: dict, depth: int) -> dict:
    out = {}
    for name, targets in hf_name_map(depth).items():
        t = sd[name]
        for hf, part, transposed in targets:
            u = t if part is None else t.chunk(3, dim=0)[part]
            out[hf] = (u.t() if transposed else u).contiguous().clone()
    return out


def hf_model(sd: dict, width, depth, heads, mlp_dim, embed_dim, patch, grid, eps=1e-5):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = CLIPVisionConfig(hidden_size=width, intermediate_size=mlp_dim, num_hidden_layers=depth, num_attention_heads=heads,
                           image_size=patch * grid, patch_size=patch, projection_dim=embed_dim, hidden_act="gelu", layer_norm_eps=eps)
    model = CLIPVisionModelWithProjection(cfg).eval()
    hf = to_hf({k: v.float() for k, v in sd.items()}, depth)
    missing, unexpected = model.load_state_dict(hf, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return model


def knn_f64(table, queries, k):
    """brute-force nearest rows in float64, ordered by (distance, index): (idx [Q,k], d2 [Q,N])"""
    t, q = np.asarray(table, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    d2 = ((q[:, None, :] - t[None, :, :]) ** 2).sum(-1)
    idx = np.stack([np.lexsort((np.arange(t.shape[0]), row))[:k] for row in d2])
    return idx, d2


def gpt4_scale_ref(feats, table, scales, query_k, depth_scales=None):
    """reference :66-80 in float64 from the normalised embeddings on: -> (scales / 2, neighbour indices, per-crop table scales)"""
    idx, _ = knn_f64(table, feats, query_k)
    s = np.asarray(scales, dtype=np.float64)[idx]
    if query_k == 1:
        chat = s[:, 0]
    else:
        chat = np.sort(s, axis=1)[:, (query_k - 1) // 2]          # torch's median: the lower middle value for even k
    if depth_scales is not None:
        ds = np.asarray(depth_scales, dtype=np.float64)
        out = ds * np.median(chat / ds)
    else:
        out = chat
    return out / 2.0, idx, chat
