"""References of the CLIP text tower and its tokenizer for the tests (not a test module).

  clip_text_forward    the tower restated in torch (fp32 or fp64) from open_clip's public TextTransformer structure; `rnd` is applied at
                       every module boundary (identity: the exact forward; `_clip_ref.bf16_round`: the rounding points of a module cast
                       to bf16)
  hf_name_map / to_hf  open_clip text names -> transformers.CLIPTextModelWithProjection names (the fused in_proj splits into q, k, v)
  hf_model             a CLIPTextModelWithProjection (hidden_act='gelu', eos_token_id = vocab - 1) carrying an open_clip-named state dict
  make_ids             [BOS, random tokens, EOS, zero padding] rows with BOS = vocab - 2 and EOS = vocab - 1, the largest id
  fixture_names        the names and sizes of tests/golden/gpt4_scale_names.json, in file order
  learn_merges         a small BPE merge list learned from those names by the plain most-frequent-pair rule (ties: the
                       lexicographically smallest pair), over the tokenizer's own word split
  write_bpe_file       such a list in the layout of open_clip's bpe_simple_vocab_16e6.txt(.gz): a header line, then `a b` per line
  hf_tokenizer         transformers.CLIPTokenizer on the vocabulary built in open_clip's order from the same merges
"""
from __future__ import annotations

import functools
import gzip
import json
from collections import Counter
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "gpt4_scale_names.json"


def clip_text_forward(sd: dict, ids: torch.Tensor, heads: int, eps: float = 1e-5, rnd=lambda t: t, dtype=torch.float32) -> torch.Tensor:
    """sd: open_clip text names; ids: integer [B, ctx] -> [B, embed_dim]"""
    F = torch.nn.functional
    w = {k: v.to(dtype) for k, v in sd.items()}
    ids = ids.long()
    B, n = ids.shape
    width = w["ln_final.weight"].numel()
    depth = 1 + max(int(k.split(".")[2]) for k in w if k.startswith("transformer.resblocks."))
    x = rnd(w["token_embedding.weight"][ids] + w["positional_embedding"][:n])
    hd = width // heads
    future = torch.triu(torch.ones((n, n), dtype=torch.bool), diagonal=1)
    for i in range(depth):
        p = f"transformer.resblocks.{i}."
        y = rnd(F.layer_norm(x, (width,), w[p + "ln_1.weight"], w[p + "ln_1.bias"], eps))
        qkv = rnd(y @ w[p + "attn.in_proj_weight"].t() + w[p + "attn.in_proj_bias"])
        q, k, v = (t.reshape(B, -1, heads, hd).permute(0, 2, 1, 3) for t in qkv.chunk(3, dim=-1))
        s = (q @ k.transpose(-1, -2) / float(np.sqrt(hd))).masked_fill(future, float("-inf"))
        a = torch.softmax(s, dim=-1) @ v
        a = rnd(a.permute(0, 2, 1, 3).reshape(B, -1, width))
        x = rnd(x + rnd(a @ w[p + "attn.out_proj.weight"].t() + w[p + "attn.out_proj.bias"]))
        y = rnd(F.layer_norm(x, (width,), w[p + "ln_2.weight"], w[p + "ln_2.bias"], eps))
        hmid = rnd(F.gelu(rnd(y @ w[p + "mlp.c_fc.weight"].t() + w[p + "mlp.c_fc.bias"])))
        x = rnd(x + rnd(hmid @ w[p + "mlp.c_proj.weight"].t() + w[p + "mlp.c_proj.bias"]))
    x = rnd(F.layer_norm(x, (width,), w["ln_final.weight"], w["ln_final.bias"], eps))      # open_clip: every row, then the index
    pooled = x[torch.arange(B), ids.argmax(dim=-1)]
    return rnd(pooled @ w["text_projection"])


def hf_name_map(depth: int) -> dict:
    """open_clip text name -> list of (HF name, row slice index or None, transposed)"""
    t = "text_model."
    m = {"token_embedding.weight": [(t + "embeddings.token_embedding.weight", None, False)],
         "positional_embedding": [(t + "embeddings.position_embedding.weight", None, False)],
         "ln_final.weight": [(t + "final_layer_norm.weight", None, False)], "ln_final.bias": [(t + "final_layer_norm.bias", None, False)],
         "text_projection": [("text_projection.weight", None, True)]}
    for i in range(depth):
        o, h = f"transformer.resblocks.{i}.", f"{t}encoder.layers.{i}."
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


def hf_model(sd: dict, width, depth, heads, mlp_dim, vocab, ctx, embed_dim, eps=1e-5):
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    cfg = CLIPTextConfig(vocab_size=vocab, hidden_size=width, intermediate_size=mlp_dim, num_hidden_layers=depth, num_attention_heads=heads,
                         max_position_embeddings=ctx, projection_dim=embed_dim, hidden_act="gelu", layer_norm_eps=eps,
                         bos_token_id=vocab - 2, eos_token_id=vocab - 1, pad_token_id=0)
    model = CLIPTextModelWithProjection(cfg).eval()
    hf = to_hf({k: v.float() for k, v in sd.items()}, depth)
    missing, unexpected = model.load_state_dict(hf, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return model


def make_ids(lengths, vocab: int, ctx: int, seed: int = 0) -> torch.Tensor:
    """one row per entry of `lengths`: BOS, that many random tokens below BOS, EOS, zeros"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros((len(lengths), ctx), dtype=torch.long)
    for i, n in enumerate(lengths):
        assert n + 2 <= ctx
        ids[i, 0] = vocab - 2
        ids[i, 1:1 + n] = torch.randint(1, vocab - 2, (n,), generator=g)
        ids[i, 1 + n] = vocab - 1
    return ids


# ---- tokenizer ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_names():
    d = json.loads(FIXTURE.read_text())
    return tuple(d.keys()), tuple(float(v) for v in d.values())


@functools.lru_cache(maxsize=None)
def learn_merges(n_merges: int = 300) -> tuple:
    import regex
    from freepose_amd import clip_tokenizer as ct
    enc = ct.bytes_to_unicode()
    pat = regex.compile(ct.SPLIT_PATTERN, regex.IGNORECASE)
    words = Counter()
    for name in fixture_names()[0]:
        for tok in regex.findall(pat, ct.clean_text(name)):
            sym = [enc[b] for b in tok.encode("utf-8")]
            sym[-1] += "</w>"
            words[tuple(sym)] += 1
    merges = []
    for _ in range(n_merges):
        pairs = Counter()
        for w, c in words.items():
            for a in zip(w[:-1], w[1:]):
                pairs[a] += c
        if not pairs:
            break
        top = max(pairs.values())
        best = min(p for p, c in pairs.items() if c == top)
        merges.append(best)
        new = Counter()
        for w, c in words.items():
            out, i = [], 0
            while i < len(w):
                if i + 1 < len(w) and (w[i], w[i + 1]) == best:
                    out.append(w[i] + w[i + 1])
                    i += 2
                else:
                    out.append(w[i])
                    i += 1
            new[tuple(out)] += c
        words = new
    return tuple(merges)


def write_bpe_file(path, merges=None) -> Path:
    """`.txt` or `.txt.gz` by the suffix of `path`"""
    merges = learn_merges() if merges is None else merges
    text = '"#version: synthetic test vocabulary\n' + "\n".join(f"{a} {b}" for a, b in merges) + "\n"
    p = Path(path)
    if p.suffix == ".gz":
        with gzip.open(p, "wb") as f:
            f.write(text.encode("utf-8"))
    else:
        p.write_bytes(text.encode("utf-8"))
    return p


def open_clip_vocab(merges) -> dict:
    from freepose_amd import clip_tokenizer as ct
    vocab = list(ct.bytes_to_unicode().values())
    vocab = vocab + [v + "</w>" for v in vocab] + ["".join(m) for m in merges] + ["<|startoftext|>", "<|endoftext|>"]
    return dict(zip(vocab, range(len(vocab))))


def hf_tokenizer(merges=None):
    from transformers import CLIPTokenizer
    merges = learn_merges() if merges is None else merges
    return CLIPTokenizer(vocab=open_clip_vocab(merges), merges=[tuple(m) for m in merges])
