"""Timings behind profiles/clip_scale.md (not a test, gates nothing):  python tools/clip_scale_perf.py [--model ViT-bigG-14]

Seeded random weights.  Prints one markdown table row per batch size (encode_image: HIP events on the launch stream around one call,
3 warm-up calls, median (minimum) of 10; the attention and LayerNorm kernels ALONE on tensors of the call's shapes, per launch, times
their launch count; the remainder is "GEMM + rest") and the two GPT4ScaleEstimator.estimate rows (wall clock around the call with a
device synchronisation before and after, median (minimum) of 5)."""
from __future__ import annotations

import argparse
import statistics
import sys
import tempfile
import time
import types
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from freepose_amd import ops                                                    # noqa: E402
from freepose_amd.src.pipeline.estimators.scale_estimators import GPT4ScaleEstimator   # noqa: E402
from freepose_amd.src.pipeline.retrieval.clip import CLIPFeatureExtractor       # noqa: E402


def event_ms(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def wall_ms(fn, warmup=2, reps=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="ViT-bigG-14")
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 5, 32])
    args = ap.parse_args()
    clip = CLIPFeatureExtractor(args.model, allow_random_weights=True)
    m = clip.model
    n_tok = 1 + m.grid * m.grid
    npad = (n_tok + 15) // 16 * 16
    g = torch.Generator().manual_seed(0)
    print(f"# {args.model}: width {m.width}, depth {m.depth}, heads {m.heads}, {n_tok} tokens padded to {npad}")
    print("| B | encode_image ms | TFLOP/s | attention ms | LayerNorm ms | GEMM + rest ms |")
    print("|---|---|---|---|---|---|")
    for B in args.batches:
        images = torch.rand((B, 3, m.image_size, m.image_size), generator=g).to("cuda", torch.bfloat16)
        enc, enc_min = event_ms(lambda: m.encode_image(images))
        qkv = (0.5 * torch.randn((B, npad, 3 * m.width), generator=g)).to("cuda", torch.bfloat16)
        o = torch.empty((B, npad, m.width), device="cuda", dtype=torch.bfloat16)
        att, _ = event_ms(lambda: ops.attention_hd(qkv, m.heads, n_tok, out=o))
        x = torch.randn((B * npad, m.width), generator=g).to("cuda", torch.bfloat16)
        w = torch.ones(m.width, device="cuda", dtype=torch.bfloat16)
        ln, _ = event_ms(lambda: ops.layernorm(x, w, w, 1e-5))
        n_att, n_ln = m.depth, 2 * m.depth + 1                                  # (+ ln_pre; ln_post runs on B rows only)
        rest = enc - n_att * att - n_ln * ln
        print(f"| {B} | {enc:.2f} ({enc_min:.2f}) | {m.flops(B) / enc / 1e9:.0f} | {n_att * att:.2f} ({1e3 * att:.0f} µs x {n_att}) | "
              f"{n_ln * ln:.2f} ({1e3 * ln:.0f} µs x {n_ln}) | {rest:.1f} |", flush=True)

    # estimate(): 5 proposals of a 480 x 640 image, 2000-row table as wide as the tower's embedding
    H, W, n = 480, 640, 5
    rng = np.random.Generator(np.random.PCG64(1))
    table = rng.standard_normal((2000, m.embed_dim)).astype(np.float32)
    table /= np.linalg.norm(table, axis=1, keepdims=True)
    with tempfile.TemporaryDirectory() as tmp:
        torch.save({"feats": torch.from_numpy(table), "scales": torch.from_numpy(rng.random(2000).astype(np.float32) + 0.05)}, f"{tmp}/feats.pt")
        est = GPT4ScaleEstimator(clip, feats_path=f"{tmp}/feats.pt")
    yy, xx = np.mgrid[0:H, 0:W]
    depth = 0.8 + 0.001 * xx + 0.0005 * yy + 0.01 * rng.random((H, W))
    masks = np.zeros((n, H, W), dtype=bool)
    for i in range(n):
        masks[i] = (yy - 120 - 50 * i) ** 2 + (xx - 100 - 100 * i) ** 2 < (40 + 5 * i) ** 2
    props = types.SimpleNamespace(masks=[torch.from_numpy(x) for x in masks],
                                  proposals=[c for c in torch.rand((n, 3, m.image_size, m.image_size), generator=g)])
    K = np.array([[800.0, 0, W / 2], [0, 800.0, H / 2], [0, 0, 1]])
    print("| estimate, 5 proposals | ms |")
    print("|---|---|")
    print("| without depth | %.2f (%.2f) |" % wall_ms(lambda: est.estimate(props)))
    print("| with depth | %.2f (%.2f) |" % wall_ms(lambda: est.estimate(props, depth, K)))


if __name__ == "__main__":
    main()
