"""Timings behind profiles/clip_text.md (not a test, gates nothing):  python tools/clip_text_perf.py [--model ViT-bigG-14]

Seeded random weights, the synthetic BPE vocabulary of the tests (tests/_clip_text_ref.py) and the 2201 names of
tests/golden/gpt4_scale_names.json; only the text tower is built.  Prints
  * GPT4ScaleEstimator.generate_clip_features over the 2201 names (tokenizer + tower + normalisation + copy to the host): wall clock
    with a device synchronisation before and after, 2 warm-up calls, median (minimum) of 5; the tokenizer's share on its own;
  * one 256-prompt encode_text call (HIP events on the launch stream, 3 warm-up calls, median (minimum) of 10) and its split: the causal
    attention and LayerNorm kernels ALONE on tensors of the call's shapes, per launch, times their launch count; the remainder is
    "GEMM + gathers";
  * the causal flavour of csrc/attention_hd.hip next to the unmasked one (fp_op_attention_hd) on the same [B, 80, 3 * width] buffer
    (77 real tokens)."""
from __future__ import annotations

import argparse
import statistics
import sys
import tempfile
import time
import types
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from freepose_amd import ops                                                    # noqa: E402
from freepose_amd.clip_tokenizer import SimpleTokenizer                         # noqa: E402
from freepose_amd.src.pipeline.estimators.scale_estimators import GPT4ScaleEstimator   # noqa: E402
from tests import _clip_text_ref as tr                                          # noqa: E402


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
    ap.add_argument("--chunk", type=int, default=256)
    args = ap.parse_args()
    tower = ops.ClipText(args.model, seed=0, chunk=args.chunk)
    npad = (tower.ctx + 15) // 16 * 16
    g = torch.Generator().manual_seed(0)
    print(f"# {args.model} text tower: width {tower.width}, depth {tower.depth}, heads {tower.heads}, {tower.ctx} tokens padded to {npad}, "
          f"{args.chunk} prompts per call")
    with tempfile.TemporaryDirectory() as tmp:
        bpe = tr.write_bpe_file(Path(tmp) / "bpe_synth.txt.gz")
        scale_file = Path(tmp) / "gpt4_scales.json"
        scale_file.write_text(tr.FIXTURE.read_text())
        clip = types.SimpleNamespace(has_text_tower=True, tokenizer=SimpleTokenizer(bpe, context_length=tower.ctx), model=tower)
        names = list(tr.fixture_names()[0])
        clip.tokenizer.cache.clear()
        t = time.perf_counter()
        ids = clip.tokenizer(names)
        cold = 1e3 * (time.perf_counter() - t)
        full = wall_ms(lambda: GPT4ScaleEstimator.generate_clip_features(str(scale_file), clip, feats_path=None))
        tok = wall_ms(lambda: clip.tokenizer(names), warmup=1)
    print(f"| generate_clip_features, {len(names)} names | ms |")
    print("|---|---|")
    print("| whole call | %.1f (%.1f) |" % full)
    print("| of it: tokenizer (host, warm word cache) | %.1f (%.1f) |" % tok)
    print(f"| tokenizer, cold word cache (first call) | {cold:.1f} |")
    n_real = float((ids != 0).sum(dim=1).float().mean())
    print(f"(mean prompt length {n_real:.1f} of {tower.ctx} positions)")

    B = args.chunk
    part = ids[:B].cuda()
    enc, enc_min = event_ms(lambda: tower.encode_text(part))
    qkv = (0.5 * torch.randn((B, npad, 3 * tower.width), generator=g)).to("cuda", torch.bfloat16)
    o = torch.empty((B, npad, tower.width), device="cuda", dtype=torch.bfloat16)
    att, att_min = event_ms(lambda: ops.attention_causal(qkv, tower.heads, tower.ctx, out=o))
    hd, hd_min = event_ms(lambda: ops.attention_hd(qkv, tower.heads, tower.ctx, out=o))
    x = torch.randn((B * npad, tower.width), generator=g).to("cuda", torch.bfloat16)
    w = torch.ones(tower.width, device="cuda", dtype=torch.bfloat16)
    ln, _ = event_ms(lambda: ops.layernorm(x, w, w, 1e-5))
    n_att, n_ln = tower.depth, 2 * tower.depth                                  # (ln_final runs on B rows only)
    rest = enc - n_att * att - n_ln * ln
    print("| B | encode_text ms | TFLOP/s | causal attention ms | LayerNorm ms | GEMM + gathers ms |")
    print("|---|---|---|---|---|---|")
    print(f"| {B} | {enc:.2f} ({enc_min:.2f}) | {tower.flops(B) / enc / 1e9:.0f} | {n_att * att:.2f} ({1e3 * att:.0f} µs x {n_att}) | "
          f"{n_ln * ln:.2f} ({1e3 * ln:.0f} µs x {n_ln}) | {rest:.1f} |")
    print(f"| attention on [{B}, {npad}, 3 x {tower.width}], {tower.ctx} tokens | µs per launch |")
    print("|---|---|")
    print(f"| fp_op_attention_causal | {1e3 * att:.1f} ({1e3 * att_min:.1f}) |")
    print(f"| fp_op_attention_hd (no mask) | {1e3 * hd:.1f} ({1e3 * hd_min:.1f}) |")


if __name__ == "__main__":
    main()
