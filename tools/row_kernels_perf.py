"""Row-kernel timing probe (development): the bank scan / select / merge, the template scorers, the view re-rank and the row normalisers
(stand-alone, FFA tail, LayerNorm tail) at their product shapes, seeded inputs, HIP events over `--calls` back-to-back calls after a warm-up.
One JSON line per shape: {"op", "shape", "us_per_call"}.  Run under `rocprofv3 --kernel-trace --stats` for the per-kernel durations.

    python tools/row_kernels_perf.py [--calls 50] [--out FILE]

It times the tree it lives in: to compare two commits, export each with its built library and run this file from each."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from freepose_amd import ops  # noqa: E402


GEN = None


def rand_bf16(rng, *shape):
    """seeded normal values; the large operands are drawn on the device (the host generator would dominate the run)"""
    global GEN
    if int(np.prod(shape)) < (1 << 22):
        return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda().to(torch.bfloat16)
    if GEN is None:
        GEN = torch.Generator(device="cuda").manual_seed(0)
    return torch.randn(shape, generator=GEN, device="cuda", dtype=torch.float32).to(torch.bfloat16)


def timed(fn, calls):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = ops.Timer()
    t.start()
    for _ in range(calls):
        fn()
    t.stop()
    return t.elapsed_ms() / calls * 1e3


def cases(rng):
    D = 1024
    bank = ops.bank_prepare(torch.from_numpy(rng.standard_normal((46037, D)).astype(np.float32)).cuda())
    for Q in (1, 4, 5):
        q = ops.l2_normalize(rand_bf16(rng, Q, D))
        yield "bank_topk", f"46037x{D} Q={Q} k=100", lambda q=q: ops.bank_topk(bank, q, 100)
    cs = rand_bf16(rng, 1, 800).float()
    ci = torch.from_numpy(rng.permutation(46037)[:800].astype(np.int32)).cuda()[None]
    yield "topk_merge", "8x100 -> 100", lambda: ops.topk_merge(cs, ci, 100)
    for T, P in ((576, 1369), (600, 900)):
        tn = ops.l2_normalize(rand_bf16(rng, T, P, D), inplace=True)
        qn = ops.l2_normalize(rand_bf16(rng, P, D))
        yield "template_score normalized", f"T={T} P={P} D={D}", lambda tn=tn, qn=qn: ops.template_score(tn, qn, normalized=True)
        if P == 1369:
            yield "template_score raw", f"T={T} P={P} D={D}", lambda tn=tn, qn=qn: ops.template_score(tn, qn)
        del tn
    views = rand_bf16(rng, 100 * 600, D)
    offsets = torch.arange(0, 101, dtype=torch.int32).cuda() * 600
    cand = torch.arange(100, dtype=torch.int32).cuda()[None]
    fq = ops.l2_normalize(rand_bf16(rng, 1, D))
    yield "rerank_views", f"100 candidates x 600 views D={D} k=5", lambda: ops.rerank_views(views, offsets, cand, fq, 5)
    del views
    big = rand_bf16(rng, 540000, D)     # in place: after the first call the rows are unit vectors, the work per row is the same
    yield "l2_normalize in place", f"540000x{D}", lambda: ops.l2_normalize(big, inplace=True)
    del big
    for B in (1, 5):
        feats = rand_bf16(rng, B, 37 * 37, D)
        masks = torch.from_numpy(rng.random((B, 37 * 14, 37 * 14)) < 0.4).cuda()
        yield "ffa normalize", f"B={B} 37x37x{D}", lambda feats=feats, masks=masks: ops.ffa(feats, masks, 14, normalize=True)
    vit = ops.ViT("dinov2_vitl14_reg", seed=0)
    imgs = torch.from_numpy(rng.random((19, 3, 420, 420)).astype(np.float32)).cuda().to(torch.bfloat16)
    out = torch.empty((19, 900, D), dtype=torch.bfloat16, device="cuda")
    yield "ViT.forward patch_normalized", "ViT-L 420x420 B=19", lambda: vit.forward(imgs, 22, "patch_normalized", out=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    lines = []
    for op, shape, fn in cases(rng):
        us = timed(fn, a.calls)
        lines.append(json.dumps({"op": op, "shape": shape, "us_per_call": round(us, 2)}))
        print(lines[-1], flush=True)
    if a.out:
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
