"""One SHA-256 per case over the raw output bytes of the two transformer drivers (fp_vit_forward, fp_clip_encode_image).

    python tools/driver_bits.py [--tree DIR] [--case NAME ...] [--out FILE]

Seeded inputs, weights from ops.random_state_dict / ops.random_clip_state_dict.  Two trees whose drivers compute the same thing print
the same table: run it with --tree on each (DIR = the root that holds freepose_amd/ with its built library) and diff the outputs.
--case restricts the run to the named cases (e.g. under a kernel trace).  The cases cover both context options of the ViT driver
(ln_fused, gemm_row_split), both routes of the LayerNorm-statistics hand-off in one forward (vits_b32_l2), the position-embedding resize,
the fold event across streams and the re-fold after a weight was registered again, and CLIP towers of head dimension 64 / 80 / 104.
"""
from __future__ import annotations

import argparse
import hashlib
import sys
from pathlib import Path


def sha(t) -> str:
    import torch
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().cpu().view(torch.int16).numpy().tobytes()).hexdigest()


def images(B, S, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, 3, S, S, generator=g).to(torch.bfloat16).cuda()


def vit_cases(ops):
    import torch
    models = {}

    def vit(name):
        if name not in models:
            sd = ops.random_state_dict(name, seed=11)
            models[name] = (ops.ViT(name, sd), sd)
        return models[name]

    for ln_fused in (1, 0):
        for split in (-1, 0):
            for ft in ("cls", "reg", "patch", "patch_normalized"):
                def run(ln_fused=ln_fused, split=split, ft=ft):
                    ops.set_option("ln_fused", ln_fused)
                    ops.set_option("gemm_row_split", split)
                    try:
                        return sha(vit("dinov2_vits14_reg")[0](images(2, 224, 21), layer=22, feature_type=ft))
                    finally:
                        ops.set_option("ln_fused", -1)
                        ops.set_option("gemm_row_split", -1)
                yield f"vits_b2_l22_{ft}_ln{ln_fused}_split{'default' if split < 0 else split}", run
    yield "vits_b32_l2", lambda: sha(vit("dinov2_vits14_reg")[0](images(32, 224, 22), layer=2, feature_type="patch"))
    yield "vitl_518_l2", lambda: sha(vit("dinov2_vitl14_reg")[0](images(1, 518, 23), layer=2, feature_type="patch"))
    yield "vitl_420_l1", lambda: sha(vit("dinov2_vitl14_reg")[0](images(1, 420, 24), layer=1, feature_type="patch"))

    # fold on the first stream, the fold event on a second one, a re-fold after a block weight was registered again: a fresh model
    fold = {}

    def fold_model():
        if not fold:
            sd = ops.random_state_dict("dinov2_vits14_reg", seed=12)
            fold["m"], fold["sd"], fold["x"] = ops.ViT("dinov2_vits14_reg", sd), sd, images(1, 224, 25)
        return fold["m"], fold["sd"], fold["x"]

    def first():
        m, _, x = fold_model()
        return sha(m(x, layer=12, feature_type="patch"))

    def second_stream():
        m, _, x = fold_model()
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.Stream()):
            return sha(m(x, layer=12, feature_type="patch"))

    def refold():
        m, sd, x = fold_model()
        name = "blocks.3.mlp.fc1.weight"
        m.load_state_dict({name: sd[name]})
        return sha(m(x, layer=12, feature_type="patch"))

    yield "vits_fold_first", first
    yield "vits_fold_second_stream", second_stream
    yield "vits_fold_refold", refold


def clip_cases(ops):
    for name, B in (("tiny-64-s56", 3), ("tiny-80-s56", 3), ("tiny-104-s56", 3), ("tiny-bigG-wide", 2), ("tiny-64", 1)):
        def run(name=name, B=B):
            m = ops.ClipVisual(name, ops.random_clip_state_dict(name, seed=13))
            return sha(m.encode_image(images(B, m.image_size, 31)))
        yield f"clip_{name}_b{B}", run


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=str(Path(__file__).resolve().parent.parent), help="root of the tree whose library runs")
    ap.add_argument("--case", action="append", help="run only this case (repeatable)")
    ap.add_argument("--out", help="also write the table to this file")
    args = ap.parse_args(argv)
    sys.path.insert(0, str(Path(args.tree).resolve()))
    from freepose_amd import _lib, ops
    print(f"# library: {_lib.LIB_PATH}", flush=True)
    lines = []
    for name, run in list(vit_cases(ops)) + list(clip_cases(ops)):
        if args.case and name not in args.case:
            continue
        lines.append(f"{name} {run()}")
        print(lines[-1], flush=True)
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
