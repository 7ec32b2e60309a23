"""Drop-in for the reference's `src/pipeline/retrieval/clip.py` (CLIPFeatureExtractor :7-18), image side only.

The reference builds an open_clip model (`create_model_from_pretrained`) and calls `encode_image(Normalize(images))` on a module cast to
bf16; here the same forward is one call into libfreepose_hip.so (fp_clip_encode_image: CLIP normalisation, patch GEMM, pre-LayerNorm
blocks with the general-head-dimension attention kernel, ln_post on the class token, projection).  Weights use open_clip's visual
state-dict names, so the `visual.*` tensors of an open_clip checkpoint load unchanged.  The text tower and the tokenizer are not provided:
GPT4ScaleEstimator reads its text embeddings from a file (`data/scale_feats.pt`).
"""
from __future__ import annotations

import os
import warnings
from pathlib import Path

import torch

from freepose_amd import ops


def visual_state_dict(sd: dict) -> dict:
    """the image tower's tensors of a checkpoint: a full open_clip state dict (`visual.` prefix, possibly under "state_dict" and a
    `module.` prefix) or the visual state dict itself"""
    if isinstance(sd, dict) and "state_dict" in sd and "conv1.weight" not in sd and "visual.conv1.weight" not in sd:
        sd = sd["state_dict"]
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    if any(k.startswith("visual.") for k in sd):
        sd = {k[7:]: v for k, v in sd.items() if k.startswith("visual.")}
    return sd


class CLIPFeatureExtractor(torch.nn.Module):
    """Same surface as the reference nn.Module: construct, call with bf16 images [B,3,224,224] in [0,1] -> bf16 [B, embed_dim].
    The weights live in the HIP library's device tables (ops.ClipVisual); `.to(...)` is a no-op by construction."""

    def __init__(self, model_name: str = "ViT-bigG-14", pretrained: str = "laion2b_s39b_b160k", state_dict: dict | None = None,
                 seed: int = 0, allow_random_weights: bool | None = None):
        """Weights: `state_dict` if given, else the file FREEPOSE_CLIP_WEIGHTS names (a torch.save'd open_clip checkpoint or visual
        state dict; `pretrained` is the tag the reference downloads and only documents which file that should be).  A missing
        checkpoint is an ERROR unless random weights were asked for: `allow_random_weights=True` (the CLIs' --allow_random_weights;
        an argument the reference's constructor does not have, as on DINOv2FeatureExtractor) or FREEPOSE_ALLOW_RANDOM_WEIGHTS=1 —
        benchmarks and tests only.  `seed` only picks WHICH random weights; it grants no permission."""
        super().__init__()
        if model_name not in ops.CLIP_ARCHS:
            raise ValueError(f"unknown CLIP model {model_name} (known: {sorted(ops.CLIP_ARCHS)})")
        self.model_name, self.pretrained = model_name, pretrained
        self.checkpoint = None
        if state_dict is None:
            env = os.environ.get("FREEPOSE_CLIP_WEIGHTS")
            if env and Path(env).is_file():
                state_dict = torch.load(env, map_location="cpu")
                self.checkpoint = Path(env)
            else:
                if allow_random_weights is None:
                    allow_random_weights = os.environ.get("FREEPOSE_ALLOW_RANDOM_WEIGHTS", "0") == "1"
                if not allow_random_weights:
                    raise FileNotFoundError(
                        f"CLIP checkpoint for {model_name} ({pretrained}) not found: set FREEPOSE_CLIP_WEIGHTS to the file (now "
                        f"{env or '<unset>'}).  Pass --allow_random_weights / allow_random_weights=True to run on seeded random-init "
                        "weights of the same architecture (benchmarks and tests only).")
                warnings.warn(f"no CLIP checkpoint for {model_name} (set FREEPOSE_CLIP_WEIGHTS); using seeded random-init weights — "
                              "features are NOT meaningful for real images", RuntimeWarning)
        if state_dict is not None:
            state_dict = visual_state_dict(state_dict)
        self.model = ops.ClipVisual(model_name, state_dict, seed=seed)
        self.embed_dim = self.model.embed_dim
        self._anchor = torch.nn.Parameter(torch.zeros((), device="cuda"), requires_grad=False)   # `next(clip.parameters()).device`

    @property
    def tokenizer(self):
        raise NotImplementedError("the CLIP text tower and its tokenizer are not provided: text embeddings come from a file (scale_feats.pt)")

    def encode_text(self, *args, **kwargs):
        raise NotImplementedError("the CLIP text tower is not provided: text embeddings come from a file (scale_feats.pt)")

    def forward(self, images):
        with torch.inference_mode():
            return self.model.encode_image(images)
