"""Drop-in for the reference's `src/pipeline/retrieval/clip.py` (CLIPFeatureExtractor :7-18).

The reference builds an open_clip model (`create_model_from_pretrained`) and calls `encode_image(Normalize(images))` on a module cast to
bf16; here the same forward is one call into libfreepose_hip.so (fp_clip_encode_image: CLIP normalisation, patch GEMM, pre-LayerNorm
blocks with the general-head-dimension attention kernel, ln_post on the class token, projection).  Weights use open_clip's visual
state-dict names, so the `visual.*` tensors of an open_clip checkpoint load unchanged.

The text side — `clip.tokenizer(names)`, `clip.model.encode_text(ids)`, what GPT4ScaleEstimator.generate_clip_features calls
(scale_estimators.py:91-94) — is fp_clip_text_encode (token + positional embedding, the blocks under the causal attention kernel,
ln_final on the end-of-text token, text_projection) behind freepose_amd.clip_tokenizer.SimpleTokenizer.  It exists when the checkpoint
holds the text tensors (top-level open_clip names or a `text.` prefix), or on explicitly allowed random weights; the tower is created
on first use, so image-only users pay no memory for it.  Without it the three calls raise NotImplementedError.
"""
from __future__ import annotations

import os
import warnings
from pathlib import Path

import torch

from freepose_amd import ops

_TEXT_TOP = ("token_embedding.weight", "positional_embedding", "ln_final.weight", "ln_final.bias", "text_projection")


def _unwrap(sd: dict) -> dict:
    """a checkpoint's tensors without the "state_dict" level and the `module.` prefix"""
    if isinstance(sd, dict) and "state_dict" in sd and not any(torch.is_tensor(v) for v in sd.values()):
        sd = sd["state_dict"]
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


def visual_state_dict(sd: dict) -> dict:
    """the image tower's tensors of a checkpoint: a full open_clip state dict (`visual.` prefix, possibly under "state_dict" and a
    `module.` prefix) or the visual state dict itself"""
    if isinstance(sd, dict) and "state_dict" in sd and "conv1.weight" not in sd and "visual.conv1.weight" not in sd:
        sd = sd["state_dict"]
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    if any(k.startswith("visual.") for k in sd):
        sd = {k[7:]: v for k, v in sd.items() if k.startswith("visual.")}
    return sd


def text_state_dict(sd: dict) -> dict:
    """the text tower's tensors of a checkpoint under their open_clip names: the top-level `token_embedding.weight`,
    `positional_embedding`, `transformer.resblocks.*`, `ln_final.*`, `text_projection` of a full CLIP state dict, or the same names
    behind a `text.` prefix (open_clip's custom-text models).  Never a `visual.*` tensor; {} when the checkpoint has no text side
    (a visual-only state dict has a `conv1.weight`, and its top-level `transformer.*` belongs to the image tower)."""
    sd = _unwrap(sd)
    if any(k.startswith("text.") for k in sd):
        sd = {k[5:]: v for k, v in sd.items() if k.startswith("text.")}
    if "token_embedding.weight" not in sd or "conv1.weight" in sd:
        return {}
    return {k: v for k, v in sd.items() if k in _TEXT_TOP or k.startswith("transformer.resblocks.")}


class _ClipModel:
    """what the reference reaches as `clip.model`: the image tower's attributes and calls, plus `encode_text`"""

    def __init__(self, visual, owner):
        self._visual, self._owner = visual, owner

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return getattr(self._visual, name)

    def encode_text(self, ids):
        return self._owner.encode_text(ids)


class CLIPFeatureExtractor(torch.nn.Module):
    """Same surface as the reference nn.Module: construct, call with bf16 images [B,3,224,224] in [0,1] -> bf16 [B, embed_dim].
    The weights live in the HIP library's device tables (ops.ClipVisual, ops.ClipText); `.to(...)` is a no-op by construction."""

    def __init__(self, model_name: str = "ViT-bigG-14", pretrained: str = "laion2b_s39b_b160k", state_dict: dict | None = None,
                 seed: int = 0, allow_random_weights: bool | None = None, bpe_vocab: str | None = None):
        """Weights: `state_dict` if given, else the file FREEPOSE_CLIP_WEIGHTS names (a torch.save'd open_clip checkpoint or visual
        state dict; `pretrained` is the tag the reference downloads and only documents which file that should be).  A missing
        checkpoint is an ERROR unless random weights were asked for: `allow_random_weights=True` (the CLIs' --allow_random_weights;
        an argument the reference's constructor does not have, as on DINOv2FeatureExtractor) or FREEPOSE_ALLOW_RANDOM_WEIGHTS=1 —
        benchmarks and tests only.  `seed` only picks WHICH random weights; it grants no permission.
        `bpe_vocab`: the tokenizer's merges file (else FREEPOSE_CLIP_BPE), read on the first use of `tokenizer`."""
        super().__init__()
        if model_name not in ops.CLIP_ARCHS:
            raise ValueError(f"unknown CLIP model {model_name} (known: {sorted(ops.CLIP_ARCHS)})")
        self.model_name, self.pretrained = model_name, pretrained
        self.checkpoint = None
        self.bpe_vocab = bpe_vocab
        self._seed = seed
        self._text_sd, self._text, self._tokenizer = None, None, None
        random_text = False
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
                random_text = model_name in ops.CLIP_TEXT_ARCHS
        if state_dict is not None:
            self._text_sd = text_state_dict(state_dict) or None
            state_dict = visual_state_dict(state_dict)
        self.has_text_tower = model_name in ops.CLIP_TEXT_ARCHS and (self._text_sd is not None or random_text)
        self.model = _ClipModel(ops.ClipVisual(model_name, state_dict, seed=seed), self)
        self.embed_dim = self.model.embed_dim
        self._anchor = torch.nn.Parameter(torch.zeros((), device="cuda"), requires_grad=False)   # `next(clip.parameters()).device`

    def require_text_tower(self):
        if not self.has_text_tower:
            raise NotImplementedError(f"CLIP text tower not available for {self.model_name}: the loaded weights hold no text tensors "
                                      "(token_embedding.weight, transformer.resblocks.*, ln_final.*, text_projection); text embeddings "
                                      "then come from a file (scale_feats.pt)")

    @property
    def text_model(self):
        """ops.ClipText, created on first use (about 1.4 GB of weights for ViT-bigG-14)"""
        self.require_text_tower()
        if self._text is None:
            self._text = ops.ClipText(self.model_name, self._text_sd, seed=self._seed)
            self._text_sd = None          # the tower keeps its own device copies
        return self._text

    @property
    def tokenizer(self):
        """callable: list of str -> int64 [N, 77] (reference: `clip.tokenizer(object_names)`, scale_estimators.py:91)"""
        self.require_text_tower()
        if self._tokenizer is None:
            from freepose_amd.clip_tokenizer import SimpleTokenizer
            self._tokenizer = SimpleTokenizer(self.bpe_vocab, context_length=ops.CLIP_TEXT_ARCHS[self.model_name][5])
        return self._tokenizer

    def encode_text(self, ids):
        """token ids [N, ctx] -> bf16 [N, embed_dim] on the device (not normalised, like open_clip's encode_text)"""
        self.require_text_tower()
        with torch.inference_mode():
            return self.text_model.encode_text(ids)

    def forward(self, images):
        with torch.inference_mode():
            return self.model.encode_image(images)
