"""CLIP image tower (csrc/clip.hip) against the fp32 restatement and the bf16 torch module on the CPU."""
import functools

import pytest
import torch

from tests import _clip_ref as cr

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


@functools.lru_cache(maxsize=None)
def _tower(name):
    """(device tower, fp32 reference, bf16-module-on-CPU output, images) for 3 crops; computed once per tower and left unchanged"""
    from freepose_amd import ops
    width, depth, heads, mlp, embed, patch, grid = ops.CLIP_ARCHS[name]
    sd = ops.random_clip_state_dict(name, seed=11)                       # bf16 tensors
    S = patch * grid
    g = torch.Generator().manual_seed(13)
    images = torch.rand((3, 3, S, S), generator=g).to(torch.bfloat16)
    xn = cr.normalize_bf16(images)
    ref32 = cr.clip_forward({k: v.float() for k, v in sd.items()}, xn.float(), heads)
    model = cr.hf_model(sd, width, depth, heads, mlp, embed, patch, grid).to(torch.bfloat16)
    with torch.no_grad():
        mod16 = model(pixel_values=xn).image_embeds.float()
    return ops.ClipVisual(name, sd), ref32, mod16, images


def test_feature_is_present():
    from src.pipeline.retrieval.clip import CLIPFeatureExtractor  # noqa: F401
    from freepose_amd.src.pipeline.estimators import scale_estimators
    from freepose_amd import _lib
    assert hasattr(scale_estimators, "GPT4ScaleEstimator") and hasattr(_lib.load(), "fp_op_attention_hd")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", ["tiny-64-s56", "tiny-80-s56", "tiny-104-s56", "tiny-64", "tiny-80", "tiny-104", "tiny-bigG-wide"])
def test_clip_tower(name, B):
    tower, ref32, mod16, images = _tower(name)
    got = tower(images[:B].cuda()).float().cpu()
    assert got.shape == ref32[:B].shape and torch.isfinite(got).all()
    cos = torch.nn.functional.cosine_similarity(got, ref32[:B], dim=-1).min().item()
    e_hip, e_mod = _rel(got, ref32[:B]), _rel(mod16[:B], ref32[:B])
    print(f"{name} B={B}: min cosine {cos:.6f}, rel(hip, fp32) {e_hip:.3e}, rel(torch bf16 module, fp32) {e_mod:.3e}")
    assert cos >= 0.999
    assert e_hip <= 1.25 * e_mod + 1e-4


@pytest.mark.parametrize("name", ["tiny-104-s56", "tiny-80", "tiny-bigG-wide"])
def test_clip_embedding_does_not_depend_on_the_batch(name):
    tower, _, _, images = _tower(name)
    batch = tower(images.cuda())
    for i in range(3):
        assert torch.equal(tower(images[i:i + 1].cuda())[0], batch[i])


def test_clip_refusals():
    from freepose_amd import ops
    tower, _, _, images = _tower("tiny-64-s56")
    with pytest.raises(RuntimeError, match="56 x 56"):
        tower(torch.zeros((1, 3, 70, 70), dtype=torch.bfloat16, device="cuda"))
    with pytest.raises(RuntimeError, match="quick_gelu"):
        ops.ClipVisual("tiny-64-s56", quick_gelu=True)
    sd = ops.random_clip_state_dict("tiny-64-s56", 1)
    sd.pop("proj")
    with pytest.raises(KeyError):
        ops.ClipVisual("tiny-64-s56", sd)


def test_layernorm_width_1664():
    """the LayerNorm kernel at ViT-bigG/14's width (four 16-byte loads per lane)"""
    from freepose_amd import ops
    g = torch.Generator().manual_seed(41)
    x = (torch.randn((37, 1664), generator=g) * 2).to(torch.bfloat16)
    gm, b = torch.randn(1664, generator=g).to(torch.bfloat16), (torch.randn(1664, generator=g) * 0.5).to(torch.bfloat16)
    y = ops.layernorm(x, gm, b, 1e-5)
    ref = torch.nn.functional.layer_norm(x.float(), (1664,), gm.float(), b.float(), 1e-5)
    assert (y.float().cpu() - ref).abs().max().item() < 0.03 + 0.01 * ref.abs().max().item()
    assert _rel(y, ref) < 5e-3
