"""CLIP text tower (csrc/clip_text.hip) against the fp32 restatement and the bf16 torch module on the CPU; the scale table end to end."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _clip_ref as cr
from tests import _clip_text_ref as tr

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


def _text_towers():
    from freepose_amd import ops
    return sorted(n for n in ops.CLIP_TEXT_ARCHS if n.startswith("tiny-"))


@functools.lru_cache(maxsize=None)
def _reference(arch):
    """(state dict, ids, fp32 restatement, bf16-module-on-CPU output) of one text configuration: 3 prompts of 1, 5 and 75 tokens (1, 8
    and 15 at 17 positions); computed once per configuration — towers that differ only in their image side share it — and left unchanged"""
    from freepose_amd import ops
    width, depth, heads, mlp, vocab, ctx, embed = arch
    name = next(n for n in sorted(ops.CLIP_TEXT_ARCHS) if ops.CLIP_TEXT_ARCHS[n] == arch)
    sd = ops.random_clip_text_state_dict(name, seed=11)                       # bf16 tensors
    ids = tr.make_ids([1, 5, 75] if ctx == 77 else [1, 8, 15], vocab, ctx, seed=13)
    ref32 = tr.clip_text_forward({k: v.float() for k, v in sd.items()}, ids, heads)
    model = tr.hf_model(sd, width, depth, heads, mlp, vocab, ctx, embed).to(torch.bfloat16)
    with torch.no_grad():
        mod16 = model(input_ids=ids).text_embeds.float()
    return sd, ids, ref32, mod16


@functools.lru_cache(maxsize=None)
def _tower(name):
    from freepose_amd import ops
    sd, ids, ref32, mod16 = _reference(ops.CLIP_TEXT_ARCHS[name])
    return ops.ClipText(name, sd), ids, ref32, mod16


def test_feature_is_present():
    from freepose_amd import _lib, ops
    assert hasattr(_lib.load(), "fp_clip_text_encode") and "tiny-bigG-text" in ops.CLIP_TEXT_ARCHS      # fails without the feature


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", _text_towers())
def test_clip_text_tower(name, B):
    tower, ids, ref32, mod16 = _tower(name)
    got = tower(ids[:B]).float().cpu()
    assert got.shape == ref32[:B].shape and torch.isfinite(got).all()
    cos = torch.nn.functional.cosine_similarity(got, ref32[:B], dim=-1).min().item()
    e_hip, e_mod = _rel(got, ref32[:B]), _rel(mod16[:B], ref32[:B])
    print(f"{name} B={B}: min cosine {cos:.6f}, rel(hip, fp32) {e_hip:.3e}, rel(torch bf16 module, fp32) {e_mod:.3e}")
    assert cos >= 0.999
    assert e_hip <= 1.25 * e_mod + 1e-4


@pytest.mark.parametrize("name", ["tiny-104", "tiny-64-c17", "tiny-bigG-text"])
def test_embedding_depends_on_the_prompt_alone(name):
    """bit for bit: not on the batch, not on the chunk it rides in, not on the ids after the end-of-text token"""
    from freepose_amd import ops
    tower, ids, _, _ = _tower(name)
    vocab, ctx = ops.CLIP_TEXT_ARCHS[name][4:6]
    five = torch.cat([ids, ids[:2]])
    batch = tower(five)
    for i in range(3):
        assert torch.equal(tower(ids[i:i + 1])[0], batch[i])
    assert torch.equal(tower.encode_text(five, chunk=2), batch)
    other = ids.clone()
    for row in other:
        eot = int(row.argmax())
        row[eot + 1:] = torch.randint(0, vocab - 1, (ctx - eot - 1,), generator=torch.Generator().manual_seed(eot))
    assert not torch.equal(other, ids)
    assert torch.equal(tower(other), batch[:3])
    assert torch.equal(tower(ids.int()), batch[:3]) and torch.equal(tower(ids.cuda()), batch[:3])


def test_clip_text_refusals():
    from freepose_amd import ops
    tower, ids, _, _ = _tower("tiny-64")
    vocab = ops.CLIP_TEXT_ARCHS["tiny-64"][4]
    good = tower(ids)
    for bad_id in (vocab, -1, 2 ** 31 - 1):
        bad = ids.clone()
        bad[1, 3] = bad_id
        with pytest.raises(RuntimeError, match="outside the vocabulary"):
            tower(bad)
    assert torch.equal(tower(ids), good)                    # the refusal leaves the tower usable
    with pytest.raises(ValueError, match="integer"):
        tower(ids[:, :50])
    with pytest.raises(ValueError, match="integer"):
        tower(ids.float())
    sd = ops.random_clip_text_state_dict("tiny-64", 1)
    sd.pop("text_projection")
    with pytest.raises(KeyError):
        ops.ClipText("tiny-64", sd)
    sd = ops.random_clip_text_state_dict("tiny-64", 1)
    sd["positional_embedding"] = sd["positional_embedding"][:17]
    with pytest.raises(RuntimeError, match="positional_embedding"):
        ops.ClipText("tiny-64", sd)


# ---- the extractor's text side and the scale table ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bpe_file(tmp_path_factory):
    return tr.write_bpe_file(tmp_path_factory.mktemp("bpe") / "bpe_synth.txt.gz")


@pytest.fixture(scope="module")
def scale_file(tmp_path_factory):
    """40 names of the fixture (every 55th) with their sizes, as the reference's data/gpt4_scales.json lays them out"""
    names, sizes = tr.fixture_names()
    path = tmp_path_factory.mktemp("scales") / "gpt4_scales.json"
    path.write_text(json.dumps({names[i]: sizes[i] for i in range(0, 2200, 55)}))
    return path


def test_extractor_without_text_tensors_fails_closed(bpe_file):
    from freepose_amd import ops
    from freepose_amd.src.pipeline.estimators.scale_estimators import GPT4ScaleEstimator
    from freepose_amd.src.pipeline.retrieval.clip import CLIPFeatureExtractor
    clip = CLIPFeatureExtractor("tiny-64-s56", state_dict=ops.random_clip_state_dict("tiny-64-s56", 2), bpe_vocab=str(bpe_file))
    assert not clip.has_text_tower
    with pytest.raises(NotImplementedError, match="text tower"):
        clip.tokenizer
    with pytest.raises(NotImplementedError, match="text tower"):
        clip.encode_text(torch.zeros((1, 77), dtype=torch.long))
    with pytest.raises(NotImplementedError, match="text tower"):
        clip.model.encode_text(torch.zeros((1, 77), dtype=torch.long))
    with pytest.raises(NotImplementedError, match="text tower"):
        GPT4ScaleEstimator(clip, scale_file="no_such_file.json")
    assert clip.model.width == 128 and clip(torch.zeros((1, 3, 56, 56), dtype=torch.bfloat16)).shape == (1, 64)   # the image side is as before


def test_extractor_takes_the_text_tower_from_a_full_checkpoint(bpe_file):
    from freepose_amd import ops
    from freepose_amd.src.pipeline.retrieval.clip import CLIPFeatureExtractor
    sd_t, ids, _, _ = _reference(ops.CLIP_TEXT_ARCHS["tiny-64-s56"])
    full = {**{"visual." + k: v for k, v in ops.random_clip_state_dict("tiny-64-s56", 2).items()}, **sd_t, "logit_scale": torch.zeros(())}
    clip = CLIPFeatureExtractor("tiny-64-s56", state_dict=full, bpe_vocab=str(bpe_file))
    assert clip.has_text_tower and clip._text is None              # created on first use
    got = clip.model.encode_text(ids)
    assert clip._text is not None and torch.equal(got, _tower("tiny-64-s56")[0](ids)) and torch.equal(clip.encode_text(ids), got)
    assert clip.tokenizer(["a photo of desk"]).shape == (1, 77)


def test_generate_clip_features(bpe_file, scale_file, tmp_path):
    from freepose_amd import ops
    from freepose_amd.src.pipeline.estimators.scale_estimators import GPT4ScaleEstimator
    from freepose_amd.src.pipeline.retrieval.clip import CLIPFeatureExtractor
    clip = CLIPFeatureExtractor("tiny-64", seed=4, allow_random_weights=True, bpe_vocab=str(bpe_file))
    assert clip.has_text_tower
    feats_path = tmp_path / "scale_feats.pt"
    out = GPT4ScaleEstimator.generate_clip_features(str(scale_file), clip, feats_path=str(feats_path))
    table = json.loads(scale_file.read_text())
    feats, scales = out["feats"], out["scales"]
    assert feats.dtype == torch.float32 and feats.device.type == "cpu" and tuple(feats.shape) == (40, 64)
    assert scales.dtype == torch.float32 and torch.equal(scales, torch.tensor(list(table.values()), dtype=torch.float32))
    # unit norm within bf16: the quotient of bf16 values by a bf16 norm, each rounded (8 significant bits)
    assert (feats.norm(dim=-1) - 1.0).abs().max().item() <= 2.0 ** -7
    ids = clip.tokenizer(list(table))
    sd = {k: v.float() for k, v in ops.random_clip_text_state_dict("tiny-64", 4).items()}
    ref = tr.clip_text_forward(sd, ids, ops.CLIP_TEXT_ARCHS["tiny-64"][2])
    cos = torch.nn.functional.cosine_similarity(feats, ref, dim=-1).min().item()
    print("scale table vs the restatement: min cosine", cos)
    assert cos >= 0.999
    # the saved file, reloaded, is the same table and finds the same neighbours
    saved = torch.load(feats_path, map_location="cpu")
    assert torch.equal(saved["feats"], feats) and torch.equal(saved["scales"], scales)
    est_mem = GPT4ScaleEstimator(clip, query_k=4, scale_file=str(scale_file), feats_path=None)
    est_file = GPT4ScaleEstimator(clip, query_k=4, feats_path=str(feats_path))
    g = torch.Generator().manual_seed(3)
    q = torch.nn.functional.normalize(torch.randn((6, 64), generator=g), dim=-1).cuda()
    assert np.array_equal(est_mem.neighbours(q), est_file.neighbours(q))
    assert np.array_equal(est_file.neighbours(q), cr.knn_f64(feats.numpy(), q.cpu().numpy(), 4)[0])


def test_compute_scale_cli_builds_the_table(bpe_file, scale_file, tmp_path_factory, monkeypatch):
    """--scale_file: the table is computed at start-up and written to --scale_feats; a second run that only reads it gives the same bytes"""
    from PIL import Image
    from tests import _synth_scene as sc
    from scripts import compute_scale as cs
    root = tmp_path_factory.mktemp("scale_ws_text")
    sc.write_meshes(root)
    frames, props, _, K = sc.draw_frames(root, 2, 64)
    for fr in props:
        for e in fr:
            e.pop("scale", None)
    sc.write_bop(root, "synth", frames, props, K)
    dp = root / "data" / "datasets" / "synth" / "test" / "000048" / "depth_pred"
    dp.mkdir()
    for i, d in enumerate(sc.draw_frames.depths):     # the predicted-depth convention of the reference's BOPDataset: 16-bit PNG, value / 65535
        Image.fromarray(np.round(d / 2.0 * 65535.0).astype(np.uint16)).save(dp / f"{i + 1:06d}.png")
    monkeypatch.chdir(root)
    feats = root / "data" / "scale_feats.pt"
    argv = ["--dataset", "synth", "--proposals", "props.json", "--clip_model", "tiny-64", "--allow_random_weights"]
    out = cs.run(argv + ["--scale_file", str(scale_file), "--bpe_vocab", str(bpe_file)])
    assert out.is_file() and feats.is_file()
    table = torch.load(feats, map_location="cpu")
    assert tuple(table["feats"].shape) == (40, 64) and tuple(table["scales"].shape) == (40,)
    text_1 = out.read_text()
    assert all(isinstance(p["scale"], float) for p in json.loads(text_1))
    out.unlink()
    assert cs.run(argv).read_text() == text_1
    # two ranks: rank 0 computes and writes the table, rank 1 waits for it and loads the file; the same bytes, table included
    out.unlink()
    feats.unlink()
    env = dict(os.environ, FP_DIST_BACKEND="gloo", FP_ALLOW_SHARED_GPU="1", MASTER_ADDR="127.0.0.1", PYTHONPATH=str(tr.ROOT))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29771",
           "-m", "scripts.compute_scale"] + argv + ["--scale_file", str(scale_file), "--bpe_vocab", str(bpe_file)]
    r = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert out.read_text() == text_1 and torch.equal(torch.load(feats, map_location="cpu")["feats"], table["feats"])
