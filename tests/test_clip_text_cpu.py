"""No-GPU checks of the CLIP text tower's references, of the tokenizer and of the new kernels' compiled resources."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from tests import _clip_text_ref as tr

ROOT = Path(__file__).resolve().parent.parent
TINY = "tiny-64"
HAND_MADE = ["A Photo OF a Cat", "two   spaces \t and\na newline", "cat's", "abc 123 4", "wow!!", "(a-b)", "naïve", "it's done, isn't it?"]


def _tiny_sd(seed=3):
    from freepose_amd import ops
    return {k: v.float() for k, v in ops.random_clip_text_state_dict(TINY, seed).items()}


def test_feature_is_present():
    """fails without the feature: the entry points in the header, the binding table and the library, and the text arch table"""
    from freepose_amd import _lib, ops
    header = (ROOT / "include" / "freepose_hip.h").read_text()
    lib = _lib.load()
    for fn in ("fp_op_attention_causal", "fp_clip_text_encode", "fp_clip_text_create", "fp_clip_text_destroy", "fp_clip_text_set_weight",
               "fp_clip_text_flops"):
        assert re.search(r"\b%s\(" % fn, header), fn
        assert fn in _lib.SIGNATURES and hasattr(lib, fn), fn
    for name, row in {"ViT-bigG-14": (1280, 32, 20, 5120, 49408, 77, 1280), "ViT-H-14": (1024, 24, 16, 4096, 49408, 77, 1024),
                      "ViT-L-14": (768, 12, 12, 3072, 49408, 77, 768)}.items():
        assert ops.CLIP_TEXT_ARCHS[name] == row
    for name in ops.CLIP_ARCHS:                      # every image tower has its text tower, with the same embedding size
        assert ops.CLIP_TEXT_ARCHS[name][6] == ops.CLIP_ARCHS[name][4], name
        if name.startswith("tiny-"):
            assert ops.CLIP_TEXT_ARCHS[name][4:6] == (1024, 77) and ops.CLIP_TEXT_ARCHS[name][1] == 2
    assert ops.CLIP_TEXT_ARCHS["tiny-64-c17"][5] == 17 and ops.CLIP_TEXT_ARCHS["tiny-bigG-text"][:4] == (1280, 1, 20, 256)
    assert len(next(iter(ops.CLIP_ARCHS.values()))) == 7          # the image table keeps its 7-tuples
    assert callable(ops.attention_causal) and callable(ops.ClipText)


def test_state_dict_mapping_is_a_bijection():
    from freepose_amd import ops
    width, depth, heads, mlp, vocab, ctx, embed = ops.CLIP_TEXT_ARCHS[TINY]
    names = ops.clip_text_state_dict_names(TINY)
    m = tr.hf_name_map(depth)
    assert set(m) == set(names)
    hf_targets = [t[0] for ts in m.values() for t in ts]
    assert len(hf_targets) == len(set(hf_targets))
    sd = _tiny_sd()
    assert {k: tuple(v.shape) for k, v in sd.items()} == names
    model = tr.hf_model(sd, width, depth, heads, mlp, vocab, ctx, embed)
    params = {k for k in model.state_dict() if "position_ids" not in k}
    assert set(hf_targets) == params
    hf = tr.to_hf(sd, depth)
    assert sum(v.numel() for v in hf.values()) == sum(v.numel() for v in sd.values())
    back = torch.cat([hf[f"text_model.encoder.layers.0.self_attn.{n}_proj.weight"] for n in "qkv"])
    assert torch.equal(back, sd["transformer.resblocks.0.attn.in_proj_weight"])


def test_restatement_matches_transformers():
    """the fp32 restatement equals transformers' CLIPTextModelWithProjection on the same weights to <= 1e-4 relative, for prompts of
    1, 5 and 75 tokens; neither side looks at the ids after the end-of-text token"""
    from freepose_amd import ops
    width, depth, heads, mlp, vocab, ctx, embed = ops.CLIP_TEXT_ARCHS[TINY]
    sd = _tiny_sd()
    model = tr.hf_model(sd, width, depth, heads, mlp, vocab, ctx, embed)
    ids = tr.make_ids([1, 5, 75], vocab, ctx, seed=5)
    with torch.no_grad():
        ref = model(input_ids=ids).text_embeds
    got = tr.clip_text_forward(sd, ids, heads)
    rel = ((got - ref).norm() / ref.norm()).item()
    print("restatement vs transformers: relative", rel)
    assert rel <= 1e-4
    other = ids.clone()
    other[0, 3:] = 7
    other[1, 7:] = torch.arange(ctx - 7) + 1
    with torch.no_grad():
        assert (model(input_ids=other).text_embeds - ref).abs().max().item() == 0.0
    assert torch.equal(tr.clip_text_forward(sd, other, heads), got)


# ---- tokenizer --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vocab_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("bpe")
    return tr.write_bpe_file(d / "bpe_synth.txt.gz"), tr.write_bpe_file(d / "bpe_synth.txt")


def test_synthetic_vocabulary_is_deterministic_and_fits_the_tiny_towers():
    from freepose_amd import ops
    merges = tr.learn_merges()
    assert 200 <= len(merges) <= 510 and len(set(merges)) == len(merges)
    assert len(tr.open_clip_vocab(merges)) <= ops.CLIP_TEXT_ARCHS[TINY][4]
    names, sizes = tr.fixture_names()
    assert len(names) == 2201 and len(sizes) == 2201 and all(n.isascii() for n in names) and min(sizes) > 0


def test_tokenizer_matches_transformers(vocab_files):
    from freepose_amd.clip_tokenizer import SimpleTokenizer
    tok = SimpleTokenizer(vocab_files[0])
    hf = tr.hf_tokenizer()
    nm = len(tr.learn_merges())
    assert tok.vocab_size == 512 + nm + 2 and (tok.sot_token_id, tok.eot_token_id) == (512 + nm, 512 + nm + 1)
    texts = list(tr.fixture_names()[0]) + HAND_MADE
    rows = tok(texts)
    assert rows.dtype == torch.long and tuple(rows.shape) == (len(texts), 77)
    merged = 0
    for text, row in zip(texts, rows.tolist()):
        want = hf(text, add_special_tokens=False)["input_ids"]
        assert tok.encode(text) == want, text
        assert row[:len(want) + 2] == [tok.sot_token_id] + want + [tok.eot_token_id], text      # ids between BOS and EOS
        assert not any(row[len(want) + 2:]), text                                                # zero padding
        merged += any(i >= 512 for i in want)
    assert merged > 2000                                  # the merges are in play, not only byte symbols
    assert hf("a cat")["input_ids"] == tok("a cat")[0, :5].tolist()   # BOS / EOS ids agree as well


def test_tokenizer_padding_truncation_and_files(vocab_files, tmp_path, monkeypatch):
    from freepose_amd import clip_tokenizer as ct
    tok = ct.SimpleTokenizer(vocab_files[0])
    empty = tok([""])[0].tolist()
    assert empty == [tok.sot_token_id, tok.eot_token_id] + [0] * 75
    long = " ".join(["zq"] * 100)                         # at least 100 tokens
    assert len(tok.encode(long)) >= 100
    row = tok([long])[0].tolist()
    assert len(row) == 77 and row[0] == tok.sot_token_id and row[-1] == tok.eot_token_id and row[1:76] == tok.encode(long)[:75]
    short = tok([long], context_length=17)
    assert short.shape == (1, 17) and short[0, -1].item() == tok.eot_token_id and short[0, :16].tolist() == row[:16]
    # .txt == .txt.gz, by argument and by the environment variable
    texts = list(tr.fixture_names()[0][:50]) + HAND_MADE
    assert torch.equal(ct.SimpleTokenizer(vocab_files[1])(texts), tok(texts))
    monkeypatch.setenv(ct.BPE_ENV, str(vocab_files[1]))
    assert torch.equal(ct.SimpleTokenizer()(texts), tok(texts))
    # no file, no tokenizer: the error names the file and where it comes from
    monkeypatch.delenv(ct.BPE_ENV)
    with pytest.raises(FileNotFoundError, match="open_clip"):
        ct.SimpleTokenizer()
    with pytest.raises(FileNotFoundError, match="nowhere.txt.gz.*bpe_simple_vocab_16e6"):
        ct.SimpleTokenizer(tmp_path / "nowhere.txt.gz")
    assert ct.N_MERGES == 48894
    assert ct.clean_text("  A &amp;lt; B \n c ") == "a < b c"


# ---- compiled resources and index arithmetic --------------------------------------------------------------------------------------------------
def _kernel_notes(obj: Path, tmp_path):
    llvm = Path("/opt/rocm/lib/llvm/bin")
    if not (llvm / "clang-offload-bundler").exists() or not (llvm / "llvm-readelf").exists():
        pytest.skip("ROCm LLVM tools not found")
    fat, co = tmp_path / (obj.stem + ".fatbin"), tmp_path / (obj.stem + ".co")
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(obj), str(fat)], check=True)
    subprocess.run([str(llvm / "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950:sramecc+", f"--input={fat}",
                    f"--output={co}", "--unbundle"], check=True)
    notes = subprocess.run([str(llvm / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True, check=True).stdout
    kernels, name = {}, None
    for ln in notes.splitlines():
        m = re.search(r"\.name:\s+(\S+)", ln)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count"):
            m = re.search(r"\.%s:\s+(\d+)" % key, ln)
            if m and name:
                kernels[name][key] = int(m.group(1))
    return kernels


def test_new_kernels_have_no_scratch(tmp_path):
    """the eight instantiations of the general-head attention kernel (padded head dimension 32 / 64 / 96 / 128, causal and not), the
    text tower's gathers and the projection transpose compile to zero scratch and no spills, read from the code objects' metadata
    notes; attention_hd.o holds exactly those eight"""
    from freepose_amd import build
    build.build_hip(verbose=False)
    obj = ROOT / "freepose_amd" / "lib" / "obj"
    attn = {k: v for k, v in _kernel_notes(obj / "attention_hd.o", tmp_path).items() if "attn_hd_kernel" in k}
    assert len(attn) == 8, sorted(attn)
    assert len([k for k in attn if "Lb1" in k]) == 4 and len([k for k in attn if "Lb0" in k]) == 4, sorted(attn)   # CAUSAL = true / false
    text = _kernel_notes(obj / "clip_text.o", tmp_path)
    gathers = {k: v for k, v in text.items() if "text_embed_kernel" in k or "text_pool_kernel" in k}
    assert len(gathers) == 2, sorted(text)
    misc = _kernel_notes(obj / "vit_misc.o", tmp_path)
    transpose = {k: v for k, v in misc.items() if "transpose_bf16_kernel" in k}
    assert len(transpose) == 1, sorted(misc)
    for k, v in {**attn, **gathers, **transpose}.items():
        print(k, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 256, (k, v)


def test_causal_index_arithmetic_under_the_host_sanitizers(tmp_path):
    """tools/attn_causal_host_check.cpp replays the tile walk and the visibility predicate of csrc/attn_hd_core.h — the functions the
    kernel itself calls — as a stand-alone program built with -fsanitize=address,undefined"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path / "attn_causal_host_check"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "freepose_amd" / "csrc"),
                        str(ROOT / "tools" / "attn_causal_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "attn_causal_host_check: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    csrc = ROOT / "freepose_amd" / "csrc"
    src = (csrc / "attention_hd.hip").read_text()
    for fn in ("fp_ahd_causal_num_tiles", "fp_ahd_causal_visible", "fp_ahd_kstage_off", "fp_ahd_vstage_off", "fp_ahd_kfrag_off", "fp_ahd_vfrag_off",
               "fp_ahd_acc_key", "fp_ahd_row_real", "fp_ahd_chunk_real"):
        assert fn + "(" in src, fn
    assert not (csrc / "attention_causal.hip").exists()


# ---- fail closed ----------------------------------------------------------------------------------------------------------------------------
def test_text_state_dict_selection():
    from freepose_amd import ops
    from freepose_amd.src.pipeline.retrieval.clip import text_state_dict, visual_state_dict
    text = {k: torch.zeros(1) for k in ops.clip_text_state_dict_names(TINY)}
    visual = {"visual." + k: torch.ones(1) for k in ops.clip_state_dict_names(TINY)}
    full = {**visual, **text, "logit_scale": torch.zeros(())}
    assert set(text_state_dict(full)) == set(text) and all(v.item() == 0 for v in text_state_dict(full).values())
    assert set(visual_state_dict(full)) == set(ops.clip_state_dict_names(TINY))
    assert set(text_state_dict({"state_dict": {"module." + k: v for k, v in full.items()}})) == set(text)
    prefixed = {**visual, **{"text." + k: v for k, v in text.items()}, "logit_scale": torch.zeros(())}
    assert set(text_state_dict(prefixed)) == set(text)
    # no text side: a visual-only state dict (whose transformer.* is the IMAGE tower's), a visual.-prefixed one, an empty one
    assert text_state_dict({k: torch.ones(1) for k in ops.clip_state_dict_names(TINY)}) == {}
    assert text_state_dict(visual) == {} and text_state_dict({}) == {}


def test_parsers_keep_their_defaults_and_gain_the_text_flags():
    from freepose_amd.scripts import compute_scale as cs, compute_scale_video as csv_
    a = cs.build_parser().parse_args(["--dataset", "ycbv", "--proposals", "p.json"])
    assert (a.split, a.clip_model, a.scale_feats, a.allow_random_weights, a.query_k, a.no_depth) == ("test", "ViT-bigG-14", "data/scale_feats.pt", False, 11, False)
    assert a.scale_file is None and a.bpe_vocab is None
    v = csv_.build_parser().parse_args(["--video", "c", "--proposals", "p.json"])
    assert (v.depth_dir, v.clip_model, v.scale_feats, v.scale_file, v.bpe_vocab) == (None, "ViT-bigG-14", "data/scale_feats.pt", None, None)
    for parser, base in ((cs.build_parser(), ["--dataset", "d", "--proposals", "p.json"]), (csv_.build_parser(), ["--video", "c", "--proposals", "p.json"])):
        b = parser.parse_args(base + ["--scale_file", "data/gpt4_scales.json", "--bpe_vocab", "bpe.txt.gz"])
        assert (b.scale_file, b.bpe_vocab) == ("data/gpt4_scales.json", "bpe.txt.gz")
        assert "--scale_file" in parser.format_help() and "--bpe_vocab" in parser.format_help()


def test_estimator_refuses_before_touching_the_scale_file(tmp_path):
    import types
    from freepose_amd.src.pipeline.estimators.scale_estimators import GPT4ScaleEstimator
    missing = str(tmp_path / "no_such_scales.json")
    for clip in (None, types.SimpleNamespace(has_text_tower=False), object()):
        with pytest.raises(NotImplementedError, match="text tower"):
            GPT4ScaleEstimator.generate_clip_features(missing, clip)
        with pytest.raises(NotImplementedError, match="text tower"):
            GPT4ScaleEstimator(clip, scale_file=missing)
