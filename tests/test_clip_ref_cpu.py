"""No-GPU checks of the CLIP / GPT4ScaleEstimator references the GPU tests lean on, and of the new kernels' compiled resources."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _clip_ref as cr

ROOT = Path(__file__).resolve().parent.parent
TINY = dict(width=128, depth=2, heads=2, mlp_dim=512, embed_dim=64, patch=14, grid=4)


def _tiny_sd(seed=3):
    from freepose_amd import ops
    return {k: v.float() for k, v in ops.random_clip_state_dict("tiny-64-s56", seed).items()}


def test_feature_is_present():
    """fails without the feature: the extractor's import path and the estimator class"""
    from src.pipeline.retrieval.clip import CLIPFeatureExtractor
    from freepose_amd.src.pipeline.estimators import scale_estimators
    assert CLIPFeatureExtractor is not None and hasattr(scale_estimators, "GPT4ScaleEstimator")
    from freepose_amd import _lib
    assert "fp_op_attention_hd" in _lib.SIGNATURES and hasattr(_lib.load(), "fp_op_attention_hd")


def test_state_dict_mapping_is_a_bijection():
    from freepose_amd import ops
    names = ops.clip_state_dict_names("tiny-64-s56")
    m = cr.hf_name_map(TINY["depth"])
    assert set(m) == set(names)
    hf_targets = [t[0] for ts in m.values() for t in ts]
    assert len(hf_targets) == len(set(hf_targets))
    model = cr.hf_model(_tiny_sd(), **TINY)
    params = {k for k in model.state_dict() if "position_ids" not in k}
    assert set(hf_targets) == params
    sd = _tiny_sd()
    hf = cr.to_hf(sd, TINY["depth"])
    assert sum(v.numel() for v in hf.values()) == sum(v.numel() for v in sd.values())
    back = torch.cat([hf[f"vision_model.encoder.layers.0.self_attn.{n}_proj.weight"] for n in "qkv"])
    assert torch.equal(back, sd["transformer.resblocks.0.attn.in_proj_weight"])


def test_restatement_matches_transformers():
    """the fp32 restatement equals transformers' CLIPVisionModelWithProjection on the same weights to <= 1e-4 relative"""
    sd = _tiny_sd()
    model = cr.hf_model(sd, **TINY)
    g = torch.Generator().manual_seed(5)
    x = cr.normalize_bf16(torch.rand((3, 3, 56, 56), generator=g)).float()
    with torch.no_grad():
        ref = model(pixel_values=x).image_embeds
    got = cr.clip_forward(sd, x, TINY["heads"])
    rel = ((got - ref).norm() / ref.norm()).item()
    print("restatement vs transformers: relative", rel)
    assert rel <= 1e-4


def test_gpt4_scale_reference_matches_the_reference_class():
    """tests/golden/gpt4_scale.npz holds what the reference's own GPT4ScaleEstimator returned on CPU for planted inputs (a stand-in
    clip returning the planted bf16 features; with depth, planted point clouds in place of generate_pointcloud, whose skimage calls
    cannot run in this image): no-depth, depth-corrected and one-mask cases at query_k 11, 1 and 4"""
    g = np.load(ROOT / "tests" / "golden" / "gpt4_scale.npz")
    f = torch.from_numpy(g["feats_bf16_bits"].view(np.int16)).view(torch.bfloat16)
    f = (f / f.norm(dim=-1, keepdim=True)).float().numpy()            # reference :63-64
    for k in (11, 1, 4):
        out, idx, _ = cr.gpt4_scale_ref(f, g["table"], g["scales"], k)
        np.testing.assert_allclose(out, g[f"nodepth_k{k}"], rtol=1e-6)
        out, _, _ = cr.gpt4_scale_ref(f, g["table"], g["scales"], k, depth_scales=g["planted_depth_scales"])
        np.testing.assert_allclose(out, g[f"depth_k{k}"], rtol=1e-6)
    out, _, _ = cr.gpt4_scale_ref(f[:1], g["table"], g["scales"], 11)
    np.testing.assert_allclose(out, g["onemask_depth_k11"], rtol=1e-6)   # one mask: depth given but unused
    idx, _ = cr.knn_f64(g["table"], f[1:2], 4)
    assert idx[0, :3].tolist() == [3, 7, 21]                             # the planted duplicates, in index order


def test_text_side_and_missing_checkpoint_fail_closed(tmp_path, monkeypatch):
    from freepose_amd.src.pipeline.retrieval.clip import CLIPFeatureExtractor, visual_state_dict
    from freepose_amd.src.pipeline.estimators.scale_estimators import GPT4ScaleEstimator
    monkeypatch.setenv("FREEPOSE_CLIP_WEIGHTS", str(tmp_path / "nowhere.pt"))
    monkeypatch.delenv("FREEPOSE_ALLOW_RANDOM_WEIGHTS", raising=False)
    with pytest.raises(FileNotFoundError, match="allow_random_weights"):
        CLIPFeatureExtractor("ViT-L-14")
    with pytest.raises(NotImplementedError, match="text tower"):
        GPT4ScaleEstimator(None, scale_file="scales.json")
    with pytest.raises(NotImplementedError, match="text tower"):
        GPT4ScaleEstimator.generate_clip_features("scales.json", None)
    full = {"visual.proj": torch.zeros(2, 2), "text_projection": torch.zeros(2, 2), "visual.conv1.weight": torch.zeros(1)}
    assert sorted(visual_state_dict(full)) == ["conv1.weight", "proj"]
    assert sorted(visual_state_dict({"state_dict": {"module.visual.proj": torch.zeros(1)}})) == ["proj"]
    assert GPT4ScaleEstimator.mask_to_bbox(torch.tensor([[0, 0, 0], [0, 1, 1], [0, 0, 0]]).bool()) == (1, 1, 1, 2)


def test_attention_hd_kernels_have_no_scratch(tmp_path):
    """the four non-causal instantiations (padded head dimension 32 / 64 / 96 / 128) compile to zero scratch and no spills, read from the code
    object's metadata notes like the DINOv2 attention kernels in test_capi_cpu.py"""
    llvm = Path("/opt/rocm/lib/llvm/bin")
    if not (llvm / "clang-offload-bundler").exists() or not (llvm / "llvm-readelf").exists():
        pytest.skip("ROCm LLVM tools not found")
    from freepose_amd import build
    build.build_hip(verbose=False)
    obj = ROOT / "freepose_amd" / "lib" / "obj" / "attention_hd.o"
    fat, co = tmp_path / "a.fatbin", tmp_path / "a.co"
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
    attn = {k: v for k, v in kernels.items() if "attn_hd_kernel" in k and "Lb0" in k}   # CAUSAL = false
    assert len(attn) == 4, sorted(kernels)
    for k, v in attn.items():
        print(k, v)
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["vgpr_count"] <= 256, (k, v)


def test_attention_index_arithmetic_under_the_host_sanitizers(tmp_path):
    """tools/attn_hd_host_check.cpp replays the staging, fragment and mask arithmetic of csrc/attn_hd_core.h — the functions the kernel
    itself calls — on host images of the LDS tiles, as a stand-alone program built with -fsanitize=address,undefined"""
    import shutil
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path / "attn_hd_host_check"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "freepose_amd" / "csrc"),
                        str(ROOT / "tools" / "attn_hd_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "attn_hd_host_check: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    # the kernel takes its offsets from the header, not from expressions of its own
    src = (ROOT / "freepose_amd" / "csrc" / "attention_hd.hip").read_text()
    for fn in ("fp_ahd_kstage_key", "fp_ahd_kstage_d0", "fp_ahd_kstage_off", "fp_ahd_vstage_pair", "fp_ahd_vstage_d0", "fp_ahd_vstage_off",
               "fp_ahd_kfrag_off", "fp_ahd_vfrag_off", "fp_ahd_k_pitch", "fp_ahd_acc_key", "fp_ahd_row_real", "fp_ahd_chunk_real"):
        assert fn + "(" in src, fn


def test_seed_alone_does_not_allow_random_weights(tmp_path, monkeypatch):
    import inspect
    from freepose_amd.src.pipeline.retrieval.clip import CLIPFeatureExtractor
    sig = inspect.signature(CLIPFeatureExtractor.__init__).parameters
    assert list(sig)[1:5] == ["model_name", "pretrained", "state_dict", "seed"] and sig["seed"].default == 0
    monkeypatch.setenv("FREEPOSE_CLIP_WEIGHTS", str(tmp_path / "nowhere.pt"))
    monkeypatch.delenv("FREEPOSE_ALLOW_RANDOM_WEIGHTS", raising=False)
    with pytest.raises(FileNotFoundError, match="allow_random_weights"):
        CLIPFeatureExtractor("tiny-64", seed=3)


def test_compute_scale_clis_surface(tmp_path):
    """flags, output names, the per-object median and the predicted-depth key of the dataset mirror (no GPU)"""
    import scripts.compute_scale as alias
    import scripts.compute_scale_video as alias_v
    from freepose_amd.scripts import compute_scale as cs, compute_scale_video as csv_
    from PIL import Image
    assert alias.run is cs.run and alias_v.run is csv_.run and cs.OUT_SUFFIX == "_gpt4_scaled.json"
    a = cs.build_parser().parse_args(["--dataset", "ycbv", "--proposals", "p.json"])
    assert (a.split, a.clip_model, a.scale_feats, a.allow_random_weights, a.query_k, a.no_depth) == ("test", "ViT-bigG-14", "data/scale_feats.pt", False, 11, False)
    v = csv_.build_parser().parse_args(["--video", "c", "--proposals", "p.json", "--depth_dir", "d", "--clip_model", "ViT-L-14", "--allow_random_weights"])
    assert (v.depth_dir, v.clip_model, v.allow_random_weights, v.scale_feats) == ("d", "ViT-L-14", True, "data/scale_feats.pt")
    assert csv_.build_parser().parse_args(["--video", "c", "--proposals", "p.json"]).depth_dir is None
    assert "ZoeDepth" in csv_.build_parser().format_help() and "NO depth correction" in csv_.build_parser().format_help()
    # frame-major, 2 objects, 4 frames: numpy's median averages the middle two
    assert csv_.object_medians([1.0, 10.0, 3.0, 30.0, 2.0, 20.0, 8.0, 80.0], 2) == [2.5, 25.0] * 4
    assert csv_.object_medians([1.0, 5.0, 2.0, 9.0, 7.0, 6.0], 2) == [2.0, 6.0] * 3
    # BOPDataset: depth_pred/<frame>.png, 16-bit / 65535, as an additional key only
    from freepose_amd.src.dataloader.bop import BOPDataset
    sd = tmp_path / "ds" / "test" / "000001"
    (sd / "rgb").mkdir(parents=True)
    Image.fromarray(np.zeros((4, 6, 3), np.uint8)).save(sd / "rgb" / "000003.png")
    (sd / "scene_camera.json").write_text('{"3": {"cam_K": [1, 0, 0, 0, 1, 0, 0, 0, 1]}}')
    assert sorted(BOPDataset(str(tmp_path / "ds"), "test")[0]) == ["frame_id", "image", "intrinsic", "scene_id"]
    (sd / "depth_pred").mkdir()
    Image.fromarray(np.full((4, 6), 13107, np.uint16)).save(sd / "depth_pred" / "000003.png")
    e = BOPDataset(str(tmp_path / "ds"), "test")[0]                  # (the index file written by the first open is still valid)
    assert sorted(e) == ["depth_pred", "frame_id", "image", "intrinsic", "scene_id"] and np.allclose(e["depth_pred"], 0.2) and e["depth_pred"].shape == (4, 6)
