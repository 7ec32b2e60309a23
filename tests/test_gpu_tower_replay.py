"""The tower drivers held to a step-by-step replay of the model, bit for bit.

fp_vit_forward, fp_clip_encode_image and fp_clip_text_encode wire kernels together that all have exact-answer tests of their own; the
end-to-end tests see the wiring only through an aggregate tolerance (cosine 0.999, relative L2 2e-2 after up to 22 blocks).  Here every
driver call is followed by tests/_tower_replay.py's replay of the same forward on kernel-level ops, written from the model definition,
and the driver's output AND every workspace buffer its last block touched must carry the replay's bits (all B * npad rows, pad rows
included).  A wiring or state error — a LayerScale swapped, statistics of the wrong block, stale folded weights after a reload, a stale
position cache — changes bits.  A mismatch names the first buffer in forward order that differs and its first differing row.

  test_vit_forward_is_its_replay        sizes 14^2 / 28x42 / 224^2 / 518^2, B 1 / 3, layers 1-3 (and 0 / 12 / 99), four feature types, folded and
                                        separate LayerNorm, both statistics routes
  test_vit_large_batches                8192 and 16384 rows: who finalises the row sums
  test_vit_replay_meets_the_oracle_bar  the replay itself against oracle/vit_ref.py in fp32 (the bar of tests/test_gpu_vit.py)
  test_vit_state_*                      incremental fold, re-fold after a reload, position cache, streams, workspaces regrown and shared, ln_fused
  test_clip_visual_is_its_replay, test_clip_text_is_its_replay
  test_*_fault_is_visible               each wiring fault injected into the replay must change bits: the inputs distinguish what matters

The one step without a kernel-level entry is the CLIP image tower's normalise + unfold (fp_op_im2col_norm carries the ImageNet
constants): the replay states it as torchvision's two bf16 operations in torch, the reference tests/test_gpu_kernels.py pins the
ImageNet form to with no tolerance, and `clip.im2col` is compared with it bit for bit like every other buffer.
"""
import numpy as np
import pytest
import torch

from tests import _tower_replay as tr

pytestmark = pytest.mark.gpu

MODEL = "dinov2_vits14_reg"     # the smallest shipped arch: dim 384, 6 heads, 12 blocks, 4 registers
D, HEADS, N_REG, KP = 384, 6, 4, 640
FEATURES = ("cls", "reg", "patch", "patch_normalized")


def _ops():
    from freepose_amd import ops
    return ops


@pytest.fixture(scope="module")
def vit_sd_cpu():
    """LayerScale != 1 and uneven, LayerNorm gains over an order of magnitude with non-zero shifts, massive channels"""
    return tr.massive_state_dict(MODEL, 5)


@pytest.fixture(scope="module")
def vit_sd(vit_sd_cpu):
    """the same on the device: what the towers and the replays are given (uploaded once)"""
    return {k: v.cuda() for k, v in vit_sd_cpu.items()}


@pytest.fixture(scope="module")
def vit(vit_sd):
    return _ops().ViT(MODEL, vit_sd)


def _geom(B, H, W):
    P = (H // 14) * (W // 14)
    n_tok = P + 1 + N_REG
    npad = tr.cdiv(n_tok, 16) * 16
    return P, n_tok, npad, B * npad


def _vit_buffers(B, H, W, names):
    """what fp_vit_forward left in the context's workspaces, over the extent this call used"""
    ops = _ops()
    P, _, npad, M = _geom(B, H, W)
    shapes = {"im2col": (B * P, KP), "x": (M, D), "y": (M, D), "qk": (M, 2 * D), "vt": (B, HEADS, 64, npad), "ao": (M, D), "h1": (M, 4 * D)}
    return {n: ops.workspace_read("vit." + n, shapes[n]) for n in names}


def _hold(what, order, drv_out, drv_bufs, rep_out, rep_bufs):
    """the driver's buffers and output carry the replay's bits; the first buffer in forward order that does not is named"""
    for name in order:
        if name in rep_bufs:
            diff = tr.first_difference(drv_bufs[name], rep_bufs[name])
            assert diff is None, f"{what}: first differing buffer '{name}': {diff}"
    diff = tr.first_difference(drv_out, rep_out)
    assert diff is None, f"{what}: the buffers agree, the output differs: {diff}"


def _vit_check(vit, sd, img, layer, ft, ln_fused, route=None, what=""):
    """one driver call against its replay (the context's ln_fused option is the caller's to set); returns the driver's output"""
    B, _, H, W = img.shape
    got = vit(img, layer=layer, feature_type=ft)
    torch.cuda.synchronize()
    rep_out, rep = tr.replay_vit(sd, img, layer, ft, ln_fused, route=route)
    drv = _vit_buffers(B, H, W, [n for n in tr.VIT_ORDER if n in rep])
    _hold(f"{what} {H}x{W} B={B} layer={layer} {ft} ln_fused={ln_fused} route={route}", tr.VIT_ORDER, got, drv, rep_out, rep)
    return got


class _LnFused:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        _ops().set_option("ln_fused", self.value)

    def __exit__(self, *exc):
        _ops().set_option("ln_fused", -1)


# ---- a. the ViT ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln_fused", [1, 0], ids=["folded", "separate"])
@pytest.mark.parametrize("H,W,B", [(14, 14, 1), (14, 14, 3), (28, 42, 1), (28, 42, 3), (224, 224, 1), (224, 224, 3), (518, 518, 1)])
def test_vit_forward_is_its_replay(vit, vit_sd, H, W, B, ln_fused):
    """14^2: 1 patch, 6 tokens in 16 rows; 28x42: non-square, position rows resized, 11 tokens; 224^2: 261 tokens in 272 rows; 518^2: the
    native 37 x 37 grid, no resize, 1374 tokens in 1376 rows.  At 14^2 also layer 0 / 12 / 99: all twelve blocks (dino.py:18-21)."""
    img = tr.smooth_images(B, H, W, 11).cuda()
    layers = (1, 2, 3) + ((0, 12, 99) if H == 14 else ())
    with _LnFused(ln_fused):
        for layer in layers:
            for ft in FEATURES:
                _vit_check(vit, vit_sd, img, layer, ft, ln_fused)
            if ln_fused:                                     # the driver's bits do not depend on who finalises the row sums
                for route in (0, 1):
                    _vit_check(vit, vit_sd, img, layer, "patch", ln_fused, route=route)


@pytest.mark.parametrize("B,fc1_pending,qk_pending", [(512, False, True), (1024, False, False)])
def test_vit_large_batches(vit, vit_sd, B, fc1_pending, qk_pending):
    """8192 rows: fc1 (1536 wide) can reach the big tile tier, so its records are finalised by the stand-alone kernel, while qk's (768
    wide) ride along to the small tiers' prologue; 16384 rows: both are finalised up front"""
    M = _geom(B, 14, 14)[3]
    assert M == 16 * B and tr.sums_stay_pending(M, 4 * D) == fc1_pending and tr.sums_stay_pending(M, 2 * D) == qk_pending
    img = tr.smooth_images(B, 14, 14, 12).cuda()
    with _LnFused(1):
        _vit_check(vit, vit_sd, img, 2, "patch", 1)


@pytest.mark.parametrize("H,W", [(14, 14), (28, 42), (224, 224), (518, 518)])
def test_vit_replay_meets_the_oracle_bar(vit_sd, vit_sd_cpu, H, W):
    """ties the replay to the model: its patch features meet the bar tests/test_gpu_vit.py states for these weights against
    oracle/vit_ref.py in fp32 — cosine >= 0.995, rel <= 2 * rel(torch bf16 model) + 2e-3"""
    from oracle import vit_ref
    from tests.test_gpu_vit import _metrics
    img = tr.smooth_images(1, H, W, 11)
    sdf = {k: v.float() for k, v in vit_sd_cpu.items()}
    ref32 = vit_ref.vit_forward(sdf, img.float(), layer=3, feature_type="patch", dtype=torch.float32)
    ref16 = vit_ref.vit_forward(vit_sd_cpu, img.float(), layer=3, feature_type="patch", dtype=torch.bfloat16)
    c16, r16 = _metrics(ref16, ref32)
    for ln_fused in (1, 0):
        out, _ = tr.replay_vit(vit_sd, img, 3, "patch", ln_fused)
        cg, rg = _metrics(out, ref32)
        print(f"\n[anchor] {H}x{W} ln_fused={ln_fused}: replay vs fp32 cos {cg:.5f} rel {rg:.4f} | torch-bf16 vs fp32 cos {c16:.5f} rel {r16:.4f}")
        assert cg >= 0.995 and rg <= 2.0 * r16 + 2e-3, (H, W, ln_fused, cg, rg, c16, r16)


# ---- b. driver state -------------------------------------------------------------------------------------------------------------------
STATE_SIZES = pytest.mark.parametrize("H,W", [(28, 42), (224, 224)])


def _perturbed(t, seed, scale=0.5):
    g = torch.Generator().manual_seed(seed)
    dev, t = t.device, t.cpu()
    return (t.float() * (1.0 + scale * (torch.rand(t.shape, generator=g) - 0.5)) + 0.05 * torch.randn(t.shape, generator=g)).to(torch.bfloat16).to(dev)


@STATE_SIZES
def test_vit_state_fold_extended(vit_sd, H, W):
    """layer 2, then layer 4 on the same object: blocks 2 and 3 are folded behind blocks 0 and 1, which keep their fold"""
    vit = _ops().ViT(MODEL, vit_sd)
    img = tr.smooth_images(3, H, W, 13).cuda()
    with _LnFused(1):
        for layer in (2, 4, 2):
            _vit_check(vit, vit_sd, img, layer, "patch", 1, what="fold extended:")


@STATE_SIZES
def test_vit_state_refold_after_reload(vit_sd, H, W):
    """three tensors replaced through load_state_dict on a tower that has run: the LayerNorm gain and the fc1 weight live in folded copies,
    the LayerScale gamma is read in place.  The next forward is the replay with the weights then current, and a fresh tower's."""
    ops = _ops()
    vit = ops.ViT(MODEL, vit_sd)
    img = tr.smooth_images(3, H, W, 14).cuda()
    names = ("blocks.0.norm1.weight", "blocks.1.mlp.fc1.weight", "blocks.1.ls2.gamma")
    with _LnFused(1):
        before = _vit_check(vit, vit_sd, img, 3, "patch", 1, what="before the reload:").clone()
        sd2 = dict(vit_sd)
        for i, n in enumerate(names):
            sd2[n] = _perturbed(vit_sd[n], 20 + i)
            assert not torch.equal(sd2[n], vit_sd[n])
        vit.load_state_dict({n: sd2[n] for n in names})
        after = _vit_check(vit, sd2, img, 3, "patch", 1, what="after the reload:")
        assert not torch.equal(after, before)
        assert torch.equal(after.view(torch.int16), ops.ViT(MODEL, sd2)(img, layer=3, feature_type="patch").view(torch.int16))
        # one tensor at a time: each is observable on its own
        for n in names:
            sd3 = dict(sd2)
            sd3[n] = _perturbed(sd2[n], 30)
            vit.load_state_dict({n: sd3[n]})
            one = _vit_check(vit, sd3, img, 3, "patch", 1, what=f"after replacing {n}:")
            assert not torch.equal(one, after), n
            vit.load_state_dict({n: sd2[n]})


@STATE_SIZES
def test_vit_state_position_cache_dropped(vit_sd, H, W):
    """a forward at a non-native size caches the resized position rows; replacing pos_embed drops them (same size again) and the native
    size reads the new tensor directly"""
    ops = _ops()
    vit = ops.ViT(MODEL, vit_sd)
    img, native = tr.smooth_images(2, H, W, 15).cuda(), tr.smooth_images(1, 518, 518, 16).cuda()
    with _LnFused(1):
        before = _vit_check(vit, vit_sd, img, 2, "patch", 1, what="old pos_embed:").clone()
        _vit_check(vit, vit_sd, native, 1, "patch", 1, what="old pos_embed, native:")
        sd2 = dict(vit_sd, pos_embed=_perturbed(vit_sd["pos_embed"], 40))
        vit.load_state_dict({"pos_embed": sd2["pos_embed"]})
        after = _vit_check(vit, sd2, img, 2, "patch", 1, what="new pos_embed, same size:")
        assert not torch.equal(after, before)
        _vit_check(vit, sd2, native, 1, "patch", 1, what="new pos_embed, native:")
        assert torch.equal(after.view(torch.int16), ops.ViT(MODEL, sd2)(img, layer=2, feature_type="patch").view(torch.int16))


@STATE_SIZES
def test_vit_state_streams(vit_sd, H, W):
    """the fold is enqueued on the stream of the forward that needs it; a forward on another stream waits for it through an event, may
    extend it from there, and the first stream then waits in turn"""
    ops = _ops()
    vit = ops.ViT(MODEL, vit_sd)
    img = tr.smooth_images(3, H, W, 17).cuda()
    B = img.shape[0]
    names = [n for n in tr.VIT_ORDER if n != "y"]
    rep = {layer: tr.replay_vit(vit_sd, img, layer, "patch", 1) for layer in (2, 4)}
    other = torch.cuda.Stream()
    with _LnFused(1):
        _vit_check(vit, vit_sd, img, 2, "patch", 1, what="default stream, folds blocks 0-1:")
        other.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(other):
            for layer in (2, 4):                          # reads the fold made on the default stream, then extends it from here
                got = vit(img, layer=layer, feature_type="patch")
                other.synchronize()
                _hold(f"other stream, layer={layer}:", tr.VIT_ORDER, got, _vit_buffers(B, H, W, names), *rep[layer])
        torch.cuda.current_stream().wait_stream(other)
        _vit_check(vit, vit_sd, img, 4, "patch", 1, what="default stream again, fold extended from the other:")


def test_vit_state_workspaces_regrown_and_shared(vit_sd):
    """(B, size) = (3, 224^2), (1, 28x42), (3, 224^2) in one context with a CLIP image tower in between: the workspaces are grown, reused
    at a smaller extent with stale rows behind it, and the other tower allocates its own next to them"""
    ops = _ops()
    vit = ops.ViT(MODEL, vit_sd)
    clip_sd = ops.random_clip_state_dict("tiny-64-s56", seed=4)
    clip = ops.ClipVisual("tiny-64-s56", clip_sd)
    cimg = tr.smooth_images(3, 56, 56, 19).cuda()
    big, small = tr.smooth_images(3, 224, 224, 18).cuda(), tr.smooth_images(1, 28, 42, 18).cuda()
    with _LnFused(1):
        for i, img in enumerate((big, small, big, small)):
            _vit_check(vit, vit_sd, img, 2, "patch", 1, what=f"call {i}:")
            _clip_visual_check(clip, "tiny-64-s56", clip_sd, cimg)


@STATE_SIZES
def test_vit_state_ln_fused_flipped(vit, vit_sd, H, W):
    """the option is read per call: the folded and the separate LayerNorm alternate on one object, each its own replay"""
    ops = _ops()
    img = tr.smooth_images(3, H, W, 21).cuda()
    try:
        for ln_fused in (1, 0, 1, 0):
            ops.set_option("ln_fused", ln_fused)
            _vit_check(vit, vit_sd, img, 2, "patch", ln_fused, what="flipped:")
    finally:
        ops.set_option("ln_fused", -1)
    _vit_check(vit, vit_sd, img, 2, "patch", 1, what="default restored (folded):")


# ---- c. the CLIP towers ----------------------------------------------------------------------------------------------------------------
def _assert_layernorms_distinct(sd):
    """ops.random_clip_state_dict / random_clip_text_state_dict draw every LayerNorm's gain as 1 + N(0, 0.05) and its shift as N(0, 0.02),
    each independently: no two LayerNorms (ln_pre, ln_post / ln_final, every ln_1 / ln_2) share either, none is the identity — the
    seeded dicts are used as they are, and this holds them to it"""
    gains = {k: v for k, v in sd.items() if k.endswith(".weight") and v.dim() == 1 and ("ln_" in k)}
    assert len(gains) >= 3                                 # ln_final or ln_pre + ln_post, and ln_1 / ln_2 of at least one block
    keys = sorted(gains)
    for i, a in enumerate(keys):
        ga, ba = sd[a].float(), sd[a[:-len("weight")] + "bias"].float()
        assert (ga - 1.0).abs().max() > 0.05 and ba.abs().max() > 0.02, a
        for b in keys[i + 1:]:
            gb, bb = sd[b].float(), sd[b[:-len("weight")] + "bias"].float()
            assert (ga != gb).float().mean() > 0.5 and (ba != bb).float().mean() > 0.5, (a, b)


def _clip_visual_check(clip, name, sd, img):
    ops = _ops()
    width, depth, heads, mlp, embed, ps, grid = ops.CLIP_ARCHS[name]
    B = img.shape[0]
    P = grid * grid
    npad = tr.cdiv(P + 1, 16) * 16
    M = B * npad
    got = clip(img)
    torch.cuda.synchronize()
    rep_out, rep = tr.replay_clip_visual(name, sd, img)
    shapes = {"im2col": (B * P, tr.cdiv(3 * ps * ps, 64) * 64), "x": (M, width), "y": (M, width), "qkv": (M, 3 * width), "ao": (M, width),
              "h1": (M, mlp), "pool": (B, width)}
    drv = {n: ops.workspace_read("clip." + n, s) for n, s in shapes.items()}
    _hold(f"CLIP image tower {name} B={B}", tr.CLIP_ORDER, got, drv, rep_out, rep)
    return got


@pytest.mark.parametrize("name,B", [("tiny-64-s56", 1), ("tiny-64-s56", 3), ("tiny-80-s56", 1), ("tiny-80-s56", 3), ("tiny-104-s56", 1),
                                    ("tiny-104-s56", 3), ("tiny-bigG-wide", 1), ("tiny-bigG-wide", 3), ("tiny-64", 1)])
def test_clip_visual_is_its_replay(name, B):
    """head dimensions 64 / 80 / 104 and one block at ViT-bigG/14's width at 56^2 (17 tokens in 32 rows), 257 tokens at 224^2.  The
    residual stream lives in clip.y and the LayerNorm outputs in clip.x; ln_post reads row 0 of every crop with stride npad."""
    ops = _ops()
    sd = ops.random_clip_state_dict(name, seed=4)
    _assert_layernorms_distinct(sd)
    S = 14 * ops.CLIP_ARCHS[name][6]
    _clip_visual_check(ops.ClipVisual(name, sd), name, sd, tr.smooth_images(B, S, S, 23).cuda())


def _text_prompts(vocab, ctx, seed):
    """three prompts: the largest id at position 0; at position ctx - 1; twice (the first occurrence is pooled)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, vocab - 2, (3, ctx), generator=g)
    ids[0, 0] = vocab - 1
    ids[1, ctx - 1] = vocab - 1
    first, second = ctx // 3, ctx - 2
    ids[2, first] = ids[2, second] = vocab - 1
    assert tr.first_maximum(ids) == [0, ctx - 1, first]
    return ids


def _clip_text_check(text, name, sd, ids):
    ops = _ops()
    width, depth, heads, mlp, vocab, ctx, embed = ops.CLIP_TEXT_ARCHS[name]
    B = ids.shape[0]
    npad = tr.cdiv(ctx, 16) * 16
    M = B * npad
    got = text(ids)
    torch.cuda.synchronize()
    rep_out, rep = tr.replay_clip_text(name, sd, ids)
    shapes = {"x": (M, width), "y": (M, width), "qkv": (M, 3 * width), "ao": (M, width), "h1": (M, mlp), "pool": (B, width), "pooln": (B, width)}
    drv = {n: ops.workspace_read("clip_text." + n, s) for n, s in shapes.items()}
    _hold(f"CLIP text tower {name} B={B}", tr.TEXT_ORDER, got, drv, rep_out, rep)
    # the pooled row is the residual stream's row at the FIRST maximum of the ids
    stream = drv["x"].view(B, npad, width)
    for b, at in enumerate(tr.first_maximum(ids)):
        assert torch.equal(drv["pool"][b].view(torch.int16), stream[b, at].view(torch.int16)), f"prompt {b}: not the row at position {at}"
    return got, drv


@pytest.mark.parametrize("name", ["tiny-64-c17", "tiny-64", "tiny-bigG-text"])
@pytest.mark.parametrize("B", [1, 3])
def test_clip_text_is_its_replay(name, B):
    """17 positions in 32 rows, 77 in 80, and one block at ViT-bigG/14's text width.  B = 1: each of the three prompts as a call of its own."""
    ops = _ops()
    sd = ops.random_clip_text_state_dict(name, seed=6)
    _assert_layernorms_distinct(sd)
    text = ops.ClipText(name, sd)
    ids = _text_prompts(ops.CLIP_TEXT_ARCHS[name][4], ops.CLIP_TEXT_ARCHS[name][5], 8)
    for batch in ([ids] if B == 3 else [ids[i:i + 1] for i in range(3)]):
        _clip_text_check(text, name, sd, batch)


# ---- d. the inputs distinguish the faults that matter ---------------------------------------------------------------------------------------
FAULT_CASES = ((3, 28, 42), (1, 224, 224))       # non-square and resized; more than one attention tile.  layer 3, patch features, folded
OLD_BAR = 2e-2                                   # relative L2 against the fp32 oracle that tests/test_gpu_vit.py asks of a forward


@pytest.fixture(scope="module")
def fault_ground(vit, vit_sd, vit_sd_cpu):
    """per fault case: the image, the driver's output and buffers, the fp32 oracle"""
    from oracle import vit_ref
    sdf = {k: v.float() for k, v in vit_sd_cpu.items()}
    ground = []
    with _LnFused(1):
        for B, H, W in FAULT_CASES:
            img = tr.smooth_images(B, H, W, 25).cuda()
            got = _vit_check(vit, vit_sd, img, 3, "patch", 1, what="fault ground:").clone()
            drv = _vit_buffers(B, H, W, [n for n in tr.VIT_ORDER if n != "y"])
            ref = vit_ref.vit_forward(sdf, img.cpu().float(), layer=3, feature_type="patch", dtype=torch.float32)
            ground.append((img, got, drv, ref))
    return ground


def _rel(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return ((got - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("fault", tr.FAULTS_VIT)
def test_vit_fault_is_visible(vit_sd, fault_ground, fault):
    """the replay with ONE wiring fault must differ from the driver's bits on at least one case; printed next to it (pytest -s), the
    faulty forward's relative L2 against the fp32 oracle and the 2e-2 the end-to-end tests ask: below the bar = a fault the suite could
    not see before.  Nothing is asserted on that figure."""
    seen = []
    for (B, H, W), (img, got, drv, ref) in zip(FAULT_CASES, fault_ground):
        out, rep = tr.replay_vit(vit_sd, img, 3, "patch", 1, fault=fault)
        differs = [n for n in tr.VIT_ORDER if n in rep and tr.first_difference(drv[n], rep[n]) is not None]
        if tr.first_difference(got, out) is not None:
            differs.append("out")
        rel, rel0 = _rel(out, ref), _rel(got, ref)
        print(f"\n[fault] {fault:24s} {H}x{W} B={B}: differs in {differs or 'nothing'}; rel vs fp32 oracle {rel:.4g} "
              f"(driver {rel0:.4g}, old bar {OLD_BAR:g}: {'UNSEEN before' if rel <= OLD_BAR else 'seen'})")
        seen.append(bool(differs))
    assert any(seen), f"{fault}: the faulty replay carries the driver's bits on every case — the inputs are too weak"


def test_clip_fault_is_visible():
    from tests import _clip_ref as cr
    ops = _ops()
    name = "tiny-64-s56"
    sd = ops.random_clip_state_dict(name, seed=4)
    img = tr.smooth_images(3, 56, 56, 23).cuda()
    got = _clip_visual_check(ops.ClipVisual(name, sd), name, sd, img)
    out, _ = tr.replay_clip_visual(name, sd, img, fault="ln_pre_post_swapped")
    sdf = {k: v.float() for k, v in sd.items()}
    xn = cr.normalize_bf16(img.cpu()).float()
    ref = cr.clip_forward(sdf, xn, ops.CLIP_ARCHS[name][2])
    r16 = _rel(cr.clip_forward(sdf, xn, ops.CLIP_ARCHS[name][2], rnd=cr.bf16_round), ref)
    print(f"\n[fault] ln_pre_post_swapped {name}: rel vs fp32 oracle {_rel(out, ref):.4g} (driver {_rel(got, ref):.4g}, "
          f"old bar 1.25 * {r16:.4g} + 1e-4 = {1.25 * r16 + 1e-4:.4g})")
    assert tr.first_difference(got, out) is not None, "ln_pre / ln_post swapped: the same bits — the inputs are too weak"


def test_clip_text_fault_is_visible():
    from tests import _clip_ref as cr
    from tests import _clip_text_ref as ctr
    ops = _ops()
    name = "tiny-64-c17"
    sd = ops.random_clip_text_state_dict(name, seed=6)
    ids = _text_prompts(ops.CLIP_TEXT_ARCHS[name][4], ops.CLIP_TEXT_ARCHS[name][5], 8)
    got, _ = _clip_text_check(ops.ClipText(name, sd), name, sd, ids)
    out, _ = tr.replay_clip_text(name, sd, ids, fault="pool_last_maximum")
    sdf = {k: v.float() for k, v in sd.items()}
    ref = ctr.clip_text_forward(sdf, ids, ops.CLIP_TEXT_ARCHS[name][2])
    r16 = _rel(ctr.clip_text_forward(sdf, ids, ops.CLIP_TEXT_ARCHS[name][2], rnd=cr.bf16_round), ref)
    print(f"\n[fault] pool_last_maximum {name}: rel vs fp32 oracle {_rel(out, ref):.4g} (driver {_rel(got, ref):.4g}, "
          f"old bar 1.25 * {r16:.4g} + 1e-4 = {1.25 * r16 + 1e-4:.4g})")
    # only the prompt whose largest id occurs twice is pooled elsewhere
    assert torch.equal(got[:2].view(torch.int16), out[:2].view(torch.int16))
    assert tr.first_difference(got[2], out[2]) is not None, "pooling at the last maximum: the same bits — the inputs are too weak"
