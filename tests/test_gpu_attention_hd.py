"""attention for a general head dimension (csrc/attention_hd.hip) against a float64 softmax reference on the bf16 inputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16)


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-20)).item()


def _poisoned(B, npad, width, pad_cols=8, guard_rows=16):
    """0xFF-filled buffer with guard columns (row stride width + 8) and guard rows; returns (buffer as int16, the [B,npad,width] view)"""
    buf = torch.full((B * npad + guard_rows, width + pad_cols), -1, dtype=torch.int16, device="cuda")
    view = buf.view(torch.bfloat16)[:B * npad, :width].unflatten(0, (B, npad))
    return buf, view


def _reference(qkv, n_tok, heads, scale):
    B, npad, w3 = qkv.shape
    hd = w3 // 3 // heads
    t = qkv.reshape(B, npad, 3, heads, hd)
    q, k, v = (t[:, :n_tok, i].permute(0, 2, 1, 3).double() for i in range(3))
    ref = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v
    return ref.permute(0, 2, 1, 3).reshape(B, n_tok, heads * hd)


def test_entry_point_is_exported():
    from freepose_amd import _lib
    assert hasattr(_lib.load(), "fp_op_attention_hd")          # fails without the feature


# 64-key tiles: 1, 15, 16, 17 -> one partial tile; 257 -> 4 full tiles + 1 key; 300 -> 4 full + 44 keys; 65 -> one key past the first tile
@pytest.mark.parametrize("n_tok", [1, 15, 16, 17, 65, 257, 300])
@pytest.mark.parametrize("B,heads", [(1, 1), (2, 3)])
@pytest.mark.parametrize("head_dim", [8, 64, 72, 80, 104, 128])
def test_attention_hd(head_dim, B, heads, n_tok):
    from freepose_amd import ops
    npad = (n_tok + 15) // 16 * 16
    width = heads * head_dim
    qkv = _rand((B, npad, 3 * width), 21, 1.5)
    scale = 1.0 / float(np.sqrt(head_dim))
    # pad rows of QKV hold NaNs in one run and zeros in the other: no real output row may differ, bit for bit
    q_nan, q_zero = qkv.clone(), qkv.clone()
    q_nan[:, n_tok:] = float("nan")
    q_zero[:, n_tok:] = 0
    buf, out = _poisoned(B, npad, width)
    ops.attention_hd(q_nan.cuda(), heads, n_tok, out=out)
    buf2, out2 = _poisoned(B, npad, width)
    ops.attention_hd(q_zero.cuda(), heads, n_tok, out=out2)
    torch.cuda.synchronize()
    assert torch.equal(buf[:B * npad, :width], buf2[:B * npad, :width])
    assert (buf[:, width:] == -1).all() and (buf[B * npad:] == -1).all(), "guard columns / rows were written"
    assert torch.isfinite(out.float()).all(), "pad rows must stay finite"
    ref = _reference(qkv, n_tok, heads, scale)
    got = out[:, :n_tok].float().cpu()
    err = _rel(got, ref)
    mx = (got - ref.float()).abs().max().item()
    print(f"hd={head_dim} B={B} heads={heads} n_tok={n_tok}: rel {err:.2e} max abs {mx:.2e}")
    assert err < 1e-2, f"attention_hd rel err {err}"
    assert mx < 0.05


@pytest.mark.parametrize("head_dim", [64, 104])
def test_attention_hd_forced_rescale(head_dim):
    """spike one key against one query at a late tile so the running maximum jumps (the online-softmax rescale); queries whose logits
    all sit far below zero must not underflow to 0 / 0"""
    from freepose_amd import ops
    B, heads, n_tok, npad = 1, 1, 300, 304
    qkv = _rand((B, npad, 3, heads, head_dim), 31, 0.3).float()
    qkv[0, 5, 0, 0] = 4.0          # query 5
    qkv[0, 250, 1, 0] = 4.0        # key 250 (4th tile): q.k = 16 hd -> logit 16 sqrt(hd) >= 128
    qkv[0, :, 1, 0, 1] = 6.0       # every key: component 1 = 6
    qkv[0, 9, 0, 0, 1] = -48.0     # query 9: logits ~ -288 / sqrt(hd)
    qkv[0, 11, 0, 0, 1] = -400.0   # query 11: logits ~ -2400 / sqrt(hd)
    qkv = qkv.to(torch.bfloat16).reshape(B, npad, 3 * head_dim)
    o = ops.attention_hd(qkv.cuda(), heads, n_tok).float().cpu().reshape(npad, head_dim)
    assert torch.isfinite(o).all()
    ref = _reference(qkv, n_tok, heads, 1.0 / float(np.sqrt(head_dim)))[0]
    v = qkv.reshape(npad, 3, head_dim)[:, 2].float()
    assert (o[:n_tok] - ref.float()).abs().max().item() < 0.02
    assert (o[5] - v[250]).abs().max().item() < 0.02   # query 5 attends (almost) only to key 250


def test_attention_hd_custom_scale_and_long_sequence():
    """an explicit scale, and 1100 tokens (18 key tiles, 18 query blocks)"""
    from freepose_amd import ops
    B, heads, hd, n_tok = 1, 2, 104, 1100
    npad = 1104
    qkv = _rand((B, npad, 3 * heads * hd), 41, 1.0)
    o = ops.attention_hd(qkv.cuda(), heads, n_tok, scale=0.05)
    ref = _reference(qkv, n_tok, heads, 0.05)
    got = o[:, :n_tok].float().cpu()
    assert _rel(got, ref) < 1e-2 and (got - ref.float()).abs().max().item() < 0.05


def test_attention_hd_refusals():
    from freepose_amd import ops
    for hd, npad, what in ((12, 16, "head_dim=12"), (136, 16, "head_dim=136"), (64, 24, "npad=24")):
        qkv = torch.zeros((1, npad, 3 * hd), dtype=torch.bfloat16, device="cuda")
        with pytest.raises(RuntimeError, match=what):
            ops.attention_hd(qkv, 1, 5)
    with pytest.raises(RuntimeError, match="n_tok=20"):
        ops.attention_hd(torch.zeros((1, 16, 192), dtype=torch.bfloat16, device="cuda"), 1, 20)
