"""causal attention for a general head dimension (csrc/attention_causal.hip) against a float64 masked softmax on the bf16 inputs."""
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
    """float64: query t over the keys 0 .. t"""
    B, npad, w3 = qkv.shape
    hd = w3 // 3 // heads
    t = qkv.reshape(B, npad, 3, heads, hd)
    q, k, v = (t[:, :n_tok, i].permute(0, 2, 1, 3).double() for i in range(3))
    future = torch.triu(torch.ones((n_tok, n_tok), dtype=torch.bool), diagonal=1)
    ref = torch.softmax((q @ k.transpose(-1, -2) * scale).masked_fill(future, float("-inf")), dim=-1) @ v
    return ref.permute(0, 2, 1, 3).reshape(B, n_tok, heads * hd)


def _bits(t):
    return t.contiguous().view(torch.int16)


def test_entry_point_is_exported():
    from freepose_amd import _lib, ops
    assert hasattr(_lib.load(), "fp_op_attention_causal") and callable(ops.attention_causal)          # fails without the feature


# 64-key tiles, 64-query blocks, 16-query waves: 16 / 17 cross a wave boundary, 63 / 64 / 65 the tile and block boundary, 77 is the text
# tower's length (the first query block skips the second tile), 130 = two full tiles + 2 keys and three query blocks
@pytest.mark.parametrize("n_tok", [1, 2, 16, 17, 63, 64, 65, 77, 130])
@pytest.mark.parametrize("B,heads", [(1, 1), (2, 3)])
@pytest.mark.parametrize("head_dim", [8, 64, 104])
def test_attention_causal(head_dim, B, heads, n_tok):
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
    ops.attention_causal(q_nan.cuda(), heads, n_tok, out=out)
    buf2, out2 = _poisoned(B, npad, width)
    ops.attention_causal(q_zero.cuda(), heads, n_tok, out=out2)
    torch.cuda.synchronize()
    assert torch.equal(buf[:B * npad, :width], buf2[:B * npad, :width])
    assert (buf[:, width:] == -1).all() and (buf[B * npad:] == -1).all(), "guard columns / rows were written"
    assert torch.isfinite(out.float()).all(), "pad rows must stay finite"
    ref = _reference(qkv, n_tok, heads, scale)
    got = out[:, :n_tok].float().cpu()
    err = _rel(got, ref)
    mx = (got - ref.float()).abs().max().item()
    print(f"hd={head_dim} B={B} heads={heads} n_tok={n_tok}: rel {err:.2e} max abs {mx:.2e}")
    assert err < 1e-2, f"attention_causal rel err {err}"
    assert mx < 0.05
    # query 0 sees key 0 only: P = 1, the output is V row 0 bit for bit
    v = qkv.reshape(B, npad, 3, width)[:, :, 2]
    assert torch.equal(_bits(out[:, 0].cpu()), _bits(v[:, 0]))
    # nothing after query t reaches rows <= t: replace every K and V row > t by large finite values of both signs
    base = out.cpu()
    for t in sorted({0, 15, 16, 63, 64, n_tok - 2}):
        if t < 0 or t + 1 >= n_tok:
            continue
        loud = qkv.clone().reshape(B, npad, 3, width)
        sign = torch.where(torch.arange(width) % 2 == 0, 1.0, -1.0).to(torch.bfloat16)
        loud[:, t + 1:n_tok, 1] = 1e30 * sign
        loud[:, t + 1:n_tok, 2] = -1e30 * sign
        o = ops.attention_causal(loud.reshape(B, npad, 3 * width).cuda(), heads, n_tok).cpu()
        assert torch.equal(_bits(o[:, :t + 1]), _bits(base[:, :t + 1])), f"rows <= {t} changed with the rows after them"


@pytest.mark.parametrize("head_dim", [64, 104])
def test_attention_causal_forced_rescale(head_dim):
    """a spiked key in the second tile: the late query that sees it has its running maximum jump there (the online-softmax rescale of
    what the first tile accumulated), the early query of the same block, for which the key is masked, is untouched by it"""
    from freepose_amd import ops
    B, heads, n_tok, npad = 1, 1, 130, 144
    qkv = _rand((B, npad, 3, heads, head_dim), 31, 0.3).float()
    qkv[0, 90, 0, 0] = 4.0         # query 90: key 100 lies after it
    qkv[0, 120, 0, 0] = 4.0        # query 120 sees key 100
    qkv[0, 100, 1, 0] = 4.0        # key 100 (second tile): q.k = 16 hd -> logit 16 sqrt(hd) >= 128
    qkv = qkv.to(torch.bfloat16).reshape(B, npad, 3 * head_dim)
    o = ops.attention_causal(qkv.cuda(), heads, n_tok).float().cpu().reshape(npad, head_dim)
    assert torch.isfinite(o).all()
    ref = _reference(qkv, n_tok, heads, 1.0 / float(np.sqrt(head_dim)))[0].float()
    v = qkv.reshape(npad, 3, head_dim)[:, 2].float()
    assert (o[:n_tok] - ref).abs().max().item() < 0.02
    assert (o[120] - v[100]).abs().max().item() < 0.02       # query 120 attends (almost) only to key 100
    assert (o[90] - v[100]).abs().max().item() > 0.1         # query 90 does not
    quiet = qkv.clone().reshape(npad, 3, head_dim)
    quiet[100, 1] = 0                                        # without the spike query 90 gives the same bits: the key was masked, not down-weighted
    o2 = ops.attention_causal(quiet.reshape(B, npad, 3 * head_dim).cuda(), heads, n_tok).float().cpu().reshape(npad, head_dim)
    assert torch.equal(o2[:100], o[:100])


def test_attention_causal_custom_scale_and_output_slice():
    """an explicit scale, and an output that is a column slice of a wider buffer"""
    from freepose_amd import ops
    B, heads, hd, n_tok, npad = 2, 2, 64, 77, 80
    qkv = _rand((B, npad, 3 * heads * hd), 41, 1.0)
    wide = torch.zeros((B, npad, 2 * heads * hd), dtype=torch.bfloat16, device="cuda")
    ops.attention_causal(qkv.cuda(), heads, n_tok, scale=0.05, out=wide[:, :, heads * hd:])
    ref = _reference(qkv, n_tok, heads, 0.05)
    got = wide[:, :n_tok, heads * hd:].float().cpu()
    assert _rel(got, ref) < 1e-2 and (got - ref.float()).abs().max().item() < 0.05
    assert (wide[:, :, :heads * hd] == 0).all()


def test_attention_causal_refusals():
    from freepose_amd import ops
    for hd, npad, what in ((12, 16, "head_dim=12"), (136, 16, "head_dim=136"), (64, 24, "npad=24")):
        qkv = torch.zeros((1, npad, 3 * hd), dtype=torch.bfloat16, device="cuda")
        with pytest.raises(RuntimeError, match=what):
            ops.attention_causal(qkv, 1, 5)
    with pytest.raises(RuntimeError, match="n_tok=20"):
        ops.attention_causal(torch.zeros((1, 16, 192), dtype=torch.bfloat16, device="cuda"), 1, 20)
