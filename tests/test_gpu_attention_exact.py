"""The three attention kernels on inputs whose answer is known exactly or to one bf16 neighbour (tests/_attn_cases.py): a selected key
must come back bit for bit, a uniform softmax must be the mean over exactly the visible keys, power-of-two softmaxes walk the lazy
running maximum of attention.hip across its threshold, and the plain path is held to the bound derived from its one bf16 rounding of P.
attention.hip is called through fp_op_attention directly, dense and through column slices of wider buffers, into poisoned outputs."""
import numpy as np
import pytest
import torch

from tests import _attn_cases as ac

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0
GUARD = 8   # guard rows before and after the strided output, guard columns after each of its rows


def _dev(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda()


def _split_heads(rows, case):
    """[B, n_tok, H * hd] -> [B, H, n_tok, hd]"""
    return rows.reshape(case.B, case.n_tok, case.H, case.hd).transpose(0, 2, 1, 3)


def _assert_expected(case, real_bits, what):
    got = _split_heads(ac.bits_to_f64(real_bits), case)
    ok = ac.check_output(case, got)
    if case.family == "nat8":
        big = case.expected > 2.0 ** -90
        print(f"\n[nat8] B{case.B} H{case.H} n{case.n_tok}: max |got - ref| / |ref| = "
              f"{float(np.max(np.abs(got - case.expected)[big] / case.expected[big])):.6e} (bound {ac.NAT8_RTOL:.6e})")
    if not ok.all():
        bad = np.argwhere(~ok)
        lines = [f"(b{b} h{h} t{t} d{d}): got {got[b, h, t, d]!r} want {case.expected[b, h, t, d]!r}" for b, h, t, d in bad[:6]]
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} elements break the '{case.rule}' rule; rows {sorted(set(bad[:, 2].tolist()))[:12]}\n"
                             + "\n".join(lines))


def _run_dino(case, strided):
    """fp_op_attention the way ops.attention calls it, dense or on column slices; returns (whole output buffer, its [B*npad, D] part)
    as int16 numpy arrays.  Every output buffer starts as 0xFFFF."""
    from freepose_amd import _lib
    lib = _lib.load()
    B, H, npad, D = case.B, case.H, case.npad, case.H * 64
    qk_bits, vt_bits = ac.pack_qk_vt(case)
    vt = _dev(vt_bits)
    if strided:
        ldqk, ldo = 2 * D + 64, D + 8
        wide = torch.full((B * npad, ldqk), NAN_BITS, dtype=torch.int16, device="cuda")
        wide[:, 32:32 + 2 * D] = _dev(qk_bits)
        qk = wide[:, 32:32 + 2 * D]
        buf = torch.full((B * npad + 2 * GUARD, ldo), -1, dtype=torch.int16, device="cuda")
        out = buf[GUARD:GUARD + B * npad, :D]
    else:
        ldqk, ldo = 2 * D, D
        qk = _dev(qk_bits)
        buf = torch.full((B * npad, D), -1, dtype=torch.int16, device="cuda")
        out = buf
    assert qk.stride(0) == ldqk and out.stride(0) == ldo
    _lib.check(lib.fp_op_attention(_lib.ptr(qk), ldqk, _lib.ptr(vt), _lib.ptr(out), ldo, B, H, case.n_tok, npad, int(case.prescaled),
                                   _lib.current_stream()), "fp_op_attention")
    torch.cuda.synchronize()
    return buf.cpu().numpy(), out.cpu().numpy()


def _real_rows(out, case):
    """[B * npad, width] -> the rows of real tokens, [B, n_tok, width]"""
    return out.reshape(case.B, case.npad, -1)[:, :case.n_tok]


def _assert_written_and_finite(out, what):
    vals = ac.bits_to_f64(out)
    rows = np.flatnonzero((out == -1).any(axis=1))
    assert rows.size == 0, f"{what}: rows {rows[:16].tolist()} still hold the 0xFFFF fill: a block or a store was skipped"
    assert np.isfinite(vals).all(), f"{what}: non-finite output in rows {np.flatnonzero(~np.isfinite(vals).all(axis=1))[:16].tolist()}"


@pytest.mark.parametrize("build", [pytest.param(f, id=n) for n, f in ac.dino_cases()])
def test_attention_exact(build):
    case = build()
    _, dense = _run_dino(case, strided=False)
    buf, strided = _run_dino(case, strided=True)
    D = case.H * 64
    _assert_written_and_finite(dense, "dense")            # pad rows included: every row below B * npad is written and finite
    _assert_written_and_finite(strided, "strided")
    assert (buf[:GUARD] == -1).all() and (buf[GUARD + case.B * case.npad:] == -1).all(), "guard rows were written"
    assert (buf[:, D:] == -1).all(), "guard columns were written"
    _assert_expected(case, _real_rows(dense, case), "dense")
    assert np.array_equal(_real_rows(dense, case), _real_rows(strided, case)), "dense and strided runs differ on real rows"


PAD_FAMILIES = {
    "select-plain": lambda n, pk, pv: ac.select_case("dino", 1, 3, 64, n, 2, False, pk, pv),
    "select-pre": lambda n, pk, pv: ac.select_case("dino", 1, 3, 64, n, 3, True, pk, pv),
    "pow2-pre": lambda n, pk, pv: ac.pow2_case("dino", 1, 3, 64, n, 1, pk, pv),
}


@pytest.mark.parametrize("n_tok", ac.DINO_PAD_NTOK)
@pytest.mark.parametrize("family", sorted(PAD_FAMILIES))
def test_attention_pads_cannot_reach_real_rows(family, n_tok):
    """pad K rows as the family builds them, then all NaN, all Inf, all zero; pad V columns +-2^14 / 2^12, then zero: the real rows must
    not move by a bit (masked logits are overwritten after the first product and exp2(-1e30) is exactly 0)"""
    base_case = PAD_FAMILIES[family](n_tok, "default", "default")
    _, base = _run_dino(base_case, strided=False)
    _assert_expected(base_case, _real_rows(base, base_case), "default pads")
    for pad_v in ("default", "zero"):
        for pad_k in ("nan", "inf", "zero"):
            case = PAD_FAMILIES[family](n_tok, pad_k, pad_v)
            assert np.array_equal(case.expected, base_case.expected)
            _, out = _run_dino(case, strided=False)
            _assert_written_and_finite(out, f"pad K {pad_k}, pad V {pad_v}")
            assert np.array_equal(_real_rows(out, case), _real_rows(base, base_case)), f"pad K {pad_k}, pad V {pad_v}: real rows moved"


def _run_hd(case):
    """ops.attention_hd / ops.attention_causal into a 0xFFFF-filled buffer with guard columns and rows"""
    from freepose_amd import ops
    B, npad, width = case.B, case.npad, case.H * case.hd
    qkv = _dev(ac.pack_qkv(case)).view(torch.bfloat16)
    buf = torch.full((B * npad + 2 * GUARD, width + 8), -1, dtype=torch.int16, device="cuda")
    out = buf[GUARD:GUARD + B * npad, :width]
    fn = ops.attention_causal if case.causal else ops.attention_hd
    fn(qkv, case.H, case.n_tok, scale=case.scale, out=buf.view(torch.bfloat16)[GUARD:GUARD + B * npad, :width].unflatten(0, (B, npad)))
    torch.cuda.synchronize()
    return buf.cpu().numpy(), out.cpu().numpy()


def _check_hd(case):
    buf, out = _run_hd(case)
    width = case.H * case.hd
    _assert_written_and_finite(out, case.kernel)
    assert (buf[:GUARD] == -1).all() and (buf[GUARD + case.B * case.npad:] == -1).all() and (buf[:, width:] == -1).all(), \
        "guard rows / columns were written"
    _assert_expected(case, _real_rows(out, case), case.kernel)


@pytest.mark.parametrize("build", [pytest.param(f, id=n) for n, f in ac.hd_cases()])
def test_attention_hd_exact(build):
    _check_hd(build())


@pytest.mark.parametrize("build", [pytest.param(f, id=n) for n, f in ac.causal_cases()])
def test_attention_causal_exact(build):
    _check_hd(build())
