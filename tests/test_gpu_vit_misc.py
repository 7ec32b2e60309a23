"""The helper kernels of csrc/vit_misc.hip one at a time, through their kernel-level entries (fp_op_posembed_aa, fp_op_token_init,
fp_op_layernorm_rows, fp_op_row_stats, fp_op_stats_finalize, fp_op_ln_fold, fp_op_transpose), against the float64 references of
tests/_vit_misc_cases.py at the smallest shapes that reach every branch and launch form.  Where the comparison is not bit for bit the bound is

    |got - ref64| <= half_ulp_bf16(ref64) + 4 * E_case * S(elem)          (fp32 outputs: 2^-16 |ref64| instead of the half ulp)

with E_case measured on the CPU (tests/_vit_misc_cases.py; tests/test_vit_misc_cases_cpu.py shows that every listed mutant of a kernel's
arithmetic breaks it).  Every test prints the worst |got - ref| / bound it saw.

  test                       kernel                         what can go wrong there
  test_posembed              posembed_aa_kernel             cubic coefficient, antialias stretch, normalisation, gh / gw, window start, centre; D > 256
  test_token_init            token_init_kernel              registers with a position, class row without, stale pad rows, a patch row written
  test_layernorm_plain       layernorm_kernel<1..4, 0>      variance over D - 1, eps, one-pass variance, chunk tails (D = 520, 1032, 1544), grid stride
  test_layernorm_l2          layernorm_kernel<1..3, 1>      the bits of fp_l2_normalize on the plain output
  test_layernorm_gather      rows_per_b / in_stride_b / in_off of the towers' final norm; unselected rows are NaN
  test_row_stats             row_stats_kernel<1, 2, 3>      record layout, two-pass statistics, 1 / sigma
  test_stats_finalize        stats_finalize_kernel          block-order sums, part_ld > rows (NaN padding), the one-pass variance's conditioning
  test_ln_fold               ln_fold_kernel                 W' bit for bit, the column sum over the ROUNDED W', row n_scaled unscaled, b' scaled once
  test_transpose             transpose_bf16_kernel          exact, including the stride loop past 4096 blocks
  test_refusals / test_empty_calls                          loud refusals and empty calls return before any launch
"""
import numpy as np
import pytest
import torch

from tests import _vit_misc_cases as vc

pytestmark = pytest.mark.gpu


def _api():
    from freepose_amd import _lib, ops
    return _lib.load(), ops


def _dev(bits):
    """uint16 bf16 bits -> bf16 tensor on the device"""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def _bits(t):
    """bf16 / int32 device tensor -> uint16 bits on the host (int32 rows [n, 4] -> [n, 8])"""
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _within(what, got64, ref, bound):
    ok = np.abs(got64 - ref) <= bound                                       # a NaN is not within
    ratio = np.abs(got64 - ref) / np.where(bound > 0, bound, 1.0)
    worst = float(np.nanmax(np.where(bound > 0, ratio, 0.0))) if ratio.size else 0.0
    print(f"[vit_misc] {what}: worst |got - ref| / bound = {worst:.3f}")
    if not ok.all():
        i = np.unravel_index(np.argmax(np.where(ok, -1.0, np.nan_to_num(ratio, nan=np.inf))), ok.shape)
        pytest.fail(f"{what}: {int((~ok).sum())} of {ok.size} elements outside the bound; worst at {i}: got {got64[i]!r}, reference {ref[i]!r}, "
                    f"bound {bound[i]!r}")


# ---- resized position embedding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vc.POSEMBED_CASES, ids=lambda c: c.name)
def test_posembed(case):
    _, ops = _api()
    x = vc.posembed_input(case)
    got = _bits(ops.posembed_aa(_dev(x), case.gh, case.gw))
    assert got.shape == (case.gh * case.gw, case.D)
    if case.name == "pos_identity":
        assert np.array_equal(got, x), "identity resize: the weights are 0, 1, 0, 0 and the output bits the input's"
    ref, S = vc.posembed_ref64(x, case.G, case.gh, case.gw)
    _within(f"posembed {case.name}", vc.bits_f32(got).astype(np.float64), ref, vc.bound_bf16(ref, vc.E_CASE[case.name], S))
    share = float((got != vc.posembed_torch_f32_bits(x, case.G, case.gh, case.gw)).mean())
    print(f"[vit_misc] posembed {case.name}: {share:.5%} of the elements differ in bits from torch's float32 path")
    assert share <= vc.POS_MISMATCH_GPU


# ---- token init ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vc.TOKEN_CASES, ids=lambda c: c.name)
def test_token_init(case):
    _, ops = _api()
    cls, pos0, reg = vc.token_inputs(case)
    n_tok, npad = vc.token_dims(case)
    X = _dev(np.full((case.B, npad, case.D), vc.TOKEN_PATTERN, dtype=np.uint16))
    ops.token_init(X, _dev(cls), _dev(pos0), _dev(reg) if case.nreg else None, n_tok)
    got, want = _bits(X), vc.token_expected(case, cls, pos0, reg)
    assert np.array_equal(got[:, 0], want[:, 0]), "class row: bf16(cls + pos[0])"
    assert np.array_equal(got[:, 1:1 + case.nreg], want[:, 1:1 + case.nreg]), "register rows: the register bits, no position"
    assert not got[:, n_tok:].any(), "pad rows: +0"
    assert (got[:, 1 + case.nreg:n_tok] == vc.TOKEN_PATTERN).all(), "a patch row was written"


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ln_plain():
    """the plain form's output bits per case, computed once (the L2 test reads them)"""
    cache = {}

    def run(case):
        if case.name not in cache:
            _, ops = _api()
            x, g, b = vc.ln_inputs(case)
            cache[case.name] = _bits(ops.layernorm_rows(_dev(x), _dev(g), _dev(b), eps=vc.EPS))
        return cache[case.name]
    return run


@pytest.mark.parametrize("case", vc.LN_CASES, ids=lambda c: c.name)
def test_layernorm_plain(case, ln_plain):
    _, ops = _api()
    x, g, b = vc.ln_inputs(case)
    got = ln_plain(case)
    assert got.shape == x.shape
    if case.regime == "const":
        assert np.array_equal(got, np.broadcast_to(b, x.shape)), "constant rows: (x - mean) is 0 and the output bits are beta's"
    ref, S = vc.ln_ref64(x, g, b)
    _within(f"layernorm {case.name}", vc.bits_f32(got).astype(np.float64), ref, vc.bound_bf16(ref, vc.E_CASE[case.name], S))
    assert np.array_equal(_bits(ops.layernorm(_dev(x), _dev(g), _dev(b), eps=vc.EPS)), got), "fp_op_layernorm: the same launch, the same bits"


@pytest.mark.parametrize("case", [c for c in vc.LN_CASES if c.D <= vc.LN_L2_MAX_D], ids=lambda c: c.name)
def test_layernorm_l2(case, ln_plain):
    _, ops = _api()
    x, g, b = vc.ln_inputs(case)
    got = _bits(ops.layernorm_rows(_dev(x), _dev(g), _dev(b), eps=vc.EPS, l2_normalize=True))
    want = _bits(ops.l2_normalize(_dev(ln_plain(case))))
    assert np.array_equal(got, want), f"{case.name}: {int((got != want).sum())} elements differ from l2_normalize(plain LayerNorm)"


@pytest.mark.parametrize("form", sorted(vc.gather_forms()))
@pytest.mark.parametrize("l2", (False, True), ids=("plain", "l2"))
def test_layernorm_gather(form, l2):
    _, ops = _api()
    rpb, stride, off = vc.gather_forms()[form]
    rows, D = vc.GATHER_B * rpb, vc.GATHER_D
    sel = vc.gather_rows(rows, rpb, stride, off)
    buf = np.full((vc.GATHER_B * vc.GATHER_NPAD, D), 0x7FC0, dtype=np.uint16)          # every unselected row: NaN
    buf[sel] = vc.regime_rows(700 + rpb, rows, D, "normal")
    g, b = vc.randn_bf16(710, (D,), 0.25, 1.0), vc.randn_bf16(711, (D,), 0.5)
    got = _bits(ops.layernorm_rows(_dev(buf), _dev(g), _dev(b), eps=vc.EPS, rows=rows, rows_per_b=rpb, in_stride_b=stride, in_off=off,
                                   l2_normalize=l2))
    want = _bits(ops.layernorm_rows(_dev(buf[sel]), _dev(g), _dev(b), eps=vc.EPS, l2_normalize=l2))
    assert got.shape == (rows, D) and not np.isnan(vc.bits_f32(want)).any()
    assert np.array_equal(got, want), f"{form}: {int((got != want).any(axis=1).sum())} of {rows} rows differ from the plain form on the selected rows"


# ---- row statistics ------------------------------------------------------------------------------------------------------------------------------------
def _check_stats(what, name, rec, rstd, refs):
    mean, sigma = vc.decode_row_record(_bits(rec))                                        # asserts the record's layout
    for out, got in (("mean", mean), ("sigma", sigma), ("rstd", rstd.cpu().numpy().astype(np.float64))):
        ref, S = refs[out]
        _within(f"{what} {name} {out}", got, ref, vc.bound_f32(ref, vc.E_CASE[f"{name}:{out}"], S))


@pytest.mark.parametrize("case", vc.STAT_CASES, ids=lambda c: c.name)
def test_row_stats(case):
    _, ops = _api()
    x = vc.stat_inputs(case)
    rec, rstd = ops.row_stats(_dev(x), eps=vc.EPS)
    _check_stats("row_stats", case.name, rec, rstd, vc.row_stats_ref64(x))


@pytest.mark.parametrize("case", vc.FIN_CASES, ids=lambda c: c.name)
def test_stats_finalize(case):
    _, ops = _api()
    part = vc.partial_sums(vc.stat_inputs(case), case.pad)
    rec, rstd = ops.stats_finalize(torch.from_numpy(part).cuda(), case.rows, eps=vc.EPS)
    _check_stats("stats_finalize", case.name, rec, rstd, vc.finalize_ref64(part, case.rows))


# ---- LayerNorm fold ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vc.FOLD_CASES, ids=lambda c: c.name)
def test_ln_fold(case):
    _, ops = _api()
    W, g, be, bi = vc.fold_inputs(case)
    wf, cb = ops.ln_fold(_dev(W), _dev(g), _dev(be), _dev(bi), n_scaled=case.n_scaled, row_scale=case.row_scale)
    got = _bits(wf)
    want, _, _ = vc.fold_restate(W, g, be, bi, case.n_scaled, case.row_scale)
    assert np.array_equal(got, want), f"{case.name}: W' differs in rows {sorted(set(np.nonzero(got != want)[0]))[:8]}"
    plain = vc.bf16_bits(vc.bits_f32(W) * vc.bits_f32(g))
    assert np.array_equal(got[case.n_scaled:], plain[case.n_scaled:]), "rows n >= n_scaled carry no scale"
    bp, cs = vc.decode_fold_record(_bits(cb))
    refs = vc.fold_ref64(W, be, bi, got, case.n_scaled, case.row_scale)
    for out, val in (("colsum", cs), ("bprime", bp)):
        ref, S = refs[out]
        _within(f"ln_fold {case.name} {out}", val, ref, vc.bound_f32(ref, vc.E_CASE[f"{case.name}:{out}"], S))


# ---- transpose -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", vc.TRANSPOSE_CASES)
def test_transpose(rows, cols):
    _, ops = _api()
    x = vc.transpose_input(rows, cols)
    got = _bits(ops.transpose(_dev(x)))
    assert got.shape == (cols, rows) and np.array_equal(got, x.T)


# ---- refusals and empty calls: nothing is launched -------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib, ops = _api()
    t = torch.zeros(4096, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p, s = ops.ptr, ops.current_stream

    def refused(rc, needle):
        msg = lib.fp_last_error().decode()
        assert rc != 0 and needle in msg, (rc, msg)

    G, gh, gw, D = vc.POSEMBED_REFUSED
    refused(lib.fp_op_posembed_aa(p(t), p(t), G, gh, gw, D, s()), "downscale factor too large")
    for D, l2 in vc.LN_REFUSED:
        refused(lib.fp_op_layernorm_rows(p(t), p(t), p(t), p(t), 1, D, vc.EPS, 0, 0, 0, l2, s()), "layernorm: D=")
    refused(lib.fp_op_row_stats(p(t), 1, vc.STAT_REFUSED_D, vc.EPS, p(f), p(f), s()), "row_stats: D=")
    refused(lib.fp_op_stats_finalize(p(f), 1, vc.FIN_REFUSED_D, vc.EPS, 0, p(f), p(f), s()), "stats_finalize: D=")
    refused(lib.fp_op_ln_fold(p(t), p(t), p(t), p(t), 4, vc.FOLD_REFUSED_K, 0, 1.0, p(t), p(f), s()), "ln_fold:")
    refused(lib.fp_op_token_init(p(t), p(t), p(t), p(t), 4, 1, 4, 16, 8, s()), "op_token_init:")            # n_tok < 1 + nreg
    torch.cuda.synchronize()
    assert not bool(t.any()) and not bool(f.any())


def test_empty_calls():
    _, ops = _api()
    g = torch.ones(64, dtype=torch.bfloat16, device="cuda")
    e = torch.empty((0, 64), dtype=torch.bfloat16, device="cuda")
    assert ops.layernorm(e, g, g).shape == (0, 64) and ops.layernorm_rows(e, g, g, l2_normalize=True).shape == (0, 64)
    rec, rstd = ops.row_stats(e)
    assert rec.shape == (0, 4) and rstd.shape == (0,)
    rec, rstd = ops.stats_finalize(torch.empty((1, 0, 2), dtype=torch.float32, device="cuda"), 0)
    assert rec.shape == (0, 4) and rstd.shape == (0,)
    assert ops.transpose(e).shape == (64, 0) and ops.transpose(e.reshape(64, 0)).shape == (0, 64)
    assert ops.posembed_aa(torch.zeros((9, 8), dtype=torch.bfloat16, device="cuda"), 0, 3).shape == (0, 8)
    assert ops.token_init(torch.empty((0, 16, 64), dtype=torch.bfloat16, device="cuda"), g, g, None, 16).shape == (0, 16, 64)
    wf, cb = ops.ln_fold(e, g, g, torch.empty(0, dtype=torch.bfloat16, device="cuda"))
    assert wf.shape == (0, 64) and cb.shape == (0, 4)
    torch.cuda.synchronize()
