"""Every tile tier, epilogue and row split of the ViT GEMM family (csrc/gemm_bf16.hip, gemm_epilogue.h, gemm_asm.hip) against exact arithmetic,
bit for bit, through the C entries with leading dimensions and guards under the test's control; and the LayerNorm chain (LS_RES_STATS
producer -> LN-folded consumer) on both routes the partial row statistics can take.  Cases, references and the dispatch mirror live in
tests/_gemm_cases.py; tests/test_gemm_cases_cpu.py shows without a GPU that the library's statement of the dispatch (csrc/gemm_plan.h) sends
every case to the branch named here on 256 CUs, on the ring depths named here, and equals the mirror on 10^5 shapes.  Here every test first
asks the library which plan it executes for its launch on this device (fp_op_gemm_plan, _assert_claim): on a device with another CU count a
case whose shape would reach another branch fails with that message instead of passing on the wrong tier, and the split tests take the
split row from the library.

Outputs are allocated with ldc > N and 64 extra rows, filled with 0xFF bytes (a NaN pattern no case produces): the [M, N] block must equal the
reference, every other byte must still hold the poison.  Input padding columns (ldx > K, ldw > K, ldr > N) hold NaN: a read outside an operand
row poisons the result.  No tolerance appears in this file except the derived bound of the chain's float64 restatement.

  test                      cases                  branch / what can go wrong there
  test_tiny                 tiny_*                 64x64 tiles on a K ring of depth 2 .. 4 (K = 64: ring deeper than K; 1, 2, 3, 5 K tiles), M = 1 .. 257 and
                                                   N = 16 .. 272 ragged against the tile, the 32-row wave halves and the 8-column store chunks;
                                                   BIAS, GELU (table), LS_RES, LS_RES_STATS; one-hot rows and a column ramp in the bias
  test_small                small_*                128x128 tiles, ragged last row and column tile, relocated GELU slabs, 1 / 2 / 3 K tiles
  test_big                  big_*, stream_*        16-wave persistent 256x256 kernel: one tile per workgroup (192) and a five-round walk with
                                                   non-temporal stores (160 MiB output), one row / one column chunk in the ragged tiles
  test_big_asm              asm_*                  hand-scheduled 256x256 kernel, pipelined epilogue, all four epilogues it is built for
  test_row_splits           splitbig_*, splitmid_* whole rounds + remainder: X / C / resid / stat_part offsets of the second launch, stat_ld
  test_vt                   vt_*                   transposed V store on 64x64 (one wave), 128x128 and 256x256 tiles (cached and streaming)
  test_patch                patch_*                fp_op_gemm_patch: scatter row b npad + tok_off + p, + pos[p], rounding bf16(bf16(acc) + pos)
  test_ln_chain             chain_*                fp_op_ln_chain route 0 (finalisation kernel) == route 1 (ln_part: small-tier prologue, both parts of a
                                                   split_mid, host finalisation in front of the big tier), and both within the derived bound
                                                   of the float64 fold (the worst |diff| / bound is printed per case)
"""
import numpy as np
import pytest
import torch

from tests import _gemm_cases as gc

pytestmark = pytest.mark.gpu

GUARD_ROWS = 64
CHUNK = 32768           # reference rows per block


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.fixture(scope="module")
def gelu_tab():
    """the device's direct GELU expression on all 65 536 bf16 patterns (pinned to torch by tests/test_gpu_kernels.py)"""
    from freepose_amd import ops
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.bfloat16)
    return ops.gelu_direct(pats).cpu().view(torch.int16).numpy().view(np.uint16).copy()


def _api():
    from freepose_amd import _lib, ops
    return _lib.load(), ops


def _assert_claim(case, claims, ncu):
    """The library itself says which plan it executes for this launch on this device (fp_op_gemm_plan: the function fp_gemm_bf16 launches
    from): it must be the branch the case is there for, and the mirror must say the same.  The shapes are chosen for 256 CUs; on another
    count a case that would reach another branch fails here instead of passing on the wrong tier (derive its shape anew from
    _gemm_cases.branch(..., n_cu=ncu)).  Returns the plan."""
    from freepose_amd import ops
    if isinstance(case, gc.Chain):                                                # the consumer launch with the partial sums handed over
        plan = ops.gemm_plan(case.M, case.N2, case.D, gc.LN_BIAS if case.mode == 0 else gc.LN_GELU, ln_part=True)
        mirror = case.branch(ncu, ln_part=True)
    else:
        plan = ops.gemm_plan(case.M, case.N, case.K, case.epi, case.ld("x"), case.ld("w"))
        mirror = case.branch(ncu)
    got = plan["label"]
    assert got == claims, f"{case.name}: on {ncu} CUs this shape reaches {got}, not {claims}; derive the shape from _gemm_cases.branch for this device"
    assert mirror == got, f"{case.name}: the library runs {plan['text']}, tests/_gemm_cases.py says {mirror}"
    return plan


def _poison(rows, ld):
    return torch.full((rows, ld), -1, dtype=torch.int16, device="cuda")


def _dev_rows(ints_fn, nrows, width, ld, scale):
    """bf16 [nrows, ld] on the device: columns < width from ints_fn(rows) * scale (exact), the padding columns NaN"""
    buf = _poison(nrows, ld).view(torch.bfloat16)
    step = max(1, (1 << 22) // max(width, 1))
    for r0 in range(0, nrows, step):
        rows = torch.arange(r0, min(nrows, r0 + step), dtype=torch.int64, device="cuda")
        buf[r0:r0 + len(rows), :width] = (ints_fn(rows).to(torch.float32) * scale).to(torch.bfloat16)
    return buf


def _dev_host(ints, ld, scale):
    ints = np.atleast_2d(ints)
    buf = _poison(ints.shape[0], ld).view(torch.bfloat16)
    buf[:, :ints.shape[1]] = torch.from_numpy(ints.astype(np.float32) * np.float32(scale)).to(torch.bfloat16).cuda()
    return buf


def _operands(case):
    x = _dev_rows(lambda r: gc.x_ints(case, r, xp=torch), case.M, case.K, case.ld("x"), gc.QX)
    w = _dev_host(gc.w_ints(case), case.ld("w"), gc.QW)
    bias = _dev_host(gc.bias_ints(case), case.N, gc.Q_BIAS)
    return x, w, bias


def _i16(bits_u16):
    return torch.from_numpy(np.ascontiguousarray(bits_u16).view(np.int16)).cuda()


def _assert_rows(case, got_i16, rows, gelu_tab, what="output"):
    """got_i16 [M, >= N] int16 view of the device rows; bit for bit against the reference on `rows`"""
    blocks = []                                                                   # (rows, reference bits): computed once, shared with the statistics check
    for r0 in range(0, len(rows), CHUNK):
        rr = rows[r0:r0 + CHUNK]
        bits = gc.reference_bits(case, rr, gelu_tab)
        blocks.append((rr, bits))
        want = _i16(bits)
        got = got_i16[torch.from_numpy(rr).cuda(), :case.N]
        if not torch.equal(got, want):
            bad = (got != want).nonzero()
            i, j = (int(v) for v in bad[0])
            pytest.fail(f"{case.name} {what}: {len(bad)} of {want.numel()} elements differ in rows {rr[0]}..{rr[-1]}; first at row {rr[i]} col {j}: "
                        f"got 0x{int(got[i, j]) & 0xFFFF:04x}, want 0x{int(want[i, j]) & 0xFFFF:04x}")
    return blocks


def _assert_guards(case, cbuf, M, N):
    assert bool((cbuf[:M, N:] == -1).all()), f"{case.name}: a store into the ldc padding"
    assert bool((cbuf[M:] == -1).all()), f"{case.name}: a store past row M"
    assert not bool((cbuf[:M, :N] == -1).any()), f"{case.name}: an output element was never stored"


def _run_plain(case, ncu, gelu_tab):
    """BIAS / GELU / LS_RES through fp_op_gemm, LS_RES_STATS through fp_op_gemm_stats; returns the decoded statistics for the latter"""
    lib, ops = _api()
    plan = _assert_claim(case, case.claims, ncu)
    M, N, K = case.M, case.N, case.K
    x, w, bias = _operands(case)
    gamma = resid = None
    if case.epi in (gc.LS_RES, gc.LS_RES_STATS):
        gamma = _dev_host(gc.gamma_ints(case), N, gc.Q_GAMMA)
        resid = _dev_rows(lambda r: gc.resid_ints(case, r, xp=torch), M, N, case.ld("r"), gc.Q_RESID)
    cbuf = _poison(M + GUARD_ROWS, case.ld("c"))
    stat = None
    if case.epi == gc.LS_RES_STATS:
        stat = torch.full((M, 6), -1, dtype=torch.int32, device="cuda").view(torch.float32)   # word 5 is never written
        ops.check(lib.fp_op_gemm_stats(ops.context(), ops.ptr(x), case.ld("x"), ops.ptr(w), case.ld("w"), ops.ptr(cbuf), case.ld("c"), ops.ptr(bias),
                                       ops.ptr(gamma), ops.ptr(resid), case.ld("r"), M, N, K, float(gc.LN_EPS), ops.ptr(stat), ops.current_stream()),
                  "fp_op_gemm_stats")
    else:
        ops.check(lib.fp_op_gemm(ops.context(), ops.ptr(x), case.ld("x"), ops.ptr(w), case.ld("w"), ops.ptr(cbuf), case.ld("c"), ops.ptr(bias),
                                 ops.ptr(gamma), ops.ptr(resid), case.ld("r"), M, N, K, {gc.BIAS: 0, gc.GELU: 1, gc.LS_RES: 2}[case.epi],
                                 ops.current_stream()), "fp_op_gemm")
    torch.cuda.synchronize()
    assert gc.split_point(M, N, ncu) == plan["row0"], f"{case.name}: the library splits at row {plan['row0']}, the mirror at {gc.split_point(M, N, ncu)}"
    rows = gc.check_rows(case, ncu, split_row=plan["row0"])
    blocks = _assert_rows(case, cbuf, rows, gelu_tab)
    _assert_guards(case, cbuf, M, N)
    if case.epi == gc.LS_RES_STATS:
        _assert_stats(case, stat, blocks)
        plain = _poison(M + GUARD_ROWS, case.ld("c"))                              # the plain LayerScale + residual epilogue on the same operands
        ops.check(lib.fp_op_gemm(ops.context(), ops.ptr(x), case.ld("x"), ops.ptr(w), case.ld("w"), ops.ptr(plain), case.ld("c"), ops.ptr(bias),
                                 ops.ptr(gamma), ops.ptr(resid), case.ld("r"), M, N, K, 2, ops.current_stream()), "fp_op_gemm")
        torch.cuda.synchronize()
        assert torch.equal(plain, cbuf), f"{case.name}: the statistics epilogue does not store the plain epilogue's bits"


def _assert_stats(case, stat, blocks):
    """decoded mean and sigma within 2^-15 relative, rstd within 2^-12 relative, of the statistics of the exact output rows (the records hold
    two-piece bf16 splits, 16 bits; rstd is a 1-ulp reciprocal of the fp32 sigma); every checked row, the last ragged tile included"""
    raw = stat.cpu().numpy()
    for rr, bits in blocks:
        mean, sigma, rstd = gc.row_stats(gc.bits_to_f64(bits))
        dm, ds = gc.decode_record(raw[rr, :4].copy().view(np.uint32))
        dr = raw[rr, 4].astype(np.float64)
        assert (raw[rr, 3].copy().view(np.uint32) == 0).all() and np.isfinite(dr).all(), f"{case.name}: a row record was never copied out"
        assert np.abs(mean).min() > 1.0                                           # the operands keep the means away from zero
        em, es, er = np.abs(dm - mean) / np.abs(mean), np.abs(ds - sigma) / sigma, np.abs(dr - rstd) / rstd
        assert em.max() <= 2.0 ** -15 and es.max() <= 2.0 ** -15 and er.max() <= 2.0 ** -12, (case.name, em.max(), es.max(), er.max())


_ids = dict(ids=lambda c: c.name)


@pytest.mark.parametrize("case", gc.TINY, **_ids)
def test_tiny(case, ncu, gelu_tab):
    _run_plain(case, ncu, gelu_tab)


@pytest.mark.parametrize("case", gc.SMALL, **_ids)
def test_small(case, ncu, gelu_tab):
    _run_plain(case, ncu, gelu_tab)


@pytest.mark.parametrize("case", gc.BIG, **_ids)
def test_big(case, ncu, gelu_tab):
    _run_plain(case, ncu, gelu_tab)


@pytest.mark.parametrize("case", gc.ASM, **_ids)
def test_big_asm(case, ncu, gelu_tab):
    _run_plain(case, ncu, gelu_tab)


@pytest.mark.parametrize("case", gc.SPLIT, **_ids)
def test_row_splits(case, ncu, gelu_tab):
    _run_plain(case, ncu, gelu_tab)


@pytest.mark.parametrize("case", gc.VT_CASES, **_ids)
def test_vt(case, ncu, gelu_tab):
    lib, ops = _api()
    _assert_claim(case, case.claims, ncu)
    M, N, K, npad, H = case.M, case.N, case.K, case.npad, case.heads
    B = M // npad
    x, w, bias = _operands(case)
    numel, guard = B * H * 64 * npad, 4096
    buf = torch.full((numel + 2 * guard,), -1, dtype=torch.int16, device="cuda")
    vt = buf[guard:guard + numel]
    ops.check(lib.fp_op_gemm_vt(ops.context(), ops.ptr(x), case.ld("x"), ops.ptr(w), case.ld("w"), ops.ptr(vt), ops.ptr(bias), M, N, K, npad, H,
                                ops.current_stream()), "fp_op_gemm_vt")
    torch.cuda.synchronize()
    got = vt.view(B, H, 64, npad)
    per = max(1, CHUNK // npad)
    for b0 in range(0, B, per):                                                   # whole crops per block
        b1 = min(B, b0 + per)
        rows = np.arange(b0 * npad, b1 * npad, dtype=np.int64)
        want = _i16(gc.reference_bits(case, rows)).view(b1 - b0, npad, H, 64).permute(0, 2, 3, 1)
        if not torch.equal(got[b0:b1], want):
            bad = (got[b0:b1] != want).nonzero()
            pytest.fail(f"{case.name}: {len(bad)} elements differ in crops {b0}..{b1 - 1}; first at [b, h, d, t] = {[int(v) for v in bad[0]]}")
    assert bool((buf[:guard] == -1).all()) and bool((buf[guard + numel:] == -1).all()), f"{case.name}: a store outside Vt"


@pytest.mark.parametrize("case", gc.PATCH_CASES, **_ids)
def test_patch(case, ncu, gelu_tab):
    lib, ops = _api()
    _assert_claim(case, case.claims, ncu)
    M, N, K, P, npad, off = case.M, case.N, case.K, case.P, case.npad, case.tok_off
    B = M // P
    x, w, bias = _operands(case)
    pos = _dev_host(gc.pos_ints(case), N, gc.Q_POS)
    ldc = case.ld("c")
    tok = _poison(B * npad + GUARD_ROWS, ldc)
    ops.check(lib.fp_op_gemm_patch(ops.context(), ops.ptr(x), case.ld("x"), ops.ptr(w), case.ld("w"), ops.ptr(tok), ldc, ops.ptr(bias), ops.ptr(pos),
                                   M, N, K, P, npad, off, ops.current_stream()), "fp_op_gemm_patch")
    torch.cuda.synchronize()
    rows = np.arange(M, dtype=np.int64)
    want = np.full((B * npad + GUARD_ROWS, ldc), 0xFFFF, dtype=np.uint16)         # cls, register, pad rows and the padding keep the poison
    want[(rows // P) * npad + off + rows % P, :N] = gc.reference_bits(case, rows)
    want = _i16(want)
    if not torch.equal(tok, want):
        bad = (tok != want).nonzero()
        i, j = (int(v) for v in bad[0])
        pytest.fail(f"{case.name}: {len(bad)} elements differ; first at token row {i} (crop {i // npad}, token {i % npad}) col {j}: "
                    f"got 0x{int(tok[i, j]) & 0xFFFF:04x}, want 0x{int(want[i, j]) & 0xFFFF:04x}")


def test_patch_entry_refuses_rows_outside_the_crop():
    lib, ops = _api()
    t = torch.zeros((64, 64), dtype=torch.bfloat16, device="cuda")
    rc = lib.fp_op_gemm_patch(ops.context(), ops.ptr(t), 64, ops.ptr(t), 64, ops.ptr(t), 64, ops.ptr(t), ops.ptr(t), 35, 64, 64, 35, 48, 14,
                              ops.current_stream())
    assert rc != 0 and b"op_gemm_patch" in lib.fp_last_error()


# ---- the LayerNorm chain -----------------------------------------------------------------------------------------------------------------
def _run_chain(ch, route, dev):
    lib, ops = _api()
    M, D, N2 = ch.M, ch.D, ch.N2
    ldo = N2 + 8
    y = _poison(M, D)
    out = _poison(M + GUARD_ROWS, ldo)
    rec = torch.zeros((M, 4), dtype=torch.int32, device="cuda")
    rstd = torch.zeros((M,), dtype=torch.float32, device="cuda")
    ops.check(lib.fp_op_ln_chain(ops.context(), ops.ptr(dev["x1"]), ch.K1, ops.ptr(dev["w1"]), ops.ptr(dev["b1"]), ops.ptr(dev["gamma"]),
                                 ops.ptr(dev["resid"]), ops.ptr(y), M, D, ops.ptr(dev["g_ln"]), ops.ptr(dev["b_ln"]), float(gc.LN_EPS),
                                 ops.ptr(dev["w2"]), N2, ops.ptr(dev["b2"]), ch.mode, ch.n_scaled, float(ch.row_scale), route, ops.ptr(out), ldo,
                                 ops.ptr(rec), ops.ptr(rstd), ops.current_stream()), "fp_op_ln_chain")
    torch.cuda.synchronize()
    return y, out, rec, rstd


@pytest.mark.parametrize("ch", gc.CHAINS, ids=lambda c: c.name)
def test_ln_chain(ch, ncu, gelu_tab):
    """Route equality, bit for bit (consumer output, row records, rstd, guards), the producer's rows against the exact reference, and both
    routes against the float64 restatement of the fold within the bound derived in _gemm_cases.chain_reference.

    The worst |diff| / bound of each case is printed (pytest -s); a ratio above 1 is a finding, not a reason to widen the bound.  Measured
    on an MI355X (256 CUs), identical on both routes: chain_tiny_160_m0 0.926, chain_tiny_160_m1 0.877, chain_tiny_150_m0_qscale 0.910,
    chain_tiny_17_m1 0.883, chain_small_2048_m0 0.957, chain_small_2090_m1 0.913, chain_splitmid_8256_m0 0.954, chain_splitmid_8250_m1
    0.912, chain_finalize_49152_m0 0.954, chain_finalize_48897_m1 0.909.  The worst elements sit next to a bf16 rounding boundary of the
    output (for example got 2.03125 against 2.0474: half an ulp of 2^-6 is the dominant term of the bound), so the ratios approach 1
    from the output rounding alone, not from the statistics."""
    import dataclasses
    _assert_claim(ch, ch.claims, ncu)
    prod = dataclasses.replace(ch.producer, subset=ch.M > 10000)
    w2, b2, g_ln, b_ln = gc.chain_operands(ch)
    x1, w1, b1 = _operands(prod)
    dev = dict(x1=x1, w1=w1, b1=b1, gamma=_dev_host(gc.gamma_ints(prod), ch.D, gc.Q_GAMMA),
               resid=_dev_rows(lambda r: gc.resid_ints(prod, r, xp=torch), ch.M, ch.D, ch.D, gc.Q_RESID),
               w2=_dev_host(w2, ch.D, 1.0), b2=_dev_host(b2, ch.N2, 1.0), g_ln=_dev_host(g_ln, ch.D, 1.0), b_ln=_dev_host(b_ln, ch.D, 1.0))
    y0, out0, rec0, rstd0 = _run_chain(ch, 0, dev)
    y1, out1, rec1, rstd1 = _run_chain(ch, 1, dev)
    rows = gc.check_rows(prod, ncu)
    _assert_rows(prod, y0, rows, gelu_tab, "producer rows")
    assert not bool((y0 == -1).any()) and torch.equal(y0, y1)
    for out in (out0, out1):
        _assert_guards(prod, out, ch.M, ch.N2)
    assert torch.equal(out0, out1), f"{ch.name}: the routes differ in {int((out0 != out1).sum())} output elements"
    assert torch.equal(rec0, rec1) and torch.equal(rstd0.view(torch.int32), rstd1.view(torch.int32)), f"{ch.name}: the routes differ in the row records"
    assert bool((rec0[:, 3] == 0).all()) and bool(torch.isfinite(rstd0).all()), f"{ch.name}: a row record was never written"
    # the float64 restatement on the checked rows (every row of the small cases)
    sel = rows if len(rows) <= 2200 else np.unique(np.concatenate([rows[:700], rows[-700:], rows[::max(1, len(rows) // 700)]]))
    yv = gc.bits_to_f64(y0.cpu().numpy().view(np.uint16))
    ref, bound = gc.chain_reference(ch, yv, sel)
    got = gc.bits_to_f64(out1[:ch.M, :ch.N2].cpu().numpy().view(np.uint16)[sel])
    ratio = np.abs(got - ref) / bound
    worst = np.unravel_index(int(ratio.argmax()), ratio.shape)
    print(f"\n[chain] {ch.name}: worst |diff|/bound = {ratio.max():.3f} at row {sel[worst[0]]} col {worst[1]} "
          f"(got {got[worst]:.6g}, ref {ref[worst]:.6g}, bound {bound[worst]:.3g})")
    assert ratio.max() <= 1.0
    mean, sigma, rstd = gc.row_stats(yv[sel])
    dm, ds = gc.decode_record(rec1.cpu().numpy().view(np.uint32)[sel])
    assert np.abs(mean).min() > 1.0                                               # shown for the exact rows by tests/test_gemm_cases_cpu.py
    assert (np.abs(dm - mean) <= 2.0 ** -15 * np.abs(mean)).all() and (np.abs(ds - sigma) <= 2.0 ** -15 * sigma).all()
    assert (np.abs(rstd1.cpu().numpy().astype(np.float64)[sel] - rstd) <= 2.0 ** -12 * rstd).all()
