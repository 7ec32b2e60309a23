"""No-GPU proof obligations of tests/_gemm_cases.py: every case reaches the branch it claims on 256 CUs, the exact operands really are
exact (every partial sum below 2^24 quanta, float32 and float64 evaluation of the rounding chains agree), the rounding points are exercised
(values bf16 cannot represent, exact ties) and round_bf16_rne is torch's round-to-nearest-even on every bf16 neighbourhood."""
import numpy as np
import pytest
import torch

from tests import _gemm_cases as gc

# subset rows of the largest cases only: the operands are pure functions of (row, column), so this costs no full matrix
def _rows(case, cap=1500):
    rows = gc.check_rows(case)
    if len(rows) > cap:
        rows = np.unique(np.concatenate([rows[:cap // 3], rows[-cap // 3:], rows[::max(1, len(rows) // (cap // 3))]]))
    return rows


def test_case_names_are_unique():
    names = [c.name for c in gc.EXACT_CASES] + [c.name for c in gc.CHAINS]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("case", gc.EXACT_CASES, ids=lambda c: c.id)
def test_case_lands_in_the_branch_it_claims(case):
    assert case.branch(256) == case.claims
    for which in "xwcr":
        assert case.ld(which) % 8 == 0
    assert case.ld("c") > case.N and case.N % 16 == 0 and case.K % 64 == 0
    if case.claims == "big_asm":
        assert case.ld("c") % 64 == 0 and case.ld("x") % 64 == 0 and case.ld("w") % 64 == 0
    if case.epi == gc.PATCH:
        assert case.M % case.P == 0 and case.tok_off + case.P <= case.npad
    if case.epi == gc.VT:
        assert case.M % case.npad == 0 and case.npad % 16 == 0 and case.N == case.heads * 64


def test_every_branch_label_is_claimed():
    claimed = {c.claims for c in gc.EXACT_CASES} | {c.claims for c in gc.CHAINS}
    for label in ("tiny64", "small128", "big_hip", "big_hip_stream", "big_asm", "split_big+tiny64", "split_mid+tiny64",
                  "finalize_then_big_hip"):
        assert label in claimed, label
    for tier in ("tiny64", "small128", "big_hip", "big_asm"):                      # padded input strides in at least one case per tier
        assert any(c.claims == tier and (c.ld("x") > c.K or c.ld("w") > c.K or (c.ldr and c.ldr > c.N)) for c in gc.EXACT_CASES), tier


@pytest.mark.parametrize("ch", gc.CHAINS, ids=lambda c: c.name)
def test_chain_lands_in_the_branch_it_claims(ch):
    assert ch.branch(256, ln_part=True) == ch.claims
    plain = ch.branch(256, ln_part=False)
    assert ch.claims in (plain, "finalize_then_" + plain)                        # handing the partial sums over never changes the tier
    assert gc.fuses_ln_part(ch.M, ch.N2) == (not ch.claims.startswith("finalize"))
    assert ch.M >= 16 and ch.D % 64 == 0 and ch.N2 % 64 == 0
    prod = ch.producer
    assert gc.branch(prod.M, prod.N, prod.K, prod.epi) in ("tiny64", "small128", "big_hip", "split_mid+tiny64")


def test_dispatch_mirror_on_the_documented_shapes():
    """shapes whose path the sources state in words (gemm_bf16.hip launch_epi, tests/test_gpu_kernels.py)"""
    assert gc.branch(19152, 1024, 1024, gc.LS_RES) == "split_big+tiny64"          # the video path's ~20-crop batches
    assert gc.branch(19152, 1024, 1024, gc.LS_RES, row_split=False) == "small128"
    assert gc.branch(6 * 1376, 1024, 1024, gc.BIAS) == "split_mid+tiny64"         # 520 tiles = one 128x128 round + 8
    assert gc.branch(1370 + 6, 1024, 1024, gc.BIAS) == "tiny64"                   # one 518^2 crop: 88 tiles
    assert gc.branch(70000, 1024, 1024, gc.BIAS) == "split_big+small128"          # 4.28 rounds: 4 on the big tier, 4464 rows on 128x128
    assert gc.branch(70000, 1024, 1024, gc.BIAS, row_split=False) == "big_hip_stream"
    assert gc.branch(70000, 1024, 4096, gc.LS_RES, row_split=False) == "big_asm"
    assert gc.branch(70000, 1024, 4096, gc.LS_RES, ldx=4096 + 8, row_split=False) == "big_hip_stream"
    assert gc.branch(65536, 1024, 1024, gc.BIAS) == "big_hip"                     # 128 MiB exactly: not above the streaming threshold
    assert gc.branch(2600, 1024, 4096, gc.LS_RES) == "tiny64"                     # 168 tiles of 128x128 < 256 CUs
    assert gc.branch(52 * 1376, 1024, 1024, gc.VT) == "big_hip_stream"
    assert gc.branch(49152, 256, 256, gc.LN_BIAS, ln_part=True) == "finalize_then_big_hip"
    assert gc.branch(49151 - 255, 256, 256, gc.LN_BIAS, ln_part=True) == "split_mid+tiny64"   # 191 big tiles: the small tiers finalise
    assert gc.branch(48897, 256, 64, gc.BIAS, n_cu=304, row_split=False) == "small128"   # 75 % fill rule: 192 tiles < 0.75 x 304


@pytest.mark.parametrize("case", gc.EXACT_CASES, ids=lambda c: c.id)
def test_exact_cases_are_exact(case):
    rows = _rows(case)
    acc, bound = gc.acc_quanta(case, rows)
    assert bound < 2 ** 24, bound
    a = gc.amplitude(case.K) + 3                                                  # the analytic bound covers the rows not evaluated here
    assert case.K * a * a + 4 * 128 < 2 ** 24
    for ints in (gc.x_ints(case, rows), gc.w_ints(case), gc.bias_ints(case), gc.gamma_ints(case), gc.resid_ints(case, rows)):
        assert np.abs(ints).max() < 256                                           # 8 significant bits: bf16 holds every operand exactly
    r64 = gc.reference(case, rows, dtype=np.float64)
    r32 = gc.reference(case, rows, dtype=np.float32)
    assert np.array_equal(gc.bf16_bits(r64), gc.bf16_bits(r32)) and np.array_equal(r64, r32)
    assert np.isfinite(r64).all() and not (gc.bf16_bits(r64) == 0xFFFF).any()     # the poison pattern is never a result
    assert np.array_equal(gc.reference_bits(case, rows), gc.bf16_bits(r64))       # the fast path of the GPU tests is the same function


def test_rounding_points_are_exercised():
    """per case: a share of the accumulators is not representable in bf16; ties: in every case with >= 4096 outputs, and over the smaller ones
    together"""
    small_n = small_ties = 0
    for case in gc.EXACT_CASES:
        acc, _ = gc.acc_quanta(case, _rows(case))
        nonrep, ties = gc.rounding_shares(acc)
        if case.kind == "rand":
            assert nonrep > 0.25, (case.name, nonrep)
        else:
            assert nonrep > 0.0, (case.name, nonrep)
        if acc.size >= 4096 and case.kind == "rand":
            assert ties > 0.01, (case.name, ties)
        else:
            small_n += acc.size
            small_ties += ties * acc.size
    assert small_ties / small_n > 0.01


_STATS_CASES = [c for c in gc.EXACT_CASES if c.epi == gc.LS_RES_STATS] + [ch.producer for ch in gc.CHAINS]


@pytest.mark.parametrize("case", _STATS_CASES, ids=lambda c: c.name)
def test_statistics_rows_have_means_away_from_zero(case):
    """the GPU tests bound the decoded mean relative to the mean itself: every row they check has |mean| > 1 (and sigma > 1), so that bound is
    never a statement about a cancelled sum"""
    import dataclasses
    rows = gc.check_rows(dataclasses.replace(case, subset=case.subset or case.M > 10000 and case.claims == ""))
    for r0 in range(0, len(rows), 8192):
        mean, sigma, _ = gc.row_stats(gc.bits_to_f64(gc.reference_bits(case, rows[r0:r0 + 8192])))
        assert np.abs(mean).min() > 1.0 and sigma.min() > 1.0, (case.name, np.abs(mean).min(), sigma.min())


def test_ls_res_chain_rounds_three_times():
    """the three rounding points matter: dropping any of them changes outputs of the LS_RES cases (else the reference could not tell the
    orders apart)"""
    case = next(c for c in gc.SMALL if c.epi == gc.LS_RES)
    rows = np.arange(256, dtype=np.int64)
    acc, _ = gc.acc_quanta(case, rows)
    v = acc * gc.Q
    g, r = gc.gamma_ints(case)[None, :] * gc.Q_GAMMA, gc.resid_ints(case, rows) * gc.Q_RESID
    ref = gc.reference(case, rows)
    gamma_first = gc.round_bf16_rne(gc.round_bf16_rne(v * g) + r)                  # multiplies before the first rounding
    no_mid = gc.round_bf16_rne(gc.round_bf16_rne(v) * g + r)                       # no rounding of the product
    assert (ref != gamma_first).mean() > 0.05 and (ref != no_mid).mean() > 0.05


def test_hash_ints_numpy_equals_torch():
    r, c = np.arange(0, 400000, 997, dtype=np.int64)[:, None], np.arange(0, 2048, 13, dtype=np.int64)[None, :]
    a = gc.hash_ints(r, c, 7, -24, 27)
    b = gc.hash_ints(torch.from_numpy(r), torch.from_numpy(c), 7, -24, 27).numpy()
    assert np.array_equal(a, b) and a.min() == -24 and a.max() == 27
    assert abs(a.mean() - 1.5) < 0.3 and len(np.unique(a)) == 52


def test_round_bf16_rne_is_torch_on_every_neighbourhood():
    """all fp32 values at, half a bf16 ulp around and one fp32 ulp beside the rounding boundaries of all 65 536 bf16 patterns"""
    base = np.arange(65536, dtype=np.int64) << 16
    bits = np.concatenate([base + d for d in (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF, -1, -0x7FFF, -0x8000, -0x8001)])
    bits = np.unique(bits[(bits >= 0) & (bits < 2 ** 32)]).astype(np.uint32)
    f32 = bits.view(np.float32)
    want = torch.from_numpy(f32.copy()).to(torch.bfloat16)
    with np.errstate(invalid="ignore"):
        got = gc.round_bf16_rne(f32.astype(np.float64))
    nan = np.isnan(f32)
    assert np.array_equal(np.isnan(got), nan) and bool(torch.isnan(want.float()).numpy()[nan].all())
    assert np.array_equal(gc.bf16_bits(got[~nan]), want.view(torch.int16).numpy().view(np.uint16)[~nan])
    assert len(bits) > 9 * 65536 // 2


def test_chain_reference_is_layernorm():
    """the float64 restatement of the fold equals LayerNorm -> Linear (-> GELU) in float64 up to the bf16 rounding of W gamma"""
    ch = gc.CHAINS[1]
    g = np.random.default_rng(3)
    y = gc.round_bf16_rne(g.normal(1.0, 2.0, (64, ch.D)))
    w2, b2, g_ln, b_ln = gc.chain_operands(ch)
    ref, bound = gc.chain_reference(ch, y)
    yt = torch.nn.functional.layer_norm(torch.from_numpy(y), (ch.D,), torch.from_numpy(g_ln), torch.from_numpy(b_ln), gc.LN_EPS)
    want = torch.nn.functional.gelu(yt @ torch.from_numpy(w2).T + torch.from_numpy(b2)).numpy()
    assert np.abs(ref - want).max() < 0.02 and np.abs(ref - want).mean() < 1e-3
    assert (bound > 0).all() and np.median(bound / np.maximum(np.abs(ref), 1e-3)) < 0.05    # not vacuous
