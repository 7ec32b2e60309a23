"""No-GPU proof obligations of tests/_gemm_cases.py: every case reaches the branch it claims on 256 CUs, the exact operands really are
exact (every partial sum below 2^24 quanta, float32 and float64 evaluation of the rounding chains agree), the rounding points are exercised
(values bf16 cannot represent, exact ties) and round_bf16_rne is torch's round-to-nearest-even on every bf16 neighbourhood."""
import shutil
import subprocess
from pathlib import Path

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


# ---- the library's own statement of the dispatch (csrc/gemm_plan.h) against the mirror -----------------------------------------------------
ROOT = Path(__file__).resolve().parent.parent
LN_EPIS = (gc.LN_BIAS, gc.LN_GELU, gc.LN_VT)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """tools/gemm_plan_host_check.cpp under the host sanitizers: [(M, N, K, epi, ldx, ldw, ln_part, no_split, ncu)] -> [(label, row0, rings,
    grids)], exit status 0 (its own checks of every plan and the sanitizers)"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_host_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "freepose_amd" / "csrc"),
           str(ROOT / "tools" / "gemm_plan_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(shapes):
        text = "".join(" ".join(str(int(v)) for v in s) + "\n" for s in shapes)
        r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        out = []
        for ln in r.stdout.splitlines():
            label, row0, ring, grid = ln.split()
            out.append((label, int(row0.split("=")[1]), tuple(int(v) for v in ring.split("=")[1].split(",")),
                        tuple(int(v) for v in grid.split("=")[1].split(","))))
        assert len(out) == len(shapes)
        return out
    return run


def _mirror(shape):
    M, N, K, epi, ldx, ldw, ln_part, no_split, ncu = shape
    return gc.plan(M, N, K, epi, ncu, ldx, ldw, not no_split, bool(ln_part))


def _assert_plans_equal_mirror(plan_check, shapes):
    got = plan_check(shapes)
    for s, g in zip(shapes, got):
        label, row0 = _mirror(s)
        assert (g[0], g[1]) == (label, row0), f"M N K epi ldx ldw ln_part no_split ncu = {s}: gemm_plan.h says {g[0]} row0={g[1]}, the mirror {label} row0={row0}"
        if s[3] not in (gc.VT, gc.LN_VT, gc.PATCH) and not s[7]:
            assert gc.split_point(s[0], s[1], s[8]) == g[1], s
    return got


def test_plan_of_every_committed_case_is_its_claim(plan_check):
    """planner == mirror == the case's claim at 256 CUs, chains with the partial sums handed over; and the tiny cases that
    tests/test_gpu_gemm_branches.py names "a K ring of depth 2 .. 4" really run on rings of 2, 3 and 4 buffers"""
    cases = [(c.M, c.N, c.K, c.epi, c.ld("x"), c.ld("w"), 0, 0, 256) for c in gc.EXACT_CASES]
    chains = [(c.M, c.N2, c.D, gc.LN_BIAS if c.mode == 0 else gc.LN_GELU, c.D, c.D, 1, 0, 256) for c in gc.CHAINS]
    got = _assert_plans_equal_mirror(plan_check, cases + chains)
    for c, g in zip(list(gc.EXACT_CASES) + list(gc.CHAINS), got):
        assert g[0] == c.claims, (c.name, g)
    rings = {g[2][0] for c, g in zip(gc.EXACT_CASES, got) if c in gc.TINY}
    assert rings == {2, 3, 4}, rings


SPOT_SHAPES = [   # (M, N, K, epi, ldx, ldw, ln_part, no_split, ncu): the shapes of test_dispatch_mirror_on_the_documented_shapes
    (19152, 1024, 1024, gc.LS_RES, 1024, 1024, 0, 0, 256), (19152, 1024, 1024, gc.LS_RES, 1024, 1024, 0, 1, 256),
    (6 * 1376, 1024, 1024, gc.BIAS, 1024, 1024, 0, 0, 256), (1370 + 6, 1024, 1024, gc.BIAS, 1024, 1024, 0, 0, 256),
    (70000, 1024, 1024, gc.BIAS, 1024, 1024, 0, 0, 256), (70000, 1024, 1024, gc.BIAS, 1024, 1024, 0, 1, 256),
    (70000, 1024, 4096, gc.LS_RES, 4096, 4096, 0, 1, 256), (70000, 1024, 4096, gc.LS_RES, 4096 + 8, 4096, 0, 1, 256),
    (65536, 1024, 1024, gc.BIAS, 1024, 1024, 0, 0, 256), (2600, 1024, 4096, gc.LS_RES, 4096, 4096, 0, 0, 256),
    (52 * 1376, 1024, 1024, gc.VT, 1024, 1024, 0, 0, 256), (49152, 256, 256, gc.LN_BIAS, 256, 256, 1, 0, 256),
    (49151 - 255, 256, 256, gc.LN_BIAS, 256, 256, 1, 0, 256), (48897, 256, 64, gc.BIAS, 64, 64, 0, 1, 304),
]


def test_plan_on_the_documented_shapes(plan_check):
    got = _assert_plans_equal_mirror(plan_check, SPOT_SHAPES)
    assert [g[0] for g in got] == ["split_big+tiny64", "small128", "split_mid+tiny64", "tiny64", "split_big+small128", "big_hip_stream", "big_asm",
                                   "big_hip_stream", "big_hip", "tiny64", "big_hip_stream", "finalize_then_big_hip", "split_mid+tiny64", "small128"]
    assert got[0][1] == 16384 and got[0][3] == (256, 704)          # one whole round of 256 big tiles, 2768 rows on 44 x 16 one-wave tiles
    assert got[3][2] == (4, 0) and got[3][3] == (22 * 16, 0)       # one 518^2 crop: 352 tiles of 64x64 on the deepest ring


def sweep_shapes(n=120000, seed=20261):
    """seeded: M log-uniform in [1, 400 000] or k 128 or k 256 +- 1; N 16 .. 8192 with ragged values; K in {64, 256, 1024, 2048, 4096}; all nine
    epilogues (their own constraints kept: N % 64 for the LN / statistics / V^T forms, M % 16 for V^T, M >= 16 for LN); ln_part on half the
    LN launches; row split on and off; ldx in {K, K + 8}; 32 .. 304 CUs"""
    g = np.random.default_rng(seed)
    kind = g.integers(0, 3, n)
    m_log = np.exp(g.uniform(0.0, np.log(400000.0), n)).astype(np.int64)
    m_128 = g.integers(1, 400000 // 128 + 1, n) * 128
    m_256 = g.integers(1, 400000 // 256, n) * 256 + g.choice([-1, 1], n)
    M = np.clip(np.where(kind == 0, m_log, np.where(kind == 1, m_128, m_256)), 1, 400000)
    n_any = np.array([16, 48, 80, 144, 256, 272, 384, 400, 768, 1024, 1040, 1536, 1936, 2048, 3072, 4096, 4112, 8176, 8192])
    n_64 = np.array([64, 192, 256, 320, 384, 768, 1024, 1088, 1536, 1984, 2048, 3072, 4096, 4160, 8128, 8192])
    epi = g.integers(0, 9, n)
    plain = np.isin(epi, (gc.BIAS, gc.GELU, gc.LS_RES, gc.PATCH))
    N = np.where(plain, g.choice(n_any, n), g.choice(n_64, n))
    trans = np.isin(epi, (gc.VT, gc.LN_VT))
    M = np.where(trans, cdiv16(M), M)
    M = np.where(np.isin(epi, LN_EPIS), np.maximum(M, 16), M)
    K = g.choice([64, 256, 1024, 2048, 4096], n)
    ldx = K + 8 * g.integers(0, 2, n)
    ln_part = np.isin(epi, LN_EPIS) & (g.integers(0, 2, n) == 1)
    no_split = g.integers(0, 2, n)
    ncu = g.choice([32, 64, 120, 256, 304], n)
    return [tuple(int(v) for v in row) for row in zip(M, N, K, epi, ldx, K, ln_part, no_split, ncu)]


def cdiv16(m):
    return (m + 15) // 16 * 16


# Every form of label the sweep must produce, so that it cannot silently cover one side of a threshold only: the five tiers and both splits
# with each remainder tier that occurs.  The remainder of a split_big is less than a round + one row of tiles, which can still be a filled
# round (big_hip, big_asm) but never 128 MiB of output; a split_mid whose remainder fills the CUs with 128x128 tiles saves no round, so its
# remainder is always tiny64.  FINALIZED: what follows finalize_then_ — V^T launches on any tier, row-major ones from 192 big tiles on;
# never big_asm (the product has no hand-scheduled LN kernel) and with it no split_big+big_asm.
SWEEP_LABELS = {"tiny64", "small128", "big_hip", "big_hip_stream", "big_asm", "split_big+tiny64", "split_big+small128", "split_big+big_hip",
                "split_big+big_asm", "split_mid+tiny64"}
FINALIZED = {"tiny64", "small128", "big_hip", "big_hip_stream", "split_big+tiny64", "split_big+small128", "split_big+big_hip", "split_mid+tiny64"}


def test_plan_equals_mirror_on_a_sweep(plan_check):
    shapes = sweep_shapes()
    assert len(shapes) >= 100000
    got = _assert_plans_equal_mirror(plan_check, shapes)
    labels = {g[0] for g in got}
    plain = {lb for lb in labels if not lb.startswith("finalize_then_")}
    assert plain == SWEEP_LABELS, sorted(plain ^ SWEEP_LABELS)
    fin = {lb[len("finalize_then_"):] for lb in labels - plain}
    assert fin == FINALIZED, sorted(fin ^ FINALIZED)
    for s, g in zip(shapes, got):                                                 # what a split and a finalisation are for
        if g[0].startswith("finalize_then_"):
            assert s[6] and s[3] in LN_EPIS
        if g[1]:
            assert not s[7] and s[3] not in (gc.VT, gc.LN_VT, gc.PATCH) and 0 < g[1] < s[0]


def test_dispatch_mirror_on_the_documented_shapes():
    """shapes whose path the sources state in words (csrc/gemm_plan.h, tests/test_gpu_kernels.py)"""
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


# ---- the kernels' index arithmetic (csrc/gemm_core.h) under the host sanitizers --------------------------------------------------------------
@pytest.fixture(scope="module")
def core_check(tmp_path_factory):
    """tools/gemm_core_host_check.cpp built with -fsanitize=address,undefined and run once: its output lines"""
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path_factory.mktemp("gemm_core") / "gemm_core_host_check"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(ROOT / "freepose_amd" / "csrc"),
           str(ROOT / "tools" / "gemm_core_host_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout.splitlines()


def test_core_host_check_is_clean(core_check):
    """DMA -> read round trip, tile order, accumulator map, ring and waits, stream-K partition, LDS budget: every check held, no sanitizer report"""
    assert core_check[-1] == "ok"
    assert not any(ln.startswith("FAILED") for ln in core_check)


def test_core_fragment_reads_are_conflict_free(core_check):
    """the kernels' comments claim conflict-free fragment reads: degree 1 under the ds_read_b128 bank model for every geometry, both operands,
    and for the hand-scheduled kernel's image; the slab's read is conflict-free, its write is recorded as the program prints it"""
    recs = {}
    for ln in core_check:
        if ln.startswith("conflict "):
            f = ln.split()
            recs[f[1]] = dict(kv.split("=") for kv in f[2:])
    geos = ["big256_4x4", "big256_4x4_gelu", "big256_4x4_trans", "small128_2x2", "small128_2x2_gelu", "small128_2x2_trans", "tiny64_2x1",
            "tiny64_2x1_gelu", "tiny64_1x1_trans", "lab128_4x2", "lab128_2x4_trans"]
    for g in geos:
        assert recs[g]["R"] == "1" and recs[g]["C"] == "1", (g, recs[g])
        assert int(recs[g]["lds"]) <= 160 * 1024
    for g in ("asm256_4waves", "asm256_8waves", "asm128_4waves"):
        assert recs[g] == {"W": "1", "X": "1"}, (g, recs[g])
    assert recs["slab"]["read"] == "1"
    assert recs["slab"]["write"] == "2"            # two lanes of a pass share a bank on the phase-1 write (profiles/gemm_kernel_refactor.md)
    # the rings the plan may ask for fit: the tiny tier's kernels take up to 8 buffers, the others 2
    assert {g: recs[g]["ring_max"] for g in geos if g.startswith("tiny")} == {"tiny64_2x1": "8", "tiny64_2x1_gelu": "8", "tiny64_1x1_trans": "8"}
    assert all(recs[g]["ring_max"] == "2" for g in geos if not g.startswith("tiny"))
