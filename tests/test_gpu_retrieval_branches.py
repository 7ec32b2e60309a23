"""Every scan, select, merge and scorer branch of csrc/retrieval.hip, and both row normalisers of csrc/vit_misc.hip, against the C oracle bit
for bit and, where one exists, an independent numpy reference (tests/_retrieval_cases.py; tests/test_retrieval_cases_cpu.py shows without a
GPU that every case reaches the branch named here).  No tolerance appears in this file except the derived bound of the scan matrix.  NaN mixed
with numbers is left out: the oracle's comparator does not define an order for it.

  test                               case                       kernel / branch
  test_select_matrix                 n1 .. n49, n100, n1024     topk_select_reg_kernel: staging (16-byte groups, ragged tail), ownership of 48 keys
                                                                per thread, L = 0 (fewer than k non-empty threads), k = N; fast path
                                     n49151, spread*, neg, den  fast path (rank sort of M <= KMAX candidates) at k = 1, 100; counting search at k = 1024
                                     m1024 / m1025              M == KMAX stays on the fast path, M == KMAX + 1 leaves it by a single key
                                     plat2000_k100              counting search with 0 < L < T < G, need_eq cut inside a thread, k <= 256 rank sort
                                     plat2000_k257/500/1024     counting search with 0 < L < T < G, bitonic sort (257 and 500 pad n2)
                                     plat_ragged_*              the plateau over the last N % 48 ragged keys of the row
                                     plat40000_*                packed 16+16-bit scan with the upper count >= 2^15 and a non-zero lower count
                                     *49153, *60001, *65536     topk_select_kernel<true> (key row in LDS)
                                     *65537, *106501, plat70000 topk_select_kernel<false> (key row in global memory); a plateau > 65 535
                                     ohb*                       all keys in one high-byte bin (LDS atomics on one address)
                                     exact*                     `c + hist[b] == k` exactly in the high-byte (k = 100) and low-byte (k = 1024) scans
                                     *_offmax                   idx_offset = 2^31 - 1 - N
  test_stale_pad_keys_stay_out       N = 9, 4999, 49151, 60001  pad keys [N, ldk) of the recycled workspace hold +inf keys of an earlier call
  test_scan_forms                    D x Q                      bank_scan_kernel<NCH, QT, FULL>: D = 8 / 384 (1, partial), 512 (1, FULL), 520 (2, partial),
                                                                1024 (2, FULL), 1032 (3, partial), 1536 (3, FULL); passes of 1, 4, 4+1, 4+4, 4+4+1 queries
  test_scan_rows_per_wave            rows0 .. rows21            rows a wave owns: 0/1 (idle waves), 1 .. 12 (prologue fetches only), 13 and 21 (the in-loop
                                                                fetch(bufB) once and twice); both run lengths (rem != 0)
  test_scan_rows_per_wave_d1536      rows5, rows13              the same with three 16-byte loads per lane and row
  test_scan_q9_equals_nine_q1                                   query passes are independent
  test_topk_merge                    C1 .. C8192                topk_merge_kernel: C = 1, non-powers of two, 8192 (64 KB of dynamic LDS), k = C,
                                                                ties under shuffled indices, +-inf, -inf/2^31-1 padding, arbitrary f32 scores
  test_template_scorers_normed       ts1_T1 .. T8               template_dots_normed_kernel: a wave owns 1 .. 8 templates: every exit of the three-buffer
                                                                rotation on the first, second and third turn
                                     ts_eq_T, ts586, tail_waves TS = T; waves owning 1 and 2; trailing waves with pidx >= P
  test_template_scorers_raw          stride_*                   template_dots_kernel: T*P > 16 384 rows (waves stride and prefetch), T*P % 4 != 0
  test_template_mean                 P1 .. P65                  template_mean_kernel: P around the wave width, zero weights, an all-zero weight row (NaN)
  test_div_rbf_*                                                div_rbf in template_dots_kernel and rerank_views_kernel: every bf16 mantissa over
                                                                every bf16 norm mantissa; denormal quotients, 1 342 of them in the fallback window
  test_rerank_views                  D8, D384, D1536            rerank_views_kernel<1 / 3>: nv = 0 .. 1030 (clamped to 1024), k around the 8-wide blocks
                                                                of the pairwise sum, a mesh named twice, exactly tied views
  test_l2_normalize_*                                           l2norm_rows_vec_kernel<1,2,3> and the scalar l2norm_rows_kernel (misaligned, D > 1536)
"""
import numpy as np
import pytest
import torch

from tests import _retrieval_cases as rc

pytestmark = pytest.mark.gpu

GUARD = 64          # elements of poison kept on both sides of an output buffer


def _fo():
    from oracle import fp_oracle as fo
    return fo


def _dev_bits(b):
    return _fo().bits_to_torch(b).cuda()


def _poisoned(numel, dtype):
    raw = torch.full(((numel + 2 * GUARD) * dtype.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
    buf = raw.view(dtype)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel):
    g = torch.cat([buf[:GUARD], buf[GUARD + numel:]]).view(torch.uint8)
    return bool((g == 0xFF).all())


def _bank_topk_poisoned(bank_d, q_d, k, off):
    """fp_bank_topk through the C ABI into the middle of buffers filled with 0xFF bytes (a NaN score, index -1: neither can be a result).  A
    rank slot no thread wrote keeps the poison; a store outside the output shows in the guards."""
    from freepose_amd import _lib, ops
    lib = _lib.load()
    N, D = bank_d.shape
    Q = q_d.shape[0]
    sbuf, s = _poisoned(Q * k, torch.float32)
    ibuf, i = _poisoned(Q * k, torch.int32)
    ops.check(lib.fp_bank_topk(ops.context(), ops.ptr(bank_d), N, D, ops.ptr(q_d), Q, k, int(off), ops.ptr(s), ops.ptr(i),
                               ops.current_stream()), "fp_bank_topk")
    torch.cuda.synchronize()
    assert _guards_intact(sbuf, Q * k) and _guards_intact(ibuf, Q * k), "a store outside the output"
    return s.cpu().numpy().reshape(Q, k), i.cpu().numpy().reshape(Q, k)


def _merge_poisoned(cs_d, ci_d, k):
    from freepose_amd import _lib, ops
    lib = _lib.load()
    Q, Cn = cs_d.shape
    sbuf, s = _poisoned(Q * k, torch.float32)
    ibuf, i = _poisoned(Q * k, torch.int32)
    ops.check(lib.fp_topk_merge(ops.context(), ops.ptr(cs_d), ops.ptr(ci_d), Q, Cn, k, ops.ptr(s), ops.ptr(i), ops.current_stream()),
              "fp_topk_merge")
    torch.cuda.synchronize()
    assert _guards_intact(sbuf, Q * k) and _guards_intact(ibuf, Q * k), "a store outside the output"
    return s.cpu().numpy().reshape(Q, k), i.cpu().numpy().reshape(Q, k)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


# ---- 3.1 select matrix ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    """bank id -> (score bits, device bank, oracle scores [3, kmax], oracle indices [3, kmax] at offset 0), built on first use, never changed"""
    cache = {}

    def get(bank_id):
        if bank_id not in cache:
            bits = rc.SELECT_BANKS[bank_id]()
            bank = rc.planted_bank(bits)
            s_o, i_o = _fo().bank_topk(bank, rc.planted_queries(), min(len(bits), rc.KMAX))
            cache[bank_id] = (bits, _dev_bits(bank), s_o, i_o)
        return cache[bank_id]
    return get


@pytest.mark.parametrize("case", rc.SELECT_CASES, ids=[c[0] for c in rc.SELECT_CASES])
def test_select_matrix(planted, case):
    """planted scores (D = 8), Q = 3: query 0 sees the planted scores, query 1 their negation (the order reversed), query 2 their double.
    Checked against the oracle (its top-kmax, cut to k: the order is total) and against topk_ref."""
    cid, bank_id, k, off, claim = case
    bits, bank_d, s_o, i_o = planted(bank_id)
    assert rc.select_path(rc.key16(bits), k)["path"] == claim
    s_g, i_g = _bank_topk_poisoned(bank_d, _dev_bits(rc.planted_queries()), k, off)
    assert np.array_equal(i_g, (i_o[:, :k].astype(np.int64) + off).astype(np.int32)), cid
    assert _same_bits(s_g, s_o[:, :k]), cid
    for qi, qb in enumerate((rc.Q_E0, rc.Q_NEG, rc.Q_TWO)):
        s_r, i_r = rc.topk_ref(rc.planted_scores(bits, qb), k, off)
        assert np.array_equal(i_g[qi], i_r) and _same_bits(s_g[qi], s_r), (cid, qi)


def test_stale_pad_keys_stay_out():
    """fp_bank_topk takes its key rows from a recycled workspace.  An all-+inf bank of 106 501 rows fills it with the largest real key; the
    pad keys [N, ldk) of the calls that follow (N % 8 != 0) still hold it, in every select kernel but the global-memory one"""
    from freepose_amd import ops
    fo = _fo()
    q = _dev_bits(rc.planted_queries()[[0, 0, 2]])                       # +inf under all three (no -e0: +inf is what has to be left behind)
    inf_bank = _dev_bits(rc.planted_bank(np.full(106501, 0x7F80, np.uint16)))
    for N in rc.STALE_PAD_N:
        assert N % 8 != 0
        s, _ = ops.bank_topk(inf_bank, q, 1024)
        assert bool(torch.isinf(s).all())
        bits = rc.key_to_bits(rc._finite_keys(rc._rng(N), N))
        bank = rc.planted_bank(bits)
        k = min(N, 1024)
        s_g, i_g = _bank_topk_poisoned(_dev_bits(bank), q, k, 0)
        s_o, i_o = fo.bank_topk(bank, rc.planted_queries()[[0, 0, 2]], k)
        assert not np.isposinf(s_g[:2]).any() and (i_g < N).all() and (i_g >= 0).all(), N
        assert np.array_equal(i_g, i_o) and _same_bits(s_g, s_o), N


# ---- 3.2 scan matrix ------------------------------------------------------------------------------------------------------------------
def _random_bits(shape, seed):
    """random bf16 values of both signs with magnitudes in [2^-7, 2): cheap to make for the largest bank, 98 305 rows
    of D = 1536 at 256 CUs (13 rows per wave need 7 168 waves there: 288 MiB)"""
    r = rc._rng(seed).integers(0, 2 ** 16, size=shape, dtype=np.uint16)
    return ((r & 0x807F) | ((120 + ((r >> 7) & 7)) << 7)).astype(np.uint16)


def _check_scan(bank, q, k=100, off=0):
    """scores and indices are the oracle's bits.  Second opinion on the scores, an fp64 dot product of the same bf16 inputs:
        |s - dot64| <= 2^-8 |dot64| + D 2^-23 sum_i |a_i b_i|
    The products of two bf16 values are exact in fp32.  The canonical sum adds them in a tree of depth < D, every addition rounding by at
    most 2^-24 relative to a partial sum that is itself at most sum_i |a_i b_i| (1 + 2^-24)^D: the fp32 sum is within D 2^-24 (1 + ..) <=
    D 2^-23 sum |a_i b_i| of the exact one; that is the second term, granted at twice what the additions can use.  Rounding the fp32 sum s32
    to bf16 (8 significant bits, to nearest) moves it by at most half a bf16 ulp, 2^-8 of the power of two below |s32|, hence by at most
    2^-8 |s32| <= 2^-8 (|dot64| + D 2^-24 sum |a_i b_i|): the first term, its excess inside the unused half of the second."""
    fo = _fo()
    N, D = bank.shape
    k = min(k, N)
    s_g, i_g = _bank_topk_poisoned(_dev_bits(bank), _dev_bits(q), k, off)
    s_o, i_o = fo.bank_topk(bank, q, k, idx_offset=off)
    assert np.array_equal(i_g, i_o), (N, D, len(q))
    assert _same_bits(s_g, s_o), (N, D, len(q))
    for qi in range(len(q)):
        a = rc.bits_f32(bank[i_g[qi] - off]).astype(np.float64)
        b = rc.bits_f32(q[qi]).astype(np.float64)
        dot, mag = a @ b, np.abs(a) @ np.abs(b)
        assert (np.abs(s_g[qi].astype(np.float64) - dot) <= 2.0 ** -8 * np.abs(dot) + D * 2.0 ** -23 * mag).all(), (N, D, qi)
    return s_g, i_g


@pytest.mark.parametrize("D", rc.SCAN_D)
def test_scan_forms(D):
    N = 1003                                              # one row per wave, N % 4 != 0: the last workgroup has an idle wave
    bank = _random_bits((N, D), 100 + D)
    for Q in rc.SCAN_Q:
        _check_scan(bank, _random_bits((Q, D), 200 + D + Q), off=12345 if Q % 2 else 0)


@pytest.mark.parametrize("rows", rc.SCAN_ROWS, ids=[f"rows{r}" for r in rc.SCAN_ROWS])
def test_scan_rows_per_wave(ncu, rows):
    N = rc.scan_n_for(rows, ncu)
    base, rem, _ = rc.scan_rows_per_wave(N, ncu)
    assert base == rows and (rem != 0 or rows == 0)
    for D in ((8, 64) if rows >= 12 else (8,)):
        _check_scan(_random_bits((N, D), 300 + rows + D), _random_bits((5, D), 400 + rows + D))


@pytest.mark.parametrize("rows", rc.SCAN_ROWS_D1536, ids=[f"rows{r}" for r in rc.SCAN_ROWS_D1536])
def test_scan_rows_per_wave_d1536(ncu, rows):
    N = rc.scan_n_for(rows, ncu)
    assert rc.scan_rows_per_wave(N, ncu)[0] == rows
    _check_scan(_random_bits((N, 1536), 500 + rows), _random_bits((1, 1536), 600 + rows))


def test_scan_q9_equals_nine_q1(ncu):
    from freepose_amd import ops
    bank = _dev_bits(_random_bits((rc.scan_n_for(5, ncu), 520), 700))
    q = _dev_bits(_random_bits((9, 520), 701))
    s9, i9 = ops.bank_topk(bank, q, 100)
    for j in range(9):
        s1, i1 = ops.bank_topk(bank, q[j:j + 1], 100)
        assert torch.equal(i1[0], i9[j]) and torch.equal(s1[0].view(torch.int32), s9[j].view(torch.int32)), j


# ---- 3.3 topk_merge -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", rc.MERGE_C, ids=[f"C{c}" for c in rc.MERGE_C])
def test_topk_merge(Cn):
    fo = _fo()
    cs, ci = rc.merge_case(Cn)
    cs_d, ci_d = torch.from_numpy(cs).cuda(), torch.from_numpy(ci).cuda()
    for k in sorted({1, Cn, min(Cn, 1024)}):
        s_g, i_g = _merge_poisoned(cs_d, ci_d, k)
        s_o, i_o = fo.topk_merge(cs, ci, k)
        assert np.array_equal(i_g, i_o) and _same_bits(s_g, s_o), (Cn, k)
        for q in range(rc.MERGE_Q):
            s_r, i_r = rc.merge_ref(cs[q], ci[q], k)
            assert np.array_equal(i_g[q], i_r) and _same_bits(s_g[q], s_r), (Cn, k, q)


# ---- 3.4 template scorers -------------------------------------------------------------------------------------------------------------
def _check_scorers(T, P, D, seed):
    """oracle bits from the on-the-fly scorer, and the same bits from the streaming scorer on l2_normalize()d rows, on all T"""
    from freepose_amd import ops
    fo = _fo()
    tm = rc.bf16_rne((rc._rng(seed).standard_normal((T, P, D)) * 3).astype(np.float32))
    q = fo.l2norm_rows(rc.random_bf16((P, D), seed + 1))
    tm_d, q_d = _dev_bits(tm), _dev_bits(q)
    s_o = fo.template_score(tm, q)
    s_g = ops.template_score(tm_d, q_d).cpu().numpy()
    assert _same_bits(s_g, s_o), (T, P, D)
    tn = ops.l2_normalize(tm_d.clone(), inplace=True)
    s_n = ops.template_score(tn, q_d, normalized=True).cpu().numpy()
    assert _same_bits(s_n, s_o), (T, P, D)


@pytest.mark.parametrize("D", rc.TEMPLATE_D)
@pytest.mark.parametrize("case", rc.NORMED_CASES, ids=[c[0] for c in rc.NORMED_CASES])
def test_template_scorers_normed(case, D):
    cid, T, P, owns = case
    assert rc.normed_ts(T, P)[1] == owns
    _check_scorers(T, P, D, 800 + T + D)


@pytest.mark.parametrize("D", rc.TEMPLATE_D)
@pytest.mark.parametrize("case", rc.RAW_CASES, ids=[c[0] for c in rc.RAW_CASES])
def test_template_scorers_raw(case, D):
    _check_scorers(case[1], case[2], D, 900 + D)


@pytest.mark.parametrize("P", rc.MEAN_P, ids=[f"P{p}" for p in rc.MEAN_P])
def test_template_mean(P):
    from freepose_amd import ops
    fo = _fo()
    T, D = 5, 8
    rng = rc._rng(1000 + P)
    tm = rc.random_bf16((T, P, D), 1001 + P, scale=3.0)
    q = fo.l2norm_rows(rc.random_bf16((P, D), 1002 + P))
    w = rng.random((T, P)).astype(np.float32)
    w[rng.random((T, P)) < 0.3] = 0
    w[:, 0] = 0.5                                          # (no row all zero by chance)
    w[3] = 0                                               # one template whose weights are all zero: 0 / 0
    want = fo.template_score(tm, q, w)
    assert np.isnan(want[3]) and not np.isnan(np.delete(want, 3)).any()
    tm_d, q_d, w_d = _dev_bits(tm), _dev_bits(q), torch.from_numpy(w).cuda()
    tn = ops.l2_normalize(tm_d.clone(), inplace=True)
    for got in (ops.template_score(tm_d, q_d, w_d).cpu().numpy(), ops.template_score(tn, q_d, w_d, normalized=True).cpu().numpy()):
        assert np.isnan(got[3]) and _same_bits(np.delete(got, 3), np.delete(want, 3)), P
    assert _same_bits(ops.template_score(tm_d, q_d).cpu().numpy(), fo.template_score(tm, q))


# ---- 3.5 div_rbf ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def div_rows():
    rows = np.concatenate([rc.div_sweep(), rc.div_small_group()])
    want, q, _ = rc.div_ref(rows)
    assert rc.div_fallback_lanes(q).sum() >= 1000
    return rows, rc.bits_f32(rc.div_observed(want))


def _onehot():
    q = np.zeros((1, 8), np.uint16)
    q[0, 0] = 0x3F80
    return q


def test_div_rbf_in_template_score(div_rows):
    """P = 1, D = 8, query e0: the score of row (x, y, 0, ...) is bf16(x / n) itself, n the row's bf16 norm"""
    from freepose_amd import ops
    rows, want = div_rows
    got = ops.template_score(_dev_bits(rows.reshape(-1, 1, 8)), _dev_bits(_onehot())).cpu().numpy()
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} rows differ from bf16_rne(x / n); first {bad[:5]}: rows {rows[bad[:5], :2]}, got {got[bad[:5]]}, want {want[bad[:5]]}"
    assert _same_bits(got, _fo().template_score(rows.reshape(-1, 1, 8), _onehot()))


def test_div_rbf_in_rerank_views(div_rows):
    """the same rows as one view per mesh, k = 1: the re-rank score is the same bf16(x / n)"""
    from freepose_amd import ops
    rows, want = div_rows
    off = np.arange(len(rows) + 1, dtype=np.int32)
    cand = np.arange(len(rows), dtype=np.int32)[None]
    got = ops.rerank_views(_dev_bits(rows), torch.from_numpy(off), torch.from_numpy(cand), _dev_bits(_onehot()), 1).cpu().numpy()[0]
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} rows differ from bf16_rne(x / n); first {bad[:5]}: rows {rows[bad[:5], :2]}, got {got[bad[:5]]}, want {want[bad[:5]]}"
    assert _same_bits(got, _fo().rerank_views(rows, off, cand, _onehot(), 1)[0])


# ---- 3.6 rerank_views -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", rc.RERANK_D, ids=[f"D{d}" for d in rc.RERANK_D])
def test_rerank_views(D):
    """meshes with 0 .. 1030 views; of the 1030 only the first 1024 may count (the best views are planted after row 1024)"""
    from freepose_amd import ops
    fo = _fo()
    views, off, cand, q = rc.rerank_case(D)
    v_d, off_d, cand_d, q_d = _dev_bits(views), torch.from_numpy(off), torch.from_numpy(cand), _dev_bits(q)
    for k in rc.RERANK_K:
        got = ops.rerank_views(v_d, off_d, cand_d, q_d, k).cpu().numpy()
        assert _same_bits(got, fo.rerank_views(views, off, cand, q, k)), (D, k)
        assert _same_bits(got[0, 3:4], got[0, -1:]) and _same_bits(got[1, 0:1], got[1, -4:-3]), "one mesh named twice scores the same twice"
        if D == 8:
            assert _same_bits(got, rc.rerank_ref8(views, off, cand, q, k, maxv=rc.RR_MAXV)), (D, k)


# ---- 3.7 l2_normalize -----------------------------------------------------------------------------------------------------------------
def _misaligned(x_d):
    """the same rows in storage that starts 2 bytes off 16-byte alignment: fp_l2norm_rows takes the scalar kernel"""
    flat = torch.empty(x_d.numel() + 8, dtype=torch.bfloat16, device="cuda")
    v = flat[1:1 + x_d.numel()].view(x_d.shape)
    v.copy_(x_d)
    assert v.data_ptr() % 16 == 2 and v.is_contiguous()
    return v


@pytest.mark.parametrize("D", (8, 520, 1536))
@pytest.mark.parametrize("rows", (1, 5))
def test_l2_normalize_vector_and_scalar_kernels(rows, D):
    from freepose_amd import ops
    fo = _fo()
    x = rc.random_bf16((rows, D), 1100 + rows + D, scale=2.0)
    x[-1, ::3] = 0
    want = fo.l2norm_rows(x)
    x_d = _dev_bits(x)
    assert x_d.data_ptr() % 16 == 0
    out = ops.l2_normalize(x_d)
    assert np.array_equal(fo.torch_to_bits(out), want) and np.array_equal(fo.torch_to_bits(x_d), x), "out of place"
    inp = x_d.clone()
    assert ops.l2_normalize(inp, inplace=True).data_ptr() == inp.data_ptr() and np.array_equal(fo.torch_to_bits(inp), want), "in place"
    sc = ops.l2_normalize(_misaligned(x_d))
    assert np.array_equal(fo.torch_to_bits(sc), want), "the scalar kernel gives the vector kernel's bits"


def test_l2_normalize_scalar_fallback_wide_rows_and_zero_row():
    from freepose_amd import ops
    fo = _fo()
    x = rc.random_bf16((5, 2048), 1200, scale=2.0)         # D > 1536: no vector instantiation
    x[2] = 0                                               # an all-zero row: the 1e-12 clamp, 0 / 1e-12 = 0
    want = fo.l2norm_rows(x)
    assert not want[2].any()
    assert np.array_equal(fo.torch_to_bits(ops.l2_normalize(_dev_bits(x))), want)
    assert np.array_equal(fo.torch_to_bits(ops.l2_normalize(_misaligned(_dev_bits(x)))), want)
    z = np.zeros((3, 520), np.uint16)
    z[1] = rc.random_bf16(520, 1201)
    assert np.array_equal(fo.torch_to_bits(ops.l2_normalize(_dev_bits(z))), fo.l2norm_rows(z))
