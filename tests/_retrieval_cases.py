"""Planted inputs, independent references and a mirror of the dispatch predicates of csrc/retrieval.hip, for
tests/test_retrieval_cases_cpu.py (no GPU) and for GPU tests that walk those branches.  Pure numpy: no torch, no GPU.

Planted scores: with D = 8, bank row r = (v_r, 0, ..., 0) and query (c, 0, ..., 0) the canonical dot product is exactly bf16(v_r * c), so any
distribution of 16-bit keys can be put in front of the select kernels through ops.bank_topk.  Two values stay out of planted data: NaN (the
oracle's qsort comparator is no total order once NaN is mixed with numbers; only the all-NaN query of test_gpu_retrieval.py is well defined)
and -0.0 (the fmaf chain starts from +0, so a score of -0.0 cannot arise).

The mirror (select_path, scan_rows_per_wave, normed_ts) restates launch conditions only; it is how a case knows which branch it reaches."""
import functools

import numpy as np

# ---- constants of freepose_amd/csrc/retrieval.hip (line numbers as of this file's writing) ------------------------------------------------------------------------------------------------
RU = 4                            # retrieval.hip:38   rows per chunk of bank_scan_kernel
SEL_T = 1024                      # retrieval.hip:111  threads of a select workgroup
KMAX = 1024                       # retrieval.hip:112  largest k, and the capacity of the candidate buffer
SEL_W = 24                        # retrieval.hip:268  packed words per thread: a thread owns 2 * SEL_W = 48 consecutive keys
SEL_CAP = SEL_T * 2 * SEL_W       # retrieval.hip:269  49 152 keys: the register kernel's largest row
RR_MAXV = 1024                    # retrieval.hip:553  views per mesh the re-rank looks at
HIST_LDS_MAX = 65536              # retrieval.hip:670  key_bytes <= 128 KB  <=>  padded row <= 65 536 keys
PER = 2 * SEL_W

Q_E0, Q_NEG, Q_TWO = 0x3F80, 0xBF80, 0x4000     # bf16 bits of the three planted queries' first element: 1, -1, 2


# ---- bf16 / key helpers -------------------------------------------------------------------------------------------------------------
def bf16_rne(x) -> np.ndarray:
    """float32 -> bf16 bits, round to nearest even (no NaN handling: callers keep NaN out)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bits_f32(b) -> np.ndarray:
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def key16(bits) -> np.ndarray:
    """retrieval.hip score_key16: bf16 bits -> 16-bit key whose unsigned order is the score's order"""
    b = np.asarray(bits, dtype=np.uint16).astype(np.uint32)
    return np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000).astype(np.uint16)


def key_to_bits(keys) -> np.ndarray:
    k = np.asarray(keys).astype(np.uint32)
    return np.where(k & 0x8000, k & 0x7FFF, ~k & 0xFFFF).astype(np.uint16)


K_NINF, K_PINF, K_NEG0, K_ZERO = 0x007F, 0xFF80, 0x7FFF, 0x8000      # keys of -inf, +inf, -0.0 (never planted), +0.0


def planted_bank(score_bits) -> np.ndarray:
    b = np.zeros((len(score_bits), 8), dtype=np.uint16)
    b[:, 0] = score_bits
    return b


def planted_queries() -> np.ndarray:
    q = np.zeros((3, 8), dtype=np.uint16)
    q[:, 0] = (Q_E0, Q_NEG, Q_TWO)
    return q


def planted_scores(score_bits, qbits: int) -> np.ndarray:
    """bf16 bits of the score of every row under the query (c, 0, ...): fmaf(v, c, +0) and seven fmaf(0, 0, acc), then + 0"""
    with np.errstate(over="ignore"):
        s = bits_f32(score_bits) * bits_f32(np.array([qbits], np.uint16))[0] + np.float32(0.0)
    return bf16_rne(s)


# ---- independent references ---------------------------------------------------------------------------------------------------------
def topk_ref(score_bits, k: int, idx_offset: int = 0):
    """(scores f32 [k], idx i32 [k]) by score descending, index ascending"""
    s = bits_f32(score_bits)
    idx = np.arange(len(s), dtype=np.int64)
    order = np.lexsort((idx, -s.astype(np.float64)))[:k]
    return s[order].copy(), (idx[order] + idx_offset).astype(np.int32)


def merge_ref(cs, ci, k: int):
    cs = np.asarray(cs, dtype=np.float32)
    ci = np.asarray(ci, dtype=np.int32)
    order = np.lexsort((ci.astype(np.int64), -cs.astype(np.float64)))[:k]
    return cs[order].copy(), ci[order].copy()


# ---- mirror of the dispatch predicates ----------------------------------------------------------------------------------------------
def scan_rows_per_wave(N: int, ncu: int):
    """fp_bank_scan's grid choice (retrieval.hip:615-624): (base_rows, rem, nwave); the first `rem` waves own base_rows + 1 rows"""
    blocks, best = ncu * 2, 1e30
    for bpc in range(2, 9):
        nw = ncu * bpc * 4
        waste = float((N + nw - 1) // nw * nw) / N
        if waste <= best:
            best, blocks = waste, ncu * bpc
    blocks = min(blocks, (N + 3) // 4)
    nwave = blocks * 4
    return N // nwave, N % nwave, nwave


def scan_inloop_fetches(rows: int) -> int:
    """how often a wave that owns `rows` rows executes the in-loop fetch(bufB, r0 + RU) (retrieval.hip:99)"""
    return sum(1 for r0 in range(2 * RU, rows, 2 * RU) if r0 + RU < rows)


@functools.lru_cache(maxsize=None)
def scan_n_for(base_rows: int, ncu: int) -> int:
    """the smallest N found for which every wave owns base_rows or base_rows + 1 rows, both run lengths occurring (rem != 0)"""
    if base_rows == 0:
        return 3
    best = None
    for bpc in range(2, 9):
        nw = ncu * bpc * 4
        for r in range(1, nw):
            N = base_rows * nw + r
            if best is not None and N >= best:
                break
            b, rem, _ = scan_rows_per_wave(N, ncu)
            if b == base_rows and rem != 0:
                best = N
                break
    assert best is not None, (base_rows, ncu)
    return best


def scan_form(D: int):
    """(NCH, FULL) of the bank_scan_kernel instantiation fp_bank_scan launches for D (retrieval.hip:612, 629)"""
    nch = (D + 511) // 512
    return nch, D == nch * 512


def scan_passes(Q: int):
    """queries per pass (retrieval.hip:636-645): 4 while at least 4 are left, then one at a time"""
    out = []
    while Q >= 4:
        out.append(4)
        Q -= 4
    return out + [1] * Q


def select_path(keys, k: int) -> dict:
    """Which select kernel and branch fp_topk_select takes for one query's key row (product library), computed the way the kernels do.
    path: 'reg-fast' | 'reg-count-rank' | 'reg-count-bitonic' | 'hist-lds' | 'hist-global'."""
    keys = np.asarray(keys, dtype=np.uint16).astype(np.int64)
    N = len(keys)
    assert 0 < k <= KMAX and k <= N
    ldk = (N + 7) & ~7
    if N > SEL_CAP:                                    # retrieval.hip:663
        hist = np.bincount(keys >> 8, minlength=256)
        c, b = 0, 255
        while b >= 0 and c + hist[b] < k:              # retrieval.hip:226
            c += hist[b]
            b -= 1
        hi_exact = c + hist[b] == k
        hb = b
        hist = np.bincount(keys[(keys >> 8) == hb] & 255, minlength=256)
        b = 255
        while b >= 0 and c + hist[b] < k:              # retrieval.hip:239
            c += hist[b]
            b -= 1
        lo_exact = c + hist[b] == k
        T = (hb << 8) | b
        return dict(path="hist-lds" if ldk <= HIST_LDS_MAX else "hist-global", T=T, ngt=int(c), neq=int((keys == T).sum()),
                    hi_exact=bool(hi_exact), lo_exact=bool(lo_exact), hi_bins=int((np.bincount(keys >> 8, minlength=256) > 0).sum()))
    row = np.zeros(SEL_CAP, dtype=np.int64)            # staged row: zero beyond N (retrieval.hip:292)
    row[:N] = keys
    maxima = row.reshape(SEL_T, PER).max(axis=1)       # retrieval.hip:312-315
    G = int(maxima.max())
    L = 0
    for bit in range(15, -1, -1):                      # retrieval.hip:336-340
        c = L | (1 << bit)
        if c > G:
            continue
        if int((maxima >= c).sum()) >= k:
            L = c
    M = int((row >= max(L, 1)).sum())                  # retrieval.hip:346-354
    out = dict(L=L, G=G, M=M, T=None, ngt=None, iters=0)
    if M <= KMAX:
        out.update(path="reg-fast")
        return out
    tlo, thi, it = L, G, 0
    while tlo < thi:                                   # retrieval.hip:381-384
        mid = (tlo + thi + 1) >> 1
        if int((row >= mid).sum()) >= k:
            tlo = mid
        else:
            thi = mid - 1
        it += 1
    T = tlo
    ngt = 0 if T >= 65535 else int((row >= T + 1).sum())
    neq = int((row[:N] == T).sum())
    need_eq = k - ngt
    cut = int(np.flatnonzero(row[:N] == T)[need_eq - 1]) + 1        # index just past the last tied key that is kept
    out.update(path="reg-count-rank" if k <= 256 else "reg-count-bitonic", T=T, ngt=ngt, iters=it, neq=neq, need_eq=need_eq,
               # the cut falls strictly inside one thread's keys: that thread keeps a tied key and drops a later one
               cut_inside=bool(need_eq < neq and cut % PER != 0 and row[cut - 1] == T and (row[cut:cut - cut % PER + PER] == T).any()))
    return out


def normed_ts(T: int, P: int):
    """fp_template_score_launch, normalised store (retrieval.hip:700): (TS, sorted set of how many templates a wave owns, number of waves
    launched with pidx >= P)"""
    TS = max(1, min(T, (256 * 16 + P - 1) // P))
    owns = sorted({len(range(t0, T, TS)) for t0 in range(TS)})
    nblk = (P * TS + 3) // 4
    return TS, owns, nblk * 4 - P * TS


# ---- planted key distributions ------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _finite_keys(rng, n, lo=K_NINF + 1, hi=K_PINF - 1):
    """n random keys of finite scores in [lo, hi], never -0.0"""
    k = rng.integers(lo, hi + 1, size=n)
    k[k == K_NEG0] = K_ZERO
    return k


def spread(N, seed):
    """finite values of both signs over every exponent, a few +-inf, zeros"""
    rng = _rng(seed)
    k = _finite_keys(rng, N)
    if N >= 16:
        pos = rng.choice(N, size=min(N // 4, 12), replace=False)
        k[pos[0::3]] = K_PINF
        k[pos[1::3]] = K_NINF
        k[pos[2::3]] = K_ZERO
    return key_to_bits(k)


def one_high_byte(N, seed, hb=0xBF):
    """every key shares its high byte (scores in [0.5, 1)): the histogram kernels' skew case, 256 distinct values -> ties everywhere"""
    return key_to_bits((hb << 8) | _rng(seed).integers(0, 256, size=N))


def negatives(N, seed):
    rng = _rng(seed)
    k = _finite_keys(rng, N, hi=K_NEG0 - 1)
    k[rng.choice(N, size=max(1, N // 50), replace=False)] = K_NINF
    return key_to_bits(k)


def denormals(N, seed):
    """bf16 denormals of both signs (exponent field 0) among normals"""
    rng = _rng(seed)
    k = _finite_keys(rng, N)
    den = rng.random(N) < 0.5
    mant = rng.integers(1, 128, size=N)
    k[den] = np.where(rng.random(N) < 0.5, 0x8000 | mant, 0x7FFF - mant)[den]      # +denormal keys 0x8001.., -denormal keys ..0x7ffe
    return key_to_bits(k)


def plateau(N, length, at, above, seed, tie_key=0xC000, above_at=None):
    """`length` consecutive rows tie at tie_key from row `at`; `above` rows carry distinct higher keys, one per thread, in threads away from the
    plateau; everything else is lower"""
    rng = _rng(seed)
    k = _finite_keys(rng, N, hi=tie_key - 0x100)
    k[at:at + length] = tie_key
    free = np.setdiff1d(np.arange((N + PER - 1) // PER), np.arange(at // PER, (at + length - 1) // PER + 1))
    thr = free[:: max(1, len(free) // max(above, 1))][:above] if above_at is None else np.asarray(above_at)
    assert len(thr) == above
    rows = np.minimum(thr * PER + 5, N - 1)
    k[rows] = tie_key + 1 + 3 * np.arange(above)
    return key_to_bits(k)


def fast_edge(M, k=100, seed=7, N=SEL_CAP, lval=0xB000):
    """exactly M keys >= L: k threads hold them all, one of those threads has nothing above lval, so L = lval.  M = KMAX stays on the fast path,
    M = KMAX + 1 falls to the counting search by a single key."""
    rng = _rng(seed)
    key = _finite_keys(rng, N, hi=lval - 1)
    thr = np.sort(rng.choice(SEL_T, size=k, replace=False))
    per = np.full(k, M // k)
    per[: M - per.sum()] += 1
    for j, (t, n) in enumerate(zip(thr, per)):
        pos = t * PER + rng.choice(PER, size=n, replace=False)
        key[pos] = lval if j == 0 else lval + rng.integers(0, 400, size=n)
    return key_to_bits(key)


def exact_bins(N, seed, tie_len=None):
    """for the histogram kernels: `c + hist[b] == k` holds exactly (the `>=` of both scans decides, with a plateau of tied keys ending right
    at k) at the high-byte step for k = 100 and, inside one crowded high-byte bin, at the low-byte step for k = 1024; k = 1 is exact at both.
       1 key in bin 0xC3; 99 keys in bin 0xC2, the last 60 of them tied      -> through bin 0xC2 the count is exactly 100
       bin 0xC1: 924 keys >= 0xC180 with the last 500 tied at 0xC180        -> count exactly 1024 at low byte 0x80, and more keys below"""
    rng = _rng(seed)
    k = _finite_keys(rng, N, hi=0xC0FF)
    pos = rng.permutation(N)
    k[pos[0]] = 0xC310
    k[pos[1:40]] = 0xC201 + rng.integers(0, 255, size=39)
    k[pos[40:100]] = 0xC200
    k[pos[100:524]] = 0xC181 + rng.integers(0, 127, size=424)
    k[pos[524:1024]] = 0xC180
    k[pos[1024:3000]] = 0xC100 + rng.integers(0, 128, size=1976)
    return key_to_bits(k)


# ---- the select matrix: banks, then (case id, bank id, k, idx_offset, claimed path) ---------------------------------------------------
# bank id -> builder of the N score bits (query e0 sees exactly these scores)
SELECT_BANKS = {
    "n1": lambda: spread(1, 1), "n7": lambda: spread(7, 2), "n8": lambda: spread(8, 3), "n9": lambda: spread(9, 4),
    "n47": lambda: spread(47, 5), "n48": lambda: spread(48, 6), "n49": lambda: spread(49, 7), "n100": lambda: spread(100, 8),
    "n1024": lambda: spread(1024, 9), "n49151": lambda: spread(49151, 10), "spread5000": lambda: spread(5000, 11),
    "spread49152": lambda: spread(49152, 12),
    "neg5000": lambda: negatives(5000, 13), "den5000": lambda: denormals(5000, 14), "ohb49152": lambda: one_high_byte(49152, 15),
    "m1024": lambda: fast_edge(KMAX), "m1025": lambda: fast_edge(KMAX + 1),
    # 2 000 tied rows inside 42 threads (rows 20 013 .. 22 012), 40 rows above, each in a thread of its own: 82 threads reach the tie key,
    # fewer than the smallest k, so L comes from the background and the search has to move up to T.  The cut for k = 100 / 257 / 500 / 1024 is
    # at row 20 073 / 20 230 / 20 473 / 20 997, none of them a multiple of 48
    "plat2000": lambda: plateau(49151, 2000, 20013, 40, 16),
    # the same plateau ending with the row: the last thread owns 49 130 % 48 = 26 ragged keys, all tied
    "plat_ragged": lambda: plateau(49130, 2000, 49130 - 2000, 40, 17),
    # 40 000 tied rows at N = 49 152: the packed 16+16-bit scan carries an upper count >= 2^15 beside a non-zero lower count
    "plat40000": lambda: plateau(49152, 40000, 5003, 60, 18),
}
for _n in (49153, 60001, 65536, 65537, 106501):
    SELECT_BANKS[f"spread{_n}"] = (lambda n=_n: spread(n, 100 + n % 97))
    SELECT_BANKS[f"ohb{_n}"] = (lambda n=_n: one_high_byte(n, 200 + n % 97))
    SELECT_BANKS[f"exact{_n}"] = (lambda n=_n: exact_bins(n, 300 + n % 97))
SELECT_BANKS["plat70000"] = lambda: plateau(106501, 70000, 30001, 50, 19)          # a plateau longer than 65 535

def OFF_MAX(N):
    """the largest idx_offset whose indices still fit an int32"""
    return 2 ** 31 - 1 - N


# `spread` at k = 1024 is listed with the fast path in the plan of these cases, but cannot take it: at N = 5 000 only 105 threads hold keys, so
# L = 0 and M = N; at N = 49 152 L is the smallest thread maximum and M is several thousand.  Both are claimed for what they reach, the counting
# search with the bitonic sort; the fast path at k = 1024 is run by n1024_k1024 (M == k == KMAX) and m1024.

_S = []
for _b, _k, _p in (("n1", 1, "reg-fast"), ("n7", 7, "reg-fast"), ("n8", 3, "reg-fast"), ("n9", 9, "reg-fast"), ("n47", 47, "reg-fast"),
                   ("n48", 48, "reg-fast"), ("n49", 49, "reg-fast"), ("n100", 100, "reg-fast"), ("n1024", 1024, "reg-fast"),
                   ("n49151", 100, "reg-fast"), ("n49151", 1024, "reg-count-bitonic"),
                   ("spread5000", 1, "reg-fast"), ("spread5000", 100, "reg-fast"), ("spread5000", 1024, "reg-count-bitonic"),
                   ("spread49152", 1, "reg-fast"), ("spread49152", 100, "reg-fast"), ("spread49152", 1024, "reg-count-bitonic"),
                   ("neg5000", 100, "reg-fast"), ("den5000", 100, "reg-fast"), ("den5000", 1024, "reg-count-bitonic"),
                   ("ohb49152", 100, "reg-fast"), ("ohb49152", 1024, "reg-count-bitonic"),
                   ("m1024", 100, "reg-fast"), ("m1025", 100, "reg-count-rank"),
                   ("plat2000", 100, "reg-count-rank"), ("plat2000", 257, "reg-count-bitonic"), ("plat2000", 500, "reg-count-bitonic"),
                   ("plat2000", 1024, "reg-count-bitonic"), ("plat_ragged", 100, "reg-count-rank"), ("plat_ragged", 1024, "reg-count-bitonic"),
                   ("plat40000", 100, "reg-count-rank"), ("plat40000", 1024, "reg-count-bitonic")):
    _S.append((f"{_b}_k{_k}", _b, _k, 12345 if len(_S) % 2 else 0, _p))
for _n in (49153, 60001, 65536, 65537, 106501):
    _p = "hist-lds" if _n <= HIST_LDS_MAX else "hist-global"
    for _d in ("spread", "ohb", "exact") + (("plat",) if _n == 106501 else ()):
        _b = "plat70000" if _d == "plat" else f"{_d}{_n}"
        for _k in (1, 100, 1024):
            _S.append((f"{_b}_k{_k}", _b, _k, 12345 if len(_S) % 2 else 0, _p))
_S.append(("n49151_k100_offmax", "n49151", 100, OFF_MAX(49151), "reg-fast"))
_S.append(("spread106501_k1024_offmax", "spread106501", 1024, OFF_MAX(106501), "hist-global"))
SELECT_CASES = _S
PLATEAU_SEARCH_CASES = [c[0] for c in _S if c[1] in ("plat2000", "plat_ragged")]     # 0 < L < T < G, >= 3 iterations, cut inside a thread

STALE_PAD_N = (9, 4999, 49151, 60001)

# ---- scan matrix ----------------------------------------------------------------------------------------------------------------------
SCAN_D = (8, 384, 512, 520, 1024, 1032, 1536)
SCAN_Q = (1, 3, 4, 5, 8, 9)
SCAN_ROWS = (0, 1, 4, 5, 8, 9, 12, 13, 21)        # base_rows classes; 13 and 21 run the in-loop fetch(bufB) once and twice
SCAN_ROWS_D1536 = (5, 13)


def random_bf16(shape, seed, scale=1.0):
    return bf16_rne((_rng(seed).standard_normal(shape) * scale).astype(np.float32))


# ---- template scorers -----------------------------------------------------------------------------------------------------------------
#              id            T    P     owns (templates per wave, normed kernel)
NORMED_CASES = [(f"ts1_T{T}", T, 4100, [T]) for T in range(1, 9)] + [
    ("ts_eq_T", 5, 3, [1]), ("ts586", 600, 7, [1, 2]), ("tail_waves", 19, 1023, [3, 4])]
TEMPLATE_D = (8, 520, 1536)
RAW_CASES = [("stride_odd", 3, 5462), ("stride_T7", 7, 2341)]          # T * P = 16 386 and 16 387 rows: > 16 384 waves' worth, T*P % 4 != 0
MEAN_P = (1, 63, 64, 65)


# ---- div_rbf sweep --------------------------------------------------------------------------------------------------------------------
def div_sweep():
    """rows (x, y, 0, ...) [R, 8] bf16 bits.  Main sweep: x over all 128 mantissas at exponents -20, -1, 0, 7 and both signs, y so that the
    row norm's bf16 value takes every mantissa.  Its quotients are ratios of two 8-bit mantissas, which never come within 2^-17 (relative) of a
    bf16 midpoint, so none of them takes div_rbf's exact-division fallback; the second block does: tiny x (exponent fields 0 .. 10: denormals and
    the smallest normals) beside y = m * 2^3 or m * 2^10, so that n = y exactly and x / n is an fp32 DENORMAL, whose bf16 rounding has fewer significant bits and
    meets exact ties."""
    m = np.arange(128, dtype=np.uint16)
    rows = []
    for e in (-20, -1, 0, 7):
        for sign in (0, 0x8000):
            x = (sign | ((e + 127) << 7) | m).astype(np.uint16)
            xf = bits_f32(x).astype(np.float64)
            target = (1 + m.astype(np.float64) / 128) * 2.0 ** (e + 2)                 # > |x|
            y = bf16_rne(np.sqrt(target[None, :] ** 2 - xf[:, None] ** 2).astype(np.float32))
            blk = np.zeros((128, 128, 8), np.uint16)
            blk[:, :, 0] = x[:, None]
            blk[:, :, 1] = y
            rows.append(blk.reshape(-1, 8))
    for yexp, ebits_range in ((3, range(0, 4)), (10, range(3, 11))):                   # exponent field 0: bf16 denormals (mantissa 0 is +-0)
        y = ((yexp + 127) << 7 | m).astype(np.uint16)
        for ebits in ebits_range:
            for sign in (0, 0x8000):
                x = (sign | (ebits << 7) | m).astype(np.uint16)
                blk = np.zeros((128, 128, 8), np.uint16)
                blk[:, :, 0] = x[:, None]
                blk[:, :, 1] = y[None, :]
                rows.append(blk.reshape(-1, 8))
    return np.concatenate(rows)


DIV_MAIN_ROWS = 4 * 2 * 128 * 128


def div_small_group():
    """rows that mix magnitude 2^10 with bf16 denormals (the quotient is an fp32 denormal), and an all-zero row (the 1e-12 clamp)"""
    rows = np.zeros((12, 8), np.uint16)
    big = (10 + 127) << 7
    for i, d in enumerate((0x0001, 0x0003, 0x0040, 0x007F, 0x8001, 0x8055)):
        rows[i, 0], rows[i, 1:4] = d, (big, big | 0x20, 0x8000 | big)
        rows[6 + i, 0], rows[6 + i, 1], rows[6 + i, 5] = d, big | (i * 17), d
    rows[11] = 0
    return rows


def div_ref(rows):
    """bf16 bits of bf16_rne(float32(x) / float32(n)) for element 0 of every row, n = max(bf16(sqrt(sum x_i^2)), 1e-12), and the quotients.
    The squares of bf16 values are exact in fp32, so `acc + x*x` in fp32 is the kernel's fmaf(x, x, acc); lane 0 owns all eight elements."""
    f = bits_f32(rows)
    acc = np.zeros(len(rows), np.float32)
    for e in range(rows.shape[1]):
        acc = (acc + f[:, e] * f[:, e]).astype(np.float32)
    n = np.maximum(bits_f32(bf16_rne(np.sqrt(acc))), np.float32(1e-12))
    q = (f[:, 0] / n).astype(np.float32)
    return bf16_rne(q), q, n


def div_observed(bits) -> np.ndarray:
    """what the one-hot scorer shows of a normalised element: fmaf(tn, 1, +0) turns a quotient that rounded to -0.0 into +0.0"""
    return np.where(np.asarray(bits) == 0x8000, 0, bits).astype(np.uint16)


def div_fallback_lanes(q) -> np.ndarray:
    """quotients whose low 16 bits lie within 4 of 0x8000: where div_rbf must take the exact division (dot64.h:136)"""
    low = (np.ascontiguousarray(q, np.float32).view(np.uint32) & 0xFFFF).astype(np.int64)
    return np.abs(low - 0x8000) <= 4


# ---- rerank ---------------------------------------------------------------------------------------------------------------------------
RERANK_NV = (0, 1, 7, 8, 9, 127, 128, 129, 1024, 1030)
RERANK_K = (1, 7, 8, 9, 15, 16, 17, 128)
RERANK_D = (8, 384, 1536)


def rerank_case(D, seed=5):
    """(view bits [sum nv, D], offsets, cand [2, C], query bits [2, D]).  Mesh i has RERANK_NV[i] views.  In the 1030-view mesh the six rows
    past 1024 are copies of query 0 (cosine ~1, better than every counted view) and must not count; meshes 5 and 6 hold duplicated views
    (exactly tied scores); the candidate lists name mesh 3 twice."""
    rng = _rng(seed + D)
    q = bits_f32(random_bf16((2, D), seed + 1))
    q = bf16_rne(q / np.linalg.norm(q, axis=1, keepdims=True))          # unit queries (to bf16 precision): scores are cosines
    views, off = [], [0]
    for i, nv in enumerate(RERANK_NV):
        v = random_bf16((nv, D), seed + 10 + i, scale=3.0)
        if nv == 1030:
            v[1024:] = q[0]
        if nv in (127, 128):
            v[nv // 2:nv // 2 + 20] = v[:20]
        views.append(v)
        off.append(off[-1] + nv)
    nm = len(RERANK_NV)
    cand = np.stack([np.concatenate([np.arange(nm), [3]]), np.concatenate([[3], np.arange(nm)[::-1]])]).astype(np.int32)
    return np.concatenate(views), np.array(off, np.int32), cand, q


def rerank_ref8(view_bits, off, cand, q_bits, k, maxv=RR_MAXV):
    """the re-rank restated in numpy for D = 8, bit for bit (f32 [Q, C]): lane 0 owns all eight elements, so the canonical dot is one fp32
    chain, and the products of two bf16 values are exact in fp32, so `acc + a*b` IS fmaf(a, b, acc).  Only the first `maxv` views count."""
    assert view_bits.shape[1] == 8
    _, _, n = div_ref(view_bits) if len(view_bits) else (None, None, np.zeros(0, np.float32))
    v = bits_f32(view_bits)
    tn = bits_f32(bf16_rne((v / n[:, None]).astype(np.float32)))
    out = np.full(cand.shape, -3.0e38, np.float32)
    for qi in range(cand.shape[0]):
        qf = bits_f32(q_bits[qi])
        acc = np.zeros(len(v), np.float32)
        for e in range(8):
            acc = (acc + tn[:, e] * qf[e]).astype(np.float32)
        sc = bits_f32(bf16_rne(acc))
        for c, mesh in enumerate(cand[qi]):
            s = np.sort(sc[off[mesh]:off[mesh + 1]][:maxv])[::-1]
            kk = min(k, len(s))
            if kk:
                out[qi, c] = np.mean(np.ascontiguousarray(s[:kk]), dtype=np.float32)
    return out


# ---- topk_merge -----------------------------------------------------------------------------------------------------------------------
MERGE_C = (1, 2, 3, 1000, 4096, 4097, 8192)
MERGE_Q = 5


def merge_case(C, seed=3):
    """(scores f32 [5, C], idx i32 [5, C]): row 0 few distinct bf16 scores under distinct shuffled indices; row 1 negative scores; row 2 with
    +-inf; row 3 the -inf / 2^31-1 padding of a short shard in its second half; row 4 arbitrary f32 scores (not bf16 values) incl. denormals"""
    rng = _rng(seed + C)
    cs = np.empty((MERGE_Q, C), np.float32)
    ci = np.stack([rng.permutation(C) + 1000 * q for q in range(MERGE_Q)]).astype(np.int32)
    cs[0] = bits_f32(bf16_rne(rng.integers(0, 4, size=C).astype(np.float32) * 0.25))
    cs[1] = -np.abs(bits_f32(random_bf16(C, seed + 1))) - np.float32(0.5)
    cs[2] = bits_f32(random_bf16(C, seed + 2))
    cs[2, rng.integers(0, C, size=max(1, C // 10))] = np.inf
    cs[2, rng.integers(0, C, size=max(1, C // 10))] = -np.inf
    cs[3] = bits_f32(random_bf16(C, seed + 3))
    cs[3, (C + 1) // 2:] = -np.inf
    ci[3, (C + 1) // 2:] = 2 ** 31 - 1
    raw = rng.integers(0, 2 ** 32, size=C, dtype=np.uint64).astype(np.uint32)
    raw[(raw & 0x7F800000) == 0x7F800000] &= 0xBFFFFFFF                    # no NaN / inf patterns
    raw[raw == 0x80000000] = 0                                             # no -0.0: the oracle's comparator ties it with +0.0 by index, the kernel's key does not
    raw[: max(1, C // 8)] &= 0x807FFFFF                                    # fp32 denormals
    raw[raw == 0x80000000] = 0
    cs[4] = raw.view(np.float32)
    return cs, ci
