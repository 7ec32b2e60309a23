"""Cases, exact-arithmetic references and a Python mirror of the dispatch for the ViT GEMM family (csrc/gemm_bf16.hip, gemm_epilogue.h,
gemm_asm.hip, the LayerNorm-fold helpers of vit_misc.hip).  No GPU is needed to import or evaluate anything here: tests/test_gemm_cases_cpu.py
proves the branch claims, the exactness of the operands and the rounding helper; tests/test_gpu_gemm_branches.py runs the cases.

EXACT OPERANDS.  X = ix 2^-3, W = iw 2^-5, bias = 4 ib 2^-8 with small integers ix, iw, ib, so every product and every partial sum, in any
order, is an integer number of quanta 2^-8 below 2^24: the fp32 accumulator (bias included, wherever a kernel adds it) is known exactly and
does not depend on K order, tile tier or the init MFMA.  The amplitude of ix, iw shrinks with K (amplitude()) so that the sums come out at
9 .. 13 significant bits: most pre-rounding values are not representable in bf16 (8 bits) and, with only 1 .. 5 bits dropped, a good
share are exact round-to-even ties.  The operands are asymmetric (ix in [-a, a + 3], iw in [-a + 2, a]) and every element is a pure
function hash_ints(row, column, seed): a reference for any subset of rows needs no full matrix, and the same function runs on the
device (torch int64) to fill operands too large to build on the host.  gamma = ig 2^-6, resid = ir 2^-5 and pos = ip 2^-4 keep every
intermediate of the LayerScale + residual and position-embedding chains exact in fp32 (a product of two bf16 values has 16 bits; the
sums span at most 20), so only the documented bf16 rounding points matter and a float32 and a float64 evaluation agree bit for bit.
"""
import math
from dataclasses import dataclass

import numpy as np

BIAS, GELU, LS_RES, PATCH, VT, LN_BIAS, LN_GELU, LN_VT, LS_RES_STATS = range(9)      # FpGemmEpi (csrc/gemm_bf16.h)
EPI_NAMES = {BIAS: "bias", GELU: "gelu", LS_RES: "lsres", PATCH: "patch", VT: "vt", LN_BIAS: "ln_bias", LN_GELU: "ln_gelu", LN_VT: "ln_vt",
             LS_RES_STATS: "stats"}
BIG_MIN_TILES = 192
STREAM_BYTES = 128 << 20
LN_EPS = 1e-6


def cdiv(a, b):
    return -(-a // b)


# ---- dispatch mirror (csrc/gemm_plan.h make_plan under the product's options).  A restatement written by hand, held to the header itself by
# tests/test_gemm_cases_cpu.py (tools/gemm_plan_host_check.cpp on every case and a sweep of 10^5 shapes) and to the library on the device by
# tests/test_gpu_gemm_branches.py (fp_op_gemm_plan).  The part in FRONT of a split picks its tier by the same rule as any launch: nearly
# always the 256x256 / 128x128 tiles the split is named for, but e.g. 139 775 x 48 on 256 CUs — 546 big tiles, 2.13 rounds, not filled — takes
# split_mid, whose front of 131 072 rows is 512 big tiles = two full rounds and runs on the big tier.
def asm_preferred(K, epi, ldx, ldw):
    """fp_plan::asm_preferred: the hand-scheduled 256x256 kernel is instantiated for BIAS, GELU, LS_RES, LS_RES_STATS, takes K steps in pairs
    and 128-byte aligned rows, and is the faster one from K = 2048 on"""
    supported = epi in (BIAS, GELU, LS_RES, LS_RES_STATS) and K % 128 == 0 and K >= 256 and ldx % 64 == 0 and ldw % 64 == 0
    return supported and K >= 2048


def fuses_ln_part(M, N):
    return cdiv(M, 256) * cdiv(N, 256) < BIG_MIN_TILES


def _ncu(n_cu):
    return (n_cu & ~7) if n_cu > 8 else 256


def _is_big(M, N, ncu):
    tiles_big = cdiv(M, 256) * cdiv(N, 256)
    return tiles_big >= BIG_MIN_TILES and tiles_big * 4 >= cdiv(tiles_big, ncu) * ncu * 3      # >= 75 % of the big-tile rounds are real work


def _tier(M, N, K, epi, ncu, ldx, ldw):
    """the tier of M rows launched unsplit"""
    if _is_big(M, N, ncu):
        if epi not in (VT, LN_VT) and asm_preferred(K, epi, ldx, ldw):
            return "big_asm"
        return "big_hip_stream" if M * N * 2 > STREAM_BYTES else "big_hip"
    return "tiny64" if cdiv(M, 128) * cdiv(N, 128) < ncu else "small128"


def plan(M, N, K, epi, n_cu=256, ldx=None, ldw=None, row_split=True, ln_part=False):
    """(label, row0) of the path fp_gemm_bf16 takes.  label: tiny64 | small128 | big_hip | big_hip_stream | big_asm, split_big+<rest> /
    split_mid+<rest> (<rest> = the tier of the remaining rows; the whole rounds in front run on 256x256 / on 128x128 tiles),
    finalize_then_<path> when a launch that carries partial row statistics is finalised by the host-side kernel first.  row0: the rows in
    front of the split (0 = none)"""
    ldx = K if ldx is None else ldx
    ldw = K if ldw is None else ldw
    ncu = _ncu(n_cu)
    trans, ln = epi in (VT, LN_VT), epi in (LN_BIAS, LN_GELU, LN_VT)
    prefix = ""
    if ln and ln_part and (trans or not fuses_ln_part(M, N)):
        prefix, ln_part = "finalize_then_", False
    tiles_big = cdiv(M, 256) * cdiv(N, 256)
    big = _is_big(M, N, ncu)
    assert not (big and ln_part)
    if epi not in (VT, LN_VT, PATCH) and row_split:
        tiles_n = cdiv(N, 256)
        full = tiles_big // ncu
        rb = full * ncu // tiles_n
        if full >= 1 and rb * 256 < M and tiles_big >= BIG_MIN_TILES:
            def small_cost(rows):
                return float(cdiv(cdiv(rows, 128) * cdiv(N, 128), 2 * ncu)) * 0.56
            t_now = float(cdiv(tiles_big, ncu)) if big else small_cost(M)
            t_split = float(cdiv(rb * tiles_n, ncu)) + small_cost(M - rb * 256)
            if t_split < 0.96 * t_now:
                return prefix + "split_big+" + _tier(M - rb * 256, N, K, epi, ncu, ldx, ldw), rb * 256
        tn, slots = cdiv(N, 128), 2 * ncu
        tiles_mid_all = cdiv(M, 128) * tn
        fullm = tiles_mid_all // slots
        rbm = fullm * slots // tn
        if not big and fullm >= 1 and rbm * 128 < M:
            rem_rows = M - rbm * 128
            rem_mid = cdiv(rem_rows, 128) * tn
            t_now = float(cdiv(tiles_mid_all, slots))
            t_rem = 0.5 * float(cdiv(cdiv(rem_rows, 64) * cdiv(N, 64), 4 * ncu)) if rem_mid < ncu else float(cdiv(rem_mid, slots))
            t_split = float(cdiv(rbm * tn, slots)) + t_rem
            if t_split < 0.9 * t_now:
                return prefix + "split_mid+" + _tier(rem_rows, N, K, epi, ncu, ldx, ldw), rbm * 128
    return prefix + _tier(M, N, K, epi, ncu, ldx, ldw), 0


def branch(M, N, K, epi, n_cu=256, ldx=None, ldw=None, row_split=True, ln_part=False):
    return plan(M, N, K, epi, n_cu, ldx, ldw, row_split, ln_part)[0]


def split_point(M, N, n_cu=256):
    """rows in front of the row split a row-major launch of this size takes (0 = none), for choosing the rows a subset check must contain"""
    return plan(M, N, 64, BIAS, n_cu)[1]


# ---- bf16 rounding -------------------------------------------------------------------------------------------------------------------
def round_bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even, gradual underflow below 2^-126, overflow to infinity), as float64"""
    x = np.asarray(x, dtype=np.float64)
    ax = np.abs(x)
    with np.errstate(invalid="ignore", over="ignore"):
        _, e = np.frexp(np.where(np.isfinite(ax), ax, 1.0))
        q = np.maximum(e - 8, -133)
        y = np.ldexp(np.rint(np.ldexp(ax, -q)), q)
        y = np.where(y >= 2.0 ** 128, np.inf, y)
    y = np.where(np.isfinite(ax), y, ax)
    return np.copysign(y, x)


def bf16_bits(x):
    """bf16-representable float64 / float32 values -> their 16-bit patterns"""
    return (np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32) >> 16).astype(np.uint16)


def bits_to_f64(b):
    return (np.asarray(b, dtype=np.uint32) << 16).view(np.float32).astype(np.float64)


# ---- operands ------------------------------------------------------------------------------------------------------------------------
QX, QW = 2.0 ** -3, 2.0 ** -5
Q = QX * QW                                   # the accumulator quantum, 2^-8
Q_BIAS, Q_GAMMA, Q_RESID, Q_POS = 4 * Q, 2.0 ** -6, 2.0 ** -5, 2.0 ** -4


def amplitude(K):
    """|ix|, |iw| <= a + 3 with a^2 sqrt(K) / 3 ~ 1500 quanta: sums of 9 .. 13 significant bits whatever K"""
    return max(4, int(round(math.sqrt(4500.0 / math.sqrt(K)))))


def hash_ints(r, c, seed, lo, hi):
    """integers in [lo, hi], a pure function of (row, column, seed): r, c int64 numpy arrays or torch tensors (broadcast against each
    other); 32-bit mixing carried in int64 so that numpy and torch give the same values"""
    m32 = 0xFFFFFFFF
    h = (r * 0x45D9F3B + c * 0x119DE1F3 + (seed * 0x3C6EF372 + 0x1B873593) % (1 << 31)) & m32
    h = ((h ^ (h >> 16)) * 0x45D9F3B) & m32
    h = ((h ^ (h >> 16)) * 0x45D9F3B) & m32
    h = h ^ (h >> 16)
    return lo + h % (hi - lo + 1)


@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    epi: int
    claims: str                 # the branch this case is there for, at n_cu = 256
    ldx: int = 0                # 0 = the width (K / N); outputs always get ldc > N
    ldw: int = 0
    ldc: int = 0
    ldr: int = 0
    kind: str = "rand"          # "rand" | "onehot" (row m of X is e_{m % K}: acc = iw[n, m % K] + 4 ib[n] quanta) | "ramp" (bias[n] = n % 256 - 128)
    seed: int = 1
    subset: bool = False        # check the first, the last and every ragged / split-boundary tile and a stride of the other rows
    P: int = 0                  # PATCH: patches per crop; VT: unused
    npad: int = 0               # PATCH / VT: token rows per crop
    tok_off: int = 0
    heads: int = 0

    @property
    def id(self):
        return self.name

    def ld(self, which):
        width = {"x": self.K, "w": self.K, "c": self.N, "r": self.N}[which]
        v = {"x": self.ldx, "w": self.ldw, "c": self.ldc, "r": self.ldr}[which]
        if which == "c" and v == 0:
            return cdiv(self.N, 64) * 64 + 64 if self.claims == "big_asm" else self.N + 8
        return v or width

    def branch(self, n_cu=256):
        return branch(self.M, self.N, self.K, self.epi, n_cu, self.ld("x"), self.ld("w"))


def x_ints(case, rows, xp=np, cols=None):
    """rows: int64 index array (numpy or torch) -> [len(rows), K] integers ix (X = ix 2^-3)"""
    k = xp.arange(case.K, dtype=xp.int64) if cols is None else cols
    if xp is not np:
        k = k.to(rows.device)
    r, c = rows[:, None], k[None, :]
    if case.kind == "onehot":
        return ((r % case.K) == c) * 1
    a = amplitude(case.K)
    return hash_ints(r, c, case.seed, -a, a + 3)


def w_ints(case):
    a = amplitude(case.K)
    n, k = np.arange(case.N, dtype=np.int64)[:, None], np.arange(case.K, dtype=np.int64)[None, :]
    return hash_ints(n, k, case.seed + 101, -a + 2, a)


def bias_ints(case):
    n = np.arange(case.N, dtype=np.int64)
    if case.kind == "ramp":
        return n % 256 - 128
    return hash_ints(n, n * 0, case.seed + 202, -127, 127)


def gamma_ints(case):
    n = np.arange(case.N, dtype=np.int64)
    return hash_ints(n, n * 0, case.seed + 303, -100, 127)


def resid_ints(case, rows, xp=np):
    """stats cases keep the row means away from zero so that a relative bound on the mean is meaningful: ir in [128, 255], resid in [4, 8),
    against a row mean of bf16(acc) gamma that scatters by about 0.75 (N = 64) around 0 .. 2; tests/test_gemm_cases_cpu.py shows
    |mean| > 1 on every checked row of every statistics case"""
    n = xp.arange(case.N, dtype=xp.int64)
    if xp is not np:
        n = n.to(rows.device)
    lo, hi = (128, 255) if case.epi == LS_RES_STATS else (-40, 127)
    return hash_ints(rows[:, None], n[None, :], case.seed + 404, lo, hi)


def pos_ints(case):
    p, n = np.arange(case.P, dtype=np.int64)[:, None], np.arange(case.N, dtype=np.int64)[None, :]
    return hash_ints(p, n, case.seed + 505, -127, 127)


def check_rows(case, n_cu=256, split_row=None):
    """all rows, or for `subset` cases: the first tile, the last two tiles (every ragged one), 256 rows on both sides of a row split and a
    stride of 61 through the rest.  split_row: where the library says it splits the launch (default: where the mirror says)"""
    if not case.subset:
        return np.arange(case.M, dtype=np.int64)
    pick = set(range(0, min(256, case.M))) | set(range(max(0, case.M - 512), case.M)) | set(range(0, case.M, 61))
    sp = split_row if split_row is not None else split_point(case.M, case.N, n_cu) if case.epi not in (VT, PATCH) else 0
    if sp:
        pick |= set(range(max(0, sp - 256), min(case.M, sp + 256)))
    return np.array(sorted(pick), dtype=np.int64)


def acc_quanta(case, rows):
    """the exact accumulator, bias included, in quanta of 2^-8 (int64 [len(rows), N]) and the bound sum |x| |w| + |bias| on every partial sum"""
    xi, wi, bi = x_ints(case, rows).astype(np.float64), w_ints(case).astype(np.float64), bias_ints(case) * 4
    acc = (xi @ wi.T).astype(np.int64) + bi[None, :]
    bound = int((np.abs(xi) @ np.abs(wi).T).max() + np.abs(bi).max())
    return acc, bound


def rounding_shares(acc_q):
    """share of the pre-rounding values that bf16 cannot represent, and share that are exact ties of the round-to-nearest-even"""
    v = acc_q.astype(np.float64) * Q
    r = round_bf16_rne(v)
    _, e = np.frexp(np.where(v == 0, 1.0, np.abs(v)))
    half_ulp = np.ldexp(1.0, e - 9)
    return float((r != v).mean()), float(((r != v) & (np.abs(r - v) == half_ulp)).mean())


def ls_res_chain(t, gamma, resid, dtype=np.float64):
    """bf16(bf16(t * gamma) + resid) from t = bf16(acc), evaluated in `dtype` (every intermediate is exact in float32 for these operands)"""
    t, gamma, resid = t.astype(dtype), gamma.astype(dtype), resid.astype(dtype)
    u = round_bf16_rne(t * gamma).astype(dtype)
    return round_bf16_rne(u + resid)


def reference(case, rows, gelu_tab=None, dtype=np.float64):
    """bf16 values (as float64) of the output rows `rows` at the documented rounding points (gemm_bf16.h, gemm_epilogue.h):
      BIAS / VT  bf16(acc)                                   GELU   gelu_direct(bf16(acc)) through `gelu_tab` (uint16 [65536], the device's
      LS_RES(_STATS)  bf16(bf16(bf16(acc) gamma) + resid)           direct expression on every bf16 pattern; None: the pre-activation)
      PATCH      bf16(bf16(acc) + pos[m % P])
    VT and PATCH: the caller places row m (tests: scatter_rows / vt_layout)."""
    acc, _ = acc_quanta(case, rows)
    t = round_bf16_rne((acc.astype(dtype) * dtype(Q)).astype(np.float64))
    if case.epi in (BIAS, VT):
        return t
    if case.epi == GELU:
        return t if gelu_tab is None else bits_to_f64(gelu_tab[bf16_bits(t)])
    if case.epi in (LS_RES, LS_RES_STATS):
        return ls_res_chain(t, gamma_ints(case)[None, :] * Q_GAMMA, resid_ints(case, rows) * Q_RESID, dtype)
    if case.epi == PATCH:
        pos = pos_ints(case)[rows % case.P] * Q_POS
        return round_bf16_rne((t.astype(dtype) + pos.astype(dtype)).astype(np.float64))
    raise ValueError(case.epi)


def round_bits_f32(x32):
    """float32 -> bf16 patterns by the integer form of round-to-nearest-even (finite inputs); the fast path of reference_bits, shown equal to
    round_bf16_rne by tests/test_gemm_cases_cpu.py"""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    return ((u + (0x7FFF + ((u >> 16) & 1))) >> 16).astype(np.uint16)


def reference_bits(case, rows, gelu_tab=None):
    """reference() as 16-bit patterns, with the accumulator from a float32 product (exact: every partial sum is below 2^24 quanta) and the
    first rounding in integer arithmetic — the same values at a tenth of the time for the cases with 10^7 .. 10^8 outputs"""
    xi, wi = x_ints(case, rows).astype(np.float32), w_ints(case).astype(np.float32)
    acc = xi @ wi.T
    acc += (bias_ints(case) * 4).astype(np.float32)[None, :]
    acc *= np.float32(Q)
    t = round_bits_f32(acc)
    if case.epi in (BIAS, VT):
        return t
    if case.epi == GELU:
        return t if gelu_tab is None else gelu_tab[t]
    tv = bits_to_f64(t)
    if case.epi in (LS_RES, LS_RES_STATS):
        return bf16_bits(ls_res_chain(tv, gamma_ints(case)[None, :] * Q_GAMMA, resid_ints(case, rows) * Q_RESID))
    if case.epi == PATCH:
        return bf16_bits(round_bf16_rne(tv + pos_ints(case)[rows % case.P] * Q_POS))
    raise ValueError(case.epi)


def row_stats(out_rows):
    """(mean, sigma, rstd) of bf16 output rows in float64: what the finalised record of a row must decode to"""
    o = np.asarray(out_rows, dtype=np.float64)
    mean = o.mean(axis=1)
    var = np.maximum((o * o).mean(axis=1) - mean * mean, 0.0)
    sigma = np.sqrt(var + LN_EPS)
    return mean, sigma, 1.0 / sigma


def decode_record(rec_u32):
    """row record {sh, sl, sh, -mh, -ml, -mh, 0, 0} (uint32 [M,4]) -> (mean, sigma) as the init MFMA sees them: sums of the two pieces"""
    b = np.ascontiguousarray(rec_u32).view(np.uint16).reshape(-1, 8)
    f = bits_to_f64(b)
    return -(f[:, 3] + f[:, 4]), f[:, 0] + f[:, 1]


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _tiny_cross():
    Ms, Ns, Ks = (1, 15, 16, 17, 63, 65, 129, 257), (16, 48, 80, 144, 272), (64, 128, 192, 320)
    out = []
    for j in range(2):
        for i, M in enumerate(Ms):
            N, K = Ns[(i + j) % 5], Ks[(i + 2 * j + (i >> 2)) % 4]
            for epi in (BIAS, GELU, LS_RES):
                pad = dict(ldx=K + 8, ldw=K + 16, ldr=N + 24, ldc=N + 40) if j == 1 else {}
                out.append(Case(f"tiny_{EPI_NAMES[epi]}_{M}x{N}x{K}", M, N, K, epi, "tiny64", seed=len(out) + 1, **pad))
    for i, M in enumerate(Ms):                      # the statistics need whole 64-column blocks
        N, K = (64, 192, 320)[i % 3], Ks[(i + 1) % 4]
        pad = dict(ldx=K + 8, ldw=K + 8, ldr=N + 8) if i % 2 else {}
        out.append(Case(f"tiny_stats_{M}x{N}x{K}", M, N, K, LS_RES_STATS, "tiny64", seed=100 + i, **pad))
    out.append(Case("tiny_onehot_129x144x192", 129, 144, 192, BIAS, "tiny64", kind="onehot", seed=120))
    out.append(Case("tiny_ramp_65x272x128", 65, 272, 128, BIAS, "tiny64", kind="ramp", seed=121))
    out.append(Case("tiny_ramp_lsres_63x80x320", 63, 80, 320, LS_RES, "tiny64", kind="ramp", seed=122))
    return out


TINY = _tiny_cross()

SMALL = [
    Case("small_bias_2049x1936x64", 2049, 1936, 64, BIAS, "small128", seed=201),
    Case("small_gelu_2049x1936x64", 2049, 1936, 64, GELU, "small128", seed=202, ldx=72, ldw=80),
    Case("small_lsres_2049x1936x64", 2049, 1936, 64, LS_RES, "small128", seed=203, ldr=1936 + 16),
    Case("small_stats_2049x1984x64", 2049, 1984, 64, LS_RES_STATS, "small128", seed=204),
    Case("small_onehot_2049x1936x128", 2049, 1936, 128, BIAS, "small128", kind="onehot", seed=205),
    Case("small_bias_2050x2048x192", 2050, 2048, 192, BIAS, "small128", seed=206),            # an odd number of K tiles on the two-buffer loop
]

BIG = [
    Case("big_bias_48897x256x64", 48897, 256, 64, BIAS, "big_hip", seed=301, ldx=72, ldw=72),
    Case("big_stats_48897x256x64", 48897, 256, 64, LS_RES_STATS, "big_hip", seed=302, ldr=264),
    Case("big_gelu_49152x256x64", 49152, 256, 64, GELU, "big_hip", seed=303),
    Case("big_lsres_24321x272x64", 24321, 272, 64, LS_RES, "big_hip", seed=304),
    Case("big_bias_24321x272x192", 24321, 272, 192, BIAS, "big_hip", seed=305),               # an odd number of K tiles on the persistent loop
    Case("stream_bias_327680x256x64", 327680, 256, 64, BIAS, "big_hip_stream", seed=306),
    Case("stream_stats_327680x256x64", 327680, 256, 64, LS_RES_STATS, "big_hip_stream", seed=307, ldr=264, subset=True),   # non-temporal residual load
]

ASM = [
    Case("asm_bias_49152x256x2048", 49152, 256, 2048, BIAS, "big_asm", seed=401, ldx=2048 + 64, ldw=2048 + 128, subset=True),
    Case("asm_lsres_24321x272x2048", 24321, 272, 2048, LS_RES, "big_asm", seed=402, ldr=272 + 8, subset=True),
    Case("asm_gelu_24321x272x2048", 24321, 272, 2048, GELU, "big_asm", seed=403, subset=True),
    Case("asm_stats_48897x256x2048", 48897, 256, 2048, LS_RES_STATS, "big_asm", seed=404, subset=True),
]

SPLIT = [
    Case("splitbig_bias_19152x1024x64", 19152, 1024, 64, BIAS, "split_big+tiny64", seed=501),
    Case("splitbig_stats_19152x1024x64", 19152, 1024, 64, LS_RES_STATS, "split_big+tiny64", seed=502, ldr=1032),
    Case("splitmid_gelu_8256x1024x64", 8256, 1024, 64, GELU, "split_mid+tiny64", seed=503),
    Case("splitmid_stats_8256x1024x64", 8256, 1024, 64, LS_RES_STATS, "split_mid+tiny64", seed=504),
]


def _vt(B, npad, heads, claims, seed, K=64, subset=False):
    return Case(f"vt_B{B}_npad{npad}_H{heads}", B * npad, heads * 64, K, VT, claims, npad=npad, heads=heads, seed=seed, subset=subset)


VT_CASES = [
    _vt(1, 16, 1, "tiny64", 601), _vt(3, 16, 6, "tiny64", 602), _vt(1, 272, 6, "tiny64", 603), _vt(3, 272, 1, "tiny64", 604),
    _vt(3, 912, 6, "tiny64", 605, K=128), _vt(1, 912, 1, "tiny64", 606), _vt(12, 912, 6, "small128", 607),
    _vt(36, 1376, 16, "big_hip", 608), _vt(52, 1376, 16, "big_hip_stream", 609),
]


def _patch(B, gh, gw, npad, tok_off, N, K, claims, seed):
    P = gh * gw
    return Case(f"patch_B{B}_P{P}_npad{npad}_off{tok_off}_N{N}_K{K}", B * P, N, K, PATCH, claims, P=P, npad=npad, tok_off=tok_off, seed=seed)


PATCH_CASES = [
    _patch(3, 5, 7, 48, 1, 64, 64, "tiny64", 701), _patch(3, 5, 7, 48, 5, 64, 640, "tiny64", 702),
    _patch(3, 5, 7, 48, 1, 384, 640, "tiny64", 703), _patch(3, 5, 7, 48, 5, 384, 64, "tiny64", 704),
    _patch(3, 37, 37, 1376, 5, 1024, 64, "small128", 705),
]

EXACT_CASES = TINY + SMALL + BIG + ASM + SPLIT + VT_CASES + PATCH_CASES


# ---- the LayerNorm chain: LS_RES_STATS producer -> LN-folded consumer ------------------------------------------------------------------
@dataclass(frozen=True)
class Chain:
    name: str
    M: int
    D: int
    N2: int
    mode: int                   # 0: LN_BIAS, 1: LN_GELU
    claims: str                 # consumer branch with ln_part set (route 1), n_cu = 256
    K1: int = 64
    n_scaled: int = 0
    row_scale: float = 1.0
    seed: int = 1

    @property
    def producer(self):
        return Case(self.name + "_producer", self.M, self.D, self.K1, LS_RES_STATS, "", seed=self.seed)

    def branch(self, n_cu=256, ln_part=True):
        return branch(self.M, self.N2, self.D, LN_BIAS if self.mode == 0 else LN_GELU, n_cu, ln_part=ln_part)


QSCALE = 1.4426950408889634 / 8.0

CHAINS = [
    Chain("chain_tiny_160_m0", 160, 384, 1536, 0, "tiny64", seed=801),
    Chain("chain_tiny_160_m1", 160, 384, 1536, 1, "tiny64", seed=802),
    Chain("chain_tiny_150_m0_qscale", 150, 384, 1536, 0, "tiny64", seed=803, n_scaled=768, row_scale=QSCALE),     # ragged against 16
    Chain("chain_tiny_17_m1", 17, 384, 1536, 1, "tiny64", seed=804),
    Chain("chain_small_2048_m0", 2048, 256, 2048, 0, "small128", seed=805),
    Chain("chain_small_2090_m1", 2090, 256, 2048, 1, "small128", seed=806),                                       # ragged against 16, 64, 128
    Chain("chain_splitmid_8256_m0", 8256, 256, 1024, 0, "split_mid+tiny64", seed=807),
    Chain("chain_splitmid_8250_m1", 8250, 256, 1024, 1, "split_mid+tiny64", seed=808),                            # remainder ragged against 16, 64
    # the two below: fp_vit_forward finalises such shapes itself and never sets ln_part on them; route 1 pins the plan's finalize_first,
    # which runs the same finalisation kernel as route 0, so the routes agree by construction and only the bound and the records tell
    Chain("chain_finalize_49152_m0", 49152, 256, 256, 0, "finalize_then_big_hip", seed=809),
    Chain("chain_finalize_48897_m1", 48897, 256, 256, 1, "finalize_then_big_hip", seed=810),
]


def chain_operands(ch):
    """consumer-side operands: W2 [N2, D] ~ N(0, 0.05), b2, LayerNorm gamma ~ 1 +- 0.3 and beta ~ +- 0.2 as bf16 values (float64 arrays)"""
    g = np.random.default_rng(ch.seed)
    w2 = round_bf16_rne(g.normal(0.0, 0.05, (ch.N2, ch.D)))
    b2 = round_bf16_rne(g.normal(0.0, 0.5, ch.N2))
    g_ln = round_bf16_rne(1.0 + 0.3 * g.normal(size=ch.D))
    b_ln = round_bf16_rne(0.2 * g.normal(size=ch.D))
    return w2, b2, g_ln, b_ln


def chain_reference(ch, y, rows=None):
    """float64 restatement of the fold on the bf16 rows y [M, D] (float64): returns (ref, bound) of the consumer's output, both [len(rows), N2].

    ref  = rstd (y W'^T - mean cs) + b' (mode 1: GELU of it), with W' = bf16(W gamma_ln [row_scale]) — the scaled rows through the fold
           kernel's fp32 product (w gamma is exact in fp32, times row_scale rounds once to fp32, then to bf16) —, cs the column sum over the
           bf16 W', b' = (b + W beta) [row_scale], mean and sigma = sqrt(var + eps) from the bf16 rows, rstd = 1 / sigma.
    bound on |device - ref|, from the arithmetic of the kernels (never fitted):
      e_pre = 2^-15 (|b'| sigma + |mean cs|) rstd         the two-piece bf16 splits of (b', cs) and (sigma, -mean) in the init MFMA: each
                                                          product of two 16-bit splits drops the lo x lo term, 2^-16 relative, twice that
                                                          for what the fp32 statistics add
            + D 2^-23 sum_k |y| |w'| rstd                 fp32 accumulation of D products in any order
            + 1.5 2^-23 |pre|                             the 1-ulp reciprocal and the rounding of the product with it
      mode 0:  e_pre + 2^-8 (|pre| + e_pre)               one bf16 rounding (half an ulp <= 2^-8 of the value)
      mode 1:  1.13 (e_pre + 2^-8 (|pre| + e_pre)) + 2^-8 (|gelu| + that)     the GELU input rounding through a slope <= 1.13, then the output's"""
    import torch
    w2, b2, g_ln, b_ln = chain_operands(ch)
    scale = np.ones(ch.N2)
    scale[:ch.n_scaled] = ch.row_scale
    wg = (w2.astype(np.float32) * g_ln.astype(np.float32)[None, :]) * scale.astype(np.float32)[:, None]      # the fold kernel's fp32 ops
    wf = round_bf16_rne(wg.astype(np.float64))
    cs = wf.sum(axis=1)
    bp = (b2 + w2 @ b_ln) * scale.astype(np.float32).astype(np.float64)
    yr = y if rows is None else y[rows]
    mean, sigma, rstd = row_stats(yr)
    xw = yr @ wf.T
    pre = rstd[:, None] * (xw - mean[:, None] * cs[None, :]) + bp[None, :]
    e_pre = (2.0 ** -15 * (np.abs(bp)[None, :] * sigma[:, None] + np.abs(mean[:, None] * cs[None, :])) * rstd[:, None]
             + ch.D * 2.0 ** -23 * (np.abs(yr) @ np.abs(wf).T) * rstd[:, None] + 1.5 * 2.0 ** -23 * np.abs(pre))
    e_lin = e_pre + 2.0 ** -8 * (np.abs(pre) + e_pre)
    if ch.mode == 0:
        return pre, e_lin
    gelu = 0.5 * pre * (1.0 + torch.erf(torch.from_numpy(pre * 0.70710678118654752440)).numpy())
    e_in = 1.13 * e_lin
    return gelu, e_in + 2.0 ** -8 * (np.abs(gelu) + e_in)
