"""Structured inputs for the three attention kernels (csrc/attention.hip, attention_hd.hip and its causal flavour) whose correct output
is known exactly or to one bf16 neighbour, the float64 references, and a Python mirror of each kernel's dispatch.  Imports without a GPU;
tests/test_attn_cases_cpu.py proves the claims made here, tests/test_gpu_attention_exact.py runs the kernels on the cases.

Every case is a pure function of (shape, seed): q, k, v as float32 arrays [B, H, npad, hd] whose finite values are bf16-exact, the
expected rows as float64 [B, H, n_tok, hd], and the rule the kernel's output is held to.  `pack_qk_vt` / `pack_qkv` emit the layout
each kernel reads (qk + transposed v for attention.hip, [q | k | v] rows for the other two) as uint16 bf16 bit patterns.

Families
--------
select   key j carries a code in {-1, +1}^hd, query t carries c * code(pi(t)): the selected key leads every other one by at least 64 nats
         (64 log2 units on the pre-scaled path), so every other P is below 2^-64 and the output is V[pi(t)] BIT FOR BIT.  Exchanging two
         keys anywhere in the operand layouts moves a whole row.  The first pad key repeats a selected key's code, the other pad keys
         are NaN, pad V is +-2^14: a key that leaks past the mask halves a row or poisons it.
uniform  Q = 0, every P is exactly 1, V holds integers 0..15: the fp32 sums are exact and the output is the bf16 rounding of the mean
         over the visible keys — held to a bf16 neighbour of the float64 mean.  One key too many or too few moves the mean by 1/n.
pow2     one-hot queries pick one column of integer keys, so every logit is an integer; run in base 2 (the pre-scaled path of
         attention.hip as it stands, the other kernels with scale = ln 2) every P is a power of two, exact in bf16.  Sums of the
         non-negative terms P * V in fp32 stay within n * 2^-24 relative of the truth, the reciprocal and the product add a few fp32
         ulp: the output is a bf16 neighbour of the float64 reference (both neighbours of a tie are accepted).  The profiles (profile_table:
         ten named ones and six variations to fill 16 columns) walk the lazy running maximum of attention.hip across its threshold
         THR2 = 40 log2(e) / 8 = 7.21 from both sides, tile after tile; pad keys continue their profile and pad V is 2^12.  Query t
         takes column t % 16, except that every third 16-query half (one ballot of the lazy test) takes only columns that never ask
         for a rescale after the first tile, so that both a quiet ballot and a mixed one occur.
nat8     the plain path of attention.hip (q_prescaled = False): the same construction with logits that are multiples of 8, i.e.
         integer nats after the kernel's / 8, and the thresholds of the profiles moved to LAZY_THR = 40 logits = 5 nats.

The nat8 bound.  P = e^-k is no longer exact: it is rounded to bf16 by one v_cvt_pk_bf16_f32 (round to nearest even).  bf16 carries 8
significant bits (7 stored), so neighbouring values are 2^-7 apart relative to a power of two and rounding to nearest errs by at most
delta = 2^-8 relative (1 + 2^-8 rounds to 1) — not 2^-9, which would be the unit of a 9-bit significand.  With V >= 0 the numerator
sum_j P_j V_j and the denominator sum_j P_j are sums of non-negative terms each perturbed by at most delta relative, so each sum is within
delta of its true value and the quotient within (1 + delta) / (1 - delta) - 1 = 2 delta / (1 - delta) = 2^-7 + 2^-14 + ...  The final store
rounds once more to bf16: 2^-8, and the product of the two factors adds 2^-15.  The fp32 steps (the fused multiply-add that forms the
exponent with a rounded -max * log2(e) / 8, v_exp_f32, the fp32 accumulation, the reciprocal and the product) stay below 2^-13 together:
the exponent's error is at most half an ulp of a number below 2^8, 2^-17 log2 units = 5e-6 relative, v_exp_f32 is good to about 2^-22,
and n <= 336 accumulated terms add at most 336 * 2^-24 = 2e-5.  All second-order and fp32 terms fit in 2^-12.  Hence, element-wise,
        |got - ref| <= (2^-7 + 2^-8 + 2^-12) * |ref|                                                       (NAT8_RTOL)
The bound is reached in practice: a reference just above 1 + 2^-8 whose quotient lands just below it stores 1.0, 2^-8 off by the last
rounding alone.

Underflow.  v_exp_f32 returns 0 for results below 2^-126 (the kernels rely on it: that is what a masked or negligible weight should be),
so a weight that is 2^-150 of the row maximum is dropped.  With at most 336 keys of V <= 15 the dropped terms are below
336 * 15 * 2^-126 < 2^-113 of the row's scale; the neighbour and nat8 rules therefore carry the absolute term FLUSH_ATOL = 2^-110.  It
is twenty orders of magnitude below anything a wrong weight could produce here (the smallest genuine non-zero weight a profile gives a
key next to the leading ones is 2^-12) and matters only where a column of V happens to be 0 at every leading key.  Where the reference is
exactly 0 the output must be exactly 0.

What no output can show.  The VALUE of the lazy threshold is not observable while it stays far from the exponent range: a reference that
lags the row maximum by k multiplies every P, O and l of the row by 2^k until the next rescale, and binary floating point is invariant
under such a factor (bf16 P and the fp32 accumulators alike), so with integer exponents the stored bits are the same for any threshold
below about 100.  What the profiles pin is that a rescale, WHEN it happens, multiplies O and l by the same exact factor, on both sides
of the threshold and in both tile orders, and that the reference does move before P leaves the range: the lone key of profile 7 stands
150 log2 units above a settled reference, which a threshold of 150 or more turns into an infinity.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

NAT8_RTOL = 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -12
FLUSH_ATOL = 2.0 ** -110
LN2 = math.log(2.0)

# ---- bf16 helpers (numpy only) ----------------------------------------------------------------------------------------------------------


def bf16_round(x):
    """float32 values rounded to bf16 (round to nearest even), returned as float32; NaN and Inf pass through"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u >> 16) & 1) + 0x7FFF
    out = (((u + r) & 0xFFFF0000) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(x), out, x).astype(np.float32)


def bf16_exact(x) -> bool:
    """every finite value survives a round trip through bf16 unchanged"""
    x = np.asarray(x, dtype=np.float32)
    fin = np.isfinite(x)
    return bool(np.array_equal(bf16_round(x)[fin], x[fin]))


def bf16_bits(x):
    """uint16 bit patterns of bf16-exact float32 values (asserted); NaN -> 0x7FC0, +-Inf -> 0x7F80 / 0xFF80"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert bf16_exact(x), "value is not representable in bf16"
    bits = (x.view(np.uint32) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), bits).astype(np.uint16)


def bits_to_f64(bits):
    """bf16 bit patterns (uint16 or int16) -> float64"""
    b = np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << 16
    return b.view(np.float32).astype(np.float64)


def ulp_bf16(ref):
    """spacing of the bf16 numbers in the binade of |ref| (float64): 2^(floor(log2 |ref|) - 7); 0 at 0"""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    _, e = np.frexp(ref)                     # |ref| = m * 2^e, m in [0.5, 1)
    return np.where(ref == 0, 0.0, np.ldexp(1.0, e - 8))


def bf16_neighbour(got, ref, atol=0.0):
    """element-wise: got lies within one bf16 spacing of ref (|got - ref| <= ulp_bf16(ref) + atol), and is exactly 0 where ref is 0.
    At a tie (ref half way between two bf16 numbers) both are accepted; at ref = 2^k the spacing above the power of two is used."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.abs(got - ref) <= ulp_bf16(ref) + atol
    return np.where(ref == 0, got == 0, ok) & np.isfinite(got)


# ---- dispatch mirrors -------------------------------------------------------------------------------------------------------------------

KV_TILE = 64            # keys per tile, all three kernels
DINO_QB, DINO_QW = 128, 32   # attention.hip: queries per workgroup / per wave (two 16-query halves)
HD_QB, HD_QW = 64, 16        # attention_hd.hip, either mask
THR2 = 40.0 * 1.4426950408889634 / 8.0   # attention.hip, pre-scaled path: the lazy threshold in log2 units
THR_NAT = 5.0                            # attention.hip, plain path: LAZY_THR = 40 logits = 5 nats


def cdiv(a, b):
    return (a + b - 1) // b


def pad16(n):
    return cdiv(n, 16) * 16


@dataclass(frozen=True)
class DinoDispatch:
    npad: int
    ntile: int
    short_tail: bool       # the tail tile goes first through the half-length body
    clamped_last: bool     # the last tile's staging takes the clamped path (kv0 + 64 > npad)
    partial_full_pad: bool  # npad == n_tok with a partial last tile: the clamped loads duplicate the last REAL key
    ntile_odd: bool
    idle_waves: int        # waves of the last query block with q0 >= npad
    half_waves: int        # waves of the last query block that store only their first 16-query half
    nwg: int
    nwg_mod8: int
    tile_order: tuple      # key tiles in the order the kernel visits them


def dino_dispatch(B, H, n_tok) -> DinoDispatch:
    """what fp_attention_fwd / attn_fwd_kernel do with (B, H, n_tok) when npad = n_tok rounded up to 16"""
    npad = pad16(n_tok)
    ntile = cdiv(n_tok, KV_TILE)
    short = n_tok > KV_TILE and n_tok - (ntile - 1) * KV_TILE <= KV_TILE // 2
    nqb = cdiv(npad, DINO_QB)
    q0s = [(nqb - 1) * DINO_QB + w * DINO_QW for w in range(4)]
    idle = sum(q0 >= npad for q0 in q0s)
    half = sum(q0 < npad and q0 + 16 >= npad for q0 in q0s)
    nwg = nqb * H * B
    order = tuple([ntile - 1] + list(range(ntile - 1))) if short else tuple(range(ntile))
    return DinoDispatch(npad, ntile, short, (ntile - 1) * KV_TILE + KV_TILE > npad, npad == n_tok and n_tok % KV_TILE != 0,
                        ntile % 2 == 1, idle, half, nwg, nwg % 8, order)


def xcd_remap(nwg):
    """attention.hip's block order: hardware block id -> logical id; a bijection of range(nwg)"""
    q, r = nwg >> 3, nwg & 7
    out = []
    for bid in range(nwg):
        xcd, pos = bid & 7, bid >> 3
        out.append((xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + pos)
    return out


@dataclass(frozen=True)
class HdDispatch:
    npad: int
    ntile: int
    nkk: int               # 32-wide MFMA k steps (kernel instantiation 1..4)
    hd_padded: bool        # the head dimension is zero-padded in LDS (hd % 32 != 0)
    nqb: int               # 64-query blocks
    idle_waves: int        # 16-query waves of the last block with q0 >= npad
    partial_tile: bool     # the last key tile holds masked keys
    causal_tiles: tuple    # per query block: key tiles the causal kernel visits
    causal_skipped: int    # key tiles above the diagonal that are never staged, summed over the blocks


def hd_dispatch(hd, n_tok) -> HdDispatch:
    npad = pad16(n_tok)
    ntile = cdiv(n_tok, KV_TILE)
    nqb = cdiv(npad, HD_QB)
    idle = sum((nqb - 1) * HD_QB + w * HD_QW >= npad for w in range(4))
    visited = tuple(min(qb * HD_QB + HD_QB - 1, n_tok - 1) // KV_TILE + 1 for qb in range(nqb))
    return HdDispatch(npad, ntile, cdiv(hd, 32), hd % 32 != 0, nqb, idle, n_tok % KV_TILE != 0, visited, sum(ntile - v for v in visited))


# ---- shape lists ------------------------------------------------------------------------------------------------------------------------

DINO_NTOK = (1, 15, 16, 17, 32, 33, 63, 64, 65, 96, 97, 128, 129, 160, 161, 193, 257, 321)
DINO_BH = ((1, 1), (1, 3), (2, 2), (1, 5), (1, 7))
# (B, H, n_tok): every n_tok once with the (B, H) pairs in rotation, then two more for nwg = 15 and 21
DINO_SHAPES = tuple((*DINO_BH[i % 5], n) for i, n in enumerate(DINO_NTOK)) + ((1, 5, 257), (1, 7, 321))
DINO_PAD_NTOK = (17, 65, 97)

HD_DIMS = (8, 64, 80, 104, 128)   # 1, 2, 3, 4, 4 MFMA k steps: 80 (ViT-H/14) is there for the three-step instantiation
HD_NTOK = (1, 16, 17, 64, 65, 130, 257)
CAUSAL_DIMS = (8, 64, 104)
CAUSAL_NTOK = (1, 2, 16, 17, 63, 64, 65, 77, 130)


def hd_batch(n_tok):
    """(B, heads) of the attention_hd / attention_causal cases"""
    return (1, 2) if n_tok > 130 else (2, 2)


# ---- the case record --------------------------------------------------------------------------------------------------------------------


@dataclass
class Case:
    family: str            # select | uniform | pow2 | nat8
    kernel: str            # dino | hd | causal
    B: int
    H: int
    hd: int
    n_tok: int
    npad: int
    q: np.ndarray          # [B, H, npad, hd] float32, finite values bf16-exact
    k: np.ndarray
    v: np.ndarray
    expected: np.ndarray   # [B, H, n_tok, hd] float64
    rule: str              # exact | neighbour | nat8
    prescaled: bool = False   # attention.hip: q_prescaled
    scale: float = 0.125      # attention_hd / attention_causal: the scale argument
    info: dict = field(default_factory=dict)

    @property
    def causal(self):
        return self.kernel == "causal"


def softmax_ref(q, k, v, n_tok, scale=1.0, base2=False, causal=False):
    """float64 softmax(q k^T * scale) v over the first n_tok rows; base2: the logits are exponents of 2.  [B,H,n_tok,hd]"""
    q, k, v = (np.asarray(a[:, :, :n_tok], dtype=np.float64) for a in (q, k, v))
    s = np.einsum("bhqd,bhkd->bhqk", q, k) * scale
    if causal:
        s = np.where(np.tril(np.ones((n_tok, n_tok), dtype=bool)), s, -np.inf)
    s = s - s.max(axis=-1, keepdims=True)
    p = np.exp2(s) if base2 else np.exp(s)
    p /= p.sum(axis=-1, keepdims=True)
    return p @ v


def check_output(case: Case, got):
    """element-wise verdict (bool [B,H,n_tok,hd]) of the real output rows `got` (float64) under the case's rule"""
    got = np.asarray(got, dtype=np.float64)
    ref = case.expected
    if case.rule == "exact":
        return got == ref
    if case.rule == "neighbour":
        return bf16_neighbour(got, ref, FLUSH_ATOL)
    assert case.rule == "nat8"
    ok = np.abs(got - ref) <= NAT8_RTOL * np.abs(ref) + FLUSH_ATOL
    return np.where(ref == 0, got == 0, ok) & np.isfinite(got)


# ---- layouts ----------------------------------------------------------------------------------------------------------------------------


def _rows(a):
    """[B, H, npad, hd] -> [B, npad, H * hd]"""
    B, H, npad, hd = a.shape
    return a.transpose(0, 2, 1, 3).reshape(B, npad, H * hd)


def pack_qk_vt(case: Case):
    """attention.hip: qk uint16 [B * npad, 2 * H * 64] (q | k, head h at columns h * 64), vt uint16 [B, H, 64, npad]"""
    assert case.hd == 64
    qk = np.concatenate([_rows(case.q), _rows(case.k)], axis=2).reshape(case.B * case.npad, 2 * case.H * 64)
    vt = np.ascontiguousarray(case.v.transpose(0, 1, 3, 2))
    return bf16_bits(qk), bf16_bits(vt)


def pack_qkv(case: Case):
    """attention_hd / attention_causal: uint16 [B, npad, 3 * H * hd], columns [q | k | v]"""
    return bf16_bits(np.concatenate([_rows(case.q), _rows(case.k), _rows(case.v)], axis=2))


def expected_rows(case: Case):
    """expected as the kernels store it: float64 [B, n_tok, H * hd]"""
    return case.expected.transpose(0, 2, 1, 3).reshape(case.B, case.n_tok, case.H * case.hd)


def _fill_pad_k(k, n_tok, pad_k):
    if pad_k != "default":
        k[:, :, n_tok:] = {"nan": np.nan, "inf": np.inf, "zero": 0.0}[pad_k]


def _fill_pad_v(v, n_tok, pad_v):
    if pad_v != "default":
        assert pad_v == "zero"
        v[:, :, n_tok:] = 0.0


def _pad_q(q, n_tok, kernel):
    # attention.hip reads its pad query rows (their outputs are stored and must be finite); the other two never read them
    q[:, :, n_tok:] = 0.0 if kernel == "dino" else np.nan


# ---- select -----------------------------------------------------------------------------------------------------------------------------


def _select_v(rng, shape):
    mant = rng.integers(128, 256, size=shape).astype(np.float32) / 128.0
    expo = rng.integers(-4, 2, size=shape)
    sign = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=shape)
    return (sign * np.ldexp(mant, expo)).astype(np.float32)   # |v| in [2^-4, 4), 8 significant bits, never 0


@lru_cache(maxsize=None)
def select_case(kernel, B, H, hd, n_tok, seed=0, prescaled=False, pad_k="default", pad_v="default") -> Case:
    assert hd >= 64, "select needs 64 code bits"
    rng = np.random.default_rng([11, B, H, hd, n_tok, seed])
    npad = pad16(n_tok)
    causal = kernel == "causal"
    # gap between the selected key and any other: 2 c d * scale with d the Hamming distance (>= 8)
    if kernel == "dino":
        c = 4.0 if prescaled else 32.0      # 8 d log2 units on the accumulators / 8 d nats after the kernel's / 8
        gap = (lambda d: 2 * c * d) if prescaled else (lambda d: 2 * c * d / 8.0)
    else:
        c, gap = 32.0, (lambda d: 2 * 32.0 * d * 0.125)
    code = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(B, H, npad, hd))
    pi = np.empty((B, H, n_tok), dtype=np.int64)
    for b in range(B):
        for h in range(H):
            pi[b, h] = (rng.integers(0, np.arange(n_tok) + 1) if causal else rng.permutation(n_tok))
    k = code.copy()
    q = np.zeros_like(code)
    bi, hi = np.arange(B)[:, None, None], np.arange(H)[None, :, None]
    q[:, :, :n_tok] = c * code[bi, hi, pi]
    v = _select_v(rng, (B, H, npad, hd))
    # pads: the first pad key repeats the code of a key some query selects, the rest are NaN; pad V is +-2^14
    if npad > n_tok:
        k[:, :, n_tok + 1:] = np.nan
        k[:, :, n_tok] = code[np.arange(B)[:, None], np.arange(H)[None, :], pi[:, :, n_tok // 2]]
        v[:, :, n_tok:] = 16384.0 * rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(B, H, npad - n_tok, hd))
    _pad_q(q, n_tok, kernel)
    _fill_pad_k(k, n_tok, pad_k)
    _fill_pad_v(v, n_tok, pad_v)
    expected = v[bi, hi, pi].astype(np.float64)
    # preconditions
    real = code[:, :, :n_tok].astype(np.int32)
    ham = (hd - np.einsum("bhid,bhjd->bhij", real, real)) // 2
    ham[:, :, np.arange(n_tok), np.arange(n_tok)] = hd
    min_ham = int(ham.min()) if n_tok > 1 else hd
    assert min_ham >= 8, f"select: two codes only {min_ham} apart"
    assert gap(min_ham) >= 64.0
    if kernel == "dino":
        ref = softmax_ref(q, k, v, n_tok, scale=1.0 if prescaled else 0.125, base2=prescaled)
    else:
        ref = softmax_ref(q, k, v, n_tok, scale=0.125, causal=causal)
    dev = float(np.max(np.abs(ref - expected) / np.abs(expected)))
    assert dev < 2.0 ** -20, f"select: float64 softmax is {dev} away from V[pi(t)]"
    return Case("select", kernel, B, H, hd, n_tok, npad, q, k, v, expected, "exact", prescaled=prescaled, scale=0.125,
                info={"min_hamming": min_ham, "ref_dev": dev, "pi": pi})


# ---- uniform ----------------------------------------------------------------------------------------------------------------------------


@lru_cache(maxsize=None)
def uniform_case(kernel, B, H, hd, n_tok, seed=0, prescaled=False) -> Case:
    rng = np.random.default_rng([12, B, H, hd, n_tok, seed])
    npad = pad16(n_tok)
    q = np.zeros((B, H, npad, hd), dtype=np.float32)
    k = rng.integers(-8, 9, size=(B, H, npad, hd)).astype(np.float32)   # any finite keys: Q = 0 makes every logit 0
    v = rng.integers(0, 16, size=(B, H, npad, hd)).astype(np.float32)
    k[:, :, n_tok:] = np.nan     # masked after the first product (attention.hip) / never read (the other two)
    v[:, :, n_tok:] = 4096.0
    _pad_q(q, n_tok, kernel)
    csum = np.cumsum(v[:, :, :n_tok].astype(np.float64), axis=2)
    if kernel == "causal":
        expected = csum / np.arange(1, n_tok + 1, dtype=np.float64)[None, None, :, None]
    else:
        expected = np.broadcast_to(csum[:, :, -1:] / n_tok, (B, H, n_tok, hd)).copy()
    return Case("uniform", kernel, B, H, hd, n_tok, npad, q, k, v, expected, "neighbour", prescaled=prescaled, scale=0.125)


# ---- pow2 / nat8 ------------------------------------------------------------------------------------------------------------------------

N_PROFILES = 16


def profile_table(n_tok, npad, under, over, rng):
    """integer logits L[j, p] for keys j < npad (pad rows continue the profile) and the 16 profiles p; `under` / `over`: per-tile steps
    just below / above the lazy threshold (7 / 8 log2 units, 5 / 6 nats)"""
    j = np.arange(npad)
    tile = j // KV_TILE
    last = n_tok - 1
    L = np.zeros((npad, N_PROFILES), dtype=np.int64)
    L[:, 0] = j // 2                               # rising ramp
    L[:, 1] = -(j // 2)                            # falling ramp
    L[:, 2] = under * tile                         # staircase just under the threshold: the reference moves every second step
    L[:, 3] = over * tile                          # staircase over the threshold: the reference moves every tile
    L[:, 4] = -over * tile                         # falling staircase
    L[:, 5] = -100                                 # flat: the first tile pulls the reference down from 0
    if last - KV_TILE >= 0:                        # flat 0 with one `under` key a tile before the end and one `over` key at the end
        L[last - KV_TILE, 6] = under
    elif last - 2 >= 0:
        L[last - 2, 6] = under
    if last - 1 >= 0:
        L[last - 1, 6] = over
    L[last, 7] = 150                               # flat 0 with a single dominant key in the last valid position
    L[1:, 8] = -150                                # a single dominant key at position 0
    L[:, 9] = rng.integers(-12, 1, size=npad)      # random
    L[:, 10] = rng.integers(-12, 1, size=npad)
    L[:, 11] = rng.integers(-3, 1, size=npad)
    L[:, 12] = under * tile - 50
    L[:, 13] = j // 3 - 60
    L[:, 14] = over * (tile % 2)                   # up and down again
    L[:, 15] = 0
    return L


def lazy_rescales(col, n_tok, thr, order):
    """rescales AFTER the first visited tile that a query with these logits asks for, under attention.hip's lazy rule (the reference
    moves to the row maximum when a tile's maximum exceeds it by more than thr) with the tiles visited in `order`"""
    ref, count = None, 0
    for t in order:
        mx = col[t * KV_TILE:min((t + 1) * KV_TILE, n_tok)].max()
        if ref is None:
            ref = mx
        elif mx - ref > thr:
            ref, count = mx, count + 1
    return count


def _onehot_case(family, kernel, B, H, hd, n_tok, seed, pad_k, pad_v):
    nat = family == "nat8"
    rng = np.random.default_rng([13 + nat, B, H, hd, n_tok, seed])
    npad = pad16(n_tok)
    nprof = min(hd, N_PROFILES)
    under, over, thr, mult = (5, 6, THR_NAT, 8) if nat else (7, 8, THR2, 1)
    order = dino_dispatch(B, H, n_tok).tile_order
    q = np.zeros((B, H, npad, hd), dtype=np.float32)
    k = np.zeros((B, H, npad, hd), dtype=np.float32)
    logits = np.empty((B, H, n_tok, npad), dtype=np.int64)   # [query, key], pad keys included
    prof_of_query = np.empty((B, H, n_tok), dtype=np.int64)
    loud = np.zeros((B, H, n_tok), dtype=bool)
    for b in range(B):
        for h in range(H):
            table = profile_table(n_tok, npad, under, over, rng)
            cols = (np.arange(nprof) + b * H + h) % nprof if nprof == N_PROFILES else np.arange(nprof)   # column a holds profile cols[a]
            Lc = table[:, cols]
            k[b, h, :, :nprof] = mult * Lc
            rescales = np.array([lazy_rescales(Lc[:n_tok, a], n_tok, thr, order) for a in range(nprof)])
            quiet = np.flatnonzero(rescales == 0)
            for t in range(n_tok):
                # every third 16-query half (one ballot of the lazy test) holds only profiles that never ask for a rescale
                a = quiet[t % len(quiet)] if (t // 16) % 3 == 1 and len(quiet) else t % nprof
                q[b, h, t, a] = 1.0
                prof_of_query[b, h, t] = cols[a]
                loud[b, h, t] = rescales[a] > 0
                logits[b, h, t] = Lc[:, a]
    v = rng.integers(0, 16, size=(B, H, npad, hd)).astype(np.float32)
    v[:, :, n_tok:] = 4096.0
    _pad_q(q, n_tok, kernel)
    _fill_pad_k(k, n_tok, pad_k)
    _fill_pad_v(v, n_tok, pad_v)
    if nat:
        expected = softmax_ref(q, k, v, n_tok, scale=0.125)
    else:
        expected = softmax_ref(q, k, v, n_tok, base2=True, causal=kernel == "causal")
    return Case(family, kernel, B, H, hd, n_tok, npad, q, k, v, expected, "nat8" if nat else "neighbour", prescaled=not nat, scale=LN2,
                info={"logits": logits[..., :n_tok], "profile": prof_of_query, "loud": loud})


@lru_cache(maxsize=None)
def pow2_case(kernel, B, H, hd, n_tok, seed=0, pad_k="default", pad_v="default") -> Case:
    return _onehot_case("pow2", kernel, B, H, hd, n_tok, seed, pad_k, pad_v)


@lru_cache(maxsize=None)
def nat8_case(B, H, n_tok, seed=0) -> Case:
    return _onehot_case("nat8", "dino", B, H, 64, n_tok, seed, "default", "default")


def half_census(case: Case):
    """(halves whose real queries are all quiet, halves that mix quiet and rescaling queries) over the 16-query ballots of a one-hot
    case; only shapes of more than one tile can hold a rescaling query"""
    loud = case.info["loud"]
    quiet_only = mixed = 0
    for b in range(case.B):
        for h in range(case.H):
            for t0 in range(0, case.n_tok, 16):
                x = loud[b, h, t0:t0 + 16]
                quiet_only += int(not x.any())
                mixed += int(x.any() and not x.all())
    return quiet_only, mixed


# ---- case lists -------------------------------------------------------------------------------------------------------------------------


def dino_cases():
    """(id, builder) for attention.hip: both select paths, both uniform paths, pow2 (pre-scaled) and nat8 (plain) at every shape"""
    out = []
    for B, H, n in DINO_SHAPES:
        s = f"B{B}H{H}n{n}"
        out.append((f"select-plain-{s}", lambda B=B, H=H, n=n: select_case("dino", B, H, 64, n, 0, False)))
        out.append((f"select-pre-{s}", lambda B=B, H=H, n=n: select_case("dino", B, H, 64, n, 1, True)))
        out.append((f"uniform-plain-{s}", lambda B=B, H=H, n=n: uniform_case("dino", B, H, 64, n, 0, False)))
        out.append((f"uniform-pre-{s}", lambda B=B, H=H, n=n: uniform_case("dino", B, H, 64, n, 1, True)))
        out.append((f"pow2-pre-{s}", lambda B=B, H=H, n=n: pow2_case("dino", B, H, 64, n, 0)))
        out.append((f"nat8-plain-{s}", lambda B=B, H=H, n=n: nat8_case(B, H, n, 0)))
    return out


def _hd_cases(kernel, dims, ntoks):
    out = []
    for hd in dims:
        for n in ntoks:
            B, H = hd_batch(n)
            s = f"hd{hd}n{n}"
            if hd >= 64:
                out.append((f"select-{s}", lambda hd=hd, n=n, B=B, H=H: select_case(kernel, B, H, hd, n, 0)))
            out.append((f"uniform-{s}", lambda hd=hd, n=n, B=B, H=H: uniform_case(kernel, B, H, hd, n, 0)))
            out.append((f"pow2-{s}", lambda hd=hd, n=n, B=B, H=H: pow2_case(kernel, B, H, hd, n, 0)))
    return out


def hd_cases():
    return _hd_cases("hd", HD_DIMS, HD_NTOK)


def causal_cases():
    return _hd_cases("causal", CAUSAL_DIMS, CAUSAL_NTOK)
