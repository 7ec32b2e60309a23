"""Cases, float64 references and float32 restatements for the helper kernels of csrc/vit_misc.hip (CPU only: numpy, nothing on the device).

Shared by tests/test_vit_misc_cases_cpu.py (the references are right, every listed mutant of a restatement is rejected by the bound on a
committed case) and tests/test_gpu_vit_misc.py (the kernels against the references).

Bound rule, wherever a comparison is not bit for bit:

    |got - ref64| <= half_ulp_bf16(ref64) + 4 * E_case * S(elem)

S(elem) is the element's natural scale, the sum of the absolute values of the terms that make it; E_case = max |restatement_f32 - ref64| / S
over the case, where the restatement is the kernel's arithmetic in numpy float32 in the kernel's operation order.  E_case is MEASURED ON THE CPU
and stands in E_CASE below (measure_e() prints the table; the CPU test asserts that the restatements still stay under it).  The factor 4: the
device differs from the restatement by contracting multiply-adds, by its 1-ulp reciprocal / square root instructions and by nothing else, each a
few float32 ulps of S.  For fp32 outputs (decoded mean, sigma, rstd, column sum, b') the half-ulp term is replaced by the representation error of
the two-piece bf16 split, 2^-16 |value|.  No number here comes from a device.
"""
from collections import namedtuple

import numpy as np

F32 = np.float32
EPS = 1e-6


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> bf16 bits (uint16), round to nearest even, NaN kept quiet"""
    x = np.ascontiguousarray(x, dtype=F32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def bits_f32(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def rbf(x):
    return bits_f32(bf16_bits(x))


def half_ulp_bf16(v):
    """half the spacing of bf16 values around |v| (v float64); 0 at 0"""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, e = np.frexp(v)                                 # v = m 2^e, m in [0.5, 1): 8 significant bits -> ulp 2^(e-8)
    return np.where(v > 0, np.ldexp(0.5, np.maximum(e, -125) - 8), 0.0)


def bound_bf16(ref64, E, S):
    return half_ulp_bf16(ref64) + 4.0 * E * S


def bound_f32(ref64, E, S):
    return np.abs(ref64) * 2.0 ** -16 + 4.0 * E * S


def randn_bf16(seed, shape, scale=1.0, offset=0.0):
    """bf16 bits of offset + scale * N(0, 1)"""
    rng = np.random.default_rng(seed)
    return bf16_bits((offset + scale * rng.standard_normal(shape)).astype(F32))


# ---- the wave: lane l owns elements (c * 64 + l) * 8 + e; xor-butterfly sum, masks 32 -> 1 ----------------------------------------------------
_LANES = np.arange(64)


def wave_sum(v):
    """[..., 64] float32 -> [...]: the butterfly of common.h (every lane ends with the same value)"""
    for m in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANES ^ m]
    return v[..., 0]


def lanes(x):
    """[R, D] -> ([R, C, 64, 8] zero-padded, valid [C, 64]): chunk c of lane l holds elements (c * 64 + l) * 8 .. + 7"""
    R, D = x.shape
    C = -(-D // 512)
    p = np.zeros((R, C * 512), dtype=x.dtype)
    p[:, :D] = x
    valid = (np.arange(C * 64) < D // 8).reshape(C, 64)
    return p.reshape(R, C, 64, 8), valid


def fma32(a, b, c):
    """float32 fma: the product of two bf16-valued (or any 24-bit) operands is exact in float64; one rounding of the sum"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


# ---- the two-piece bf16 split of the init-MFMA records ----------------------------------------------------------------------------------------
def split_bf16(v):
    v = np.asarray(v, dtype=F32)
    h = rbf(v)
    return h, rbf(v - h)


def row_record(mean, sigma):
    """(mean, sigma) float32 [R] -> bf16 bits [R, 8] {sh, sl, sh, -mh, -ml, -mh, 0, 0} (gemm_bf16.h fp_ln_row_record)"""
    sh, sl = split_bf16(sigma)
    mh, ml = split_bf16(-np.asarray(mean, dtype=F32))
    z = np.zeros_like(sh)
    return bf16_bits(np.stack([sh, sl, sh, mh, ml, mh, z, z], axis=-1))


def decode_row_record(rec_bits):
    """bf16 bits [R, 8] -> (mean, sigma) float64; asserts the record is well formed"""
    h = bits_f32(rec_bits).astype(np.float64)
    assert np.array_equal(rec_bits[:, 0], rec_bits[:, 2]) and np.array_equal(rec_bits[:, 3], rec_bits[:, 5]), "row record: duplicated halves differ"
    assert not rec_bits[:, 6:].any(), "row record: fourth word not 0"
    return -(h[:, 3] + h[:, 4]), h[:, 0] + h[:, 1]


def decode_fold_record(rec_bits):
    """bf16 bits [N, 8] {b'h, b'h, b'l, ch, ch, cl, 0, 0} -> (b', column sum) float64"""
    h = bits_f32(rec_bits).astype(np.float64)
    assert np.array_equal(rec_bits[:, 0], rec_bits[:, 1]) and np.array_equal(rec_bits[:, 3], rec_bits[:, 4]), "fold record: duplicated halves differ"
    assert not rec_bits[:, 6:].any(), "fold record: fourth word not 0"
    return h[:, 0] + h[:, 2], h[:, 3] + h[:, 5]


# =================================================================================================================================================
# resized position embedding (posembed_aa_kernel)
PosCase = namedtuple("PosCase", "name G gh gw D offset")
POSEMBED_CASES = [
    PosCase("pos_224", 37, 16, 16, 384, 0.0),        # the 224-px product shape
    PosCase("pos_wide", 37, 16, 30, 64, 3.0),        # non-square, wide; +3: no value near zero
    PosCase("pos_tall", 37, 30, 16, 64, 0.0),        # non-square, tall
    PosCase("pos_up", 37, 40, 38, 64, 0.0),          # upscale: scale < 1
    PosCase("pos_one_axis", 37, 37, 36, 8, 0.0),     # one axis identity
    PosCase("pos_1x1", 37, 1, 1, 8, 0.0),            # the whole grid in one window
    PosCase("pos_taps", 96, 3, 5, 8, 0.0),           # ~130 taps, the largest window under AA_MAX_TAPS
    PosCase("pos_d520", 5, 3, 7, 520, 0.0),          # D not a multiple of the 256 threads
    PosCase("pos_identity", 37, 37, 37, 64, 0.0),    # identity: weights 0, 1, 0, 0, output bits == input bits
]
POSEMBED_REFUSED = (100, 2, 2, 8)
POSEMBED_MUTANTS = {"a_075": dict(a=-0.75), "no_stretch": dict(stretch=False), "unnormalised": dict(normalise=False), "swapped": dict(swap=True),
                    "start_off": dict(start_off=1), "centre": dict(half=False)}
POS_MISMATCH_GPU = 0.005      # share of elements that may differ in bits from bf16(F.interpolate(x.float(), ...))
POS_MISMATCH_CPU = 0.00125    # the restatement alone against the same


def posembed_input(case):
    return randn_bf16(100 + POSEMBED_CASES.index(case), (case.G * case.G, case.D), 1.0, case.offset)


def _cubic(t, a, dt):
    t = np.abs(t)
    one, two = dt(1), dt(2)
    near = ((dt(a) + two) * t - (dt(a) + dt(3))) * t * t + one
    far = (((t - dt(5)) * t + dt(8)) * t - dt(4)) * dt(a)
    return np.where(t < one, near, np.where(t < two, far, dt(0))).astype(dt)


def aa_weights(i, n_in, n_out, dt, a=-0.5, stretch=True, normalise=True, start_off=0, half=True):
    """window of output cell i: (first tap, weights), torch's upsample_bicubic2d_aa in precision dt"""
    scale = dt(n_in) / dt(n_out)
    shrink = bool(scale >= dt(1)) and stretch
    support = dt(2) * scale if shrink else dt(2)
    inv = dt(1) / scale if shrink else dt(1)
    centre = scale * (dt(i) + dt(0.5)) if half else scale * dt(i)
    xmin = max(int(centre - support + dt(0.5)) + start_off, 0)
    xsize = min(int(centre + support + dt(0.5)), n_in) - xmin
    w = _cubic((np.arange(xmin, xmin + xsize).astype(dt) - centre + dt(0.5)) * inv, a, dt)
    if normalise:
        s = dt(0)
        for v in w:                                   # the kernel's sequential sum
            s = dt(s + v)
        w = (w / s).astype(dt)
    return xmin, w


def posembed_restate(x_bits, G, gh, gw, swap=False, **mut):
    """posembed_aa_kernel in float32: per output cell, rows first (sequential over the x taps), then the column of row sums; [gh*gw, D] before
    the bf16 rounding"""
    x = bits_f32(x_bits).reshape(G, G, -1)
    wys = [aa_weights(oy, G, gw if swap else gh, F32, **mut) for oy in range(gh)]
    wxs = [aa_weights(ox, G, gh if swap else gw, F32, **mut) for ox in range(gw)]
    out = np.zeros((gh, gw, x.shape[2]), dtype=F32)
    for oy, (ymin, wy) in enumerate(wys):
        for ox, (xmin, wx) in enumerate(wxs):
            win = x[ymin:ymin + len(wy), xmin:xmin + len(wx)]
            row = np.zeros((len(wy), x.shape[2]), dtype=F32)
            for jx in range(len(wx)):
                row = row + wx[jx] * win[:, jx]
            acc = np.zeros(x.shape[2], dtype=F32)
            for jy in range(len(wy)):
                acc = acc + wy[jy] * row[jy]
            out[oy, ox] = acc
    return out.reshape(gh * gw, -1)


def posembed_ref64(x_bits, G, gh, gw):
    """(reference, S = sum |wy| |wx| |x|) float64 [gh*gw, D]"""
    x = bits_f32(x_bits).astype(np.float64).reshape(G, G, -1)
    Wy, Wx = np.zeros((gh, G)), np.zeros((gw, G))
    for o in range(gh):
        m, w = aa_weights(o, G, gh, np.float64)
        Wy[o, m:m + len(w)] = w
    for o in range(gw):
        m, w = aa_weights(o, G, gw, np.float64)
        Wx[o, m:m + len(w)] = w
    ref = np.einsum("yi,xj,ijd->yxd", Wy, Wx, x, optimize=True)
    S = np.einsum("yi,xj,ijd->yxd", np.abs(Wy), np.abs(Wx), np.abs(x), optimize=True)
    return ref.reshape(gh * gw, -1), S.reshape(gh * gw, -1)


def posembed_torch_f32_bits(x_bits, G, gh, gw):
    """bits of bf16(F.interpolate(x.float(), size=(gh, gw), mode="bicubic", antialias=True)): torch's own float32 path"""
    import torch
    import torch.nn.functional as Fn
    x = torch.from_numpy(bits_f32(x_bits).reshape(1, G, G, -1).copy()).permute(0, 3, 1, 2).contiguous()
    y = Fn.interpolate(x, size=(gh, gw), mode="bicubic", antialias=True)
    return bf16_bits(y.permute(0, 2, 3, 1).reshape(gh * gw, -1).numpy())


# =================================================================================================================================================
# token init (token_init_kernel)
TokCase = namedtuple("TokCase", "name B nreg P D")
TOKEN_CASES = [
    TokCase("tok_224", 2, 4, 256, 384),              # n_tok 261, npad 272
    TokCase("tok_clip", 1, 0, 15, 8),                # n_tok == npad: no pad rows, no registers (the CLIP form)
    TokCase("tok_ragged", 3, 4, 3, 72),              # nrows * D not a multiple of the block
]
TOKEN_PATTERN = 0x4B1D                               # a finite non-zero bf16 (1.0e7): what the patch rows hold before and after
TOKEN_MUTANTS = ("reg_pos", "cls_no_pos", "pad_unwritten", "patch_written")


def token_dims(case):
    n_tok = 1 + case.nreg + case.P
    return n_tok, (n_tok + 15) // 16 * 16


def token_inputs(case):
    k = 200 + TOKEN_CASES.index(case)
    return (randn_bf16(k, (case.D,)), randn_bf16(k + 50, (case.D,), 0.5), randn_bf16(k + 100, (case.nreg, case.D)))


def token_expected(case, cls, pos0, reg, mutant=None):
    """bits [B, npad, D] after the kernel ran on a buffer filled with TOKEN_PATTERN"""
    n_tok, npad = token_dims(case)
    X = np.full((case.B, npad, case.D), TOKEN_PATTERN, dtype=np.uint16)
    p = bits_f32(pos0)
    X[:, 0] = bf16_bits(bits_f32(cls) + (0 if mutant == "cls_no_pos" else p))
    if case.nreg:
        X[:, 1:1 + case.nreg] = bf16_bits(bits_f32(reg) + p) if mutant == "reg_pos" else reg
    if mutant != "pad_unwritten":
        X[:, n_tok:] = 0
    if mutant == "patch_written":
        X[:, 1 + case.nreg] = 0
    return X


# =================================================================================================================================================
# LayerNorm (layernorm_kernel<MAXC, L2>)
LnCase = namedtuple("LnCase", "name rows D regime")
LN_DIMS = (8, 384, 512, 520, 1024, 1032, 1280, 1536, 1544, 1664, 2048)
LN_REGIMES = ("normal", "offset", "lowvar", "const")
LN_CASES = ([LnCase(f"ln_d{D}", 5, D, "normal") for D in LN_DIMS] +
            [LnCase(f"ln_{r}_d{D}", 5, D, r) for D in (384, 1280) for r in LN_REGIMES[1:]] +
            [LnCase("ln_stride", 8193, 8, "normal")])                       # the grid-stride loop past 2048 blocks
LN_L2_MAX_D = 1536
LN_REFUSED = ((1664, 1), (2056, 0), (12, 0))         # (D, l2_normalize)
LN_MUTANTS = ("var_dm1", "eps_1e5", "eps_dropped", "one_pass", "l2_norm_unrounded")   # + the gather offset: gather_rows(off_by=1)
# the gather forms of the towers' final norm on a [B, npad, D] token buffer: (rows_per_b, in_off) for patches, class token, registers
GATHER_B, GATHER_NREG, GATHER_P, GATHER_D = 3, 4, 11, 384
GATHER_NPAD = 16


def gather_forms():
    return {"patch": (GATHER_P, GATHER_NPAD, 1 + GATHER_NREG), "cls": (1, GATHER_NPAD, 0), "reg": (GATHER_NREG, GATHER_NPAD, 1)}


def gather_rows(rows, rows_per_b, in_stride_b, in_off, off_by=0):
    r = np.arange(rows)
    return (r // rows_per_b) * in_stride_b + in_off + off_by + r % rows_per_b


def regime_rows(seed, rows, D, regime):
    if regime == "normal":
        return randn_bf16(seed, (rows, D), 2.0)
    if regime == "offset":
        return randn_bf16(seed, (rows, D), 1.0, 64.0)
    if regime == "lowvar":
        return randn_bf16(seed, (rows, D), 2.0 ** -10)
    return np.full((rows, D), 0x3F80, dtype=np.uint16)                      # constant rows of 1.0


def ln_inputs(case):
    k = 300 + LN_CASES.index(case)
    return (regime_rows(k, case.rows, case.D, case.regime), randn_bf16(k + 100, (case.D,), 0.25, 1.0), randn_bf16(k + 200, (case.D,), 0.5))


def _mean_var32(x, D, mutant=None, eps=EPS):
    """layernorm_kernel / row_stats_kernel: lane sums over (c, e) ascending, butterfly, two-pass variance; float32 [R]"""
    xv, valid = lanes(x)
    C = xv.shape[1]
    s = np.zeros((x.shape[0], 64), dtype=F32)
    for c in range(C):
        for e in range(8):
            s = s + xv[:, c, :, e]
    mean = wave_sum(s) / F32(D)
    sq = np.zeros_like(s)
    for c in range(C):
        for e in range(8):
            if mutant == "one_pass":
                sq = sq + xv[:, c, :, e] * xv[:, c, :, e]
            else:
                d = xv[:, c, :, e] - mean[:, None]
                sq = sq + np.where(valid[c], d * d, F32(0))
    if mutant == "one_pass":
        var = wave_sum(sq) / F32(D) - mean * mean
    else:
        var = wave_sum(sq) / F32(D - 1 if mutant == "var_dm1" else D)
    return mean, var


def ln_restate(x_bits, g_bits, b_bits, eps=EPS, mutant=None):
    """float32 [R, D] before the bf16 rounding"""
    x, g, b = bits_f32(x_bits), bits_f32(g_bits), bits_f32(b_bits)
    mean, var = _mean_var32(x, x.shape[1], mutant)
    e = {"eps_1e5": F32(1e-5), "eps_dropped": F32(0)}.get(mutant, F32(eps))
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = F32(1) / np.sqrt(var + e)
        return (x - mean[:, None]) * rstd[:, None] * g + b


def ln_ref64(x_bits, g_bits, b_bits, eps=EPS):
    """(reference, S = (|x| + |mean|) rstd |g| + |b|) float64"""
    x, g, b = (bits_f32(t).astype(np.float64) for t in (x_bits, g_bits, b_bits))
    mean = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=1, keepdims=True) + np.float64(F32(eps)))
    return (x - mean) * rstd * g + b, (np.abs(x) + np.abs(mean)) * rstd * np.abs(g) + np.abs(b)


def l2_restate(y_bits, round_norm=True):
    """F.normalize on bf16 rows with dot64.h's arithmetic: fma chain per lane, butterfly, n = max(bf16(sqrt(ss)), 1e-12), bf16(y / n)"""
    y = bits_f32(y_bits)
    yv, _ = lanes(y)
    acc = np.zeros((y.shape[0], 64), dtype=F32)
    for c in range(yv.shape[1]):
        for e in range(8):
            acc = fma32(yv[:, c, :, e], yv[:, c, :, e], acc)
    n = np.sqrt(wave_sum(acc))
    n = np.maximum(rbf(n) if round_norm else n, F32(1e-12))
    return bf16_bits(y / n[:, None])


# =================================================================================================================================================
# row statistics (row_stats_kernel<1,2,3>) and their finalisation from partial sums (stats_finalize_kernel)
StatCase = namedtuple("StatCase", "name rows D regime")
STAT_DIMS = (8, 384, 520, 1024, 1536)
STAT_CASES = ([StatCase(f"rs_{r}_d{D}", 3, D, r) for D in STAT_DIMS for r in LN_REGIMES] + [StatCase("rs_stride", 8193, 8, "normal")])
STAT_REFUSED_D = 1544
FinCase = namedtuple("FinCase", "name rows D regime pad")
FIN_CASES = [FinCase(f"fin_{r}_d{D}_pad{pad}", 257, D, r, pad) for D in (64, 1536) for r in LN_REGIMES for pad in (0, 13)]
FIN_REFUSED_D = 72
STAT_MUTANTS = ("sigma_no_eps", "mean_dm1")


def stat_inputs(case):
    cases = STAT_CASES if isinstance(case, StatCase) else FIN_CASES
    return regime_rows((400 if isinstance(case, StatCase) else 500) + cases.index(case), case.rows, case.D, case.regime)


def row_stats_restate(x_bits, eps=EPS, mutant=None):
    """(mean, sigma, rstd) float32 [R]"""
    x = bits_f32(x_bits)
    mean, var = _mean_var32(x, x.shape[1])
    sigma = np.sqrt(var + (F32(0) if mutant == "sigma_no_eps" else F32(eps)))
    with np.errstate(divide="ignore"):
        return mean, sigma, F32(1) / sigma


def row_stats_ref64(x_bits, eps=EPS):
    """{name: (reference, S)}: every term of the two-pass variance is positive, so sigma and rstd are their own scale; S(mean) = sum |x| / D"""
    x = bits_f32(x_bits).astype(np.float64)
    mean = x.mean(axis=1)
    sigma = np.sqrt(((x - mean[:, None]) ** 2).mean(axis=1) + np.float64(F32(eps)))
    return {"mean": (mean, np.abs(x).mean(axis=1)), "sigma": (sigma, sigma), "rstd": (1 / sigma, 1 / sigma)}


def partial_sums(x_bits, pad):
    """float32 [D / 64, rows + pad, 2] = (sum x, sum x^2) per 64-column block, the sums exact then rounded once; NaN in the padding columns"""
    x = bits_f32(x_bits).astype(np.float64)
    R, D = x.shape
    xb = x.reshape(R, D // 64, 64)
    part = np.full((D // 64, R + pad, 2), np.nan, dtype=F32)
    part[:, :R, 0] = xb.sum(axis=2).T.astype(F32)
    part[:, :R, 1] = (xb * xb).sum(axis=2).T.astype(F32)
    return part


def finalize_restate(part, rows, eps=EPS, mutant=None):
    """gemm_bf16.h fp_ln_finalize_row: block-order sums, mean = s / D, var = max(fma(-mean, mean, q / D), 0); (mean, sigma, rstd) float32"""
    nb = part.shape[0]
    s = np.zeros(rows, dtype=F32)
    q = np.zeros(rows, dtype=F32)
    for b in range(nb):
        s = s + part[b, :rows, 0]
        q = q + part[b, :rows, 1]
    inv_d = F32(1.0) / F32(nb * 64)
    mean = s * (F32(1.0) / F32(nb * 64 - 1) if mutant == "mean_dm1" else inv_d)
    var = np.maximum(fma32(-mean, mean, q * inv_d), F32(0))
    sigma = np.sqrt(var + (F32(0) if mutant == "sigma_no_eps" else F32(eps)))
    with np.errstate(divide="ignore"):
        return mean, sigma, F32(1) / sigma


def finalize_ref64(part, rows, eps=EPS):
    """from the float32 partial sums as given.  var = q / D - mean^2 cancels: S(sigma) = (q / D + mean^2 + eps) / (2 sigma), the terms of the
    variance through the square root's derivative, and S(rstd) = S(sigma) / sigma^2"""
    p = part[:, :rows].astype(np.float64)
    D = part.shape[0] * 64
    s, q = p[..., 0].sum(axis=0), p[..., 1].sum(axis=0)
    mean = s / D
    e = np.float64(F32(eps))
    sigma = np.sqrt(np.maximum(q / D - mean * mean, 0) + e)
    S_sigma = (q / D + mean * mean + e) / (2 * sigma)
    return {"mean": (mean, np.abs(p[..., 0]).sum(axis=0) / D), "sigma": (sigma, S_sigma), "rstd": (1 / sigma, S_sigma / sigma ** 2)}


# =================================================================================================================================================
# LayerNorm fold (ln_fold_kernel)
FoldCase = namedtuple("FoldCase", "name N K n_scaled row_scale")
FOLD_CASES = [
    FoldCase("fold_unscaled", 12, 8, 0, 1.0),                          # no scaled rows
    FoldCase("fold_ragged", 5, 520, 3, 0.18),                          # a partly filled last block; K not a multiple of 512
    FoldCase("fold_qkv", 192, 64, 64, 1.4426950408889634 / 8.0),       # the qkv form
    FoldCase("fold_two_trips", 8, 1024, 8, 0.18),                      # two trips of the K loop
]
FOLD_REFUSED_K = 12
FOLD_MUTANTS = ("colsum_unrounded", "boundary_le", "beta_unscaled")


def fold_inputs(case):
    k = 600 + FOLD_CASES.index(case)
    return (randn_bf16(k, (case.N, case.K), 0.05), randn_bf16(k + 10, (case.K,), 0.25, 1.0), randn_bf16(k + 20, (case.K,), 0.5),
            randn_bf16(k + 30, (case.N,), 0.5))


def fold_restate(W_bits, g_bits, beta_bits, bias_bits, n_scaled, row_scale, mutant=None):
    """(Wf bits [N, K], column sum float32 [N], b' float32 [N]).  Wf: the exact product of two bf16 values, times row_scale in float32, one bf16
    rounding; the column sum adds the ROUNDED Wf per lane in k order, b' = (bias + fma chain of W beta) row_scale"""
    W, g, be, bi = (bits_f32(t) for t in (W_bits, g_bits, beta_bits, bias_bits))
    N, K = W.shape
    n = np.arange(N)
    rs = np.where((n <= n_scaled) if mutant == "boundary_le" else (n < n_scaled), F32(row_scale), F32(1))[:, None].astype(F32)
    wf32 = (W * g) * rs                                                    # W * g: 16 significant bits, exact
    Wf_bits = bf16_bits(wf32)
    fv, _ = lanes(wf32 if mutant == "colsum_unrounded" else bits_f32(Wf_bits))
    wv, _ = lanes(W)
    bv, _ = lanes(np.broadcast_to(be, W.shape).copy())
    cs = np.zeros((N, 64), dtype=F32)
    wb = np.zeros((N, 64), dtype=F32)
    for c in range(fv.shape[1]):
        for e in range(8):
            cs = cs + fv[:, c, :, e]
            wb = fma32(wv[:, c, :, e], bv[:, c, :, e], wb)
    cs, wb = wave_sum(cs), wave_sum(wb)
    bp = bi * rs[:, 0] + wb if mutant == "beta_unscaled" else (bi + wb) * rs[:, 0]
    return Wf_bits, cs, bp


def fold_ref64(W_bits, beta_bits, bias_bits, Wf_bits, n_scaled, row_scale):
    """{name: (reference, S)}: the column sum over the ROUNDED W' as given, b' = (bias + W beta) scale"""
    W, be, bi, Wf = (bits_f32(t).astype(np.float64) for t in (W_bits, beta_bits, bias_bits, Wf_bits))
    rs = np.where(np.arange(W.shape[0]) < n_scaled, np.float64(F32(row_scale)), 1.0)
    return {"colsum": (Wf.sum(axis=1), np.abs(Wf).sum(axis=1)),
            "bprime": ((bi + W @ be) * rs, (np.abs(bi) + np.abs(W) @ np.abs(be)) * rs)}


# =================================================================================================================================================
# transpose (transpose_bf16_kernel): exact
TRANSPOSE_CASES = [(1, 7), (7, 1), (33, 65), (1025, 1024)]              # the last: past the 4096-block cap, the stride loop runs


def transpose_input(rows, cols):
    return (np.arange(rows * cols, dtype=np.uint32) * np.uint32(40503) >> 3).astype(np.uint16).reshape(rows, cols)


# =================================================================================================================================================
# E_case = max |restatement_f32 - ref64| / S, measured on the CPU by measure_e() and rounded up to two digits
E_CASE = {
    "pos_224": 1.1e-06, "pos_wide": 1.5e-06, "pos_tall": 4.4e-06, "pos_up": 4.6e-05, "pos_one_axis": 5.4e-05, "pos_1x1": 6.8e-09, "pos_taps": 3.7e-08,
    "pos_d520": 1.1e-06, "pos_identity": 0.0e+00, "ln_d8": 1.1e-07, "ln_d384": 1.7e-07, "ln_d512": 1.4e-07, "ln_d520": 1.3e-07, "ln_d1024": 2.3e-07,
    "ln_d1032": 1.4e-07, "ln_d1280": 1.8e-07, "ln_d1536": 2.1e-07, "ln_d1544": 2.0e-07, "ln_d1664": 1.7e-07, "ln_d2048": 1.9e-07,
    "ln_offset_d384": 2.2e-08, "ln_lowvar_d384": 1.3e-07, "ln_const_d384": 0.0e+00, "ln_offset_d1280": 2.6e-08, "ln_lowvar_d1280": 2.2e-07,
    "ln_const_d1280": 0.0e+00, "ln_stride": 2.2e-07, "rs_normal_d8:mean": 0.0e+00, "rs_normal_d8:sigma": 5.9e-08, "rs_normal_d8:rstd": 6.5e-08,
    "rs_offset_d8:mean": 0.0e+00, "rs_offset_d8:sigma": 6.6e-08, "rs_offset_d8:rstd": 9.1e-08, "rs_lowvar_d8:mean": 0.0e+00,
    "rs_lowvar_d8:sigma": 5.8e-08, "rs_lowvar_d8:rstd": 5.3e-08, "rs_const_d8:mean": 0.0e+00, "rs_const_d8:sigma": 4.9e-08,
    "rs_const_d8:rstd": 6.3e-08, "rs_normal_d384:mean": 1.6e-09, "rs_normal_d384:sigma": 3.7e-08, "rs_normal_d384:rstd": 5.9e-08,
    "rs_offset_d384:mean": 4.0e-08, "rs_offset_d384:sigma": 9.5e-08, "rs_offset_d384:rstd": 1.2e-07, "rs_lowvar_d384:mean": 1.7e-09,
    "rs_lowvar_d384:sigma": 5.0e-08, "rs_lowvar_d384:rstd": 4.8e-08, "rs_const_d384:mean": 0.0e+00, "rs_const_d384:sigma": 4.9e-08,
    "rs_const_d384:rstd": 6.3e-08, "rs_normal_d520:mean": 2.3e-09, "rs_normal_d520:sigma": 8.8e-08, "rs_normal_d520:rstd": 6.4e-08,
    "rs_offset_d520:mean": 1.6e-08, "rs_offset_d520:sigma": 4.7e-08, "rs_offset_d520:rstd": 4.7e-08, "rs_lowvar_d520:mean": 2.3e-09,
    "rs_lowvar_d520:sigma": 1.8e-08, "rs_lowvar_d520:rstd": 4.5e-08, "rs_const_d520:mean": 0.0e+00, "rs_const_d520:sigma": 4.9e-08,
    "rs_const_d520:rstd": 6.3e-08, "rs_normal_d1024:mean": 0.0e+00, "rs_normal_d1024:sigma": 5.8e-08, "rs_normal_d1024:rstd": 5.2e-08,
    "rs_offset_d1024:mean": 0.0e+00, "rs_offset_d1024:sigma": 9.8e-08, "rs_offset_d1024:rstd": 1.1e-07, "rs_lowvar_d1024:mean": 0.0e+00,
    "rs_lowvar_d1024:sigma": 2.5e-08, "rs_lowvar_d1024:rstd": 6.3e-08, "rs_const_d1024:mean": 0.0e+00, "rs_const_d1024:sigma": 4.9e-08,
    "rs_const_d1024:rstd": 6.3e-08, "rs_normal_d1536:mean": 7.6e-10, "rs_normal_d1536:sigma": 6.8e-08, "rs_normal_d1536:rstd": 4.2e-08,
    "rs_offset_d1536:mean": 2.0e-08, "rs_offset_d1536:sigma": 1.5e-07, "rs_offset_d1536:rstd": 1.7e-07, "rs_lowvar_d1536:mean": 1.2e-09,
    "rs_lowvar_d1536:sigma": 5.9e-08, "rs_lowvar_d1536:rstd": 1.1e-07, "rs_const_d1536:mean": 0.0e+00, "rs_const_d1536:sigma": 4.9e-08,
    "rs_const_d1536:rstd": 6.3e-08, "rs_stride:mean": 3.8e-08, "rs_stride:sigma": 1.8e-07, "rs_stride:rstd": 1.9e-07,
    "fin_normal_d64_pad0:mean": 0.0e+00, "fin_normal_d64_pad0:sigma": 1.7e-07, "fin_normal_d64_pad0:rstd": 1.8e-07,
    "fin_normal_d64_pad13:mean": 0.0e+00, "fin_normal_d64_pad13:sigma": 1.5e-07, "fin_normal_d64_pad13:rstd": 1.8e-07,
    "fin_offset_d64_pad0:mean": 0.0e+00, "fin_offset_d64_pad0:sigma": 2.2e-11, "fin_offset_d64_pad0:rstd": 2.8e-11,
    "fin_offset_d64_pad13:mean": 0.0e+00, "fin_offset_d64_pad13:sigma": 2.1e-11, "fin_offset_d64_pad13:rstd": 3.0e-11,
    "fin_lowvar_d64_pad0:mean": 0.0e+00, "fin_lowvar_d64_pad0:sigma": 1.5e-07, "fin_lowvar_d64_pad0:rstd": 2.1e-07,
    "fin_lowvar_d64_pad13:mean": 0.0e+00, "fin_lowvar_d64_pad13:sigma": 1.6e-07, "fin_lowvar_d64_pad13:rstd": 1.9e-07,
    "fin_const_d64_pad0:mean": 0.0e+00, "fin_const_d64_pad0:sigma": 4.9e-14, "fin_const_d64_pad0:rstd": 6.3e-14, "fin_const_d64_pad13:mean": 0.0e+00,
    "fin_const_d64_pad13:sigma": 4.9e-14, "fin_const_d64_pad13:rstd": 6.3e-14, "fin_normal_d1536_pad0:mean": 4.8e-08,
    "fin_normal_d1536_pad0:sigma": 2.6e-07, "fin_normal_d1536_pad0:rstd": 3.2e-07, "fin_normal_d1536_pad13:mean": 4.9e-08,
    "fin_normal_d1536_pad13:sigma": 2.8e-07, "fin_normal_d1536_pad13:rstd": 3.0e-07, "fin_offset_d1536_pad0:mean": 8.0e-08,
    "fin_offset_d1536_pad0:sigma": 1.6e-07, "fin_offset_d1536_pad0:rstd": 1.6e-07, "fin_offset_d1536_pad13:mean": 8.0e-08,
    "fin_offset_d1536_pad13:sigma": 1.6e-07, "fin_offset_d1536_pad13:rstd": 1.6e-07, "fin_lowvar_d1536_pad0:mean": 9.7e-08,
    "fin_lowvar_d1536_pad0:sigma": 2.9e-07, "fin_lowvar_d1536_pad0:rstd": 3.7e-07, "fin_lowvar_d1536_pad13:mean": 5.7e-08,
    "fin_lowvar_d1536_pad13:sigma": 2.7e-07, "fin_lowvar_d1536_pad13:rstd": 2.5e-07, "fin_const_d1536_pad0:mean": 0.0e+00,
    "fin_const_d1536_pad0:sigma": 4.9e-14, "fin_const_d1536_pad0:rstd": 6.3e-14, "fin_const_d1536_pad13:mean": 0.0e+00,
    "fin_const_d1536_pad13:sigma": 4.9e-14, "fin_const_d1536_pad13:rstd": 6.3e-14, "fold_unscaled:colsum": 0.0e+00, "fold_unscaled:bprime": 4.1e-08,
    "fold_ragged:colsum": 0.0e+00, "fold_ragged:bprime": 6.9e-09, "fold_qkv:colsum": 3.8e-09, "fold_qkv:bprime": 5.0e-08,
    "fold_two_trips:colsum": 4.2e-09, "fold_two_trips:bprime": 6.4e-09,
}
# share of elements whose restatement bits differ from bf16(F.interpolate(x.float(), ...)), measured on the CPU by measure_e()
POS_MISMATCH_MEASURED = {
    "pos_224": 0.00046, "pos_wide": 0.00000, "pos_tall": 0.00029, "pos_up": 0.00031, "pos_one_axis": 0.00028, "pos_1x1": 0.00000, "pos_taps": 0.00000,
    "pos_d520": 0.00027, "pos_identity": 0.00000,
}


def e_ratio(restated, ref, S):
    """max |restated - ref| / S over the elements with S > 0 (0 where every term is 0)"""
    err = np.abs(np.asarray(restated, dtype=np.float64) - ref)
    S = np.broadcast_to(S, err.shape)
    assert not err[S == 0].any()
    return float((err[S > 0] / S[S > 0]).max()) if (S > 0).any() else 0.0


def measured_e(name):
    """the measurement behind E_CASE[name]; stats and fold cases hold one value per output, keyed name + ':' + output"""
    for c in POSEMBED_CASES:
        if c.name == name:
            x = posembed_input(c)
            ref, S = posembed_ref64(x, c.G, c.gh, c.gw)
            return e_ratio(posembed_restate(x, c.G, c.gh, c.gw), ref, S)
    for c in LN_CASES:
        if c.name == name:
            x, g, b = ln_inputs(c)
            ref, S = ln_ref64(x, g, b)
            return e_ratio(ln_restate(x, g, b), ref, S)
    base, _, out = name.partition(":")
    for c in STAT_CASES + FIN_CASES:
        if c.name == base:
            x = stat_inputs(c)
            if isinstance(c, StatCase):
                got, refs = row_stats_restate(x), row_stats_ref64(x)
            else:
                part = partial_sums(x, c.pad)
                got, refs = finalize_restate(part, c.rows), finalize_ref64(part, c.rows)
            return e_ratio(got[("mean", "sigma", "rstd").index(out)], *refs[out])
    for c in FOLD_CASES:
        if c.name == base:
            W, g, be, bi = fold_inputs(c)
            Wf, cs, bp = fold_restate(W, g, be, bi, c.n_scaled, c.row_scale)
            refs = fold_ref64(W, be, bi, Wf, c.n_scaled, c.row_scale)
            return e_ratio({"colsum": cs, "bprime": bp}[out], *refs[out])
    raise KeyError(name)


def e_names():
    return ([c.name for c in POSEMBED_CASES] + [c.name for c in LN_CASES] +
            [f"{c.name}:{o}" for c in STAT_CASES + FIN_CASES for o in ("mean", "sigma", "rstd")] +
            [f"{c.name}:{o}" for c in FOLD_CASES for o in ("colsum", "bprime")])


def measure_e():
    """prints the two tables above (python -c "from tests import _vit_misc_cases as m; m.measure_e()")"""
    from math import ceil, floor, log10
    print("E_CASE = {")
    for n in e_names():
        v = measured_e(n)
        up = 0.0 if v == 0 else ceil(v / 10 ** (floor(log10(v)) - 1)) * 10 ** (floor(log10(v)) - 1)
        print(f'    "{n}": {up:.1e},')
    print("}\nPOS_MISMATCH_MEASURED = {")
    for c in POSEMBED_CASES:
        x = posembed_input(c)
        share = float((bf16_bits(posembed_restate(x, c.G, c.gh, c.gw)) != posembed_torch_f32_bits(x, c.G, c.gh, c.gw)).mean())
        print(f'    "{c.name}": {share:.5f},')
    print("}")
