// Which kernel a bf16 GEMM launch runs on: the tile tier, the row split, who finalises the row statistics, the K-tile ring depth of the
// 64x64 tier and the grid after the residency clamp — as ONE pure function of the launch's shape, the CU count and a set of options that
// is a constant in the product.  Host-only C++17 without HIP headers: gemm_bf16.hip executes the plan, tools/gemm_plan_host_check.cpp and
// tests/test_gemm_cases_cpu.py check it on a CPU, fp_op_gemm_plan reads it out of the library.  Nothing here is queried: `ncu` is an argument.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include <initializer_list>

enum FpGemmEpi {
    FP_EPI_BIAS = 0,        // C = acc + bias                           (QK part of qkv)
    FP_EPI_BIAS_GELU = 1,   // C = gelu_erf(acc + bias)                 (fc1)
    FP_EPI_BIAS_LS_RES = 2, // C = resid + gamma * (acc + bias)         (attn.proj / fc2 + LayerScale + residual)
    FP_EPI_PATCH = 3,       // C[tokrow(m)] = bf16(acc + bias) + pos[p] (patch-embed -> token buffer)
    FP_EPI_VT = 4,          // Vt[b,h,d,t] = acc + bias                 (V part of qkv, stored transposed per head)
    // ---- LayerNorm folded into the consuming GEMM:  LN(x) W^T + b  =  rstd (x W'^T - mean colsum(W')) + b'
    // with W' = W diag(gamma_ln) (bf16), colsum over the bf16 W', b' = b + W beta_ln (fp32).  X is the RAW residual stream.
    // The correction rides in the ACCUMULATOR INIT: acc0[m][n] = b'[n] sigma[m] - mean[m] cs[n] (sigma = 1/rstd), the K loop adds
    // x W'^T on top in fp32, and the epilogue is one multiply by rstd[m] — no per-feature constants are live in the epilogue.
    // acc0 is a rank-2 outer product and is formed ON THE MATRIX PIPE: one extra MFMA per accumulator block whose operands carry,
    // in 6 of their 32 k-slots, the two-piece bf16 splits (hi + lo, 16 mantissa bits) of (b', cs) per feature and (sigma, -mean) per
    // row:  b' sigma ~ b'h sh + b'h sl + b'l sh  (relative error 2^-16), likewise mean cs.  Vector-ALU work at a tile boundary costs
    // four times its instruction count (the four waves of a SIMD do it in lock-step with the matrix pipe idle): the VALU form of this
    // init was +4-5 % on the qk / V / fc1 launches (profiles/r03_ab.md).
    FP_EPI_LN_BIAS = 5,     // C = rstd (acc - mean cs) + b'            (QK part of qkv on the un-normalised x)
    FP_EPI_LN_GELU = 6,     // C = gelu_erf(bf16(rstd (acc - mean cs) + b'))   (fc1)
    FP_EPI_LN_VT = 7,       // Vt[b,h,d,t] = rstd (acc - mean cs) + b'  (V part of qkv)
    // ---- the producer side: LS_RES that also writes, per row and 64-column block, (sum x, sum x^2) of its bf16 OUTPUT rows
    FP_EPI_LS_RES_STATS = 8 // C = resid + gamma * (acc + bias);  stat_part[n/64][m] = (sum, sum of squares) over the block
};

namespace fp_plan {

constexpr bool epi_ln(int epi) { return epi == FP_EPI_LN_BIAS || epi == FP_EPI_LN_GELU || epi == FP_EPI_LN_VT; }
constexpr bool epi_trans(int epi) { return epi == FP_EPI_VT || epi == FP_EPI_LN_VT; }
constexpr bool epi_gelu(int epi) { return epi == FP_EPI_BIAS_GELU || epi == FP_EPI_LN_GELU; }
// the row -> output mapping of the transposed-V and patch-embed epilogues is per crop: their launches are never split by rows
constexpr bool epi_row_major(int epi) { return !epi_trans(epi) && epi != FP_EPI_PATCH; }

constexpr long cdiv(long a, long b) { return (a + b - 1) / b; }

// ---- LDS geometry of the tile kernels (gemm_bf16.hip gemm_bf16_kernel, gemm_asm.hip gemm_asm_kernel; their launchers static_assert these)
constexpr int BK = 64;                       // bf16 per K stage (128-byte LDS rows)
constexpr int ROW_BYTES = BK * 2;
constexpr int LDS_BUDGET = 160 * 1024;       // per CU = per workgroup at most
constexpr int GELU_TAB_BYTES = 8192 * 2;     // the table of the table-GELU epilogues, at LDS address 0 of their kernels
constexpr int EPI_STAGE_BYTES = 2048;        // row-coalescing slab of one wave's epilogue (16 rows x 128 B)
constexpr int stage_bytes(int bm, int bn) { return (bm + bn) * ROW_BYTES; }                       // one K tile of both operands
// LDS beside the K-tile buffers: the table-GELU kernels keep their slabs inside a K-tile buffer, the others one slab per wave
constexpr int fixed_bytes(int waves, bool lut) { return lut ? GELU_TAB_BYTES : waves * EPI_STAGE_BYTES; }
constexpr int dma_per_stage(int bm, int bn, int waves) { return (bm + bn) / 8 / waves; }          // LDS-DMA instructions per wave per K tile
constexpr int ring_max(int bm, int bn, int waves, bool lut) {                                     // deepest ring that fits (16 spare bytes behind it)
    return (LDS_BUDGET - fixed_bytes(waves, lut) - 16) / stage_bytes(bm, bn) < 8 ? (LDS_BUDGET - fixed_bytes(waves, lut) - 16) / stage_bytes(bm, bn) : 8;
}
// the hand-scheduled 256x256 kernel on 4 waves: [GELU table][2 K-tile buffers][2 slabs per wave]
constexpr int asm_big_lds(bool gelu) { return (gelu ? GELU_TAB_BYTES : 0) + 2 * stage_bytes(256, 256) + 4 * 2 * EPI_STAGE_BYTES; }

// ---- the CU count as its three users see it.  `n` is hipDeviceAttributeMultiprocessorCount, queried once by fp_gemm_device_cus().
// The dispatch and the persistent grids count whole groups of 8 (one CU per XCD): a persistent workgroup's tiles then keep their XCD.
// A failed query or a count below 16 (no gfx950 partition mode has one) reads as the full chip everywhere.
constexpr int ncu_dispatch(int n) { return n > 8 ? (n & ~7) : 256; }             // rounds, splits and tier thresholds
constexpr int ncu_persistent(int n) { return ncu_dispatch(n); }                  // grid clamp of the persistent kernels (n & ~7 for n >= 16)
constexpr int ncu_resident(int n) { return n >= 16 ? n : ncu_dispatch(n); }      // residency of the 64x64 tier's rings: every CU counts

// ---- the policy's constants, each stated once
// fewer 256x256 tiles than this never run on the big tier; a launch that still carries partial row statistics is promised the small tiers
// below it (fuses_ln_part), which finalise them in their prologue — the 256x256 kernels would read stale records
constexpr long BIG_MIN_TILES = 192;
// The 256x256 kernels run one resident workgroup per CU, so their time goes in whole rounds of `ncu` tiles.  When the last round would be
// mostly empty (e.g. 300 tiles on 256 CUs: the ~20-crop batches of the video path) the 128x128 kernel — ~15-20 % less efficient per flop
// but 8x finer grained — is faster: measured 0.053 vs 0.068 ms (proj), 0.157 vs 0.192 (fc2), 0.046 vs 0.063 (V) at M = 19 152, while the
// big tile wins whenever >= 75 % of its rounds are filled.
constexpr long BIG_FILL_NUM = 3, BIG_FILL_DEN = 4;
// ROW SPLIT (round 3): whole rounds of the resident grid on 256x256 tiles, the remaining rows on the finer tiers — for the launch sizes in
// between (the video path's ~20-crop batches: 600 qk tiles = 2.34 rounds, 300 proj / fc2 tiles = 1.17) where the big tile wastes most of a
// round and the small tile, ~0.56 of a big round per round of 2 tiles per CU at half the work, pays its lower efficiency on every row.
// Rows are independent and every tier produces the same bits (tests/test_gpu_fullsize.py), so the split is invisible in the results.
// Cost model in units of one big round; the split must win by 4 %.
constexpr double SMALL_ROUND_COST = 0.56;       // a round of two 128x128 tiles per CU in units of a big round (half its work)
constexpr double ASM_SMALL_ROUND_COST = 0.45;   // the same for the hand-scheduled 128x128 kernel (lab build)
constexpr double SPLIT_BIG_GAIN = 0.96;
// ROW SPLIT below the big tier (round 4): the 128x128 kernel keeps two workgroups per CU resident, so its time also goes in whole rounds
// (2 x ncu tiles) — 6 crops @518^2 give the N = 1024 layers 520 tiles = one round + 8 tiles, i.e. TWO rounds (the B = 5 -> 6 step of a
// ViT-L forward was 6.1 -> 8.7 ms).  Whole rounds run on 128x128 tiles, the remaining rows pick their own tier (a remainder below one tile
// per CU takes the 64x64 tiles, whose round is ~half the cost).  Cost model in units of one 128x128 round; the split must win by 10 %.
constexpr double TINY_ROUND_COST = 0.5;
constexpr double SPLIT_MID_GAIN = 0.9;
// STREAMING POLICY of the big tier (round 5).  Non-temporal full-line stores (and residual loads) keep a large output from dirtying every
// XCD's L2 (round 1: qk 0.373 -> 0.312 ms at 214 crops) — but an output that fits in the 256 MiB Infinity Cache beside its consumer's other
// operands is what the next kernel reads, and bypassing the caches sends that kernel to HBM.  Same-process A/B of ViT-L forwards with the
// threshold at 0 / 128 / 256 / 512 MiB / never, three boxes (profiles/r05_stream_policy_ab.log): ordinary stores below 128 MiB are
// 1.8-3.1 % faster at 5, 8 and 32 crops @420^2, -3 ... +1 % at 12 / 21 crops (box-dependent), neutral from 96 crops on; a 256 MiB
// threshold loses up to 1.5 % at 21-32 crops on two of the boxes; never streaming loses 1-3 % from 48 crops on.
constexpr long FP_GEMM_STREAM_BYTES = 128L << 20;   // big-tier outputs above this are stored non-temporally
// Where the hand-scheduled 256x256 kernel is the faster one (profiles/r04_ab.md §2, same-process A/B at M = 294 464): its main loop is
// 6-10 % faster on every ViT shape, but with one wave per SIMD the epilogue's vector-ALU work (table GELU, LayerScale + residual + row
// statistics) issues at half the rate four interleaved waves reach, so it wins when the K loop is long relative to the epilogue: fc2
// (K = 4096) +4.7 %, qk (K = 1024, plain epilogue) even, proj -2 %, fc1 (table GELU) -4 %.
constexpr int ASM_MIN_K = 2048;
// K-tile ring of the 64x64 tier: the deepest of 4 / 3 / 2 buffers with which the whole grid is still resident at once; no deeper than K.
// Deeper rings were measured and bring nothing (profiles/r04_ab.md §3: caps 8 / 6 / 4 / 3 within 1 %, 2 buffers 20-28 % slower at B = 1).
constexpr int RING_CAP = 4;

// ---- what the policy sees of a launch, and what may change its mind
struct Shape {
    int M, N, K, epi, ldx, ldw;
    bool ln_part;    // the launch carries partial row statistics nobody has finalised (FpGemmArgs::ln_part)
    bool no_split;   // FpGemmArgs::no_split
};
// The product's value is the constant Options{}.  Only the lab build fills another one, from gemm_variant / gemm_stream_mb / gemm_ring
// (gemm_bf16.hip lab_options): exactly the toggles that change the choice of tier, the split or the ring.
struct Options {
    bool force_small = false;       // never the 256x256 tier and no split
    bool never_split = false;
    bool keep_small = false;        // never the 64x64 tier
    bool tiny_unless_big = false;   // the 64x64 tier whenever not big
    bool asm_never = false;         // never the hand-scheduled big kernel
    bool asm_always = false;        // ... or wherever it supports the shape
    bool asm_ln = false;            // the hand-scheduled kernels are instantiated for LN_BIAS / LN_GELU (the lab build's are)
    // the hand-scheduled 128x128 kernel as the small tier of the row-major epilogues (lab build only: +8 ... 30 % on isolated launches with a
    // resident X, -4 ... +17 % on ViT forwards, profiles/r05_ab.md §3, not shipped): a persistent walk over two resident workgroups per CU,
    // so 0.45 of a big round per round and no split below the big tier.  _filled: only where every CU gets a tile; _long_k: K >= 2048 only
    bool asm_small = false, asm_small_filled = false, asm_small_long_k = false;
    long stream_bytes = FP_GEMM_STREAM_BYTES;
    int ring_cap = RING_CAP;
};

enum Tier { TINY64 = 0, SMALL128 = 1, BIG_HIP = 2, BIG_HIP_STREAM = 3, BIG_ASM = 4 };
enum Split { SPLIT_NONE = 0, SPLIT_BIG = 1, SPLIT_MID = 2 };
struct Part {
    int row0, rows;
    Tier tier;
    int ring;   // K-tile ring depth of a TINY64 part (0 on the other tiers: two fixed buffers)
    int grid;   // workgroups, after the residency clamp of the persistent kernels
};
// The parts of a split are never split again: two is the maximum.  Each part, the front included, takes the tier an unsplit launch of its
// rows would (part_of): a split is named for the tile its whole rounds were counted in, and nearly always its front runs on that tile.
struct Plan {
    bool finalize_first;   // fp_stats_finalize runs in front; no part carries ln_part then
    Split split;
    int nparts;
    Part part[2];
};

// ---- predicates
// the hand-scheduled kernels (gemm_asm.hip): row-major epilogues (transposed stores and the patch scatter keep the 16-wave kernel), K steps
// in pairs, 128-byte-aligned rows
inline bool asm_supported(const Shape& s, const Options& o) {
    if (!epi_row_major(s.epi)) return false;
    if (epi_ln(s.epi) && !o.asm_ln) return false;
    return s.K % 128 == 0 && s.K >= 256 && s.ldx % 64 == 0 && s.ldw % 64 == 0;
}
inline bool asm_preferred(const Shape& s, const Options& o) { return asm_supported(s, o) && s.K >= ASM_MIN_K; }   // supported AND measured faster
inline bool asm_small_supported(const Shape& s) {
    if (!epi_row_major(s.epi) || epi_gelu(s.epi)) return false;   // GELU: 96 KiB with the table = one workgroup per CU, slower than the HIP tiers
    return s.K % 128 == 0 && s.K >= 256 && s.ldx % 64 == 0 && s.ldw % 64 == 0;
}
inline bool asm_small_used(const Shape& s, long rows, int ncu, const Options& o) {
    if (!o.asm_small || !asm_small_supported(s)) return false;
    if (o.asm_small_filled && cdiv(rows, 128) * cdiv(s.N, 128) < ncu) return false;
    return !(o.asm_small_long_k && s.K < 2048);
}
inline long big_tiles(long M, long N) { return cdiv(M, 256) * cdiv(N, 256); }
// a row-major LN-folded launch of this size stays on the small tiers, i.e. finalises the partial row statistics in its prologue
inline bool fuses_ln_part(long M, long N) { return big_tiles(M, N) < BIG_MIN_TILES; }

// ---- ring and grid
// deepest ring of a kernel with this geometry whose whole grid is resident at once; `ncu` = ncu_resident(n)
inline int ring_depth(long grid, int nkt, int bm, int bn, int waves, bool lut, int ncu, int cap) {
    for (const int r : {8, 6, 4, 3}) {
        if ((r - 1) * dma_per_stage(bm, bn, waves) > 63 || r > nkt || r > cap || r > ring_max(bm, bn, waves, lut)) continue;   // (vmcnt counts 63)
        const long resident = (long)ncu * (LDS_BUDGET / (fixed_bytes(waves, lut) + r * stage_bytes(bm, bn)));
        if (grid <= resident) return r;
    }
    return 2;
}
// a persistent grid: one workgroup per resident slot at most
inline int resident_grid(long tiles, int ncu, int lds_bytes) {
    const long slots = (long)ncu * (LDS_BUDGET / lds_bytes);
    return (int)(tiles < slots ? tiles : slots);
}
// the 64x64 tier splits its tile over two waves (32 x 64 each) for the row-major epilogues: a launch that cannot fill the chip is bound by
// one wave's walk along K, and per K step a lone wave issues 16 LDS-DMA pieces for 32 MFMAs — two waves halve both (ViT-L B = 1 @518^2:
// profiles/r04_ab.md §4).  The transposed V store needs 64-token wave tiles and keeps one wave.
constexpr int tiny_waves(int epi) { return epi_trans(epi) ? 1 : 2; }

// ---- the tier of `rows` rows launched unsplit
inline bool takes_big(const Shape& s, long rows, int ncu, const Options& o) {
    const long tiles = big_tiles(rows, s.N), rounds = cdiv(tiles, ncu);
    const bool filled = tiles * BIG_FILL_DEN >= rounds * ncu * BIG_FILL_NUM;
    return tiles >= BIG_MIN_TILES && filled && !o.force_small;
}
inline Part part_of(const Shape& s0, int row0, int rows, int n, const Options& o) {
    const int ncu = ncu_dispatch(n);
    Shape s = s0;
    s.M = rows;
    Part p{row0, rows, SMALL128, 0, 0};
    if (takes_big(s, rows, ncu, o)) {
        // the hand-scheduled one-wave-per-SIMD kernel where it is the faster one, the 16-wave HIP kernel otherwise
        const bool use_asm = !o.asm_never && (o.asm_always ? asm_supported(s, o) : asm_preferred(s, o));
        p.tier = use_asm ? BIG_ASM : ((long)rows * s.N * 2 > o.stream_bytes ? BIG_HIP_STREAM : BIG_HIP);
        // both are persistent with one workgroup per CU (128 KiB and more of LDS each)
        p.grid = use_asm ? resident_grid(big_tiles(rows, s.N), ncu, asm_big_lds(epi_gelu(s.epi))) : resident_grid(big_tiles(rows, s.N), ncu_persistent(n), LDS_BUDGET);
        return p;
    }
    // A launch that cannot even give every CU one 128x128 tile (a single 518^2 crop: 88 tiles for N = 1024) runs 64x64 tiles instead — 4x the
    // workgroups, all CUs busy
    const long tiles_mid = cdiv(rows, 128) * cdiv(s.N, 128);
    if ((tiles_mid < ncu && !o.keep_small) || o.tiny_unless_big) {
        p.tier = TINY64;
        p.grid = (int)(cdiv(rows, 64) * cdiv(s.N, 64));
        p.ring = ring_depth(p.grid, s.K / BK, 64, 64, tiny_waves(s.epi), epi_gelu(s.epi), ncu_resident(n), o.ring_cap);
    } else {
        p.grid = (int)tiles_mid;
    }
    return p;
}

// ---- the plan.  `n` = the device's CU count as queried
inline Plan make_plan(const Shape& s, int n, const Options& o = Options{}) {
    const int ncu = ncu_dispatch(n);
    Plan pl{};
    // row statistics handed over as partial sums: the small tiers finalise them in the kernel prologue; anything that may touch the big tier
    // (or is a transposed store) gets them from the finalisation kernel first
    pl.finalize_first = epi_ln(s.epi) && s.ln_part && (epi_trans(s.epi) || !fuses_ln_part(s.M, s.N));
    pl.nparts = 1;
    const long M = s.M, tiles_big = big_tiles(M, s.N);
    const bool big = takes_big(s, M, ncu, o), asm_small = asm_small_used(s, M, ncu, o);
    const bool may_split = epi_row_major(s.epi) && !o.force_small && !o.never_split && !s.no_split;
    long m1 = 0;
    if (may_split) {
        const long tiles_n = cdiv(s.N, 256);
        const long full = tiles_big / ncu;              // whole rounds
        const long rb = full * ncu / tiles_n;           // 256-row blocks they cover
        if (full >= 1 && rb * 256 < M && tiles_big >= BIG_MIN_TILES) {
            const double r_small = asm_small ? ASM_SMALL_ROUND_COST : SMALL_ROUND_COST;
            auto small_cost = [&](long rows) { return (double)cdiv(cdiv(rows, 128) * cdiv(s.N, 128), 2L * ncu) * r_small; };
            const double t_now = big ? (double)cdiv(tiles_big, ncu) : small_cost(M);
            const double t_split = (double)cdiv(rb * tiles_n, ncu) + small_cost(M - rb * 256);
            if (t_split < SPLIT_BIG_GAIN * t_now) {
                pl.split = SPLIT_BIG;   // whole rounds take the 256x256 tier, the remainder picks its own (128x128 or 64x64)
                m1 = rb * 256;
            }
        }
    }
    if (may_split && pl.split == SPLIT_NONE && !big && !asm_small) {
        const long tn = cdiv(s.N, 128), slots = 2L * ncu, tiles_mid_all = cdiv(M, 128) * tn;
        const long fullm = tiles_mid_all / slots;
        const long rbm = fullm * slots / tn;            // 128-row blocks the whole rounds cover
        if (fullm >= 1 && rbm * 128 < M) {
            const long rem_rows = M - rbm * 128, rem_mid = cdiv(rem_rows, 128) * tn;
            const double t_now = (double)cdiv(tiles_mid_all, slots);
            const double t_rem = rem_mid < ncu ? TINY_ROUND_COST * (double)cdiv(cdiv(rem_rows, 64) * cdiv(s.N, 64), 4L * ncu) : (double)cdiv(rem_mid, slots);
            const double t_split = (double)cdiv(rbm * tn, slots) + t_rem;
            if (t_split < SPLIT_MID_GAIN * t_now) {
                pl.split = SPLIT_MID;
                m1 = rbm * 128;
            }
        }
    }
    if (pl.split == SPLIT_NONE) {
        pl.part[0] = part_of(s, 0, s.M, n, o);
    } else {
        pl.nparts = 2;
        pl.part[0] = part_of(s, 0, (int)m1, n, o);
        pl.part[1] = part_of(s, (int)m1, s.M - (int)m1, n, o);
    }
    return pl;
}

// ---- the plan in words: tiny64 | small128 | big_hip | big_hip_stream | big_asm, split_big+<rest> / split_mid+<rest> (<rest> = the tier of the
// remaining rows), finalize_then_<path>; then " row0=<r> ring=<a>,<b> grid=<a>,<b>" (row0 = first row of the second part; 0 = no such part)
inline const char* tier_name(Tier t) {
    switch (t) {
        case TINY64: return "tiny64";
        case SMALL128: return "small128";
        case BIG_HIP: return "big_hip";
        case BIG_HIP_STREAM: return "big_hip_stream";
        default: return "big_asm";
    }
}
inline int plan_label(const Plan& p, char* out, size_t n) {
    return snprintf(out, n, "%s%s%s", p.finalize_first ? "finalize_then_" : "", p.split == SPLIT_BIG ? "split_big+" : p.split == SPLIT_MID ? "split_mid+" : "",
                    tier_name(p.part[p.nparts - 1].tier));
}
inline int plan_text(const Plan& p, char* out, size_t n) {
    const int k = plan_label(p, out, n);
    if (k < 0 || (size_t)k >= n) return k;
    const Part& a = p.part[0];
    const Part b = p.nparts == 2 ? p.part[1] : Part{0, 0, TINY64, 0, 0};
    return k + snprintf(out + k, n - k, " row0=%d ring=%d,%d grid=%d,%d", b.row0, a.ring, b.ring, a.grid, b.grid);
}

}  // namespace fp_plan
