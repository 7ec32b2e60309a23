// Fused GEMM epilogues shared by the GEMM kernels (same accumulator layout: acc[TC][TR], R operand = permuted rows in the
// MFMA A slot, so a lane owns 4*TR consecutive R indices for each of its TC C-operand rows).
#pragma once
#include <type_traits>

#include "gemm_bf16.h"

namespace fp_gemm {

__device__ __forceinline__ float gelu_erf(float x) {
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}
// ---- table GELU -----------------------------------------------------------------------------------------------------------
// The GELU input is the fc1 output ROUNDED TO BF16 (the reference's rounding point) and its output is rounded to bf16 again,
// so the whole activation is a map bf16 -> bf16.  Outside |x| in [2^-15, 2^17) it is closed-form in bf16 (0.5 x below — exact,
// a power-of-two scaling; x or -0 above), inside that window a 8192-entry table (2 signs x 32 exponents x 128 mantissas, 16 KiB
// of LDS) holds bf16(gelu_erf(x)) for every input pattern, filled once per device by gelu_table_kernel with the SAME device
// expression gelu_erf() the direct variant evaluates — the table variant is bit-identical to it by construction (tested over all
// 65 536 input patterns) at ~5.5 VALU ops + one LDS gather per element instead of ~11 + v_rcp + v_exp.  On gfx950 the vector ALU
// and the matrix pipe do not overlap, so the fc1 epilogue's ALU time is paid in full: ~7 us of a 34 us tile before.
//
// Index of pattern p (16 bit): (p & 0xfff) | ((p >> 3) & 0x1000): the low 5 exponent bits + mantissa are taken as they are (the
// window 112 <= exp < 144 is a bijection onto exp & 31), the sign moves next to them.
constexpr int GELU_TAB_ENTRIES = 8192;
constexpr int GELU_TAB_BYTES = fp_plan::GELU_TAB_BYTES;   // (stated in gemm_plan.h: the launch policy budgets the LDS with it)
static_assert(GELU_TAB_BYTES == GELU_TAB_ENTRIES * 2, "GELU table: one bf16 per entry");
constexpr uint32_t GELU_WIN_LO = 112u << 7, GELU_WIN_HI = 144u << 7;      // abs-pattern window [LO, HI)

__device__ __forceinline__ uint32_t gelu_tab_pattern(int i) {              // table index -> bf16 input pattern
    const uint32_t s = (uint32_t)i >> 12, e5 = ((uint32_t)i >> 7) & 31u, m = (uint32_t)i & 127u;
    const uint32_t ex = e5 >= 16u ? 96u + e5 : 128u + e5;
    return (s << 15) | (ex << 7) | m;
}
// generic (any input) table GELU of one bf16 pattern; `tab` = LDS table
__device__ __forceinline__ uint32_t gelu_tab_any(uint32_t p16, const uint16_t* tab) {
    const uint32_t a = p16 & 0x7fffu;
    if (a >= GELU_WIN_LO && a < GELU_WIN_HI) return tab[(p16 & 0xfffu) | ((p16 >> 3) & 0x1000u)];
    const float x = __uint_as_float(p16 << 16);
    if (a > 0x7f80u || p16 == 0xff80u) return p16 | 0x40u;                  // NaN stays NaN; -inf * (1 + erf(-inf)) = -inf * 0 = NaN
    const float y = (a < GELU_WIN_LO) ? 0.5f * x : fmaxf(x, -0.0f);         // tiny: x/2 (exact); huge: x or -0
    return __float_as_uint(rbf(y)) >> 16;
}
// 16 values of one lane (already + bias, fp32) -> 8 packed bf16 pairs of gelu(bf16(v))
__device__ __forceinline__ void gelu_tab16(const float (&v)[16], uint32_t (&out)[8], const char* tab) {
    uint32_t w[8];
    uint32_t amin = 0x7fff7fffu, amax = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        w[k] = pack_bf2(v[2 * k], v[2 * k + 1]);
        const uint32_t a2 = w[k] & 0x7fff7fffu;
        amin = pk_min_u16(amin, a2);
        amax = pk_max_u16(amax, a2);
    }
    const uint32_t lo = min(amin & 0xffffu, amin >> 16), hi = max(amax & 0xffffu, amax >> 16);
    const bool inside = lo >= GELU_WIN_LO && hi < GELU_WIN_HI;
    if (__builtin_amdgcn_ballot_w64(!inside) == 0ull) {
        // every element of the wave's block is inside the window: two indices per VALU op
        // the gathers address the table at LDS byte 0: the GEMM kernels put it first in their dynamic LDS, have no static LDS,
        // and TRAP at entry if the table's LDS address is not 0 (gemm_bf16.hip) — adding the base here would cost a VALU add per
        // address in a loop whose VALU time is paid in full
        uint32_t alo[8], ahi[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t u = (((w[k] >> 3) & 0x10001000u) | (w[k] & 0x0fff0fffu)) << 1;   // two byte offsets
            alo[k] = u & 0xffffu;
            ahi[k] = u >> 16;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // (with SRAM ECC a d16 load clears the other half of its destination instead of keeping it, so the halves of a pair
            // are gathered into two registers — low element zero-extended, high element by d16_hi — and OR-ed.  The library is
            // built for gfx950:sramecc+ only (build.py), so the code object does not load on a device in the other mode.)
            uint32_t r0, r1, r2, r3, q0, q1, q2, q3;
            asm volatile(
                "ds_read_u16 %0, %8\n\tds_read_u16 %1, %9\n\tds_read_u16 %2, %10\n\tds_read_u16 %3, %11\n\t"
                "ds_read_u16_d16_hi %4, %12\n\tds_read_u16_d16_hi %5, %13\n\tds_read_u16_d16_hi %6, %14\n\tds_read_u16_d16_hi %7, %15\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3)
                : "v"(alo[4 * h]), "v"(alo[4 * h + 1]), "v"(alo[4 * h + 2]), "v"(alo[4 * h + 3]),
                  "v"(ahi[4 * h]), "v"(ahi[4 * h + 1]), "v"(ahi[4 * h + 2]), "v"(ahi[4 * h + 3])
                : "memory");
            r0 |= q0; r1 |= q1; r2 |= q2; r3 |= q3;
            out[4 * h] = r0; out[4 * h + 1] = r1; out[4 * h + 2] = r2; out[4 * h + 3] = r3;
        }
    } else {
        const uint16_t* t16 = (const uint16_t*)tab;
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = gelu_tab_any(w[k] & 0xffffu, t16) | (gelu_tab_any(w[k] >> 16, t16) << 16);
    }
}

// The same table GELU in two halves for a software-pipelined epilogue (epilogue_pipe): `issue` packs the 16 values, checks the window
// and sends the 16 LDS gathers WITHOUT waiting; `finish` — at least one block of other work later — waits and combines.  hipcc does not
// see the gathers (inline asm): between the two calls the caller must not let a compiler-counted LDS wait depend on them (see there).
struct GeluPending {
    uint32_t w[8];       // packed bf16 inputs (fallback path)
    uint32_t r[8], q[8]; // gather destinations: low / high element of each pair
    bool inside;         // wave-uniform: every element of the wave's block is inside the table window
};
__device__ __forceinline__ void gelu_tab16_issue(const float (&v)[16], GeluPending& st) {
    uint32_t amin = 0x7fff7fffu, amax = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        st.w[k] = pack_bf2(v[2 * k], v[2 * k + 1]);
        const uint32_t a2 = st.w[k] & 0x7fff7fffu;
        amin = pk_min_u16(amin, a2);
        amax = pk_max_u16(amax, a2);
    }
    const uint32_t lo = min(amin & 0xffffu, amin >> 16), hi = max(amax & 0xffffu, amax >> 16);
    const bool in = lo >= GELU_WIN_LO && hi < GELU_WIN_HI;
    st.inside = __builtin_amdgcn_ballot_w64(!in) == 0ull;
    if (st.inside) {
        uint32_t alo[8], ahi[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t u = (((st.w[k] >> 3) & 0x10001000u) | (st.w[k] & 0x0fff0fffu)) << 1;   // two byte offsets (table at LDS byte 0)
            alo[k] = u & 0xffffu;
            ahi[k] = u >> 16;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
            asm volatile(
                "ds_read_u16 %0, %8\n\tds_read_u16 %1, %9\n\tds_read_u16 %2, %10\n\tds_read_u16 %3, %11\n\t"
                "ds_read_u16_d16_hi %4, %12\n\tds_read_u16_d16_hi %5, %13\n\tds_read_u16_d16_hi %6, %14\n\tds_read_u16_d16_hi %7, %15"
                : "=&v"(st.r[4 * h]), "=&v"(st.r[4 * h + 1]), "=&v"(st.r[4 * h + 2]), "=&v"(st.r[4 * h + 3]),
                  "=&v"(st.q[4 * h]), "=&v"(st.q[4 * h + 1]), "=&v"(st.q[4 * h + 2]), "=&v"(st.q[4 * h + 3])
                : "v"(alo[4 * h]), "v"(alo[4 * h + 1]), "v"(alo[4 * h + 2]), "v"(alo[4 * h + 3]),
                  "v"(ahi[4 * h]), "v"(ahi[4 * h + 1]), "v"(ahi[4 * h + 2]), "v"(ahi[4 * h + 3])
                : "memory");
    }
}
__device__ __forceinline__ void gelu_tab16_finish(GeluPending& st, uint32_t (&out)[8], const char* tab) {
    if (st.inside) {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(st.r[0]), "+v"(st.r[1]), "+v"(st.r[2]), "+v"(st.r[3]), "+v"(st.r[4]), "+v"(st.r[5]), "+v"(st.r[6]), "+v"(st.r[7]),
                       "+v"(st.q[0]), "+v"(st.q[1]), "+v"(st.q[2]), "+v"(st.q[3]), "+v"(st.q[4]), "+v"(st.q[5]), "+v"(st.q[6]), "+v"(st.q[7])
                     :
                     : "memory");
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = st.r[k] | st.q[k];
    } else {
        const uint16_t* t16 = (const uint16_t*)tab;
#pragma unroll
        for (int k = 0; k < 8; ++k) out[k] = gelu_tab_any(st.w[k] & 0xffffu, t16) | (gelu_tab_any(st.w[k] >> 16, t16) << 16);
    }
}

// bytes of LDS each wave needs for the row-coalescing stage of the non-transposed epilogues (16 rows x 128 B)
constexpr int EPI_STAGE_BYTES = fp_plan::EPI_STAGE_BYTES;

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

// compile-time loop: f(std::integral_constant<int, I>) for I = 0 .. N-1 (the accumulator accessors need constant indices)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// Accumulator accessors.  The epilogues consume a wave's accumulators in 16-token x 64-feature blocks: for row block I and
// 64-feature group G the lane's 16 values are acc[I][4 G + j][r], j = 0..3, r = 0..3 (feature 64 G + 16 lg + 4 j + r of token 16 I + li).
//   RegAcc : the compiler-managed f32x4 array of the HIP main loops (gemm_bf16.hip)
//   AgprAcc: the accumulator file of the hand-scheduled main loop (gemm_asm.hip): fragment f = I TR + jj lives in a[4 f .. 4 f + 3],
//            so a block is the 16 CONSECUTIVE registers a[4 (I TR + 4 G) ..]; read with v_accvgpr_read (constant indices)
template <int TC, int TR>
struct RegAcc {
    f32x4_t (&a)[TC][TR];
    template <int I, int G>
    __device__ __forceinline__ void load16(float (&v)[16]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[4 * j + r] = a[I][G * 4 + j][r];
    }
};
template <int TR>
struct AgprAcc {
    template <int I, int G>
    __device__ __forceinline__ void load16(float (&v)[16]) const {
        constexpr int B = 4 * (I * TR + 4 * G);
        asm volatile("v_accvgpr_read_b32 %0, a[%c8]\n\tv_accvgpr_read_b32 %1, a[%c9]\n\tv_accvgpr_read_b32 %2, a[%c10]\n\tv_accvgpr_read_b32 %3, a[%c11]\n\t"
                     "v_accvgpr_read_b32 %4, a[%c12]\n\tv_accvgpr_read_b32 %5, a[%c13]\n\tv_accvgpr_read_b32 %6, a[%c14]\n\tv_accvgpr_read_b32 %7, a[%c15]"
                     : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3]), "=v"(v[4]), "=v"(v[5]), "=v"(v[6]), "=v"(v[7])
                     : "n"(B), "n"(B + 1), "n"(B + 2), "n"(B + 3), "n"(B + 4), "n"(B + 5), "n"(B + 6), "n"(B + 7));
        asm volatile("v_accvgpr_read_b32 %0, a[%c8]\n\tv_accvgpr_read_b32 %1, a[%c9]\n\tv_accvgpr_read_b32 %2, a[%c10]\n\tv_accvgpr_read_b32 %3, a[%c11]\n\t"
                     "v_accvgpr_read_b32 %4, a[%c12]\n\tv_accvgpr_read_b32 %5, a[%c13]\n\tv_accvgpr_read_b32 %6, a[%c14]\n\tv_accvgpr_read_b32 %7, a[%c15]"
                     : "=v"(v[8]), "=v"(v[9]), "=v"(v[10]), "=v"(v[11]), "=v"(v[12]), "=v"(v[13]), "=v"(v[14]), "=v"(v[15])
                     : "n"(B + 8), "n"(B + 9), "n"(B + 10), "n"(B + 11), "n"(B + 12), "n"(B + 13), "n"(B + 14), "n"(B + 15));
    }
};

// `stg`: this wave's private EPI_STAGE_BYTES slab of LDS (unused by the transposed epilogue).
//
// Non-transposed epilogues run in two phases per 16-token x 64-feature block of the wave tile:
//   phase 1 (accumulator layout: lane = token row li, 16 consecutive features; bias already accumulated): [GELU,] round to bf16, write the
//            lane's 32 B into the slab (row li; 16-B slots XOR-swizzled with (row>>1)&7 like the operand tiles);
//   phase 2 (row layout: 8 lanes x 16 B = one full 128-B output row, 8 rows per instruction): read back, apply
//            LayerScale+residual / position embedding with equally coalesced loads, store.
// Full rows are what allows STREAMING stores (fp_gemm::V_STREAM_IO, used by the big-tile kernels whose outputs are far larger than
// L2 + MALL): measured (profiles/r01_ab.md) the write-back tail of plain stores cost 10-25 % of each GEMM — every tile
// round dirties the whole L2 and the next round stalls on its eviction — while non-temporal full-line stores bring the
// bias-only GEMM to the vendor library's epilogue-free time.  From the accumulator layout (16 lines per 16-lane pass)
// streaming stores would be partial-line writes.
//
// LN-folded epilogues (FP_EPI_LN_*, gemm_bf16.h): the kernels start the accumulators at  b'[n] sigma[m] - mean[m] cs[n]  instead of the
// bias, so after the K loop  acc = x W'^T - mean cs + b' sigma  and phase 1 is ONE multiply by rstd[m] (the lane's token row; one
// 4-byte load per 16-row block, all requested up front) before the bf16 rounding point.  A first version applied the correction here
// (2 FMAs per element, the 64 (cs, b') pairs of the wave staged in LDS, relocated slabs in the 16-wave kernel): measured +4.8 % GEMM
// time (r03), i.e. almost all of the LayerNorm kernel it replaced; the init form needs no per-feature constant in the epilogue.
// (Carrying rstd from the init to the epilogue through LDS instead of re-loading it was also tried: the 128-VGPR kernels then
// spill 17-21 registers around the epilogue and run 12 % slower.)
// FP_EPI_LS_RES_STATS (producer side): phase 2 additionally reduces (sum, sum of squares) of each bf16 OUTPUT row over the wave's
// 64 columns — v_dot2c_f32_bf16 on the packed pairs, xor-butterfly over the row's 8 lanes, fixed order — and writes them to
// stat_part[n/64][m].  The partials are per 64-column block whatever the tile shape, so every tile tier produces the same bits.
template <int BM, int BN, int WM, int WN, int EPI, int VAR, int TC, int TR, class Acc>
__device__ __forceinline__ void epilogue_acc(const FpGemmArgs& p, const Acc& accs, int m0, int n0, int wm, int wn,
                                             int li, int lg, char* stg, const char* gelu_tab = nullptr) {
    // Everything below that depends only on the lane (slab addresses, row / chunk roles, output offsets) is re-derived per tile from
    // these two laundered values: left to itself hipcc hoists it out of the persistent tile loop, keeps it live through the K loop
    // of a 128-VGPR kernel and spills it — and a scratch reload inside the epilogue waits (vmcnt is in-order) for every output
    // store issued before it.
    asm volatile("" : "+v"(li), "+v"(lg));
    constexpr bool TRANS = FpEpiTraits<EPI>::TRANS;
    constexpr bool LNF = FpEpiTraits<EPI>::LN;
    constexpr bool EGELU = FpEpiTraits<EPI>::GELU;
    constexpr bool LSRES = FpEpiTraits<EPI>::LSRES;
    constexpr bool STATS = FpEpiTraits<EPI>::STATS;
    constexpr int TM = BM / WM / 16;
    constexpr int TN = BN / WN / 16;
    if constexpr (!TRANS) {
        static_assert(TN % 4 == 0, "wave tile width must be a multiple of 64 columns");
        constexpr int NG = TN / 4;
        const int lane = lg * 16 + li;
        const int prow = lane >> 3, pslot = lane & 7;           // phase-2 role: row inside an 8-row half, 16-B column chunk
        char* wr = stg + li * 128;
        const int wkey = key_plain(li);                        // slab_addr(li, slot) = wr + ((slot ^ wkey) << 4)
        const int mbase = m0 + wm * (16 * TM);
        // Output stores and residual loads go through buffer descriptors clipped at row M (an out-of-range offset is dropped / reads
        // zero) and a lane whose 8 columns lie past N gets an offset past every range: no bounds branch, no 64-bit address arithmetic
        // per access (a fifth of the plain epilogue's vector-ALU instructions).  The patch scatter keeps pointers (rows move per crop).
        constexpr bool BUF = EPI != FP_EPI_PATCH;
        constexpr int AUX = stream_io(VAR) ? 2 : 0;                 // streaming (non-temporal) policy of the big-tile kernels
        const int rows_left = max(p.M - mbase, 0);
        auto records = [&](int ld) { const unsigned long long bb = (unsigned long long)rows_left * (unsigned)ld * 2ull; return (int)(bb > 0x7fffffffull ? 0x7fffffffull : bb); };
        __amdgpu_buffer_rsrc_t rsC, rsR;
        if constexpr (BUF) {
            rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(p.C + (size_t)min(mbase, p.M) * p.ldc), 0, records(p.ldc), 0x00020000);
            rsR = rsC;
            if constexpr (LSRES) rsR = __builtin_amdgcn_make_buffer_rsrc((void*)(p.resid + (size_t)min(mbase, p.M) * p.ldr), 0, records(p.ldr), 0x00020000);
        }
        const int ldc2 = p.ldc * 2, ldr2 = p.ldr * 2;
        static_for<0, NG>([&](auto grp_c) {
            constexpr int grp = decltype(grp_c)::value;
            const int nbw = n0 + wn * (16 * TN) + grp * 64;     // the wave's 64-feature group
            const int nb1 = nbw + lg * 16;                      // phase-1 features of this lane
            const int nb2 = nbw + pslot * 8;                    // phase-2 features of this lane
            // (the bias is already in the accumulators: the GEMM kernels start them at it, gemm_bf16.hip init_acc; the transposed
            //  V store below still adds it here)
            // LayerScale stays packed (bf16 pairs) and is unpacked at use: the 16-wave kernels run at 128 VGPRs
            uint32_t gamw[4];
            (void)nb1;
            // LayerScale+residual: the residual rows of block i+1 are requested (row layout, 16 B per lane) before block i
            // is processed, so their HBM latency overlaps a whole block instead of sitting between an LDS read and its store
            uint4 res[2][2];
            const bool col_ok = nb2 < p.N;
            auto load_res = [&](int i, uint4 (&r)[2]) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int off = col_ok ? (16 * i + h * 8 + prow) * ldr2 + nb2 * 2 : 0x7fffffff;
                    const u32x4_t rv = __builtin_amdgcn_raw_buffer_load_b128(rsR, off, 0, AUX);        // read once: streaming too
                    r[h] = make_uint4(rv.x, rv.y, rv.z, rv.w);
                }
            };
            if constexpr (LSRES) {
                const uint4 g0 = *(const uint4*)(p.gamma + min(nb2, p.N - 8));
                gamw[0] = g0.x; gamw[1] = g0.y; gamw[2] = g0.z; gamw[3] = g0.w;
                load_res(0, res[0]);
            }
            float rs[LNF ? TM : 1];                                // rstd of this lane's row in each 16-row block
            if constexpr (LNF) {
#pragma unroll
                for (int i = 0; i < TM; ++i) rs[i] = p.ln_rstd[min(mbase + 16 * i + li, p.M - 1)];
            }
            static_for<0, TM>([&](auto i_c) {
                constexpr int i = decltype(i_c)::value;
                if constexpr (LSRES) {
                    if (i + 1 < TM) load_res(i + 1, res[(i + 1) & 1]);
                }
                // ---- phase 1 ----------------------------------------------------------------------------------------
                float v[16];
                accs.template load16<i, grp>(v);
                if constexpr (LNF) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e] *= rs[i];
                }
                u32x4_t w0, w1;                                  // bf16 rounding point of the linear layer (/ GELU) output
                if constexpr (EGELU && table_gelu(VAR)) {
                    uint32_t g[8];
                    gelu_tab16(v, g, gelu_tab);
                    w0 = u32x4_t{g[0], g[1], g[2], g[3]};
                    w1 = u32x4_t{g[4], g[5], g[6], g[7]};
                } else {
                    if constexpr (EGELU) {
#pragma unroll
                        for (int e = 0; e < 16; ++e) v[e] = gelu_erf(rbf(v[e]));
                    }
                    w0.x = pack_bf2(v[0], v[1]);   w0.y = pack_bf2(v[2], v[3]);
                    w0.z = pack_bf2(v[4], v[5]);   w0.w = pack_bf2(v[6], v[7]);
                    w1.x = pack_bf2(v[8], v[9]);   w1.y = pack_bf2(v[10], v[11]);
                    w1.z = pack_bf2(v[12], v[13]); w1.w = pack_bf2(v[14], v[15]);
                }
                *(bf16x8_t*)(wr + (((2 * lg) ^ wkey) << 4)) = __builtin_bit_cast(bf16x8_t, w0);
                *(bf16x8_t*)(wr + (((2 * lg + 1) ^ wkey) << 4)) = __builtin_bit_cast(bf16x8_t, w1);
                // ---- phase 2 (DS operations of one wave execute in issue order: no barrier) ---------------------------
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int r = h * 8 + prow;
                    const u32x4_t t = __builtin_bit_cast(
                        u32x4_t, *(const bf16x8_t*)(stg + r * 128 + ((pslot ^ key_plain(r)) << 4)));
                    const int m = mbase + 16 * i + r;
                    if constexpr (!BUF) {
                        if (m >= p.M || nb2 >= p.N) continue;
                    }
                    size_t orow = (size_t)m;
                    u32x4_t o = t;
                    if constexpr (LSRES) {
                        const uint4 rr = res[i & 1][h];
                        const uint32_t rw[4] = {rr.x, rr.y, rr.z, rr.w};
                        const uint32_t tw[4] = {t.x, t.y, t.z, t.w};
                        uint32_t ow[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e)   // reference rounding points: linear -> bf16, *gamma -> bf16, +resid -> bf16
                            ow[e] = pack_bf2(lo_bf(rw[e]) + rbf(lo_bf(gamw[e]) * lo_bf(tw[e])),
                                             hi_bf(rw[e]) + rbf(hi_bf(gamw[e]) * hi_bf(tw[e])));
                        o = u32x4_t{ow[0], ow[1], ow[2], ow[3]};
                        if constexpr (STATS) {
                            // row statistics of the bf16 values just formed (what the consuming GEMM will read), 64 columns:
                            // 8 per lane by dot2c, then the row's 8 lanes (pslot = lane & 7) by xor 4, 2, 1.  N % 64 == 0 and the
                            // 8 lanes of a row share m, so the `continue` above never splits a reduction group.
                            typedef __bf16 bf16x2_hw __attribute__((ext_vector_type(2)));
                            float sm = 0.f, sq = 0.f;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const bf16x2_hw pr = __builtin_bit_cast(bf16x2_hw, ow[e]);
                                sm = __builtin_amdgcn_fdot2_f32_bf16(pr, __builtin_bit_cast(bf16x2_hw, 0x3f803f80u), sm, false);
                                sq = __builtin_amdgcn_fdot2_f32_bf16(pr, pr, sq, false);
                            }
                            sm += lane_xor<4>(sm); sq += lane_xor<4>(sq);
                            sm += lane_xor<2>(sm); sq += lane_xor<2>(sq);
                            sm += lane_xor<1>(sm); sq += lane_xor<1>(sq);
                            if (pslot == 0 && m < p.M && nbw < p.N) p.stat_part[(size_t)(nbw >> 6) * p.stat_ld + m] = make_float2(sm, sq);
                        }
                    } else if constexpr (EPI == FP_EPI_PATCH) {
                        const int b = m / p.P, pp = m - b * p.P;
                        orow = (size_t)b * p.npad + p.tok_off + pp;
                        const uint4 q = *(const uint4*)(p.pos + (size_t)pp * p.N + nb2);
                        const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
                        const uint32_t tw[4] = {t.x, t.y, t.z, t.w};
                        uint32_t ow[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            ow[e] = pack_bf2(lo_bf(tw[e]) + lo_bf(qw[e]), hi_bf(tw[e]) + hi_bf(qw[e]));
                        o = u32x4_t{ow[0], ow[1], ow[2], ow[3]};
                    }
                    if (FP_GEMM_DBG_BIT(p, 16) && o.x != 0x12345678u) continue;   // lab build only (gemm_dbg = 16): everything but the stores
                    if constexpr (BUF) __builtin_amdgcn_raw_buffer_store_b128(o, rsC, col_ok ? (16 * i + r) * ldc2 + nb2 * 2 : 0x7fffffff, 0, AUX);
                    else if constexpr (stream_io(VAR)) __builtin_nontemporal_store(o, (u32x4_t*)(p.C + orow * p.ldc + nb2));
                    else *(u32x4_t*)(p.C + orow * p.ldc + nb2) = o;
                }
            });
        });
    } else if constexpr (TM == 4) {
        auto& acc = accs.a;   // transposed stores: compiler-managed accumulators only
        // transposed V store, staged like the row-major epilogues with the roles swapped: a block is 16 FEATURES (rows,
        // lane li) x 64 TOKENS (lane lg owns 16 consecutive ones); phase 2 writes one full 128-B line of Vt[b,h,d,:]
        // (64 tokens of one feature) per 8 lanes.  Blocks never straddle a crop: npad and the tile origin are
        // multiples of 16 and a lane's 8-token chunk is 8-aligned.
        const int lane = lg * 16 + li;
        const int prow = lane >> 3, pslot = lane & 7;
        char* wr = stg + li * 128;
        const int wkey = key_plain(li);                        // slab_addr(li, slot) = wr + ((slot ^ wkey) << 4)
        const int m2 = m0 + wm * (16 * TM) + pslot * 8;        // phase-2 tokens of this lane (first of 8)
        const int b2 = m2 / p.npad, t2 = m2 - b2 * p.npad;
        float rt[LNF ? 16 : 1];                                // rstd of this lane's 16 consecutive tokens
        if constexpr (LNF) {
            const f32x4_t* rp = (const f32x4_t*)(p.ln_rstd + min(m0 + wm * (16 * TM) + lg * 16, p.M - 16));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4_t q = rp[j];
                rt[4 * j] = q[0]; rt[4 * j + 1] = q[1]; rt[4 * j + 2] = q[2]; rt[4 * j + 3] = q[3];
            }
        }
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int n1 = n0 + wn * (16 * TN) + 16 * i + li;
            float v[16];
            if constexpr (LNF) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[4 * j + r] = acc[i][j][r] * rt[4 * j + r];
            } else {
                const float bias = (p.bias && n1 < p.N) ? bf2f(p.bias[n1]) : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[4 * j + r] = acc[i][j][r] + bias;
            }
            u32x4_t w0, w1;
            w0.x = pack_bf2(v[0], v[1]);   w0.y = pack_bf2(v[2], v[3]);
            w0.z = pack_bf2(v[4], v[5]);   w0.w = pack_bf2(v[6], v[7]);
            w1.x = pack_bf2(v[8], v[9]);   w1.y = pack_bf2(v[10], v[11]);
            w1.z = pack_bf2(v[12], v[13]); w1.w = pack_bf2(v[14], v[15]);
            *(bf16x8_t*)(wr + (((2 * lg) ^ wkey) << 4)) = __builtin_bit_cast(bf16x8_t, w0);
            *(bf16x8_t*)(wr + (((2 * lg + 1) ^ wkey) << 4)) = __builtin_bit_cast(bf16x8_t, w1);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = h * 8 + prow;
                const u32x4_t t = __builtin_bit_cast(
                    u32x4_t, *(const bf16x8_t*)(stg + r * 128 + ((pslot ^ key_plain(r)) << 4)));
                const int n = n0 + wn * (16 * TN) + 16 * i + r;
                if (n >= p.N || m2 >= p.M) continue;
                u32x4_t* op = (u32x4_t*)(p.C + (((size_t)b2 * p.heads + (n >> 6)) * 64 + (n & 63)) * p.npad + t2);
                if constexpr (stream_io(VAR)) __builtin_nontemporal_store(t, op);
                else *op = t;
            }
        }
    } else {
        auto& acc = accs.a;
        // transposed V store (direct form, wave tiles taller than 64 tokens): lane owns, for each of its TN features, 4*TM consecutive tokens
        static_assert(!LNF, "the LN-folded V store exists for 64-token wave tiles only");
        constexpr int RUN = 4 * TM;
        static_assert(RUN % 16 == 0, "token runs are stored in 16-token groups");
#pragma unroll
        for (int i = 0; i < TN; ++i) {
            const int n = n0 + wn * (16 * TN) + 16 * i + li;
            if (n >= p.N) continue;
            const float bias = p.bias ? bf2f(p.bias[n]) : 0.f;
            const int h = n >> 6, d = n & 63;
#pragma unroll
            for (int half = 0; half < RUN / 16; ++half) {
                const int m16 = m0 + wm * (16 * TM) + lg * RUN + half * 16;
                if (m16 >= p.M) continue;
                const int b = m16 / p.npad, t = m16 - b * p.npad;
                float v[16];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[4 * j + r] = acc[i][half * 4 + j][r] + bias;
                uint4 o0, o1;
                o0.x = pack_bf2(v[0], v[1]);   o0.y = pack_bf2(v[2], v[3]);
                o0.z = pack_bf2(v[4], v[5]);   o0.w = pack_bf2(v[6], v[7]);
                o1.x = pack_bf2(v[8], v[9]);   o1.y = pack_bf2(v[10], v[11]);
                o1.z = pack_bf2(v[12], v[13]); o1.w = pack_bf2(v[14], v[15]);
                uint4* op = (uint4*)(p.C + (((size_t)b * p.heads + h) * 64 + d) * p.npad + t);
                op[0] = o0;
                op[1] = o1;
            }
        }
    }
}


// ---- software-pipelined row-major epilogue for ONE wave per SIMD (gemm_asm.hip) -------------------------------------------------
// Same arithmetic, rounding points and slab layout as epilogue_acc above — outputs are bit-identical — but scheduled for a lone in-order
// wave, which has nobody to hide an LDS round trip or a residual load behind: the wave owns TWO slabs; the slab reads of block b are
// issued, then phase 1 of block b+1 (accumulator reads, rstd / GELU, bf16 rounding, slab writes) runs while they are in flight, then
// block b is finished and stored; residual rows are requested two blocks ahead.  Rows past M and columns past N are handled by the
// buffer descriptors of the stores / residual loads (an out-of-range offset is dropped / reads zero), so there is no branch in the loop.
// Blocks are enumerated b = grp * TM + i (64-feature group, 16-row block).  Epilogues: BIAS, BIAS_GELU, BIAS_LS_RES, LN_BIAS, LN_GELU,
// LS_RES_STATS.
template <int BM, int BN, int WM, int WN, int EPI, int TC, int TR, class Acc>
__device__ __forceinline__ void epilogue_pipe(const FpGemmArgs& p, const Acc& accs, int m0, int n0, int wm, int wn, int li, int lg,
                                              char* stg2, const char* gelu_tab) {
    asm volatile("" : "+v"(li), "+v"(lg));
    constexpr bool LNF = FpEpiTraits<EPI>::LN;
    constexpr bool EGELU = FpEpiTraits<EPI>::GELU;
    constexpr bool LSRES = FpEpiTraits<EPI>::LSRES;
    constexpr bool STATS = FpEpiTraits<EPI>::STATS;
    static_assert(!FpEpiTraits<EPI>::TRANS && EPI != FP_EPI_PATCH, "row-major epilogues without the patch scatter");
    constexpr int TM = BM / WM / 16, TN = BN / WN / 16, NG = TN / 4, NB = TM * NG;
    static_assert(TN % 4 == 0 && TM == TC && TN == TR, "wave tile");
    const int lane = lg * 16 + li;
    const int prow = lane >> 3, pslot = lane & 7;
    const int wkey = key_plain(li);                        // slab_addr(li, slot) = wr + ((slot ^ wkey) << 4)
    const int mbase = m0 + wm * (16 * TM), nw0 = n0 + wn * (16 * TN);
    const int rows_left = max(p.M - mbase, 0);
    auto records = [&](int ld) { const unsigned long long b = (unsigned long long)rows_left * (unsigned)ld * 2ull; return (int)(b > 0x7fffffffull ? 0x7fffffffull : b); };
    const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc((void*)(p.C + (size_t)min(mbase, p.M) * p.ldc), 0, records(p.ldc), 0x00020000);
    __amdgpu_buffer_rsrc_t rsR = rsC;
    if constexpr (LSRES) rsR = __builtin_amdgcn_make_buffer_rsrc((void*)(p.resid + (size_t)min(mbase, p.M) * p.ldr), 0, records(p.ldr), 0x00020000);
    // per 64-feature group: this lane's phase-2 column (8 features), its byte offset in an output / residual row, LayerScale
    int colC[NG], colR[NG];
    uint32_t gamw[NG][4];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int nb2 = nw0 + g * 64 + pslot * 8;
        const bool ok = nb2 < p.N;
        colC[g] = ok ? nb2 * 2 : 0x7fffffff;      // an offset past num_records: the store is dropped
        colR[g] = colC[g];
        if constexpr (LSRES) {
            const uint4 g0 = *(const uint4*)(p.gamma + min(nb2, p.N - 8));
            gamw[g][0] = g0.x; gamw[g][1] = g0.y; gamw[g][2] = g0.z; gamw[g][3] = g0.w;
        }
    }
    float rs[LNF ? TM : 1];
    if constexpr (LNF) {
#pragma unroll
        for (int i = 0; i < TM; ++i) rs[i] = p.ln_rstd[min(mbase + 16 * i + li, p.M - 1)];
    }
    const int ldc2 = p.ldc * 2, ldr2 = p.ldr * 2;
    u32x4_t res[3][2];
    auto load_res = [&](auto bc) {
        constexpr int b = decltype(bc)::value, g = b / TM, i = b % TM;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = 16 * i + 8 * h + prow;
            res[b % 3][h] = __builtin_amdgcn_raw_buffer_load_b128(rsR, (colR[g] == 0x7fffffff) ? 0x7fffffff : r * ldr2 + colR[g], 0, 2);   // read once: streaming
        }
    };
    // phase 1 of block b in two halves: `p1_front` reads the accumulators, applies rstd, rounds to bf16 (or, for the table GELU, packs the
    // inputs and SENDS the 16 table gathers); `p1_back` (table GELU: waits for the gathers sent one block earlier) writes the slab.
    u32x4_t pw[3][2];
    GeluPending gp[EGELU ? 3 : 1];
    auto p1_front = [&](auto bc, bool send) {
        constexpr int b = decltype(bc)::value, g = b / TM, i = b % TM;
        float v[16];
        accs.template load16<i, g>(v);
        if constexpr (LNF) {
#pragma unroll
            for (int e = 0; e < 16; ++e) v[e] *= rs[i];
        }
        if constexpr (EGELU) {
            (void)send;
            gelu_tab16_issue(v, gp[b % 3]);
        } else {
            u32x4_t w0, w1;
            w0.x = pack_bf2(v[0], v[1]);   w0.y = pack_bf2(v[2], v[3]);
            w0.z = pack_bf2(v[4], v[5]);   w0.w = pack_bf2(v[6], v[7]);
            w1.x = pack_bf2(v[8], v[9]);   w1.y = pack_bf2(v[10], v[11]);
            w1.z = pack_bf2(v[12], v[13]); w1.w = pack_bf2(v[14], v[15]);
            pw[b % 3][0] = w0; pw[b % 3][1] = w1;
        }
    };
    auto p1_back = [&](auto bc) {
        constexpr int b = decltype(bc)::value;
        if constexpr (EGELU) {
            uint32_t q[8];
            gelu_tab16_finish(gp[b % 3], q, gelu_tab);
            pw[b % 3][0] = u32x4_t{q[0], q[1], q[2], q[3]};
            pw[b % 3][1] = u32x4_t{q[4], q[5], q[6], q[7]};
        }
        char* wr = stg2 + (b & 1) * EPI_STAGE_BYTES + li * 128;
        *(bf16x8_t*)(wr + (((2 * lg) ^ wkey) << 4)) = __builtin_bit_cast(bf16x8_t, pw[b % 3][0]);
        *(bf16x8_t*)(wr + (((2 * lg + 1) ^ wkey) << 4)) = __builtin_bit_cast(bf16x8_t, pw[b % 3][1]);
    };
    if constexpr (LSRES) { load_res(std::integral_constant<int, 0>{}); if constexpr (NB > 1) load_res(std::integral_constant<int, 1>{}); }
    // pipeline per block b:  back(b+1) -> slab reads of b -> front(b+2) (covers the reads; table GELU: its gathers fly until the next
    // block's back) -> finish and store b.  Slab b+1 was last read by block b-1, whose reads were consumed before its stores.
    p1_front(std::integral_constant<int, 0>{}, true);
    p1_back(std::integral_constant<int, 0>{});
    if constexpr (NB > 1) p1_front(std::integral_constant<int, 1>{}, true);
    static_for<0, NB>([&](auto bc) {
        constexpr int b = decltype(bc)::value, g = b / TM, i = b % TM;
        if constexpr (b + 1 < NB) p1_back(std::integral_constant<int, b + 1>{});
        u32x4_t t[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = h * 8 + prow;
            t[h] = __builtin_bit_cast(u32x4_t, *(const bf16x8_t*)(stg2 + (b & 1) * EPI_STAGE_BYTES + r * 128 + ((pslot ^ key_plain(r)) << 4)));
        }
        if constexpr (EGELU) {
            // the slab reads must have landed BEFORE the next gathers are sent: hipcc counts only its own LDS operations, so a wait it
            // places behind the (invisible) gathers would wait for them too
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t[0]), "+v"(t[1]) : : "memory");
        }
        if constexpr (b + 2 < NB) p1_front(std::integral_constant<int, b + 2>{}, true);
        if constexpr (LSRES && b + 2 < NB) load_res(std::integral_constant<int, b + 2>{});
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = 16 * i + 8 * h + prow;
            u32x4_t o = t[h];
            if constexpr (LSRES) {
                const u32x4_t rr = res[b % 3][h];
                const uint32_t rw[4] = {rr.x, rr.y, rr.z, rr.w};
                const uint32_t tw[4] = {t[h].x, t[h].y, t[h].z, t[h].w};
                uint32_t ow[4];
#pragma unroll
                for (int e = 0; e < 4; ++e)   // reference rounding points: linear -> bf16, *gamma -> bf16, +resid -> bf16
                    ow[e] = pack_bf2(lo_bf(rw[e]) + rbf(lo_bf(gamw[g][e]) * lo_bf(tw[e])),
                                     hi_bf(rw[e]) + rbf(hi_bf(gamw[g][e]) * hi_bf(tw[e])));
                o = u32x4_t{ow[0], ow[1], ow[2], ow[3]};
                if constexpr (STATS) {
                    typedef __bf16 bf16x2_hw __attribute__((ext_vector_type(2)));
                    float sm = 0.f, sq = 0.f;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bf16x2_hw pr = __builtin_bit_cast(bf16x2_hw, ow[e]);
                        sm = __builtin_amdgcn_fdot2_f32_bf16(pr, __builtin_bit_cast(bf16x2_hw, 0x3f803f80u), sm, false);
                        sq = __builtin_amdgcn_fdot2_f32_bf16(pr, pr, sq, false);
                    }
                    sm += lane_xor<4>(sm); sq += lane_xor<4>(sq);
                    sm += lane_xor<2>(sm); sq += lane_xor<2>(sq);
                    sm += lane_xor<1>(sm); sq += lane_xor<1>(sq);
                    const int m = mbase + r;
                    if (pslot == 0 && m < p.M && nw0 + g * 64 < p.N) p.stat_part[(size_t)((nw0 + g * 64) >> 6) * p.stat_ld + m] = make_float2(sm, sq);
                }
            }
            if (FP_GEMM_DBG_BIT(p, 16) && o.x != 0x12345678u) continue;   // lab build only (gemm_dbg = 16): everything but the stores
            __builtin_amdgcn_raw_buffer_store_b128(o, rsC, (colC[g] == 0x7fffffff) ? 0x7fffffff : r * ldc2 + colC[g], 0, 2);   // streaming full-line stores
        }
    });
}

// the HIP main loops' entry: accumulators in a compiler-managed register array
template <int BM, int BN, int WM, int WN, int EPI, int VAR, int TC, int TR>
__device__ __forceinline__ void epilogue(const FpGemmArgs& p, f32x4_t (&acc)[TC][TR], int m0, int n0, int wm, int wn,
                                         int li, int lg, char* stg, const char* gelu_tab = nullptr) {
    epilogue_acc<BM, BN, WM, WN, EPI, VAR, TC, TR>(p, RegAcc<TC, TR>{acc}, m0, n0, wm, wn, li, lg, stg, gelu_tab);
}

}  // namespace fp_gemm
