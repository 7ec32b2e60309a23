// The "dot64" row arithmetic of the retrieval, template-score and row-normalisation kernels (device only), stated once.
//
// Canonical arithmetic ("dot64"), shared with the tests' C oracle (fp_oracle.c) so indices AND scores are bit-exact:
//   lane l (0..63) owns elements (c*64 + l)*8 + e  (c = 0.., e = 0..7) of the D-vector,
//   p_l = fmaf chain over (c, e) ascending; s = xor-butterfly sum over offsets 32,16,8,4,2,1;
//   score = bf16_rne(s)  (the reference rounds bank@feature to bf16 before .float()/topk:
//   scripts/extract_proposals_ground.py:137-140).
// Ordering for top-k: score descending, then index ascending (torch.topk's tie order is unspecified;
// this is the documented canonical rule).
//
// F.normalize(x, dim=-1) on a bf16 row with the reference's rounding points:
//   n = max(bf16(sqrt(sum x^2)), eps), the sum in the dot64 order;  y = bf16(x / n).
//
// Everything here is a plain function on one wave's registers: NCH = ceil(D / 512) chunks of 8 elements per lane.  A kernel keeps
// its own schedule (what is requested ahead of which reduction); these are only the pieces it is made of.
#pragma once
#include "common.h"

#include <type_traits>

// element offset of lane `lane`'s 8-element slot in chunk c
__device__ __forceinline__ int d64_base(int c, int lane) { return (c * 64 + lane) * 8; }

// ---- loads --------------------------------------------------------------------------------------------------------------------
// 16-byte loads of the 16-byte-aligned row that starts `off` elements into `mat`, zero beyond D.
// FULL: D == NCH * 512, every slot is in range and the per-load test is dropped (bank scan).  NT: non-temporal (streamed once).
// The shapes below are the ones the compiler keeps the kernels' schedules with (profiles/row_kernels_refactor.md): the address is one
// sum, the load a plain dereference into a reference (a helper RETURNING the uint4 made the scan wait for a chunk right behind its
// fetch), and `live` stays out of the rows' path.
template <bool FULL = false, bool NT = false>
__device__ __forceinline__ void d64_load_chunk(uint4& dst, const bf16_t* mat, size_t off, int c, int D, int lane) {
    const int base = d64_base(c, lane);
    if constexpr (NT) {
        typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (FULL || base < D) v = __builtin_nontemporal_load((const u32x4_t*)(mat + off + base));
        dst = make_uint4(v.x, v.y, v.z, v.w);
    } else {
        dst = (FULL || base < D) ? *(const uint4*)(mat + off + base) : make_uint4(0, 0, 0, 0);
    }
}
// ... of a row that exists only when `live` (a query or a template past the last one): zero otherwise
template <bool FULL = false, bool NT = false>
__device__ __forceinline__ void d64_load_chunk(uint4& dst, const bf16_t* mat, size_t off, int c, int D, int lane, bool live) {
    if (live) d64_load_chunk<FULL, NT>(dst, mat, off, c, D, lane);
    else dst = make_uint4(0, 0, 0, 0);
}
template <int NCH, bool FULL = false, bool NT = false>
__device__ __forceinline__ void d64_load(uint4 (&dst)[NCH], const bf16_t* mat, size_t off, int D, int lane) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) d64_load_chunk<FULL, NT>(dst[c], mat, off, c, D, lane);
}
template <int NCH, bool FULL = false, bool NT = false>
__device__ __forceinline__ void d64_load(uint4 (&dst)[NCH], const bf16_t* mat, size_t off, int D, int lane, bool live) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) d64_load_chunk<FULL, NT>(dst[c], mat, off, c, D, lane, live);
}
// two rows of one length under ONE test per chunk: both requests of a chunk leave from the same branch, neither waits for the other
// (template_dots_kernel; two d64_load calls compile to a branch per request with a wait inside the first: +2 % on the kernel, measured)
template <int NCH>
__device__ __forceinline__ void d64_load2(uint4 (&a)[NCH], const bf16_t* row_a, uint4 (&b)[NCH], const bf16_t* row_b, int D, int lane) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        a[c] = make_uint4(0, 0, 0, 0);
        b[c] = make_uint4(0, 0, 0, 0);
        if (d64_base(c, lane) < D) {
            d64_load_chunk<true>(a[c], row_a, 0, c, D, lane);
            d64_load_chunk<true>(b[c], row_b, 0, c, D, lane);
        }
    }
}
// eight bf16 in memory order -> eight floats (lo_bf / hi_bf of each word)
__device__ __forceinline__ void d64_unpack(const uint4& w, float (&x)[8]) {
    const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) { x[2 * e] = lo_bf(u[e]); x[2 * e + 1] = hi_bf(u[e]); }
}
template <int NCH>
__device__ __forceinline__ void d64_unpack(const uint4 (&w)[NCH], float (&x)[NCH][8]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) d64_unpack(w[c], x[c]);
}
// the same slot of a row that may be misaligned: element-wise loads, zero beyond D
__device__ __forceinline__ void d64_load_elems(float (&x)[8], const bf16_t* row, int base, int D) {
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = base < D ? bf2f(row[base + e]) : 0.f;
}
template <int NCH>
__device__ __forceinline__ void d64_load_elems(float (&x)[NCH][8], const bf16_t* row, int D, int lane) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) d64_load_elems(x[c], row, d64_base(c, lane), D);
}

// ---- lane partials: the fmaf chain over e ascending (callers walk c ascending); the accumulator goes in and comes out -----------
__device__ __forceinline__ float d64_sumsq(const float (&x)[8], float acc) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = __fmaf_rn(x[e], x[e], acc);
    return acc;
}
__device__ __forceinline__ float d64_sumsq(const uint4& w, float acc) {
    float x[8];
    d64_unpack(w, x);
    return d64_sumsq(x, acc);
}
__device__ __forceinline__ float d64_dot(const float (&x)[8], const float (&q)[8], float acc) {
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = __fmaf_rn(x[e], q[e], acc);
    return acc;
}
__device__ __forceinline__ float d64_dot(const uint4& w, const float (&q)[8], float acc) {
    float x[8];
    d64_unpack(w, x);
    return d64_dot(x, q, acc);
}
template <int NCH>
__device__ __forceinline__ float d64_sumsq(const float (&x)[NCH][8], float acc) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) acc = d64_sumsq(x[c], acc);
    return acc;
}

// ---- F.normalize ----------------------------------------------------------------------------------------------------------------
// ss: the wave_sum of the lanes' d64_sumsq partials
__device__ __forceinline__ float d64_row_norm(float ss) { return fmaxf(rbf(fp_sqrt_rn(ss)), 1e-12f); }

// bf16(x / n), two forms with the same bits.  The normalisers store the quotient and are bound by memory: they take the IEEE division.
__device__ __forceinline__ bf16_t d64_div_bf(float x, float n) { return f2bf(__fdiv_rn(x, n)); }
// The scorers feed it to a dot product and were VALU-bound on the division's ~12-instruction expansion: r = v_rcp_f32(n) (1 ulp), one
// residual correction step puts q within 1 fp32 ulp of the correctly rounded quotient, and that can only change the
// bf16 rounding when q's discarded 16 bits sit next to the midpoint 0x8000 — only those lanes (9 in 65536) take the exact
// division.  Bit-identical to rbf(__fdiv_rn(x, n)) (what the oracle computes).
__device__ __forceinline__ float div_rbf(float x, float n, float r) {
    float q = x * r;
    const float e = __fmaf_rn(-q, n, x);
    q = __fmaf_rn(e, r, q);
    if ((__float_as_uint(q) & 0xffffu) - 0x7ffcu <= 8u) q = __fdiv_rn(x, n);
    return rbf(q);
}

// bf16( normalize(x) . q ) of a row held unpacked in registers
template <int NCH>
__device__ __forceinline__ float d64_normed_dot(const float (&x)[NCH][8], const float (&q)[NCH][8]) {
    const float nrm = d64_row_norm(wave_sum(d64_sumsq<NCH>(x, 0.f)));
    const float rinv = __builtin_amdgcn_rcpf(nrm);
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = __fmaf_rn(div_rbf(x[c][e], nrm, rinv), q[c][e], acc);
    return rbf(wave_sum(acc));
}

// normalize(x) of a lane's slot(s), stored with one 16-byte store each (pack_bf2 of two quotients is d64_div_bf of each: one
// v_cvt_pk_bf16_f32).  n = d64_row_norm(..).  `dst` is the slot / the row; slots beyond D are not written.
__device__ __forceinline__ void d64_norm_store(const uint4& w, float n, bf16_t* dst) {
    float x[8];
    d64_unpack(w, x);
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = pack_bf2(__fdiv_rn(x[2 * e], n), __fdiv_rn(x[2 * e + 1], n));
    *(uint4*)dst = make_uint4(o[0], o[1], o[2], o[3]);
}
template <int NCH>
__device__ __forceinline__ void d64_norm_store(const uint4 (&w)[NCH], float n, bf16_t* row, int D, int lane) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int base = d64_base(c, lane);
        if (base < D) d64_norm_store(w[c], n, row + base);
    }
}

// ---- host: nch = cdiv(D, 512) in 1..3 -> the kernels' NCH template argument: f(std::integral_constant<int, NCH>) ------------------
template <class F>
static inline void fp_nch_dispatch(int nch, F&& f) {
    if (nch == 1) f(std::integral_constant<int, 1>{});
    else if (nch == 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, 3>{});
}
