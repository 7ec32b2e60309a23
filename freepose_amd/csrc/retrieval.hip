// Retrieval kernels (K10, K12, K13 of SURVEY.md §2.3), gfx950 only.  All HBM-bound byte/row streaming:
// coalesced 16-byte loads, one wave per row, wave-shuffle reductions, no MFMA.
// The canonical "dot64" arithmetic and the (score desc, index asc) order they share with oracle/fp_oracle.c: dot64.h.
#include "internal.h"
#include "dot64.h"

#include <stdlib.h>

namespace {

__device__ __forceinline__ uint32_t score_key16(float s_bf16_rounded) {
    const uint32_t b = __float_as_uint(s_bf16_rounded) >> 16;
    return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float key16_to_float(uint32_t k) {
    const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
    return __uint_as_float(b << 16);
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] = f2bf(x[i]);
}

// ---------------------------------------------------------------------------------------------
// bank scan: keys[q, r] = sortable16( bf16( bank[r] . query[q] ) )
template <int NCH, int QT, bool FULL>   // FULL: D == NCH * 512, every lane's 8-element slot is in range (no per-load test)
__global__ __launch_bounds__(256) void bank_scan_kernel(const bf16_t* __restrict__ bank,
                                                        const bf16_t* __restrict__ queries,
                                                        uint16_t* __restrict__ keys, int N, int D, int q_begin,
                                                        int Q, int ldk) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwave = (gridDim.x * blockDim.x) >> 6;
    // Balanced partition: wave w owns a contiguous run of floor(N/nwave) (+1 for the first N%nwave waves) rows, streamed in
    // chunks of RU rows (RU x 2 KB in flight) with the next chunk requested before the current one is reduced.  The host
    // picks the grid (2..8 workgroups per CU) that leaves the smallest remainder, e.g. 3 per CU for N = 46 037 (0.1 %).
    constexpr int RU = 4;
    const int base_rows = N / nwave, rem = N - base_rows * nwave;
    const int r_begin = wave * base_rows + min(wave, rem);
    const int r_end = r_begin + base_rows + (wave < rem ? 1 : 0);
    uint4 bufA[RU][NCH], bufB[RU][NCH];
    float qv[QT][NCH][8];                 // the queries, unpacked (filled in after the first row requests are out)
    auto fetch = [&](uint4 (&dst)[RU][NCH], int r0) {
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            if (r0 + u >= r_end) break;      // wave-uniform: rows past the run are neither fetched nor stored
            d64_load<NCH, FULL>(dst[u], bank, (size_t)(r0 + u) * D, D, lane);
        }
    };
    auto reduce_chunk = [&](const uint4 (&raw)[RU][NCH], int r0) {
        float acc[RU][QT];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
#pragma unroll
            for (int q = 0; q < QT; ++q) acc[u][q] = 0.f;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                // d64_dot's chain, one word (two steps) of each of the QT queries at a time: the words are unpacked as they are
                // consumed (unpacking the slot first, as d64_unpack does, made the compiler wait for a chunk right behind its fetch)
                const uint32_t w[4] = {raw[u][c].x, raw[u][c].y, raw[u][c].z, raw[u][c].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x0 = lo_bf(w[e]), x1 = hi_bf(w[e]);
#pragma unroll
                    for (int q = 0; q < QT; ++q) {
                        acc[u][q] = __fmaf_rn(x0, qv[q][c][2 * e], acc[u][q]);
                        acc[u][q] = __fmaf_rn(x1, qv[q][c][2 * e + 1], acc[u][q]);
                    }
                }
            }
        }
        // the chunk's four rows are reduced together; 16-lane row u of the wave ends up with row (r0 + u)'s dot product
        static_assert(RU == 4, "wave_sum4 reduces four rows");
        const int urow = lane >> 4;
#pragma unroll
        for (int q = 0; q < QT; ++q) {
            const float sdot = wave_sum4(acc[0][q], acc[1][q], acc[2][q], acc[3][q]);
            if ((lane & 15) == 0 && r0 + urow < r_end && q_begin + q < Q)
                keys[(size_t)(q_begin + q) * ldk + r0 + urow] = (uint16_t)score_key16(rbf(sdot));
        }
    };
    // two chunk buffers used alternately (no register copy at the hand-over): B is requested before A is reduced, etc.
    // The first two chunks are requested BEFORE the queries: a wave owns only ~9 rows of the 46 037-row bank (5 120 waves), so the
    // kernel is a start-up transient, and queries-then-rows cost two dependent memory round trips where one suffices (r03: the
    // cold-bank pass went 19.3 -> see profiles/r03_ab.md).
    if (r_begin < r_end) fetch(bufA, r_begin);
    if (r_begin + RU < r_end) fetch(bufB, r_begin + RU);
#pragma unroll
    for (int q = 0; q < QT; ++q) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {      // chunk by chunk: each is unpacked where it is loaded
            uint4 qw;
            d64_load_chunk<FULL>(qw, queries, (size_t)(q_begin + q) * D, c, D, lane, q_begin + q < Q);
            d64_unpack(qw, qv[q][c]);
        }
    }
    for (int r0 = r_begin; r0 < r_end; r0 += 2 * RU) {
        if (r0 != r_begin && r0 + RU < r_end) fetch(bufB, r0 + RU);
        reduce_chunk(bufA, r0);
        if (r0 + RU < r_end) {
            if (r0 + 2 * RU < r_end) fetch(bufA, r0 + 2 * RU);
            reduce_chunk(bufB, r0 + RU);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// exact top-k of 16-bit keys with (key desc, index asc) order: two-level radix select + ordered
// compaction + bitonic sort of the k survivors.  One workgroup per query.
constexpr int SEL_T = 1024;
constexpr int KMAX = 1024;

__device__ __forceinline__ int block_excl_scan(int v, int* sh, int& total) {
    // sh: SEL_T ints.  simple Hillis-Steele over waves: wave scan + wave totals
    // all sums are carried in unsigned arithmetic: callers pack two 16-bit counts into one word, and the upper one reaches
    // 2^15 and beyond on degenerate rows (46 037 equal keys), which would overflow a signed add
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned x = (unsigned)v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned y = (unsigned)__shfl_up((int)x, off, 64);
        if (lane >= off) x += y;
    }
    __syncthreads();
    if (lane == 63) sh[w] = (int)x;
    __syncthreads();
    unsigned base = 0, tot = 0;
    for (int i = 0; i < SEL_T / 64; ++i) {
        const unsigned t = (unsigned)sh[i];
        if (i < w) base += t;
        tot += t;
    }
    total = (int)tot;
    __syncthreads();
    return (int)(base + x - (unsigned)v);
}

// ---- candidates: (key desc, index asc) as ONE descending order of distinct 64-bit composites ------------------------------------
// high word = key, low word = cand_flip(index): a smaller index is a larger composite; the flip is its own inverse (pack and decode)
__device__ __forceinline__ int cand_flip(int i) { return 0x7fffffff - i; }
__device__ __forceinline__ unsigned long long cand_pack(uint32_t key, int i) {
    return ((unsigned long long)key << 32) | (unsigned)cand_flip(i);
}
__device__ __forceinline__ int cand_index(unsigned long long c) { return cand_flip((int)(unsigned)(c & 0xffffffffu)); }
// candidate c of query q is the rank-th best: its score (16-bit key) and bank row
__device__ __forceinline__ void cand_emit(unsigned long long c, int q, int k, int rank, int idx_offset, float* out_scores,
                                          int* out_idx) {
    out_scores[(size_t)q * k + rank] = key16_to_float((uint32_t)(c >> 32));
    out_idx[(size_t)q * k + rank] = idx_offset + cand_index(c);
}
// one key of the ordered compaction (index order): all keys > T take slots [0, ngt), the first need_eq keys == T the slots after them
__device__ __forceinline__ void cand_place(unsigned long long* cand, int key, int i, int T, int ngt, int need_eq, int& og, int& oe) {
    if (key > T) cand[og++] = cand_pack(key, i);
    else if (key == T) { if (oe < need_eq) cand[ngt + oe] = cand_pack(key, i); ++oe; }
}
// in-place bitonic sort of a[0, n2) in LDS, descending; n2 a power of two; ends on a barrier
template <typename T>
__device__ __forceinline__ void lds_bitonic_desc(T* a, int n2, int tid, int nthreads) {
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < n2; i += nthreads) {
                const int j = i ^ stride;
                if (j > i) {
                    const bool desc = ((i & size) == 0);
                    const T x = a[i], y = a[j];
                    if ((x < y) == desc) { a[i] = y; a[j] = x; }
                }
            }
            __syncthreads();
        }
}
// the k survivors of a select: pad to a power of two, sort, emit in order
__device__ __forceinline__ void cand_sort_emit(unsigned long long* cand, int q, int k, int tid, int idx_offset, float* out_scores,
                                               int* out_idx) {
    int n2 = 1;
    while (n2 < k) n2 <<= 1;
    for (int i = k + tid; i < n2; i += SEL_T) cand[i] = 0ull;
    __syncthreads();
    lds_bitonic_desc(cand, n2, tid, SEL_T);
    for (int i = tid; i < k; i += SEL_T) cand_emit(cand[i], q, k, i, idx_offset, out_scores, out_idx);
}
// rank sort of n <= SEL_T candidates: they are distinct 64-bit values, so a candidate's rank is the number of larger ones (broadcast
// LDS reads); the best k are emitted
__device__ __forceinline__ void rank_sort_emit(const unsigned long long* cand, int n, int q, int k, int tid, int idx_offset,
                                               float* out_scores, int* out_idx) {
    if (tid < n) {
        const unsigned long long mine = cand[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += cand[j] > mine;
        if (rank < k) cand_emit(mine, q, k, rank, idx_offset, out_scores, out_idx);
    }
}

// LDSKEYS: the query's whole key row (N x 2 B; 92 KB for the 46 037-row bank) is staged into LDS once with coalesced loads
// and every later pass (two histograms, the ordered compaction's count and write sweeps) reads LDS — the global-read form
// spent its 54 us in four latency-bound sweeps, two of them with a 90-byte stride between neighbouring threads.
template <bool LDSKEYS>
__global__ __launch_bounds__(SEL_T) void topk_select_kernel(const uint16_t* __restrict__ keys, int ldk, int N, int k,
                                                            int idx_offset, float* __restrict__ out_scores,
                                                            int* __restrict__ out_idx) {
    extern __shared__ uint16_t lkeys[];   // [ldk] when LDSKEYS (rows are padded to 8 keys: 16-byte staging loads)
    __shared__ int hist[256];
    __shared__ int sh[SEL_T / 64 + 2];
    __shared__ int s_hi, s_T, s_gt;
    __shared__ unsigned long long cand[KMAX];
    const int q = blockIdx.x, tid = threadIdx.x;
    const uint16_t* kq = keys + (size_t)q * ldk;
    if constexpr (LDSKEYS) {
        const uint4* src = (const uint4*)kq;
        uint4* dst = (uint4*)lkeys;
        for (int i = tid; i < ldk / 8; i += SEL_T) dst[i] = src[i];   // pad keys (>= N) are never read below
        __syncthreads();
        kq = lkeys;
    }
    const int per = (N + SEL_T - 1) / SEL_T;
    const int lo = tid * per, hi = min(lo + per, N);

    // pass 1: histogram of the high byte
    for (int i = tid; i < 256; i += SEL_T) hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += SEL_T) atomicAdd(&hist[kq[i] >> 8], 1);
    __syncthreads();
    if (tid == 0) {
        int c = 0, b = 255;
        for (; b >= 0; --b) { if (c + hist[b] >= k) break; c += hist[b]; }
        s_hi = b; s_gt = c;  // c keys strictly above bin b
    }
    __syncthreads();
    const int hb = s_hi;
    __syncthreads();
    // pass 2: histogram of the low byte inside bin hb
    for (int i = tid; i < 256; i += SEL_T) hist[i] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += SEL_T) { const int key = kq[i]; if ((key >> 8) == hb) atomicAdd(&hist[key & 255], 1); }
    __syncthreads();
    if (tid == 0) {
        int c = s_gt, b = 255;
        for (; b >= 0; --b) { if (c + hist[b] >= k) break; c += hist[b]; }
        s_T = (hb << 8) | b; s_gt = c;  // c keys strictly greater than T
    }
    __syncthreads();
    const int T = s_T, ngt = s_gt, need_eq = k - ngt;
    // ordered compaction (index order): first all > T, then the first need_eq == T
    int cg = 0, ce = 0;
    for (int i = lo; i < hi; ++i) { const int key = kq[i]; cg += key > T; ce += key == T; }
    int tot;
    int og = block_excl_scan(cg, sh, tot);
    int oe = block_excl_scan(ce, sh, tot);
    for (int i = lo; i < hi; ++i) cand_place(cand, kq[i], i, T, ngt, need_eq, og, oe);
    // pad to a power of two and bitonic-sort descending on (key, -index)
    cand_sort_emit(cand, q, k, tid, idx_offset, out_scores, out_idx);
}

// ---- register-resident select (N <= 48 * SEL_T keys per query) ---------------------------------------------------------------
// The two-level histogram above serialises on LDS atomics when the keys are skewed — and bf16 cosine scores are: with an
// anisotropic bank nearly every key shares one high byte, so each ds_add hits one address 64 ways (43 us for 46 037 keys).
// Here no atomics are used at all: a thread keeps its 2*MAXW consecutive keys packed in MAXW registers and the exact k-th
// largest key T is found by COUNTING,
//   1. per-thread maximum; L = the k-th largest of the SEL_T maxima (bit-wise binary search over 1024 values: one compare per
//      thread and iteration).  At least k keys are >= L, so T >= L; G = the block maximum bounds T from above;
//   2. binary search for T in [L, G] with exact block-wide counts of keys >= mid (packed 16-bit saturating subtract / min /
//      add: 3 VALU per two keys); [L, G] spans a handful of bf16 values, so this takes ~4-6 iterations;
//   3. ordered compaction (all keys > T, then the first k - #greater keys == T in index order) and the bitonic sort of the k
//      survivors, as before.  Same total order (key desc, index asc) -> bit-identical results.
typedef unsigned short u16x2_t __attribute__((ext_vector_type(2)));

constexpr int SEL_W = 24;                 // packed words per thread: thread t owns keys [48 t, 48 t + 48)
constexpr int SEL_CAP = SEL_T * 2 * SEL_W;   // 49 152 keys

__global__ __launch_bounds__(SEL_T) void topk_select_reg_kernel(const uint16_t* __restrict__ keys, int ldk, int N, int k,
                                                                int idx_offset, float* __restrict__ out_scores,
                                                                int* __restrict__ out_idx) {
    extern __shared__ uint16_t lkeys[];   // [SEL_CAP] staged key row, zero beyond N
    __shared__ int slots[8][SEL_T / 64];  // per-iteration wave partials (one barrier per block-wide count)
    __shared__ unsigned short smax[SEL_T];
    __shared__ int sh[SEL_T / 64 + 2];
    __shared__ unsigned long long cand[KMAX];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint16_t* kq = keys + (size_t)q * ldk;
    {
        // all six 16-byte loads of a thread are issued before the first is stored: a load -> store loop pays the full memory
        // latency per iteration (the key row was just written by the scan kernel: it comes from HBM / MALL, not from this XCD's L2)
        const uint4* src = (const uint4*)kq;
        uint4* dst = (uint4*)lkeys;
        const int n16 = N >> 3;                      // whole 16-byte groups inside the row
        constexpr int NLD = SEL_CAP / 8 / SEL_T;     // 6
        uint4 v[NLD];
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + j * SEL_T;
            v[j] = i < n16 ? src[i] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int j = 0; j < NLD; ++j) dst[tid + j * SEL_T] = v[j];
        __syncthreads();
        if (tid < 8) { const int i = (n16 << 3) + tid; if (i < N) lkeys[i] = kq[i]; }   // the ragged tail of the row
    }
    __syncthreads();
    uint32_t w[SEL_W];
    {
        const uint4* lw = (const uint4*)lkeys + (size_t)tid * (SEL_W / 4);
#pragma unroll
        for (int j = 0; j < SEL_W / 4; ++j) {
            const uint4 v = lw[j];
            w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w;
        }
    }
    const int lo = tid * 2 * SEL_W, hi = min(lo + 2 * SEL_W, N);

    // ---- 1. maxima: every wave finds L (k-th largest thread maximum) and G (largest) redundantly from the LDS copy ----------
    uint32_t m2 = 0u;
#pragma unroll
    for (int j = 0; j < SEL_W; ++j) m2 = pk_max_u16(m2, w[j]);
    smax[tid] = (unsigned short)max(m2 & 0xffffu, m2 >> 16);
    __syncthreads();
    uint32_t mw[SEL_T / 128];                          // this lane's 16 maxima, packed
    {
        const uint4* sm = (const uint4*)smax + lane * 2;
        const uint4 a = sm[0], b = sm[1];
        mw[0] = a.x; mw[1] = a.y; mw[2] = a.z; mw[3] = a.w; mw[4] = b.x; mw[5] = b.y; mw[6] = b.z; mw[7] = b.w;
    }
    const uint32_t ones = 0x00010001u;
    auto pk_count_ge = [&](const uint32_t* v, int n, int c) -> int {   // halves of v[0..n) that are >= c (c >= 1)
        const uint32_t cc = (uint32_t)(c - 1) * 0x00010001u;
        uint32_t acc = 0u;
#pragma unroll
        for (int j = 0; j < n; ++j) acc = pk_add_u16(acc, pk_min_u16(pk_sub_sat_u16(v[j], cc), ones));
        return (int)(acc & 0xffffu) + (int)(acc >> 16);
    };
    uint32_t g2 = 0u;
#pragma unroll
    for (int j = 0; j < SEL_T / 128; ++j) g2 = pk_max_u16(g2, mw[j]);
    const int G = wave_max_i((int)max(g2 & 0xffffu, g2 >> 16));
    int L = 0;
    for (int bit = 15; bit >= 0; --bit) {
        const int c = L | (1 << bit);
        if (c > G) continue;
        if (wave_sum_i(pk_count_ge(mw, SEL_T / 128, c)) >= k) L = c;
    }
    // ---- 1b. fast path: every key >= L is a candidate (at least k of them; typically k .. 2k).  If they fit the candidate buffer
    // the answer is a rank sort of their (key, index) composites — distinct 64-bit values whose descending order IS the canonical
    // (key desc, index asc) order — and no threshold search is needed.  Tie-heavy rows (more than KMAX keys >= L) take the
    // counting search below.
    {
        unsigned long long gem = 0ull;               // bit b: this thread's key lo + b is >= max(L, 1) (pads are 0)
        const uint32_t cc = (uint32_t)(max(L, 1) - 1) * 0x00010001u;
#pragma unroll
        for (int j = 0; j < SEL_W; ++j) {
            const uint32_t d = pk_min_u16(pk_sub_sat_u16(w[j], cc), ones);
            gem |= (unsigned long long)((d & 1u) | ((d >> 15) & 2u)) << (2 * j);
        }
        int M;
        int off = block_excl_scan(__popcll(gem), sh, M);
        if (M <= KMAX) {
            while (gem) {
                const int b = __ffsll((long long)gem) - 1;
                gem &= gem - 1;
                const int i = lo + b;
                cand[off++] = cand_pack(lkeys[i], i);
            }
            __syncthreads();
            rank_sort_emit(cand, M, q, k, tid, idx_offset, out_scores, out_idx);
            return;
        }
    }
    // ---- 2. exact k-th largest key T in [L, G]: block-wide counts, one barrier each ----------------------------------------
    int it = 0;
    auto block_count_ge = [&](int c) -> int {
        const int part = wave_sum_i(pk_count_ge(w, SEL_W, c));
        int* sl = slots[it & 7];
        ++it;
        if (lane == 0) sl[wv] = part;
        __syncthreads();
        int t = 0;
#pragma unroll
        for (int i = 0; i < SEL_T / 64; ++i) t += sl[i];
        return t;
    };
    int tlo = L, thi = G;                            // invariant: #keys >= tlo is >= k (L = 0 counts every real key: k <= N)
    while (tlo < thi) {
        const int mid = (tlo + thi + 1) >> 1;
        if (block_count_ge(mid) >= k) tlo = mid; else thi = mid - 1;
    }
    const int T = tlo;
    const int ngt = T >= 65535 ? 0 : block_count_ge(T + 1);
    const int need_eq = k - ngt;
    // ---- 3. ordered compaction (index order): first all > T, then the first need_eq == T -----------------------------------
    int cg = 0, ce = 0;
#pragma unroll
    for (int j = 0; j < SEL_W; ++j) {
        const int i0 = lo + 2 * j;
        const int k0 = (int)(w[j] & 0xffffu), k1 = (int)(w[j] >> 16);
        if (i0 < hi) { cg += k0 > T; ce += k0 == T; }
        if (i0 + 1 < hi) { cg += k1 > T; ce += k1 == T; }
    }
    int tot;
    // both counts stay below 65 536 (a row holds <= 49 152 keys): one unsigned scan carries the two
    const unsigned both = (unsigned)block_excl_scan((int)((unsigned)cg | ((unsigned)ce << 16)), sh, tot);
    int og = (int)(both & 0xffffu), oe = (int)(both >> 16);
#pragma unroll
    for (int j = 0; j < SEL_W; ++j) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = lo + 2 * j + h;
            if (i >= hi) continue;
            cand_place(cand, h ? (int)(w[j] >> 16) : (int)(w[j] & 0xffffu), i, T, ngt, need_eq, og, oe);
        }
    }
    __syncthreads();
    if (k <= 256) rank_sort_emit(cand, k, q, k, tid, idx_offset, out_scores, out_idx);   // the k candidates ARE the answer: order them
    else cand_sort_emit(cand, q, k, tid, idx_offset, out_scores, out_idx);
}

// merge C candidates (score f32 holding a bf16 value, global idx) per query down to k, same ordering
__global__ __launch_bounds__(1024) void topk_merge_kernel(const float* __restrict__ cs, const int* __restrict__ ci,
                                                           int C, int k, float* __restrict__ out_scores,
                                                           int* __restrict__ out_idx) {
    extern __shared__ unsigned long long mc[];
    const int q = blockIdx.x, tid = threadIdx.x;
    int n2 = 1;
    while (n2 < C) n2 <<= 1;
    for (int i = tid; i < n2; i += blockDim.x) {
        unsigned long long v = 0ull;
        if (i < C) {
            const float s = cs[(size_t)q * C + i];
            // full 32-bit sortable key (scores are bf16 values, but keep it generic)
            uint32_t b = __float_as_uint(s);
            b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
            v = cand_pack(b, ci[(size_t)q * C + i]);
        }
        mc[i] = v;
    }
    __syncthreads();
    lds_bitonic_desc(mc, n2, tid, blockDim.x);
    for (int i = tid; i < k; i += blockDim.x) {
        const unsigned long long c = mc[i];
        uint32_t b = (uint32_t)(c >> 32);
        b = (b & 0x80000000u) ? (b & 0x7fffffffu) : ~b;
        out_scores[(size_t)q * k + i] = __uint_as_float(b);
        out_idx[(size_t)q * k + i] = cand_index(c);
    }
}

// ---------------------------------------------------------------------------------------------
// K13 patchwise template score (src/pipeline/estimators/pose_estimator.py:85-88,
// online_pose_estimator.py:68-79) with the reference's bf16 rounding points:
//   tn = bf16(t / max(bf16(||t||), eps)) per patch row;  d[t,p] = bf16( tn . qn[p] );
//   score[t] = bf16( (sum_p d[t,p]) / P )
// qn is the already-normalised (or, frame-0 quirk, raw) query [P, D]; weights optional [T,P] f32
// (mask_scores variant: score = sum(d*w)/sum(w)).  The normalise-then-dot of one row is dot64.h's d64_normed_dot (div_rbf).
template <int NCH>
__global__ __launch_bounds__(256) void template_dots_kernel(const bf16_t* __restrict__ tmpl,
                                                            const bf16_t* __restrict__ qn, float* __restrict__ dots,
                                                            int T, int P, int D) {
    const int lane = threadIdx.x & 63;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long nwave = ((long)gridDim.x * blockDim.x) >> 6;
    const long rows = (long)T * P;
    // the row a wave will process NEXT is requested before the current one is reduced: two rows (4 KB) in flight per wave
    uint4 na[NCH], nb[NCH];
    auto fetch = [&](long r) { d64_load2<NCH>(na, tmpl + (size_t)r * D, nb, qn + (size_t)(r % P) * D, D, lane); };
    if (wave < rows) fetch(wave);
    for (long r = wave; r < rows; r += nwave) {
        float x[NCH][8], qq[NCH][8];
        uint4 ca[NCH], cb[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) { ca[c] = na[c]; cb[c] = nb[c]; }
        if (r + nwave < rows) fetch(r + nwave);
        d64_unpack(ca, x);
        d64_unpack(cb, qq);
        const float d = d64_normed_dot<NCH>(x, qq);
        if (lane == 0) dots[r] = d;
    }
}

// Pre-normalised template store: the reference normalises the cached [T,P,D] tensor on every call
// (pose_estimator.py:85-88); F.normalize of a bf16 tensor IS a bf16 tensor, so storing tn once (fp_l2_normalize when the
// features enter the cache) is bit-identical to the reference's intermediate, and the scorer becomes a streaming dot:
//   d[t,p] = bf16( tn[t,p,:] . qn[p,:] )   in the canonical dot64 order (same chain as template_dots_kernel).
// A wave owns ONE patch index p and walks templates t = t0, t0 + TS, ...: its query row stays unpacked in registers (no
// second load stream), template rows (2 KB, full lines) are requested two ahead of the one being reduced.
template <int NCH>
__global__ __launch_bounds__(256) void template_dots_normed_kernel(const bf16_t* __restrict__ tn, const bf16_t* __restrict__ qn,
                                                                   float* __restrict__ dots, int T, int P, int D, int TS) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)(((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const int pidx = wave / TS, t0 = wave % TS;
    if (pidx >= P) return;
    float qq[NCH][8];
    {
        uint4 b[NCH];
        d64_load<NCH>(b, qn, (size_t)pidx * D, D, lane);
        d64_unpack(b, qq);
    }
    const size_t tstride = (size_t)P * D;
    const bf16_t* row = tn + (size_t)pidx * D;
    auto fetch = [&](int t, uint4 (&dst)[NCH]) { d64_load<NCH, false, true>(dst, row, (size_t)t * tstride, D, lane, t < T); };
    auto reduce = [&](const uint4 (&src)[NCH], int t) {
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc = d64_dot(src[c], qq[c], acc);
        acc = wave_sum(acc);
        if (lane == 0) dots[(size_t)t * P + pidx] = rbf(acc);
    };
    uint4 a0[NCH], a1[NCH], a2[NCH];
    fetch(t0, a0);
    fetch(t0 + TS, a1);
    for (int t = t0; t < T; t += 3 * TS) {          // three register buffers in rotation: two rows always in flight
        fetch(t + 2 * TS, a2);
        reduce(a0, t);
        if (t + TS >= T) break;
        fetch(t + 3 * TS, a0);
        reduce(a1, t + TS);
        if (t + 2 * TS >= T) break;
        fetch(t + 4 * TS, a1);
        reduce(a2, t + 2 * TS);
    }
}

__global__ __launch_bounds__(64) void template_mean_kernel(const float* __restrict__ dots,
                                                           const float* __restrict__ weights,
                                                           float* __restrict__ scores, int T, int P) {
    const int t = blockIdx.x, lane = threadIdx.x;
    float acc = 0.f, wacc = 0.f;
    for (int pidx = lane; pidx < P; pidx += 64) {
        const float d = dots[(size_t)t * P + pidx];
        if (weights) {
            const float w = weights[(size_t)t * P + pidx];
            acc += d * w;  // bf16 score * fp32 mask promotes to fp32 in the reference (online :72-74)
            wacc += w;
        } else {
            acc += d;
        }
    }
    acc = wave_sum(acc);
    if (weights) {
        wacc = wave_sum(wacc);
        if (lane == 0) scores[t] = acc / wacc;
    } else if (lane == 0) {
        scores[t] = rbf(acc / (float)P);
    }
}


// ---------------------------------------------------------------------------------------------
// K11 per-view fine re-rank (scripts/extract_proposals_ground.py:147-160; video variant :160-176):
//   for each coarse candidate c of query q:  s_v = bf16( normalize_bf16(view_v) . f_q ) over the mesh's views,
//   score[q,c] = float32 numpy mean of the top-k s_v (sorted descending, numpy pairwise summation order).
// The per-view descriptors are kept raw fp32->bf16 (as np.load(...).to(bf16)) in one device-resident store
// [sum_views, D] with per-mesh row offsets; they are normalised on the fly with the reference's rounding points.
// One workgroup per (query, candidate); one wave per view row, scores into LDS, bitonic sort, ordered mean.
constexpr int RR_MAXV = 1024;
template <int NCH>
__global__ __launch_bounds__(256) void rerank_views_kernel(const bf16_t* __restrict__ views, const int* __restrict__ offsets,
                                                           const int* __restrict__ cand, const bf16_t* __restrict__ queries,
                                                           float* __restrict__ out, int C, int D, int k) {
    __shared__ float sc[RR_MAXV];
    const int q = blockIdx.y, c = blockIdx.x;
    const int mesh = cand[(size_t)q * C + c];
    const int r0 = offsets[mesh], nv = min(offsets[mesh + 1] - r0, RR_MAXV);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float qv[NCH][8];
    d64_load_elems<NCH>(qv, queries + (size_t)q * D, D, lane);   // element-wise: the caller's query rows need not be 16-byte aligned
    for (int v = wave; v < nv; v += 4) {
        uint4 a[NCH];
        float x[NCH][8];
        d64_load<NCH>(a, views, (size_t)(r0 + v) * D, D, lane);
        d64_unpack(a, x);
        const float s = d64_normed_dot<NCH>(x, qv);
        if (lane == 0) sc[v] = s;
    }
    int n2 = 1;
    while (n2 < nv) n2 <<= 1;
    __syncthreads();
    for (int i = nv + threadIdx.x; i < n2; i += blockDim.x) sc[i] = -3.0e38f;
    __syncthreads();
    lds_bitonic_desc(sc, n2, threadIdx.x, blockDim.x);
    if (threadIdx.x == 0) {
        // numpy float32 mean of the kk top values: pairwise summation (8 running sums, tree, sequential tail; n <= 128)
        const int kk = min(k, nv);
        float res;
        if (kk < 8) {
            res = 0.f;
            for (int i = 0; i < kk; ++i) res += sc[i];
        } else {
            float r[8];
            for (int j = 0; j < 8; ++j) r[j] = sc[j];
            int i = 8;
            for (; i < kk - (kk % 8); i += 8)
                for (int j = 0; j < 8; ++j) r[j] += sc[i + j];
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
            for (; i < kk; ++i) res += sc[i];
        }
        out[(size_t)q * C + c] = kk > 0 ? __fdiv_rn(res, (float)kk) : -3.0e38f;
    }
}

}  // namespace

int fp_cast_f32_bf16(const float* x, bf16_t* y, size_t n, hipStream_t s) {
    if (n == 0) return FP_OK;
    const int blocks = (int)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(blocks), dim3(256), 0, s, x, y, n);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

// keys: workspace [Q, N] u16
int fp_bank_scan(const bf16_t* bank, const bf16_t* queries, uint16_t* keys, int ldk, int N, int D, int Q, hipStream_t s) {
    FP_REQUIRE(N > 0 && Q > 0 && D % 8 == 0 && D <= 1536, "bank_scan: bad shape N=%d D=%d Q=%d", N, D, Q);
    const int nch = cdiv(D, 512);
    // grid: 2..8 workgroups (4 waves each) per CU, whichever leaves the smallest remainder of rows per wave
    static int ncu = [] { int dev = 0, n = 256; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n; }();
    int blocks = ncu * 2;
    {
        double best = 1e30;
        for (int bpc = 2; bpc <= 8; ++bpc) {
            const long nw = (long)ncu * bpc * 4;
            const double waste = (double)(((long)N + nw - 1) / nw * nw) / N;
            if (waste <= best) { best = waste; blocks = ncu * bpc; }
        }
        blocks = std::min(blocks, cdiv(N, 4));
    }
    for (int qb = 0; qb < Q;) {
        const int left = Q - qb;
#define FP_SCAN(NCHV, QTV)                                                                                          \
    do {                                                                                                            \
        if (D == NCHV * 512)                                                                                        \
            hipLaunchKernelGGL((bank_scan_kernel<NCHV, QTV, true>), dim3(blocks), dim3(256), 0, s, bank, queries,   \
                               keys, N, D, qb, Q, ldk);                                                             \
        else                                                                                                        \
            hipLaunchKernelGGL((bank_scan_kernel<NCHV, QTV, false>), dim3(blocks), dim3(256), 0, s, bank, queries,  \
                               keys, N, D, qb, Q, ldk);                                                             \
    } while (0)
        const int qt = left >= 4 ? 4 : 1;
        // (8 queries per pass was measured in round 4 — profiles/r04_ab.md §3: 44.4 us against 2 x 21.9 us for two 4-query passes.
        // Beyond one query the pass is bound by vector-ALU issue, ~4 us per extra query, and at 8 x 16 unpacked query values per
        // lane the kernel drops to one wave per SIMD; a matrix-pipe form would change the canonical summation order that makes the
        // indices bit-exact.  Four per pass stays.)
        fp_nch_dispatch(nch, [&](auto c) {
            constexpr int NCH = decltype(c)::value;
            if (qt == 4) FP_SCAN(NCH, 4); else FP_SCAN(NCH, 1);
        });
        qb += qt;
#undef FP_SCAN
        FP_LAUNCH_CHECK();
    }
    return FP_OK;
}

int fp_topk_select(const uint16_t* keys, int ldk, int N, int Q, int k, int idx_offset, float* out_scores, int* out_idx,
                   hipStream_t s) {
    FP_REQUIRE(k > 0 && k <= KMAX && k <= N, "topk: k=%d out of range (N=%d, max %d)", k, N, KMAX);
    FP_REQUIRE(ldk >= N && ldk % 8 == 0, "topk: key row stride %d must be >= N and a multiple of 8", ldk);
    const size_t key_bytes = (size_t)ldk * 2;
#ifdef FP_LAB
    static int env_sel = [] { const char* e = getenv("FP_TOPK_SELECT"); return e ? atoi(e) : 1; }();   // 0: histogram kernels (A/B)
    const bool use_sel = fp_opt_get(FP_OPT_TOPK_SELECT, env_sel) != 0;
#else
    constexpr bool use_sel = true;
#endif
    if (use_sel && N <= SEL_CAP) {   // counting select on register-resident keys (no LDS atomics)
        const size_t lds = (size_t)SEL_CAP * 2;
        FP_DYN_LDS_ONCE(topk_select_reg_kernel, 128 * 1024);
        hipLaunchKernelGGL(topk_select_reg_kernel, dim3(Q), dim3(SEL_T), lds, s, keys, ldk, N, k, idx_offset, out_scores, out_idx);
        FP_LAUNCH_CHECK();
        return FP_OK;
    }
    if (key_bytes <= 128 * 1024) {   // the key row fits beside the candidate buffer: all passes from LDS
        FP_DYN_LDS_ONCE(topk_select_kernel<true>, 128 * 1024);
        hipLaunchKernelGGL(topk_select_kernel<true>, dim3(Q), dim3(SEL_T), key_bytes, s, keys, ldk, N, k, idx_offset, out_scores, out_idx);
    } else {
        hipLaunchKernelGGL(topk_select_kernel<false>, dim3(Q), dim3(SEL_T), 0, s, keys, ldk, N, k, idx_offset, out_scores, out_idx);
    }
    FP_LAUNCH_CHECK();
    return FP_OK;
}

int fp_topk_merge_launch(const float* cs, const int* ci, int Q, int C, int k, float* out_scores, int* out_idx,
                  hipStream_t s) {
    FP_REQUIRE(C > 0 && k > 0 && k <= C && C <= 8192, "topk_merge: bad C=%d k=%d", C, k);
    int n2 = 1;
    while (n2 < C) n2 <<= 1;
    hipLaunchKernelGGL(topk_merge_kernel, dim3(Q), dim3(1024), n2 * sizeof(unsigned long long), s, cs, ci, C, k,
                       out_scores, out_idx);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

// dots: workspace [T*P] f32
int fp_template_score_launch(const bf16_t* tmpl, const bf16_t* qn, const float* weights, float* dots, float* scores, int T,
                      int P, int D, int templates_normalised, hipStream_t s) {
    FP_REQUIRE(T > 0 && P > 0 && D % 8 == 0 && D <= 1536, "template_score: bad shape");
    const long rows = (long)T * P;
    fp_nch_dispatch(cdiv(D, 512), [&](auto c) {
        constexpr int NCH = decltype(c)::value;
        if (templates_normalised) {
            // ~16 waves per CU in flight: TS template slices per patch index
            const int TS = std::max(1, std::min(T, cdiv(256 * 16, P)));
            hipLaunchKernelGGL(template_dots_normed_kernel<NCH>, dim3(cdiv(P * TS, 4)), dim3(256), 0, s, tmpl, qn, dots, T, P, D, TS);
        } else {
            const int blocks = (int)std::min<long>((rows + 3) / 4, 256 * 16);
            hipLaunchKernelGGL(template_dots_kernel<NCH>, dim3(blocks), dim3(256), 0, s, tmpl, qn, dots, T, P, D);
        }
    });
    FP_LAUNCH_CHECK();
    hipLaunchKernelGGL(template_mean_kernel, dim3(T), dim3(64), 0, s, dots, weights, scores, T, P);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

// per-view re-rank: out [Q,C] f32.  k <= 128 (numpy pairwise block), views per mesh <= 1024.
int fp_rerank_views_launch(const bf16_t* views, const int* offsets, const int* cand, const bf16_t* queries, float* out,
                           int Q, int C, int D, int k, hipStream_t s) {
    FP_REQUIRE(Q > 0 && C > 0 && D % 8 == 0 && D <= 1536 && k > 0 && k <= 128, "rerank_views: bad shape");
    fp_nch_dispatch(cdiv(D, 512), [&](auto c) {
        hipLaunchKernelGGL(rerank_views_kernel<decltype(c)::value>, dim3(C, Q), dim3(256), 0, s, views, offsets, cand, queries, out, C, D, k);
    });
    FP_LAUNCH_CHECK();
    return FP_OK;
}

// ---------------------------------------------------------------------------------------------
// Exact k nearest rows in Euclidean distance: scipy.spatial.KDTree(table).query(queries, k) of GPT4ScaleEstimator
// (src/pipeline/estimators/scale_estimators.py:48,66) as a brute-force scan.  Squared distances in fp32 in a FIXED order — lane l of a
// wave adds (t[e] - q[e])^2 for e = l, l + 64, ... with one fmaf each, then the xor butterfly of wave_sum — so equal rows get equal
// bits and two calls agree.  Results ordered by (distance ascending, row index ascending): attn_hd_core.h fp_knn_key.
#include "attn_hd_core.h"

namespace {

__global__ __launch_bounds__(256) void knn_dist_kernel(const float* __restrict__ table, const float* __restrict__ queries,
                                                       float* __restrict__ d2, int N, int E) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float* t = table + (size_t)row * E;
    const float* q = queries + (size_t)blockIdx.y * E;
    float acc = 0.f;
    for (int e = lane; e < E; e += 64) {
        const float d = t[e] - q[e];
        acc = __fmaf_rn(d, d, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) d2[(size_t)blockIdx.y * N + row] = acc;
}

// one workgroup per query: k rounds, each the minimum key strictly above the previous round's (keys are unique: they carry the row)
__global__ __launch_bounds__(256) void knn_select_kernel(const float* __restrict__ d2, int N, int k, int* __restrict__ out_idx,
                                                         float* __restrict__ out_d2) {
    __shared__ unsigned long long red[256];
    const float* d = d2 + (size_t)blockIdx.x * N;
    unsigned long long prev = 0ull;
    for (int j = 0; j < k; ++j) {
        unsigned long long best = ~0ull;
        for (int i = threadIdx.x; i < N; i += 256) {
            const unsigned long long key = fp_knn_key(__float_as_uint(d[i]), (uint32_t)i);
            if ((j == 0 || key > prev) && key < best) best = key;
        }
        red[threadIdx.x] = best;
        __syncthreads();
        for (int sft = 128; sft > 0; sft >>= 1) {
            if ((int)threadIdx.x < sft) {
                const unsigned long long o = red[threadIdx.x + sft];
                if (o < red[threadIdx.x]) red[threadIdx.x] = o;
            }
            __syncthreads();
        }
        prev = red[0];
        __syncthreads();
        if (threadIdx.x == 0) {
            out_idx[(size_t)blockIdx.x * k + j] = (int)fp_knn_key_row(prev);
            out_d2[(size_t)blockIdx.x * k + j] = __uint_as_float(fp_knn_key_bits(prev));
        }
    }
}

}  // namespace

// d2_ws: f32 [Q,N] scratch
int fp_knn_l2_launch(const float* table, int N, int E, const float* queries, int Q, int k, float* d2_ws, int* out_idx, float* out_d2,
                     hipStream_t s) {
    FP_REQUIRE(table && queries && d2_ws && out_idx && out_d2, "knn_l2: null argument");
    FP_REQUIRE(N > 0 && E > 0 && Q > 0 && Q <= 65535, "knn_l2: bad shape N=%d E=%d Q=%d", N, E, Q);
    FP_REQUIRE(k >= 1 && k <= 64 && k <= N, "knn_l2: k=%d (1 <= k <= 64 and k <= N=%d)", k, N);
    hipLaunchKernelGGL(knn_dist_kernel, dim3(cdiv(N, 4), Q), dim3(256), 0, s, table, queries, d2_ws, N, E);
    FP_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_select_kernel, dim3(Q), dim3(256), 0, s, d2_ws, N, k, out_idx, out_d2);
    FP_LAUNCH_CHECK();
    return FP_OK;
}
