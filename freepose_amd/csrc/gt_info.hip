// gt_info.hip — what the BOP toolkit's dataset-preparation scripts compute per ground-truth instance and per model, without their OpenGL
// renderer and without the Python loop over all point pairs:
//
//   a. gi_visibility_kernel   one fused pass over a rendered depth canvas and the scene's test depth image -> px_count_all / valid /
//                             visib, the two bounding boxes, the mask and mask_visib images
//                             (bop_toolkit/scripts/calc_gt_info.py:131-173, calc_gt_masks.py:107-126)
//   b. gi_diameter_kernel     brute-force maximum of the squared fp64 distances over all point pairs, tile pair by tile pair
//      gi_diameter_final      maximum of the per-block slots, one square root, the model's bounding box
//                             (bop_toolkit_lib/misc.py:289-303 calc_pts_diameter, scripts/calc_model_info.py:36-37)
//
// Numerics: a. is integer-exact given the depth images — the per-pixel float64 expressions are gt_info_core.h's, the
// sums and extrema are integer atomics, so two calls give the same bits.  b. is bit-exact: the maximum is order-independent, the pair
// expression is (dx dx + dy dy) + dz dz in fp64 without FMA (this file is compiled with -ffp-contract=off), and sqrt is monotone, so
// sqrt(max of squares) is the reference's max of square roots.  No floating-point atomics.
#include "gt_info_core.h"
#include "internal.h"

namespace {

constexpr int VIS_THREADS = 256;
constexpr int VIS_MAX_BLOCKS = 128;       // blocks per instance; beyond that the block strides over the canvas

__device__ __forceinline__ int wave_sum_s32(int v) {
#pragma unroll
    for (int mk = 32; mk > 0; mk >>= 1) v += __shfl_xor(v, mk, 64);
    return v;
}
__device__ __forceinline__ int wave_min_s32(int v) {
#pragma unroll
    for (int mk = 32; mk > 0; mk >>= 1) v = min(v, __shfl_xor(v, mk, 64));
    return v;
}
__device__ __forceinline__ int wave_max_s32(int v) {
#pragma unroll
    for (int mk = 32; mk > 0; mk >>= 1) v = max(v, __shfl_xor(v, mk, 64));
    return v;
}

// ---- a. visibility (GiAcc and gi_pixel: gt_info_core.h) -------------------------------------------------------------------------------
__global__ void gi_init_kernel(int32_t* __restrict__ out, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int32_t* o = out + (size_t)b * FP_GI_OUT_LD;
    o[0] = o[1] = o[2] = o[3] = 0;
    o[4] = o[5] = o[8] = o[9] = FP_GI_BOX_EMPTY_MIN;
    o[6] = o[7] = o[10] = o[11] = FP_GI_BOX_EMPTY_MAX;
}

// grid (pixel blocks, instance).  VEC: 4 canvas pixels of one row per lane and step (16-byte loads of both depth stacks, 4-byte stores of
// the masks); the launcher takes it only when Wr, W and ox are multiples of 4 and the stacks are 16-byte aligned, so that a group of 4
// lies wholly inside or wholly outside the window.
template <bool VEC>
__global__ __launch_bounds__(VIS_THREADS) void gi_visibility_kernel(const float* __restrict__ d_gt, int Hr, int Wr, int ox, int oy,
                                                                    const float* __restrict__ d_test, int n_img, int H, int W,
                                                                    const int* __restrict__ img_idx, const double* __restrict__ params,
                                                                    uint8_t* __restrict__ mask, uint8_t* __restrict__ mask_visib,
                                                                    int32_t* __restrict__ out) {
    __shared__ int32_t acc[FP_GI_OUT_LD];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < FP_GI_OUT_LD) acc[tid] = (tid < 4) ? 0 : (((tid - 4) & 3) < 2 ? FP_GI_BOX_EMPTY_MIN : FP_GI_BOX_EMPTY_MAX);
    __syncthreads();
    const int im = img_idx[b];
    if (!gi_img_ok(im, n_img) || !gi_window_ok(Wr, Hr, ox, oy, W, H)) return;      // block-uniform: the row keeps the launcher's values
    const size_t npix = (size_t)Hr * Wr, nwin = (size_t)H * W;
    const float* G = d_gt + (size_t)b * npix;
    const float* T = d_test + (size_t)im * nwin;
    uint8_t* M = mask ? mask + (size_t)b * nwin : nullptr;
    uint8_t* V = mask_visib ? mask_visib + (size_t)b * nwin : nullptr;
    double prm[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) prm[k] = params[(size_t)b * FP_GI_PARAM_LD + k];
    const float delta = (float)prm[4];                // numpy compares the float32 difference image with the scalar in float32
    GiAcc a;
    if (VEC) {
        const int n4 = (int)(npix >> 2), Wr4 = Wr >> 2;
        for (int i = blockIdx.x * VIS_THREADS + tid; i < n4; i += gridDim.x * VIS_THREADS) {
            const int y = i / Wr4, x = (i - y * Wr4) << 2;
            const float4 g = reinterpret_cast<const float4*>(G)[i];
            const bool inw = gi_in_window(x, y, ox, oy, W, H);
            const size_t w = inw ? (size_t)(y - oy) * W + (x - ox) : 0;
            float4 t = {0.f, 0.f, 0.f, 0.f};
            if (inw && (g.x != 0.f || g.y != 0.f || g.z != 0.f || g.w != 0.f)) t = *reinterpret_cast<const float4*>(T + w);
            const int b0 = gi_pixel(g.x, t.x, inw, x, y, ox, oy, prm, delta, a);
            const int b1 = gi_pixel(g.y, t.y, inw, x + 1, y, ox, oy, prm, delta, a);
            const int b2 = gi_pixel(g.z, t.z, inw, x + 2, y, ox, oy, prm, delta, a);
            const int b3 = gi_pixel(g.w, t.w, inw, x + 3, y, ox, oy, prm, delta, a);
            if (inw && M)
                *reinterpret_cast<uchar4*>(M + w) = make_uchar4((b0 & FP_GI_MASK) ? 255 : 0, (b1 & FP_GI_MASK) ? 255 : 0,
                                                                (b2 & FP_GI_MASK) ? 255 : 0, (b3 & FP_GI_MASK) ? 255 : 0);
            if (inw && V)
                *reinterpret_cast<uchar4*>(V + w) = make_uchar4((b0 & FP_GI_VISIB) ? 255 : 0, (b1 & FP_GI_VISIB) ? 255 : 0,
                                                                (b2 & FP_GI_VISIB) ? 255 : 0, (b3 & FP_GI_VISIB) ? 255 : 0);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * VIS_THREADS + tid; i < npix; i += (size_t)gridDim.x * VIS_THREADS) {
            const int y = (int)(i / Wr), x = (int)(i - (size_t)y * Wr);
            const float g = G[i];
            const bool inw = gi_in_window(x, y, ox, oy, W, H);
            const size_t w = inw ? (size_t)(y - oy) * W + (x - ox) : 0;
            const float t = (inw && g != 0.f) ? T[w] : 0.f;
            const int bits = gi_pixel(g, t, inw, x, y, ox, oy, prm, delta, a);
            if (inw && M) M[w] = (bits & FP_GI_MASK) ? 255 : 0;
            if (inw && V) V[w] = (bits & FP_GI_VISIB) ? 255 : 0;
        }
    }
    // wave butterflies, then one LDS atomic per wave and value, then one global atomic per block and value: integers, any order
    const bool lead = (tid & 63) == 0;
    int v;
    v = wave_sum_s32(a.all);   if (lead && v) atomicAdd(&acc[0], v);
    v = wave_sum_s32(a.valid); if (lead && v) atomicAdd(&acc[1], v);
    v = wave_sum_s32(a.visib); if (lead && v) atomicAdd(&acc[2], v);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        v = wave_min_s32(a.box_all[k]);     if (lead) atomicMin(&acc[4 + k], v);
        v = wave_max_s32(a.box_all[2 + k]); if (lead) atomicMax(&acc[6 + k], v);
        v = wave_min_s32(a.box_vis[k]);     if (lead) atomicMin(&acc[8 + k], v);
        v = wave_max_s32(a.box_vis[2 + k]); if (lead) atomicMax(&acc[10 + k], v);
    }
    __syncthreads();
    int32_t* o = out + (size_t)b * FP_GI_OUT_LD;
    if (tid < 3) {
        if (acc[tid]) atomicAdd(&o[tid], acc[tid]);
    } else if (tid >= 4 && tid < FP_GI_OUT_LD) {
        if (((tid - 4) & 3) < 2) atomicMin(&o[tid], acc[tid]);
        else atomicMax(&o[tid], acc[tid]);
    }
}

// ---- b. diameter ---------------------------------------------------------------------------------------------------------------------
constexpr int DM_THREADS = 256;
constexpr int DM_IPL = 4;                          // i points per lane, their running maxima in registers
constexpr int DM_TILE = DM_THREADS * DM_IPL;       // points per tile, i and j alike (the j tile: 3 x 8 KiB of LDS)

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int mk = 32; mk > 0; mk >>= 1) v = fmax(v, __shfl_xor(v, mk, 64));
    return v;
}

// grid (tile pair, model): pair p enumerates (ti, tj), ti <= tj < n_tiles, row by row.  A model with fewer tiles leaves its other slots 0
// (the pair of a point with itself is 0 in every model, so 0 never changes a maximum).  Lanes and LDS slots past the end of the range
// hold the range's first point: such a pair is a real pair of the cloud.
__global__ __launch_bounds__(DM_THREADS) void gi_diameter_kernel(const double* __restrict__ pts, int n_pts, const int* __restrict__ ranges,
                                                                 int n_tiles, int n_pairs, double* __restrict__ slots) {
    __shared__ double tx[DM_TILE], ty[DM_TILE], tz[DM_TILE];
    __shared__ double red[DM_THREADS / 64];
    const int m = blockIdx.y, tid = threadIdx.x;
    const int first = ranges[2 * m], count = ranges[2 * m + 1];
    int p = blockIdx.x, ti = 0;
    while (p >= n_tiles - ti) {
        p -= n_tiles - ti;
        ++ti;
    }
    const int tj = ti + p;
    double* slot = slots + (size_t)m * n_pairs + blockIdx.x;
    if (!gi_range_ok(first, count, n_pts) || (long long)tj * DM_TILE >= count) {      // block-uniform
        if (tid == 0) *slot = 0.0;
        return;
    }
    const double* P = pts + (size_t)first * 3;
    double ix[DM_IPL], iy[DM_IPL], iz[DM_IPL], mx[DM_IPL];
#pragma unroll
    for (int k = 0; k < DM_IPL; ++k) {
        const int i = ti * DM_TILE + k * DM_THREADS + tid, s = i < count ? i : 0;
        ix[k] = P[3 * (size_t)s], iy[k] = P[3 * (size_t)s + 1], iz[k] = P[3 * (size_t)s + 2];
        mx[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < DM_IPL; ++k) {
        const int l = k * DM_THREADS + tid, j = tj * DM_TILE + l, s = j < count ? j : 0;
        tx[l] = P[3 * (size_t)s], ty[l] = P[3 * (size_t)s + 1], tz[l] = P[3 * (size_t)s + 2];
    }
    __syncthreads();
    const int cnt = min(DM_TILE, (count - tj * DM_TILE + 3) & ~3);      // whole groups of 4: the first point fills the last one
#pragma unroll 4
    for (int j = 0; j < cnt; ++j) {
        const double bx = tx[j], by = ty[j], bz = tz[j];                // every lane reads the same address: an LDS broadcast
#pragma unroll
        for (int k = 0; k < DM_IPL; ++k) mx[k] = fmax(mx[k], gi_pair_d2(ix[k], iy[k], iz[k], bx, by, bz));
    }
    double v = fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
    v = wave_max_f64(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) *slot = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// one block per model: maximum of its slots -> one square root; minima and maxima of the coordinates -> the box of calc_model_info.py
__global__ __launch_bounds__(DM_THREADS) void gi_diameter_final(const double* __restrict__ pts, int n_pts, const int* __restrict__ ranges,
                                                                int n_pairs, const double* __restrict__ slots, double* __restrict__ out) {
    __shared__ double red[7][DM_THREADS / 64];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int first = ranges[2 * m], count = ranges[2 * m + 1];
    double* o = out + (size_t)m * FP_GI_DIAM_LD;
    if (!gi_range_ok(first, count, n_pts)) {                       // block-uniform: a refused range answers NaN
        if (tid < FP_GI_DIAM_LD) o[tid] = tid < 7 ? __builtin_nan("") : 0.0;
        return;
    }
    const double* P = pts + (size_t)first * 3;
    double d2 = 0.0, lo[3] = {P[0], P[1], P[2]}, hi[3] = {P[0], P[1], P[2]};
    for (int i = tid; i < n_pairs; i += DM_THREADS) d2 = fmax(d2, slots[(size_t)m * n_pairs + i]);
    for (int i = tid; i < count; i += DM_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double c = P[3 * (size_t)i + k];
            lo[k] = fmin(lo[k], c);
            hi[k] = fmax(hi[k], c);
        }
    }
    double v[7] = {d2, -lo[0], -lo[1], -lo[2], hi[0], hi[1], hi[2]};     // minima as maxima of the negated values (exact)
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double w = wave_max_f64(v[k]);
        if ((tid & 63) == 0) red[k][tid >> 6] = w;
    }
    __syncthreads();
    if (tid == 0) {
        double r[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) r[k] = fmax(fmax(red[k][0], red[k][1]), fmax(red[k][2], red[k][3]));
        o[0] = gi_sqrt(r[0]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double mn = -r[1 + k];
            o[1 + k] = mn;
            o[4 + k] = r[4 + k] - mn;                              // pts.max(axis=0) - ref_pt
        }
        o[7] = 0.0;
    }
}

}  // namespace

int fp_gt_visibility_launch(const float* d_gt, int B, int Hr, int Wr, int ox, int oy, const float* d_test, int n_img, int H, int W,
                            const int* img_idx, const double* params, uint8_t* mask, uint8_t* mask_visib, int32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(gi_init_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, out, B);
    const size_t npix = (size_t)Hr * Wr;
    const uintptr_t align = (uintptr_t)d_gt | (uintptr_t)d_test | (uintptr_t)mask | (uintptr_t)mask_visib;
    const bool vec = (Wr & 3) == 0 && (W & 3) == 0 && (ox & 3) == 0 && (align & 15) == 0;      // else the scalar loop (same answers)
    const size_t work = vec ? npix >> 2 : npix;
    const dim3 grid((unsigned)std::max<size_t>(1, std::min<size_t>((work + VIS_THREADS - 1) / VIS_THREADS, VIS_MAX_BLOCKS)), B);
    if (vec)
        hipLaunchKernelGGL(gi_visibility_kernel<true>, grid, dim3(VIS_THREADS), 0, s, d_gt, Hr, Wr, ox, oy, d_test, n_img, H, W, img_idx, params,
                           mask, mask_visib, out);
    else
        hipLaunchKernelGGL(gi_visibility_kernel<false>, grid, dim3(VIS_THREADS), 0, s, d_gt, Hr, Wr, ox, oy, d_test, n_img, H, W, img_idx, params,
                           mask, mask_visib, out);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

int fp_pts_diameter_tile(void) { return DM_TILE; }

int fp_pts_diameter_launch(const double* pts, int n_pts, const int* ranges, int M, int max_count, double* slots, double* out, hipStream_t s) {
    const int n_tiles = cdiv(max_count, DM_TILE), n_pairs = n_tiles * (n_tiles + 1) / 2;
    hipLaunchKernelGGL(gi_diameter_kernel, dim3(n_pairs, M), dim3(DM_THREADS), 0, s, pts, n_pts, ranges, n_tiles, n_pairs, slots);
    hipLaunchKernelGGL(gi_diameter_final, dim3(M), dim3(DM_THREADS), 0, s, pts, n_pts, ranges, n_pairs, slots, out);
    FP_LAUNCH_CHECK();
    return FP_OK;
}
