// lk_track.hip — the built-in point tracker: pyramidal Lucas-Kanade (Bouguet's formulation) with a forward-backward check, a classical
// stand-in for the learned tracker the reference fetches (no parity claim).  lk_core.h holds the arithmetic.
//
//   fp_lk_pyramid   grey + level 0 in one kernel, then one kernel per further level over all T frames ([1 4 6 4 1] / 16, rows then
//                   columns, replicate border, even pixels); levels back to back, each [T, h_l, w_l] float32
//   fp_lk_track     an init kernel writes the query rows, then chain step s = 1 .. T-1, one launch each: item i = (query i >> 1,
//                   direction i & 1) moves its chain one frame outward, src = t_q +- (s - 1) -> dst = t_q +- s.  One wave per item, four
//                   items per workgroup; the window's pixels lie on the lanes (pixel k on lane k % 64), the five sums of G and b are
//                   reduced with an __shfl_xor butterfly in a fixed order, so every lane holds the same value and two calls give the same
//                   bits.  The pyramid is fp32; samples, sums, updates and the chain positions (a [T,N,2] fp64 workspace beside the
//                   float32 tracks that are returned) are fp64.  No LDS, no atomics; lane 0 writes the item's results.
#include "internal.h"
#include "lk_core.h"

namespace {
constexpr int WG = 256, ITEMS_PER_WG = WG / FP_LK_LANES;

__global__ __launch_bounds__(WG) void lk_grey_kernel(const uint8_t* __restrict__ frames, float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * WG + threadIdx.x;
    if (i >= n) return;
    const uint8_t* p = frames + i * 3;
    out[i] = lk_grey(p[0], p[1], p[2]);
}

// blockIdx.y = frame
__global__ __launch_bounds__(WG) void lk_down_kernel(const float* __restrict__ src, int hs, int ws, float* __restrict__ dst, int hd, int wd) {
    const int i = blockIdx.x * WG + threadIdx.x;
    if (i >= hd * wd) return;
    const int t = blockIdx.y;
    dst[(long long)t * hd * wd + i] = lk_down_pixel(src + (long long)t * hs * ws, hs, ws, i / wd, i % wd);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = FP_LK_LANES / 2; m > 0; m >>= 1) v = v + __shfl_xor(v, m, FP_LK_LANES);
    return v;
}

// one LK run from frame ta to frame tb for the point (px, py) of the image; every lane of the wave returns the same values
template <int SLOTS>
__device__ void lk_run(const LkPyramid& P, const float* __restrict__ pyr, int ta, int tb, double px, double py, int r, int iters, double& ox,
                       double& oy, double& eig, double& res) {
    const int lane = threadIdx.x & (FP_LK_LANES - 1);
    const int npix = (2 * r + 1) * (2 * r + 1);
    double gx = 0.0, gy = 0.0;
    ox = px;
    oy = py;
    eig = 0.0;
    res = 0.0;
    for (int l = P.levels - 1; l >= 0; --l) {
        const int w = P.w[l], h = P.h[l];
        const float* A = pyr + P.off[l] + (long long)ta * h * w;
        const float* B = pyr + P.off[l] + (long long)tb * h * w;
        const double sc = lk_level_scale(l), plx = px * sc, ply = py * sc;
        double a[SLOTS], ix[SLOTS], iy[SLOTS];
        double gxx = 0.0, gxy = 0.0, gyy = 0.0;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const int k = lane + FP_LK_LANES * j;
            a[j] = ix[j] = iy[j] = 0.0;
            if (k < npix) {
                lk_window_pixel(A, w, h, plx, ply, k, r, a[j], ix[j], iy[j]);
                lk_g_terms(ix[j], iy[j], gxx, gxy, gyy);
            }
        }
        gxx = wave_sum(gxx);
        gxy = wave_sum(gxy);
        gyy = wave_sum(gyy);
        double vx = 0.0, vy = 0.0;
        if (lk_solvable(gxx, gxy, gyy, npix)) {
            for (int it = 0; it < iters; ++it) {
                double bx = 0.0, by = 0.0;
#pragma unroll
                for (int j = 0; j < SLOTS; ++j) {
                    const int k = lane + FP_LK_LANES * j;
                    if (k < npix) lk_b_terms(a[j], lk_moved_sample(B, w, h, plx, ply, gx, gy, vx, vy, k, r), ix[j], iy[j], bx, by);
                }
                bx = wave_sum(bx);
                by = wave_sum(by);
                lk_solve(gxx, gxy, gyy, bx, by, vx, vy);
            }
        }
        if (l == 0) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < SLOTS; ++j) {
                const int k = lane + FP_LK_LANES * j;
                if (k < npix) s = s + fabs(a[j] - lk_moved_sample(B, w, h, plx, ply, gx, gy, vx, vy, k, r));
            }
            res = wave_sum(s) / (double)npix;
            eig = lk_min_eig(gxx, gxy, gyy, npix);
            ox = plx + (gx + vx);
            oy = ply + (gy + vy);
        } else {
            gx = 2.0 * (gx + vx);
            gy = 2.0 * (gy + vy);
        }
    }
}

__global__ __launch_bounds__(WG) void lk_init_kernel(const float* __restrict__ queries, int N, int T, int H, int W, double* __restrict__ state,
                                                     float* __restrict__ tracks, uint8_t* __restrict__ vis, float* __restrict__ diag) {
    const int n = blockIdx.x * WG + threadIdx.x;
    if (n >= N) return;
    const int tq = lk_query_time(queries[n * 3], T);
    const float x = lk_finite_or_zero(queries[n * 3 + 1]), y = lk_finite_or_zero(queries[n * 3 + 2]);
    const long long row = (long long)tq * N + n;
    const bool in = lk_inside(x, y, W, H);
    state[row * 2] = x;
    state[row * 2 + 1] = y;
    tracks[row * 2] = x;
    tracks[row * 2 + 1] = y;
    vis[row] = in ? 1 : 0;
    diag[row * 4] = 0.0f;
    diag[row * 4 + 1] = 0.0f;
    diag[row * 4 + 2] = 0.0f;
    diag[row * 4 + 3] = in ? 0.0f : (float)FP_LK_FLAG_OUTSIDE;
}

template <int SLOTS>
__global__ __launch_bounds__(WG) void lk_step_kernel(LkPyramid P, const float* __restrict__ pyr, const float* __restrict__ queries, int N,
                                                     int step, int r, int iters, float fb_thresh, float min_eig, float max_residual,
                                                     double* __restrict__ state, float* __restrict__ tracks, uint8_t* __restrict__ vis,
                                                     float* __restrict__ diag) {
    const int item = blockIdx.x * ITEMS_PER_WG + (threadIdx.x >> 6);      // uniform over the wave
    if (item >= 2 * N) return;
    const int n = item >> 1, dir = item & 1;
    const int tq = lk_query_time(queries[n * 3], P.T);
    const int src = dir ? tq - (step - 1) : tq + (step - 1), dst = dir ? tq - step : tq + step;
    if (dst < 0 || dst >= P.T) return;
    const long long rs = (long long)src * N + n, rd = (long long)dst * N + n;
    const double sx = state[rs * 2], sy = state[rs * 2 + 1];
    const bool prev = vis[rs] != 0;
    double fx, fy, eig, res, bx, by, eig_b, res_b, fb;
    lk_run<SLOTS>(P, pyr, src, dst, sx, sy, r, iters, fx, fy, eig, res);
    lk_run<SLOTS>(P, pyr, dst, src, fx, fy, r, iters, bx, by, eig_b, res_b);
    const int flags = lk_judge(sx, sy, fx, fy, bx, by, eig, res, fb_thresh, min_eig, max_residual, P.w[0], P.h[0], prev, fb);
    if ((threadIdx.x & (FP_LK_LANES - 1)) == 0) {
        state[rd * 2] = fx;
        state[rd * 2 + 1] = fy;
        tracks[rd * 2] = (float)fx;
        tracks[rd * 2 + 1] = (float)fy;
        vis[rd] = flags == 0 ? 1 : 0;
        diag[rd * 4] = (float)fb;
        diag[rd * 4 + 1] = (float)eig;
        diag[rd * 4 + 2] = (float)res;
        diag[rd * 4 + 3] = (float)flags;
    }
}
}  // namespace

int fp_lk_pyramid_launch(const uint8_t* frames, const LkPyramid& P, float* pyr, hipStream_t s) {
    const long long n0 = (long long)P.T * P.h[0] * P.w[0];
    hipLaunchKernelGGL(lk_grey_kernel, dim3((unsigned)((n0 + WG - 1) / WG)), dim3(WG), 0, s, frames, pyr, n0);
    for (int l = 1; l < P.levels; ++l)
        hipLaunchKernelGGL(lk_down_kernel, dim3(cdiv(P.h[l] * P.w[l], WG), P.T), dim3(WG), 0, s, pyr + P.off[l - 1], P.h[l - 1], P.w[l - 1],
                           pyr + P.off[l], P.h[l], P.w[l]);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

int fp_lk_track_launch(const LkPyramid& P, const float* pyr, const float* queries, int N, int radius, int iters, float fb_thresh,
                       float min_eig, float max_residual, double* state, float* tracks, uint8_t* vis, float* diag, hipStream_t s) {
    if (N == 0) return FP_OK;
    hipLaunchKernelGGL(lk_init_kernel, dim3(cdiv(N, WG)), dim3(WG), 0, s, queries, N, P.T, P.h[0], P.w[0], state, tracks, vis, diag);
    const int npix = (2 * radius + 1) * (2 * radius + 1);
    const dim3 grid(cdiv(2 * N, ITEMS_PER_WG));
    for (int step = 1; step < P.T; ++step) {
        if (npix <= 4 * FP_LK_LANES)
            hipLaunchKernelGGL(lk_step_kernel<4>, grid, dim3(WG), 0, s, P, pyr, queries, N, step, radius, iters, fb_thresh, min_eig,
                               max_residual, state, tracks, vis, diag);
        else
            hipLaunchKernelGGL(lk_step_kernel<16>, grid, dim3(WG), 0, s, P, pyr, queries, N, step, radius, iters, fb_thresh, min_eig,
                               max_residual, state, tracks, vis, diag);
    }
    FP_LAUNCH_CHECK();
    return FP_OK;
}
