// eval.hip — pose-error evaluation on the device: the model-free errors of the FreePose paper as the reference's modified BOP toolkit
// computes them (bop_toolkit/bop_toolkit_lib/pose_error.py: chamfer :188-201, chamfer_proj :204-218, cus :357-386, vsd :17-112),
// without its OpenGL renderer and its two kd-trees per estimate x ground-truth pair.
//
//   a. eval_prep_kernel      posed (or projected) vertex clouds of every pair, fp64, centred on the pair's origin, rounded ONCE to fp32
//   b. eval_nn_kernel        exact brute-force nearest neighbour, both directions, target cloud streamed through LDS
//      eval_nn_final_kernel  fixed-order fp64 sum of the per-block partial sums -> mean_y(min_x) + mean_x(min_y)
//   c. eval_depth_compare_kernel   per-pixel compare of two rendered depth stacks (+ the test depth image for VSD) -> integer counts
//
// Numerics (DESIGN.md "Scoring"):
//   * a. follows misc.transform_pts_Rt / misc.project_pts in fp64 (pts * s_e first, then R p + t; P = K [R|t], then the divide).  The
//     origin (posed / projected centroid of the ground-truth cloud) is subtracted from BOTH clouds before the one rounding to fp32, so
//     the rounding error is 2^-24 of the object's size, not of its distance from the camera.  Distances do not change under a common shift.
//   * b. keeps min(dx^2 + dy^2 (+ dz^2)) in fp32 in the difference form, takes one fp64 sqrt per query, and adds in a fixed order:
//     threads own fixed queries, the block tree is fixed, the per-block slots are added in index order.  No floating-point atomics:
//     two runs give the same bits.
//   * c. is integer-exact: every float64 the reference forms per pixel is formed by the same operations in the same order (this file is
//     compiled with -ffp-contract=off: no FMA appears that numpy would not execute); the counts are added with integer atomics.
#include "internal.h"

namespace {

constexpr int XF_LD = FP_EVAL_XF_LD;      // doubles per pair in d_xf
constexpr int TB_LD = FP_EVAL_TABLE_LD;   // ints per pair in d_table
constexpr int NN_THREADS = 256;
constexpr int NN_QPL = 8;                 // queries per lane, minima in registers
constexpr int NN_QCHUNK = NN_THREADS * NN_QPL;
constexpr int NN_TILE = 1024;             // target points per LDS tile (float4 each: 16 KiB)
constexpr float NN_FAR = 1.0e30f;         // padding target: its squared distance overflows to +inf and never wins a min

// ---- a. posed clouds ---------------------------------------------------------------------------------------------------------------
// d_xf [B, XF_LD] f64: 0 s_e | 1..9 R_e | 10..12 t_e | 13..21 R_g | 22..24 t_g | 25..27 centroid of the GT cloud (model frame) | 28..36 K
// d_table [B, TB_LD] i32: 0 first point of the estimate's cloud in d_pts | 1 its size | 2, 3 the same for the GT cloud | 4, 5 first slot of
//                         the two centred clouds in the workspace
__device__ __forceinline__ void posed(const double* R, const double* t, double x, double y, double z, double* q) {
    q[0] = R[0] * x + R[1] * y + R[2] * z + t[0];
    q[1] = R[3] * x + R[4] * y + R[5] * z + t[1];
    q[2] = R[6] * x + R[7] * y + R[8] * z + t[2];
}
// misc.project_pts: P = K.dot(hstack(R, t)); pts_im = P.dot(pts_h.T); pts_im /= pts_im[2]
__device__ __forceinline__ void projected(const double* K, const double* R, const double* t, double x, double y, double z, double* uv) {
    double P[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) P[r * 4 + c] = K[r * 3] * R[c] + K[r * 3 + 1] * R[3 + c] + K[r * 3 + 2] * R[6 + c];
        P[r * 4 + 3] = K[r * 3] * t[0] + K[r * 3 + 1] * t[1] + K[r * 3 + 2] * t[2];
    }
    const double a = P[0] * x + P[1] * y + P[2] * z + P[3];
    const double b = P[4] * x + P[5] * y + P[6] * z + P[7];
    const double w = P[8] * x + P[9] * y + P[10] * z + P[11];
    uv[0] = a / w;
    uv[1] = b / w;
}

template <int DIM>
__global__ __launch_bounds__(256) void eval_prep_kernel(const double* __restrict__ pts, int n_pts, const int* __restrict__ table,
                                                        const double* __restrict__ xf, int ws_pts, float* __restrict__ ws) {
    const int b = blockIdx.z, side = blockIdx.y;      // side 0: the estimate's cloud, 1: the ground truth's
    const int* tb = table + (size_t)b * TB_LD;
    const int src = tb[side * 2], n = tb[side * 2 + 1], dst = tb[4 + side];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (src < 0 || dst < 0 || (long long)src + n > n_pts || (long long)dst + n > ws_pts) return;   // a table that points outside: nothing is touched
    const double* X = xf + (size_t)b * XF_LD;
    const double* R = side ? X + 13 : X + 1;
    const double* t = side ? X + 22 : X + 10;
    const double* p = pts + ((size_t)src + i) * 3;
    double x = p[0], y = p[1], z = p[2];
    if (side == 0) { x *= X[0]; y *= X[0]; z *= X[0]; }   // models[inf_id]["pts"] *= s_e (eval_calc_errors.py:380)
    const double* c = X + 25;
    double q[3], o[3];
    if (DIM == 3) {
        posed(R, t, x, y, z, q);
        posed(X + 13, X + 22, c[0], c[1], c[2], o);
    } else {
        projected(X + 28, R, t, x, y, z, q);
        projected(X + 28, X + 13, X + 22, c[0], c[1], c[2], o);
    }
#pragma unroll
    for (int k = 0; k < DIM; ++k) ws[(size_t)k * ws_pts + dst + i] = (float)(q[k] - o[k]);
}

// ---- b. nearest neighbour ------------------------------------------------------------------------------------------------------------
// grid (query chunk, direction, pair).  direction 0: queries = GT cloud, targets = estimate (mean_y min_x), 1: the other way round.
// Every lane of a wave reads the same float4 of the tile (an LDS broadcast: one LDS read per target and wave) and updates its
// NN_QPL running minima: 3 subtractions, 1 multiply, 2 FMAs and half a v_min3 per point pair in 3-D.
template <int DIM>
__global__ __launch_bounds__(NN_THREADS) void eval_nn_kernel(const float* __restrict__ ws, int ws_pts, int n_pts,
                                                             const int* __restrict__ table, int n_chunks, double* __restrict__ slots) {
    __shared__ float4 tile[NN_TILE];
    __shared__ double red[NN_THREADS];
    const int b = blockIdx.z, dir = blockIdx.y, tid = threadIdx.x;
    const int* tb = table + (size_t)b * TB_LD;
    const int qs = dir == 0 ? 1 : 0, ts = 1 - qs;
    const int nq = tb[qs * 2 + 1], qoff = tb[4 + qs], nt = tb[ts * 2 + 1], toff = tb[4 + ts];
    const int q0 = blockIdx.x * NN_QCHUNK;
    double* slot = slots + ((size_t)b * 2 + dir) * n_chunks + blockIdx.x;
    // the checks of eval_prep_kernel, for both clouds: a row it refused left its workspace slots unwritten
    const bool bad = nq <= 0 || nt <= 0 || qoff < 0 || toff < 0 || (long long)qoff + nq > ws_pts || (long long)toff + nt > ws_pts ||
                     tb[0] < 0 || tb[2] < 0 || (long long)tb[0] + tb[1] > n_pts || (long long)tb[2] + tb[3] > n_pts;
    if (bad || q0 >= nq) {     // block-uniform: a bad table row (its result becomes NaN), chunks past the end of a shorter cloud
        if (tid == 0) *slot = bad ? __builtin_nan("") : 0.0;
        return;
    }
    const float* X = ws + qoff;
    const float* Y = ws + (size_t)ws_pts + qoff;
    const float* Z = ws + 2 * (size_t)ws_pts + qoff;
    float qx[NN_QPL], qy[NN_QPL], qz[NN_QPL], m[NN_QPL];
#pragma unroll
    for (int j = 0; j < NN_QPL; ++j) {
        const int i = q0 + j * NN_THREADS + tid;
        const bool in = i < nq;
        qx[j] = in ? X[i] : 0.f;
        qy[j] = in ? Y[i] : 0.f;
        qz[j] = (DIM == 3 && in) ? Z[i] : 0.f;
        m[j] = __builtin_inff();
    }
    const float* TX = ws + toff;
    const float* TY = ws + (size_t)ws_pts + toff;
    const float* TZ = ws + 2 * (size_t)ws_pts + toff;
    for (int t0 = 0; t0 < nt; t0 += NN_TILE) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < NN_TILE / NN_THREADS; ++k) {
            const int l = k * NN_THREADS + tid, i = t0 + l;
            const bool in = i < nt;
            float4 p;
            p.x = in ? TX[i] : NN_FAR;
            p.y = in ? TY[i] : NN_FAR;
            p.z = (DIM == 3) ? (in ? TZ[i] : NN_FAR) : 0.f;
            p.w = 0.f;
            tile[l] = p;
        }
        __syncthreads();
        const int cnt = min(NN_TILE, (nt - t0 + 7) & ~7);   // whole groups of 8: the padding targets fill the last one
#pragma unroll 8
        for (int k = 0; k < cnt; ++k) {
            const float4 p = tile[k];
#pragma unroll
            for (int j = 0; j < NN_QPL; ++j) {
                const float dx = qx[j] - p.x, dy = qy[j] - p.y;
                float d = fmaf(dy, dy, dx * dx);
                if (DIM == 3) {
                    const float dz = qz[j] - p.z;
                    d = fmaf(dz, dz, d);
                }
                m[j] = fminf(m[j], d);
            }
        }
    }
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NN_QPL; ++j)
        if (q0 + j * NN_THREADS + tid < nq) s += sqrt((double)m[j]);
    red[tid] = s;
    __syncthreads();
#pragma unroll
    for (int w = NN_THREADS / 2; w > 0; w >>= 1) {    // fixed tree
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) *slot = red[0];
}

__global__ void eval_nn_final_kernel(const double* __restrict__ slots, const int* __restrict__ table, int n_chunks, int B,
                                     double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double e = 0.0;
    for (int dir = 0; dir < 2; ++dir) {
        const int nq = table[(size_t)b * TB_LD + (dir == 0 ? 3 : 1)];
        const double* s = slots + ((size_t)b * 2 + dir) * n_chunks;
        double a = 0.0;
        for (int c = 0; c < n_chunks; ++c) a += s[c];
        e += nq > 0 ? a / (double)nq : __builtin_nan("");      // np.mean(min_y_to_x) + np.mean(min_x_to_y) (pose_error.py:181)
    }
    out[b] = e;
}

// ---- c. depth compare ----------------------------------------------------------------------------------------------------------------
// misc.depth_im_to_dist_im_fast (misc.py:136-167): pre_X = (x - K[0,2]) / K[0,0] in float64, dist = sqrt((pre_X d)^2 + (pre_Y d)^2 + d^2)
__device__ __forceinline__ double dist_of(double pre_x, double pre_y, float depth) {
    const double d = (double)depth;
    const double a = pre_x * d, b = pre_y * d;
    return __dsqrt_rn(a * a + b * b + d * d);
}

struct PixelCounts {
    int inter = 0, uni = 0, vinter = 0, vuni = 0;
    int cost[FP_EVAL_MAX_TAUS] = {};
};

template <bool VSD>
__device__ __forceinline__ void eval_pixel(float de, float dg, float dt, int pix, int W, const double* prm, float delta, const double* taus,
                                           int n_tau, PixelCounts& c) {
    const bool me = de > 0.f, mg = dg > 0.f;          // pose_error.py:376-379
    c.inter += (me && mg) ? 1 : 0;
    c.uni += (me || mg) ? 1 : 0;
    if (!VSD) return;
    const int y = pix / W, x = pix - y * W;
    const double pre_x = ((double)x - prm[2]) / prm[0], pre_y = ((double)y - prm[3]) / prm[1];
    const double dist_t = dist_of(pre_x, pre_y, dt), dist_g = dist_of(pre_x, pre_y, dg), dist_e = dist_of(pre_x, pre_y, de);
    const float ft = (float)dist_t, fg = (float)dist_g, fe = (float)dist_e;   // .astype(np.float32), visibility.py:35
    // visibility._estimate_visib_mask, mode bop19 (:34-38)
    const bool vg = ((fg - ft) <= delta || dist_t == 0.0) && dist_g > 0.0;
    bool ve = ((fe - ft) <= delta || dist_t == 0.0) && dist_e > 0.0;
    ve = ve || (vg && dist_e > 0.0);                  // estimate_visib_mask_est (:74-75)
    const bool vi = vg && ve, vu = vg || ve;
    c.vinter += vi ? 1 : 0;
    c.vuni += vu ? 1 : 0;
    if (vi) {
        const double dd = fabs(dist_g - dist_e) / prm[5];     // dists /= diameter; prm[5] = 1.0 without the normalisation (x / 1.0 == x)
#pragma unroll
        for (int k = 0; k < FP_EVAL_MAX_TAUS; ++k)
            if (k < n_tau) c.cost[k] += (dd >= taus[k]) ? 1 : 0;   // costs = dists >= tau (pose_error.py:102)
    }
}

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int mk = 32; mk > 0; mk >>= 1) v += __shfl_xor(v, mk, 64);
    return v;
}

// grid (pixel blocks, pair); out i32 [B, 4 + n_tau] zeroed by the launcher: inter, union, visib_inter, visib_union, cost counts
template <bool VSD>
__global__ __launch_bounds__(256) void eval_depth_compare_kernel(const float* __restrict__ d_est, const float* __restrict__ d_gt,
                                                                 const float* __restrict__ d_test, const int* __restrict__ img_idx, int n_img,
                                                                 const double* __restrict__ params, const double* __restrict__ taus,
                                                                 int n_tau, int HW, int W, int vec4, int* __restrict__ out) {
    __shared__ int acc[4 + FP_EVAL_MAX_TAUS];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < 4 + FP_EVAL_MAX_TAUS) acc[tid] = 0;
    __syncthreads();
    const float* E = d_est + (size_t)b * HW;
    const float* G = d_gt + (size_t)b * HW;
    const float* T = nullptr;
    double prm[6] = {1, 1, 0, 0, 0, 1};
    float delta = 0.f;
    double tau[FP_EVAL_MAX_TAUS];
    bool ok = true;
    if (VSD) {
        const int im = img_idx[b];
        ok = im >= 0 && im < n_img;                   // block-uniform
        T = d_test + (size_t)(ok ? im : 0) * HW;
#pragma unroll
        for (int k = 0; k < 6; ++k) prm[k] = params[(size_t)b * 8 + k];
        delta = (float)prm[4];                        // numpy compares the float32 difference image with the scalar in float32
#pragma unroll
        for (int k = 0; k < FP_EVAL_MAX_TAUS; ++k) tau[k] = k < n_tau ? taus[k] : 0.0;
    }
    PixelCounts c;
    if (ok) {
        if (vec4) {                                   // 16 bytes per lane: HW % 4 == 0 and 16-byte aligned stacks (the launcher checks)
            const int n4 = HW >> 2;
            for (int i = blockIdx.x * 256 + tid; i < n4; i += gridDim.x * 256) {
                const float4 e = reinterpret_cast<const float4*>(E)[i], g = reinterpret_cast<const float4*>(G)[i];
                float4 t = {0.f, 0.f, 0.f, 0.f};
                if (VSD) t = reinterpret_cast<const float4*>(T)[i];
                eval_pixel<VSD>(e.x, g.x, t.x, 4 * i, W, prm, delta, tau, n_tau, c);
                eval_pixel<VSD>(e.y, g.y, t.y, 4 * i + 1, W, prm, delta, tau, n_tau, c);
                eval_pixel<VSD>(e.z, g.z, t.z, 4 * i + 2, W, prm, delta, tau, n_tau, c);
                eval_pixel<VSD>(e.w, g.w, t.w, 4 * i + 3, W, prm, delta, tau, n_tau, c);
            }
        } else {
            for (int i = blockIdx.x * 256 + tid; i < HW; i += gridDim.x * 256)
                eval_pixel<VSD>(E[i], G[i], VSD ? T[i] : 0.f, i, W, prm, delta, tau, n_tau, c);
        }
    }
    const bool lead = (tid & 63) == 0;
    int v;
    v = wave_sum_i32(c.inter);  if (lead && v) atomicAdd(&acc[0], v);
    v = wave_sum_i32(c.uni);    if (lead && v) atomicAdd(&acc[1], v);
    if (VSD) {
        v = wave_sum_i32(c.vinter); if (lead && v) atomicAdd(&acc[2], v);
        v = wave_sum_i32(c.vuni);   if (lead && v) atomicAdd(&acc[3], v);
#pragma unroll
        for (int k = 0; k < FP_EVAL_MAX_TAUS; ++k) {
            if (k < n_tau) {
                v = wave_sum_i32(c.cost[k]);
                if (lead && v) atomicAdd(&acc[4 + k], v);
            }
        }
    }
    __syncthreads();
    if (tid < 4 + n_tau && acc[tid]) atomicAdd(&out[(size_t)b * (4 + n_tau) + tid], acc[tid]);   // integers: the order does not matter
}

}  // namespace

int fp_chamfer_launch(const double* pts, int n_pts, const int* table, const double* xf, int B, int max_n, int ws_pts, int projected,
                      float* ws, double* slots, double* out, hipStream_t s) {
    const int n_chunks = cdiv(max_n, NN_QCHUNK);
    const dim3 gp(cdiv(max_n, 256), 2, B), gn(n_chunks, 2, B);
    if (projected) {
        hipLaunchKernelGGL(eval_prep_kernel<2>, gp, dim3(256), 0, s, pts, n_pts, table, xf, ws_pts, ws);
        hipLaunchKernelGGL(eval_nn_kernel<2>, gn, dim3(NN_THREADS), 0, s, ws, ws_pts, n_pts, table, n_chunks, slots);
    } else {
        hipLaunchKernelGGL(eval_prep_kernel<3>, gp, dim3(256), 0, s, pts, n_pts, table, xf, ws_pts, ws);
        hipLaunchKernelGGL(eval_nn_kernel<3>, gn, dim3(NN_THREADS), 0, s, ws, ws_pts, n_pts, table, n_chunks, slots);
    }
    hipLaunchKernelGGL(eval_nn_final_kernel, dim3(cdiv(B, 64)), dim3(64), 0, s, slots, table, n_chunks, B, out);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

int fp_chamfer_chunks(int max_n) { return cdiv(max_n, NN_QCHUNK); }

int fp_depth_compare_launch(const float* d_est, const float* d_gt, int B, int Hh, int W, const float* d_test, int n_img, const int* img_idx,
                            const double* params, const double* taus, int n_tau, int* out, hipStream_t s) {
    const int HW = Hh * W;
    FP_HIP(hipMemsetAsync(out, 0, (size_t)B * (4 + n_tau) * sizeof(int), s));
    const dim3 grid(std::max(1, std::min(cdiv(HW, 1024), 64)), B);
    const int vec4 = (HW & 3) == 0 && (((uintptr_t)d_est | (uintptr_t)d_gt | (uintptr_t)d_test) & 15) == 0;   // else the scalar loop
    if (d_test)
        hipLaunchKernelGGL(eval_depth_compare_kernel<true>, grid, dim3(256), 0, s, d_est, d_gt, d_test, img_idx, n_img, params, taus, n_tau, HW,
                           W, vec4, out);
    else
        hipLaunchKernelGGL(eval_depth_compare_kernel<false>, grid, dim3(256), 0, s, d_est, d_gt, d_test, img_idx, n_img, params, taus, 0, HW, W,
                           vec4, out);
    FP_LAUNCH_CHECK();
    return FP_OK;
}
