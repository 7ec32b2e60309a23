// refine.hip — the host arithmetic of the reference's TrackingRefiner on the device, batched over the frames of a tracking interval:
//
//   fp_patch_points   TrackingRefiner._compute_3d_points (src/pipeline/estimators/tracking_refiner.py:102-130): which surface sample
//                     stands for each 14 x 14 patch cell.
//     patch_project_kernel   one thread per (item, sample): projection in the documented fp64 operation order -> cell (floor(u / patch),
//                            floor(v / patch)) as doubles (NaN: the sample belongs to no cell), d^2 to the cell centre, camera depth Zc.
//     patch_select_kernel    one workgroup per (cell, item): members counted (and listed in LDS when there are at most LIST_CAP of them,
//                            else every pass scans all S keys), the q = ceil(m / 4) smallest by (d^2, sample index) found EXACTLY by a
//                            radix select on the 96-bit key (bits of d^2, index) — keys are unique, so there are no ties to break —
//                            and among those the minimum by (Zc, d^2, index).  Integer LDS atomics only (histograms, list slots); the
//                            result does not depend on their order.
//
//   fp_pnp_epnp       cv2.solvePnP(..., SOLVEPNP_EPNP) (tracking_refiner.py:173, scripts/smooth_poses_video.py:182), one workgroup of
//                     256 threads per problem.  Point-parallel phases (centroid, scatter, barycentrics + the sums of M^T M, camera-frame
//                     centroids, Horn's 3 x 3 sums, reprojection errors of the three candidates) run across the workgroup: thread t adds
//                     points t, t + 256, ... in order, then a fixed tree in LDS.  The small dense phases (pnp_core.h) run in one thread
//                     (the two eigen-solvers) or three (one per candidate).  fp64 throughout, no floating-point atomics: two calls give
//                     the same bits, and a problem's result does not depend on its neighbours in the batch.
//
// Compiled with -ffp-contract=off: the projection is the reference's operation sequence.
#include "internal.h"
#include "pnp_core.h"

namespace {

constexpr int T = FP_PNP_LANES;         // threads of the EPnP workgroup = accumulation lanes of its sums
constexpr int SEL_T = 256;              // threads of patch_select_kernel: one per bin of its 8-bit radix histogram
constexpr int LIST_CAP = 1024;
static_assert(SEL_T == 256, "patch_select_kernel clears and fills a 256-bin histogram with one thread per bin");

// ---- fp_patch_points -------------------------------------------------------------------------------------------------------------------
// ws [B][4][S] doubles: cell x, cell y, d^2, Zc
__global__ __launch_bounds__(256) void patch_project_kernel(const double* __restrict__ samples, int S, const double* __restrict__ Tm,
                                                            const double* __restrict__ Km, double patch, double* __restrict__ ws) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= S) return;
    const double* Tb = Tm + (size_t)b * 16;
    const double* Kb = Km + (size_t)b * 9;
    const double x = samples[(size_t)i * 3], y = samples[(size_t)i * 3 + 1], z = samples[(size_t)i * 3 + 2];
    const double Xc = ((Tb[0] * x + Tb[1] * y) + Tb[2] * z) + Tb[3];
    const double Yc = ((Tb[4] * x + Tb[5] * y) + Tb[6] * z) + Tb[7];
    const double Zc = ((Tb[8] * x + Tb[9] * y) + Tb[10] * z) + Tb[11];
    const double up = (Kb[0] * Xc + Kb[1] * Yc) + Kb[2] * Zc;
    const double vp = (Kb[3] * Xc + Kb[4] * Yc) + Kb[5] * Zc;
    const double wp = (Kb[6] * Xc + Kb[7] * Yc) + Kb[8] * Zc;
    const double u = up / wp, v = vp / wp;
    const double a = u / patch, c = v / patch, fa = floor(a), fc = floor(c);
    const double dx = (a - fa) - 0.5, dy = (c - fc) - 0.5;
    const bool ok = isfinite(u) && isfinite(v);
    double* w = ws + (size_t)b * 4 * S;
    w[i] = ok ? fa : __builtin_nan("");
    w[(size_t)S + i] = ok ? fc : __builtin_nan("");
    w[(size_t)2 * S + i] = dx * dx + dy * dy;
    w[(size_t)3 * S + i] = Zc;
}

struct SelSh {
    int list[LIST_CAP];
    int hist[256];
    int cnt;
    int pick[2];
    double bz[SEL_T];
    unsigned long long bd[SEL_T];
    int bi[SEL_T];
};

__global__ __launch_bounds__(SEL_T) void patch_select_kernel(const double* __restrict__ ws, int S, const int* __restrict__ cells,
                                                         const int* __restrict__ ncells, int C, int* __restrict__ out) {
    __shared__ SelSh sh;
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    int* dst = out + (size_t)b * C + c;
    if (c >= ncells[b]) {                                   // block-uniform
        if (t == 0) *dst = -1;
        return;
    }
    const double* cxs = ws + (size_t)b * 4 * S;
    const double* cys = cxs + S;
    const double* d2s = cxs + (size_t)2 * S;
    const double* zcs = cxs + (size_t)3 * S;
    const double qx = (double)cells[((size_t)b * C + c) * 2], qy = (double)cells[((size_t)b * C + c) * 2 + 1];
    if (t == 0) sh.cnt = 0;
    __syncthreads();
    for (int i = t; i < S; i += SEL_T)
        if (cxs[i] == qx && cys[i] == qy) {
            const int slot = atomicAdd(&sh.cnt, 1);
            if (slot < LIST_CAP) sh.list[slot] = i;
        }
    __syncthreads();
    const int m = sh.cnt;
    if (m == 0) {                                           // block-uniform
        if (t == 0) *dst = -1;
        return;
    }
    const bool listed = m <= LIST_CAP;
    const auto for_members = [&](auto f) {
        if (listed) {
            for (int j = t; j < m; j += SEL_T) f(sh.list[j]);
        } else {
            for (int i = t; i < S; i += SEL_T)
                if (cxs[i] == qx && cys[i] == qy) f(i);
        }
    };
    // d^2 >= +0 and finite for every member: its bit pattern orders like its value
    const auto dkey = [&](int i) { return (unsigned long long)__double_as_longlong(d2s[i]); };
    int k = (m + 3) / 4 - 1;                                // rank (0-based) of the last member kept: q = ceil(m / 4)
    const auto pick_bucket = [&]() {
        __syncthreads();
        if (t == 0) {
            int acc = 0, bkt = 0;
            for (; bkt < 255; ++bkt) {
                if (acc + sh.hist[bkt] > k) break;
                acc += sh.hist[bkt];
            }
            sh.pick[0] = bkt;
            sh.pick[1] = acc;
        }
        __syncthreads();
        k -= sh.pick[1];
        return (unsigned long long)sh.pick[0];
    };
    unsigned long long dstar = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();
        sh.hist[t] = 0;
        __syncthreads();
        const unsigned long long hi = shift == 56 ? 0ull : (~0ull << (shift + 8));
        for_members([&](int i) {
            const unsigned long long kk = dkey(i);
            if ((kk & hi) == dstar) atomicAdd(&sh.hist[(int)((kk >> shift) & 255)], 1);
        });
        dstar |= pick_bucket() << shift;
    }
    unsigned istar = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        __syncthreads();
        sh.hist[t] = 0;
        __syncthreads();
        const unsigned hi = shift == 24 ? 0u : (~0u << (shift + 8));
        for_members([&](int i) {
            if (dkey(i) == dstar && ((unsigned)i & hi) == istar) atomicAdd(&sh.hist[(int)(((unsigned)i >> shift) & 255)], 1);
        });
        istar |= (unsigned)pick_bucket() << shift;
    }
    // among the kept members, the minimum by (Zc, d^2, index)
    double bz = 0.0;
    unsigned long long bd = 0;
    int bi = -1;
    const auto less = [](double z1, unsigned long long d1, int i1, double z2, unsigned long long d2, int i2) {
        if (i2 < 0) return i1 >= 0;
        if (i1 < 0) return false;
        if (z1 != z2) return z1 < z2;
        if (d1 != d2) return d1 < d2;
        return i1 < i2;
    };
    for_members([&](int i) {
        const unsigned long long kk = dkey(i);
        if (kk < dstar || (kk == dstar && (unsigned)i <= istar)) {
            const double z = zcs[i];
            if (less(z, kk, i, bz, bd, bi)) { bz = z; bd = kk; bi = i; }
        }
    });
    sh.bz[t] = bz; sh.bd[t] = bd; sh.bi[t] = bi;
    __syncthreads();
    for (int w = SEL_T / 2; w > 0; w >>= 1) {
        if (t < w && less(sh.bz[t + w], sh.bd[t + w], sh.bi[t + w], sh.bz[t], sh.bd[t], sh.bi[t])) {
            sh.bz[t] = sh.bz[t + w]; sh.bd[t] = sh.bd[t + w]; sh.bi[t] = sh.bi[t + w];
        }
        __syncthreads();
    }
    if (t == 0) *dst = sh.bi[0];
}

// ---- fp_pnp_epnp ---------------------------------------------------------------------------------------------------------------------------
constexpr int RK = 10;                 // sums reduced per round

struct PnpSh {
    double red[RK][T];
    double S[FP_PNP_NSUM];
    double work[FP_PNP_WORK];
    double v[4][12];
    double cc[3][4][3];
    double pc0[3][3];
    double R[3][9];
    double t[3][3];
    PnpCtrl ctrl;
    int n, status;
};

// vals[0..K) of every thread -> their sums over the block in the fixed tree order, on every thread
template <int K>
__device__ __forceinline__ void block_sums(double (&vals)[K], PnpSh& sh) {
    static_assert(K <= RK, "one round");
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) sh.red[k][t] = vals[k];
    __syncthreads();
    for (int w = T / 2; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh.red[k][t] = sh.red[k][t] + sh.red[k][t + w];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) vals[k] = sh.red[k][0];
}

__global__ __launch_bounds__(T) void pnp_epnp_kernel(const double* __restrict__ pts3d, const double* __restrict__ pts2d,
                                                     const uint8_t* __restrict__ vis, const double* __restrict__ K9, int N,
                                                     double* __restrict__ out) {
    __shared__ PnpSh sh;
    const int b = blockIdx.x, t = threadIdx.x;
    const double* p2 = pts2d + (size_t)b * N * 2;
    const uint8_t* vb = vis ? vis + (size_t)b * N : nullptr;
    double* o = out + (size_t)b * 16;
    double K[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) K[k] = K9[k];
    const auto used = [&](int i) { return !vb || vb[i] != 0; };
    // used points (integers below 2^53: exact in any order)
    {
        double c[1] = {0.0};
        for (int i = t; i < N; i += T) c[0] += used(i) ? 1.0 : 0.0;
        block_sums(c, sh);
        if (t == 0) { sh.n = (int)c[0]; sh.status = (int)c[0] < 4 ? FP_PNP_FEW : FP_PNP_OK; }
    }
    __syncthreads();
    const int n = sh.n;
    if (sh.status) {                                       // block-uniform
        if (t == 0) pnp_write(o, nullptr, nullptr, 0.0, n, sh.status);
        return;
    }
    double mu[3];
    {
        double s[3] = {0.0, 0.0, 0.0};
        for (int i = t; i < N; i += T)
            if (used(i)) { s[0] += pts3d[i * 3]; s[1] += pts3d[i * 3 + 1]; s[2] += pts3d[i * 3 + 2]; }
        block_sums(s, sh);
#pragma unroll
        for (int k = 0; k < 3; ++k) mu[k] = s[k] / (double)n;
    }
    {
        double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = t; i < N; i += T)
            if (used(i)) {
                const double x = pts3d[i * 3] - mu[0], y = pts3d[i * 3 + 1] - mu[1], z = pts3d[i * 3 + 2] - mu[2];
                c[0] += x * x; c[1] += x * y; c[2] += x * z; c[3] += y * y; c[4] += y * z; c[5] += z * z;
            }
        block_sums(c, sh);
        if (t == 0) sh.status = pnp_control_points(mu, c, n, sh.ctrl);
    }
    __syncthreads();
    if (sh.status) {                                       // block-uniform
        if (t == 0) pnp_write(o, nullptr, nullptr, 0.0, n, sh.status);
        return;
    }
    {
        double acc[FP_PNP_NSUM];
#pragma unroll
        for (int k = 0; k < FP_PNP_NSUM; ++k) acc[k] = 0.0;
        for (int i = t; i < N; i += T)
            if (used(i)) {
                double a[4], x, y;
                pnp_alphas(sh.ctrl, pts3d + i * 3, a);
                pnp_normalise(K, p2[i * 2], p2[i * 2 + 1], x, y);
                pnp_accum_mtm(a, x, y, acc);
            }
#pragma unroll
        for (int r = 0; r < FP_PNP_NSUM / RK; ++r) {
            double part[RK];
#pragma unroll
            for (int k = 0; k < RK; ++k) part[k] = acc[r * RK + k];
            block_sums(part, sh);
            if (t == 0) {
#pragma unroll
                for (int k = 0; k < RK; ++k) sh.S[r * RK + k] = part[k];
            }
        }
    }
    __syncthreads();
    if (t == 0) pnp_null_vectors(sh.S, sh.work, sh.v);
    __syncthreads();
    if (t < 3) pnp_candidate(sh.v, sh.ctrl, t, sh.cc[t]);
    __syncthreads();
    // camera-frame centroids of the three candidates; the sign that puts the points in front of the camera
    {
        double s[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) s[k] = 0.0;
        for (int i = t; i < N; i += T)
            if (used(i)) {
                double a[4], pc[3];
                pnp_alphas(sh.ctrl, pts3d + i * 3, a);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    pnp_camera_point(sh.cc[c], a, pc);
                    s[c * 3] += pc[0]; s[c * 3 + 1] += pc[1]; s[c * 3 + 2] += pc[2];
                }
            }
        block_sums(s, sh);
        __syncthreads();
        if (t < 3) {
            const double sgn = s[t * 3 + 2] < 0.0 ? -1.0 : 1.0;
            for (int j = 0; j < 3; ++j) sh.pc0[t][j] = sgn * (s[t * 3 + j] / (double)n);
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 3; ++j) sh.cc[t][i][j] = sgn * sh.cc[t][i][j];
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        double h[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) h[k] = 0.0;
        for (int i = t; i < N; i += T)
            if (used(i)) {
                double a[4], pc[3];
                pnp_alphas(sh.ctrl, pts3d + i * 3, a);
                pnp_camera_point(sh.cc[c], a, pc);
#pragma unroll
                for (int j = 0; j < 3; ++j)
#pragma unroll
                    for (int k = 0; k < 3; ++k) h[j * 3 + k] += (pc[j] - sh.pc0[c][j]) * (pts3d[i * 3 + k] - mu[k]);
            }
        block_sums(h, sh);
        if (t == 0) pnp_horn(h, sh.pc0[c], mu, sh.R[c], sh.t[c]);
    }
    __syncthreads();
    double e[3] = {0.0, 0.0, 0.0};
    for (int i = t; i < N; i += T)
        if (used(i)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) e[c] += pnp_reproj(K, sh.R[c], sh.t[c], pts3d + i * 3, p2[i * 2], p2[i * 2 + 1]);
        }
    block_sums(e, sh);
    if (t == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) e[c] = e[c] / (double)n;
        const int best = pnp_choose(e);
        pnp_write(o, sh.R[best], sh.t[best], e[best], n, FP_PNP_OK);
    }
}

}  // namespace

int fp_patch_points_launch(const double* samples, int S, const double* Tm, const double* Km, const int* cells, const int* ncells, int B, int C,
                           double patch, double* ws, int* out, hipStream_t s) {
    hipLaunchKernelGGL(patch_project_kernel, dim3(cdiv(S, 256), B), dim3(256), 0, s, samples, S, Tm, Km, patch, ws);
    hipLaunchKernelGGL(patch_select_kernel, dim3(C, B), dim3(SEL_T), 0, s, ws, S, cells, ncells, C, out);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

int fp_pnp_epnp_launch(const double* pts3d, const double* pts2d, const uint8_t* vis, const double* K9, int B, int N, double* out,
                       hipStream_t s) {
    hipLaunchKernelGGL(pnp_epnp_kernel, dim3(B), dim3(T), 0, s, pts3d, pts2d, vis, K9, N, out);
    FP_LAUNCH_CHECK();
    return FP_OK;
}
