// fp_video_errors — the video velocity errors of the reference's src/utils/video_evaluation.py for M tracks against V ground-truth
// trajectories in one call (scripts/eval_videos.py scores 32 videos x 6 methods with a triple Python loop: offset x frame pair x 101
// symmetries).  All fp64 vector code on the arithmetic of video_eval_core.h; every sum is taken in a fixed order and there is no atomic, so
// two calls give the same bits.
//
//   ve_align_kernel    one workgroup of 256 per track.  Lane t adds the kept frame origins of frames t, t + 256, ... (align_object_origins
//                      :112-140), a fixed tree sums the lanes, every thread forms the clamped mean and the workgroup writes the moved
//                      translations (change_object_origin :151-155) and the frame table the error kernel reads: pi(t) and |t| of the
//                      aligned estimate and of the ground truth.
//   ve_errors_kernel   one workgroup of 4 waves per (offset, track).  Wave w takes the pairs t1 = w, w + 4, ...; log(R2e R1e^T) does not
//                      depend on the symmetry and is computed once per pair; lane l takes the symmetries l, l + 64, ... (101 = two
//                      passes, the second with a masked tail), the wave minimum goes over DPP / permlane moves, and the three errors
//                      are added to wave-uniform sums in pair order.  Wave sums meet in LDS and are added in wave order.
//   ve_final_kernel    one thread per track: the mean over the offsets, rot in degrees, proj in percent of the image diagonal.
//
// Occupancy: the error kernel is VALU-bound fp64 (sincos, atan2 and two 3 x 3 products per symmetry) with no LDS traffic in the loop.
// hipcc gives it 119 VGPRs and no scratch: 4 waves per SIMD, i.e. four workgroups per CU; a table of 192 tracks x 10 offsets is 1920
// workgroups, 7.5 per CU.  The alignment kernel (62 VGPRs, 8 KiB LDS) and the final kernel are a few microseconds of work.
#include "internal.h"
#include "video_eval_core.h"

namespace {
constexpr int T = FP_VE_LANES;
static_assert(T == FP_VE_WAVES * FP_WAVE, "four waves");

template <int MASK>
__device__ __forceinline__ double lane_xor_f64(double v) {
    const long long b = __double_as_longlong(v);
    const float lo = lane_xor<MASK>(__int_as_float((int)(b & 0xffffffffll)));
    const float hi = lane_xor<MASK>(__int_as_float((int)(b >> 32)));
    return __longlong_as_double(((long long)__float_as_int(hi) << 32) | (unsigned int)__float_as_int(lo));
}
__device__ __forceinline__ double wave_min_f64(double v) {
    v = fmin(v, lane_xor_f64<32>(v));
    v = fmin(v, lane_xor_f64<16>(v));
    v = fmin(v, lane_xor_f64<8>(v));
    v = fmin(v, lane_xor_f64<4>(v));
    v = fmin(v, lane_xor_f64<2>(v));
    v = fmin(v, lane_xor_f64<1>(v));
    return v;
}

__global__ __launch_bounds__(T) void ve_align_kernel(const double* __restrict__ est, const double* __restrict__ gt,
                                                     const int* __restrict__ meta, const double* __restrict__ params, int Nmax,
                                                     double* __restrict__ aligned, double* __restrict__ frames) {
    __shared__ double red[4][T];
    const int m = blockIdx.x, t = threadIdx.x;
    const int* mt = meta + (size_t)m * FP_VE_META_LD;
    const double* pr = params + (size_t)m * FP_VE_PARAM_LD;
    const int N = mt[1];
    const double* pe = est + (size_t)m * Nmax * 12;
    const double* pg = gt + (size_t)mt[0] * Nmax * 12;
    const double scale = pr[0];
    double s[4] = {0.0, 0.0, 0.0, 0.0};                      // kept frames (an integer below 2^53: exact), sum of their origins
    for (int i = t; i < N; i += T) {
        double o[3];
        ve_frame_origin(pe + (size_t)i * 12, pe + (size_t)i * 12 + 9, pg + (size_t)i * 12 + 9, o);
        if (ve_norm3(o) < scale) { s[0] += 1.0; s[1] += o[0]; s[2] += o[1]; s[3] += o[2]; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) red[k][t] = s[k];
    __syncthreads();
    for (int w = T / 2; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int k = 0; k < 4; ++k) red[k][t] = red[k][t] + red[k][t + w];
        }
        __syncthreads();
    }
    const int kept = (mt[3] & FP_VE_NO_ALIGN) ? 0 : (int)red[0][0];
    double o[3] = {0.0, 0.0, 0.0};
    if (kept > 0) {
        const double sum[3] = {red[1][0], red[2][0], red[3][0]};
        ve_mean_origin(sum, kept, scale, o);
    }
    double K[9];
    if (mt[3] & FP_VE_HAS_K) {
#pragma unroll
        for (int k = 0; k < 9; ++k) K[k] = pr[7 + k];
    } else {
        ve_default_K(pr[2], pr[3], K);
    }
    for (int i = t; i < N; i += T) {
        const double* Re = pe + (size_t)i * 12;
        double te[3] = {Re[9], Re[10], Re[11]};
        if (kept > 0) ve_move_origin(Re, Re + 9, o, te);
        double* a = aligned + ((size_t)m * Nmax + i) * 3;
        a[0] = te[0]; a[1] = te[1]; a[2] = te[2];
        double* f = frames + ((size_t)m * Nmax + i) * FP_VE_FRAME_LD;
        double u[2];
        ve_project(K, te, u);
        f[0] = u[0]; f[1] = u[1]; f[2] = ve_norm3(te);
        const double* tg = pg + (size_t)i * 12 + 9;
        ve_project(K, tg, u);
        f[3] = u[0]; f[4] = u[1]; f[5] = ve_norm3(tg);
    }
}

__global__ __launch_bounds__(T) void ve_errors_kernel(const double* __restrict__ est, const double* __restrict__ gt,
                                                      const int* __restrict__ meta, const double* __restrict__ params,
                                                      const double* __restrict__ frames, int Nmax, int D,
                                                      double* __restrict__ per_offset, double* __restrict__ pairs_out) {
    __shared__ double wsum[3][FP_VE_WAVES];
    const int d = blockIdx.x, m = blockIdx.y;
    const int lane = threadIdx.x & (FP_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int* mt = meta + (size_t)m * FP_VE_META_LD;
    const double* pr = params + (size_t)m * FP_VE_PARAM_LD;
    const int N = mt[1], dt = mt[4 + d];
    const bool has_axis = (mt[3] & FP_VE_HAS_AXIS) != 0;
    const int n_sym = has_axis ? mt[2] : 1;
    const double se = pr[0], sg = pr[1];
    const double axis[3] = {pr[4], pr[5], pr[6]};
    const double* pe = est + (size_t)m * Nmax * 12;
    const double* pg = gt + (size_t)mt[0] * Nmax * 12;
    const double* fr = frames + (size_t)m * Nmax * FP_VE_FRAME_LD;
    const int npairs = N - dt;                               // >= 1: the entry checked 1 <= dt <= N - 1
    double acc[3] = {0.0, 0.0, 0.0};
    for (int t1 = wave; t1 < npairs; t1 += FP_VE_WAVES) {
        const int t2 = t1 + dt;
        const double* R1e = pe + (size_t)t1 * 12;
        const double* R2e = pe + (size_t)t2 * 12;
        const double* R1g = pg + (size_t)t1 * 12;
        const double* R2g = pg + (size_t)t2 * 12;
        double a[3];
        ve_rel_log(R2e, R1e, a);
        double e = INFINITY;
        if (has_axis) {
            for (int k = lane; k < n_sym; k += FP_WAVE) {
                double S[9];
                ve_sym(axis, ve_sym_angle(k, n_sym), S);
                e = fmin(e, ve_rot_err(a, R2g, S, R1g));
            }
            e = wave_min_f64(e);
        } else {
            e = ve_rot_err(a, R2g, nullptr, R1g);
        }
        const double* f1 = fr + (size_t)t1 * FP_VE_FRAME_LD;
        const double* f2 = fr + (size_t)t2 * FP_VE_FRAME_LD;
        const double ep = ve_proj_err(f1, f2, f1 + 3, f2 + 3);
        const double ed = ve_depth_err(f1[2], f2[2], se, f1[5], f2[5], sg);
        acc[0] += e; acc[1] += ep; acc[2] += ed;
        if (pairs_out && lane == 0) {
            double* po = pairs_out + (((size_t)m * D + d) * Nmax + t1) * 3;
            po[0] = e; po[1] = ep; po[2] = ed;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) wsum[k][wave] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) per_offset[((size_t)m * D + d) * 3 + threadIdx.x] = ve_offset_mean(wsum[threadIdx.x], npairs, dt);
}

__global__ void ve_final_kernel(const double* __restrict__ per_offset, const double* __restrict__ params, int M, int D,
                                double* __restrict__ final_out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const double* pr = params + (size_t)m * FP_VE_PARAM_LD;
    ve_final(per_offset + (size_t)m * D * 3, D, pr[2], pr[3], final_out + (size_t)m * 3);
}
}  // namespace

int fp_video_errors_launch(const double* est, const double* gt, const int* meta, const double* params, int M, int Nmax, int D,
                           double* aligned, double* frames, double* per_offset, double* final_out, double* pairs_out, hipStream_t s) {
    hipLaunchKernelGGL(ve_align_kernel, dim3(M), dim3(T), 0, s, est, gt, meta, params, Nmax, aligned, frames);
    hipLaunchKernelGGL(ve_errors_kernel, dim3(D, M), dim3(T), 0, s, est, gt, meta, params, frames, Nmax, D, per_offset, pairs_out);
    hipLaunchKernelGGL(ve_final_kernel, dim3(cdiv(M, 64)), dim3(64), 0, s, per_offset, params, M, D, final_out);
    FP_LAUNCH_CHECK();
    return FP_OK;
}
