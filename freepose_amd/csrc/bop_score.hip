// fp_bop_scores — pose matching and recall counts of the BOP toolkit (bop_toolkit_lib/pose_matching.py match_poses, score.py
// calc_localization_scores) for every (scene, image, object) group of an errors directory and ALL T thresholds in one call.  The
// reference's driver starts one process per (error type, threshold) and walks nested dicts; here the host packs one table and the
// device does comparisons and integer sums only (bop_score_core.h), so every answer is exact and does not depend on the launch shape.
//
//   bs_match_kernel   one thread per (group, threshold), the thresholds of a group in adjacent lanes: the lanes of a group read the same
//                     error and validity addresses (one request, broadcast).  The thread walks its E x G block serially and uses its own
//                     slice d_match[t, first_gt_row .. + G) as the "already matched" marker: no cap on G, no LDS.  It then adds the
//                     group's true positives to d_tp_obj / d_tp_scene [t, .] and, for t == 0, the group's targets to d_tar_obj /
//                     d_tar_scene with integer atomics — integer addition commutes, so two calls give the same bits.
//
// d_match is set to -1 and the counts to 0 by memsets in stream order before the kernel.  A table of ycbv-test size is about 4 k groups x
// 30 thresholds = 120 k threads with E x G around 5 x 1: the whole call including upload and download measures 0.4 ms
// (profiles/bop_scores.md) and nothing here is tuned (hipcc: 30 VGPRs, no scratch, no LDS).
#include "internal.h"
#include "bop_score_core.h"

namespace {
constexpr int BS_THREADS = 256;

__global__ __launch_bounds__(BS_THREADS) void bs_match_kernel(const double* __restrict__ err, const int32_t* __restrict__ groups,
                                                              const uint8_t* __restrict__ gt_valid, const int32_t* __restrict__ gt_obj,
                                                              const int32_t* __restrict__ gt_scene, const double* __restrict__ th, int P,
                                                              int Gr, int R, int T, int n_obj, int n_scene, int n_top,
                                                              int32_t* __restrict__ match, int32_t* __restrict__ tp_obj,
                                                              int32_t* __restrict__ tp_scene, int32_t* __restrict__ tar_obj,
                                                              int32_t* __restrict__ tar_scene) {
    const int64_t tid = (int64_t)blockIdx.x * BS_THREADS + threadIdx.x;
    if (tid >= (int64_t)Gr * T) return;
    const int g = (int)(tid / T), t = (int)(tid % T);
    const int32_t* grp = groups + (size_t)g * FP_BS_GROUP_LD;
    if (!bs_group_in_bounds(grp, P, R)) return;
    const int E = grp[1], G = grp[2], first = grp[3];
    if (G == 0) return;                                      // no ground truth: nothing to match, no target
    const uint8_t* valid = gt_valid + first;
    int32_t* m = match + (size_t)t * R + first;
    bs_match_group(err + grp[0], E, G, valid, th[t], m);
    const int obj = gt_obj[first], scene = gt_scene[first];  // one object and one scene per group
    if (obj < 0 || obj >= n_obj || scene < 0 || scene >= n_scene) return;
    const int tp = bs_group_tp(m, G);
    if (tp) {
        atomicAdd(tp_obj + (size_t)t * n_obj + obj, tp);
        atomicAdd(tp_scene + (size_t)t * n_scene + scene, tp);
    }
    if (t == 0) {
        const int tar = bs_group_targets(valid, G, n_top);
        if (tar) {
            atomicAdd(tar_obj + obj, tar);
            atomicAdd(tar_scene + scene, tar);
        }
    }
}
}  // namespace

int fp_bop_scores_launch(const double* err, const int32_t* groups, const uint8_t* gt_valid, const int32_t* gt_obj, const int32_t* gt_scene,
                         const double* th, int P, int Gr, int R, int T, int n_obj, int n_scene, int n_top, int32_t* match, int32_t* tp_obj,
                         int32_t* tp_scene, int32_t* tar_obj, int32_t* tar_scene, hipStream_t s) {
    if (R > 0) FP_HIP(hipMemsetAsync(match, 0xff, (size_t)T * R * sizeof(int32_t), s));       // every byte 0xff: int32 -1
    FP_HIP(hipMemsetAsync(tp_obj, 0, (size_t)T * n_obj * sizeof(int32_t), s));
    FP_HIP(hipMemsetAsync(tp_scene, 0, (size_t)T * n_scene * sizeof(int32_t), s));
    FP_HIP(hipMemsetAsync(tar_obj, 0, (size_t)n_obj * sizeof(int32_t), s));
    FP_HIP(hipMemsetAsync(tar_scene, 0, (size_t)n_scene * sizeof(int32_t), s));
    if (Gr == 0 || R == 0) return FP_OK;
    const int64_t threads = (int64_t)Gr * T;
    hipLaunchKernelGGL(bs_match_kernel, dim3((unsigned)((threads + BS_THREADS - 1) / BS_THREADS)), dim3(BS_THREADS), 0, s, err, groups, gt_valid,
                       gt_obj, gt_scene, th, P, Gr, R, T, n_obj, n_scene, n_top, match, tp_obj, tp_scene, tar_obj, tar_scene);
    FP_LAUNCH_CHECK();
    return FP_OK;
}
