// The arithmetic of fp_bop_scores (bop_score.hip) as __host__ __device__ functions, so that tools/bop_score_host_check.cpp can run exactly
// what the kernel runs, serially, under the host sanitizers.  Reproduces bop_toolkit_lib/pose_matching.py match_poses (:39-87) for
// one-element errors and the target count of score.py calc_localization_scores (:77-99).  Comparisons and integer sums only: the host
// has sorted the estimates by score, cut them to n_top and normalised the errors while packing, so every answer is exact.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FP_BS_HD __host__ __device__ __forceinline__
#else
#define FP_BS_HD inline
#endif

#define FP_BS_GROUP_LD 4   // d_groups row: {err_offset, E, G, first_gt_row}

// Greedy matching of one group under one threshold.  err [E,G] row-major: rows = estimates in matching order (score descending, ties in
// file order, cut to n_top), columns = the group's ground truths in visiting order; valid [G]; match [G] holds -1 on entry and is both
// the result (row of the estimate matched to each ground truth) and the "already matched" marker.  An estimate takes the valid,
// unmatched ground truth with the lowest error strictly below th; equal errors go to the column visited first; NaN compares false and
// never matches.
FP_BS_HD void bs_match_group(const double* err, int E, int G, const uint8_t* valid, double th, int32_t* match) {
    for (int e = 0; e < E; ++e) {
        int best = -1;
        double best_err = th;
        for (int g = 0; g < G; ++g) {
            if (!valid[g] || match[g] >= 0) continue;
            const double x = err[(int64_t)e * G + g];
            if (x < best_err) {
                best = g;
                best_err = x;
            }
        }
        if (best >= 0) match[best] = e;
    }
}

// Targets of one group = its valid ground truths, at most n_top of them when n_top > 0 (score.py:92-95).
FP_BS_HD int bs_group_targets(const uint8_t* valid, int G, int n_top) {
    int n = 0;
    for (int g = 0; g < G; ++g) n += valid[g] ? 1 : 0;
    return (n_top > 0 && n > n_top) ? n_top : n;
}

// True positives of one group under one threshold: matched ground truths (only valid ones can be matched).
FP_BS_HD int bs_group_tp(const int32_t* match, int G) {
    int n = 0;
    for (int g = 0; g < G; ++g) n += match[g] >= 0 ? 1 : 0;
    return n;
}

// A group's row of d_groups stays inside the tables: the kernel skips a group that does not (the entry's callers check the host twins
// of the tables and refuse such a table with a message before anything is launched).
FP_BS_HD bool bs_group_in_bounds(const int32_t* grp, int64_t P, int R) {
    const int64_t off = grp[0], E = grp[1], G = grp[2], first = grp[3];
    return off >= 0 && E >= 0 && G >= 0 && first >= 0 && first + G <= R && off <= P && E * G <= P - off;
}
