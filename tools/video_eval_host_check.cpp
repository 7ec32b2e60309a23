// video_eval_host_check — runs freepose_amd/csrc/video_eval_core.h serially in the order of video_eval.hip's kernels: the alignment with
// its 256 accumulation lanes and tree, the (offset, pair, symmetry) errors with the four waves' sums added in wave order, the final
// numbers.  Plain C++ with its own main: build it with
//     g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I freepose_amd/csrc tools/video_eval_host_check.cpp
// and compare its output with the numpy restatement (tests/test_video_eval_cpu.py).  This is the part of the video scorer that can be
// debugged on a machine without a GPU.
//
//   video_eval_host_check errors IN OUT
//     input : int32 {M, V, D}; per video int32 N, float64 [N,12] (R[9] row-major, t[3]);
//             per track int32 meta[20] (video, n_frames, n_sym, flags, dt[16]), float64 params[16] (est_scale, gt_scale, w, h,
//             sym_axis[3], K[9]), float64 est [n_frames,12]
//     output: per track float64 per_offset[D,3], final[3], {kept frames, origin[3]}, aligned t [n_frames,3]
//   video_eval_host_check so3 IN OUT
//     input : int32 n, float64 R [n,9]      output: per matrix float64 {log R [3], exp(log R) [9]}
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "video_eval_core.h"

namespace {
bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
bool put(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

int run_so3(FILE* fi, FILE* fo) {
    int32_t n = 0;
    if (!get(fi, &n, 4) || n < 0) return 3;
    for (int i = 0; i < n; ++i) {
        double R[9], out[12];
        if (!get(fi, R, sizeof R)) return 3;
        ve_so3_log(R, out);
        ve_so3_exp(out, out + 3);
        if (!put(fo, out, sizeof out)) return 4;
    }
    return 0;
}

// one track in the kernels' order -> out: per_offset[D,3], final[3], kept, origin[3], aligned [N,3]
void score(const int32_t* mt, const double* pr, const double* est, const double* gt, int D, std::vector<double>& out) {
    const int N = mt[1];
    const double scale = pr[0];
    // ve_align_kernel
    std::vector<double> lanes(4 * FP_VE_LANES, 0.0);
    for (int t = 0; t < FP_VE_LANES; ++t)
        for (int i = t; i < N; i += FP_VE_LANES) {
            double o[3];
            ve_frame_origin(est + (size_t)i * 12, est + (size_t)i * 12 + 9, gt + (size_t)i * 12 + 9, o);
            if (ve_norm3(o) < scale) {
                lanes[t] += 1.0;
                for (int k = 0; k < 3; ++k) lanes[(k + 1) * FP_VE_LANES + t] += o[k];
            }
        }
    double red[4];
    for (int k = 0; k < 4; ++k) red[k] = ve_tree_sum(&lanes[(size_t)k * FP_VE_LANES]);
    const int kept = (mt[3] & FP_VE_NO_ALIGN) ? 0 : (int)red[0];
    double o[3] = {0.0, 0.0, 0.0};
    if (kept > 0) ve_mean_origin(red + 1, kept, scale, o);
    double K[9];
    if (mt[3] & FP_VE_HAS_K) memcpy(K, pr + 7, sizeof K);
    else ve_default_K(pr[2], pr[3], K);
    std::vector<double> aligned((size_t)N * 3), frames((size_t)N * FP_VE_FRAME_LD);
    for (int i = 0; i < N; ++i) {
        const double* Re = est + (size_t)i * 12;
        double te[3] = {Re[9], Re[10], Re[11]};
        if (kept > 0) ve_move_origin(Re, Re + 9, o, te);
        for (int k = 0; k < 3; ++k) aligned[(size_t)i * 3 + k] = te[k];
        double* f = &frames[(size_t)i * FP_VE_FRAME_LD];
        ve_project(K, te, f);
        f[2] = ve_norm3(te);
        ve_project(K, gt + (size_t)i * 12 + 9, f + 3);
        f[5] = ve_norm3(gt + (size_t)i * 12 + 9);
    }
    // ve_errors_kernel
    const bool has_axis = (mt[3] & FP_VE_HAS_AXIS) != 0;
    const int n_sym = has_axis ? mt[2] : 1;
    std::vector<double> per_offset((size_t)D * 3);
    for (int d = 0; d < D; ++d) {
        const int dt = mt[4 + d], npairs = N - dt;
        double wsum[3][FP_VE_WAVES] = {};
        for (int wave = 0; wave < FP_VE_WAVES; ++wave)
            for (int t1 = wave; t1 < npairs; t1 += FP_VE_WAVES) {
                const int t2 = t1 + dt;
                double a[3];
                ve_rel_log(est + (size_t)t2 * 12, est + (size_t)t1 * 12, a);
                double e = INFINITY;
                if (has_axis) {
                    for (int k = 0; k < n_sym; ++k) {          // a minimum does not depend on the order it is taken in
                        double S[9];
                        ve_sym(pr + 4, ve_sym_angle(k, n_sym), S);
                        e = fmin(e, ve_rot_err(a, gt + (size_t)t2 * 12, S, gt + (size_t)t1 * 12));
                    }
                } else {
                    e = ve_rot_err(a, gt + (size_t)t2 * 12, nullptr, gt + (size_t)t1 * 12);
                }
                const double* f1 = &frames[(size_t)t1 * FP_VE_FRAME_LD];
                const double* f2 = &frames[(size_t)t2 * FP_VE_FRAME_LD];
                wsum[0][wave] += e;
                wsum[1][wave] += ve_proj_err(f1, f2, f1 + 3, f2 + 3);
                wsum[2][wave] += ve_depth_err(f1[2], f2[2], pr[0], f1[5], f2[5], pr[1]);
            }
        for (int k = 0; k < 3; ++k) per_offset[(size_t)d * 3 + k] = ve_offset_mean(wsum[k], npairs, dt);
    }
    // ve_final_kernel
    double fin[3];
    ve_final(per_offset.data(), D, pr[2], pr[3], fin);
    out = per_offset;
    out.insert(out.end(), fin, fin + 3);
    out.push_back((double)kept);
    out.insert(out.end(), o, o + 3);
    out.insert(out.end(), aligned.begin(), aligned.end());
}

int run_errors(FILE* fi, FILE* fo) {
    int32_t hdr[3];
    if (!get(fi, hdr, sizeof hdr)) return 3;
    const int M = hdr[0], V = hdr[1], D = hdr[2];
    if (M < 0 || V < 1 || V > 4096 || D < 1 || D > FP_VE_MAX_D) return 3;
    std::vector<std::vector<double>> gts(V);
    for (int v = 0; v < V; ++v) {
        int32_t n = 0;
        if (!get(fi, &n, 4) || n < FP_VE_MIN_N || n > (1 << 20)) return 3;
        gts[v].resize((size_t)n * 12);
        if (!get(fi, gts[v].data(), gts[v].size() * 8)) return 3;
    }
    for (int m = 0; m < M; ++m) {
        int32_t mt[FP_VE_META_LD];
        double pr[FP_VE_PARAM_LD];
        if (!get(fi, mt, sizeof mt) || !get(fi, pr, sizeof pr)) return 3;
        // the limits of fp_video_errors
        if (mt[0] < 0 || mt[0] >= V || mt[1] < FP_VE_MIN_N || (size_t)mt[1] * 12 != gts[mt[0]].size()) return 3;
        if (mt[2] < 1 || mt[2] > FP_VE_MAX_SYM) return 3;
        for (int d = 0; d < D; ++d)
            if (mt[4 + d] < 1 || mt[4 + d] > mt[1] - 1) return 3;
        std::vector<double> est((size_t)mt[1] * 12), out;
        if (!get(fi, est.data(), est.size() * 8)) return 3;
        score(mt, pr, est.data(), gts[mt[0]].data(), D, out);
        if (!put(fo, out.data(), out.size() * 8)) return 4;
    }
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 4 || (strcmp(argv[1], "errors") && strcmp(argv[1], "so3"))) {
        fprintf(stderr, "usage: video_eval_host_check errors|so3 IN OUT\n");
        return 2;
    }
    FILE* fi = fopen(argv[2], "rb");
    FILE* fo = fopen(argv[3], "wb");
    if (!fi || !fo) {
        fprintf(stderr, "video_eval_host_check: cannot open files\n");
        return 2;
    }
    const int rc = strcmp(argv[1], "so3") ? run_errors(fi, fo) : run_so3(fi, fo);
    fclose(fi);
    if (fclose(fo) != 0) return 4;
    return rc;
}
