// video_eval_core.h — the arithmetic of video_eval.hip as plain __host__ __device__ fp64 functions: the SO(3) log and exp maps, the three
// per-pair velocity errors of the reference's src/utils/video_evaluation.py:37-109 (relative rotation with the symmetry sweep, projected
// translation, depth), the object-origin alignment of :112-155 and the fixed reduction trees.  No HIP type appears here, so the same text
// compiles with g++ into tools/video_eval_host_check.cpp, which runs the kernels' phases serially (under -fsanitize=address,undefined).
//
// Thresholds of the two maps (theta = rotation angle, v = 1/2 vee(R - R^T) = sin(theta) n, c = (tr R - 1) / 2 = cos(theta)):
//   FP_VE_SMALL = 1e-3   below it theta / sin(theta), sin(theta) / theta and (1 - cos(theta)) / theta^2 are their series up to theta^4:
//                        the first dropped term is < theta^6 / 487 = 2e-21 relative, far under the fp64 rounding of the kept ones.
//   FP_VE_NEAR_PI = 1e-2 log only: with c < 0 and |v| < 1e-2 (theta > pi - 0.010000167) the axis is not v / |v| — theta / sin(theta)
//                        multiplies the rounding error of v by up to pi / |v|, 7 digits lost at pi - 1e-9 and a division by 0 at pi —
//                        but comes from the symmetric part (R + R^T) / 2 = c I + (1 - c) n n^T, where 1 - c ~ 2: the largest n_i is
//                        sqrt((S_ii - c) / (1 - c)) >= 0.577, the other two are S_ij / ((1 - c) n_i), n is renormalised, and its sign is
//                        the one that makes n . v > 0 (v == 0, i.e. theta == pi exactly where n and -n are the same rotation: the
//                        largest component is positive).  Below the threshold the plain formula loses at most pi / 1e-2 = 314 ulps.
// The angle is atan2(|v|, c) in [0, pi] on every branch (acos(c) alone loses half the digits near 0 and pi), and every branch is finite
// for every orthonormal R.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef FP_HD
#if defined(__HIPCC__)
#define FP_HD __host__ __device__ __forceinline__
#else
#define FP_HD inline
#endif
#endif

#define FP_VE_LANES 256        // accumulation lanes of the alignment's sums over frames: lane t adds frames t, t + 256, ... in order, then a tree
#define FP_VE_WAVES 4          // waves of the error kernel's workgroup: wave w adds pairs w, w + 4, ... in order, then wave 0 + 1 + 2 + 3
#define FP_VE_MAX_D 16         // time offsets per track
#define FP_VE_MAX_SYM 1024     // symmetry grid points
#define FP_VE_MIN_N 2          // frames per track
#define FP_VE_META_LD 20       // int32 per track: video, n_frames, n_sym, flags, dts[16]
#define FP_VE_PARAM_LD 16      // fp64 per track: est_scale, gt_scale, w, h, sym_axis[3], K[9]
#define FP_VE_FRAME_LD 6       // fp64 per frame of the frame table: pi(t_est aligned)[2], |t_est aligned|, pi(t_gt)[2], |t_gt|
#define FP_VE_HAS_AXIS 1       // flags: sym_axis is given (otherwise S = I and n_sym is not used)
#define FP_VE_HAS_K 2          // flags: K is given (otherwise f = sqrt(w^2 + h^2), c = (w / 2, h / 2))
#define FP_VE_NO_ALIGN 4       // flags: score the translations as given (get_translation_errors_* on their own)
#define FP_VE_PI 3.141592653589793
#define FP_VE_SMALL 1e-3
#define FP_VE_NEAR_PI 1e-2

FP_HD double ve_norm3(const double* x) { return sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]); }

// C = A B (row-major 3 x 3)
FP_HD void ve_mul(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}
// C = A B^T
FP_HD void ve_mul_abt(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i * 3] * B[j * 3] + A[i * 3 + 1] * B[j * 3 + 1]) + A[i * 3 + 2] * B[j * 3 + 2];
}

// rotation vector of R, angle in [0, pi] (see the head of the file)
FP_HD void ve_so3_log(const double* R, double* w) {
    const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double s = ve_norm3(v);
    const double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double th = atan2(s, c);
    if (c < 0.0 && s < FP_VE_NEAR_PI) {
        const double omc = 1.0 - c;
        const double d[3] = {R[0] - c, R[4] - c, R[8] - c};                    // (1 - c) n_i^2
        const double o01 = 0.5 * (R[1] + R[3]), o02 = 0.5 * (R[2] + R[6]), o12 = 0.5 * (R[5] + R[7]);   // (1 - c) n_i n_j
        double n[3];
        if (d[0] >= d[1] && d[0] >= d[2]) {
            n[0] = sqrt(fmax(d[0], 0.0) / omc);
            n[1] = o01 / (omc * n[0]);
            n[2] = o02 / (omc * n[0]);
        } else if (d[1] >= d[2]) {
            n[1] = sqrt(fmax(d[1], 0.0) / omc);
            n[0] = o01 / (omc * n[1]);
            n[2] = o12 / (omc * n[1]);
        } else {
            n[2] = sqrt(fmax(d[2], 0.0) / omc);
            n[0] = o02 / (omc * n[2]);
            n[1] = o12 / (omc * n[2]);
        }
        const double len = ve_norm3(n);
        const double dot = (n[0] * v[0] + n[1] * v[1]) + n[2] * v[2];
        const double k = (dot < 0.0 ? -th : th) / len;
        w[0] = k * n[0]; w[1] = k * n[1]; w[2] = k * n[2];
        return;
    }
    double k;
    if (th < FP_VE_SMALL) {
        const double t2 = th * th;
        k = 1.0 + t2 * (1.0 / 6.0 + t2 * (7.0 / 360.0));
    } else {
        k = th / s;
    }
    w[0] = k * v[0]; w[1] = k * v[1]; w[2] = k * v[2];
}

// Rodrigues: R = I + A [w]x + B [w]x^2, A = sin(theta) / theta, B = (1 - cos(theta)) / theta^2 = 1/2 (sin(theta / 2) / (theta / 2))^2
FP_HD void ve_so3_exp(const double* w, double* R) {
    const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double th = sqrt(t2);
    double A, B;
    if (th < FP_VE_SMALL) {
        A = 1.0 - t2 * (1.0 / 6.0 - t2 * (1.0 / 120.0));
        B = 0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0));
    } else {
        const double h = sin(0.5 * th) / (0.5 * th);
        A = sin(th) / th;
        B = 0.5 * (h * h);
    }
    const double x = w[0], y = w[1], z = w[2];
    R[0] = 1.0 - B * (y * y + z * z); R[1] = B * (x * y) - A * z;       R[2] = B * (x * z) + A * y;
    R[3] = B * (x * y) + A * z;       R[4] = 1.0 - B * (x * x + z * z); R[5] = B * (y * z) - A * x;
    R[6] = B * (x * z) - A * y;       R[7] = B * (y * z) + A * x;       R[8] = 1.0 - B * (x * x + y * y);
}

// numpy.linspace(-pi, pi, n)[k]: start + k * step, the last point is the stop itself
FP_HD double ve_sym_angle(int k, int n) {
    if (n > 1 && k == n - 1) return FP_VE_PI;
    if (k == 0) return -FP_VE_PI;
    return (double)k * ((FP_VE_PI - (-FP_VE_PI)) / (double)(n - 1)) + (-FP_VE_PI);
}
// S = exp(sym_axis * a); the axis is used as given (video_evaluation.py:50 does not normalise it)
FP_HD void ve_sym(const double* axis, double a, double* S) {
    const double w[3] = {axis[0] * a, axis[1] * a, axis[2] * a};
    ve_so3_exp(w, S);
}
// a = log(R2 R1^T): the estimate's side of rot_error_in_cframe (:61), the same for every symmetry
FP_HD void ve_rel_log(const double* R2, const double* R1, double* a) {
    double M[9];
    ve_mul_abt(R2, R1, M);
    ve_so3_log(M, a);
}
// |a - log((R2g S) R1g^T)| (:54, :60-63); S == nullptr stands for the identity
FP_HD double ve_rot_err(const double* a, const double* R2g, const double* S, const double* R1g) {
    double G[9], b[3];
    if (S) {
        ve_mul(R2g, S, G);
        ve_rel_log(G, R1g, b);
    } else {
        ve_rel_log(R2g, R1g, b);
    }
    const double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
    return ve_norm3(d);
}

FP_HD void ve_default_K(double w, double h, double* K) {
    const double f = sqrt(w * w + h * h);
    K[0] = f; K[1] = 0.0; K[2] = w / 2.0;
    K[3] = 0.0; K[4] = f; K[5] = h / 2.0;
    K[6] = 0.0; K[7] = 0.0; K[8] = 1.0;
}
// project (:100-109): (K x)[:2] / (K x)[2]
FP_HD void ve_project(const double* K, const double* x, double* u) {
    const double a = (K[0] * x[0] + K[1] * x[1]) + K[2] * x[2];
    const double b = (K[3] * x[0] + K[4] * x[1]) + K[5] * x[2];
    const double c = (K[6] * x[0] + K[7] * x[1]) + K[8] * x[2];
    u[0] = a / c;
    u[1] = b / c;
}
// get_translation_errors_proj (:87-95) on projected points
FP_HD double ve_proj_err(const double* p1e, const double* p2e, const double* p1g, const double* p2g) {
    const double dx = (p2e[0] - p1e[0]) - (p2g[0] - p1g[0]), dy = (p2e[1] - p1e[1]) - (p2g[1] - p1g[1]);
    return sqrt(dx * dx + dy * dy);
}
// get_translation_errors_depth (:73-76) on the norms of the translations
FP_HD double ve_depth_err(double n1e, double n2e, double se, double n1g, double n2g, double sg) {
    return fabs((n1e / se - n2e / se) - (n1g / sg - n2g / sg));
}

// align_object_origins (:118-124), one frame: where the ground-truth origin, pushed along its ray to the estimate's distance, lies in the
// estimate's object frame
FP_HD void ve_frame_origin(const double* Re, const double* te, const double* tg, double* o) {
    const double ng = ve_norm3(tg), ne = ve_norm3(te);
    const double d[3] = {tg[0] / ng * ne - te[0], tg[1] / ng * ne - te[1], tg[2] / ng * ne - te[2]};
    for (int j = 0; j < 3; ++j) o[j] = (Re[j] * d[0] + Re[3 + j] * d[1]) + Re[6 + j] * d[2];       // R^T d
}
// :127-136: mean of the kept origins, its length limited to scale / 2.  kept == 0: no change (the caller leaves the poses alone)
FP_HD void ve_mean_origin(const double* sum, int kept, double scale, double* o) {
    for (int j = 0; j < 3; ++j) o[j] = sum[j] / (double)kept;
    const double norm = ve_norm3(o), max_change = scale / 2.0;
    if (norm > max_change)
        for (int j = 0; j < 3; ++j) o[j] = o[j] / norm * max_change;
}
// change_object_origin (:151-155): translation of pose * SE3(I, o)
FP_HD void ve_move_origin(const double* Re, const double* te, const double* o, double* out) {
    for (int i = 0; i < 3; ++i) out[i] = ((Re[i * 3] * o[0] + Re[i * 3 + 1] * o[1]) + Re[i * 3 + 2] * o[2]) + te[i];
}

// the fixed tree over the alignment's lanes: the pairing of video_eval.hip's block reduction
FP_HD double ve_tree_sum(double* v) {
    for (int w = FP_VE_LANES / 2; w > 0; w >>= 1)
        for (int t = 0; t < w; ++t) v[t] = v[t] + v[t + w];
    return v[0];
}
// per-offset mean of one metric: the four waves' sums in wave order, / pairs, / dt (get_average_*_errors_dt: np.mean(e) / dt)
FP_HD double ve_offset_mean(const double* wave_sums, int pairs, int dt) {
    const double s = ((wave_sums[0] + wave_sums[1]) + wave_sums[2]) + wave_sums[3];
    return s / (double)pairs / (double)dt;
}
// the final numbers of a track from its [D,3] per-offset means (eval_videos.py:195-205): mean over the offsets; rot in degrees, proj in
// percent of the image diagonal
FP_HD void ve_final(const double* per_offset, int D, double w, double h, double* out) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < D; ++d)
        for (int k = 0; k < 3; ++k) s[k] += per_offset[d * 3 + k];
    out[0] = s[0] / (double)D * (180.0 / FP_VE_PI);
    out[1] = s[1] / (double)D / sqrt(w * w + h * h) * 100.0;
    out[2] = s[2] / (double)D;
}
