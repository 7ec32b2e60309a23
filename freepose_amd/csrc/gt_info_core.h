// The arithmetic of fp_gt_visibility and fp_pts_diameter (gt_info.hip) as __host__ __device__ functions, so that
// tools/gt_info_host_check.cpp can run exactly what the kernels run, serially, under the host sanitizers.  Reproduces, per pixel,
// bop_toolkit/scripts/calc_gt_info.py:131-152 / calc_gt_masks.py:107-115 (misc.depth_im_to_dist_im_fast misc.py:146-167,
// visibility._estimate_visib_mask mode bop19 visibility.py:34-38) and, per point pair, misc.calc_pts_diameter (misc.py:289-303).
// Every float64 the reference forms is formed by the same operations in the same order (both compilers run with -ffp-contract=off: no
// FMA appears that numpy would not execute); everything else is comparisons and integers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FP_GI_HD __host__ __device__ __forceinline__
#else
#define FP_GI_HD inline
#endif

#define FP_GI_OUT_LD 12       // d_out row of fp_gt_visibility: {all, valid, visib, 0, box of the silhouette [4], box of the visible mask [4]}
#define FP_GI_PARAM_LD 8      // d_params row: {fx, fy, cx, cy, delta, 0, 0, 0}
#define FP_GI_DIAM_LD 8       // d_out row of fp_pts_diameter: {diameter, min x, y, z, size x, y, z, 0}
#define FP_GI_BOX_EMPTY_MIN INT32_MAX    // what the launcher writes into the minima / maxima: a box that no pixel has touched
#define FP_GI_BOX_EMPTY_MAX INT32_MIN
#define FP_GI_MASK 1          // gi_classify bits: dist_gt > 0
#define FP_GI_VALID 2         //                   dist_gt > 0 and dist_test > 0
#define FP_GI_VISIB 4         //                   on the bop19 visibility mask

// IEEE square root: sqrt() of the host's libm and the device's correctly rounded instruction sequence give the same bits
FP_GI_HD double gi_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(x);
#else
    return sqrt(x);
#endif
}

// misc.depth_im_to_dist_im_fast: pre_X = (x - K[0,2]) / K[0,0], dist = sqrt((pre_X d)^2 + (pre_Y d)^2 + d^2), all float64
FP_GI_HD double gi_pre(int x, double c, double f) { return ((double)x - c) / f; }
FP_GI_HD double gi_dist(double pre_x, double pre_y, float depth) {
    const double d = (double)depth;
    const double a = pre_x * d, b = pre_y * d;
    return gi_sqrt(a * a + b * b + d * d);
}

// One pixel of the image: rendered depth dg, test depth dt -> FP_GI_MASK | FP_GI_VALID | FP_GI_VISIB.  The float32 difference of the
// two distances is compared with delta in float32, as numpy does for a float32 array and a Python scalar.
FP_GI_HD int gi_classify(float dg, float dt, double pre_x, double pre_y, float delta) {
    const double dist_g = gi_dist(pre_x, pre_y, dg), dist_t = gi_dist(pre_x, pre_y, dt);
    if (!(dist_g > 0.0)) return 0;
    const float diff = (float)dist_g - (float)dist_t;             // .astype(np.float32) of both, visibility.py:35
    int bits = FP_GI_MASK;
    if (dist_t > 0.0) bits |= FP_GI_VALID;                        // np.sum(dist_im[obj_mask_gt] > 0), calc_gt_info.py:149
    if (diff <= delta || dist_t == 0.0) bits |= FP_GI_VISIB;      // visibility.py:36-38
    return bits;
}

// canvas pixel (x, y) lies in the image window [ox, ox + W) x [oy, oy + H)
FP_GI_HD bool gi_in_window(int x, int y, int ox, int oy, int W, int H) { return x >= ox && x < ox + W && y >= oy && y < oy + H; }

// box = {min x, min y, max x, max y}, empty = {FP_GI_BOX_EMPTY_MIN, .., FP_GI_BOX_EMPTY_MAX, ..}
FP_GI_HD void gi_box_update(int32_t* box, int x, int y) {
    box[0] = x < box[0] ? x : box[0];
    box[1] = y < box[1] ? y : box[1];
    box[2] = x > box[2] ? x : box[2];
    box[3] = y > box[3] ? y : box[3];
}

// what one lane (or the serial host run) gathers over its pixels of one instance
struct GiAcc {
    int all = 0, valid = 0, visib = 0;
    int32_t box_all[4] = {FP_GI_BOX_EMPTY_MIN, FP_GI_BOX_EMPTY_MIN, FP_GI_BOX_EMPTY_MAX, FP_GI_BOX_EMPTY_MAX};
    int32_t box_vis[4] = {FP_GI_BOX_EMPTY_MIN, FP_GI_BOX_EMPTY_MIN, FP_GI_BOX_EMPTY_MAX, FP_GI_BOX_EMPTY_MAX};
};

// canvas pixel (x, y) with rendered depth dg; inw = it lies in the window, then dt is the test depth under it; prm = {fx, fy, cx, cy} of
// the image.  Returns the gi_classify bits of a window pixel, 0 elsewhere.
FP_GI_HD int gi_pixel(float dg, float dt, bool inw, int x, int y, int ox, int oy, const double* prm, float delta, GiAcc& a) {
    if (dg > 0.f) {                                   // obj_mask_gt_large = depth_gt_large > 0 (calc_gt_info.py:140)
        a.all += 1;
        gi_box_update(a.box_all, x - ox, y - oy);
    }
    if (!inw || dg == 0.f) return 0;                  // depth 0 -> distance 0: off the mask, neither valid nor visible
    const int ix = x - ox, iy = y - oy;
    const int bits = gi_classify(dg, dt, gi_pre(ix, prm[2], prm[0]), gi_pre(iy, prm[3], prm[1]), delta);
    a.valid += (bits & FP_GI_VALID) ? 1 : 0;
    if (bits & FP_GI_VISIB) {
        a.visib += 1;
        gi_box_update(a.box_vis, ix, iy);
    }
    return bits;
}

// squared distance of one pair, (dx dx + dy dy) + dz dz: the order in which (pts_diff * pts_diff).sum(axis=1) adds the three columns
FP_GI_HD double gi_pair_d2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// ---- bounds predicates (the C entries refuse what fails them; the kernels skip it) ---------------------------------------------------
FP_GI_HD bool gi_window_ok(int Wr, int Hr, int ox, int oy, int W, int H) {
    return W > 0 && H > 0 && ox >= 0 && oy >= 0 && (int64_t)ox + W <= Wr && (int64_t)oy + H <= Hr;
}
FP_GI_HD bool gi_img_ok(int img, int n_img) { return img >= 0 && img < n_img; }
FP_GI_HD bool gi_range_ok(int first, int count, int n_pts) { return first >= 0 && count > 0 && (int64_t)first + count <= n_pts; }
