// lk_core.h — the per-sample and per-point arithmetic of lk_track.hip's pyramidal Lucas-Kanade tracker (Bouguet, "Pyramidal
// Implementation of the Lucas Kanade Feature Tracker", 2000) as plain __host__ __device__ functions: grey value, pyramid tap, clamp,
// bilinear sample, window pixel with its gradient, the terms of G and b, the guard, the solve, the smaller eigenvalue, and the fixed
// order in which the 64 lane sums are combined.  No HIP type appears here, so the same text compiles with g++ into
// tools/lk_host_check.cpp, which runs the tracker serially in the kernel's order (under -fsanitize=address,undefined).
//
// The pyramid is fp32, every expression written out in one order, and the build contracts nothing into FMAs (-ffp-contract=off), so it
// equals a float32 numpy restatement bit for bit (tests/_lk_ref.py).  The tracker samples that pyramid and does everything else in fp64,
// chain positions included (a float32 tracker drifts from a float64 restatement by a rounding per step and more where a window's texture
// is weak: 6e-4 px over twelve frames of the mesh clip), so it differs from the float64 restatement by the order of its sums and by
// the one rounding of each stored float32 result.  This is a classical stand-in for a learned point tracker, not a port of one.
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

#define FP_LK_MAX_LEVELS 8
#define FP_LK_MAX_RADIUS 15
#define FP_LK_MAX_ITERS 64
#define FP_LK_MAX_SIDE 16384      // H and W: a level's pixel index stays far inside int32
#define FP_LK_LANES 64            // window pixel k belongs to lane k % 64, slot k / 64
#define FP_LK_EIG_FLOOR 1e-4      // guard: a level whose smaller eigenvalue of G per window pixel is below this contributes no update
// flags of a chain step (diagnostics column 3, as a float): why the step is not good
#define FP_LK_FLAG_FB 1           // forward-backward distance above fb_thresh (or not a number)
#define FP_LK_FLAG_EIG 2          // smaller eigenvalue / window pixels below min_eig
#define FP_LK_FLAG_RESIDUAL 4     // mean |A - B| above max_residual
#define FP_LK_FLAG_OUTSIDE 8      // forward result (or the query itself) outside [0, W-1] x [0, H-1]
#define FP_LK_FLAG_LOST_BEFORE 16 // the previous frame of the chain was not visible (loss is sticky)

// levels back to back, level l = [T, h[l], w[l]] float32 starting at float off[l]
struct LkPyramid {
    int levels, T;
    int h[FP_LK_MAX_LEVELS], w[FP_LK_MAX_LEVELS];
    long long off[FP_LK_MAX_LEVELS];
};

// level sizes h_l = (h_{l-1} + 1) / 2; a level whose smaller side is below 2 r + 1 is dropped (and every coarser one), level 0 stays.
// Returns the number of floats of the whole pyramid.
FP_HD long long lk_pyramid_layout(int T, int H, int W, int levels, int radius, LkPyramid& p) {
    p.T = T;
    p.levels = 1;
    p.h[0] = H;
    p.w[0] = W;
    p.off[0] = 0;
    long long total = (long long)T * H * W;
    for (int l = 1; l < FP_LK_MAX_LEVELS; ++l) {
        p.h[l] = p.w[l] = 0;
        p.off[l] = 0;
    }
    for (int l = 1; l < levels && l < FP_LK_MAX_LEVELS; ++l) {
        const int h = (p.h[l - 1] + 1) / 2, w = (p.w[l - 1] + 1) / 2;
        if ((h < w ? h : w) < 2 * radius + 1) break;
        p.h[l] = h;
        p.w[l] = w;
        p.off[l] = total;
        total += (long long)T * h * w;
        p.levels = l + 1;
    }
    return total;
}

FP_HD float lk_grey(int r, int g, int b) { return (float)((77 * r + 150 * g + 29 * b + 128) >> 8); }

// [1 4 6 4 1] / 16
FP_HD float lk_tap5(float a, float b, float c, float d, float e) { return (((a + e) + 4.0f * (b + d)) + 6.0f * c) * 0.0625f; }

FP_HD int lk_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// pixel (y, x) of the next level: rows filtered first (along x), then columns, replicate border, centred on (2 y, 2 x)
FP_HD float lk_down_pixel(const float* src, int hs, int ws, int y, int x) {
    float r[5];
    const int c0 = lk_clampi(2 * x - 2, ws - 1), c1 = lk_clampi(2 * x - 1, ws - 1), c2 = lk_clampi(2 * x, ws - 1),
              c3 = lk_clampi(2 * x + 1, ws - 1), c4 = lk_clampi(2 * x + 2, ws - 1);
    for (int j = 0; j < 5; ++j) {
        const float* row = src + (long long)lk_clampi(2 * y - 2 + j, hs - 1) * ws;
        r[j] = lk_tap5(row[c0], row[c1], row[c2], row[c3], row[c4]);
    }
    return lk_tap5(r[0], r[1], r[2], r[3], r[4]);
}

// into [0, hi]; anything that is not >= 0 (NaN included) becomes 0, so no coordinate can address memory outside an image
FP_HD double lk_clamp(double v, double hi) {
    if (!(v >= 0.0)) v = 0.0;
    if (v > hi) v = hi;
    return v;
}

FP_HD double lk_sample(const float* img, int w, int h, double x, double y) {
    x = lk_clamp(x, (double)(w - 1));
    y = lk_clamp(y, (double)(h - 1));
    const int x0 = (int)x, y0 = (int)y;                 // x, y >= 0: truncation is floor
    const int x1 = x0 + 1 < w ? x0 + 1 : w - 1, y1 = y0 + 1 < h ? y0 + 1 : h - 1;
    const double fx = x - (double)x0, fy = y - (double)y0;
    const double a = img[y0 * w + x0], b = img[y0 * w + x1], c = img[y1 * w + x0], d = img[y1 * w + x1];
    const double top = a + fx * (b - a), bot = c + fx * (d - c);
    return top + fy * (bot - top);
}

// window pixel k of the (2 r + 1)^2 window around (px, py): value and half central differences of bilinear samples at +-1 pixel
FP_HD void lk_window_pixel(const float* A, int w, int h, double px, double py, int k, int r, double& a, double& ix, double& iy) {
    const int win = 2 * r + 1;
    const double x = px + (double)(k % win - r), y = py + (double)(k / win - r);
    a = lk_sample(A, w, h, x, y);
    ix = 0.5 * (lk_sample(A, w, h, x + 1.0, y) - lk_sample(A, w, h, x - 1.0, y));
    iy = 0.5 * (lk_sample(A, w, h, x, y + 1.0) - lk_sample(A, w, h, x, y - 1.0));
}

// B at window pixel k around p + (g + v)
FP_HD double lk_moved_sample(const float* B, int w, int h, double px, double py, double gx, double gy, double vx, double vy, int k, int r) {
    const int win = 2 * r + 1;
    return lk_sample(B, w, h, (px + (gx + vx)) + (double)(k % win - r), (py + (gy + vy)) + (double)(k / win - r));
}

FP_HD void lk_g_terms(double ix, double iy, double& gxx, double& gxy, double& gyy) {
    gxx = gxx + ix * ix;
    gxy = gxy + ix * iy;
    gyy = gyy + iy * iy;
}

FP_HD void lk_b_terms(double a, double b, double ix, double iy, double& bx, double& by) {
    const double d = a - b;
    bx = bx + d * ix;
    by = by + d * iy;
}

// the butterfly of __shfl_xor over 64 lanes (offsets 32, 16, ..., 1): every lane ends with the same value; v is destroyed
FP_HD double lk_combine64(double* v) {
    for (int m = FP_LK_LANES / 2; m > 0; m >>= 1) {
        double t[FP_LK_LANES];
        for (int i = 0; i < FP_LK_LANES; ++i) t[i] = v[i] + v[i ^ m];
        for (int i = 0; i < FP_LK_LANES; ++i) v[i] = t[i];
    }
    return v[0];
}

// smaller eigenvalue of G = [gxx gxy; gxy gyy] divided by the window's pixel count
FP_HD double lk_min_eig(double gxx, double gxy, double gyy, int npix) {
    const double d = gxx - gyy;
    return (0.5 * ((gxx + gyy) - sqrt(d * d + 4.0 * (gxy * gxy)))) / (double)npix;
}

FP_HD double lk_det(double gxx, double gxy, double gyy) { return gxx * gyy - gxy * gxy; }

// the guard: G is inverted only when its determinant is positive and its smaller eigenvalue per pixel reaches FP_LK_EIG_FLOOR
// (comparisons that are false for NaN); otherwise the level contributes no update
FP_HD bool lk_solvable(double gxx, double gxy, double gyy, int npix) {
    return lk_det(gxx, gxy, gyy) > 0.0 && lk_min_eig(gxx, gxy, gyy, npix) >= FP_LK_EIG_FLOOR;
}

// v += G^-1 b
FP_HD void lk_solve(double gxx, double gxy, double gyy, double bx, double by, double& vx, double& vy) {
    const double det = lk_det(gxx, gxy, gyy);
    vx = vx + (gyy * bx - gxy * by) / det;
    vy = vy + (gxx * by - gxy * bx) / det;
}

FP_HD double lk_level_scale(int l) { return 1.0 / (double)(1 << l); }

// frame of a query: int(t) held inside [0, T-1] (NaN -> 0)
FP_HD int lk_query_time(float t, int T) {
    if (!(t >= 0.0f)) return 0;
    if (t > (float)(T - 1)) return T - 1;
    return (int)t;
}

FP_HD float lk_finite_or_zero(float v) { return (v - v == 0.0f) ? v : 0.0f; }

FP_HD bool lk_inside(double x, double y, int W, int H) { return x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1); }

// verdict of one chain step.  (sx, sy) the chain's position in src, (fx, fy) the forward result, (rx, ry) the point the backward run
// returned; eig and res belong to the forward run.  A forward result that is not finite as a float32 (the type it is stored in) is
// replaced by the source position and counts as outside.  Returns the flags; fb = forward-backward distance.
FP_HD int lk_judge(double sx, double sy, double& fx, double& fy, double rx, double ry, double eig, double res, double fb_thresh, double min_eig,
                   double max_residual, int W, int H, bool prev_visible, double& fb) {
    const double dx = rx - sx, dy = ry - sy;
    fb = sqrt(dx * dx + dy * dy);
    int flags = 0;
    if (!(fb <= fb_thresh)) flags |= FP_LK_FLAG_FB;
    if (!(eig >= min_eig)) flags |= FP_LK_FLAG_EIG;
    if (!(res <= max_residual)) flags |= FP_LK_FLAG_RESIDUAL;
    const float ffx = (float)fx, ffy = (float)fy;
    if (!(ffx - ffx == 0.0f) || !(ffy - ffy == 0.0f)) {
        fx = sx;
        fy = sy;
        flags |= FP_LK_FLAG_OUTSIDE;
    } else if (!lk_inside(fx, fy, W, H)) {
        flags |= FP_LK_FLAG_OUTSIDE;
    }
    if (!prev_visible) flags |= FP_LK_FLAG_LOST_BEFORE;
    if (!((float)fb - (float)fb == 0.0f)) fb = 0.0;          // diagnostics stay finite; the flag records the failure
    return flags;
}
