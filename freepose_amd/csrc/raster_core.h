// The rasteriser's per-vertex and per-triangle arithmetic, stated once for host and device: vertex projection, triangle set-up, the edge functions
// on both integer paths, the two forms of the barycentric quotient, the visibility key, near-plane straddlers and the row / column split of the
// per-lane coverage mask.  Plain C++17 without HIP types: raster.hip's kernels execute it; on a CPU tools/raster_core_host_check.cpp holds its
// arithmetic claims, and tests/_raster_cases.py setup() (its Python mirror), to it.  The contract is raster.hip's header; the oracle restates it in C.
#pragma once
#include <math.h>
#include <stdint.h>

#include "raster_plan.h"

namespace fp_raster {

template <class To, class From> FP_RASTER_HD inline To bit_cast(From v) { return __builtin_bit_cast(To, v); }
FP_RASTER_HD constexpr int imin(int a, int b) { return a < b ? a : b; }
FP_RASTER_HD constexpr int imax(int a, int b) { return a > b ? a : b; }

// ---- vertex stage: P = the pose's rows (3 x 4, row-major), (vx, vy, vz) the object-space vertex
struct SVert { int xi, yi; float iz, zc; };
FP_RASTER_HD inline SVert project_vertex(const float* P, float vx, float vy, float vz, float scale, float fx, float fy, float cx, float cy) {
    const float sx = scale * vx, sy = scale * vy, sz = scale * vz;
    const float Xc = fmaf(P[0], sx, fmaf(P[1], sy, fmaf(P[2], sz, P[3])));
    const float Yc = fmaf(P[4], sx, fmaf(P[5], sy, fmaf(P[6], sz, P[7])));
    const float Zc = fmaf(P[8], sx, fmaf(P[9], sy, fmaf(P[10], sz, P[11])));
    SVert o;
    o.zc = Zc;
    if (Zc > ZNEAR) {
        const float iz = 1.0f / Zc;
        const float u = fmaf(fx, Xc * iz, cx), v = fmaf(fy, Yc * iz, cy);
        // clamp far-off-screen coordinates so the fixed-point products stay inside int64
        const float uc = fminf(fmaxf(u, -CLAMP_PX), CLAMP_PX), vc = fminf(fmaxf(v, -CLAMP_PX), CLAMP_PX);
        o.xi = (int)rintf(uc * 256.0f); o.yi = (int)rintf(vc * 256.0f); o.iz = iz;
    } else {   // behind the near plane: homogeneous pixel coordinates for straddling triangles (contract in raster.hip's header)
        o.xi = bit_cast<int>(fmaf(fx, Xc, cx * Zc)); o.yi = bit_cast<int>(fmaf(fy, Yc, cy * Zc)); o.iz = 0.f;
    }
    return o;
}

// ---- triangle set-up
struct TriSetup {
    int x0, y0, x1, y1, x2, y2;
    float iz0, iz1, iz2;
    long long area2;
    int bx0, by0, bx1, by1;  // pixel bbox, inclusive, clipped
    bool ok;
    bool swapped;            // corners 1 and 2 were exchanged (callers exchange the per-corner attributes)
    bool strad;              // straddles the near plane: homogeneous rasterisation over the whole frame (struct Strad)
    bool small;              // spans < 128 px in x and y: every edge function at a candidate pixel fits 32 bits (EdgeFn::weights<int>)
};

FP_RASTER_HD inline bool topleft(int dx, int dy) { return (dy < 0) || (dy == 0 && dx > 0); }

// set-up from the three screen-space vertices already in registers (callers that batch their gathers load them first)
FP_RASTER_HD inline TriSetup tri_setup_v(SVert a, SVert b, SVert c, int W, int Hh) {
    TriSetup t;
    const int nfront = (a.zc > ZNEAR) + (b.zc > ZNEAR) + (c.zc > ZNEAR);
    t.ok = nfront == 3;
    t.strad = nfront == 1 || nfront == 2;
    if (t.strad) {   // near-plane straddler: candidate pixels = the whole frame, original corner order, no fixed-point set-up
        t.ok = true; t.swapped = false; t.area2 = 1; t.small = false;
        t.x0 = t.y0 = t.x1 = t.y1 = t.x2 = t.y2 = 0;
        t.iz0 = t.iz1 = t.iz2 = 0.f;
        t.bx0 = 0; t.by0 = 0; t.bx1 = W - 1; t.by1 = Hh - 1;
        return t;
    }
    long long area2 = (long long)(b.xi - a.xi) * (c.yi - a.yi) - (long long)(b.yi - a.yi) * (c.xi - a.xi);
    t.swapped = area2 < 0;
    if (area2 < 0) { const SVert tmp = b; b = c; c = tmp; area2 = -area2; }
    t.area2 = area2;
    if (area2 == 0) t.ok = false;
    t.x0 = a.xi; t.y0 = a.yi; t.x1 = b.xi; t.y1 = b.yi; t.x2 = c.xi; t.y2 = c.yi;
    t.iz0 = a.iz; t.iz1 = b.iz; t.iz2 = c.iz;
    const int mnx = imin(a.xi, imin(b.xi, c.xi)), mxx = imax(a.xi, imax(b.xi, c.xi));
    const int mny = imin(a.yi, imin(b.yi, c.yi)), mxy = imax(a.yi, imax(b.yi, c.yi));
    // pixel p is a candidate when its centre 256p+128 lies in [mn, mx]
    t.bx0 = imax(0, (mnx - 128 + 255) >> 8);
    t.by0 = imax(0, (mny - 128 + 255) >> 8);
    t.bx1 = imin(W - 1, (mxx - 128) >> 8);
    t.by1 = imin(Hh - 1, (mxy - 128) >> 8);
    if (t.bx1 < t.bx0 || t.by1 < t.by0) t.ok = false;
    t.small = (mxx - mnx) < SMALL_SPAN && (mxy - mny) < SMALL_SPAN;
    return t;
}

// ---- edge functions.  v_mul_i32_i24 on the device (operands sign-extended from 24 bits, low 32 bits of the product; full rate, where a
// 64-bit product is four quarter-rate multiplies); the host emulates the instruction, so an operand that does not fit shows as a wrong product
FP_RASTER_HD inline int mul24(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(a, b);
#else
    const long long x = (int)((unsigned)a << 8) >> 8, y = (int)((unsigned)b << 8) >> 8;
    return (int)(unsigned)(unsigned long long)(x * y);
#endif
}
FP_RASTER_HD inline long long edge_mul(int a, long long b) { return (long long)a * b; }
FP_RASTER_HD inline int edge_mul(int a, int b) { return mul24(a, b); }

// The three edge functions of a set-up triangle (not a straddler) at a sample (sx, sy) in subpixels, E_ab(p) = (bx-ax)(py-ay) - (by-ay)(px-ax), positive
// inside for area2 > 0; w_i belongs to the edge opposite corner i.  I = long long always holds; I = int holds for a `small` triangle at one of its
// candidate pixels (centre inside the vertex bounding box): every difference is below 2^15 in magnitude, so the products fit 24 x 24 -> 32-bit multiplies
// and the sums 32 bits: the SAME integers, hence the same coverage, float conversions and depth bits (swept by tools/raster_core_host_check.cpp).
struct EdgeFn {
    int A0, B0, A1, B1, A2, B2;        // direction of the edge opposite corner 0 (v1 -> v2), 1 (v2 -> v0), 2 (v0 -> v1)
    int ox0, oy0, ox1, oy1, ox2, oy2;  // and where it starts
    bool tl0, tl1, tl2;                // top-left rule: the edge owns the samples exactly on it
    FP_RASTER_HD explicit EdgeFn(const TriSetup& t)
        : A0(t.x2 - t.x1), B0(t.y2 - t.y1), A1(t.x0 - t.x2), B1(t.y0 - t.y2), A2(t.x1 - t.x0), B2(t.y1 - t.y0),
          ox0(t.x1), oy0(t.y1), ox1(t.x2), oy1(t.y2), ox2(t.x0), oy2(t.y0), tl0(topleft(A0, B0)), tl1(topleft(A1, B1)), tl2(topleft(A2, B2)) {}
    template <class I> FP_RASTER_HD void weights(I sx, I sy, I& w0, I& w1, I& w2) const {
        w0 = edge_mul(A0, sy - oy0) - edge_mul(B0, sx - ox0);
        w1 = edge_mul(A1, sy - oy1) - edge_mul(B1, sx - ox1);
        w2 = edge_mul(A2, sy - oy2) - edge_mul(B2, sx - ox2);
    }
    template <class I> FP_RASTER_HD bool accept(I w0, I w1, I w2) const {
        return (w0 | w1 | w2) >= 0 && (w0 != 0 || tl0) && (w1 != 0 || tl1) && (w2 != 0 || tl2);
    }
};
template <class I> FP_RASTER_HD constexpr I pixel_centre(int p) { return (I)p * 256 + 128; }
// The same edge functions, written out at ONE pixel centre, with the sign tests as early returns and the top-left rule evaluated only on
// a zero: what the global-buffer path runs per candidate pixel.  Through EdgeFn the compiler no longer sees, at the weights' conversion to
// float, that each is non-negative, and converts the 64-bit ones as signed (+12 vector instructions per fragment: 0.6 to 2 % of that path
// at 327 680 triangles, measured), so this second statement stays; tools/raster_core_host_check.cpp holds the two to each other.
template <class I> FP_RASTER_HD inline bool tri_cover(const TriSetup& t, int px, int py, I& w0, I& w1, I& w2) {
    const I sx = pixel_centre<I>(px), sy = pixel_centre<I>(py);
    w0 = edge_mul(t.x2 - t.x1, sy - t.y1) - edge_mul(t.y2 - t.y1, sx - t.x1);
    w1 = edge_mul(t.x0 - t.x2, sy - t.y2) - edge_mul(t.y0 - t.y2, sx - t.x2);
    w2 = edge_mul(t.x1 - t.x0, sy - t.y0) - edge_mul(t.y1 - t.y0, sx - t.x0);
    if (w0 < 0 || w1 < 0 || w2 < 0) return false;
    if (w0 == 0 && !topleft(t.x2 - t.x1, t.y2 - t.y1)) return false;
    if (w1 == 0 && !topleft(t.x0 - t.x2, t.y0 - t.y2)) return false;
    if (w2 == 0 && !topleft(t.x1 - t.x0, t.y1 - t.y0)) return false;
    return true;
}

// ---- barycentrics b_i = float(w_i) / float(area2) and depth.  bary_quotient is the IEEE quotient.  bary_rcp gives the same bits WITHOUT
// the quotient's ~12-instruction expansion per weight: the reciprocal of the area is taken once per triangle in double (rd = RN(1 / fa)),
// each weight is then one fp64 multiply rounded to float.  The double product is within 2^-52 (relative) of the exact quotient; a quotient
// of two 24-bit significands is never closer than 2^-49 to a rounding midpoint of the float grid (|x/n - m| >= 1 / (N k) for a 25-bit
// midpoint significand k), so rounding the product gives the correctly rounded quotient: the bits of the division (and of the oracle).
// area_rcp takes area2 through int: it is for `small` triangles (area2 < 2^31).
template <class I> FP_RASTER_HD inline float bary_quotient(I w, float fa) { return (float)w / fa; }
FP_RASTER_HD inline double area_rcp(const TriSetup& t) { return 1.0 / (double)(float)(int)t.area2; }
FP_RASTER_HD inline float bary_rcp(int w, double rd) { return (float)((double)(float)w * rd); }
FP_RASTER_HD inline float depth_from_bary(const TriSetup& t, float b0, float b1, float b2) {
    const float izp = fmaf(b2, t.iz2, fmaf(b1, t.iz1, b0 * t.iz0));
    return 1.0f / izp;
}
// the three weights as barycentrics, by the quotient (the 64-bit path of the raster pass, and the resolve stages per pixel)
template <class I> FP_RASTER_HD inline void bary3(const TriSetup& t, I w0, I w1, I w2, float& b0, float& b1, float& b2) {
    const float fa = (float)t.area2;
    b0 = bary_quotient(w0, fa); b1 = bary_quotient(w1, fa); b2 = bary_quotient(w2, fa);
}
// coverage and weights at a pixel for a sink: the per-pixel statement (global buffer) or the object (LDS tile, whose kernel is smaller with it)
template <bool NARROW, class I> FP_RASTER_HD inline bool cover_at(const TriSetup& t, int px, int py, I& w0, I& w1, I& w2) {
    if (!NARROW) return tri_cover<I>(t, px, py, w0, w1, w2);
    const EdgeFn e(t);
    e.weights(pixel_centre<I>(px), pixel_centre<I>(py), w0, w1, w2);
    return e.accept(w0, w1, w2);
}
// coverage and depth of pixel (px, py).  NARROW: small triangles take the 32-bit edge functions and the reciprocal form
// (three IEEE quotients instead: measured 5 % slower at 1 280 triangles on the tiled path)
template <bool NARROW> FP_RASTER_HD inline bool fragment(const TriSetup& t, int px, int py, float& d) {
    float b0, b1, b2;
    if (NARROW && t.small) {
        int w0, w1, w2;
        if (!cover_at<NARROW, int>(t, px, py, w0, w1, w2)) return false;
        const double rd = area_rcp(t);
        b0 = bary_rcp(w0, rd); b1 = bary_rcp(w1, rd); b2 = bary_rcp(w2, rd);
    } else {
        long long w0, w1, w2;
        if (!cover_at<NARROW, long long>(t, px, py, w0, w1, w2)) return false;
        bary3(t, w0, w1, w2, b0, b1, b2);
    }
    d = depth_from_bary(t, b0, b1, b2);
    return d > 0.f;
}

// ---- visibility key: depth bits << 32 | face id.  Positive floats order as their bits: an unsigned MIN takes the nearest depth, then the lowest id
constexpr unsigned long long KEY_NONE = ~0ull;   // above every key (a positive float's bits stay below 0x7f800000)
FP_RASTER_HD inline unsigned long long vis_key(float depth, int face) { return ((unsigned long long)bit_cast<unsigned>(depth) << 32) | (unsigned)face; }
FP_RASTER_HD inline float key_depth(unsigned long long key) { return bit_cast<float>((unsigned)(key >> 32)); }
FP_RASTER_HD inline int key_face(unsigned long long key) { return (int)(unsigned)(key & 0xffffffffu); }

// ---- homogeneous edge functions of a triangle that straddles the near plane (contract in raster.hip's header)
struct Strad { double a[3], b[3], c[3], det; };
FP_RASTER_HD inline void strad_vertex(const SVert& v, double& x, double& y, double& w) {
    w = (double)v.zc;
    if (v.zc > ZNEAR) { x = ((double)v.xi * (1.0 / 256.0)) * w; y = ((double)v.yi * (1.0 / 256.0)) * w; }
    else { x = (double)bit_cast<float>(v.xi); y = (double)bit_cast<float>(v.yi); }
}
FP_RASTER_HD inline Strad strad_setup(const SVert* __restrict__ sv, const int32_t* __restrict__ faces, int f) {
    double x[3], y[3], w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) strad_vertex(sv[faces[3 * f + k]], x[k], y[k], w[k]);
    Strad q;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        q.a[k] = y[k1] * w[k2] - y[k2] * w[k1];
        q.b[k] = x[k2] * w[k1] - x[k1] * w[k2];
        q.c[k] = x[k1] * y[k2] - x[k2] * y[k1];
    }
    q.det = (x[0] * q.a[0] + y[0] * q.b[0]) + w[0] * q.c[0];
    return q;
}
// coverage, depth and perspective-correct barycentrics of pixel (px, py)
FP_RASTER_HD inline bool strad_pixel(const Strad& q, int px, int py, float& d, float& b0, float& b1, float& b2) {
    const double X = (double)px + 0.5, Y = (double)py + 0.5;
    double e0 = (q.a[0] * X + q.b[0] * Y) + q.c[0];
    double e1 = (q.a[1] * X + q.b[1] * Y) + q.c[1];
    double e2 = (q.a[2] * X + q.b[2] * Y) + q.c[2];
    double det = q.det;
    if (det < 0.0) { e0 = -e0; e1 = -e1; e2 = -e2; det = -det; }
    if (!(det > 0.0) || e0 < 0.0 || e1 < 0.0 || e2 < 0.0) return false;
    const double S = (e0 + e1) + e2;
    if (!(S > 0.0)) return false;
    const double z = det / S;
    if (!(z > (double)ZNEAR)) return false;
    d = (float)z;
    b0 = (float)(e0 / S); b1 = (float)(e1 / S); b2 = (float)(e2 / S);
    return true;
}
template <bool NARROW> FP_RASTER_HD inline bool fragment(const Strad& q, int px, int py, float& d) {
    float b0, b1, b2;
    return strad_pixel(q, px, py, d, b0, b1, b2);
}
// Back face (renderer.py:63-66, cull_faces = True -> GL_CULL_FACE with counter-clockwise front faces): in this frame (x right, y down,
// z forward) a counter-clockwise-from-outside triangle that faces the camera has a NEGATIVE screen-space area, i.e. tri_setup_v swapped
// its corners; a straddler is classified by the sign of its homogeneous determinant (same sign as the area when all w > 0).
FP_RASTER_HD inline bool back_facing(const TriSetup& t, const SVert* __restrict__ sv, const int32_t* __restrict__ faces, int f) {
    if (t.strad) return strad_setup(sv, faces, f).det > 0.0;
    return !t.swapped;
}

// ---- candidate kk of a box bw pixels wide -> row kk / bw, column kk % bw, without an integer division: rbw = split_rcp(bw) once per box.
// Exact for kk < 32, bw <= 32 (the per-lane coverage mask's range; swept exhaustively by tools/raster_core_host_check.cpp)
FP_RASTER_HD inline float split_rcp(int bw) { return 1.0f / (float)bw; }
FP_RASTER_HD inline void split_rowcol(int kk, int bw, float rbw, int& row, int& col) {
    row = (int)(((float)kk + 0.5f) * rbw);
    col = kk - row * bw;
}

}  // namespace fp_raster
