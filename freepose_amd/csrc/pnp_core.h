// pnp_core.h — the small dense phases and the per-point terms of refine.hip's EPnP as plain __host__ __device__ functions: cyclic
// Jacobi eigen-solver, control points, barycentric coordinates, the 40 sums M^T M is assembled from, the 6 x 10 system with its three
// beta initialisations, Gauss-Newton, Horn's absolute orientation, the choice among the candidates.  No HIP type appears here, so the
// same text compiles with g++ into tools/pnp_host_check.cpp, which runs the kernel's phases serially (under
// -fsanitize=address,undefined) — the part of the solver that can be debugged without a GPU.
//
// EPnP: Lepetit, Moreno-Noguer, Fua, "EPnP: An Accurate O(n) Solution to the PnP Problem", IJCV 2009, in the variant OpenCV ships
// (three beta initialisations, five Gauss-Newton steps each, the candidate with the smallest reprojection error).  Everything is fp64.
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
#if defined(__HIPCC__)
#define FP_HD_NOINL __host__ __device__ inline
#else
#define FP_HD_NOINL inline
#endif

#define FP_PNP_LANES 256     // accumulation lanes of every sum over points: lane t adds points t, t + 256, ... in order, then a fixed tree
#define FP_PNP_NSUM 40       // sums M^T M is assembled from: 10 pairs (i <= j) of barycentrics x {1, x, y, x^2 + y^2}
#define FP_PNP_MIN_N 4
#define FP_PNP_MAX_N 4096
#define FP_PNP_OK 0
#define FP_PNP_FEW 1         // fewer than 4 used points
#define FP_PNP_SINGULAR 2    // smallest eigenvalue of the 3 x 3 scatter <= 1e-12 x the largest: coplanar or coincident points
#define FP_PNP_WORK 288      // doubles of scratch pnp_null_vectors needs (12 x 12 matrix + 12 x 12 eigenvectors)

// the fixed tree over the lanes: the pairing of refine.hip's block reduction
FP_HD double pnp_tree_sum(double* v) {
    for (int w = FP_PNP_LANES / 2; w > 0; w >>= 1)
        for (int t = 0; t < w; ++t) v[t] = v[t] + v[t + w];
    return v[0];
}

// cyclic Jacobi on a symmetric n x n matrix A (row-major, destroyed: its diagonal ends as the eigenvalues); columns of V = eigenvectors.
// The rotation is the one of scale.hip's jacobi_rot.  At most 64 sweeps (it converges quadratically: 6-10 in practice).
FP_HD_NOINL void pnp_jacobi(double* A, double* V, int n) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, tr = 0.0;
        for (int p = 0; p < n; ++p) {
            tr += fabs(A[p * n + p]);
            for (int q = p + 1; q < n; ++q) off += fabs(A[p * n + q]);
        }
        if (!(off > tr * 0x1p-70)) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
}

// ---- control points and barycentric coordinates ---------------------------------------------------------------------------------------
struct PnpCtrl {
    double cw[4][3];   // control points in the object frame: the centroid, + principal axis i scaled by sqrt(lambda_i / n)
    double ci[3][3];   // inverse of the 3 x 3 matrix whose columns are cw[1..3] - cw[0] (rows: axis i / its length)
};

// mu: centroid; sc: xx xy xz yy yz zz of the centred points (sums, not means); n: used points
FP_HD_NOINL int pnp_control_points(const double* mu, const double* sc, int n, PnpCtrl& c) {
    double A[9] = {sc[0], sc[1], sc[2], sc[1], sc[3], sc[4], sc[2], sc[4], sc[5]}, V[9];
    pnp_jacobi(A, V, 3);
    int ord[3] = {0, 1, 2};                    // eigenvalues descending, ties by index
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (A[ord[j] * 4] > A[ord[i] * 4]) { const int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
    const double lmax = A[ord[0] * 4], lmin = A[ord[2] * 4];
    if (!(lmax > 0.0) || !(lmin > 1e-12 * lmax)) return FP_PNP_SINGULAR;
    for (int j = 0; j < 3; ++j) c.cw[0][j] = mu[j];
    for (int i = 0; i < 3; ++i) {
        const double k = sqrt(A[ord[i] * 4] / (double)n);
        // an eigenvector's sign is the solver's choice, and with noisy image points the pose depends (slightly) on the control points:
        // the axis points the way that makes its component of largest magnitude (the first of equals) positive
        int big = 0;
        for (int j = 1; j < 3; ++j)
            if (fabs(V[j * 3 + ord[i]]) > fabs(V[big * 3 + ord[i]])) big = j;
        const double sg = V[big * 3 + ord[i]] < 0.0 ? -1.0 : 1.0;
        for (int j = 0; j < 3; ++j) {
            const double e = sg * V[j * 3 + ord[i]];
            c.cw[i + 1][j] = mu[j] + k * e;
            c.ci[i][j] = e / k;
        }
    }
    return FP_PNP_OK;
}

FP_HD void pnp_alphas(const PnpCtrl& c, const double* p, double* a) {
    const double d0 = p[0] - c.cw[0][0], d1 = p[1] - c.cw[0][1], d2 = p[2] - c.cw[0][2];
    for (int i = 0; i < 3; ++i) a[i + 1] = (c.ci[i][0] * d0 + c.ci[i][1] * d1) + c.ci[i][2] * d2;
    a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}

// image point -> identity-camera coordinates (K without skew: fx = K[0], cx = K[2], fy = K[4], cy = K[5])
FP_HD void pnp_normalise(const double* K, double u, double v, double& x, double& y) {
    x = (u - K[2]) / K[0];
    y = (v - K[5]) / K[4];
}

// One point's share of M^T M.  Its two rows of M are [a_i, 0, -a_i x] and [0, a_i, -a_i y] (i = 0..3), so block (i, j) of M^T M is
// a_i a_j [[1, 0, -x], [0, 1, -y], [-x, -y, x^2 + y^2]]: four sums per pair i <= j.
FP_HD void pnp_accum_mtm(const double* a, double x, double y, double* acc) {
    const double r2 = x * x + y * y;
    int k = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j, k += 4) {
            const double w = a[i] * a[j];
            acc[k] += w;
            acc[k + 1] += w * x;
            acc[k + 2] += w * y;
            acc[k + 3] += w * r2;
        }
}

// ---- the four null-space vectors --------------------------------------------------------------------------------------------------------
// S: the FP_PNP_NSUM reduced sums; work: FP_PNP_WORK doubles; v[k][12], k = 0..3: eigenvectors of the 4 smallest eigenvalues of M^T M,
// smallest first (ties by index)
FP_HD_NOINL void pnp_null_vectors(const double* S, double* work, double (*v)[12]) {
    double *M = work, *V = work + 144;
    int k = 0;
    for (int i = 0; i < 4; ++i)
        for (int j = i; j < 4; ++j, k += 4) {
            const double blk[9] = {S[k], 0.0, -S[k + 1], 0.0, S[k], -S[k + 2], -S[k + 1], -S[k + 2], S[k + 3]};
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) {
                    M[(3 * i + r) * 12 + 3 * j + c] = blk[r * 3 + c];
                    M[(3 * j + c) * 12 + 3 * i + r] = blk[r * 3 + c];      // the block is symmetric: (j, i) is its transpose = itself
                }
        }
    pnp_jacobi(M, V, 12);
    bool taken[12];
    for (int i = 0; i < 12; ++i) taken[i] = false;
    for (int s = 0; s < 4; ++s) {
        int best = -1;
        for (int i = 0; i < 12; ++i)
            if (!taken[i] && (best < 0 || M[i * 13] < M[best * 13])) best = i;
        taken[best] = true;
        for (int r = 0; r < 12; ++r) v[s][r] = V[r * 12 + best];
    }
}

// least squares min |A x - b| for A [6, n], n <= 5, by Householder reflections without pivoting (A and b are destroyed).  A column
// that is (numerically) dependent on the ones before it gets x = 0.
FP_HD_NOINL void pnp_lstsq(double (*A)[5], double* b, int n, double* x) {
    double d[5];
    double dmax = 0.0;
    for (int k = 0; k < n; ++k) {
        double nn = 0.0;
        for (int i = k; i < 6; ++i) nn += A[i][k] * A[i][k];
        d[k] = 0.0;
        if (!(nn > 0.0)) continue;
        double alpha = sqrt(nn);
        if (A[k][k] > 0.0) alpha = -alpha;
        A[k][k] -= alpha;
        double vtv = 0.0;
        for (int i = k; i < 6; ++i) vtv += A[i][k] * A[i][k];
        for (int j = k + 1; j < n; ++j) {
            double s = 0.0;
            for (int i = k; i < 6; ++i) s += A[i][k] * A[i][j];
            const double f = 2.0 * s / vtv;
            for (int i = k; i < 6; ++i) A[i][j] -= f * A[i][k];
        }
        double s = 0.0;
        for (int i = k; i < 6; ++i) s += A[i][k] * b[i];
        const double f = 2.0 * s / vtv;
        for (int i = k; i < 6; ++i) b[i] -= f * A[i][k];
        d[k] = alpha;
        dmax = fmax(dmax, fabs(alpha));
    }
    for (int k = n - 1; k >= 0; --k) {
        double s = b[k];
        for (int j = k + 1; j < n; ++j) s -= A[k][j] * x[j];
        x[k] = fabs(d[k]) > 1e-13 * dmax ? s / d[k] : 0.0;
    }
}

// ---- betas: the 6 x 10 system, its three initialisations, Gauss-Newton -----------------------------------------------------------------
// L [6][10]: row = control-point pair (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); column = B11 B12 B22 B13 B23 B33 B14 B24 B34 B44.
FP_HD_NOINL void pnp_build_L(const double (*v)[12], const PnpCtrl& c, double (*L)[10], double* rho) {
    int a = 0, b = 1;
    for (int r = 0; r < 6; ++r) {
        double dv[4][3];
        for (int k = 0; k < 4; ++k)
            for (int j = 0; j < 3; ++j) dv[k][j] = v[k][3 * a + j] - v[k][3 * b + j];
        const auto dot = [&](int p, int q) { return (dv[p][0] * dv[q][0] + dv[p][1] * dv[q][1]) + dv[p][2] * dv[q][2]; };
        L[r][0] = dot(0, 0);
        L[r][1] = 2.0 * dot(0, 1);
        L[r][2] = dot(1, 1);
        L[r][3] = 2.0 * dot(0, 2);
        L[r][4] = 2.0 * dot(1, 2);
        L[r][5] = dot(2, 2);
        L[r][6] = 2.0 * dot(0, 3);
        L[r][7] = 2.0 * dot(1, 3);
        L[r][8] = 2.0 * dot(2, 3);
        L[r][9] = dot(3, 3);
        const double e0 = c.cw[a][0] - c.cw[b][0], e1 = c.cw[a][1] - c.cw[b][1], e2 = c.cw[a][2] - c.cw[b][2];
        rho[r] = (e0 * e0 + e1 * e1) + e2 * e2;
        if (++b > 3) { ++a; b = a + 1; }
    }
}

// which: 0 -> [B11 B12 B13 B14], 1 -> [B11 B12 B22], 2 -> [B11 B12 B22 B13 B23]  (OpenCV's find_betas_approx_1 / _2 / _3)
FP_HD_NOINL void pnp_betas_init(const double (*L)[10], const double* rho, int which, double* beta) {
    const int cols[3][5] = {{0, 1, 3, 6, 0}, {0, 1, 2, 0, 0}, {0, 1, 2, 3, 4}};
    const int nc = which == 0 ? 4 : which == 1 ? 3 : 5;
    double A[6][5], b[6], x[5] = {0, 0, 0, 0, 0};
    for (int r = 0; r < 6; ++r) {
        for (int k = 0; k < 5; ++k) A[r][k] = k < nc ? L[r][cols[which][k]] : 0.0;
        b[r] = rho[r];
    }
    pnp_lstsq(A, b, nc, x);
    if (which == 0) {
        const double s = x[0] < 0.0 ? -1.0 : 1.0;
        beta[0] = sqrt(s * x[0]);
        for (int k = 1; k < 4; ++k) beta[k] = beta[0] > 0.0 ? s * x[k] / beta[0] : 0.0;
        return;
    }
    if (x[0] < 0.0) {
        beta[0] = sqrt(-x[0]);
        beta[1] = x[2] < 0.0 ? sqrt(-x[2]) : 0.0;
    } else {
        beta[0] = sqrt(x[0]);
        beta[1] = x[2] > 0.0 ? sqrt(x[2]) : 0.0;
    }
    if (x[1] < 0.0) beta[0] = -beta[0];
    beta[2] = which == 2 && beta[0] != 0.0 ? x[3] / beta[0] : 0.0;
    beta[3] = 0.0;
}

FP_HD_NOINL void pnp_gauss_newton(const double (*L)[10], const double* rho, double* be, int steps) {
    for (int it = 0; it < steps; ++it) {
        double A[6][5], b[6], x[5] = {0, 0, 0, 0, 0};
        for (int r = 0; r < 6; ++r) {
            const double* l = L[r];
            A[r][0] = 2.0 * l[0] * be[0] + l[1] * be[1] + l[3] * be[2] + l[6] * be[3];
            A[r][1] = l[1] * be[0] + 2.0 * l[2] * be[1] + l[4] * be[2] + l[7] * be[3];
            A[r][2] = l[3] * be[0] + l[4] * be[1] + 2.0 * l[5] * be[2] + l[8] * be[3];
            A[r][3] = l[6] * be[0] + l[7] * be[1] + l[8] * be[2] + 2.0 * l[9] * be[3];
            A[r][4] = 0.0;
            b[r] = rho[r] - (l[0] * be[0] * be[0] + l[1] * be[0] * be[1] + l[2] * be[1] * be[1] + l[3] * be[0] * be[2] + l[4] * be[1] * be[2] +
                             l[5] * be[2] * be[2] + l[6] * be[0] * be[3] + l[7] * be[1] * be[3] + l[8] * be[2] * be[3] + l[9] * be[3] * be[3]);
        }
        pnp_lstsq(A, b, 4, x);
        for (int k = 0; k < 4; ++k) be[k] += x[k];
    }
}

// candidate `which`: camera-frame control points cc [4][3] = sum_k beta_k v[k]
FP_HD_NOINL void pnp_candidate(const double (*v)[12], const PnpCtrl& c, int which, double (*cc)[3]) {
    double L[6][10], rho[6], be[4];
    pnp_build_L(v, c, L, rho);
    pnp_betas_init(L, rho, which, be);
    pnp_gauss_newton(L, rho, be, 5);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 3; ++j)
            cc[i][j] = ((be[0] * v[0][3 * i + j] + be[1] * v[1][3 * i + j]) + be[2] * v[2][3 * i + j]) + be[3] * v[3][3 * i + j];
}

// camera-frame point from its barycentrics
FP_HD void pnp_camera_point(const double (*cc)[3], const double* a, double* pc) {
    for (int j = 0; j < 3; ++j) pc[j] = ((a[0] * cc[0][j] + a[1] * cc[1][j]) + a[2] * cc[2][j]) + a[3] * cc[3][j];
}

// ---- Horn's absolute orientation ---------------------------------------------------------------------------------------------------------
// H [3][3] = sum (pc - pc0)(pw - pw0)^T.  SVD by one-sided Jacobi (columns of H rotated until orthogonal): H = U S V^T,
// R = U diag(1, 1, det(U V^T)) V^T, t = pc0 - R pw0.  Always returns a proper rotation for finite input.
FP_HD_NOINL void pnp_horn(const double* H, const double* pc0, const double* pw0, double* R, double* t) {
    double A[3][3], V[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { A[i][j] = H[i * 3 + j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int k = 0; k < 3; ++k) { al += A[k][p] * A[k][p]; be += A[k][q] * A[k][q]; ga += A[k][p] * A[k][q]; }
                if (ga == 0.0 || !(ga * ga > 0x1p-104 * al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = c * tt;
                for (int k = 0; k < 3; ++k) {
                    const double ap = A[k][p], aq = A[k][q];
                    A[k][p] = c * ap - s * aq;
                    A[k][q] = s * ap + c * aq;
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = c * vp - s * vq;
                    V[k][q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double nn[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) nn[j] = (A[0][j] * A[0][j] + A[1][j] * A[1][j]) + A[2][j] * A[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (nn[ord[j]] > nn[ord[i]]) { const int s = ord[i]; ord[i] = ord[j]; ord[j] = s; }
    double U[3][3], W[3][3];                         // columns: left / right singular vectors, largest singular value first
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) W[k][j] = V[k][ord[j]];
    const double n0 = sqrt(nn[ord[0]]);
    for (int k = 0; k < 3; ++k) U[k][0] = n0 > 0.0 ? A[k][ord[0]] / n0 : (k == 0 ? 1.0 : 0.0);
    double a1[3], proj = 0.0;
    for (int k = 0; k < 3; ++k) { a1[k] = A[k][ord[1]]; proj += a1[k] * U[k][0]; }
    double n1 = 0.0;
    for (int k = 0; k < 3; ++k) { a1[k] -= proj * U[k][0]; n1 += a1[k] * a1[k]; }
    n1 = sqrt(n1);
    if (n1 > 1e-150 && n1 > 1e-14 * n0) {
        for (int k = 0; k < 3; ++k) U[k][1] = a1[k] / n1;
    } else {                                         // rank <= 1: any unit vector orthogonal to the first
        int m = 0;
        for (int k = 1; k < 3; ++k)
            if (fabs(U[k][0]) < fabs(U[m][0])) m = k;
        double e[3] = {0.0, 0.0, 0.0}, nn1 = 0.0;
        e[m] = 1.0;
        for (int k = 0; k < 3; ++k) { e[k] -= U[m][0] * U[k][0]; nn1 += e[k] * e[k]; }
        nn1 = sqrt(nn1);
        for (int k = 0; k < 3; ++k) U[k][1] = e[k] / nn1;
    }
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    const double detW = W[0][0] * (W[1][1] * W[2][2] - W[1][2] * W[2][1]) - W[0][1] * (W[1][0] * W[2][2] - W[1][2] * W[2][0]) +
                        W[0][2] * (W[1][0] * W[2][1] - W[1][1] * W[2][0]);
    const double d = detW < 0.0 ? -1.0 : 1.0;        // det U = +1 by construction
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = (U[i][0] * W[j][0] + U[i][1] * W[j][1]) + d * U[i][2] * W[j][2];
    for (int i = 0; i < 3; ++i) t[i] = pc0[i] - ((R[i * 3] * pw0[0] + R[i * 3 + 1] * pw0[1]) + R[i * 3 + 2] * pw0[2]);
}

// reprojection error of one point in pixels
FP_HD double pnp_reproj(const double* K, const double* R, const double* t, const double* p, double u, double v) {
    const double X = ((R[0] * p[0] + R[1] * p[1]) + R[2] * p[2]) + t[0];
    const double Y = ((R[3] * p[0] + R[4] * p[1]) + R[5] * p[2]) + t[1];
    const double Z = ((R[6] * p[0] + R[7] * p[1]) + R[8] * p[2]) + t[2];
    const double du = u - (K[2] + K[0] * X / Z), dv = v - (K[5] + K[4] * Y / Z);
    return sqrt(du * du + dv * dv);
}

// the candidate with the smallest mean error; a non-finite error loses against any finite one; ties keep the first
FP_HD int pnp_choose(const double* err) {
    int best = 0;
    for (int c = 1; c < 3; ++c)
        if (err[c] < err[best] || (err[best] != err[best] && err[c] == err[c])) best = c;
    return best;
}

// the 16 doubles of one problem: R[9], t[3], mean reprojection error, used points, status, 0
FP_HD void pnp_write(double* out, const double* R, const double* t, double err, int n, int status) {
    const double nan = NAN;
    for (int k = 0; k < 9; ++k) out[k] = status ? nan : R[k];
    for (int k = 0; k < 3; ++k) out[9 + k] = status ? nan : t[k];
    out[12] = status ? nan : err;
    out[13] = (double)n;
    out[14] = (double)status;
    out[15] = 0.0;
}
