// pnp_host_check — runs freepose_amd/csrc/pnp_core.h serially in the phase order of refine.hip's pnp_epnp_kernel (used count, centroid,
// scatter, control points, the 40 sums of M^T M, null vectors, the three candidates, camera centroids and sign, Horn's sums, reprojection
// errors, the choice), with the kernel's 256 accumulation lanes and its reduction tree, on problems read from a file.  Plain C++ with its
// own main: build it with
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I freepose_amd/csrc tools/pnp_host_check.cpp
// and compare its output with the numpy restatement (tests/test_refiner_track_cpu.py).  This is the part of EPnP that can be debugged on
// a machine without a GPU.
//
// input : int32 n_problems, then per problem  int32 {N, has_vis}, float64 K[9], float64 pts3d[N * 3], float64 pts2d[N * 2],
//                                             uint8 vis[N] when has_vis
// output: per problem float64[16] = {R[9], t[3], mean reprojection error, used points, status, 0}
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pnp_core.h"

namespace {
constexpr int T = FP_PNP_LANES;

// sum over the used points of term(i)[k], k < nk: lane t adds points t, t + T, ... in order, then the tree
template <class Term>
void lane_sums(int N, const std::vector<uint8_t>& vis, int nk, Term term, double* out) {
    std::vector<double> lanes((size_t)nk * T, 0.0), vals(nk);
    for (int t = 0; t < T; ++t)
        for (int i = t; i < N; i += T)
            if (vis[i]) {
                for (int k = 0; k < nk; ++k) vals[k] = lanes[(size_t)k * T + t];
                term(i, vals.data());
                for (int k = 0; k < nk; ++k) lanes[(size_t)k * T + t] = vals[k];
            }
    for (int k = 0; k < nk; ++k) out[k] = pnp_tree_sum(&lanes[(size_t)k * T]);
}

void solve(int N, const double* K, const double* p3, const double* p2, const std::vector<uint8_t>& vis, double* out) {
    int n = 0;
    for (int i = 0; i < N; ++i) n += vis[i] ? 1 : 0;
    if (n < 4) return pnp_write(out, nullptr, nullptr, 0.0, n, FP_PNP_FEW);
    double mu[3], sc[6];
    lane_sums(N, vis, 3, [&](int i, double* s) { s[0] += p3[i * 3]; s[1] += p3[i * 3 + 1]; s[2] += p3[i * 3 + 2]; }, mu);
    for (int k = 0; k < 3; ++k) mu[k] = mu[k] / (double)n;
    lane_sums(N, vis, 6, [&](int i, double* c) {
        const double x = p3[i * 3] - mu[0], y = p3[i * 3 + 1] - mu[1], z = p3[i * 3 + 2] - mu[2];
        c[0] += x * x; c[1] += x * y; c[2] += x * z; c[3] += y * y; c[4] += y * z; c[5] += z * z;
    }, sc);
    PnpCtrl ctrl;
    if (int st = pnp_control_points(mu, sc, n, ctrl)) return pnp_write(out, nullptr, nullptr, 0.0, n, st);
    double S[FP_PNP_NSUM];
    lane_sums(N, vis, FP_PNP_NSUM, [&](int i, double* acc) {
        double a[4], x, y;
        pnp_alphas(ctrl, p3 + i * 3, a);
        pnp_normalise(K, p2[i * 2], p2[i * 2 + 1], x, y);
        pnp_accum_mtm(a, x, y, acc);
    }, S);
    double work[FP_PNP_WORK], v[4][12], cc[3][4][3], pc0[3][3], R[3][9], t[3][3], err[3];
    pnp_null_vectors(S, work, v);
    for (int c = 0; c < 3; ++c) pnp_candidate(v, ctrl, c, cc[c]);
    double s9[9];
    lane_sums(N, vis, 9, [&](int i, double* s) {
        double a[4], pc[3];
        pnp_alphas(ctrl, p3 + i * 3, a);
        for (int c = 0; c < 3; ++c) {
            pnp_camera_point(cc[c], a, pc);
            s[c * 3] += pc[0]; s[c * 3 + 1] += pc[1]; s[c * 3 + 2] += pc[2];
        }
    }, s9);
    for (int c = 0; c < 3; ++c) {
        const double sgn = s9[c * 3 + 2] < 0.0 ? -1.0 : 1.0;
        for (int j = 0; j < 3; ++j) pc0[c][j] = sgn * (s9[c * 3 + j] / (double)n);
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 3; ++j) cc[c][i][j] = sgn * cc[c][i][j];
    }
    for (int c = 0; c < 3; ++c) {
        double h[9];
        lane_sums(N, vis, 9, [&](int i, double* hh) {
            double a[4], pc[3];
            pnp_alphas(ctrl, p3 + i * 3, a);
            pnp_camera_point(cc[c], a, pc);
            for (int j = 0; j < 3; ++j)
                for (int k = 0; k < 3; ++k) hh[j * 3 + k] += (pc[j] - pc0[c][j]) * (p3[i * 3 + k] - mu[k]);
        }, h);
        pnp_horn(h, pc0[c], mu, R[c], t[c]);
    }
    lane_sums(N, vis, 3, [&](int i, double* e) {
        for (int c = 0; c < 3; ++c) e[c] += pnp_reproj(K, R[c], t[c], p3 + i * 3, p2[i * 2], p2[i * 2 + 1]);
    }, err);
    for (int c = 0; c < 3; ++c) err[c] = err[c] / (double)n;
    const int best = pnp_choose(err);
    pnp_write(out, R[best], t[best], err[best], n, FP_PNP_OK);
}

bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: pnp_host_check IN OUT\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) {
        fprintf(stderr, "pnp_host_check: cannot open files\n");
        return 2;
    }
    int32_t np = 0;
    if (!get(fi, &np, 4) || np < 0) return 3;
    for (int p = 0; p < np; ++p) {
        int32_t hdr[2];
        double K[9], out[16];
        if (!get(fi, hdr, 8) || hdr[0] < FP_PNP_MIN_N || hdr[0] > FP_PNP_MAX_N) return 3;
        const int N = hdr[0];
        std::vector<double> p3((size_t)N * 3), p2((size_t)N * 2);
        std::vector<uint8_t> vis(N, 1);
        if (!get(fi, K, sizeof K) || !get(fi, p3.data(), p3.size() * 8) || !get(fi, p2.data(), p2.size() * 8)) return 3;
        if (hdr[1] && !get(fi, vis.data(), N)) return 3;
        solve(N, K, p3.data(), p2.data(), vis, out);
        if (fwrite(out, 8, 16, fo) != 16) return 4;
    }
    fclose(fi);
    if (fclose(fo) != 0) return 4;
    return 0;
}
