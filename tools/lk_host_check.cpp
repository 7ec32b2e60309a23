// lk_host_check — runs freepose_amd/csrc/lk_core.h serially in the order of lk_track.hip: the grey pyramid, the init rows, then chain
// step 1 .. T-1 over all (query, direction) items, each with the kernel's 64 lanes (window pixel k on lane k % 64, slot k / 64, lane sums
// in slot order) and its butterfly combination order.  Plain C++ with its own main: build it with
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I freepose_amd/csrc tools/lk_host_check.cpp
// and compare its output with the numpy restatement (tests/test_lk_tracker_cpu.py).  This is the part of the tracker that can be
// debugged on a machine without a GPU.
//
// input : int32 {T, H, W, N, levels, radius, iters}, float32 {fb_thresh, min_eig, max_residual}, uint8 frames[T*H*W*3],
//         float32 queries[N*3]
// output: int32 {kept levels, total floats (low 31 bits suffice here)}, float32 pyramid[total], float32 tracks[T*N*2], uint8 vis[T*N],
//         float32 diag[T*N*4]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "lk_core.h"

namespace {
constexpr int L = FP_LK_LANES;

double wave_sum(double* lanes) { return lk_combine64(lanes); }

void lk_run(const LkPyramid& P, const float* pyr, int ta, int tb, double px, double py, int r, int iters, double& ox, double& oy, double& eig,
            double& res) {
    const int npix = (2 * r + 1) * (2 * r + 1), slots = (npix + L - 1) / L;
    std::vector<double> a((size_t)slots * L), ix((size_t)slots * L), iy((size_t)slots * L);
    double gx = 0.0, gy = 0.0;
    ox = px;
    oy = py;
    eig = 0.0;
    res = 0.0;
    for (int l = P.levels - 1; l >= 0; --l) {
        const int w = P.w[l], h = P.h[l];
        const float* A = pyr + P.off[l] + (long long)ta * h * w;
        const float* B = pyr + P.off[l] + (long long)tb * h * w;
        const double sc = lk_level_scale(l), plx = px * sc, ply = py * sc;
        double lxx[L], lxy[L], lyy[L];
        for (int lane = 0; lane < L; ++lane) {
            lxx[lane] = lxy[lane] = lyy[lane] = 0.0;
            for (int j = 0; j < slots; ++j) {
                const int k = lane + L * j;
                if (k < npix) {
                    lk_window_pixel(A, w, h, plx, ply, k, r, a[k], ix[k], iy[k]);
                    lk_g_terms(ix[k], iy[k], lxx[lane], lxy[lane], lyy[lane]);
                }
            }
        }
        const double gxx = wave_sum(lxx), gxy = wave_sum(lxy), gyy = wave_sum(lyy);
        double vx = 0.0, vy = 0.0;
        if (lk_solvable(gxx, gxy, gyy, npix)) {
            for (int it = 0; it < iters; ++it) {
                double lbx[L], lby[L];
                for (int lane = 0; lane < L; ++lane) {
                    lbx[lane] = lby[lane] = 0.0;
                    for (int j = 0; j < slots; ++j) {
                        const int k = lane + L * j;
                        if (k < npix) lk_b_terms(a[k], lk_moved_sample(B, w, h, plx, ply, gx, gy, vx, vy, k, r), ix[k], iy[k], lbx[lane], lby[lane]);
                    }
                }
                const double bx = wave_sum(lbx), by = wave_sum(lby);
                lk_solve(gxx, gxy, gyy, bx, by, vx, vy);
            }
        }
        if (l == 0) {
            double ls[L];
            for (int lane = 0; lane < L; ++lane) {
                ls[lane] = 0.0;
                for (int j = 0; j < slots; ++j) {
                    const int k = lane + L * j;
                    if (k < npix) ls[lane] = ls[lane] + fabs(a[k] - lk_moved_sample(B, w, h, plx, ply, gx, gy, vx, vy, k, r));
                }
            }
            res = wave_sum(ls) / (double)npix;
            eig = lk_min_eig(gxx, gxy, gyy, npix);
            ox = plx + (gx + vx);
            oy = ply + (gy + vy);
        } else {
            gx = 2.0 * (gx + vx);
            gy = 2.0 * (gy + vy);
        }
    }
}

bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
bool put(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: lk_host_check IN OUT\n");
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    FILE* fo = fopen(argv[2], "wb");
    if (!fi || !fo) {
        fprintf(stderr, "lk_host_check: cannot open files\n");
        return 2;
    }
    int32_t hdr[7];
    float th[3];
    if (!get(fi, hdr, sizeof hdr) || !get(fi, th, sizeof th)) return 3;
    const int T = hdr[0], H = hdr[1], W = hdr[2], N = hdr[3], levels = hdr[4], r = hdr[5], iters = hdr[6];
    if (T < 1 || H < 1 || W < 1 || H > 4096 || W > 4096 || T > 256 || N < 0 || N > (1 << 16) || levels < 1 || levels > FP_LK_MAX_LEVELS ||
        r < 1 || r > FP_LK_MAX_RADIUS || iters < 1 || iters > FP_LK_MAX_ITERS)
        return 3;
    std::vector<uint8_t> frames((size_t)T * H * W * 3);
    std::vector<float> q((size_t)N * 3);
    if (!get(fi, frames.data(), frames.size()) || !get(fi, q.data(), q.size() * 4)) return 3;
    fclose(fi);

    LkPyramid P;
    const long long total = lk_pyramid_layout(T, H, W, levels, r, P);
    std::vector<float> pyr((size_t)total);
    for (long long i = 0; i < (long long)T * H * W; ++i) pyr[i] = lk_grey(frames[i * 3], frames[i * 3 + 1], frames[i * 3 + 2]);
    for (int l = 1; l < P.levels; ++l)
        for (int t = 0; t < T; ++t)
            for (int y = 0; y < P.h[l]; ++y)
                for (int x = 0; x < P.w[l]; ++x)
                    pyr[P.off[l] + ((long long)t * P.h[l] + y) * P.w[l] + x] =
                        lk_down_pixel(pyr.data() + P.off[l - 1] + (long long)t * P.h[l - 1] * P.w[l - 1], P.h[l - 1], P.w[l - 1], y, x);

    std::vector<float> tracks((size_t)T * N * 2, -1.0f), diag((size_t)T * N * 4, -1.0f);
    std::vector<uint8_t> vis((size_t)T * N, 255);
    std::vector<double> state((size_t)T * N * 2, -1.0);      // chain positions in fp64; tracks are their float32 copies
    for (int n = 0; n < N; ++n) {
        const int tq = lk_query_time(q[n * 3], T);
        const float x = lk_finite_or_zero(q[n * 3 + 1]), y = lk_finite_or_zero(q[n * 3 + 2]);
        const size_t row = (size_t)tq * N + n;
        const bool in = lk_inside(x, y, W, H);
        state[row * 2] = x;
        state[row * 2 + 1] = y;
        tracks[row * 2] = x;
        tracks[row * 2 + 1] = y;
        vis[row] = in ? 1 : 0;
        diag[row * 4] = diag[row * 4 + 1] = diag[row * 4 + 2] = 0.0f;
        diag[row * 4 + 3] = in ? 0.0f : (float)FP_LK_FLAG_OUTSIDE;
    }
    for (int step = 1; step < T; ++step)
        for (int item = 0; item < 2 * N; ++item) {
            const int n = item >> 1, dir = item & 1;
            const int tq = lk_query_time(q[n * 3], T);
            const int src = dir ? tq - (step - 1) : tq + (step - 1), dst = dir ? tq - step : tq + step;
            if (dst < 0 || dst >= T) continue;
            const size_t rs = (size_t)src * N + n, rd = (size_t)dst * N + n;
            const double sx = state[rs * 2], sy = state[rs * 2 + 1];
            double fx, fy, eig, res, bx, by, eig_b, res_b, fb;
            lk_run(P, pyr.data(), src, dst, sx, sy, r, iters, fx, fy, eig, res);
            lk_run(P, pyr.data(), dst, src, fx, fy, r, iters, bx, by, eig_b, res_b);
            const int flags = lk_judge(sx, sy, fx, fy, bx, by, eig, res, th[0], th[1], th[2], W, H, vis[rs] != 0, fb);
            state[rd * 2] = fx;
            state[rd * 2 + 1] = fy;
            tracks[rd * 2] = (float)fx;
            tracks[rd * 2 + 1] = (float)fy;
            vis[rd] = flags == 0 ? 1 : 0;
            diag[rd * 4] = (float)fb;
            diag[rd * 4 + 1] = (float)eig;
            diag[rd * 4 + 2] = (float)res;
            diag[rd * 4 + 3] = (float)flags;
        }
    const int32_t out_hdr[2] = {P.levels, (int32_t)total};
    if (!put(fo, out_hdr, sizeof out_hdr) || !put(fo, pyr.data(), pyr.size() * 4) || !put(fo, tracks.data(), tracks.size() * 4) ||
        !put(fo, vis.data(), vis.size()) || !put(fo, diag.data(), diag.size() * 4))
        return 4;
    if (fclose(fo) != 0) return 4;
    return 0;
}
