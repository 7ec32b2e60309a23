// scale_host_check — runs the index arithmetic of freepose_amd/csrc/scale_core.h serially, in the phase order of scale.hip (tile-local
// union-find with tile-local indices, seam merge, compression; areas and the arg-max; row and column distance passes; survivor counts
// and the radius choice), on masks read from a file.  Plain C++ with its own main: build it with
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I freepose_amd/csrc tools/scale_host_check.cpp
// and compare its output with scipy (tests/test_scale_host_cpu.py).  This is the part of the depth-map scale that can be debugged
// on a machine without a GPU.
//
// input : int32 {n, H, W, connectivity, min_vertices}, float64 erosion_radius, then n * H * W mask bytes
// output: per mask  int32 labels[H * W] (0 = background, else 1 + raster index of the component's first pixel),
//                   int32 {root of the largest component (-1: empty), its area, steps, radius index, survivors},
//                   int32 cnt[5], uint8 d2[H * W]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "scale_core.h"

namespace {
constexpr int TILE = 32;

struct SerialLabels {
    int* L;
    int operator()(int i) const { return L[i]; }
};
struct SerialMin {
    int* L;
    int operator()(int i, int v) const {
        const int old = L[i];
        if (v < old) L[i] = v;
        return old;
    }
};

void label(const uint8_t* mask, int H, int W, bool conn8, std::vector<int>& uf, std::vector<int>& labels) {
    uf.assign((size_t)H * W, -1);
    // phase 1: every tile on its own, local indices
    for (int y0 = 0; y0 < H; y0 += TILE)
        for (int x0 = 0; x0 < W; x0 += TILE) {
            int L[TILE * TILE];
            for (int i = 0; i < TILE * TILE; ++i) {
                const int gy = y0 + i / TILE, gx = x0 + i % TILE;
                L[i] = (gy < H && gx < W && mask[(size_t)gy * W + gx]) ? i : -1;
            }
            const SerialLabels load{L};
            const SerialMin amin{L};
            for (int i = 0; i < TILE * TILE; ++i) {
                const int ly = i / TILE, lx = i % TILE;
                if (L[i] < 0) continue;
                if (lx > 0 && L[i - 1] >= 0) cc_union(load, amin, i, i - 1);
                if (ly > 0 && L[i - TILE] >= 0) cc_union(load, amin, i, i - TILE);
                if (conn8 && ly > 0) {
                    if (lx > 0 && L[i - TILE - 1] >= 0) cc_union(load, amin, i, i - TILE - 1);
                    if (lx < TILE - 1 && L[i - TILE + 1] >= 0) cc_union(load, amin, i, i - TILE + 1);
                }
            }
            for (int i = 0; i < TILE * TILE; ++i) {
                const int gy = y0 + i / TILE, gx = x0 + i % TILE;
                if (gy >= H || gx >= W || L[i] < 0) continue;
                const int r = cc_find(load, i);
                uf[(size_t)gy * W + gx] = (y0 + r / TILE) * W + x0 + r % TILE;
            }
        }
    // phase 2: seams
    const SerialLabels load{uf.data()};
    const SerialMin amin{uf.data()};
    for (int p = 0; p < H * W; ++p) {
        if (uf[p] < 0) continue;
        const int y = p / W, x = p % W;
        const bool left = x % TILE == 0, top = y % TILE == 0, right = x % TILE == TILE - 1;
        if (left && x > 0 && uf[p - 1] >= 0) cc_union(load, amin, p, p - 1);
        if (top && y > 0 && uf[p - W] >= 0) cc_union(load, amin, p, p - W);
        if (conn8 && y > 0) {
            if ((left || top) && x > 0 && uf[p - W - 1] >= 0) cc_union(load, amin, p, p - W - 1);
            if ((right || top) && x < W - 1 && uf[p - W + 1] >= 0) cc_union(load, amin, p, p - W + 1);
        }
    }
    // phase 3: compression
    labels.assign((size_t)H * W, 0);
    for (int p = 0; p < H * W; ++p)
        if (uf[p] >= 0) labels[p] = cc_find(load, p) + 1;
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
        return 2;
    }
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 2; }
    int hdr[5];
    double radius;
    if (fread(hdr, sizeof(int), 5, fi) != 5 || fread(&radius, sizeof(double), 1, fi) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const int n = hdr[0], H = hdr[1], W = hdr[2], conn = hdr[3], min_vertices = hdr[4];
    if (n < 0 || H < 1 || W < 1 || (conn != 4 && conn != 8) || !(radius > 0.0 && radius <= 8.0)) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t HW = (size_t)H * W;
    std::vector<uint8_t> masks((size_t)n * HW);
    if (fread(masks.data(), 1, masks.size(), fi) != masks.size()) { fprintf(stderr, "short masks\n"); return 2; }
    fclose(fi);
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    int thr[FP_SCALE_MAX_STEPS];
    const int steps = scale_radius_chain(radius, thr);
    std::vector<int> uf, labels, area;
    std::vector<uint8_t> d2(HW), rd(HW);
    for (int m = 0; m < n; ++m) {
        label(masks.data() + m * HW, H, W, conn == 8, uf, labels);
        area.assign(HW, 0);
        for (size_t p = 0; p < HW; ++p)
            if (labels[p]) ++area[labels[p] - 1];
        unsigned long long best = 0;                       // the device's atomicMax key
        for (size_t p = 0; p < HW; ++p)
            if (labels[p] == (int)p + 1) {
                const unsigned long long key = ((unsigned long long)(unsigned)area[p] << 32) | (0xffffffffu - (unsigned)p);
                best = key > best ? key : best;
            }
        const int barea = (int)(best >> 32), root = barea ? (int)(0xffffffffu - (unsigned)(best & 0xffffffffu)) : -1;
        int cnt[FP_SCALE_MAX_STEPS] = {0, 0, 0, 0, 0};
        for (size_t p = 0; p < HW; ++p) d2[p] = rd[p] = 0;
        if (barea) {
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    rd[(size_t)y * W + x] = (uint8_t)edt_row_dist(
                        [&](int xx) { return xx < 0 || xx >= W || labels[(size_t)y * W + xx] == root + 1; }, x);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const int v = edt_col_d2([&](int dy) {
                        const int yy = y + dy;
                        return (yy < 0 || yy >= H) ? FP_SCALE_WIN + 1 : (int)rd[(size_t)yy * W + x];
                    });
                    d2[(size_t)y * W + x] = (uint8_t)v;
                    for (int s = 0; s < steps; ++s) cnt[s] += v > thr[s];
                }
        }
        const int ridx = scale_choose_radius(cnt, steps, min_vertices);
        int survivors = 0;
        const int tsel = ridx < steps ? thr[ridx] : 0;
        for (size_t p = 0; p < HW; ++p) survivors += d2[p] > tsel;
        const int rec[5] = {root, barea, steps, ridx, survivors};
        fwrite(labels.data(), sizeof(int), HW, fo);
        fwrite(rec, sizeof(int), 5, fo);
        fwrite(cnt, sizeof(int), FP_SCALE_MAX_STEPS, fo);
        fwrite(d2.data(), 1, HW, fo);
    }
    // key transform: order and round trip on a few doubles
    const double probe[] = {-1e300, -2.5, -1e-300, -0.0, 0.0, 1e-300, 0.0625, 2.5, 1e300};
    for (size_t i = 0; i + 1 < sizeof(probe) / sizeof(probe[0]); ++i) {
        uint64_t a, b;
        __builtin_memcpy(&a, &probe[i], 8);
        __builtin_memcpy(&b, &probe[i + 1], 8);
        if (!(scale_key_bits(a) < scale_key_bits(b)) || scale_unkey_bits(scale_key_bits(a)) != a) {
            fprintf(stderr, "key transform broken at probe %zu\n", i);
            return 1;
        }
    }
    if (scale_n_keep(30, 40, 25) != 30 || scale_n_keep(40, 40, 25) != 25 || scale_n_keep(10, 40, 25) != 25 || scale_n_keep(24, 24, 25) != 24) {
        fprintf(stderr, "scale_n_keep broken\n");
        return 1;
    }
    fclose(fo);
    return 0;
}
