// Host check of the rasteriser's launch arithmetic (csrc/raster_plan.h), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ifreepose_amd/csrc tools/raster_plan_host_check.cpp -o raster_plan_host_check
// Reads lines "W H F Hn mode" on stdin (mode = the context's raster_tiled: -1, 0 or 1) and prints for each the text fp_op_raster_plan
// writes for that call.  Before that it holds the plan, over a sweep of W, H in 1..8192, F in 1..2^21, Hn in 0..600 and the three modes, to
// what the kernels rely on: at most 8 x 8 tiles that cover the frame, 2 T threads for the column and row factors, the LDS budget, tile
// boxes that fit their nibbles, chunk ids of a round that fit 16 bits, and a workgroup walk (view_major) that visits every (item, view)
// of the bin and tile grids exactly once.  tests/test_raster_cases_cpu.py compares the output with tests/_raster_cases.py plan().
#include <stdio.h>

#include <vector>

#include "raster_plan.h"

static int fails = 0;
#define CHECK(c)                                                                                 \
    do {                                                                                         \
        if (!(c)) {                                                                              \
            if (fails < 20) printf("FAILED %s:%d: %s (W=%d H=%d F=%d Hn=%d mode=%d)\n", __FILE__, __LINE__, #c, W, H, F, Hn, mode); \
            ++fails;                                                                             \
        }                                                                                        \
    } while (0)

using namespace fp_raster;

static void check_plan(int W, int H, int F, int Hn, int mode) {
    const Plan p = make_plan(W, H, F, Hn, mode);
    const int side = W > H ? W : H;
    CHECK(p.T % 8 == 0 && p.T >= TILE_MIN && p.T * TILES_SIDE >= side);
    CHECK(p.T == TILE_MIN || (p.T - 8) * TILES_SIDE < side);                       // the smallest such edge
    CHECK(p.groups * 8 + p.rem == Hn && p.rem >= 0 && p.rem < 8);
    const bool fits = side <= TILE_MAX * TILES_SIDE;
    CHECK(p.tiled == (fits && (mode == 1 || (mode != 0 && F <= TILED_MAX_TRIS))));
    if (!p.tiled) {
        CHECK(p.ntile == 0 && p.nchunk == 0 && p.rounds == 0 && p.bin_grid == 0 && p.lds == 0);
        return;
    }
    CHECK(p.ntx >= 1 && p.nty >= 1 && p.ntx <= TILES_SIDE && p.nty <= TILES_SIDE && p.ntile == p.ntx * p.nty);
    CHECK(p.T * p.ntx >= W && p.T * (p.ntx - 1) < W && p.T * p.nty >= H && p.T * (p.nty - 1) < H);
    CHECK(2 * p.T <= TILE_THREADS);                                                 // column and row factor init: one thread each
    CHECK(p.lds == tile_lds(p.T) && p.lds <= (size_t)LDS_BUDGET);
    CHECK((W - 1) / p.T <= 15 && (H - 1) / p.T <= 15 && (H - 1) / p.T * 8 + (W - 1) / p.T < 64);   // tile nibbles and mask bits
    CHECK((long)p.nchunk * BIN_CHUNK >= F && (long)(p.nchunk - 1) * BIN_CHUNK < F);
    CHECK((long)p.rounds * HITS_ROUND >= p.nchunk && (long)(p.rounds - 1) * HITS_ROUND < p.nchunk && HITS_ROUND <= 65536);
    CHECK(p.bin_grid * BIN_WAVES >= p.nchunk && (p.bin_grid - 1) * BIN_WAVES < p.nchunk);
    // dword flush: every tile row starts on a dword of the rgb buffer and holds whole groups of four pixels
    bool dword = (W * 3) % 4 == 0 && p.T % 4 == 0;
    for (int tx = 0; tx < p.ntx; ++tx) {
        const int tw = (W < (tx + 1) * p.T ? W : (tx + 1) * p.T) - tx * p.T;
        if (tw % 4) dword = false;
    }
    CHECK(p.flush_dword == dword);
}

// view_major over a whole (nx, Hn) grid: a bijection onto items x views
static void check_walk(int nx, int Hn) {
    const int W = nx, H = 0, F = 0, mode = 0;   // (what CHECK prints)
    std::vector<unsigned char> seen((size_t)nx * (Hn > 0 ? Hn : 1), 0);
    for (int L = 0; L < nx * Hn; ++L) {
        int item = -1, h = -1;
        view_major(L, nx, Hn, item, h);
        CHECK(item >= 0 && item < nx && h >= 0 && h < Hn);
        if (item < 0 || item >= nx || h < 0 || h >= Hn) return;
        CHECK(!seen[(size_t)h * nx + item]);
        seen[(size_t)h * nx + item] = 1;
        if (h < (Hn & ~7)) CHECK(L % 8 == h % 8);                                   // whole groups: a view keeps its XCD
    }
}

int main() {
    static_assert(tile_edge(512, 1) == 64 && tile_edge(513, 1) == 72 && tile_edge(576, 576) == 72 && tile_edge(577, 1) == 80 &&
                      tile_edge(640, 480) == 80 && tile_edge(641, 1) == 88 && tile_edge(704, 704) == 88 && tile_edge(705, 1) == 96, "tile edge");
    const int Hs[] = {1, 2, 63, 64, 65, 511, 512, 513, 576, 577, 640, 641, 703, 704, 705, 1024, 8191, 8192};
    const int Fs[] = {1, 63, 64, 65, 255, 256, 257, 131071, 131072, 131073, 135168, 1 << 20, (1 << 21) - 1, 1 << 21};
    for (int W = 1; W <= 8192; ++W)
        for (const int H : Hs)
            for (int mode = -1; mode <= 1; ++mode) {
                check_plan(W, H, 1000, 11, mode);
                check_plan(H, W, 131073, 8, mode);
            }
    for (int k = 0; k <= 21; ++k)
        for (int d = -1; d <= 1; ++d) {
            const int F = (1 << k) + d;
            if (F < 1 || F > (1 << 21)) continue;
            for (int mode = -1; mode <= 1; ++mode)
                for (const int Hn : {0, 1, 7, 8, 9, 576, 600}) { check_plan(420, 420, F, Hn, mode); check_plan(640, 480, F, Hn, mode); check_plan(708, 24, F, Hn, mode); }
        }
    for (const int F : Fs)
        for (int Hn = 0; Hn <= 600; ++Hn) check_plan(131, 70, F, Hn, -1);
    // the grids the two view-major kernels are launched with: 1 .. 64 tiles, cdiv(nchunk, 4) bin workgroups
    for (const int nx : {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 100, 512, 513, 528, 8192})
        for (int Hn = 0; Hn <= 600; Hn += (nx > 100 && Hn >= 24 ? 97 : 1)) check_walk(nx, Hn);

    int W, H, F, Hn, mode;
    char text[384];
    while (scanf("%d %d %d %d %d", &W, &H, &F, &Hn, &mode) == 5) {
        check_plan(W, H, F, Hn, mode);
        const int k = plan_text(make_plan(W, H, F, Hn, mode), text, sizeof text);
        CHECK(k > 0 && (size_t)k < sizeof text);
        puts(text);
    }
    if (fails) printf("%d checks FAILED\n", fails);
    return fails ? 1 : 0;
}
