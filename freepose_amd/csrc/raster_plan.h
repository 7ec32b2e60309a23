// How a rasteriser call is launched: the visibility strategy (LDS-tiled or global buffer), the tile edge and grid, the chunk count and
// the rounds of the tile kernel's mask scan, the bin grid, the view groups of the XCD-major workgroup walk, the rgb flush form and the
// dynamic LDS — as ONE pure function of the frame, the triangle count, the view count and the context's "raster_tiled" option; and the
// constants of the per-triangle set-up that the kernels branch on.  Host-only C++17 without HIP types: raster.hip executes the plan and
// its kernels read the constants, tools/raster_plan_host_check.cpp and tests/test_raster_cases_cpu.py check it on a CPU,
// fp_op_raster_plan reads it out of the library.
#pragma once
#include <stddef.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define FP_RASTER_HD __host__ __device__
#else
#define FP_RASTER_HD
#endif

namespace fp_raster {

// ---- per-triangle set-up (raster.hip tri_setup_v, raster_vertex_kernel)
constexpr float ZNEAR = 0.05f;           // near plane (renderer.py:62-67 / pyrender's default)
constexpr float CLAMP_PX = 30000.f;      // window coordinates are clamped to +-CLAMP_PX px so the fixed-point products stay inside int64
constexpr int SMALL_SPAN = 32768;        // subpixels (128 px): a triangle spanning less in x and y has 32-bit edge functions (tri_cover32)
constexpr int BIG_AREA = 256;            // global path: bbox pixels above which a triangle goes to the wave-per-triangle queue
constexpr int BIG_TILE_AREA = 32;        // tiled path: candidate pixels in the tile above which a triangle is handed to the whole wave
                                         // (the per-lane coverage mask has 32 bits)
// ---- launch
constexpr int BIN_CHUNK = 64;            // triangles (Morton-ordered slots) per chunk: one wave of the bin kernel
constexpr int BIN_WAVES = 4;             // chunks per workgroup of the bin kernel
constexpr int HITS_ROUND = 2048;         // chunk masks examined per round of the tile kernel (8 per thread; 16-bit ids relative to the round's base)
constexpr int TILE_MIN = 64;             // tile edge of frames up to TILE_MIN * TILES_SIDE px
constexpr int TILE_MAX = 88;             // largest tile edge of the tiled path (its keys fit the LDS): frames up to 704 px
constexpr int TILES_SIDE = 8;            // at most 8 x 8 tiles: a chunk's tile mask has 64 bits, a triangle's tile box four nibbles
constexpr int TILED_MAX_TRIS = 131072;   // default strategy: meshes above this take the global buffer (measured, see rasterize_impl)
constexpr int TILE_THREADS = 256;        // workgroup of the tile kernel: its first 2 T threads fill the column and row factors
constexpr int LDS_BUDGET = 160 * 1024;   // per workgroup

FP_RASTER_HD constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
// tile edge: 64 px up to 512-px images, else the smallest multiple of 8 that covers the image with 8 x 8 tiles
FP_RASTER_HD constexpr int tile_edge(int W, int H) {
    return (W > H ? W : H) <= TILE_MIN * TILES_SIDE ? TILE_MIN : (cdiv(W > H ? W : H, TILES_SIDE) + 7) / 8 * 8;
}
// dynamic LDS of the tile kernel: visibility keys + DEC/THR tables (512 floats) + hit list + column / row factors
constexpr size_t tile_lds(int T) { return (size_t)T * T * 8 + 2048 + (size_t)HITS_ROUND * 2 + (size_t)2 * T * 8; }

// Workgroup L of a (nx, Hn) grid -> (item, view) with all items of a view on ONE XCD: workgroup L of a launch runs on XCD L % 8
// (observed; a speed hint only), so within a group of 8 views the linear id walks the views fastest; the remaining views item-fastest.
FP_RASTER_HD inline void view_major(int L, int nx, int Hn, int& item, int& h) {
    const int full = Hn & ~7, per_group = 8 * nx;
    if (L < (full >> 3) * per_group) {
        const int g = L / per_group, r = L - g * per_group;
        h = g * 8 + (r & 7); item = r >> 3;
    } else {
        const int r = L - (full >> 3) * per_group;
        h = full + r / nx; item = r - (r / nx) * nx;
    }
}

struct Plan {
    bool tiled;
    int T;                  // tile edge the frame asks for (the tiled path runs only when T <= TILE_MAX)
    int ntx, nty, ntile;    // tiled: tile grid; 0 on the global path
    int nchunk, rounds;     // chunks of BIN_CHUNK slots; rounds of HITS_ROUND chunk masks per tile workgroup
    int bin_grid;           // workgroups of the bin kernel per view
    int groups, rem;        // whole groups of 8 views and the remaining views of the view-major walk
    bool flush_dword;       // the tile kernel's rgb rows go out as whole dwords (else dwords + byte ends)
    size_t lds;             // dynamic LDS of the tile kernel
};

// mode = the context's "raster_tiled": < 0 (default) tiled for frames of up to 8 x 8 tiles of <= TILE_MAX px and meshes of up to
// TILED_MAX_TRIS triangles, 0 = global visibility buffer, 1 = tiled (wherever the frame fits)
inline Plan make_plan(int W, int H, int F, int Hn, int mode) {
    Plan p{};
    p.T = tile_edge(W, H);
    p.tiled = p.T <= TILE_MAX && (mode == 1 || (mode != 0 && F <= TILED_MAX_TRIS));
    p.groups = Hn >> 3;
    p.rem = Hn & 7;
    if (!p.tiled) return p;
    p.ntx = cdiv(W, p.T); p.nty = cdiv(H, p.T); p.ntile = p.ntx * p.nty;
    p.nchunk = cdiv(F, BIN_CHUNK);
    p.rounds = cdiv(p.nchunk, HITS_ROUND);
    p.bin_grid = cdiv(p.nchunk, BIN_WAVES);
    // rows start on a dword and hold whole groups of four pixels in every tile, the last column included (T is a multiple of 8)
    p.flush_dword = W % 4 == 0;
    p.lds = tile_lds(p.T);
    return p;
}

// "tiled T=80 tiles=8x1 chunks=5 rounds=1 bin=2 views=1+3 flush=bytes lds=69760 <constants>" | "global T=96 tiles=0x0 ... flush=none lds=0 ..."
inline int plan_text(const Plan& p, char* out, size_t n) {
    return snprintf(out, n,
                    "%s T=%d tiles=%dx%d chunks=%d rounds=%d bin=%d views=%d+%d flush=%s lds=%zu big_area=%d big_tile_area=%d chunk=%d "
                    "hits_round=%d small_span=%d max_tris=%d max_tile=%d clamp=%d znear=%g",
                    p.tiled ? "tiled" : "global", p.T, p.ntx, p.nty, p.nchunk, p.rounds, p.bin_grid, p.groups, p.rem,
                    !p.tiled ? "none" : p.flush_dword ? "dword" : "bytes", p.lds, BIG_AREA, BIG_TILE_AREA, BIN_CHUNK, HITS_ROUND, SMALL_SPAN,
                    TILED_MAX_TRIS, TILE_MAX, (int)CLAMP_PX, (double)ZNEAR);
}

}  // namespace fp_raster
