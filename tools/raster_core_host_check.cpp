// Host check of the rasteriser's per-triangle arithmetic (csrc/raster_core.h), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ifreepose_amd/csrc tools/raster_core_host_check.cpp -o raster_core_host_check
// Exit status 0 means that the claims the kernels rest on hold on this CPU, in the header's own text:
//   split   : split_rowcol(kk, bw) == (kk / bw, kk % bw) for every bw in 1..32 and kk < 32 (exhaustive)
//   edges   : for triangles whose spans are below SMALL_SPAN, corners anywhere in +-CLAMP_PX px, EdgeFn::weights<int> (24-bit multiplies,
//             emulated: an operand that does not fit gives a wrong product) == weights<long long> and accept agrees, at every pixel centre
//             inside the vertex box: N_TRI fixed-seed triangles (every 64th with spans up to the extreme 32767) + hand-placed extremes
//   bary    : for 0 <= w <= area2 < 2^31, bary_rcp == bary_quotient bit for bit: N_BARY fixed-seed pairs, powers of two and their
//             neighbours, area2 = 2 * 32767^2
//   key     : for positive finite depths key order == (depth, face) order, key_depth / key_face invert vis_key, KEY_NONE is above every key
// Then it reads lines "W H cull x0 y0 z0 x1 y1 z1 x2 y2 z2" (fixed-point window coordinates, eye depths) on stdin and prints for each
// "ok strad swapped area2 bx0 by0 bx1 by1 small back_facing" of tri_setup_v: tests/test_raster_cases_cpu.py compares them with
// tests/_raster_cases.py setup().
#include <float.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "raster_core.h"

using namespace fp_raster;

constexpr int N_TRI = 1000000, N_BARY = 10000000, N_KEY = 1000000;
constexpr int LIM = (int)CLAMP_PX * 256;   // fixed-point window coordinates lie in [-LIM, LIM]

static int fails = 0;
#define CHECK(c, ...)                                                        \
    do {                                                                     \
        if (!(c)) {                                                          \
            if (fails < 20) { printf("FAILED %s:%d: %s  ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } \
            ++fails;                                                         \
        }                                                                    \
    } while (0)

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;   // splitmix64, fixed seed
static unsigned long long rnd() {
    unsigned long long z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned long long)((long long)hi - lo + 1)); }   // inclusive

static void check_split() {
    for (int bw = 1; bw <= 32; ++bw) {
        const float rbw = split_rcp(bw);
        for (int kk = 0; kk < 32; ++kk) {
            int row, col;
            split_rowcol(kk, bw, rbw, row, col);
            CHECK(row == kk / bw && col == kk % bw, "kk=%d bw=%d -> row %d col %d", kk, bw, row, col);
        }
    }
}

static SVert front(int xi, int yi) { return SVert{xi, yi, 1.0f, 1.0f}; }

// both integer paths at every pixel centre inside the vertex box; returns the number of pixels walked
static long check_edges(int x0, int y0, int x1, int y1, int x2, int y2) {
    const TriSetup t = tri_setup_v(front(x0, y0), front(x1, y1), front(x2, y2), 1 << 30, 1 << 30);
    CHECK(t.small && !t.strad, "(%d,%d) (%d,%d) (%d,%d)", x0, y0, x1, y1, x2, y2);
    if (!t.small) return 0;
    const int mnx = imin(x0, imin(x1, x2)), mxx = imax(x0, imax(x1, x2)), mny = imin(y0, imin(y1, y2)), mxy = imax(y0, imax(y1, y2));
    const EdgeFn e(t);
    long n = 0;
    for (int py = (mny - 128 + 255) >> 8; py <= (mxy - 128) >> 8; ++py)
        for (int px = (mnx - 128 + 255) >> 8; px <= (mxx - 128) >> 8; ++px, ++n) {
            long long w0, w1, w2;
            int v0, v1, v2;
            e.weights(pixel_centre<long long>(px), pixel_centre<long long>(py), w0, w1, w2);
            e.weights(pixel_centre<int>(px), pixel_centre<int>(py), v0, v1, v2);
            CHECK(w0 == v0 && w1 == v1 && w2 == v2 && e.accept(w0, w1, w2) == e.accept(v0, v1, v2), "(%d,%d) (%d,%d) (%d,%d) at pixel (%d,%d)",
                  x0, y0, x1, y1, x2, y2, px, py);
            long long c0, c1, c2;   // and the per-pixel statement of both paths (tri_cover: top-left rule evaluated in place) against the object
            int d0, d1, d2;
            CHECK(tri_cover<long long>(t, px, py, c0, c1, c2) == e.accept(w0, w1, w2) && c0 == w0 && c1 == w1 && c2 == w2, "tri_cover<long long> at (%d,%d)", px, py);
            CHECK(tri_cover<int>(t, px, py, d0, d1, d2) == e.accept(w0, w1, w2) && d0 == w0 && d1 == w1 && d2 == w2, "tri_cover<int> at (%d,%d)", px, py);
        }
    return n;
}

static void check_edge_sweep() {
    long pixels = 0;
    const int S = SMALL_SPAN - 1;   // the extreme span
    for (const int ox : {-LIM, -S / 2, 0, LIM - S})
        for (const int oy : {-LIM, 0, LIM - S}) {
            pixels += check_edges(ox, oy, ox + S, oy, ox, oy + S);
            pixels += check_edges(ox + S, oy + S, ox, oy + S, ox + S, oy);
            pixels += check_edges(ox, oy, ox + S, oy + S, ox + S, oy + 1);          // slivers along the diagonal and the axes
            pixels += check_edges(ox, oy, ox + S, oy, ox + S / 2, oy + 1);
            pixels += check_edges(ox, oy, ox, oy + S, ox + 1, oy + S / 2);
            pixels += check_edges(ox, oy + S, ox + S, oy, ox + S, oy + S);
        }
    for (int i = 0; i < N_TRI; ++i) {
        const int bits = i % 64 == 0 ? 15 : 1 + (int)(rnd() % 11);                  // mostly a few pixels, every 64th up to 128 px
        const int sx = (int)(rnd() & ((1u << bits) - 1)), sy = (int)(rnd() & ((1u << bits) - 1));
        const int ox = rnd_in(-LIM, LIM - sx), oy = rnd_in(-LIM, LIM - sy);
        pixels += check_edges(rnd_in(ox, ox + sx), rnd_in(oy, oy + sy), rnd_in(ox, ox + sx), rnd_in(oy, oy + sy), rnd_in(ox, ox + sx), rnd_in(oy, oy + sy));
    }
    fprintf(stderr, "edges: %d triangles + extremes, %ld pixel centres\n", N_TRI, pixels);
}

static void check_bary_pair(long long area2, long long w) {
    TriSetup t{};
    t.area2 = area2;
    const float q = bary_quotient((int)w, (float)t.area2), r = bary_rcp((int)w, area_rcp(t));
    CHECK(bit_cast<unsigned>(q) == bit_cast<unsigned>(r), "w=%lld area2=%lld: quotient %a reciprocal %a", w, area2, (double)q, (double)r);
    CHECK(bary_quotient(w, (float)t.area2) == q, "w=%lld as int and as long long", w);
}

static void check_bary() {
    const long long top = 2ll * 32767 * 32767;
    for (int k = 0; k <= 30; ++k)
        for (int da = -1; da <= 1; ++da) {
            const long long a = (1ll << k) + da;
            if (a < 1) continue;
            for (int j = 0; j <= k; ++j)
                for (int dw = -1; dw <= 1; ++dw) {
                    const long long w = (1ll << j) + dw;
                    if (w >= 0 && w <= a) check_bary_pair(a, w);
                }
            check_bary_pair(a, a); check_bary_pair(a, a / 3); check_bary_pair(top, a < top ? a : top);
        }
    for (const long long w : {0ll, 1ll, top / 2, top - 1, top}) check_bary_pair(top, w);
    for (int i = 0; i < N_BARY; ++i) {
        const long long a = 1 + (long long)(rnd() % ((1ull << (1 + rnd() % 31)) - 1));      // 1 <= area2 < 2^31, every magnitude
        check_bary_pair(a, (long long)(rnd() % (unsigned long long)(a + 1)));
    }
}

static void check_key() {
    const float special[] = {FLT_TRUE_MIN, FLT_MIN, 0.05f, 1.0f, 1.0f + FLT_EPSILON, 64.0f, FLT_MAX};
    auto one = [](float d1, int f1, float d2, int f2) {
        const unsigned long long k1 = vis_key(d1, f1), k2 = vis_key(d2, f2);
        CHECK(key_depth(k1) == d1 && key_face(k1) == f1 && k1 < KEY_NONE, "d=%a f=%d", (double)d1, f1);
        const bool lt = d1 < d2 || (d1 == d2 && f1 < f2);
        CHECK((k1 < k2) == lt && (k1 == k2) == (d1 == d2 && f1 == f2), "(%a, %d) against (%a, %d)", (double)d1, f1, (double)d2, f2);
    };
    for (const float a : special)
        for (const float b : special)
            for (const int f1 : {0, 1, 0x7fffffff})
                for (const int f2 : {0, 1, 0x7fffffff}) one(a, f1, b, f2);
    for (int i = 0; i < N_KEY; ++i) {
        const float d1 = bit_cast<float>(1u + (unsigned)(rnd() % 0x7f7fffffu));      // every positive finite float
        const float d2 = i % 4 == 0 ? d1 : bit_cast<float>(1u + (unsigned)(rnd() % 0x7f7fffffu));
        one(d1, (int)(rnd() & 0x7fffffff), d2, (int)(rnd() & 0x7fffffff));
    }
}

int main() {
    check_split();
    check_edge_sweep();
    check_bary();
    check_key();
    int W, H, cull, x[3], y[3];
    float z[3];
    while (scanf("%d %d %d %d %d %f %d %d %f %d %d %f", &W, &H, &cull, &x[0], &y[0], &z[0], &x[1], &y[1], &z[1], &x[2], &y[2], &z[2]) == 12) {
        SVert sv[3];
        for (int k = 0; k < 3; ++k) sv[k] = SVert{x[k], y[k], z[k] > ZNEAR ? 1.0f / z[k] : 0.f, z[k]};
        const int32_t faces[3] = {0, 1, 2};
        const TriSetup t = tri_setup_v(sv[0], sv[1], sv[2], W, H);
        printf("%d %d %d %lld %d %d %d %d %d %d\n", (int)t.ok, (int)t.strad, (int)t.swapped, t.area2, t.bx0, t.by0, t.bx1, t.by1, (int)t.small,
               (int)back_facing(t, sv, faces, 0));
    }
    if (fails) printf("%d checks FAILED\n", fails);
    return fails ? 1 : 0;
}
