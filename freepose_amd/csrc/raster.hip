// Pose-hypothesis rasteriser (K15 of SURVEY.md §2.3), gfx950 only.  Replaces pyrender's OpenGL path used by
// MeshRenderer.render_from_poses (src/pipeline/retrieval/renderer.py:70-95): one mesh, Hn poses, pinhole
// intrinsics, ambient-only shading, no face culling, rgb u8 + metric eye-depth f32 (0 = background).
//
// Arithmetic contract (shared with oracle/fp_oracle.c, every step fp32 IEEE unless noted):
//   vertex : s = scale*v ; Xc = fma(R00,sx, fma(R01,sy, fma(R02,sz, tx))) (same for Yc, Zc)
//            iz = 1/Zc ; u = fma(fx, Xc*iz, cx) ; v = fma(fy, Yc*iz, cy)
//            fixed point 24.8 : xi = rint(u*256), yi = rint(v*256)      (image coords, y down)
//   near plane (znear = 0.05, renderer.py:62-67 / pyrender's default): a triangle with all three Zc <= znear is dropped; one that
//   STRADDLES the plane is rasterised in homogeneous coordinates, which clips it exactly at z = znear without generating geometry:
//       vertex k -> (xk, yk, wk) = (pixel x * z, pixel y * z, z): for Zc > znear from the snapped fixed-point pixel (xi / 256 * Zc, so
//       edges shared with ordinary triangles coincide), else xk = fma(fx, Xc, cx * Zc), yk likewise (stored as float bits in xi / yi);
//       in double: a0 = y1 w2 - y2 w1, b0 = x2 w1 - x1 w2, c0 = x1 y2 - x2 y1 (cyclic for 1, 2), det = x0 a0 + y0 b0 + w0 c0;
//       pixel (px, py): X = px + 0.5, Y = py + 0.5, e_i = (a_i X + b_i Y) + c_i, all negated when det < 0;
//       covered iff e0, e1, e2 >= 0, S = (e0 + e1) + e2 > 0 and z = |det| / S > znear; depth = (float) z;
//       barycentrics (float)(e_i / S) are perspective-correct; colour / uv interpolate with them directly, textures at level 0.
//   coverage: sample (256 px + 128, 256 py + 128); int64 edge functions; orientation normalised by
//            swapping v1,v2 when the doubled area is negative (SKIP_CULL_FACES); top-left rule on ties
//   depth  : b_i = float(E_i)/float(area2) ; izp = fma(b2,iz2, fma(b1,iz1, b0*iz0)) ; depth = 1/izp
//   visibility: 64-bit key (depth bits << 32 | triangle id), atomic MIN -> nearest depth, lowest id on
//            exact ties; order independent, hence deterministic
//   base colour of the visible fragment, q_i = b_i*iz_i:
//            vertex colours : cv = fma(q2,c2, fma(q1,c1, q0*c0)) * depth                      (0..255 units)
//            textured mesh  : per-corner UV, U = fma(q2,u2, fma(q1,u1, q0*u0)) * depth (same for V).  The texture is filtered
//                             as stored (u8 values 0..255, the image's gamma space — a GL_RGBA8 texture):
//              level k      : max(1, tw>>k) x max(1, th>>k); level k+1 = 2x2 box of level k, (a+b+c+d+2)>>2 per channel (built on
//                             the host at upload; second row / column clamped when the source size is 1)
//              bilinear(k)  : x = U*wk - 0.5, y = (1-V)*hk - 0.5 (v = 1 at the image's first row), (x0,y0) = floor, REPEAT wrap,
//                             top = fma(wx, t01-t00, t00), bot = fma(wx, t11-t10, t10), val = fma(wy, bot-top, top)
//              level of detail (filter 1, default: GL_LINEAR_MIPMAP_LINEAR with ANALYTIC derivatives — what pyrender's sampler
//                             asks GL for): g?_i = d(b_i)/d(px|py) * iz_i are constants of the triangle;
//                             dU/dx = fma(gx2,u2-U, fma(gx1,u1-U, gx0*(u0-U))) * depth (same for V, y);
//                             rho2 = max((dU/dx*tw)^2 + (dV/dx*th)^2, (dU/dy*tw)^2 + (dV/dy*th)^2);
//                             rho2 <= 1 (magnification) or a single level: bilinear(0); else e = exponent(rho2), m = mantissa,
//                             lg = LOG2P(m-1) (degree-5 polynomial in fmaf steps, |err| < 2e-5), l0 = e>>1,
//                             fr = 0.5*((e&1) + lg); l0 >= last: bilinear(last); else val = fma(fr, bilinear(l0+1)-bilinear(l0), bilinear(l0))
//                             filter 0: bilinear(0) always
//              shade 1      : lin = sRGB->linear of val/255 by linear interpolation in DEC[256] (i = min(int(val),254),
//                             lin = fma(val-i, DEC[i+1]-DEC[i], DEC[i])): sample, THEN decode (a shader's srgb_to_linear(texture()));
//                             c = lin*Kd.      shade 0: c255 = val*Kd
//   output : shade 1 (default, "gamma"): u8 = #{k in 1..255 : THR[k] <= a*c}, THR[k] = ((k-.5)/255)^2.2, i.e.
//            round(255 (a c)^(1/2.2)) found by table search so that host oracle and device agree bit for bit (vertex: c = cv/255)
//            shade 0 ("linear", the round-1 rule): (u8) min(255, a*cv + 0.5)                  (textured: cv = c255)
//            a = ambient light factor: 2 by default (renderer.py:53-55), 5 in tracking_refiner.py:33.
//   pyrender's fragment shader is third-party and absent from /root/reference: the shading rule is STATED here, not pinned
//   (DESIGN.md §5).  A GPU derives the level of detail from 2x2-quad finite differences with a few fractional bits; the analytic
//   derivative used here is the quantity those approximate.
// Launch shape (the plan is fp_raster::make_plan, raster_plan.h; the arithmetic above is raster_core.h): vertex kernel (Hn x V threads), then
//   tiled (frames up to 704 px, up to 131 072 triangles): bin kernel (one wave per chunk of 64 Morton-ordered triangles: tile boxes and chunk
//     masks), tile kernel (one workgroup per view and screen tile: visibility keys in LDS, resolve and flush in place, one extents record),
//     extents kernel (one wave per view folds the records) when boxes / extents are asked for;
//   global buffer (everything else): triangle kernel (Hn x F threads; small triangles are rasterised by their thread, large ones and
//     straddlers by a whole wave of the big kernel via a queue), resolve kernel (Hn x pixels), fp_depth_extents on the depth image.
#include "../../include/freepose_hip.h"
#include "internal.h"
#include "raster_plan.h"   // the launch arithmetic and every threshold the kernels branch on, stated once (checked on a CPU)
#include "raster_core.h"   // the per-vertex and per-triangle arithmetic, stated once for host and device (checked on a CPU)

#include <algorithm>
#include <memory>

// what shading reads of a mesh, as the kernels take it (shade_fragment; arithmetic = the contract above)
struct ShadeArgs {
    const uint8_t* colors = nullptr;   // [V,4] rgba (a unused), by device vertex id; null: white
    const float* uv = nullptr;         // [F,3,2] per-corner texture coordinates (textured meshes)
    const uint8_t* tex = nullptr;      // rgba diffuse texture, all mip levels back to back (level k at texel offset lev_off[k])
    int th = 0, tw = 0;
    float kd0 = 1.f, kd1 = 1.f, kd2 = 1.f;   // material diffuse factor (MTL Kd / glTF baseColorFactor)
    float ambient = 2.0f;              // scene ambient light factor: 2 in renderer.py:53-55, 5 in tracking_refiner.py:33
    int shade = 1;                     // 1 = gamma rule, 0 = linear
    int nlev = 0, filter = 1;          // mip levels; 1 = trilinear mip-maps, 0 = bilinear level 0
    uint32_t lev_off[16] = {};
};

struct fp_mesh {
    fp_ctx* ctx = nullptr;
    float* verts = nullptr;    // [V,3]
    int32_t* faces = nullptr;  // [F,3]
    int32_t* perm = nullptr;   // [F] slot -> face id, Morton order of the object-space centroids (tiled path: coherent 64-triangle chunks)
    int32_t* fsort = nullptr;  // [F,3] faces[perm[slot]]: the corner ids in slot order (read coalesced by the bin / tile kernels)
    std::vector<int32_t> h_vmap;   // host copy of vmap (per-vertex attributes are stored by device id)
    int32_t* vmap = nullptr;   // [V] caller's vertex id -> device vertex id (vertices are stored in order of first use by the Morton-sorted
                               // triangles, so the 3 x 64 vertex gathers of a chunk hit a few cache lines instead of one line each).  Purely
                               // internal: outputs carry no vertex id, fp_project_vertices maps back
    ShadeArgs sh;              // colours or texture, material, shading rule
    int cull = 0;              // 1 = back faces are not drawn (renderer.py:63-66: render without SKIP_CULL_FACES), 0 = both sides
    float* tables = nullptr;   // DEC[256] sRGB->linear, THR[256] gamma-encode thresholds
    int V = 0, F = 0;
};

namespace {

using namespace fp_raster;     // raster_core.h: SVert, TriSetup, EdgeFn, barycentrics, visibility key, Strad; raster_plan.h: the thresholds

__global__ void raster_vertex_kernel(const float* __restrict__ verts, int V, const float* __restrict__ poses, int Hn,
                                     float scale, float fx, float fy, float cx, float cy, SVert* __restrict__ sv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, h = blockIdx.y;
    if (i >= V) return;
    sv[(size_t)h * V + i] = project_vertex(poses + (size_t)h * 16, verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], scale, fx, fy, cx, cy);
}

__device__ __forceinline__ TriSetup tri_setup(const SVert* __restrict__ sv, const int32_t* __restrict__ faces, int f, int W, int Hh) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    return tri_setup_v(sv[i0], sv[i1], sv[i2], W, Hh);
}

// ---- where a fragment's visibility key goes.  NARROW: the sink's small triangles take the 32-bit edge functions (fragment<NARROW>)
struct GlobalSink {   // the global visibility buffer of one view
    static constexpr bool NARROW = false;
    unsigned long long* __restrict__ zb;   // [Hh, W]
    int W;
    __device__ __forceinline__ void put(int px, int py, unsigned long long key) const {
        // (a read-before-atomic "cannot win" test was measured here: the scattered 8-byte loads cost more than the L2 atomics
        //  they save — 2.4 -> 3.5 ms per 576 views — so the atomic is issued unconditionally)
        atomicMin(&zb[(size_t)py * W + px], key);
    }
};
// the tiled path's sink, and what the stages of raster_tile_kernel share: this workgroup's tile, its dynamic LDS, the view's vertices
struct TileCtx {
    static constexpr bool NARROW = true;
    int h, tx, ty, W, Hh;           // view, tile coordinates, frame
    int X0, Y0, X1, Y1, T;          // the tile's pixels (inclusive, clipped to the frame) and the tile edge = LDS row pitch
    unsigned long long* tile;       // [T*T] visibility keys; after resolve_tile depth bits << 32 | b << 16 | g << 8 | r
    float* tab;                     // DEC / THR tables (512 floats)
    unsigned short* hits;           // [HITS_ROUND] chunks of the round that touch the tile, relative to the round's base
    double *ax, *ay;                // [T] each: (pixel - c) / f of the tile's columns / rows
    const SVert* sv;                // the view's vertices; below: the mesh's faces by device vertex id
    const int32_t* faces;
    int lane, wave;
    __device__ __forceinline__ int tw() const { return X1 - X0 + 1; }
    __device__ __forceinline__ int th() const { return Y1 - Y0 + 1; }
    __device__ __forceinline__ void put(int px, int py, unsigned long long key) const {
        unsigned long long* slot = &tile[(py - Y0) * T + (px - X0)];
        // stored keys only ever decrease, so a plain (possibly stale) read bounds the current value from above: a key that does
        // not beat it cannot change the slot (LDS reads are cheap; the same test on the global buffer is a loss, see GlobalSink)
        if (key >= *(volatile unsigned long long*)slot) return;
        atomicMin(slot, key);
    }
};
// the one fragment emitter: triangle f, set up as `g` (TriSetup or Strad), at pixel (px, py)
template <class Geom, class Sink> __device__ __forceinline__ void emit(const Geom& g, int f, int px, int py, const Sink& s) {
    float d;
    if (fragment<Sink::NARROW>(g, px, py, d)) s.put(px, py, vis_key(d, f));
}
// a whole wave on one triangle: the lanes stride over the np pixels of a box bw wide from (x0, y0); near-plane straddlers by their own form
template <class Sink> __device__ __forceinline__ void wave_rasterize(const TriSetup& t, const SVert* __restrict__ sv, const int32_t* __restrict__ faces,
                                                                     int f, int x0, int y0, int bw, int np, int lane, const Sink& s) {
    if (t.strad) {   // wave-uniform
        const Strad sq = strad_setup(sv, faces, f);
        for (int j = lane; j < np; j += 64) emit(sq, f, x0 + j % bw, y0 + j / bw, s);
        return;
    }
    for (int j = lane; j < np; j += 64) emit(t, f, x0 + j % bw, y0 + j / bw, s);
}

// ---- shading of the visible fragment (shared by both visibility strategies; arithmetic = the contract in the header) ----
// largest k in [0,255] with thr[k] <= x (thr[0] = 0); the pow() estimate only decides how many table steps are taken
__device__ __forceinline__ uint8_t encode_gamma(float x, const float* thr) {
    if (!(x > 0.f)) return 0;
    int k = (int)(255.0f * __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(fminf(x, 1.0f)) * 0.45454545f) + 0.5f);
    k = min(max(k, 0), 255);
    while (k < 255 && thr[k + 1] <= x) ++k;
    while (k > 0 && thr[k] > x) --k;
    return (uint8_t)k;
}
__device__ __forceinline__ int wrapi(int a, int n) { const int m = a % n; return m < 0 ? m + n : m; }

// bilinear sample of one mip level (values in 0..255 units)
__device__ __forceinline__ void bilinear_level(const uint8_t* __restrict__ lev, int w, int h, float U, float Vv, float (&out)[3]) {
    float x = fmaf(U, (float)w, -0.5f), y = fmaf(1.0f - Vv, (float)h, -0.5f);
    x = fminf(fmaxf(x, -1.0e6f), 1.0e6f); y = fminf(fmaxf(y, -1.0e6f), 1.0e6f);
    if (!(x == x)) x = 0.f;
    if (!(y == y)) y = 0.f;
    const float xf = floorf(x), yf = floorf(y);
    const float wx = x - xf, wy = y - yf;
    const int x0 = wrapi((int)xf, w), x1 = wrapi((int)xf + 1, w);
    const int y0 = wrapi((int)yf, h), y1 = wrapi((int)yf + 1, h);
    const uint32_t e00 = *(const uint32_t*)(lev + ((size_t)y0 * w + x0) * 4), e01 = *(const uint32_t*)(lev + ((size_t)y0 * w + x1) * 4);
    const uint32_t e10 = *(const uint32_t*)(lev + ((size_t)y1 * w + x0) * 4), e11 = *(const uint32_t*)(lev + ((size_t)y1 * w + x1) * 4);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float t00 = (float)((e00 >> (8 * c)) & 255), t01 = (float)((e01 >> (8 * c)) & 255);
        const float t10 = (float)((e10 >> (8 * c)) & 255), t11 = (float)((e11 >> (8 * c)) & 255);
        const float top = fmaf(wx, t01 - t00, t00), bot = fmaf(wx, t11 - t10, t10);
        out[c] = fmaf(wy, bot - top, top);
    }
}
// LOG2P(t) ~ log2(1 + t) on [0,1)
__device__ __forceinline__ float log2p(float t) {
    float a = 0.045148879289627075f;
    a = fmaf(a, t, -0.19357527792453766f);
    a = fmaf(a, t, 0.41560569405555725f);
    a = fmaf(a, t, -0.7090963125228882f);
    a = fmaf(a, t, 1.441917061805725f);
    return a * t;
}

// tab: DEC[256] then THR[256] (LDS copy)
// per-triangle shading attributes, loaded by the caller (so a batch of pixels can have all its gathers in flight at once):
// vertex colours as rgba words of the triangle's ORIGINAL corners (face order) or the six per-corner uv floats
struct TriAttr { uint32_t cw[3]; float tc[6]; };
__device__ __forceinline__ TriAttr load_attr(const ShadeArgs& s, int f, int v0, int v1, int v2) {
    TriAttr a;
    a.cw[0] = a.cw[1] = a.cw[2] = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < 6; ++k) a.tc[k] = 0.f;
    if (s.uv) {
        const float2* tc = (const float2*)(s.uv + (size_t)f * 6);
        const float2 t0 = tc[0], t1 = tc[1], t2 = tc[2];
        a.tc[0] = t0.x; a.tc[1] = t0.y; a.tc[2] = t1.x; a.tc[3] = t1.y; a.tc[4] = t2.x; a.tc[5] = t2.y;
    } else if (s.colors) {
        const uint32_t* cw = (const uint32_t*)s.colors;
        a.cw[0] = cw[v0]; a.cw[1] = cw[v1]; a.cw[2] = cw[v2];
    }
    return a;
}

// `at`: attributes in FACE order (corner k of faces[3f + k]); t.swapped says whether set-up exchanged corners 1 and 2
__device__ __forceinline__ void shade_fragment(const ShadeArgs& s, const TriSetup& t, const TriAttr& at, float q0, float q1, float q2,
                                               float dd, const float* tab, uint8_t (&out)[3], bool lod0 = false) {
    const float* dec = tab;
    const float* thr = tab + 256;
    if (s.uv) {
        const float* tc = at.tc;
        const int k1 = t.swapped ? 2 : 1, k2 = t.swapped ? 1 : 2;
        const float u0 = tc[0], u1 = tc[2 * k1], u2 = tc[2 * k2];
        const float v0 = tc[1], v1 = tc[2 * k1 + 1], v2 = tc[2 * k2 + 1];
        const float U = fmaf(q2, u2, fmaf(q1, u1, q0 * u0)) * dd;
        const float Vv = fmaf(q2, v2, fmaf(q1, v1, q0 * v0)) * dd;
        int l0 = 0;
        bool two = false;
        float fr = 0.f;
        if (s.filter && s.nlev > 1 && !lod0) {
            const float fa = (float)t.area2;
            // d(w_i)/d(px) = -256 (y_b - y_a), d(w_i)/d(py) = 256 (x_b - x_a) of the edge opposite corner i
            const float gx0 = (float)(-(long long)(t.y2 - t.y1) * 256) / fa * t.iz0, gy0 = (float)((long long)(t.x2 - t.x1) * 256) / fa * t.iz0;
            const float gx1 = (float)(-(long long)(t.y0 - t.y2) * 256) / fa * t.iz1, gy1 = (float)((long long)(t.x0 - t.x2) * 256) / fa * t.iz1;
            const float gx2 = (float)(-(long long)(t.y1 - t.y0) * 256) / fa * t.iz2, gy2 = (float)((long long)(t.x1 - t.x0) * 256) / fa * t.iz2;
            const float dux = fmaf(gx2, u2 - U, fmaf(gx1, u1 - U, gx0 * (u0 - U))) * dd * (float)s.tw;
            const float dvx = fmaf(gx2, v2 - Vv, fmaf(gx1, v1 - Vv, gx0 * (v0 - Vv))) * dd * (float)s.th;
            const float duy = fmaf(gy2, u2 - U, fmaf(gy1, u1 - U, gy0 * (u0 - U))) * dd * (float)s.tw;
            const float dvy = fmaf(gy2, v2 - Vv, fmaf(gy1, v1 - Vv, gy0 * (v0 - Vv))) * dd * (float)s.th;
            float r2 = fmaxf(fmaf(dux, dux, dvx * dvx), fmaf(duy, duy, dvy * dvy));
            if (!(r2 == r2)) r2 = 0.f;
            if (r2 > 1.0f) {
                const uint32_t rb = __float_as_uint(r2);
                const int e = (int)(rb >> 23) - 127;
                const float m = __uint_as_float((rb & 0x7fffffu) | 0x3f800000u);
                const float lg = log2p(m - 1.0f);
                l0 = e >> 1;
                fr = 0.5f * ((float)(e & 1) + lg);
                if (l0 >= s.nlev - 1) { l0 = s.nlev - 1; fr = 0.f; } else two = true;
            }
        }
        float val[3];
        bilinear_level(s.tex + (size_t)s.lev_off[l0] * 4, max(1, s.tw >> l0), max(1, s.th >> l0), U, Vv, val);
        if (two) {
            float hi[3];
            bilinear_level(s.tex + (size_t)s.lev_off[l0 + 1] * 4, max(1, s.tw >> (l0 + 1)), max(1, s.th >> (l0 + 1)), U, Vv, hi);
#pragma unroll
            for (int c = 0; c < 3; ++c) val[c] = fmaf(fr, hi[c] - val[c], val[c]);
        }
        const float kd[3] = {s.kd0, s.kd1, s.kd2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (s.shade) {
                const int ii = min(max((int)val[c], 0), 254);
                const float lin = fmaf(val[c] - (float)ii, dec[ii + 1] - dec[ii], dec[ii]);
                out[c] = encode_gamma(s.ambient * (lin * kd[c]), thr);
            } else {
                out[c] = (uint8_t)fmaxf(fminf(s.ambient * (val[c] * kd[c]) + 0.5f, 255.0f), 0.f);
            }
        }
    } else {
        const uint32_t w0 = at.cw[0], w1 = at.cw[t.swapped ? 2 : 1], w2 = at.cw[t.swapped ? 1 : 2];   // (white = 255 when the mesh has no colours)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float c0 = (float)((w0 >> (8 * c)) & 255u), c1 = (float)((w1 >> (8 * c)) & 255u), c2 = (float)((w2 >> (8 * c)) & 255u);
            const float cv = fmaf(q2, c2, fmaf(q1, c1, q0 * c0)) * dd;
            if (s.shade) out[c] = encode_gamma(s.ambient * (cv * (1.0f / 255.f)), thr);
            else out[c] = (uint8_t)fmaxf(fminf(s.ambient * cv + 0.5f, 255.0f), 0.f);
        }
    }
}

// resolve one pixel whose visibility key is `key`: depth and colour of the winning triangle.  `t` / `at`: the winner's set-up and
// attributes (loaded by the caller; ignored for a background pixel)
template <bool NARROW> __device__ __forceinline__ void resolve_pixel_v(const SVert* __restrict__ sv, const int32_t* __restrict__ faces, const ShadeArgs& s,
                                                const float* tab, unsigned long long key, const TriSetup& t, const TriAttr& at, int px,
                                                int py, float& d, uint8_t (&out)[3]) {
    d = 0.f;
    out[0] = out[1] = out[2] = 0;
    if (key == KEY_NONE) return;
    d = key_depth(key);
    float b0, b1, b2;
    if (t.strad) {   // near-plane straddler: true (3-D) barycentrics, level-0 texture
        const Strad q = strad_setup(sv, faces, key_face(key));
        float ds;
        strad_pixel(q, px, py, ds, b0, b1, b2);
        shade_fragment(s, t, at, b0, b1, b2, 1.0f, tab, out, true);
        return;
    }
    // the winner's weights again (three IEEE quotients: per PIXEL that is cheaper than the fp64 reciprocal the raster pass amortises
    // over a triangle); its depth is the key's — the same bits the raster pass computed from the same weights
    if (t.small) { int w0, w1, w2; cover_at<NARROW, int>(t, px, py, w0, w1, w2); bary3(t, w0, w1, w2, b0, b1, b2); }
    else { long long w0, w1, w2; cover_at<NARROW, long long>(t, px, py, w0, w1, w2); bary3(t, w0, w1, w2, b0, b1, b2); }
    shade_fragment(s, t, at, b0 * t.iz0, b1 * t.iz1, b2 * t.iz2, d, tab, out);
}
__device__ __forceinline__ void resolve_pixel(const SVert* __restrict__ sv, const int32_t* __restrict__ faces, const ShadeArgs& s,
                                              const float* tab, unsigned long long key, int px, int py, int W, int Hh, float& d, uint8_t (&out)[3]) {
    if (key == KEY_NONE) { d = 0.f; out[0] = out[1] = out[2] = 0; return; }
    const int f = key_face(key);
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    const TriAttr at = load_attr(s, f, i0, i1, i2);
    const TriSetup t = tri_setup_v(sv[i0], sv[i1], sv[i2], W, Hh);
    resolve_pixel_v<GlobalSink::NARROW>(sv, faces, s, tab, key, t, at, px, py, d, out);
}

__global__ __launch_bounds__(256) void raster_tri_kernel(const SVert* __restrict__ sv_all, const int32_t* __restrict__ faces,
                                                         const int32_t* __restrict__ perm, int V, int F, int W, int Hh, unsigned long long* __restrict__ zb_all,
                                                         int* __restrict__ queue, int* __restrict__ qcount, int qcap, int cull) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    const int h = blockIdx.y;
    if (slot >= F) return;
    const int f = perm[slot];     // Morton order of the centroids: a wave's 64 triangles (and their atomics) are neighbours on the screen whatever the file's face order
    const SVert* sv = sv_all + (size_t)h * V;
    const GlobalSink zb{zb_all + (size_t)h * W * Hh, W};
    const TriSetup t = tri_setup(sv, faces, f, W, Hh);
    if (!t.ok) return;
    if (cull && back_facing(t, sv, faces, f)) return;
    const int area = (t.bx1 - t.bx0 + 1) * (t.by1 - t.by0 + 1);
    if (area > BIG_AREA || t.strad) {
        const int slot = atomicAdd(qcount, 1);
        if (slot < qcap) { queue[2 * slot] = h; queue[2 * slot + 1] = f; return; }
        // queue full: fall through and rasterise here (slow but correct)
    }
    if (t.strad) {
        const Strad q = strad_setup(sv, faces, f);
        for (int py = 0; py < Hh; ++py)
            for (int px = 0; px < W; ++px) emit(q, f, px, py, zb);
        return;
    }
    for (int py = t.by0; py <= t.by1; ++py)
        for (int px = t.bx0; px <= t.bx1; ++px) emit(t, f, px, py, zb);
}

// one wave per queued (view, triangle): lanes stride over the bbox pixels
__global__ __launch_bounds__(256) void raster_big_kernel(const SVert* __restrict__ sv_all, const int32_t* __restrict__ faces,
                                                         int V, int W, int Hh, unsigned long long* __restrict__ zb_all,
                                                         const int* __restrict__ queue, const int* __restrict__ qcount, int qcap) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int nwave = (gridDim.x * blockDim.x) >> 6;
    const int n = min(*qcount, qcap);
    for (int q = wave; q < n; q += nwave) {
        const int h = queue[2 * q], f = queue[2 * q + 1];
        const TriSetup t = tri_setup(sv_all + (size_t)h * V, faces, f, W, Hh);
        const int bw = t.bx1 - t.bx0 + 1, bh = t.by1 - t.by0 + 1;   // (a straddler's box is the frame)
        wave_rasterize(t, sv_all + (size_t)h * V, faces, f, t.bx0, t.by0, bw, bw * bh, lane, GlobalSink{zb_all + (size_t)h * W * Hh, W});
    }
}

__global__ __launch_bounds__(256) void raster_resolve_kernel(const SVert* __restrict__ sv_all, const int32_t* __restrict__ faces, ShadeArgs sh,
                                                             const float* __restrict__ tables, int V, int W, int Hh, const unsigned long long* __restrict__ zb_all,
                                                             uint8_t* __restrict__ rgb, float* __restrict__ depth) {
    __shared__ float tab[512];
    tab[threadIdx.x] = tables[threadIdx.x];
    tab[threadIdx.x + 256] = tables[threadIdx.x + 256];
    __syncthreads();
    const int h = blockIdx.y;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= W * Hh) return;
    const unsigned long long key = zb_all[(size_t)h * W * Hh + pix];
    const int py = pix / W, px = pix - py * W;
    float d;
    uint8_t out[3];
    resolve_pixel(sv_all + (size_t)h * V, faces, sh, tab, key, px, py, W, Hh, d, out);
    depth[(size_t)h * W * Hh + pix] = d;
    uint8_t* o = rgb + ((size_t)h * W * Hh + pix) * 3;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

// ---------------------------------------------------------------------------------------------------------------------
// Tiled path (images up to 704 px, any triangle count): the visibility keys of one screen tile live in LDS, so there is no global
// visibility buffer (no 8 B/pixel clear, no L2 atomics, no resolve read) — LDS triangle binning + per-wave depth test.
//   upload      : the triangles are put in Morton order of their object-space centroids once per mesh (`perm`: slot -> face id), so
//                 64 consecutive slots are neighbours on the surface and, under any pose, on the screen.  The visibility key still
//                 carries the ORIGINAL face id: results do not depend on the order.
//   bin kernel  : one wave per chunk of 64 slots.  Per (view, slot) the tile range of the triangle's clipped pixel bbox as four
//                 nibbles (16 bit), and per chunk the OR of its triangles' tile masks (64 bit, tiles <= 8 x 8) by a wave reduction.
//   tile kernel : one workgroup per (view, tile), all tiles of a view on one XCD (its screen-space vertices stay in that L2).
//                 The chunk masks are read 2048 at a time (coalesced) and the chunks that touch the tile compacted into an LDS hit
//                 list; each WAVE then takes hit chunks on its own (one triangle per lane, the next chunks' reads in flight): the
//                 candidate pixels of the chunk's triangles are flattened over the wave's lanes and depth-tested into LDS with
//                 ds_min_u64 — 32-bit edge functions for triangles below 128 px (all of a dense mesh's), a whole-wave loop for the
//                 rest and for near-plane straddlers.  A tile no chunk touches is written as background at once.  Otherwise the tile's pixels are
//                 resolved (same colour / depth arithmetic as the global path), packed into their own LDS slot, and flushed row by
//                 row as whole dwords.  The epilogue also reduces what fp_depth_extents would compute from the depth image
//                 (count, pixel bbox, fp64 cloud extents: min / max / integer sums, order-independent, hence bit-identical) to one
//                 partial record per tile; raster_extents_kernel folds the <= 64 records of a view.  The depth image itself is
//                 optional: the pose hot path needs only the extents (pose_estimator.py:104-112) and the crops.
// Same tri_setup_v / EdgeFn / barycentrics, same candidate pixel set (bbox ∩ tile over all tiles = bbox), same 64-bit key and
// an order-independent minimum: the output is bit-identical to the global-buffer path and to the oracle.
static_assert(BIN_WAVES * 64 == 256 && TILE_THREADS == 256 && HITS_ROUND % TILE_THREADS == 0 && HITS_ROUND <= 65536 && BIG_TILE_AREA <= 32 &&
                  BIN_CHUNK == 64 && 2 * TILE_MAX <= TILE_THREADS && TILES_SIDE == 8 && tile_lds(TILE_MAX) <= (size_t)LDS_BUDGET,
              "raster_plan.h describes other kernels");
constexpr uint16_t TBOX_NONE = 0x000f;   // tx0 = 15 > tx1 = 0: overlaps nothing
constexpr int PART_N = 10;               // doubles per (view, tile) extents record

__global__ __launch_bounds__(256) void raster_bin_kernel(
    const SVert* __restrict__ sv_all, const int32_t* __restrict__ faces, const int32_t* __restrict__ perm, const int32_t* __restrict__ fsort, int V, int F,
    int W, int Hh, int T, int Hn, int nchunk, uint16_t* __restrict__ tbox, unsigned long long* __restrict__ cmask, int cull) {
    int item, h;
    view_major(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, Hn, item, h);   // all items of a view on one XCD (raster_plan.h)
    const int lane = threadIdx.x & 63;
    const int chunk = item * 4 + (threadIdx.x >> 6);
    if (chunk >= nchunk) return;                         // wave-uniform
    const int slot = chunk * BIN_CHUNK + lane;
    uint16_t box = TBOX_NONE;
    unsigned long long m = 0ull;
    if (slot < F) {
        const SVert* sv = sv_all + (size_t)h * V;
        const int i0 = fsort[3 * slot], i1 = fsort[3 * slot + 1], i2 = fsort[3 * slot + 2];   // the slot's corners, read in slot order
        const TriSetup t = tri_setup_v(sv[i0], sv[i1], sv[i2], W, Hh);
        if (t.ok && !(cull && back_facing(t, sv, faces, perm[slot]))) {
            const int tx0 = t.bx0 / T, ty0 = t.by0 / T, tx1 = t.bx1 / T, ty1 = t.by1 / T;
            box = (uint16_t)(tx0 | (ty0 << 4) | (tx1 << 8) | (ty1 << 12));
            const unsigned long long row = ((1ull << (tx1 - tx0 + 1)) - 1ull) << tx0;    // <= 8 tiles per row
            for (int ty = ty0; ty <= ty1; ++ty) m |= row << (ty * 8);
        }
    }
    tbox[((size_t)h * nchunk + chunk) * BIN_CHUNK + lane] = box;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m |= __shfl_xor(m, off, 64);   // the chunk's mask: OR over the wave
    if (lane == 0) cmask[(size_t)h * nchunk + chunk] = m;
}

// what fp_depth_extents would compute from a depth image: mask count, pixel box, fp64 cloud extremes.  Every fold is a sum, a minimum or
// a maximum: order-independent, hence bit-identical however the pixels are spread over threads, waves and tiles
struct ExtAcc {
    int cnt = 0, xmin = 1 << 30, ymin = 1 << 30, xmax = -1, ymax = -1;
    double Xmin = 1e300, Xmax = -1e300, Ymin = 1e300, Ymax = -1e300;
    // pixel (px, py) of non-zero depth d, at (X, Y) in the camera frame: every non-zero depth joins the cloud, every positive one the mask
    __device__ __forceinline__ void add(int px, int py, double X, double Y, float d) {
        Xmin = fmin(Xmin, X); Xmax = fmax(Xmax, X); Ymin = fmin(Ymin, Y); Ymax = fmax(Ymax, Y);
        if (d > 0.f) { ++cnt; xmin = min(xmin, px); xmax = max(xmax, px); ymin = min(ymin, py); ymax = max(ymax, py); }
    }
    __device__ __forceinline__ void merge(const ExtAcc& o) {
        cnt += o.cnt;
        xmin = min(xmin, o.xmin); ymin = min(ymin, o.ymin); xmax = max(xmax, o.xmax); ymax = max(ymax, o.ymax);
        Xmin = fmin(Xmin, o.Xmin); Xmax = fmax(Xmax, o.Xmax); Ymin = fmin(Ymin, o.Ymin); Ymax = fmax(Ymax, o.Ymax);
    }
    __device__ __forceinline__ void wave_reduce() {   // butterfly: every lane ends with the wave's fold
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            ExtAcc o;
            o.cnt = __shfl_xor(cnt, off, 64);
            o.xmin = __shfl_xor(xmin, off, 64); o.ymin = __shfl_xor(ymin, off, 64); o.xmax = __shfl_xor(xmax, off, 64); o.ymax = __shfl_xor(ymax, off, 64);
            o.Xmin = __shfl_xor(Xmin, off, 64); o.Xmax = __shfl_xor(Xmax, off, 64); o.Ymin = __shfl_xor(Ymin, off, 64); o.Ymax = __shfl_xor(Ymax, off, 64);
            merge(o);
        }
    }
    // as a record: five integers (doubles in a (view, tile) record of `part`, ints in the tile kernel's LDS) and four doubles
    template <class I> __device__ __forceinline__ void store(I* i5, double* d4) const {
        i5[0] = (I)cnt; i5[1] = (I)xmin; i5[2] = (I)ymin; i5[3] = (I)xmax; i5[4] = (I)ymax;
        d4[0] = Xmin; d4[1] = Xmax; d4[2] = Ymin; d4[3] = Ymax;
    }
    template <class I> __device__ __forceinline__ static ExtAcc load(const I* i5, const double* d4) {
        ExtAcc e;
        e.cnt = (int)i5[0]; e.xmin = (int)i5[1]; e.ymin = (int)i5[2]; e.xmax = (int)i5[3]; e.ymax = (int)i5[4];
        e.Xmin = d4[0]; e.Xmax = d4[1]; e.Ymin = d4[2]; e.Ymax = d4[3];
        return e;
    }
};

// the set-up a lane holds, handed to the whole wave (lane `src` is wave-uniform: v_readlane, no memory round trip)
__device__ __forceinline__ int rl_i(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ float rl_f(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
__device__ __forceinline__ TriSetup bcast_setup(const TriSetup& t, int src) {
    TriSetup r;
    r.x0 = rl_i(t.x0, src); r.y0 = rl_i(t.y0, src); r.x1 = rl_i(t.x1, src); r.y1 = rl_i(t.y1, src); r.x2 = rl_i(t.x2, src); r.y2 = rl_i(t.y2, src);
    r.iz0 = rl_f(t.iz0, src); r.iz1 = rl_f(t.iz1, src); r.iz2 = rl_f(t.iz2, src);
    const unsigned lo = (unsigned)rl_i((int)(unsigned)(unsigned long long)t.area2, src), hi = (unsigned)rl_i((int)(unsigned)((unsigned long long)t.area2 >> 32), src);
    r.area2 = (long long)(((unsigned long long)hi << 32) | lo);
    r.bx0 = rl_i(t.bx0, src); r.by0 = rl_i(t.by0, src); r.bx1 = rl_i(t.bx1, src); r.by1 = rl_i(t.by1, src);
    const int flags = rl_i((t.ok ? 1 : 0) | (t.swapped ? 2 : 0) | (t.strad ? 4 : 0) | (t.small ? 8 : 0), src);
    r.ok = flags & 1; r.swapped = flags & 2; r.strad = flags & 4; r.small = flags & 8;
    return r;   // (word by word through memcpy was tried: +4 scalar instructions in the tile kernel, one above the parent)
}

// A lane's own (small) triangle against its <= 32 candidate pixels in the tile, in two passes: coverage of every candidate first (a few
// integer operations each) into a bit mask, then depth + LDS minimum for the covered ones only.  The wave waits for its slowest lane in
// both loops, so the expensive part now runs max-over-lanes(COVERED pixels) times (~1-4 for the ~1.4-pixel triangles of an 82 k mesh)
// instead of max-over-lanes(candidates) (~12): the chunk loop was 2/3 of the kernel on that mesh.
__device__ __forceinline__ void tile_tri_small(const TriSetup& t, int f, int x0, int y0, int x1, int y1, const TileCtx& sink) {
    const EdgeFn e(t);
    const int bw = x1 - x0 + 1;
    unsigned mask = 0u;
    int k = 0;
    for (int py = y0; py <= y1; ++py) {
        const int sy = pixel_centre<int>(py);
        for (int px = x0; px <= x1; ++px, ++k) {
            int w0, w1, w2;
            e.weights(pixel_centre<int>(px), sy, w0, w1, w2);
            mask |= (e.accept(w0, w1, w2) ? 1u : 0u) << k;
        }
    }
    if (!mask) return;
    const double rd = area_rcp(t);
    const float rbw = split_rcp(bw);
    while (mask) {
        const int kk = __ffs((int)mask) - 1;
        mask &= mask - 1u;
        int ry, rx, w0, w1, w2;
        split_rowcol(kk, bw, rbw, ry, rx);
        const int px = x0 + rx, py = y0 + ry;
        e.weights(pixel_centre<int>(px), pixel_centre<int>(py), w0, w1, w2);
        const float d = depth_from_bary(t, bary_rcp(w0, rd), bary_rcp(w1, rd), bary_rcp(w2, rd));
        if (d > 0.f) sink.put(px, py, vis_key(d, f));
    }
}

// ---- the lab build's hooks of the tile kernel, all behind this fence (tools/raster_ablate.py, tools/lab_selfcheck.py).  raster_dbg bits 1 / 2 / 4 / 8
// switch a stage OFF (no rasterisation / no shading / no flush / no mask scan: wrong pictures, timing only), bits 8.. = the per-lane / whole-wave threshold
// (0 = the product's); buf = shader-clock sums of all workgroups: 0 init, 1 mask scan, 2 chunk loop (slowest wave), 3 resolve, 4 flush, 6 wave 0's chunk loop, 7 hit chunks
#ifdef FP_LAB
constexpr bool LAB = true;
#else
constexpr bool LAB = false;    // every hook below folds away: bits = 0, the product's threshold, no buffer, no clock read
#endif
struct Lab {
    int bits, big_area;
    unsigned long long *buf, tstamp;
    __device__ __forceinline__ Lab(int arg, unsigned long long* b)
        : bits(LAB ? arg & 255 : 0), big_area(LAB && (arg >> 8) ? min(arg >> 8, 32) : BIG_TILE_AREA),   // (the per-lane coverage mask has 32 bits)
          buf(LAB ? b : nullptr), tstamp(LAB ? __builtin_readcyclecounter() : 0ull) {}
    __device__ __forceinline__ bool off(int bit) const { return bits & bit; }
    __device__ __forceinline__ void phase(int k) {
        if (!LAB || !buf || threadIdx.x != 0) return;
        const unsigned long long now = __builtin_readcyclecounter();
        atomicAdd(&buf[k], now - tstamp);
        tstamp = now;
    }
    __device__ __forceinline__ void chunk_stats(int n) const {
        if (!LAB || !buf || threadIdx.x != 0) return;
        atomicAdd(&buf[6], (unsigned long long)(__builtin_readcyclecounter() - tstamp));
        atomicAdd(&buf[7], (unsigned long long)n);
    }
};

// ---- the tile kernel's stages (TileCtx above)
__device__ __forceinline__ void tile_init(const TileCtx& c, const float* __restrict__ tables, double fx, double fy, double cx, double cy,
                                          int& nhit_s, int& total_s) {
    const int T = c.T;
    c.tab[threadIdx.x] = tables[threadIdx.x];
    c.tab[threadIdx.x + 256] = tables[threadIdx.x + 256];
    if (threadIdx.x < T) c.ax[threadIdx.x] = ((double)(c.X0 + (int)threadIdx.x) - cx) / fx;
    else if ((int)threadIdx.x < 2 * T) c.ay[threadIdx.x - T] = ((double)(c.Y0 + (int)threadIdx.x - T) - cy) / fy;
    for (int p = threadIdx.x; p < T * T; p += blockDim.x) c.tile[p] = KEY_NONE;
    if (threadIdx.x == 0) { nhit_s = 0; total_s = 0; }
    __syncthreads();
}

// which of the round's HITS_ROUND chunks (from `base`) touch this tile: coalesced mask reads, wave-compacted into the hit list
__device__ __forceinline__ void scan_hits(const TileCtx& c, const unsigned long long* __restrict__ cm, int base, int nchunk, int& nhit_s) {
    const int tbit = c.ty * 8 + c.tx;
    unsigned long long mk[HITS_ROUND / 256];
#pragma unroll
    for (int k = 0; k < HITS_ROUND / 256; ++k) {                      // the round's mask loads in flight together
        const int ch = base + k * 256 + (int)threadIdx.x;
        mk[k] = ch < nchunk ? cm[ch] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < HITS_ROUND / 256; ++k) {
        const int ch = base + k * 256 + (int)threadIdx.x;
        const bool hit = (mk[k] >> tbit) & 1ull;
        const unsigned long long bm = __ballot(hit);
        if (bm) {                                                     // wave-uniform
            int wbase = 0;
            if (c.lane == 0) wbase = atomicAdd(&nhit_s, __popcll(bm));
            wbase = __shfl(wbase, 0, 64);
            if (hit) c.hits[wbase + __popcll(bm & ((1ull << c.lane) - 1ull))] = (unsigned short)(ch - base);
        }
    }
    __syncthreads();
}

// what a lane needs of its triangle in a hit chunk: level 1 = coalesced reads in slot order (tile box, corner ids, face id),
// level 2 = the gathered screen-space vertices.  The chunk loop keeps the level-1 reads of chunk i+2 and the gathers of chunk i+1 in
// flight while chunk i is rasterised (a wave otherwise walks its ~30 chunks of an 82 k-triangle mesh one memory round trip at a time).
struct ChunkL1 { unsigned box; int i0, i1, i2, f; };
struct ChunkL2 { SVert a, b, c; };

// Every wave takes hit chunks (the first n of the hit list) on its own, one triangle per lane; above big_area candidate pixels: the whole wave
__device__ __forceinline__ void chunk_loop(const TileCtx& c, int n, int base, const uint16_t* __restrict__ tb, const int32_t* __restrict__ fsort,
                                           const int32_t* __restrict__ perm, int F, int big_area) {
    const int lane = c.lane, tx = c.tx, ty = c.ty, X0 = c.X0, Y0 = c.Y0, X1 = c.X1, Y1 = c.Y1, W = c.W, Hh = c.Hh;
    const SVert* sv = c.sv;
    auto level1 = [&](int i, ChunkL1& l) {
        l.box = TBOX_NONE; l.i0 = l.i1 = l.i2 = 0; l.f = 0;
        if (i < n) {
            const int slot = (base + (int)c.hits[i]) * BIN_CHUNK + lane;
            l.box = tb[slot];                                        // (TBOX_NONE for slots >= F)
            if (slot < F) { l.i0 = fsort[3 * slot]; l.i1 = fsort[3 * slot + 1]; l.i2 = fsort[3 * slot + 2]; l.f = perm[slot]; }
        }
    };
    auto overlaps = [&](unsigned box) {
        const int bx0 = box & 15, by0 = (box >> 4) & 15, bx1 = (box >> 8) & 15, by1 = (box >> 12) & 15;
        return bx0 <= tx && tx <= bx1 && by0 <= ty && ty <= by1;
    };
    auto level2 = [&](const ChunkL1& l, ChunkL2& g) {   // (lanes whose triangle misses the tile read vertex 0: one cached line, no branch, no zero fill)
        const bool o = overlaps(l.box);
        g.a = sv[o ? l.i0 : 0]; g.b = sv[o ? l.i1 : 0]; g.c = sv[o ? l.i2 : 0];
    };
    ChunkL1 c0, c1, c2;
    ChunkL2 g0, g1;
    level1(c.wave, c0);
    level1(c.wave + 4, c1);
    level2(c0, g0);
    for (int i = c.wave; i < n; i += 4) {
        level1(i + 8, c2);
        level2(c1, g1);
        // set-up on every lane (a wave executes it once whatever the number of live lanes; a branch only added register traffic)
        const int f = c0.f;
        const TriSetup t = tri_setup_v(g0.a, g0.b, g0.c, W, Hh);
        const int x0 = max(t.bx0, X0), y0 = max(t.by0, Y0), x1 = min(t.bx1, X1), y1 = min(t.by1, Y1);
        const bool mine = overlaps(c0.box) && t.ok && x0 <= x1 && y0 <= y1;
        // the wave loop: many candidate pixels, edge functions beyond 32 bits, near-plane straddlers
        const bool big = mine && ((x1 - x0 + 1) * (y1 - y0 + 1) > big_area || !t.small || t.strad);
        if (mine && !big) tile_tri_small(t, f, x0, y0, x1, y1, c);
        // triangles with many candidate pixels in this tile, and near-plane straddlers: the whole wave strides over them, one triangle
        // at a time, the owner lane's set-up broadcast by v_readlane.  (Round 6 also measured the candidates of a chunk FLATTENED over
        // the lanes — counts prefix-summed, owner found by binary search, set-up fetched by ds_bpermute: 14 permutes per item cost what
        // the idle lanes did; 2.32 / 3.03 / 6.29 ms against 1.70 / 3.13 / 5.26 at 1 280 / 81 920 / 327 680 triangles.  Not shipped.)
        unsigned long long bm = __ballot(big);
        while (bm) {
            const int src = __ffsll((long long)bm) - 1;
            bm &= bm - 1;
            const int fb = rl_i(f, src);
            const TriSetup tbg = bcast_setup(t, src);          // (was a second set-up from memory: two dependent gathers per triangle)
            const int ax0 = max(tbg.bx0, X0), ay0 = max(tbg.by0, Y0), ax1 = min(tbg.bx1, X1), ay1 = min(tbg.by1, Y1);
            wave_rasterize(tbg, sv, c.faces, fb, ax0, ay0, ax1 - ax0 + 1, (ax1 - ax0 + 1) * (ay1 - ay0 + 1), lane, c);
        }
        c0 = c1; c1 = c2; g0 = g1;
    }
}

constexpr int RES_BATCH = 2;             // pixels a thread resolves together (their gathers are issued back to back)

// resolve: same arithmetic as raster_resolve_kernel; the result replaces the pixel's key in its own LDS slot, and joins the thread's extents `e`.
// RES_BATCH pixels per thread at a time: keys -> corner ids -> vertices + attributes, each level's loads issued for the whole batch before the first is used
// (a pixel at a time, the three dependent gathers bound the whole kernel: 2 ms per 576 views).  A tile no chunk touched is background.  shade: false in the lab only
__device__ __forceinline__ void resolve_tile(const TileCtx& c, bool touched, const ShadeArgs& sh, bool shade, ExtAcc& e) {
    const int T = c.T, tw = c.tw(), th = c.th(), W = c.W, Hh = c.Hh;
    unsigned long long* tile = c.tile;
    if (!touched) {
        for (int p = threadIdx.x; p < T * T; p += blockDim.x) tile[p] = 0ull;
        __syncthreads();
        return;
    }
    for (int pb = threadIdx.x; pb < tw * th; pb += blockDim.x * RES_BATCH) {
        unsigned long long key[RES_BATCH];
        int lxs[RES_BATCH], lys[RES_BATCH], ids[RES_BATCH][3];
        SVert va[RES_BATCH], vb[RES_BATCH], vc[RES_BATCH];
        TriAttr at[RES_BATCH];
#pragma unroll
        for (int k = 0; k < RES_BATCH; ++k) {
            const int p = pb + k * (int)blockDim.x;
            key[k] = KEY_NONE; lxs[k] = lys[k] = 0;
            if (p < tw * th) { lys[k] = p / tw; lxs[k] = p - lys[k] * tw; key[k] = tile[lys[k] * T + lxs[k]]; }
        }
#pragma unroll
        for (int k = 0; k < RES_BATCH; ++k) {
            ids[k][0] = ids[k][1] = ids[k][2] = 0;
            if (key[k] != KEY_NONE) {
                const int f = key_face(key[k]);
                ids[k][0] = c.faces[3 * f]; ids[k][1] = c.faces[3 * f + 1]; ids[k][2] = c.faces[3 * f + 2];
            }
        }
#pragma unroll
        for (int k = 0; k < RES_BATCH; ++k) {
            if (key[k] != KEY_NONE) {
                va[k] = c.sv[ids[k][0]]; vb[k] = c.sv[ids[k][1]]; vc[k] = c.sv[ids[k][2]];
                at[k] = load_attr(sh, key_face(key[k]), ids[k][0], ids[k][1], ids[k][2]);
            } else {
                va[k] = vb[k] = vc[k] = SVert{0, 0, 0.f, 0.f};
                at[k] = TriAttr{};
            }
        }
#pragma unroll
        for (int k = 0; k < RES_BATCH; ++k) {
            const int p = pb + k * (int)blockDim.x;
            if (p >= tw * th) continue;
            const int lx = lxs[k], ly = lys[k], px = c.X0 + lx, py = c.Y0 + ly;
            float d = 0.f;
            uint8_t out[3] = {0, 0, 0};
            if (key[k] != KEY_NONE && shade) {
                const TriSetup t = tri_setup_v(va[k], vb[k], vc[k], W, Hh);
                resolve_pixel_v<TileCtx::NARROW>(c.sv, c.faces, sh, c.tab, key[k], t, at[k], px, py, d, out);
            }
            tile[ly * T + lx] = vis_key(d, 0) | (unsigned)out[0] | ((unsigned)out[1] << 8) | ((unsigned)out[2] << 16);
            if (d != 0.f) e.add(px, py, c.ax[lx] * (double)d, c.ay[ly] * (double)d, d);
        }
    }
    __syncthreads();
}

// ---- flush: depth rows as floats; rgb rows as whole dwords (byte stores only for a row's unaligned ends)
__device__ __forceinline__ void flush_depth(const TileCtx& c, float* __restrict__ depth) {
    const int tw = c.tw(), th = c.th(), W = c.W, Hh = c.Hh;
    for (int p = threadIdx.x; p < tw * th; p += blockDim.x) {
        const int ly = p / tw, lx = p - ly * tw;
        depth[((size_t)c.h * Hh + c.Y0 + ly) * W + c.X0 + lx] = key_depth(c.tile[ly * c.T + lx]);
    }
}
// rows start on a dword (W * 3 and X0 * 3 are multiples of 4) and hold whole groups of four pixels = three dwords: the packed results'
// low words are spliced with shifts, one 12-byte store per lane, adjacent lanes adjacent
__device__ __forceinline__ void flush_rgb_dword(const TileCtx& c, uint8_t* __restrict__ rgb) {
    const int nq = c.tw() >> 2, th = c.th(), W = c.W, Hh = c.Hh;
    for (int q = threadIdx.x; q < th * nq; q += blockDim.x) {
        const int ly = q / nq, qx = q - ly * nq;
        const unsigned long long* src = &c.tile[ly * c.T + 4 * qx];
        const unsigned p0 = (unsigned)src[0], p1 = (unsigned)src[1], p2 = (unsigned)src[2], p3 = (unsigned)src[3];
        uint3 o;
        o.x = (p0 & 0xffffffu) | (p1 << 24);
        o.y = ((p1 >> 8) & 0xffffu) | (p2 << 16);
        o.z = ((p2 >> 16) & 0xffu) | (p3 << 8);
        *(uint3*)(rgb + (((size_t)c.h * Hh + c.Y0 + ly) * W + c.X0 + 4 * qx) * 3) = o;
    }
}
// any width and alignment: one aligned dword per thread, stored whole when all four bytes belong to the tile row, else byte by byte
__device__ __forceinline__ void flush_rgb_bytes(const TileCtx& c, uint8_t* __restrict__ rgb) {
    const int tw = c.tw(), th = c.th(), W = c.W, Hh = c.Hh;
    const int ndw = (tw * 3 + 3) / 4 + 1;                          // dwords that can hold a row's bytes at any alignment
    for (int q = threadIdx.x; q < th * ndw; q += blockDim.x) {
        const int ly = q / ndw, j = q - ly * ndw;
        const size_t start = (((size_t)c.h * Hh + c.Y0 + ly) * W + c.X0) * 3;   // first byte of the tile row in the rgb buffer
        const size_t a = (start & ~(size_t)3) + (size_t)j * 4;            // this thread's aligned dword
        const long long o0 = (long long)a - (long long)start;              // row-relative offset of its first byte
        if (o0 >= (long long)tw * 3) continue;
        unsigned v = 0;
        bool in[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long o = o0 + k;
            in[k] = o >= 0 && o < (long long)tw * 3;
            if (in[k]) {
                const int pix = (int)o / 3, ch = (int)o - pix * 3;
                v |= (unsigned)((c.tile[ly * c.T + pix] >> (8 * ch)) & 255ull) << (8 * k);
            }
        }
        if (in[0] && in[3]) *(uint32_t*)(rgb + a) = v;
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (in[k]) rgb[a + k] = (uint8_t)(v >> (8 * k));
        }
    }
}

// the tile's extents record: the threads' accumulators folded over each wave, then over the four waves through LDS
__device__ __forceinline__ void write_extents_record(const TileCtx& c, ExtAcc e, int (&red_i)[4][5], double (&red_d)[4][4], double* __restrict__ rec) {
    e.wave_reduce();
    if (c.lane == 0) e.store(red_i[c.wave], red_d[c.wave]);
    __syncthreads();
    if (threadIdx.x == 0) {
        ExtAcc all = ExtAcc::load(red_i[0], red_d[0]);
        for (int w = 1; w < 4; ++w) all.merge(ExtAcc::load(red_i[w], red_d[w]));
        all.store(rec, rec + 5);
    }
}

__global__ __launch_bounds__(256) void raster_tile_kernel(
    const SVert* __restrict__ sv_all, const int32_t* __restrict__ faces, const int32_t* __restrict__ perm, const int32_t* __restrict__ fsort, ShadeArgs sh,
    const float* __restrict__ tables, int V, int F, int W, int Hh, int T, int ntx, int Hn, const uint16_t* __restrict__ tbox,
    const unsigned long long* __restrict__ cmask, int nchunk, uint8_t* __restrict__ rgb, float* __restrict__ depth, double* __restrict__ part, double fx,
    double fy, double cx, double cy, int dbg_arg, unsigned long long* dbg_buf) {
    Lab lab(dbg_arg, dbg_buf);
    extern __shared__ unsigned long long tile[];   // [T*T] visibility keys | DEC/THR tables (512 floats) | hit list | column / row factors
    __shared__ int nhit_s, total_s;
    __shared__ double red_d[4][4];                 // the four waves' extents, folded by write_extents_record
    __shared__ int red_i[4][5];
    TileCtx c;
    int tidx;
    view_major(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, Hn, tidx, c.h);   // all tiles of a view on one XCD (raster_plan.h)
    c.ty = tidx / ntx; c.tx = tidx - c.ty * ntx; c.T = T; c.W = W; c.Hh = Hh;
    c.X0 = c.tx * T; c.Y0 = c.ty * T; c.X1 = min(W - 1, c.X0 + T - 1); c.Y1 = min(Hh - 1, c.Y0 + T - 1);
    c.tile = tile; c.tab = (float*)(tile + T * T); c.hits = (unsigned short*)(c.tab + 512);
    c.ax = (double*)(c.hits + HITS_ROUND); c.ay = c.ax + T;
    c.sv = sv_all + (size_t)c.h * V; c.faces = faces; c.lane = threadIdx.x & 63; c.wave = threadIdx.x >> 6;
    tile_init(c, tables, fx, fy, cx, cy, nhit_s, total_s);
    lab.phase(0);
    const unsigned long long* cm = cmask + (size_t)c.h * nchunk;
    const uint16_t* tb = tbox + (size_t)c.h * nchunk * BIN_CHUNK;
    for (int base = 0; base < (lab.off(8) ? 0 : nchunk); base += HITS_ROUND) {
        scan_hits(c, cm, base, nchunk, nhit_s);
        lab.phase(1);
        const int n = lab.off(1) ? 0 : nhit_s;
        chunk_loop(c, n, base, tb, fsort, perm, F, lab.big_area);
        lab.chunk_stats(n);
        __syncthreads();
        lab.phase(2);
        if (threadIdx.x == 0) { total_s += n; nhit_s = 0; }
        __syncthreads();
    }
    ExtAcc e;
    resolve_tile(c, total_s > 0, sh, !lab.off(2), e);
    lab.phase(3);
    if (lab.off(4)) return;
    if (depth) flush_depth(c, depth);
    if (((W * 3) & 3) == 0 && (c.tw() & 3) == 0 && (T & 3) == 0) flush_rgb_dword(c, rgb);
    else flush_rgb_bytes(c, rgb);
    lab.phase(4);
    if (part) write_extents_record(c, e, red_i, red_d, part + ((size_t)c.h * gridDim.x + tidx) * PART_N);
}

// folds the per-tile records of a view into fp_depth_extents' row (and the int32 box CropResizePad takes): same rule for views with
// fewer than 100 mask pixels (renderer.py:116-117, template.py:75-77)
__global__ __launch_bounds__(64) void raster_extents_kernel(const double* __restrict__ part, int Hn, int ntile, int W, int Hh,
                                                            double* __restrict__ ext, int32_t* __restrict__ boxes) {
    const int v = blockIdx.x, lane = threadIdx.x;        // one wave per view, one tile record per lane (<= 64 tiles), butterfly reduction
    ExtAcc e;
    for (int t = lane; t < ntile; t += 64) {
        const double* p = part + ((size_t)v * ntile + t) * PART_N;
        e.merge(ExtAcc::load(p, p + 5));
    }
    e.wave_reduce();
    if (lane != 0) return;
    int c = e.cnt, bx0 = e.xmin, by0 = e.ymin, bx1 = e.xmax, by1 = e.ymax;
    if (c < 100) {
        const int lo = 105, hx = min(315, W) - 1, hy = min(315, Hh) - 1;
        if (c == 0) { bx0 = lo; by0 = lo; bx1 = hx; by1 = hy; }
        else { bx0 = min(bx0, lo); by0 = min(by0, lo); bx1 = max(bx1, hx); by1 = max(by1, hy); }
    }
    if (ext) {
        double* o = ext + (size_t)v * 8;
        o[0] = (double)bx0; o[1] = (double)by0; o[2] = (double)bx1; o[3] = (double)by1;
        o[4] = e.Xmax > -1e299 ? e.Xmax - e.Xmin : 0.0;
        o[5] = e.Ymax > -1e299 ? e.Ymax - e.Ymin : 0.0;
        o[6] = (double)c; o[7] = 0.0;
    }
    if (boxes) { boxes[4 * v] = bx0; boxes[4 * v + 1] = by0; boxes[4 * v + 2] = bx1; boxes[4 * v + 3] = by1; }
}

// int32 boxes of an extents table (global-buffer path of fp_rasterize_extents)
__global__ void ext_boxes_kernel(const double* __restrict__ ext, int Hn, int32_t* __restrict__ boxes) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= Hn) return;
    for (int k = 0; k < 4; ++k) boxes[4 * v + k] = (int)ext[(size_t)v * 8 + k];
}

// vertex stage export (fp_project_vertices)
__global__ void raster_export_kernel(const SVert* __restrict__ sv, const int32_t* __restrict__ vmap, int V, size_t n,
                                     int32_t* __restrict__ xy, float* __restrict__ zc) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // (view, caller's vertex id)
    if (i >= n) return;
    const size_t h = i / (size_t)V;
    const SVert v = sv[h * (size_t)V + (size_t)vmap[i - h * (size_t)V]];
    const bool front = v.zc > ZNEAR;     // behind the near plane the fields hold homogeneous coordinates (straddler path), not pixels
    xy[2 * i] = front ? v.xi : 0; xy[2 * i + 1] = front ? v.yi : 0;
    zc[i] = v.zc;
}

}  // namespace

// device copy of `bytes` bytes of host memory: *dst is allocated here (and freed by fp_mesh_destroy)
template <class T> static int upload(T** dst, const void* src, size_t bytes) {
    void* d = nullptr;
    FP_HIP(hipMalloc(&d, bytes));
    *dst = (T*)d;                  // (owned by the mesh from here on, also when the copy fails)
    FP_HIP(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    return FP_OK;
}

static int mesh_tables(fp_mesh* m) {
    // DEC[i] = sRGB -> linear of i/255 ; THR[k] = ((k - 0.5)/255)^2.2 (THR[0] = 0): double precision, rounded to float once
    float tab[512];
    for (int i = 0; i < 256; ++i) {
        const double sv = (double)i / 255.0;
        tab[i] = (float)(sv <= 0.04045 ? sv / 12.92 : pow((sv + 0.055) / 1.055, 2.4));
        tab[256 + i] = i == 0 ? 0.f : (float)pow(((double)i - 0.5) / 255.0, 2.2);
    }
    return upload(&m->tables, tab, sizeof(tab));
}

extern "C" int fp_mesh_destroy(fp_mesh* m);
// frees a half-built mesh when an upload step fails (FP_HIP / FP_REQUIRE return early); release() on success
struct MeshGuard : std::unique_ptr<fp_mesh, int (*)(fp_mesh*)> { explicit MeshGuard(fp_mesh* m) : unique_ptr(m, fp_mesh_destroy) {} };

// slot -> face id: Morton order of the triangle centroids (10 bits per axis over the vertex bounding box), ties by face id
static std::vector<int32_t> morton_order(const float* h_verts, int V, const int32_t* h_faces, int F) {
    float lo[3] = {h_verts[0], h_verts[1], h_verts[2]}, hi[3] = {h_verts[0], h_verts[1], h_verts[2]};
    for (int i = 0; i < V; ++i)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], h_verts[3 * i + a]); hi[a] = std::max(hi[a], h_verts[3 * i + a]); }
    auto spread = [](uint32_t x) {   // 10 bits -> every third bit
        x &= 0x3ffu; x = (x | (x << 16)) & 0x030000ffu; x = (x | (x << 8)) & 0x0300f00fu; x = (x | (x << 4)) & 0x030c30c3u; x = (x | (x << 2)) & 0x09249249u;
        return x;
    };
    std::vector<std::pair<uint32_t, int32_t>> key((size_t)F);
    for (int f = 0; f < F; ++f) {
        uint32_t code = 0;
        for (int a = 0; a < 3; ++a) {
            const float c = (h_verts[3 * h_faces[3 * f] + a] + h_verts[3 * h_faces[3 * f + 1] + a] + h_verts[3 * h_faces[3 * f + 2] + a]) * (1.0f / 3.0f);
            const float span = hi[a] - lo[a];
            float u = span > 0.f ? (c - lo[a]) / span : 0.f;
            if (!(u >= 0.f)) u = 0.f;                // (NaN vertices land in cell 0; they are dropped by the raster set-up anyway)
            const uint32_t q = (uint32_t)std::min(1023.0f, u * 1024.0f);
            code |= spread(q) << a;
        }
        key[f] = {code, f};
    }
    std::sort(key.begin(), key.end());
    std::vector<int32_t> perm((size_t)F);
    for (int f = 0; f < F; ++f) perm[f] = key[f].second;
    return perm;
}

// caller's vertex id -> device vertex id: order of first use along the sorted triangles, unreferenced vertices last (fp_mesh::vmap says why)
static std::vector<int32_t> first_use_order(const std::vector<int32_t>& perm, int V, const int32_t* h_faces) {
    std::vector<int32_t> vmap((size_t)V, -1);
    int next = 0;
    for (const int32_t f : perm)
        for (int a = 0; a < 3; ++a) { int32_t& id = vmap[h_faces[3 * (size_t)f + a]]; if (id < 0) id = next++; }
    for (int i = 0; i < V; ++i) if (vmap[i] < 0) vmap[i] = next++;
    return vmap;
}

static int mesh_geometry(fp_ctx* ctx, const float* h_verts, int V, const int32_t* h_faces, int F, fp_mesh** out) {
    FP_REQUIRE(ctx && h_verts && h_faces && out && V > 0 && F > 0, "mesh_upload: bad argument");
    for (int i = 0; i < 3 * F; ++i) FP_REQUIRE(h_faces[i] >= 0 && h_faces[i] < V, "mesh_upload: face index out of range");
    fp_mesh* m = new fp_mesh();
    MeshGuard guard(m);
    m->ctx = ctx; m->V = V; m->F = F;
    const std::vector<int32_t> perm = morton_order(h_verts, V, h_faces, F);
    std::vector<int32_t> vmap = first_use_order(perm, V, h_faces);
    std::vector<float> verts((size_t)V * 3);
    for (int i = 0; i < V; ++i)
        for (int a = 0; a < 3; ++a) verts[3 * (size_t)vmap[i] + a] = h_verts[3 * (size_t)i + a];
    std::vector<int32_t> faces((size_t)F * 3), fsort((size_t)F * 3);
    for (size_t i = 0; i < (size_t)F * 3; ++i) faces[i] = vmap[h_faces[i]];
    for (int k = 0; k < F; ++k)
        for (int a = 0; a < 3; ++a) fsort[3 * (size_t)k + a] = faces[3 * (size_t)perm[k] + a];
    int rc;
    if ((rc = upload(&m->verts, verts.data(), (size_t)V * 12)) || (rc = upload(&m->faces, faces.data(), (size_t)F * 12)) ||
        (rc = upload(&m->perm, perm.data(), (size_t)F * 4)) || (rc = upload(&m->fsort, fsort.data(), (size_t)F * 12)) ||
        (rc = upload(&m->vmap, vmap.data(), (size_t)V * 4)) || (rc = mesh_tables(m)))
        return rc;
    m->h_vmap = std::move(vmap);
    *out = guard.release();
    return FP_OK;
}

extern "C" int fp_mesh_upload(fp_ctx* ctx, const float* h_verts, int V, const int32_t* h_faces, int F, const uint8_t* h_colors, fp_mesh** out) {
    fp_mesh* m = nullptr;
    int rc = mesh_geometry(ctx, h_verts, V, h_faces, F, &m);
    if (rc) return rc;
    MeshGuard guard(m);
    if (h_colors) {
        std::vector<uint8_t> rgba((size_t)V * 4, 255);
        for (int i = 0; i < V; ++i) {
            const size_t d = (size_t)m->h_vmap[i];                   // vertex attributes live at the device id
            rgba[4 * d] = h_colors[3 * i]; rgba[4 * d + 1] = h_colors[3 * i + 1]; rgba[4 * d + 2] = h_colors[3 * i + 2];
        }
        if ((rc = upload(&m->sh.colors, rgba.data(), (size_t)V * 4))) return rc;
    }
    *out = guard.release();
    return FP_OK;
}

extern "C" int fp_mesh_upload_textured(fp_ctx* ctx, const float* h_verts, int V, const int32_t* h_faces, int F,
                                       const float* h_uv, const uint8_t* h_texture, int th, int tw, const float* h_kd3, fp_mesh** out) {
    FP_REQUIRE(h_uv && h_texture && th > 0 && tw > 0 && th <= 16384 && tw <= 16384, "mesh_upload_textured: bad texture argument");
    fp_mesh* m = nullptr;
    int rc = mesh_geometry(ctx, h_verts, V, h_faces, F, &m);
    if (rc) return rc;
    MeshGuard guard(m);
    // level 0 + the box-filtered chain down to 1 x 1 (contract in the header), rgba, back to back
    int lw[16], lh[16], n = 0;
    size_t total = 0;
    for (int w = tw, h = th;; w = w > 1 ? w >> 1 : 1, h = h > 1 ? h >> 1 : 1) {
        lw[n] = w; lh[n] = h; m->sh.lev_off[n] = (uint32_t)total; total += (size_t)w * h; ++n;
        if ((w == 1 && h == 1) || n == 16) break;
    }
    m->sh.nlev = n;
    std::vector<uint8_t> rgba(total * 4, 255);
    for (size_t i = 0; i < (size_t)th * tw; ++i) { rgba[4 * i] = h_texture[3 * i]; rgba[4 * i + 1] = h_texture[3 * i + 1]; rgba[4 * i + 2] = h_texture[3 * i + 2]; }
    for (int k = 1; k < n; ++k) {
        const uint8_t* src = rgba.data() + (size_t)m->sh.lev_off[k - 1] * 4;
        uint8_t* dst = rgba.data() + (size_t)m->sh.lev_off[k] * 4;
        const int sw = lw[k - 1], sh = lh[k - 1];
        for (int y = 0; y < lh[k]; ++y)
            for (int x = 0; x < lw[k]; ++x) {
                const int x0 = std::min(2 * x, sw - 1), x1 = std::min(2 * x + 1, sw - 1), y0 = std::min(2 * y, sh - 1), y1 = std::min(2 * y + 1, sh - 1);
                for (int c = 0; c < 3; ++c)
                    dst[((size_t)y * lw[k] + x) * 4 + c] = (uint8_t)((src[((size_t)y0 * sw + x0) * 4 + c] + src[((size_t)y0 * sw + x1) * 4 + c] +
                                                                     src[((size_t)y1 * sw + x0) * 4 + c] + src[((size_t)y1 * sw + x1) * 4 + c] + 2) >> 2);
            }
    }
    if ((rc = upload(&m->sh.tex, rgba.data(), rgba.size())) || (rc = upload(&m->sh.uv, h_uv, (size_t)F * 24))) return rc;
    m->sh.th = th; m->sh.tw = tw;
    if (h_kd3) { m->sh.kd0 = h_kd3[0]; m->sh.kd1 = h_kd3[1]; m->sh.kd2 = h_kd3[2]; }
    *out = guard.release();
    return FP_OK;
}
extern "C" int fp_mesh_destroy(fp_mesh* m) {
    if (!m) return FP_OK;
    for (void* p : {(void*)m->verts, (void*)m->faces, (void*)m->perm, (void*)m->fsort, (void*)m->vmap, (void*)m->sh.colors, (void*)m->sh.uv,
                    (void*)m->sh.tex, (void*)m->tables})
        if (p) (void)hipFree(p);
    delete m;
    return FP_OK;
}

// vertex stage of Hn views into the context's "raster.sv" ([Hn, V] SVert, device vertex ids)
static int project_views(fp_ctx* ctx, const fp_mesh* mesh, const float* d_poses, int Hn, float scale, float fx, float fy, float cx, float cy,
                         hipStream_t s, SVert** sv) {
    const int V = mesh->V;
    int rc;
    if ((rc = ctx->get("raster.sv", (size_t)Hn * V * sizeof(SVert), (void**)sv))) return rc;
    hipLaunchKernelGGL(raster_vertex_kernel, dim3(cdiv(V, 256), Hn), dim3(256), 0, s, mesh->verts, V, d_poses, Hn, scale, fx, fy, cx, cy, *sv);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

extern "C" int fp_project_vertices(fp_ctx* ctx, const fp_mesh* mesh, const float* d_poses, int Hn, float scale, float fx,
                                   float fy, float cx, float cy, int32_t* d_xy, float* d_zc, void* stream) {
    FP_REQUIRE(ctx && mesh && d_poses && d_xy && d_zc, "project_vertices: null argument");
    if (Hn == 0) return FP_OK;
    hipStream_t s = (hipStream_t)stream;
    SVert* sv;
    int rc;
    if ((rc = project_views(ctx, mesh, d_poses, Hn, scale, fx, fy, cx, cy, s, &sv))) return rc;
    const size_t n = (size_t)Hn * mesh->V;
    hipLaunchKernelGGL(raster_export_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, sv, mesh->vmap, mesh->V, n, d_xy, d_zc);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

// d_depth, d_ext, d_boxes: each may be null (at least rgb is always written)
static int rasterize_impl(fp_ctx* ctx, const fp_mesh* mesh, const float* d_poses, int Hn, float scale, float fx, float fy, float cx,
                          float cy, int W, int Hh, uint8_t* d_rgb, float* d_depth, double* d_ext, int32_t* d_boxes, hipStream_t s) {
    const int V = mesh->V, F = mesh->F;
    SVert* sv;
    int rc;
    if ((rc = project_views(ctx, mesh, d_poses, Hn, scale, fx, fy, cx, cy, s, &sv))) return rc;
    const bool want_ext = d_ext || d_boxes;

    // The launch arithmetic is fp_raster::make_plan (raster_plan.h).
    // fp_ctx_set_option(ctx, "raster_tiled", v): -1 / unset = tiled for images of up to 8 x 8 tiles of <= 88 px and meshes of up to
    // 131 072 triangles, 0 = global visibility buffer, 1 = tiled.  Measured, 576 views @420^2 with boxes + extents (ms; tiled | global,
    // profiles/r06_raster_perf.log): 1 280 triangles 1.64 | 2.57, 20 480: 1.65 | 2.70, 81 920: 2.28 | 2.40, 327 680: 5.04 | 2.81 —
    // both are bound by vector instructions, the tiled path per triangle (set-up in the bin AND the tile kernel, ~1.6 tiles per chunk of
    // 64), the global path per fragment (L2 atomics).  Rounds 1-5 stopped at 32 768 triangles.
    const fp_raster::Plan plan = fp_raster::make_plan(W, Hh, F, Hn, ctx->opt_raster_tiled);
    if (plan.tiled) {
        const int T = plan.T, ntx = plan.ntx, ntile = plan.ntile, nchunk = plan.nchunk;
        uint16_t* tbox;
        unsigned long long* cmask;
        double* part = nullptr;
        if ((rc = ctx->get("raster.tbox", (size_t)Hn * nchunk * BIN_CHUNK * 2, (void**)&tbox))) return rc;
        if ((rc = ctx->get("raster.cmask", (size_t)Hn * nchunk * 8, (void**)&cmask))) return rc;
        if (want_ext && (rc = ctx->get("raster.part", (size_t)Hn * ntile * PART_N * 8, (void**)&part))) return rc;
        hipLaunchKernelGGL(raster_bin_kernel, dim3(plan.bin_grid, Hn), dim3(256), 0, s, sv, mesh->faces, mesh->perm, mesh->fsort, V, F, W, Hh, T, Hn,
                           nchunk, tbox, cmask, mesh->cull);
        FP_LAUNCH_CHECK();
        unsigned long long* dbg_buf = nullptr;
        int raster_dbg = 0;
#ifdef FP_LAB
        raster_dbg = fp_opt_get(FP_OPT_RASTER_DBG, 0);
        if (raster_dbg & (1 << 30)) {                      // phase clocks: summed over all workgroups into "raster.dbg" (fp_lab_read_buffer)
            if ((rc = ctx->get("raster.dbg", 64, (void**)&dbg_buf))) return rc;
            FP_HIP(hipMemsetAsync(dbg_buf, 0, 64, s));
        }
#endif
        FP_DYN_LDS_ONCE(raster_tile_kernel, (int)fp_raster::tile_lds(fp_raster::TILE_MAX));
        hipLaunchKernelGGL(raster_tile_kernel, dim3(ntile, Hn), dim3(256), plan.lds, s, sv, mesh->faces, mesh->perm, mesh->fsort, mesh->sh, mesh->tables,
                           V, F, W, Hh, T, ntx, Hn, tbox, cmask, nchunk, d_rgb, d_depth, part, (double)fx, (double)fy, (double)cx, (double)cy, raster_dbg & ~(1 << 30), dbg_buf);
        FP_LAUNCH_CHECK();
        if (want_ext) {
            hipLaunchKernelGGL(raster_extents_kernel, dim3(Hn), dim3(64), 0, s, part, Hn, ntile, W, Hh, d_ext, d_boxes);
            FP_LAUNCH_CHECK();
        }
        return FP_OK;
    }

    // global visibility-buffer path (large images; A/B reference)
    unsigned long long* zb;
    int* queue;
    const int qcap = 1 << 20;
    if (!d_depth && (rc = ctx->get("raster.depth", (size_t)Hn * W * Hh * 4, (void**)&d_depth))) return rc;   // the extents are taken from it
    if ((rc = ctx->get("raster.zb", (size_t)Hn * W * Hh * 8, (void**)&zb))) return rc;
    if ((rc = ctx->get("raster.queue", (size_t)qcap * 8 + 64, (void**)&queue))) return rc;
    int* qcount = queue + 2 * qcap;
    FP_HIP(hipMemsetAsync(zb, 0xff, (size_t)Hn * W * Hh * 8, s));
    FP_HIP(hipMemsetAsync(qcount, 0, 4, s));
    hipLaunchKernelGGL(raster_tri_kernel, dim3(cdiv(F, 256), Hn), dim3(256), 0, s, sv, mesh->faces, mesh->perm, V, F, W, Hh, zb, queue, qcount, qcap, mesh->cull);
    FP_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_big_kernel, dim3(1024), dim3(256), 0, s, sv, mesh->faces, V, W, Hh, zb, queue, qcount, qcap);
    FP_LAUNCH_CHECK();
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(cdiv(W * Hh, 256), Hn), dim3(256), 0, s, sv, mesh->faces, mesh->sh,
                       mesh->tables, V, W, Hh, zb, d_rgb, d_depth);
    FP_LAUNCH_CHECK();
    if (want_ext) {
        double* ext = d_ext;
        if (!ext && (rc = ctx->get("raster.ext", (size_t)Hn * 64, (void**)&ext))) return rc;
        if ((rc = fp_depth_extents(ctx, d_depth, Hn, Hh, W, fx, fy, cx, cy, ext, s))) return rc;
        if (d_boxes) {
            hipLaunchKernelGGL(ext_boxes_kernel, dim3(cdiv(Hn, 64)), dim3(64), 0, s, ext, Hn, d_boxes);
            FP_LAUNCH_CHECK();
        }
    }
    return FP_OK;
}

static int check_raster_args(const char* who, const void* ctx, const void* mesh, const void* d_poses, const void* d_rgb, bool outputs, int W, int Hh) {
    FP_REQUIRE(ctx && mesh && d_poses && d_rgb && outputs, "%s: null argument", who);
    FP_REQUIRE(W > 0 && Hh > 0 && W <= 8192 && Hh <= 8192, "%s: bad image size", who);
    return FP_OK;
}

extern "C" int fp_rasterize(fp_ctx* ctx, const fp_mesh* mesh, const float* d_poses, int Hn, float scale, float fx,
                            float fy, float cx, float cy, int W, int Hh, uint8_t* d_rgb, float* d_depth, void* stream) {
    const int rc = check_raster_args("rasterize", ctx, mesh, d_poses, d_rgb, d_depth != nullptr, W, Hh);
    if (rc || Hn == 0) return rc;
    return rasterize_impl(ctx, mesh, d_poses, Hn, scale, fx, fy, cx, cy, W, Hh, d_rgb, d_depth, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int fp_rasterize_extents(fp_ctx* ctx, const fp_mesh* mesh, const float* d_poses, int Hn, float scale, float fx,
                                    float fy, float cx, float cy, int W, int Hh, uint8_t* d_rgb, float* d_depth, double* d_ext, int32_t* d_boxes, void* stream) {
    const int rc = check_raster_args("rasterize_extents", ctx, mesh, d_poses, d_rgb, d_ext || d_boxes, W, Hh);
    if (rc || Hn == 0) return rc;
    return rasterize_impl(ctx, mesh, d_poses, Hn, scale, fx, fy, cx, cy, W, Hh, d_rgb, d_depth, d_ext, d_boxes, (hipStream_t)stream);
}

// The plan rasterize_impl would execute for F triangles and Hn views on a W x H frame under this context's "raster_tiled", in words
// (raster_plan.h plan_text), with the thresholds the kernels were compiled with: nothing is launched.  What the tests of the
// rasteriser's branches hold their case table to.
extern "C" int fp_op_raster_plan(fp_ctx* ctx, int W, int H, int F, int Hn, char* out, size_t out_bytes) {
    FP_REQUIRE(ctx && out && out_bytes > 0, "op_raster_plan: null argument");
    FP_REQUIRE(W > 0 && H > 0 && W <= 8192 && H <= 8192 && F > 0 && Hn >= 0, "op_raster_plan: W=%d H=%d F=%d Hn=%d", W, H, F, Hn);
    const int n = fp_raster::plan_text(fp_raster::make_plan(W, H, F, Hn, ctx->opt_raster_tiled), out, out_bytes);
    FP_REQUIRE(n >= 0 && (size_t)n < out_bytes, "op_raster_plan: the text needs %d bytes", n + 1);
    return FP_OK;
}

extern "C" int fp_mesh_set_ambient(fp_mesh* mesh, float ambient) {
    FP_REQUIRE(mesh && ambient >= 0.f, "mesh_set_ambient: bad argument");
    mesh->sh.ambient = ambient;
    return FP_OK;
}
extern "C" int fp_mesh_set_cull(fp_mesh* mesh, int mode) {
    FP_REQUIRE(mesh && (mode == 0 || mode == 1), "mesh_set_cull: mode must be 0 (both sides) or 1 (back faces culled)");
    mesh->cull = mode;
    return FP_OK;
}
extern "C" int fp_mesh_set_filter(fp_mesh* mesh, int mode) {
    FP_REQUIRE(mesh && (mode == 0 || mode == 1), "mesh_set_filter: mode must be 0 (bilinear level 0) or 1 (trilinear mip-maps)");
    mesh->sh.filter = mode;
    return FP_OK;
}
extern "C" int fp_mesh_set_shading(fp_mesh* mesh, int mode) {
    FP_REQUIRE(mesh && (mode == 0 || mode == 1), "mesh_set_shading: mode must be 0 (linear) or 1 (gamma)");
    mesh->sh.shade = mode;
    return FP_OK;
}
