// scale.hip — object scale from the scene's depth map under each proposal mask, on the device: what `--depth_method depthmap` computes
// per proposal (reference src/pipeline/estimators/scale_estimators.py:117-187 with src/pipeline/utils.py:71-84), batched over the n
// masks [n,H,W] u8 of one image with one shared float64 depth map [H,W].
//
//   a. cc_tile_kernel / cc_seam_kernel / cc_compress_kernel   connected components (4 or 8), union-find on int32 labels whose root is
//      the component's smallest raster index: 32 x 32 tiles in LDS, seams joined with atomicMin in global memory, then every pixel
//      reads its root.  Label = 1 + raster index of the component's first pixel, 0 = background: ranked, that is scipy's numbering.
//   b. cc_compress_kernel counts pixels on the root's counter (integer atomics), cc_best_kernel takes the arg-max with one 64-bit
//      atomicMax of (area << 32 | ~root): largest area first, then the smallest root — "first label in scan order wins".
//   c. scale_d2_kernel   min(d^2, 65) to the nearest pixel outside the chosen component: row pass + column pass in an LDS tile with a
//      halo of 8 (scale_core.h); the image border is not background.  One pass counts the survivors of every radius of the chain.
//   d, e. scale_robust_kernel   one block per mask: radius choice, survivors compacted in raster order, exact median (radix select on
//      order-preserving 64-bit keys), population standard deviation, the cut, back-projection, principal axes, half the largest extent.
//
// Numerics (DESIGN.md "Depth-map scale"): everything up to the kept pixel set is integer or an exact selection; the floating-point
// sums (mean, variance, centroid, scatter matrix) are fp64 in a fixed order — thread t adds elements t, t + 1024, ... in order, then a
// fixed tree — so two calls give the same bits.  No floating-point atomics.  Compiled with -ffp-contract=off: (col - cx) * z / fx is
// the reference's operation sequence.
#include "internal.h"
#include "scale_core.h"

namespace {

constexpr int TILE = 32;                       // labelling / distance tile: 32 x 32 pixels, 256 threads x 4 pixels
constexpr int TPX = TILE * TILE;
constexpr int HALO = FP_SCALE_WIN;
constexpr int HT = TILE + 2 * HALO;            // 48: tile + halo
constexpr int RT = 1024;                       // threads of the per-mask kernel
constexpr int RPX = 4;                         // pixels per thread and compaction round
constexpr int CNT_LD = 8;                      // ints per mask in the survivor-count array

struct ScaleChain { int steps; int thr[FP_SCALE_MAX_STEPS]; };

__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int glb_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- a. labelling ------------------------------------------------------------------------------------------------------------------
// grid (tiles x, tiles y, mask).  uf [n,H,W]: -1 = background, else the raster index of the pixel's root WITHIN ITS TILE (local index
// order is raster order inside a tile, so the smallest local index is the smallest raster index).
__global__ __launch_bounds__(256) void cc_tile_kernel(const uint8_t* __restrict__ masks, int H, int W, int conn8, int* __restrict__ uf) {
    __shared__ int L[TPX];
    const size_t base = (size_t)blockIdx.z * H * W;
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE, tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < TPX / 256; ++k) {
        const int i = k * 256 + tid, gy = y0 + (i >> 5), gx = x0 + (i & 31);
        const bool fg = gy < H && gx < W && masks[base + (size_t)gy * W + gx] != 0;
        L[i] = fg ? i : -1;
    }
    __syncthreads();
    const auto load = [&](int i) { return lds_load(&L[i]); };
    const auto amin = [&](int i, int v) { return atomicMin(&L[i], v); };
#pragma unroll
    for (int k = 0; k < TPX / 256; ++k) {
        const int i = k * 256 + tid, ly = i >> 5, lx = i & 31;
        if (load(i) < 0) continue;
        // every find / union loop strictly decreases a label (scale_core.h: cc_find, cc_union), so each call ends
        if (lx > 0 && load(i - 1) >= 0) cc_union(load, amin, i, i - 1);
        if (ly > 0 && load(i - TILE) >= 0) cc_union(load, amin, i, i - TILE);
        if (conn8 && ly > 0) {
            if (lx > 0 && load(i - TILE - 1) >= 0) cc_union(load, amin, i, i - TILE - 1);
            if (lx < TILE - 1 && load(i - TILE + 1) >= 0) cc_union(load, amin, i, i - TILE + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TPX / 256; ++k) {
        const int i = k * 256 + tid, gy = y0 + (i >> 5), gx = x0 + (i & 31);
        if (gy >= H || gx >= W) continue;
        int g = -1;
        if (L[i] >= 0) {
            const int r = cc_find(load, i);
            g = (y0 + (r >> 5)) * W + x0 + (r & 31);
        }
        uf[base + (size_t)gy * W + gx] = g;
    }
}

// grid (pixel blocks, mask): a pixel joins its left / upper (/ upper-left / upper-right) neighbour when that one lies in another tile
__global__ __launch_bounds__(256) void cc_seam_kernel(int H, int W, int conn8, int* __restrict__ uf) {
    const int HW = H * W, p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    int* L = uf + (size_t)blockIdx.y * HW;
    if (L[p] < 0) return;
    const int y = p / W, x = p - y * W;
    const bool left = (x & (TILE - 1)) == 0, top = (y & (TILE - 1)) == 0, right = (x & (TILE - 1)) == TILE - 1;
    if (!left && !top && !(conn8 && right)) return;
    const auto load = [&](int i) { return glb_load(&L[i]); };
    const auto amin = [&](int i, int v) { return atomicMin(&L[i], v); };
    // labels of foreground pixels are >= 0 and only decrease towards the root: the loops of cc_find / cc_union strictly decrease
    // a label every round (scale_core.h), whatever the other threads do meanwhile
    if (left && x > 0 && load(p - 1) >= 0) cc_union(load, amin, p, p - 1);
    if (top && y > 0 && load(p - W) >= 0) cc_union(load, amin, p, p - W);
    if (conn8 && y > 0) {
        if ((left || top) && x > 0 && load(p - W - 1) >= 0) cc_union(load, amin, p, p - W - 1);
        if ((right || top) && x < W - 1 && load(p - W + 1) >= 0) cc_union(load, amin, p, p - W + 1);
    }
}

// grid (pixel blocks, mask): labels = 1 + root (0 = background); with `area`, one count per pixel on the root's counter
__global__ __launch_bounds__(256) void cc_compress_kernel(int HW, const int* __restrict__ uf, int* __restrict__ labels, int* __restrict__ area) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const size_t base = (size_t)blockIdx.y * HW;
    const int* L = uf + base;
    int r = -1;
    if (L[p] >= 0) r = cc_find([&](int i) { return L[i]; }, p);      // read-only here: plain loads; strictly decreasing as above
    labels[base + p] = r + 1;
    if (area && r >= 0) atomicAdd(&area[base + r], 1);
}

// ---- b. largest component ---------------------------------------------------------------------------------------------------------
// best[m] = max over roots of (area << 32 | 0xffffffff - root); zero-initialised: an empty mask keeps 0
__global__ __launch_bounds__(256) void cc_best_kernel(int HW, const int* __restrict__ labels, const int* __restrict__ area,
                                                      unsigned long long* __restrict__ best) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const size_t base = (size_t)blockIdx.y * HW;
    unsigned long long key = 0;
    if (p < HW && labels[base + p] == p + 1) key = ((unsigned long long)(unsigned)area[base + p] << 32) | (0xffffffffu - (unsigned)p);
#pragma unroll
    for (int mk = 32; mk > 0; mk >>= 1) {
        const unsigned long long o = __shfl_xor(key, mk, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(&best[blockIdx.y], key);
}

// ---- c. capped squared distance ---------------------------------------------------------------------------------------------------
// grid (tiles x, tiles y, mask).  d2 [n,H,W] u8 (zeroed by the launcher): 0 outside the chosen component, else min(d^2, 65).
// cnt [n,CNT_LD] (zeroed): survivors d^2 > thr[k] of every radius of the chain.
__global__ __launch_bounds__(256) void scale_d2_kernel(int H, int W, const int* __restrict__ labels, const unsigned long long* __restrict__ best,
                                                       ScaleChain ch, uint8_t* __restrict__ d2, int* __restrict__ cnt) {
    __shared__ uint8_t mem[HT][HT];        // 1: pixel of the component, or outside the image (not background)
    __shared__ uint8_t rd[HT][TILE];       // row-pass distance
    __shared__ int acc[FP_SCALE_MAX_STEPS];
    const int m = blockIdx.z, tid = threadIdx.x;
    const unsigned long long b = best[m];
    if ((b >> 32) == 0) return;            // empty mask (block-uniform)
    const int want = (int)(0xffffffffu - (unsigned)(b & 0xffffffffu)) + 1;
    const size_t base = (size_t)m * H * W;
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    if (tid < FP_SCALE_MAX_STEPS) acc[tid] = 0;
    for (int i = tid; i < HT * HT; i += 256) {
        const int ly = i / HT, lx = i - ly * HT, gy = y0 - HALO + ly, gx = x0 - HALO + lx;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        mem[ly][lx] = in ? (labels[base + (size_t)gy * W + gx] == want) : 1;
    }
    __syncthreads();
    for (int i = tid; i < HT * TILE; i += 256) {
        const int ly = i >> 5, lx = i & 31, gy = y0 - HALO + ly;
        int r = FP_SCALE_WIN + 1;          // a row outside the image holds no background
        if (gy >= 0 && gy < H) r = edt_row_dist([&](int xx) { return mem[ly][xx] != 0; }, lx + HALO);   // xx in [lx, lx + 16] < HT
        rd[ly][lx] = (uint8_t)r;
    }
    __syncthreads();
    int c[FP_SCALE_MAX_STEPS] = {};
#pragma unroll
    for (int k = 0; k < TPX / 256; ++k) {
        const int i = k * 256 + tid, ly = i >> 5, lx = i & 31, gy = y0 + ly, gx = x0 + lx;
        if (gy >= H || gx >= W) continue;
        const int v = edt_col_d2([&](int dy) { return (int)rd[ly + HALO + dy][lx]; });   // 0 for a pixel outside the component
        d2[base + (size_t)gy * W + gx] = (uint8_t)v;
#pragma unroll
        for (int s = 0; s < FP_SCALE_MAX_STEPS; ++s) c[s] += (s < ch.steps && v > ch.thr[s]) ? 1 : 0;
    }
#pragma unroll
    for (int s = 0; s < FP_SCALE_MAX_STEPS; ++s) {
        int v = c[s];
#pragma unroll
        for (int mk = 32; mk > 0; mk >>= 1) v += __shfl_xor(v, mk, 64);
        if ((tid & 63) == 0 && v) atomicAdd(&acc[s], v);
    }
    __syncthreads();
    if (tid < ch.steps && acc[tid]) atomicAdd(&cnt[m * CNT_LD + tid], acc[tid]);      // integers: the order does not matter
}

// ---- d, e. per-mask statistics ------------------------------------------------------------------------------------------------------
struct RobustSh {
    double red[RT];
    int hist[256];
    int wtot[RT / 64];
    int pick[2];
    double V[9];
};

struct OpSum { __device__ double operator()(double a, double b) const { return a + b; } };
struct OpMin { __device__ double operator()(double a, double b) const { return fmin(a, b); } };
struct OpMax { __device__ double operator()(double a, double b) const { return fmax(a, b); } };

// fixed tree over the block's 1024 values: the same pairing on every call
template <class Op>
__device__ double block_reduce(double v, RobustSh& sh, Op op) {
    const int t = threadIdx.x;
    __syncthreads();
    sh.red[t] = v;
    __syncthreads();
#pragma unroll
    for (int w = RT / 2; w > 0; w >>= 1) {
        if (t < w) sh.red[t] = op(sh.red[t], sh.red[t + w]);
        __syncthreads();
    }
    return sh.red[0];
}

// exclusive rank of this thread's `c` items among the block's (thread order), and the block's total
__device__ int block_rank(const bool* f, int nf, RobustSh& sh, int& total) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int r = 0, wt = 0;
    for (int j = 0; j < nf; ++j) {
        const unsigned long long bal = __ballot(f[j]);
        r += __popcll(bal & below);
        wt += __popcll(bal);
    }
    __syncthreads();
    if (lane == 0) sh.wtot[wv] = wt;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < RT / 64; ++i) {
        const int cw = sh.wtot[i];
        off += i < wv ? cw : 0;
        tot += cw;
    }
    total = tot;
    return off + r;
}

// key of rank k (0-based, k < S) among key(0..S-1): 8 passes of 8 bits from the top, a 256-bin histogram per pass (integer LDS atomics)
template <class KeyFn>
__device__ unsigned long long block_select(KeyFn key, int S, int k, RobustSh& sh) {
    const int t = threadIdx.x;
    unsigned long long prefix = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();
        if (t < 256) sh.hist[t] = 0;
        __syncthreads();
        const unsigned long long hi = shift == 56 ? 0ull : (~0ull << (shift + 8));
        for (int i = t; i < S; i += RT) {
            const unsigned long long kk = key(i);
            if ((kk & hi) == prefix) atomicAdd(&sh.hist[(int)((kk >> shift) & 255)], 1);
        }
        __syncthreads();
        if (t == 0) {
            int acc = 0, b = 0;
            for (; b < 255; ++b) {
                if (acc + sh.hist[b] > k) break;
                acc += sh.hist[b];
            }
            sh.pick[0] = b;
            sh.pick[1] = acc;
        }
        __syncthreads();
        prefix |= (unsigned long long)sh.pick[0] << shift;
        k -= sh.pick[1];
    }
    return prefix;
}

template <int P, int Q>
__device__ __forceinline__ void jacobi_rot(double (&A)[3][3], double (&V)[3][3]) {
    if (A[P][Q] == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * A[P][Q]);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}
// cyclic Jacobi on a symmetric 3 x 3 matrix: columns of V = eigenvectors.  At most 32 sweeps (it converges quadratically: 6-8 in practice)
__device__ void jacobi3(double (&A)[3][3], double (&V)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        const double tr = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (!(off > tr * 0x1p-70)) break;
        jacobi_rot<0, 1>(A, V);
        jacobi_rot<0, 2>(A, V);
        jacobi_rot<1, 2>(A, V);
    }
}

struct RobustArgs {
    const double* depth;       // [H,W]
    const uint8_t* d2;         // [n,H,W]
    const unsigned long long* best;
    const int* cnt;
    int* kidx;                 // [n,H,W] scratch: raster indices of the survivors, in raster order
    uint8_t* kflag;            // [n,H,W] scratch: 1 = the survivor's point enters the extent
    double* scale;             // [n]
    int* info;                 // [n,4]
    uint8_t* keep;             // [n,H,W] (zeroed) or null
    int H, W;
    double fx, fy, cx, cy, std_factor;
    int min_vertices, align;
    ScaleChain ch;
};

__global__ __launch_bounds__(RT) void scale_robust_kernel(RobustArgs a) {
    __shared__ RobustSh sh;
    const int m = blockIdx.x, t = threadIdx.x, HW = a.H * a.W, W = a.W;
    const size_t base = (size_t)m * HW;
    const int area = (int)(a.best[m] >> 32);
    const int ridx = scale_choose_radius(a.cnt + m * CNT_LD, a.ch.steps, a.min_vertices);
    const int tsel = ridx < a.ch.steps ? a.ch.thr[ridx] : 0;       // un-eroded: every pixel of the component has d^2 >= 1
    int* info = a.info + m * 4;
    if (area == 0) {                                                // block-uniform
        if (t == 0) {
            a.scale[m] = __builtin_nan("");
            info[0] = 0; info[1] = a.ch.steps; info[2] = 0; info[3] = 0;
        }
        return;
    }
    const uint8_t* d2 = a.d2 + base;
    int* kidx = a.kidx + base;
    uint8_t* kflag = a.kflag + base;
    // survivors in raster order
    int S = 0;
    for (int c0 = 0; c0 < HW; c0 += RT * RPX) {
        bool f[RPX];
        const int p0 = c0 + t * RPX;
#pragma unroll
        for (int j = 0; j < RPX; ++j) f[j] = p0 + j < HW && (int)d2[p0 + j] > tsel;
        int tot;
        int r = S + block_rank(f, RPX, sh, tot);
#pragma unroll
        for (int j = 0; j < RPX; ++j)
            if (f[j]) kidx[r++] = p0 + j;
        S += tot;
    }
    __syncthreads();                                                // kidx written by other threads is read below
    const double* depth = a.depth;
    const auto zkey = [&](int i) { return scale_key_bits((unsigned long long)__double_as_longlong(depth[kidx[i]])); };
    // exact median: the middle value, or (a + b) / 2 of the two middle values
    double med = __longlong_as_double((long long)scale_unkey_bits(block_select(zkey, S, S / 2, sh)));
    if ((S & 1) == 0) {
        const double lo = __longlong_as_double((long long)scale_unkey_bits(block_select(zkey, S, S / 2 - 1, sh)));
        med = (lo + med) / 2.0;
    }
    // population standard deviation, two passes
    double v = 0.0;
    for (int i = t; i < S; i += RT) v += depth[kidx[i]];
    const double mean = block_reduce(v, sh, OpSum()) / (double)S;
    v = 0.0;
    for (int i = t; i < S; i += RT) {
        const double d = depth[kidx[i]] - mean;
        v += d * d;
    }
    const double thr = sqrt(block_reduce(v, sh, OpSum()) / (double)S) * a.std_factor;
    v = 0.0;
    for (int i = t; i < S; i += RT) v += fabs(depth[kidx[i]] - med) <= thr ? 1.0 : 0.0;      // integers < 2^53: exact in any order
    const int count_le = (int)block_reduce(v, sh, OpSum());
    const int n_keep = scale_n_keep(count_le, S, a.min_vertices);
    if (n_keep == count_le) {                                       // the kept set is {far <= thr}
        for (int i = t; i < S; i += RT) kflag[i] = fabs(depth[kidx[i]] - med) <= thr ? 1 : 0;
    } else {                                                        // the n_keep smallest (far, raster index)
        const auto fkey = [&](int i) { return scale_key_bits((unsigned long long)__double_as_longlong(fabs(depth[kidx[i]] - med))); };
        const double fv = __longlong_as_double((long long)scale_unkey_bits(block_select(fkey, S, n_keep - 1, sh)));
        v = 0.0;
        for (int i = t; i < S; i += RT) v += fabs(depth[kidx[i]] - med) < fv ? 1.0 : 0.0;
        const int need = n_keep - (int)block_reduce(v, sh, OpSum());   // ties at fv taken in raster order
        int seen = 0;
        for (int c0 = 0; c0 < S; c0 += RT) {
            const int i = c0 + t;
            const double far = i < S ? fabs(depth[kidx[i]] - med) : 0.0;
            bool f[1] = {i < S && far == fv};
            int tot;
            const int r = seen + block_rank(f, 1, sh, tot);
            if (i < S) kflag[i] = (far < fv || (f[0] && r < need)) ? 1 : 0;
            seen += tot;
        }
    }
    __syncthreads();
    if (a.keep)
        for (int i = t; i < S; i += RT)
            if (kflag[i]) a.keep[base + kidx[i]] = 1;
    // back-projection (reference :164-169): ((col - cx) * z / fx, (row - cy) * z / fy, z)
    const auto point = [&](int i, double* q) {
        const int p = kidx[i], row = p / W, col = p - row * W;
        const double z = depth[p];
        q[0] = ((double)col - a.cx) * z / a.fx;
        q[1] = ((double)row - a.cy) * z / a.fy;
        q[2] = z;
    };
    double Vm[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    if (a.align) {
        double s[3] = {0, 0, 0}, mu[3], q[3];
        for (int i = t; i < S; i += RT)
            if (kflag[i]) {
                point(i, q);
                s[0] += q[0]; s[1] += q[1]; s[2] += q[2];
            }
#pragma unroll
        for (int k = 0; k < 3; ++k) mu[k] = block_reduce(s[k], sh, OpSum()) / (double)n_keep;
        double c[6] = {0, 0, 0, 0, 0, 0};       // xx xy xz yy yz zz of the centred points
        for (int i = t; i < S; i += RT)
            if (kflag[i]) {
                point(i, q);
                const double x = q[0] - mu[0], y = q[1] - mu[1], z = q[2] - mu[2];
                c[0] += x * x; c[1] += x * y; c[2] += x * z; c[3] += y * y; c[4] += y * z; c[5] += z * z;
            }
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = block_reduce(c[k], sh, OpSum());
        if (t == 0) {
            double A[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}}, Vt[3][3];
            jacobi3(A, Vt);
#pragma unroll
            for (int k = 0; k < 9; ++k) sh.V[k] = Vt[k / 3][k % 3];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 9; ++k) Vm[k / 3][k % 3] = sh.V[k];
    }
    double lo[3], hi[3], q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = __builtin_inf(); hi[k] = -__builtin_inf(); }
    for (int i = t; i < S; i += RT)
        if (kflag[i]) {
            point(i, q);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double w = a.align ? q[0] * Vm[0][k] + q[1] * Vm[1][k] + q[2] * Vm[2][k] : q[k];   // pts @ vh.T
                lo[k] = fmin(lo[k], w);
                hi[k] = fmax(hi[k], w);
            }
        }
    double span = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double mn = block_reduce(lo[k], sh, OpMin()), mx = block_reduce(hi[k], sh, OpMax());
        span = fmax(span, mx - mn);
    }
    if (t == 0) {
        a.scale[m] = span / 2.0;
        info[0] = area; info[1] = ridx; info[2] = S; info[3] = n_keep;
    }
}

}  // namespace

int fp_label_launch(const uint8_t* masks, int n, int H, int W, int connectivity, int* uf, int* labels, int* area, hipStream_t s) {
    const int HW = H * W, conn8 = connectivity == 8;
    const dim3 tiles(cdiv(W, TILE), cdiv(H, TILE), n), px(cdiv(HW, 256), n);
    if (area) FP_HIP(hipMemsetAsync(area, 0, (size_t)n * HW * sizeof(int), s));
    hipLaunchKernelGGL(cc_tile_kernel, tiles, dim3(256), 0, s, masks, H, W, conn8, uf);
    hipLaunchKernelGGL(cc_seam_kernel, px, dim3(256), 0, s, H, W, conn8, uf);
    hipLaunchKernelGGL(cc_compress_kernel, px, dim3(256), 0, s, HW, uf, labels, area);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

int fp_depthmap_scale_launch(const double* depth, const uint8_t* masks, int n, int H, int W, double fx, double fy, double cx, double cy,
                             double erosion_radius, double std_factor, int min_vertices, int align, const FpScaleWs& ws, double* scale,
                             int* info, uint8_t* keep, hipStream_t s) {
    const int HW = H * W;
    ScaleChain ch{};
    ch.steps = scale_radius_chain(erosion_radius, ch.thr);
    if (int rc = fp_label_launch(masks, n, H, W, 4, ws.uf, ws.labels, ws.area, s)) return rc;   // scipy.ndimage.label's default structure
    FP_HIP(hipMemsetAsync(ws.best, 0, (size_t)n * sizeof(unsigned long long), s));
    FP_HIP(hipMemsetAsync(ws.cnt, 0, (size_t)n * CNT_LD * sizeof(int), s));
    FP_HIP(hipMemsetAsync(ws.d2, 0, (size_t)n * HW, s));
    if (keep) FP_HIP(hipMemsetAsync(keep, 0, (size_t)n * HW, s));
    hipLaunchKernelGGL(cc_best_kernel, dim3(cdiv(HW, 256), n), dim3(256), 0, s, HW, ws.labels, ws.area, ws.best);
    hipLaunchKernelGGL(scale_d2_kernel, dim3(cdiv(W, TILE), cdiv(H, TILE), n), dim3(256), 0, s, H, W, ws.labels, ws.best, ch, ws.d2, ws.cnt);
    RobustArgs a{};
    a.depth = depth; a.d2 = ws.d2; a.best = ws.best; a.cnt = ws.cnt;
    a.kidx = ws.uf;                 // the union-find array is finished with: its storage holds the survivor lists
    a.kflag = ws.kflag; a.scale = scale; a.info = info; a.keep = keep;
    a.H = H; a.W = W; a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy; a.std_factor = std_factor;
    a.min_vertices = min_vertices; a.align = align; a.ch = ch;
    hipLaunchKernelGGL(scale_robust_kernel, dim3(n), dim3(RT), 0, s, a);
    FP_LAUNCH_CHECK();
    return FP_OK;
}
