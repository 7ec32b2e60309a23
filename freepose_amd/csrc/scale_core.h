// scale_core.h — the index arithmetic of scale.hip as plain __host__ __device__ functions: union / find on a label array, the row and
// column recurrences of the capped squared distance, the order-preserving key of a double, the erosion-radius chain and the cut size.
// No HIP type appears here, so the same text compiles with g++ into tools/scale_host_check.cpp, which runs it serially on masks from
// a file (under -fsanitize=address,undefined) — the part of the depth-map scale that can be debugged without a GPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FP_HD __host__ __device__ __forceinline__
#else
#define FP_HD inline
#endif

#define FP_SCALE_WIN 8         // half window of the distance pass: erosion radii up to 8
#define FP_SCALE_D2_CAP 65     // min(d^2, 65): every threshold of the chain is <= 64
#define FP_SCALE_MAX_STEPS 5   // radii r, r/2, ... down to the first one below 1 (r <= 8: at most 5)

// ---- union-find on int labels.  Invariant: L[x] <= x for every foreground x (L[x] == x: a root; background holds -1 and is never
// passed in).  Labels only ever decrease (the one write is a min), so the root of a finished component is its smallest index.
// `Load` reads one label (a plain read on the host and in LDS, an agent-scope atomic load on global memory).
template <class Load>
FP_HD int cc_find(Load load, int x) {
    // terminates: the loop continues only while load(x) != x, and then load(x) < x by the invariant, so x strictly decreases and is
    // bounded below by 0 — at most x iterations, also while other threads lower labels concurrently (they keep the invariant).
    for (;;) {
        const int p = load(x);
        if (p == x || p < 0) return x;     // p < 0 cannot happen for foreground; it ends the loop instead of indexing with -1
        x = p;
    }
}
// `AMin(i, v)` stores min(L[i], v) and returns the previous L[i] (atomicMin on the device).
template <class Load, class AMin>
FP_HD void cc_union(Load load, AMin amin, int a, int b) {
    // terminates: each round either returns or replaces (a, b) by (old, b) with old < a after a = max(a, b): max(a, b) strictly
    // decreases every round and is bounded below by 0.
    for (;;) {
        a = cc_find(load, a);
        b = cc_find(load, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }     // a > b: hang the larger root under the smaller
        const int old = amin(a, b);
        if (old == a) return;                              // a was still a root: linked
        a = old;                                           // somebody linked a first (old < a): join old's tree with b's
    }
}

// ---- capped squared distance to the nearest pixel outside the component.  Pixels outside the image are NOT background (scipy's
// distance_transform_edt sees no zeros beyond the array): the caller's `member` answers true there.
// row pass: distance along the row to the nearest non-member, 0 for a non-member itself, FP_SCALE_WIN + 1 when none within the window
template <class Member>
FP_HD int edt_row_dist(Member member, int x) {
    if (!member(x)) return 0;
    for (int d = 1; d <= FP_SCALE_WIN; ++d)
        if (!member(x - d) || !member(x + d)) return d;
    return FP_SCALE_WIN + 1;
}
// column pass: min over dy of dy^2 + rowdist(y + dy)^2, capped.  `rowdist(dy)` is the row-pass value dy rows away (FP_SCALE_WIN + 1
// for a row outside the image).  Exact whenever the true d^2 <= 64: the nearest outside pixel then lies within the window.
template <class RowDist>
FP_HD int edt_col_d2(RowDist rowdist) {
    int best = FP_SCALE_D2_CAP;
    for (int dy = -FP_SCALE_WIN; dy <= FP_SCALE_WIN; ++dy) {
        const int r = rowdist(dy);
        const int v = dy * dy + r * r;
        best = v < best ? v : best;
    }
    return best;
}

// ---- order-preserving 64-bit key of a double (a < b  <=>  key(a) < key(b) for all non-NaN a, b with -0 < +0)
FP_HD uint64_t scale_key_bits(uint64_t bits) { return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull); }
FP_HD uint64_t scale_unkey_bits(uint64_t key) { return (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key; }

// ---- erosion chain (reference scale_estimators.py:141-149): radii r, r/2, ... while the radius tried last was >= 1.
// isotropic_erosion(m, r) = d > r  <=>  d^2 > r^2  <=>  d^2 > floor(r^2) for the integer d^2.  Returns the number of steps.
FP_HD int scale_radius_chain(double radius, int* thr /*[FP_SCALE_MAX_STEPS]*/) {
    int steps = 0;
    for (;;) {
        const double r2 = radius * radius;
        thr[steps++] = (int)r2;                       // floor: r2 >= 0
        if (radius < 1.0 || steps == FP_SCALE_MAX_STEPS) return steps;
        radius /= 2;
    }
}
// first step whose survivor count exceeds min_vertices; `steps` = the un-eroded component
FP_HD int scale_choose_radius(const int* cnt, int steps, int min_vertices) {
    for (int k = 0; k < steps; ++k)
        if (cnt[k] > min_vertices) return k;
    return steps;
}
// reference :160-161: n = max(argmax(far_sorted > thr), min_vertices), then z[:n].  argmax of the sorted flags is count(far <= thr)
// when some sample exceeds thr and 0 when none does (the quirk); slicing clips n to the sample count.
FP_HD int scale_n_keep(int count_le, int count, int min_vertices) {
    const int cut = count_le < count ? count_le : 0;
    const int n = cut > min_vertices ? cut : min_vertices;
    return n < count ? n : count;
}
