// Serial host run of csrc/gt_info_core.h in the order of gi_visibility_kernel / gi_diameter_kernel (gt_info.hip): for the no-GPU tests,
// built with
//   g++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I freepose_amd/csrc tools/gt_info_host_check.cpp
//
//   gt_info_host_check visibility IN.bin OUT.bin
//     IN.bin:  i32 {B, Hr, Wr, ox, oy, n_img, H, W, want_masks}, i32 img_idx[B], f64 params[B*8], f32 depth_gt[B*Hr*Wr], f32 depth_test[n_img*H*W]
//     OUT.bin: i32 out[B*12], then with want_masks u8 mask[B*H*W], u8 mask_visib[B*H*W]
//   gt_info_host_check diameter IN.bin OUT.bin
//     IN.bin:  i32 {n_pts, M}, i32 ranges[M*2], f64 pts[n_pts*3]
//     OUT.bin: f64 out[M*8]
// Exit status 3 = refused by the bounds predicates (what the C entries refuse), 2 = unreadable input.  Every vector has exactly the
// table's size, so a read or write outside a table is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gt_info_core.h"

template <class V>
static bool read_vec(FILE* f, V& v) {
    return v.empty() || fread(v.data(), sizeof(v[0]), v.size(), f) == v.size();
}
template <class V>
static bool write_vec(FILE* f, const V& v) {
    return v.empty() || fwrite(v.data(), sizeof(v[0]), v.size(), f) == v.size();
}

static int visibility(FILE* f, FILE* o) {
    int32_t h[9];
    if (fread(h, sizeof(int32_t), 9, f) != 9) return 2;
    const int B = h[0], Hr = h[1], Wr = h[2], ox = h[3], oy = h[4], n_img = h[5], H = h[6], W = h[7], want = h[8];
    if (B < 0 || Hr <= 0 || Wr <= 0 || n_img < 1) return 3;
    if (!gi_window_ok(Wr, Hr, ox, oy, W, H)) return 3;
    std::vector<int32_t> idx(B);
    std::vector<double> prm((size_t)B * FP_GI_PARAM_LD);
    std::vector<float> gt((size_t)B * Hr * Wr), test((size_t)n_img * H * W);
    if (!read_vec(f, idx) || !read_vec(f, prm) || !read_vec(f, gt) || !read_vec(f, test)) return 2;
    for (int b = 0; b < B; ++b)
        if (!gi_img_ok(idx[b], n_img)) return 3;
    std::vector<int32_t> out((size_t)B * FP_GI_OUT_LD);
    std::vector<uint8_t> mask(want ? (size_t)B * H * W : 0), visib(want ? (size_t)B * H * W : 0);
    for (int b = 0; b < B; ++b) {
        const float* G = gt.data() + (size_t)b * Hr * Wr;
        const float* T = test.data() + (size_t)idx[b] * H * W;
        const double* p = prm.data() + (size_t)b * FP_GI_PARAM_LD;
        const float delta = (float)p[4];
        GiAcc a;
        for (int y = 0; y < Hr; ++y) {
            for (int x = 0; x < Wr; ++x) {
                const bool inw = gi_in_window(x, y, ox, oy, W, H);
                const size_t w = inw ? (size_t)(y - oy) * W + (x - ox) : 0;
                const float g = G[(size_t)y * Wr + x];
                const float t = (inw && g != 0.f) ? T[w] : 0.f;
                const int bits = gi_pixel(g, t, inw, x, y, ox, oy, p, delta, a);
                if (inw && want) {
                    mask[(size_t)b * H * W + w] = (bits & FP_GI_MASK) ? 255 : 0;
                    visib[(size_t)b * H * W + w] = (bits & FP_GI_VISIB) ? 255 : 0;
                }
            }
        }
        int32_t* r = out.data() + (size_t)b * FP_GI_OUT_LD;
        r[0] = a.all, r[1] = a.valid, r[2] = a.visib, r[3] = 0;
        memcpy(r + 4, a.box_all, sizeof(a.box_all));
        memcpy(r + 8, a.box_vis, sizeof(a.box_vis));
    }
    return write_vec(o, out) && write_vec(o, mask) && write_vec(o, visib) ? 0 : 2;
}

static int diameter(FILE* f, FILE* o) {
    int32_t h[2];
    if (fread(h, sizeof(int32_t), 2, f) != 2) return 2;
    const int n_pts = h[0], M = h[1];
    if (n_pts < 0 || M < 0) return 3;
    std::vector<int32_t> rg((size_t)M * 2);
    std::vector<double> pts((size_t)n_pts * 3), out((size_t)M * FP_GI_DIAM_LD);
    if (!read_vec(f, rg) || !read_vec(f, pts)) return 2;
    for (int m = 0; m < M; ++m)
        if (!gi_range_ok(rg[2 * m], rg[2 * m + 1], n_pts)) return 3;
    for (int m = 0; m < M; ++m) {
        const double* P = pts.data() + (size_t)rg[2 * m] * 3;
        const int n = rg[2 * m + 1];
        double d2 = 0.0, lo[3] = {P[0], P[1], P[2]}, hi[3] = {P[0], P[1], P[2]};
        for (int i = 0; i < n; ++i) {
            for (int k = 0; k < 3; ++k) {
                lo[k] = fmin(lo[k], P[3 * (size_t)i + k]);
                hi[k] = fmax(hi[k], P[3 * (size_t)i + k]);
            }
            for (int j = i; j < n; ++j)
                d2 = fmax(d2, gi_pair_d2(P[3 * (size_t)i], P[3 * (size_t)i + 1], P[3 * (size_t)i + 2], P[3 * (size_t)j], P[3 * (size_t)j + 1],
                                         P[3 * (size_t)j + 2]));
        }
        double* r = out.data() + (size_t)m * FP_GI_DIAM_LD;
        r[0] = gi_sqrt(d2);
        for (int k = 0; k < 3; ++k) r[1 + k] = lo[k], r[4 + k] = hi[k] - lo[k];
        r[7] = 0.0;
    }
    return write_vec(o, out) ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc != 4 || (strcmp(argv[1], "visibility") && strcmp(argv[1], "diameter"))) {
        fprintf(stderr, "usage: %s visibility|diameter IN.bin OUT.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    FILE* o = fopen(argv[3], "wb");
    if (!o) {
        fclose(f);
        return 2;
    }
    const int rc = strcmp(argv[1], "visibility") ? diameter(f, o) : visibility(f, o);
    fclose(f);
    fclose(o);
    return rc;
}
