// C-ABI entry points of libfreepose_hip.so (see include/freepose_hip.h): the context and its options, the thin entries over the
// launchers, the timers.  The transformer towers have their own drivers (vit.hip, clip.hip).
#include <stdarg.h>
#include <stdio.h>

#include "../../include/freepose_hip.h"
#include "tower_steps.h"
#include "pnp_core.h"
#include "video_eval_core.h"
#include "gt_info_core.h"
#include "lk_core.h"

// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void fp_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* fp_last_error(void) { return g_err; }
extern "C" int fp_version(void) { return 100; }

#ifdef FP_LAB
// lab build only: process-global experiment toggles (tools/ A/B runs)
static int g_opts[FP_OPT_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
int fp_opt_get(int key, int dflt) { return (key >= 0 && key < FP_OPT_COUNT && g_opts[key] >= 0) ? g_opts[key] : dflt; }
extern "C" int fp_lab_set_option(const char* name, int value) {
    FP_REQUIRE(name, "lab_set_option: null name");
    if (!strcmp(name, "gemm_variant")) g_opts[FP_OPT_GEMM_VARIANT] = value;
    else if (!strcmp(name, "attn_slots")) g_opts[FP_OPT_ATTN_SLOTS] = value;
    else if (!strcmp(name, "gemm_dbg")) g_opts[FP_OPT_GEMM_DBG] = value;   // measurement hooks with wrong numerics
    else if (!strcmp(name, "attn_variant")) g_opts[FP_OPT_ATTN_VARIANT] = value;
    else if (!strcmp(name, "topk_select")) g_opts[FP_OPT_TOPK_SELECT] = value;
    else if (!strcmp(name, "gemm_ring")) g_opts[FP_OPT_GEMM_RING] = value;   // cap on the 64x64 tier's K-tile ring depth
    else if (!strcmp(name, "gemm_sk")) g_opts[FP_OPT_GEMM_SK] = value;       // balanced tier: 1 never, 2 / 3 / 4 force a form (gemm_bf16.hip)
    else if (!strcmp(name, "gemm_sk_grid")) g_opts[FP_OPT_GEMM_SK_GRID] = value;
    else if (!strcmp(name, "raster_dbg")) g_opts[FP_OPT_RASTER_DBG] = value;           // tile kernel ablation bits (raster.hip)
    else if (!strcmp(name, "gemm_stream_mb")) g_opts[FP_OPT_GEMM_STREAM_MB] = value;   // big tier: outputs above this many MiB are stored non-temporally
    else { fp_set_error("lab_set_option: unknown option '%s'", name); return FP_ERR_INVALID; }
    return FP_OK;
}
// lab build only: copy the head of the balanced tier's scratch buffer to the host (gemm_dbg = 1024 leaves per-workgroup phase timestamps there)
extern "C" int fp_lab_read_scratch(fp_ctx* ctx, void* host, size_t bytes) {
    FP_REQUIRE(ctx && host && ctx->sk_ws && bytes <= fp_ctx::SK_WS_BYTES, "lab_read_scratch: no scratch");
    FP_HIP(hipDeviceSynchronize());
    FP_HIP(hipMemcpy(host, ctx->sk_ws, bytes, hipMemcpyDeviceToHost));
    return FP_OK;
}
// lab build only: copy a named workspace of the context to the host (raster.dbg: the tile kernel's phase clocks)
extern "C" int fp_lab_read_buffer(fp_ctx* ctx, const char* name, void* host, size_t bytes) { return fp_op_workspace_read(ctx, name, host, bytes); }
#endif

extern "C" int fp_ctx_set_option(fp_ctx* ctx, const char* name, int value) {
    FP_REQUIRE(ctx && name, "ctx_set_option: null argument");
    if (!strcmp(name, "ln_fused")) ctx->opt_ln_fused = value;
    else if (!strcmp(name, "raster_tiled")) ctx->opt_raster_tiled = value;
    else if (!strcmp(name, "gemm_row_split")) ctx->opt_row_split = value;
    else if (!strcmp(name, "comm_timeout_s")) ctx->opt_comm_timeout_s = value;
#ifdef FP_LAB
    else if (!strcmp(name, "gemm_stream_k")) ctx->opt_stream_k = value;   // lab: 0 = never lend the balanced tier its scratch
#endif
    else { fp_set_error("ctx_set_option: unknown option '%s'", name); return FP_ERR_INVALID; }
    return FP_OK;
}

int fp_ctx::get(const char* name, size_t bytes, void** out) {
    Buf& b = bufs[name];
    if (b.bytes < bytes) {
        if (b.p) FP_HIP(hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
        size_t want = bytes + bytes / 8 + 4096;
        FP_HIP(hipMalloc(&b.p, want));
        b.bytes = want;
    }
    *out = b.p;
    return FP_OK;
}
#ifdef FP_LAB
int fp_ctx::sk_scratch(FpGemmArgs& g, hipStream_t s) {
    g.sk_mode = opt_stream_k == 0 ? 1 : 0;
    if (g.sk_mode == 1) return FP_OK;
    if (!sk_ws) {
        FP_HIP(hipMalloc((void**)&sk_ws, SK_WS_BYTES));
        FP_HIP(hipMalloc((void**)&sk_cnt, SK_CNT_N * sizeof(int)));
        FP_HIP(hipMemsetAsync(sk_cnt, 0, SK_CNT_N * sizeof(int), s));   // the kernels leave the counters at zero
        FP_HIP(hipStreamSynchronize(s));                                 // (other streams of this context may use them next)
    }
    g.sk_ws = sk_ws; g.sk_ws_bytes = SK_WS_BYTES;
    g.sk_cnt = sk_cnt; g.sk_cnt_n = SK_CNT_N;
    return FP_OK;
}
#endif
int fp_ctx::gemm(FpGemmArgs& g, int epi, hipStream_t s) {
    g.no_split = opt_row_split == 0;   // fp_ctx_set_option(ctx, "gemm_row_split", 0)
    g.sk_mode = 1;                     // the balanced tier is compiled into the lab build only (gemm_bf16.hip): the product lends no scratch
#ifdef FP_LAB
    if (int rc = sk_scratch(g, s)) return rc;
#endif
    return fp_gemm_bf16(g, epi, s);
}
size_t fp_ctx::total() const {
    size_t t = 0;
    for (auto& kv : bufs) t += kv.second.bytes;
    return t;
}
void fp_ctx::release() {
    for (auto& kv : bufs)
        if (kv.second.p) (void)hipFree(kv.second.p);
    bufs.clear();
    if (sk_ws) (void)hipFree(sk_ws);
    if (sk_cnt) (void)hipFree(sk_cnt);
    if (ffa_arrive) (void)hipFree(ffa_arrive);
    sk_ws = nullptr;
    sk_cnt = nullptr;
    ffa_arrive = nullptr;
}

extern "C" int fp_ctx_create(int device, fp_ctx** out) {
    FP_REQUIRE(out, "ctx_create: null out");
    int n = 0;
    FP_HIP(hipGetDeviceCount(&n));
    FP_REQUIRE(device >= 0 && device < n, "ctx_create: device %d out of range (%d visible)", device, n);
    FP_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    FP_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fp_set_error("ctx_create: device %d is %s; this library contains gfx950 (MI355X) code only", device,
                     prop.gcnArchName);
        return FP_ERR_STATE;
    }
    // the code object is built for gfx950:sramecc+ only (the fc1 epilogue's LDS table gather relies on the d16 load behaviour of that
    // mode, gemm_epilogue.h): on a device or partition reporting sramecc- no kernel image would load — say so instead of failing on
    // the first launch with "no kernel image is available"
    if (strstr(prop.gcnArchName, "sramecc-")) {
        fp_set_error("ctx_create: device %d is %s; libfreepose_hip is built for gfx950:sramecc+ (SRAM ECC enabled) only", device, prop.gcnArchName);
        return FP_ERR_STATE;
    }
    if (int rc = fp_gemm_gelu_table(nullptr)) return rc;   // per-device constant table of the fc1 epilogue
    fp_ctx* c = new fp_ctx();
    c->device = device;
    *out = c;
    return FP_OK;
}
extern "C" int fp_ctx_destroy(fp_ctx* ctx) {
    if (!ctx) return FP_OK;
    (void)fp_comm_destroy(ctx);
    ctx->release();
    delete ctx;
    return FP_OK;
}
extern "C" size_t fp_ctx_workspace_bytes(const fp_ctx* ctx) { return ctx ? ctx->total() : 0; }

// ---------------------------------------------------------------------------------------------
// FFA / retrieval / template score
extern "C" int fp_ffa(fp_ctx* ctx, const void* d_feats, const uint8_t* d_mask, int B, int gh, int gw, int D, int cell,
                      int normalize, void* d_out_bf16, float* d_out_f32, void* stream) {
    FP_REQUIRE(ctx && d_feats && d_mask && (d_out_bf16 || d_out_f32), "ffa: null argument");
    if (B == 0) return FP_OK;
    hipStream_t s = (hipStream_t)stream;
    bf16_t* tmp = (bf16_t*)d_out_bf16;
    int rc;
    if (normalize || !tmp)
        FP_WS(ctx, "ffa.tmp", (size_t)B * D * 2, tmp);
    uint8_t* pm = nullptr;
    if (cell > 1) FP_WS(ctx, "ffa.pm", (size_t)B * gh * gw, pm);
    if (normalize) FP_REQUIRE(d_out_bf16, "ffa: normalize needs a bf16 output");
    // up to FFA_FUSED_MAX crops (the queries of an image / a frame window) the masked-mean kernel normalises the rows itself (its last
    // column-slab workgroup per crop); beyond (bank building) the row kernel does
    constexpr int FFA_FUSED_MAX = 16;
    int* arrive = nullptr;
    if (normalize && B <= FFA_FUSED_MAX && D % 8 == 0 && (((uintptr_t)tmp | (uintptr_t)d_out_bf16) & 15) == 0) {
        if (!ctx->ffa_arrive) {
            FP_HIP(hipMalloc((void**)&ctx->ffa_arrive, FFA_FUSED_MAX * sizeof(int)));
            FP_HIP(hipMemsetAsync(ctx->ffa_arrive, 0, FFA_FUSED_MAX * sizeof(int), s));
        }
        arrive = ctx->ffa_arrive;
    }
    if ((rc = fp_ffa_pool((const bf16_t*)d_feats, d_mask, tmp, normalize ? nullptr : d_out_f32, B, gh * gw, D, gh, gw,
                          cell, pm, s, arrive ? (bf16_t*)d_out_bf16 : nullptr, arrive)))
        return rc;
    if (normalize && !arrive)
        if ((rc = fp_l2norm_rows(tmp, (bf16_t*)d_out_bf16, B, D, s))) return rc;
    return FP_OK;
}

extern "C" int fp_l2_normalize(fp_ctx* ctx, const void* x, int rows, int D, void* y, void* stream) {
    FP_REQUIRE(ctx && x && y, "l2_normalize: null argument");
    return fp_l2norm_rows((const bf16_t*)x, (bf16_t*)y, rows, D, (hipStream_t)stream);
}

extern "C" int fp_bank_prepare(fp_ctx* ctx, const float* d_bank_f32, int N, int D, void* d_bank_bf16, void* stream) {
    FP_REQUIRE(ctx && d_bank_f32 && d_bank_bf16 && N > 0, "bank_prepare: null argument");
    hipStream_t s = (hipStream_t)stream;
    bf16_t* tmp;
    int rc;
    FP_WS(ctx, "bank.cast", (size_t)N * D * 2, tmp);
    if ((rc = fp_cast_f32_bf16(d_bank_f32, tmp, (size_t)N * D, s))) return rc;
    return fp_l2norm_rows(tmp, (bf16_t*)d_bank_bf16, N, D, s);
}

extern "C" int fp_bank_topk(fp_ctx* ctx, const void* d_bank, int N, int D, const void* d_queries, int Q, int k,
                            int idx_offset, float* d_out_scores, int32_t* d_out_idx, void* stream) {
    FP_REQUIRE(ctx && d_bank && d_queries && d_out_scores && d_out_idx, "bank_topk: null argument");
    if (Q == 0) return FP_OK;
    hipStream_t s = (hipStream_t)stream;
    uint16_t* keys;
    int rc;
    const int ldk = (N + 7) & ~7;   // key rows padded to 16 bytes (vector staging in the select kernel)
    FP_WS(ctx, "topk.keys", (size_t)Q * ldk * 2, keys);
    if ((rc = fp_bank_scan((const bf16_t*)d_bank, (const bf16_t*)d_queries, keys, ldk, N, D, Q, s))) return rc;
    return fp_topk_select(keys, ldk, N, Q, k, idx_offset, d_out_scores, d_out_idx, s);
}

extern "C" int fp_topk_merge(fp_ctx* ctx, const float* cs, const int32_t* ci, int Q, int C, int k, float* os,
                             int32_t* oi, void* stream) {
    FP_REQUIRE(ctx && cs && ci && os && oi, "topk_merge: null argument");
    if (Q == 0) return FP_OK;
    return fp_topk_merge_launch(cs, ci, Q, C, k, os, oi, (hipStream_t)stream);
}

extern "C" int fp_rerank_views(fp_ctx* ctx, const void* d_views, const int32_t* d_offsets, const int32_t* d_cand,
                               const void* d_queries, int Q, int C, int D, int k, float* d_out, void* stream) {
    FP_REQUIRE(ctx && d_views && d_offsets && d_cand && d_queries && d_out, "rerank_views: null argument");
    if (Q == 0 || C == 0) return FP_OK;
    return fp_rerank_views_launch((const bf16_t*)d_views, d_offsets, d_cand, (const bf16_t*)d_queries, d_out, Q, C, D, k,
                                  (hipStream_t)stream);
}

extern "C" int fp_template_score(fp_ctx* ctx, const void* d_tmpl, const void* d_query, const float* d_weights, int T,
                                 int P, int D, float* d_scores, void* stream) {
    FP_REQUIRE(ctx && d_tmpl && d_query && d_scores, "template_score: null argument");
    if (T == 0) return FP_OK;
    float* dots;
    FP_WS(ctx, "tmpl.dots", (size_t)T * P * 4, dots);
    return fp_template_score_launch((const bf16_t*)d_tmpl, (const bf16_t*)d_query, d_weights, dots, d_scores, T, P, D, 0,
                                    (hipStream_t)stream);
}

extern "C" int fp_template_score_normed(fp_ctx* ctx, const void* d_tmpl_normed, const void* d_query, const float* d_weights,
                                        int T, int P, int D, float* d_scores, void* stream) {
    FP_REQUIRE(ctx && d_tmpl_normed && d_query && d_scores, "template_score_normed: null argument");
    if (T == 0) return FP_OK;
    float* dots;
    FP_WS(ctx, "tmpl.dots", (size_t)T * P * 4, dots);
    return fp_template_score_launch((const bf16_t*)d_tmpl_normed, (const bf16_t*)d_query, d_weights, dots, d_scores, T, P, D, 1,
                                    (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// pose-error evaluation (eval.hip)
extern "C" int fp_chamfer(fp_ctx* ctx, const double* d_pts, int n_pts, const int32_t* d_table, const double* d_xf, int B, int max_n,
                          int ws_pts, int projected, double* d_out, void* stream) {
    FP_REQUIRE(ctx && d_pts && d_table && d_xf && d_out, "chamfer: null argument");
    FP_REQUIRE(B > 0 && B <= 65535, "chamfer: B=%d pairs (1..65535 per call)", B);
    FP_REQUIRE(n_pts > 0 && max_n > 0 && max_n <= n_pts, "chamfer: n_pts=%d max_n=%d (0 < max_n <= n_pts)", n_pts, max_n);
    FP_REQUIRE(ws_pts >= 2 && (size_t)ws_pts <= (size_t)2 * B * (size_t)max_n, "chamfer: ws_pts=%d for %d pairs of clouds up to %d points",
               ws_pts, B, max_n);
    FP_REQUIRE(projected == 0 || projected == 1, "chamfer: projected=%d (0 or 1)", projected);
    float* ws;
    double* slots;
    FP_WS(ctx, "chamfer.cloud", (size_t)ws_pts * 3 * sizeof(float), ws);
    FP_WS(ctx, "chamfer.slots", (size_t)B * 2 * fp_chamfer_chunks(max_n) * sizeof(double), slots);
    return fp_chamfer_launch(d_pts, n_pts, d_table, d_xf, B, max_n, ws_pts, projected, ws, slots, d_out, (hipStream_t)stream);
}

extern "C" int fp_depth_compare(fp_ctx* ctx, const float* d_depth_est, const float* d_depth_gt, int B, int Hh, int W,
                                const float* d_depth_test, int n_img, const int32_t* d_img_idx, const double* d_params,
                                const double* d_taus, int n_tau, int32_t* d_out, void* stream) {
    FP_REQUIRE(ctx && d_depth_est && d_depth_gt && d_out, "depth_compare: null argument");
    FP_REQUIRE(B > 0 && B <= 65535, "depth_compare: B=%d pairs (1..65535 per call)", B);
    FP_REQUIRE(Hh > 0 && W > 0 && (size_t)Hh * W <= ((size_t)1 << 30), "depth_compare: image %d x %d", W, Hh);
    if (d_depth_test) {
        FP_REQUIRE(d_img_idx && d_params && d_taus, "depth_compare: the VSD counts need d_img_idx, d_params and d_taus");
        FP_REQUIRE(n_img > 0 && n_tau > 0 && n_tau <= FP_EVAL_MAX_TAUS, "depth_compare: n_img=%d n_tau=%d (n_tau 1..%d)", n_img, n_tau,
                   FP_EVAL_MAX_TAUS);
    } else {
        FP_REQUIRE(n_tau == 0, "depth_compare: n_tau=%d without a test depth image (the CUS counts take none)", n_tau);
    }
    return fp_depth_compare_launch(d_depth_est, d_depth_gt, B, Hh, W, d_depth_test, n_img, d_img_idx, d_params, d_taus, n_tau, d_out,
                                   (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// ground-truth visibility, masks, boxes and model diameters (gt_info.hip).  d_img_idx and d_ranges are small device tables: they are
// copied to the host and checked with gt_info_core.h's predicates before anything is launched (one stream synchronisation per call).
extern "C" int fp_gt_visibility(fp_ctx* ctx, const float* d_depth_gt, int B, int Hr, int Wr, int ox, int oy, const float* d_depth_test,
                                int n_img, int H, int W, const int32_t* d_img_idx, const double* d_params, uint8_t* d_mask,
                                uint8_t* d_mask_visib, int32_t* d_out, void* stream) {
    FP_REQUIRE(ctx, "gt_visibility: null context");
    FP_REQUIRE(B >= 0 && B <= 65535, "gt_visibility: B=%d instances (0..65535 per call)", B);
    FP_REQUIRE(Hr > 0 && Wr > 0 && (size_t)Hr * Wr <= ((size_t)1 << 30), "gt_visibility: canvas %d x %d", Wr, Hr);
    FP_REQUIRE(gi_window_ok(Wr, Hr, ox, oy, W, H), "gt_visibility: window %d x %d at (%d, %d) leaves the canvas %d x %d", W, H, ox, oy, Wr, Hr);
    FP_REQUIRE(n_img > 0, "gt_visibility: n_img=%d test depth images (>= 1)", n_img);
    if (B == 0) return FP_OK;
    FP_REQUIRE(d_depth_gt && d_depth_test && d_img_idx && d_params && d_out, "gt_visibility: null d_depth_gt, d_depth_test, d_img_idx, d_params or d_out");
    std::vector<int32_t> idx(B);
    FP_HIP(hipMemcpyAsync(idx.data(), d_img_idx, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    FP_HIP(hipStreamSynchronize((hipStream_t)stream));
    for (int b = 0; b < B; ++b) FP_REQUIRE(gi_img_ok(idx[b], n_img), "gt_visibility: d_img_idx[%d] = %d outside [0, %d)", b, idx[b], n_img);
    return fp_gt_visibility_launch(d_depth_gt, B, Hr, Wr, ox, oy, d_depth_test, n_img, H, W, d_img_idx, d_params, d_mask, d_mask_visib, d_out,
                                   (hipStream_t)stream);
}

extern "C" int fp_pts_diameter(fp_ctx* ctx, const double* d_pts, int n_pts, const int32_t* d_ranges, int M, double* d_out, void* stream) {
    FP_REQUIRE(ctx, "pts_diameter: null context");
    FP_REQUIRE(M >= 0 && M <= 65535, "pts_diameter: M=%d models (0..65535 per call)", M);
    FP_REQUIRE(n_pts >= 0, "pts_diameter: n_pts=%d", n_pts);
    if (M == 0) return FP_OK;
    FP_REQUIRE(d_pts && d_ranges && d_out, "pts_diameter: null d_pts, d_ranges or d_out");
    std::vector<int32_t> rg((size_t)M * 2);
    FP_HIP(hipMemcpyAsync(rg.data(), d_ranges, rg.size() * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
    FP_HIP(hipStreamSynchronize((hipStream_t)stream));
    int max_count = 0;
    for (int m = 0; m < M; ++m) {
        FP_REQUIRE(gi_range_ok(rg[2 * m], rg[2 * m + 1], n_pts), "pts_diameter: range %d = {first %d, count %d} is empty or outside [0, %d]", m,
                   rg[2 * m], rg[2 * m + 1], n_pts);
        max_count = std::max(max_count, rg[2 * m + 1]);
    }
    FP_REQUIRE(max_count <= FP_DIAM_MAX_POINTS, "pts_diameter: a model of %d points (at most %d)", max_count, FP_DIAM_MAX_POINTS);
    const size_t tiles = (size_t)cdiv(max_count, fp_pts_diameter_tile()), n_slots = (size_t)M * (tiles * (tiles + 1) / 2);
    FP_REQUIRE(n_slots <= FP_DIAM_MAX_SLOTS, "pts_diameter: %d models of up to %d points need %zu per-block slots (at most %zu per call)", M,
               max_count, n_slots, (size_t)FP_DIAM_MAX_SLOTS);
    double* slots;
    FP_WS(ctx, "diam.slots", n_slots * sizeof(double), slots);
    return fp_pts_diameter_launch(d_pts, n_pts, d_ranges, M, max_count, slots, d_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// connected components and the depth-map object scale (scale.hip)
extern "C" int fp_label_components(fp_ctx* ctx, const uint8_t* d_masks, int n, int H, int W, int connectivity, int32_t* d_labels,
                                   void* stream) {
    FP_REQUIRE(ctx && d_masks && d_labels, "label_components: null argument");
    FP_REQUIRE(connectivity == 4 || connectivity == 8, "label_components: connectivity %d (4 or 8)", connectivity);
    FP_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W <= ((size_t)1 << 30), "label_components: image %d x %d", W, H);
    FP_REQUIRE(n >= 0 && n <= 65535, "label_components: n=%d masks (0..65535 per call)", n);
    if (n == 0) return FP_OK;
    int* uf;
    FP_WS(ctx, "scale.uf", (size_t)n * H * W * sizeof(int), uf);
    return fp_label_launch(d_masks, n, H, W, connectivity, uf, d_labels, nullptr, (hipStream_t)stream);
}

extern "C" int fp_depthmap_scale(fp_ctx* ctx, const double* d_depth, const uint8_t* d_masks, int n, int H, int W, double fx, double fy,
                                 double cx, double cy, double erosion_radius, double std_factor, int min_vertices, int align,
                                 double* d_scale, int32_t* d_info, uint8_t* d_keep, void* stream) {
    FP_REQUIRE(ctx && d_depth && d_masks && d_scale && d_info, "depthmap_scale: null argument");
    FP_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W <= ((size_t)1 << 30), "depthmap_scale: image %d x %d", W, H);
    FP_REQUIRE(n >= 0 && n <= 65535, "depthmap_scale: n=%d masks (0..65535 per call)", n);
    FP_REQUIRE(erosion_radius > 0.0 && erosion_radius <= 8.0, "depthmap_scale: erosion_radius %g (0 < r <= 8: the distance window)", erosion_radius);
    FP_REQUIRE(std_factor >= 0.0 && min_vertices >= 1, "depthmap_scale: std_factor %g, min_vertices %d (>= 0, >= 1)", std_factor, min_vertices);
    FP_REQUIRE(fx != 0.0 && fy != 0.0, "depthmap_scale: focal lengths %g, %g", fx, fy);
    FP_REQUIRE(align == 0 || align == 1, "depthmap_scale: align=%d (0 or 1)", align);
    if (n == 0) return FP_OK;
    const size_t px = (size_t)n * H * W;
    FpScaleWs ws{};
    FP_WS(ctx, "scale.uf", px * sizeof(int), ws.uf);
    FP_WS(ctx, "scale.labels", px * sizeof(int), ws.labels);
    FP_WS(ctx, "scale.area", px * sizeof(int), ws.area);
    FP_WS(ctx, "scale.d2", px, ws.d2);
    FP_WS(ctx, "scale.kflag", px, ws.kflag);
    FP_WS(ctx, "scale.best", (size_t)n * sizeof(unsigned long long), ws.best);
    FP_WS(ctx, "scale.cnt", (size_t)n * 8 * sizeof(int), ws.cnt);
    return fp_depthmap_scale_launch(d_depth, d_masks, n, H, W, fx, fy, cx, cy, erosion_radius, std_factor, min_vertices, align, ws, d_scale,
                                    d_info, d_keep, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// TrackingRefiner correspondences and pose from tracks (refine.hip)
extern "C" int fp_patch_points(fp_ctx* ctx, const double* d_samples, int S, const double* d_T, const double* d_K, const int32_t* d_cells,
                               const int32_t* d_ncells, int B, int C, double patch, int32_t* d_out, void* stream) {
    FP_REQUIRE(ctx && d_samples && d_T && d_K && d_cells && d_ncells && d_out, "patch_points: null argument");
    FP_REQUIRE(S >= 1 && S <= (1 << 24), "patch_points: S=%d samples (1..2^24)", S);
    FP_REQUIRE(B >= 0 && B <= 65535, "patch_points: B=%d items (0..65535 per call)", B);
    FP_REQUIRE(C >= 0 && C <= (1 << 20), "patch_points: C=%d cells per item (0..2^20)", C);
    FP_REQUIRE(patch > 0.0, "patch_points: patch %g (> 0)", patch);
    if (B == 0 || C == 0) return FP_OK;
    double* ws;
    FP_WS(ctx, "refine.proj", (size_t)B * 4 * S * sizeof(double), ws);
    return fp_patch_points_launch(d_samples, S, d_T, d_K, d_cells, d_ncells, B, C, patch, ws, d_out, (hipStream_t)stream);
}

extern "C" int fp_pnp_epnp(fp_ctx* ctx, const double* d_pts3d, const double* d_pts2d, const uint8_t* d_vis, const double* d_K9, int B, int N,
                           double* d_out, void* stream) {
    FP_REQUIRE(ctx && d_pts3d && d_pts2d && d_K9 && d_out, "pnp_epnp: null argument");
    FP_REQUIRE(N >= FP_PNP_MIN_N && N <= FP_PNP_MAX_N, "pnp_epnp: N=%d points (%d..%d)", N, FP_PNP_MIN_N, FP_PNP_MAX_N);
    FP_REQUIRE(B >= 0 && B <= (1 << 20), "pnp_epnp: B=%d problems (0..2^20 per call)", B);
    if (B == 0) return FP_OK;
    return fp_pnp_epnp_launch(d_pts3d, d_pts2d, d_vis, d_K9, B, N, d_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// video velocity errors (video_eval.hip).  The per-track tables come from the host: every limit is checked here, before anything is
// launched, and the tables are then copied into the context's workspace in stream order.
extern "C" int fp_video_errors(fp_ctx* ctx, const double* d_est, const double* d_gt, const int32_t* h_meta, const double* h_params, int M,
                               int V, int Nmax, int D, double* d_per_offset, double* d_final, double* d_aligned, double* d_pairs,
                               void* stream) {
    FP_REQUIRE(ctx && d_est && d_gt && h_meta && h_params && d_per_offset && d_final, "video_errors: null argument");
    FP_REQUIRE(M >= 0 && M <= 65535, "video_errors: M=%d tracks (0..65535 per call)", M);
    FP_REQUIRE(V >= 1 && V <= (1 << 20), "video_errors: V=%d ground-truth trajectories (1..2^20)", V);
    FP_REQUIRE(Nmax >= FP_VE_MIN_N && Nmax <= (1 << 20), "video_errors: Nmax=%d frames (%d..2^20)", Nmax, FP_VE_MIN_N);
    FP_REQUIRE(D >= 1 && D <= FP_VE_MAX_D, "video_errors: D=%d time offsets (1..%d)", D, FP_VE_MAX_D);
    for (int m = 0; m < M; ++m) {
        const int32_t* mt = h_meta + (size_t)m * FP_VE_META_LD;
        const double* pr = h_params + (size_t)m * FP_VE_PARAM_LD;
        FP_REQUIRE(mt[0] >= 0 && mt[0] < V, "video_errors: track %d: video %d (0..%d)", m, mt[0], V - 1);
        FP_REQUIRE(mt[1] >= FP_VE_MIN_N && mt[1] <= Nmax, "video_errors: track %d: N=%d frames (%d..Nmax=%d)", m, mt[1], FP_VE_MIN_N, Nmax);
        FP_REQUIRE(mt[2] >= 1 && mt[2] <= FP_VE_MAX_SYM, "video_errors: track %d: n_sym=%d (1..%d)", m, mt[2], FP_VE_MAX_SYM);
        FP_REQUIRE((mt[3] & ~(FP_VE_HAS_AXIS | FP_VE_HAS_K | FP_VE_NO_ALIGN)) == 0, "video_errors: track %d: flags %d", m, mt[3]);
        for (int d = 0; d < D; ++d)
            FP_REQUIRE(mt[4 + d] >= 1 && mt[4 + d] <= mt[1] - 1, "video_errors: track %d: dt[%d]=%d (1..N-1=%d)", m, d, mt[4 + d], mt[1] - 1);
        FP_REQUIRE(pr[0] > 0.0 && pr[1] > 0.0 && pr[0] < INFINITY && pr[1] < INFINITY, "video_errors: track %d: scales %g, %g (finite, > 0)",
                   m, pr[0], pr[1]);
        FP_REQUIRE(pr[2] > 0.0 && pr[3] > 0.0 && pr[2] < INFINITY && pr[3] < INFINITY, "video_errors: track %d: frame size %g x %g", m, pr[2],
                   pr[3]);
    }
    if (M == 0) return FP_OK;
    int32_t* meta;
    double *params, *frames, *aligned = d_aligned;
    FP_WS(ctx, "video.meta", (size_t)M * FP_VE_META_LD * sizeof(int32_t), meta);
    FP_WS(ctx, "video.params", (size_t)M * FP_VE_PARAM_LD * sizeof(double), params);
    FP_WS(ctx, "video.frames", (size_t)M * Nmax * FP_VE_FRAME_LD * sizeof(double), frames);
    if (!aligned) FP_WS(ctx, "video.aligned", (size_t)M * Nmax * 3 * sizeof(double), aligned);
    hipStream_t s = (hipStream_t)stream;
    FP_HIP(hipMemcpyAsync(meta, h_meta, (size_t)M * FP_VE_META_LD * sizeof(int32_t), hipMemcpyHostToDevice, s));
    FP_HIP(hipMemcpyAsync(params, h_params, (size_t)M * FP_VE_PARAM_LD * sizeof(double), hipMemcpyHostToDevice, s));
    FP_HIP(hipStreamSynchronize(s));                       // the host tables are the caller's again when this entry returns
    return fp_video_errors_launch(d_est, d_gt, meta, params, M, Nmax, D, aligned, frames, d_per_offset, d_final, d_pairs, s);
}

// ---------------------------------------------------------------------------------------------
// BOP pose matching and recall counts (bop_score.hip).  Every table is device memory: the sizes are checked here, the contents by the
// caller on the tables' host twins (ops.bop_scores); the kernel skips a group whose row reaches outside the tables.
extern "C" int fp_bop_scores(fp_ctx* ctx, const double* d_err, const int32_t* d_groups, const uint8_t* d_gt_valid, const int32_t* d_gt_obj,
                             const int32_t* d_gt_scene, const double* d_th, int P, int Gr, int R, int T, int n_obj, int n_scene, int n_top,
                             int32_t* d_match, int32_t* d_tp_obj, int32_t* d_tp_scene, int32_t* d_tar_obj, int32_t* d_tar_scene,
                             void* stream) {
    FP_REQUIRE(ctx && d_th && d_tp_obj && d_tp_scene && d_tar_obj && d_tar_scene, "bop_scores: null argument");
    FP_REQUIRE(T >= 1 && T <= 65536, "bop_scores: T=%d thresholds (1..65536)", T);
    FP_REQUIRE(P >= 0 && Gr >= 0 && R >= 0, "bop_scores: P=%d errors, Gr=%d groups, R=%d ground truths (>= 0)", P, Gr, R);
    FP_REQUIRE(n_obj >= 1 && n_scene >= 1, "bop_scores: n_obj=%d, n_scene=%d (>= 1)", n_obj, n_scene);
    FP_REQUIRE((int64_t)Gr * T <= INT32_MAX && (int64_t)R * T <= INT32_MAX && (int64_t)n_obj * T <= INT32_MAX &&
                   (int64_t)n_scene * T <= INT32_MAX,
               "bop_scores: Gr=%d, R=%d, n_obj=%d, n_scene=%d times T=%d (each product below 2^31)", Gr, R, n_obj, n_scene, T);
    FP_REQUIRE(P == 0 || d_err, "bop_scores: null d_err with P=%d", P);
    FP_REQUIRE(Gr == 0 || d_groups, "bop_scores: null d_groups with Gr=%d", Gr);
    FP_REQUIRE(R == 0 || (d_gt_valid && d_gt_obj && d_gt_scene && d_match), "bop_scores: null ground-truth table or d_match with R=%d", R);
    return fp_bop_scores_launch(d_err, d_groups, d_gt_valid, d_gt_obj, d_gt_scene, d_th, P, Gr, R, T, n_obj, n_scene, n_top, d_match,
                                d_tp_obj, d_tp_scene, d_tar_obj, d_tar_scene, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// kernel-level entry points
// (the GEMM entries are the driver's own steps of tower_steps.h with the caller's leading dimensions; fp_ctx::gemm launches them)
extern "C" int fp_op_gemm(fp_ctx* ctx, const void* X, int ldx, const void* W, int ldw, void* Cc, int ldc, const void* bias,
                          const void* gamma, const void* resid, int ldr, int M, int N, int K, int epi, void* stream) {
    FP_REQUIRE(ctx && X && W && Cc && bias, "op_gemm: null argument");
    FP_REQUIRE(epi >= 0 && epi <= 2, "op_gemm: epi %d (0..2)", epi);
    GemmStep t((const bf16_t*)X, ldx, (const bf16_t*)W, K, (bf16_t*)Cc, ldc, (const bf16_t*)bias, M, N, epi == FP_EPI_BIAS_GELU);
    if (epi == FP_EPI_BIAS_LS_RES) t.residual((const bf16_t*)gamma, (const bf16_t*)resid, ldr);
    t.g.ldw = ldw;
    return t.run(ctx, (hipStream_t)stream);
}
extern "C" int fp_op_gemm_vt(fp_ctx* ctx, const void* X, int ldx, const void* W, int ldw, void* Vt, const void* bias, int M, int N,
                             int K, int npad, int heads, void* stream) {
    FP_REQUIRE(ctx && X && W && Vt, "op_gemm_vt: null argument");
    GemmStep t((const bf16_t*)X, ldx, (const bf16_t*)W, K, (bf16_t*)Vt, 8, (const bf16_t*)bias, M, N);
    t.transposed_v(npad, heads).g.ldw = ldw;
    return t.run(ctx, (hipStream_t)stream);
}
// LayerNorm folded into a linear layer (LN1 -> qkv, LN2 -> fc1):
// fold W' / (colsum, b') -> row statistics of X -> the LN-folded GEMM.  mode 0: bias, 1: bias + GELU, 2: transposed V store.
extern "C" int fp_op_ln_linear(fp_ctx* ctx, const void* X, int M, int K, const void* g_ln, const void* b_ln, float eps,
                               const void* W, int N, const void* bias, int mode, int npad, int heads, int n_scaled, float row_scale,
                               void* out, void* stream) {
    FP_REQUIRE(ctx && X && g_ln && b_ln && W && bias && out, "op_ln_linear: null argument");
    FP_REQUIRE(mode >= 0 && mode <= 2, "op_ln_linear: mode %d (0..2)", mode);
    hipStream_t s = (hipStream_t)stream;
    const bf16_t* Xb = (const bf16_t*)X;
    bf16_t* Wf;
    uint4* cb;
    LnStats st{nullptr, nullptr, nullptr, M, K, eps};
    int rc;
    FP_WS(ctx, "op.ln_wf", (size_t)N * K * 2, Wf);
    FP_WS(ctx, "op.ln_cb", (size_t)N * sizeof(uint4), cb);
    FP_WS(ctx, "op.ln_stat", (size_t)M * sizeof(uint4), st.stat);
    FP_WS(ctx, "op.ln_rstd", (size_t)M * sizeof(float), st.rstd);
    FP_REQUIRE(n_scaled >= 0 && n_scaled <= N, "op_ln_linear: n_scaled %d outside [0, N]", n_scaled);
    if ((rc = fp_ln_fold((const bf16_t*)W, (const bf16_t*)g_ln, (const bf16_t*)b_ln, (const bf16_t*)bias, Wf, cb, N, K, n_scaled, row_scale, s))) return rc;
    if ((rc = st.ready(Xb, N, s))) return rc;
    GemmStep t(Xb, K, Wf, K, (bf16_t*)out, N, (const bf16_t*)bias, M, N, mode == 1);
    if (mode == 2) t.transposed_v(npad, heads);
    if ((rc = st.attach(t, cb))) return rc;
    return t.run(ctx, s);
}
// LayerScale + residual GEMM that also emits the row statistics of its OUTPUT (what the next LN-folded GEMM consumes):
// d_stat f32 [M,2] = (mean, rstd) of the bf16 rows of C, from the epilogue's per-64-column partial sums.
extern "C" int fp_op_gemm_stats(fp_ctx* ctx, const void* X, int ldx, const void* W, int ldw, void* Cc, int ldc, const void* bias,
                                const void* gamma, const void* resid, int ldr, int M, int N, int K, float eps, float* d_stat,
                                void* stream) {
    FP_REQUIRE(ctx && X && W && Cc && bias && gamma && resid && d_stat, "op_gemm_stats: null argument");
    hipStream_t s = (hipStream_t)stream;
    LnStats st{nullptr, nullptr, nullptr, M, N, eps};
    int rc;
    FP_WS(ctx, "op.ln_part", (size_t)M * (N / 64) * sizeof(float2), st.part);
    FP_WS(ctx, "op.ln_stat", (size_t)M * sizeof(uint4), st.stat);
    FP_WS(ctx, "op.ln_rstd", (size_t)M * sizeof(float), st.rstd);
    GemmStep t((const bf16_t*)X, ldx, (const bf16_t*)W, K, (bf16_t*)Cc, ldc, (const bf16_t*)bias, M, N);
    t.residual((const bf16_t*)gamma, (const bf16_t*)resid, ldr, st.part).g.ldw = ldw;
    if ((rc = t.run(ctx, s))) return rc;
    if ((rc = fp_stats_finalize(st.part, st.stat, st.rstd, M, N, eps, s))) return rc;   // no consumer: the records themselves are the result
    // d_stat [M,6] = the row record's 4 words {sh|sl, sh|-mh, -ml|-mh, 0} reinterpreted as floats are NOT meaningful: hand back the raw
    // record words (4 x u32 as f32 bit patterns) followed by (rstd, 0); the Python wrapper decodes mean = -(mh + ml), sigma = sh + sl
    FP_HIP(hipMemcpy2DAsync(d_stat, 24, st.stat, 16, 16, M, hipMemcpyDeviceToDevice, s));
    FP_HIP(hipMemcpy2DAsync(d_stat + 4, 24, st.rstd, 4, 4, M, hipMemcpyDeviceToDevice, s));
    return FP_OK;
}
// Patch-embed GEMM (FP_EPI_PATCH): row m = b * P + p of X lands in row b * npad + tok_off + p of the token
// buffer C as bf16(bf16(acc + bias) + pos[p]); the other rows of C (cls, registers, pad) are not touched.
extern "C" int fp_op_gemm_patch(fp_ctx* ctx, const void* X, int ldx, const void* W, int ldw, void* Cc, int ldc, const void* bias,
                                const void* pos, int M, int N, int K, int P, int npad, int tok_off, void* stream) {
    FP_REQUIRE(ctx && X && W && Cc && bias && pos, "op_gemm_patch: null argument");
    FP_REQUIRE(P > 0 && M > 0 && M % P == 0 && tok_off >= 0 && tok_off + P <= npad && ldc >= N,
               "op_gemm_patch: M=%d P=%d npad=%d tok_off=%d (M %% P == 0, tok_off + P <= npad, ldc >= N)", M, P, npad, tok_off);
    GemmStep t((const bf16_t*)X, ldx, (const bf16_t*)W, K, (bf16_t*)Cc, ldc, (const bf16_t*)bias, M, N);
    t.patch_embed((const bf16_t*)pos, P, npad, tok_off).g.ldw = ldw;
    return t.run(ctx, (hipStream_t)stream);
}
// Producer -> consumer pair of the folded LayerNorm (proj -> fc1, fc2 -> qk of the next block):
//   producer  Y[M,D] = resid + gamma * (X1 W1^T + b1) with FP_EPI_LS_RES_STATS, writing the partial row statistics [D/64][M];
//   consumer  out[M,N2] (ldo) = LN(Y) W2^T + b2 (mode 0) or its GELU (mode 1) through the LN-folded GEMM on the raw rows of Y.
// route 0: fp_stats_finalize, then the consumer reads finished row records.  route 1: the consumer launch carries the partial sums
// (LnStats::attach with the sums pending) and fp_gemm_bf16 decides who finalises them — the small tiers' prologue, each part of a row
// split, or the finalisation kernel in front of the big tier (the forward never hands the sums to a big-tier launch: LnStats::ready
// finalises up front there; route 1 on such a shape pins the plan's finalize_first, which is the same kernel with the same arguments
// as route 0).  The row records (16 bytes each)
// and rstd are poisoned with 0xFF bytes first and copied out afterwards: d_mfrag [M,4] u32, d_rstd [M] f32.
extern "C" int fp_op_ln_chain(fp_ctx* ctx, const void* X1, int K1, const void* W1, const void* b1, const void* gamma, const void* resid,
                              void* Y, int M, int D, const void* g_ln, const void* b_ln, float eps, const void* W2, int N2,
                              const void* b2, int mode, int n_scaled, float row_scale, int route, void* out, int ldo, void* d_mfrag,
                              float* d_rstd, void* stream) {
    FP_REQUIRE(ctx && X1 && W1 && b1 && gamma && resid && Y && g_ln && b_ln && W2 && b2 && out && d_mfrag && d_rstd, "op_ln_chain: null argument");
    FP_REQUIRE((mode == 0 || mode == 1) && (route == 0 || route == 1), "op_ln_chain: mode %d (0..1), route %d (0..1)", mode, route);
    FP_REQUIRE(M > 0 && D > 0 && D % 64 == 0 && ldo >= N2 && n_scaled >= 0 && n_scaled <= N2, "op_ln_chain: M=%d D=%d N2=%d ldo=%d n_scaled=%d", M, D, N2, ldo, n_scaled);
    hipStream_t s = (hipStream_t)stream;
    bf16_t* Wf;
    uint4* cb;
    LnStats st{nullptr, nullptr, nullptr, M, D, eps};
    int rc;
    FP_WS(ctx, "op.ln_wf", (size_t)N2 * D * 2, Wf);
    FP_WS(ctx, "op.ln_cb", (size_t)N2 * sizeof(uint4), cb);
    FP_WS(ctx, "op.ln_stat", (size_t)M * sizeof(uint4), st.stat);
    FP_WS(ctx, "op.ln_rstd", (size_t)M * sizeof(float), st.rstd);
    FP_WS(ctx, "op.ln_part", (size_t)M * (D / 64) * sizeof(float2), st.part);
    FP_HIP(hipMemsetAsync(st.stat, 0xFF, (size_t)M * sizeof(uint4), s));
    FP_HIP(hipMemsetAsync(st.rstd, 0xFF, (size_t)M * sizeof(float), s));
    if ((rc = fp_ln_fold((const bf16_t*)W2, (const bf16_t*)g_ln, (const bf16_t*)b_ln, (const bf16_t*)b2, Wf, cb, N2, D, n_scaled, row_scale, s))) return rc;
    GemmStep prod((const bf16_t*)X1, K1, (const bf16_t*)W1, K1, (bf16_t*)Y, D, (const bf16_t*)b1, M, D);
    if ((rc = prod.residual((const bf16_t*)gamma, (const bf16_t*)resid, D, st.part).run(ctx, s))) return rc;
    if (route == 0 && (rc = fp_stats_finalize(st.part, st.stat, st.rstd, M, D, eps, s))) return rc;
    st.pending = route == 1;
    GemmStep cons((const bf16_t*)Y, D, Wf, D, (bf16_t*)out, ldo, (const bf16_t*)b2, M, N2, mode == 1);
    if ((rc = st.attach(cons, cb))) return rc;
    if ((rc = cons.run(ctx, s))) return rc;
    FP_HIP(hipMemcpyAsync(d_mfrag, st.stat, (size_t)M * sizeof(uint4), hipMemcpyDeviceToDevice, s));
    FP_HIP(hipMemcpyAsync(d_rstd, st.rstd, (size_t)M * sizeof(float), hipMemcpyDeviceToDevice, s));
    return FP_OK;
}
// One LN-folded consumer on row records the CALLER supplies (d_mfrag u32 [M,4], d_rstd f32 [M]: what fp_op_ln_chain, fp_op_row_stats or
// fp_op_stats_finalize returned) — the second consumer of a set of records, the way fp_vit_forward's transposed-V launch reads the records
// the qk launch made out of fc2's sums.  fold W' / (colsum, b') -> the LN-folded GEMM; mode 0: bias, 1: bias + GELU, 2: transposed V
// store (ldo unused).  Nothing is recomputed from the rows of X.
extern "C" int fp_op_ln_consume(fp_ctx* ctx, const void* X, int M, int K, const void* g_ln, const void* b_ln, const void* W, int N,
                                const void* bias, int mode, int npad, int heads, int n_scaled, float row_scale, const void* d_mfrag,
                                const float* d_rstd, void* out, int ldo, void* stream) {
    FP_REQUIRE(ctx && X && g_ln && b_ln && W && bias && d_mfrag && d_rstd && out, "op_ln_consume: null argument");
    FP_REQUIRE(mode >= 0 && mode <= 2, "op_ln_consume: mode %d (0..2)", mode);
    FP_REQUIRE(M > 0 && K > 0 && K % 64 == 0 && n_scaled >= 0 && n_scaled <= N && (mode == 2 || ldo >= N), "op_ln_consume: M=%d K=%d N=%d ldo=%d n_scaled=%d",
               M, K, N, ldo, n_scaled);
    FP_REQUIRE(mode != 2 || (npad > 0 && M % npad == 0 && heads > 0 && N == heads * 64), "op_ln_consume: M=%d N=%d npad=%d heads=%d (M %% npad == 0, N == 64 heads)",
               M, N, npad, heads);
    hipStream_t s = (hipStream_t)stream;
    bf16_t* Wf;
    uint4* cb;
    // the records are the caller's: eps went into them, no sums are pending
    LnStats st{(uint4*)d_mfrag, (float*)d_rstd, nullptr, M, K, 0.0f};
    int rc;
    FP_WS(ctx, "op.ln_wf", (size_t)N * K * 2, Wf);
    FP_WS(ctx, "op.ln_cb", (size_t)N * sizeof(uint4), cb);
    if ((rc = fp_ln_fold((const bf16_t*)W, (const bf16_t*)g_ln, (const bf16_t*)b_ln, (const bf16_t*)bias, Wf, cb, N, K, n_scaled, row_scale, s))) return rc;
    GemmStep t((const bf16_t*)X, K, Wf, K, (bf16_t*)out, ldo, (const bf16_t*)bias, M, N, mode == 1);
    if (mode == 2) t.transposed_v(npad, heads);
    if ((rc = st.attach(t, cb))) return rc;
    return t.run(ctx, s);
}
// Copies the first `bytes` bytes of the context workspace `name` ("vit.x", "clip.qkv", ...) to the host, behind everything the device has
// been given: what a tower left in its buffers, for the tests that replay a forward step by step.
extern "C" int fp_op_workspace_read(fp_ctx* ctx, const char* name, void* host, size_t bytes) {
    FP_REQUIRE(ctx && name && host, "op_workspace_read: null argument");
    auto it = ctx->bufs.find(name);
    FP_REQUIRE(it != ctx->bufs.end() && it->second.bytes >= bytes, "op_workspace_read: no workspace '%s' of at least %zu bytes", name, bytes);
    FP_HIP(hipDeviceSynchronize());
    FP_HIP(hipMemcpy(host, it->second.p, bytes, hipMemcpyDeviceToHost));
    return FP_OK;
}
// The plan fp_ctx::gemm would execute for a launch of this shape on this device, with this context's gemm_row_split, in words
// (gemm_plan.h plan_text): nothing is launched.  What the tests of the tile tiers hold their case tables to.
extern "C" int fp_op_gemm_plan(fp_ctx* ctx, int M, int N, int K, int epi, int ldx, int ldw, int ln_part, char* out, size_t out_bytes) {
    FP_REQUIRE(ctx && out && out_bytes > 0, "op_gemm_plan: null argument");
    FP_REQUIRE(M > 0 && N > 0 && K > 0 && epi >= FP_EPI_BIAS && epi <= FP_EPI_LS_RES_STATS, "op_gemm_plan: M=%d N=%d K=%d epi=%d", M, N, K, epi);
    const fp_plan::Plan plan = fp_gemm_plan({M, N, K, epi, ldx, ldw, ln_part != 0, ctx->opt_row_split == 0});
    const int n = fp_plan::plan_text(plan, out, out_bytes);
    FP_REQUIRE(n >= 0 && (size_t)n < out_bytes, "op_gemm_plan: the text needs %d bytes", n + 1);
    return FP_OK;
}
// y = bf16(gelu_erf(x)) elementwise with the direct fp32 expression — the DEFINITION the fc1 epilogue's table is filled from; the
// tests compare the table-GELU GEMM against it on all 65 536 bf16 inputs
extern "C" int fp_op_gelu(const void* x, void* y, size_t n, void* stream) {
    FP_REQUIRE(x && y, "op_gelu: null argument");
    return fp_gemm_gelu_direct((const bf16_t*)x, (bf16_t*)y, n, (hipStream_t)stream);
}
extern "C" int fp_op_attention(const void* QK, int ldqk, const void* Vt, void* O, int ldo, int B, int H, int n_tok,
                               int npad, int q_prescaled, void* stream) {
    return fp_attention_fwd((const bf16_t*)QK, ldqk, (const bf16_t*)Vt, (bf16_t*)O, ldo, B, H, n_tok, npad, q_prescaled != 0,
                            (hipStream_t)stream);
}
extern "C" int fp_op_attention_hd(const void* QKV, int ldqkv, void* O, int ldo, int B, int heads, int head_dim, int n_tok, int npad,
                                  float scale, void* stream) {
    return fp_attention_hd_fwd((const bf16_t*)QKV, ldqkv, (bf16_t*)O, ldo, B, heads, head_dim, n_tok, npad, scale, (hipStream_t)stream);
}
extern "C" int fp_op_attention_causal(const void* QKV, int ldqkv, void* O, int ldo, int B, int heads, int head_dim, int n_tok, int npad,
                                      float scale, void* stream) {
    return fp_attention_causal_fwd((const bf16_t*)QKV, ldqkv, (bf16_t*)O, ldo, B, heads, head_dim, n_tok, npad, scale, (hipStream_t)stream);
}
extern "C" int fp_knn_l2(fp_ctx* ctx, const float* d_table, int N, int E, const float* d_queries, int Q, int k, int32_t* d_out_idx,
                         float* d_out_d2, void* stream) {
    FP_REQUIRE(ctx, "knn_l2: null context");
    FP_REQUIRE(N > 0 && Q > 0, "knn_l2: bad shape N=%d Q=%d", N, Q);
    float* ws = nullptr;      // all Q x N squared distances: O(Q * N) floats of context workspace (a table of a few thousand rows)
    FP_WS(ctx, "knn.d2", (size_t)Q * N * sizeof(float), ws);
    return fp_knn_l2_launch(d_table, N, E, d_queries, Q, k, ws, d_out_idx, d_out_d2, (hipStream_t)stream);
}
extern "C" int fp_op_im2col_norm(const void* img, void* A, int B, int H, int W, int ps, int KP, void* stream) {
    FP_REQUIRE(img && A && B > 0, "op_im2col_norm: null argument / empty batch");
    return fp_im2col_norm_ms((const bf16_t*)img, (bf16_t*)A, B, H, W, ps, KP, FP_IMAGENET_MEAN, FP_IMAGENET_SD, (hipStream_t)stream);
}
extern "C" int fp_op_layernorm(const void* X, void* Y, const void* g, const void* b, int rows, int D, float eps,
                               void* stream) {
    if (rows == 0) return FP_OK;   // an empty tensor has no address
    FP_REQUIRE(X && Y && g && b, "op_layernorm: null argument");
    return fp_layernorm((const bf16_t*)X, (bf16_t*)Y, (const bf16_t*)g, (const bf16_t*)b, rows, D, eps, 0, 0, 0,
                        (hipStream_t)stream);
}
// The helper kernels of vit_misc.hip one at a time: argument checks, then the launcher the towers call.  An empty call (no rows, no
// elements) returns before any launcher; everything the kernels cannot do is refused by the launchers' own checks, before a launch.
extern "C" int fp_op_layernorm_rows(const void* X, void* Y, const void* g, const void* b, int rows, int D, float eps, int rows_per_b,
                                    int in_stride_b, int in_off, int l2_normalize, void* stream) {
    FP_REQUIRE(rows >= 0 && D >= 0, "op_layernorm_rows: rows=%d, D=%d", rows, D);
    if (rows == 0 || D == 0) return FP_OK;
    FP_REQUIRE(X && Y && g && b, "op_layernorm_rows: null argument");
    FP_REQUIRE(rows_per_b <= 0 || (in_stride_b >= 0 && in_off >= 0), "op_layernorm_rows: in_stride_b=%d, in_off=%d (>= 0)", in_stride_b, in_off);
    return fp_layernorm((const bf16_t*)X, (bf16_t*)Y, (const bf16_t*)g, (const bf16_t*)b, rows, D, eps, rows_per_b, in_stride_b, in_off,
                        (hipStream_t)stream, l2_normalize != 0);
}
extern "C" int fp_op_posembed_aa(const void* src, void* dst, int G, int gh, int gw, int D, void* stream) {
    FP_REQUIRE(G >= 0 && gh >= 0 && gw >= 0 && D >= 0, "op_posembed_aa: G=%d, gh=%d, gw=%d, D=%d", G, gh, gw, D);
    if (gh == 0 || gw == 0 || D == 0) return FP_OK;
    FP_REQUIRE(src && dst, "op_posembed_aa: null argument");
    return fp_posembed_aa((const bf16_t*)src, (bf16_t*)dst, G, gh, gw, D, (hipStream_t)stream);
}
extern "C" int fp_op_token_init(void* X, const void* cls, const void* pos0, const void* reg, int nreg, int B, int n_tok, int npad, int D,
                                void* stream) {
    FP_REQUIRE(B >= 0 && B <= 65535 && D >= 0, "op_token_init: B=%d (0..65535), D=%d", B, D);
    FP_REQUIRE(nreg >= 0 && n_tok >= 1 + nreg && npad >= n_tok, "op_token_init: nreg=%d, n_tok=%d, npad=%d (1 + nreg <= n_tok <= npad)", nreg, n_tok,
               npad);
    if (B == 0 || D == 0) return FP_OK;
    FP_REQUIRE(X && cls && pos0 && (reg || nreg == 0), "op_token_init: null argument");
    FP_REQUIRE((long long)(1 + nreg + npad - n_tok) * D <= INT32_MAX, "op_token_init: %d rows of %d elements", 1 + nreg + npad - n_tok, D);
    return fp_token_init((bf16_t*)X, (const bf16_t*)cls, (const bf16_t*)pos0, (const bf16_t*)reg, nreg, B, n_tok, npad, D, (hipStream_t)stream);
}
extern "C" int fp_op_row_stats(const void* X, int rows, int D, float eps, void* d_rec, float* d_rstd, void* stream) {
    FP_REQUIRE(rows >= 0 && D >= 0, "op_row_stats: rows=%d, D=%d", rows, D);
    if (rows == 0) return FP_OK;
    FP_REQUIRE(X && d_rec && d_rstd, "op_row_stats: null argument");
    FP_REQUIRE(D > 0, "op_row_stats: D=%d", D);
    return fp_row_stats((const bf16_t*)X, (uint4*)d_rec, d_rstd, rows, D, eps, (hipStream_t)stream);
}
extern "C" int fp_op_stats_finalize(const void* part, int rows, int D, float eps, int part_ld, void* d_rec, float* d_rstd, void* stream) {
    FP_REQUIRE(rows >= 0 && D >= 0, "op_stats_finalize: rows=%d, D=%d", rows, D);
    if (rows == 0) return FP_OK;
    FP_REQUIRE(part && d_rec && d_rstd, "op_stats_finalize: null argument");
    FP_REQUIRE(D > 0 && (part_ld == 0 || part_ld >= rows), "op_stats_finalize: D=%d, part_ld=%d (0 or >= rows=%d)", D, part_ld, rows);
    return fp_stats_finalize((const float2*)part, (uint4*)d_rec, d_rstd, rows, D, eps, (hipStream_t)stream, part_ld);
}
extern "C" int fp_op_ln_fold(const void* W, const void* gamma, const void* beta, const void* bias, int N, int K, int n_scaled, float row_scale,
                             void* Wf, void* d_cb, void* stream) {
    FP_REQUIRE(N >= 0 && K >= 0, "op_ln_fold: N=%d, K=%d", N, K);
    if (N == 0) return FP_OK;
    FP_REQUIRE(K > 0 && n_scaled >= 0 && n_scaled <= N, "op_ln_fold: K=%d, n_scaled=%d outside [0, N=%d]", K, n_scaled, N);
    return fp_ln_fold((const bf16_t*)W, (const bf16_t*)gamma, (const bf16_t*)beta, (const bf16_t*)bias, (bf16_t*)Wf, (uint4*)d_cb, N, K, n_scaled,
                      row_scale, (hipStream_t)stream);
}
extern "C" int fp_op_transpose(const void* src, void* dst, int rows, int cols, void* stream) {
    FP_REQUIRE(rows >= 0 && cols >= 0, "op_transpose: rows=%d, cols=%d", rows, cols);
    if (rows == 0 || cols == 0) return FP_OK;
    FP_REQUIRE(src && dst, "op_transpose: null argument");
    return fp_transpose_bf16((const bf16_t*)src, (bf16_t*)dst, rows, cols, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// timers
struct FpTimer { hipEvent_t a, b; };
extern "C" int fp_timer_create(void** out) {
    FP_REQUIRE(out, "timer_create: null");
    FpTimer* t = new FpTimer();
    FP_HIP(hipEventCreate(&t->a));
    FP_HIP(hipEventCreate(&t->b));
    *out = t;
    return FP_OK;
}
extern "C" int fp_timer_start(void* t, void* s) { FP_HIP(hipEventRecord(((FpTimer*)t)->a, (hipStream_t)s)); return FP_OK; }
extern "C" int fp_timer_stop(void* t, void* s) { FP_HIP(hipEventRecord(((FpTimer*)t)->b, (hipStream_t)s)); return FP_OK; }
extern "C" int fp_timer_elapsed_ms(void* t, float* ms) {
    FP_HIP(hipEventSynchronize(((FpTimer*)t)->b));
    FP_HIP(hipEventElapsedTime(ms, ((FpTimer*)t)->a, ((FpTimer*)t)->b));
    return FP_OK;
}
extern "C" int fp_timer_destroy(void* t) {
    if (!t) return FP_OK;
    (void)hipEventDestroy(((FpTimer*)t)->a);
    (void)hipEventDestroy(((FpTimer*)t)->b);
    delete (FpTimer*)t;
    return FP_OK;
}

// ---- the built-in point tracker (lk_track.hip) ------------------------------------------------------------------------------------------
#define FP_LK_MAX_QUERIES (1 << 20)
static int lk_check_sizes(const char* what, int T, int H, int W, int levels, int radius) {
    FP_REQUIRE(T >= 1 && T <= 65535, "%s: T=%d frames (1..65535)", what, T);
    FP_REQUIRE(H >= 1 && W >= 1 && H <= FP_LK_MAX_SIDE && W <= FP_LK_MAX_SIDE, "%s: %d x %d frames (1..%d per side)", what, H, W, FP_LK_MAX_SIDE);
    FP_REQUIRE((long long)T * H * W <= (1ll << 30), "%s: T * H * W = %lld pixels (at most 2^30 per call)", what, (long long)T * H * W);
    FP_REQUIRE(radius >= 1 && radius <= FP_LK_MAX_RADIUS, "%s: radius=%d (1..%d)", what, radius, FP_LK_MAX_RADIUS);
    FP_REQUIRE(levels >= 1 && levels <= FP_LK_MAX_LEVELS, "%s: levels=%d (1..%d)", what, levels, FP_LK_MAX_LEVELS);
    return FP_OK;
}

extern "C" int fp_lk_pyramid(fp_ctx* ctx, const uint8_t* d_frames, int T, int H, int W, int levels, int radius, float* d_pyramid, void* stream) {
    FP_REQUIRE(ctx && d_frames && d_pyramid, "lk_pyramid: null argument");
    if (int rc = lk_check_sizes("lk_pyramid", T, H, W, levels, radius)) return rc;
    LkPyramid P;
    lk_pyramid_layout(T, H, W, levels, radius, P);
    return fp_lk_pyramid_launch(d_frames, P, d_pyramid, (hipStream_t)stream);
}

extern "C" int fp_lk_track(fp_ctx* ctx, const float* d_pyramid, int T, int H, int W, int levels, const float* d_queries, int N, int radius,
                           int iters, float fb_thresh, float min_eig, float max_residual, float* d_tracks, uint8_t* d_vis, float* d_diag,
                           void* stream) {
    if (int rc = lk_check_sizes("lk_track", T, H, W, levels, radius)) return rc;
    FP_REQUIRE(N >= 0 && N <= FP_LK_MAX_QUERIES, "lk_track: N=%d queries (0..2^20)", N);
    FP_REQUIRE(ctx && d_pyramid && (N == 0 || (d_queries && d_tracks && d_vis && d_diag)), "lk_track: null argument");
    FP_REQUIRE(iters >= 1 && iters <= FP_LK_MAX_ITERS, "lk_track: iters=%d (1..%d)", iters, FP_LK_MAX_ITERS);
    LkPyramid P;
    lk_pyramid_layout(T, H, W, levels, radius, P);
    double* state = nullptr;                       // chain positions in fp64 (the float32 tracks are their rounded copies)
    if (N > 0) FP_WS(ctx, "lk_state", (size_t)T * N * 2 * sizeof(double), state);
    return fp_lk_track_launch(P, d_pyramid, d_queries, N, radius, iters, fb_thresh, min_eig, max_residual, state, d_tracks, d_vis, d_diag,
                              (hipStream_t)stream);
}
