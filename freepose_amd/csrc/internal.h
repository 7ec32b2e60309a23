// internal launcher prototypes shared by the C-ABI translation units
#pragma once
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "common.h"
#include "gemm_bf16.h"

struct fp_ctx {
    int device = 0;
    // named, grow-only workspaces (device memory).  One context per thread/GPU, no locking.
    struct Buf { void* p = nullptr; size_t bytes = 0; };
    std::map<std::string, Buf> bufs;
    int get(const char* name, size_t bytes, void** out);
    template <class T> int ws(const char* name, size_t bytes, T*& out) { return get(name, bytes, (void**)&out); }   // typed get
    // optional RCCL communicator (comm.hip: fp_comm_init); null = single rank
    void* comm = nullptr;
    int comm_rank = 0, comm_size = 1;
    // run-time options of THIS context (fp_ctx_set_option); -1 = built-in default
    int opt_ln_fused = -1;       // 1 (default): LayerNorm 1 / 2 folded into the qkv / fc1 GEMMs of fp_vit_forward; 0: separate kernel
    int opt_raster_tiled = -1;   // default: by triangle count / image size; 1 / 0 force the LDS-tiled / global-buffer strategy
    int opt_comm_timeout_s = -1; // seconds fp_comm_init waits for the rendezvous of all ranks before it fails (default 180)
    int opt_row_split = -1;      // 1 (default): GEMM launches between the tile tiers are split by rows; 0: never
    // scratch of the balanced GEMM tier (gemm_bf16.h FpGemmArgs::sk_*): fp32 partial tiles + zero-initialised arrival counters.  The tier
    // is compiled into the lab build only: the product never allocates these and every launch goes out with sk_mode = 1 (never), so every
    // tier gives the same bits for a row
    float* sk_ws = nullptr;
    int* sk_cnt = nullptr;
    static constexpr size_t SK_WS_BYTES = (size_t)64 << 20;
    static constexpr int SK_CNT_N = 16384;
#ifdef FP_LAB
    int opt_stream_k = -1;       // lab option "gemm_stream_k": 0 = never lend the scratch; else launches below the big tier may run on the
                                 // balanced tier when gemm_sk asks for it (K slices summed in K order: results depend on the launch size)
    int sk_scratch(FpGemmArgs& g, hipStream_t s);   // lends the scratch to a launch (allocates on first use)
#endif
    // THE launch path of every bf16 GEMM of the library: applies the context's options (gemm_row_split -> no_split), in the lab build lends
    // the balanced tier its scratch, and calls fp_gemm_bf16
    int gemm(FpGemmArgs& g, int epi, hipStream_t s);
    int* ffa_arrive = nullptr;   // per-crop arrival counters of the fused FFA launch (zero between calls: the last arriver resets its own)
    size_t total() const;
    void release();
};
// p = the context's workspace `name` of at least `bytes` (grown if needed), or return the error
#define FP_WS(ctx, name, bytes, p)                                   \
    do {                                                             \
        if (int rc__ = (ctx)->ws(name, bytes, p)) return rc__;       \
    } while (0)

// attention.hip
// log2(e) / sqrt(head_dim = 64): what the softmax multiplies q k^T by before exp2 — or what the q rows of the folded qkv weights carry
constexpr float FP_ATTN_QSCALE = 1.4426950408889634f / 8.0f;
int fp_attention_fwd(const bf16_t* QK, int ldqk, const bf16_t* Vt, bf16_t* O, int ldo, int B, int H, int n_tok,
                     int npad, bool q_prescaled, hipStream_t stream);
// attention_hd.hip: any head dimension (multiple of 8 up to 128) on the plain [q | k | v] output of one bias GEMM
int fp_attention_hd_fwd(const bf16_t* QKV, int ldqkv, bf16_t* O, int ldo, int B, int heads, int head_dim, int n_tok, int npad, float scale,
                        hipStream_t stream);
// the same kernel, layout and contract, query t attending to keys 0 .. t (the CLIP text tower)
int fp_attention_causal_fwd(const bf16_t* QKV, int ldqkv, bf16_t* O, int ldo, int B, int heads, int head_dim, int n_tok, int npad, float scale,
                            hipStream_t stream);
// vit_misc.hip
// torchvision Normalize of the DINOv2 inputs (ImageNet); fp_im2col_norm_ms rounds mean / std to bf16 like its tensors in the image dtype
constexpr float FP_IMAGENET_MEAN[3] = {0.485f, 0.456f, 0.406f}, FP_IMAGENET_SD[3] = {0.229f, 0.224f, 0.225f};
int fp_im2col_norm_ms(const bf16_t* img, bf16_t* A, int B, int H, int W, int ps, int KP, const float* mean, const float* sd, hipStream_t s);
int fp_token_init(bf16_t* X, const bf16_t* cls, const bf16_t* pos0, const bf16_t* reg, int nreg, int B, int n_tok,
                  int npad, int D, hipStream_t s);
int fp_layernorm(const bf16_t* X, bf16_t* Y, const bf16_t* gamma, const bf16_t* beta, int rows, int D, float eps,
                 int rows_per_b, int in_stride_b, int in_off, hipStream_t s, int l2_normalize = 0);
int fp_posembed_aa(const bf16_t* src, bf16_t* dst, int G, int gh, int gw, int D, hipStream_t s);
int fp_ffa_pool(const bf16_t* feats, const uint8_t* mask, bf16_t* out, float* out_f32, int B, int P, int D, int gh,
                int gw, int cell, uint8_t* pm_scratch, hipStream_t s, bf16_t* out_norm = nullptr, int* arrive = nullptr);
int fp_l2norm_rows(const bf16_t* X, bf16_t* Y, int rows, int D, hipStream_t s);
int fp_transpose_bf16(const bf16_t* src, bf16_t* dst, int rows, int cols, hipStream_t s);   // dst [cols, rows] = src [rows, cols]^T
// LayerNorm folded into the consuming GEMM (gemm_bf16.h FP_EPI_LN_*): row statistics and the one-off weight fold
int fp_row_stats(const bf16_t* X, uint4* mfrag, float* rstd, int rows, int D, float eps, hipStream_t s);
int fp_stats_finalize(const float2* part, uint4* mfrag, float* rstd, int rows, int D, float eps, hipStream_t s, int part_ld = 0);   // part_ld: row stride of part (0 = rows)
int fp_ln_fold(const bf16_t* W, const bf16_t* gamma, const bf16_t* beta, const bf16_t* bias, bf16_t* Wf, uint4* cfrag, int N, int K,
               int n_scaled, float row_scale, hipStream_t s);
// retrieval.hip
int fp_cast_f32_bf16(const float* x, bf16_t* y, size_t n, hipStream_t s);
int fp_bank_scan(const bf16_t* bank, const bf16_t* queries, uint16_t* keys, int ldk, int N, int D, int Q, hipStream_t s);
int fp_topk_select(const uint16_t* keys, int ldk, int N, int Q, int k, int idx_offset, float* out_scores, int* out_idx,
                   hipStream_t s);
int fp_topk_merge_launch(const float* cs, const int* ci, int Q, int C, int k, float* out_scores, int* out_idx,
                         hipStream_t s);
int fp_rerank_views_launch(const bf16_t* views, const int* offsets, const int* cand, const bf16_t* queries, float* out,
                           int Q, int C, int D, int k, hipStream_t s);
int fp_template_score_launch(const bf16_t* tmpl, const bf16_t* qn, const float* weights, float* dots, float* scores,
                             int T, int P, int D, int templates_normalised, hipStream_t s);
int fp_knn_l2_launch(const float* table, int N, int E, const float* queries, int Q, int k, float* d2_ws, int* out_idx, float* out_d2,
                     hipStream_t s);
// eval.hip: pose-error evaluation (chamfer / chamfer_proj, CUS / VSD pixel counts)
#define FP_EVAL_XF_LD 40      // doubles per pair in fp_chamfer's d_xf
#define FP_EVAL_TABLE_LD 8    // ints per pair in fp_chamfer's d_table
#define FP_EVAL_MAX_TAUS 16   // misalignment tolerances counted in one pass of fp_depth_compare
int fp_chamfer_chunks(int max_n);   // per-block partial sums per (pair, direction)
int fp_chamfer_launch(const double* pts, int n_pts, const int* table, const double* xf, int B, int max_n, int ws_pts, int projected,
                      float* ws, double* slots, double* out, hipStream_t s);
int fp_depth_compare_launch(const float* d_est, const float* d_gt, int B, int Hh, int W, const float* d_test, int n_img, const int* img_idx,
                            const double* params, const double* taus, int n_tau, int* out, hipStream_t s);
// scale.hip: connected components and the depth-map object scale (scale_core.h holds the host-checkable index arithmetic)
struct FpScaleWs {                 // scratch of fp_depthmap_scale_launch, all from the context's workspace
    int* uf;                       // [n,H,W] union-find labels, later the survivor lists
    int* labels;                   // [n,H,W] 1 + root, 0 = background
    int* area;                     // [n,H,W] pixel count on every root
    uint8_t* d2;                   // [n,H,W] capped squared distance inside the chosen component
    uint8_t* kflag;                // [n,H,W] kept flags of the survivors
    unsigned long long* best;      // [n] (area << 32 | ~root) of the chosen component
    int* cnt;                      // [n,8] survivors per radius of the erosion chain
};
// area may be null (labels only)
int fp_label_launch(const uint8_t* masks, int n, int H, int W, int connectivity, int* uf, int* labels, int* area, hipStream_t s);
int fp_depthmap_scale_launch(const double* depth, const uint8_t* masks, int n, int H, int W, double fx, double fy, double cx, double cy,
                             double erosion_radius, double std_factor, int min_vertices, int align, const FpScaleWs& ws, double* scale,
                             int* info, uint8_t* keep, hipStream_t s);
// refine.hip: TrackingRefiner correspondences and pose from tracks (pnp_core.h holds the host-checkable dense phases)
int fp_patch_points_launch(const double* samples, int S, const double* Tm, const double* Km, const int* cells, const int* ncells, int B, int C,
                           double patch, double* ws, int* out, hipStream_t s);   // ws: B * 4 * S doubles
int fp_pnp_epnp_launch(const double* pts3d, const double* pts2d, const uint8_t* vis, const double* K9, int B, int N, double* out,
                       hipStream_t s);
// video_eval.hip: video velocity errors (video_eval_core.h holds the host-checkable arithmetic).  meta / params are the device copies of
// fp_video_errors' host tables; aligned [M,Nmax,3], frames [M,Nmax,FP_VE_FRAME_LD]; pairs_out may be null
int fp_video_errors_launch(const double* est, const double* gt, const int* meta, const double* params, int M, int Nmax, int D,
                           double* aligned, double* frames, double* per_offset, double* final_out, double* pairs_out, hipStream_t s);
// bop_score.hip: BOP pose matching and recall counts for all thresholds at once (bop_score_core.h holds the host-checkable steps)
int fp_bop_scores_launch(const double* err, const int32_t* groups, const uint8_t* gt_valid, const int32_t* gt_obj, const int32_t* gt_scene,
                         const double* th, int P, int Gr, int R, int T, int n_obj, int n_scene, int n_top, int32_t* match, int32_t* tp_obj,
                         int32_t* tp_scene, int32_t* tar_obj, int32_t* tar_scene, hipStream_t s);
// gt_info.hip: ground-truth visibility / masks / boxes per instance and model diameters (gt_info_core.h holds the host-checkable arithmetic)
int fp_gt_visibility_launch(const float* d_gt, int B, int Hr, int Wr, int ox, int oy, const float* d_test, int n_img, int H, int W,
                            const int* img_idx, const double* params, uint8_t* mask, uint8_t* mask_visib, int32_t* out, hipStream_t s);
#define FP_DIAM_MAX_POINTS (1 << 21)          // points of one model (2048 tiles: 2.1 M tile pairs)
#define FP_DIAM_MAX_SLOTS ((size_t)1 << 26)   // per-block maxima of one call (512 MiB of workspace)
int fp_pts_diameter_tile(void);   // points per tile of fp_pts_diameter_launch; slots: M * n_pairs doubles, n_pairs = t (t + 1) / 2, t = tiles of max_count
int fp_pts_diameter_launch(const double* pts, int n_pts, const int* ranges, int M, int max_count, double* slots, double* out, hipStream_t s);
// lk_track.hip: the built-in pyramidal Lucas-Kanade point tracker (lk_core.h holds the host-checkable arithmetic and the pyramid layout)
struct LkPyramid;
int fp_lk_pyramid_launch(const uint8_t* frames, const LkPyramid& P, float* pyr, hipStream_t s);
int fp_lk_track_launch(const LkPyramid& P, const float* pyr, const float* queries, int N, int radius, int iters, float fb_thresh,
                       float min_eig, float max_residual, double* state, float* tracks, uint8_t* vis, float* diag, hipStream_t s);   // state: T * N * 2 doubles
