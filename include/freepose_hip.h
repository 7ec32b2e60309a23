/* freepose_hip.h — C ABI of libfreepose_hip.so, the MI355X (gfx950) implementation of FreePose's
 * per-proposal 6D-pose hot path.  Plain pointers and sizes only; every pointer named `d_*` or documented
 * "device" is a HIP device pointer owned by the caller, every call takes the HIP stream to enqueue on
 * (void* = hipStream_t; NULL = default stream) and returns 0 on success or an FP_ERR_* code, with
 * fp_last_error() giving the text.  No exceptions cross this boundary.  Nothing here touches torch.
 *
 * Streams.  ALL device work of a call — kernels, memsets, copies, weight repacks — is enqueued on the stream the call is given, and a call
 * returns without waiting unless its comment says that it synchronises that stream (fp_geodesic_select, fp_gt_visibility,
 * fp_pts_diameter, fp_video_errors, fp_clip_text_encode).  Nothing on the steady path waits for the whole device: the only device-wide
 * waits are one-off (the GELU table of a device, the re-fold after a ViT weight was replaced), and a workspace is freed — which drains the
 * device — only when a call needs it larger than any call before.  Calls on one context are ordered by the caller: a context is "one
 * context per thread/GPU, no locking", its workspaces (and those of the ViT / CLIP / mesh handles made on it) are shared by all of its
 * calls, so two streams may use a context only with an event or wait between their calls (hipStreamWaitEvent, or a host wait); state a
 * call builds on its stream — folded weights, resized position rows, repacked patch weights, the FFA arrival counters, a workspace's
 * first allocation — is then safe to use from the other stream.  tests/test_gpu_streams.py holds every entry to this.
 *
 * Each entry names the reference interface it replaces (file:line relative to ponimatkin/freepose).
 * bf16 tensors are raw uint16 bit patterns.
 */
#ifndef FREEPOSE_HIP_H
#define FREEPOSE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FP_OK 0
#define FP_ERR_INVALID 1
#define FP_ERR_HIP 2
#define FP_ERR_STATE 3

typedef struct fp_ctx fp_ctx; /* one per (thread, GPU): owns workspaces, no hidden globals */
typedef struct fp_vit fp_vit; /* ViT weights table + per-resolution pos-embed cache         */
typedef struct fp_mesh fp_mesh; /* device copy of a triangle mesh for the rasteriser         */

const char* fp_last_error(void);
int fp_version(void);
int fp_ctx_create(int device, fp_ctx** out);
int fp_ctx_destroy(fp_ctx* ctx);
/* Run-time options of ONE context (no process-global state, no environment variables: the library never calls getenv).
 * value < 0 restores the default.
 *   "ln_fused":       1 (default) LayerNorm 1 / 2 folded into the qkv / fc1 GEMMs of fp_vit_forward on a ViT of this context,
 *                     0 the separate LayerNorm kernel (same reference rounding points; used by the parity tests)
 *   "raster_tiled":   unset = LDS-tiled rasteriser for meshes up to 131 072 triangles and images up to 704 px, global
 *                     visibility-buffer strategy otherwise; 1 / 0 force one of them (both bit-identical)
 *   "comm_timeout_s": seconds fp_comm_init waits for the rendezvous of all ranks (default 180) before it returns FP_ERR_STATE
 *   "gemm_row_split": 1 (default) a GEMM launch between the tile tiers runs whole rounds of the resident grid on 256x256 tiles and
 *                     the remaining rows on the finer tiers; 0 never splits (bit-identical; tests/test_gpu_kernels.py)
 * The measurement variants of earlier rounds (alternative GEMM main loops, attention ring depths, ...) are not in this library:
 * they are compiled only into the lab build (python -m freepose_amd.build --lab -> libfreepose_hip_lab.so, used by tools/). */
int fp_ctx_set_option(fp_ctx* ctx, const char* name, int value);
/* bytes currently held in the context's workspaces (diagnostics) */
size_t fp_ctx_workspace_bytes(const fp_ctx* ctx);

/* ---- a1/a2: DINOv2FeatureExtractor (src/pipeline/retrieval/dino.py:8-32; hub dinov2 ViT) -------------- */
typedef struct {
    int dim;       /* 1024 (ViT-L), 384 (ViT-S), 768 (ViT-B)            */
    int depth;     /* 24 / 12 / 12                                     */
    int heads;     /* dim / 64                                         */
    int mlp_dim;   /* 4 * dim                                          */
    int patch;     /* 14                                               */
    int n_reg;     /* 4 register tokens (0 for non-reg checkpoints)    */
    int pos_grid;  /* 37 (pos_embed is [1 + 37*37, dim])               */
    float ln_eps;  /* 1e-6                                             */
} fp_vit_arch;

int fp_vit_create(fp_ctx* ctx, const fp_vit_arch* arch, fp_vit** out);
int fp_vit_destroy(fp_vit* vit);
/* Register one state-dict tensor by its DINOv2 name (dino.py:10 loads exactly this checkpoint layout):
 *   cls_token, pos_embed, register_tokens, patch_embed.proj.{weight,bias}, blocks.{i}.norm1.{weight,bias},
 *   blocks.{i}.attn.qkv.{weight,bias}, blocks.{i}.attn.proj.{weight,bias}, blocks.{i}.ls1.gamma,
 *   blocks.{i}.norm2.{weight,bias}, blocks.{i}.mlp.fc1.{weight,bias}, blocks.{i}.mlp.fc2.{weight,bias},
 *   blocks.{i}.ls2.gamma, norm.{weight,bias}
 * d_bf16 is a device pointer to the bf16 tensor in its native layout; the caller keeps it alive.
 * patch_embed.proj.weight is copied into a K-padded private buffer. */
int fp_vit_set_weight(fp_vit* vit, const char* name, const void* d_bf16, size_t numel, void* stream);
/* feature_type: 0 = cls [B,dim], 1 = reg [B,n_reg,dim], 2 = patch [B,P,dim]  (dino.py:25-30);
 * 3 = patch features with every row F.normalize()d — what the estimators score (pose_estimator.py:85-88,
 * online_pose_estimator.py:72-76 normalise the template / hypothesis features right after this call): the bits of
 * fp_l2_normalize(feature_type 2), written by the final-norm kernel itself.
 * d_images: bf16 [B,3,H,W] in [0,1] (ImageNet normalisation is fused, dino.py:12,16);
 * runs blocks 0..layer-1 (all blocks if layer > depth, dino.py:18-21) then the final norm. */
int fp_vit_forward(fp_vit* vit, const void* d_images, int B, int H, int W, int layer, int feature_type,
                   void* d_out_bf16, void* stream);
/* algorithmic FLOPs of one fp_vit_forward call (SURVEY §8d formula) */
double fp_vit_flops(const fp_vit* vit, int B, int H, int W, int layer);

/* ---- a3: FFA descriptor (scripts/extract_retrieval_features.py:49-57, extract_proposals_ground.py:126-134) */
/* d_feats bf16 [B,P,D]; d_mask u8 [B, gh*cell, gw*cell] (cell=14: any-pool == cv2 INTER_AREA > 0) or
 * [B,P] with cell=1.  d_out_bf16 [B,D] (may be NULL), d_out_f32 [B,D] (bf16 values widened, may be NULL);
 * normalize != 0 applies F.normalize(dim=-1) with bf16 rounding points to d_out_bf16. */
int fp_ffa(fp_ctx* ctx, const void* d_feats, const uint8_t* d_mask, int B, int gh, int gw, int D, int cell,
           int normalize, void* d_out_bf16, float* d_out_f32, void* stream);

/* ---- a4: cosine top-k retrieval (scripts/extract_proposals_ground.py:39-41,136-140) ------------------- */
/* bank prep: fp32 [N,D] -> bf16 -> row L2-normalise in bf16 (ground.py:40-41).  d_bank_bf16 out [N,D]. */
int fp_bank_prepare(fp_ctx* ctx, const float* d_bank_f32, int N, int D, void* d_bank_bf16, void* stream);
/* scores = bf16(bank @ q).float(); top-k by (score desc, index asc).  d_queries bf16 [Q,D].
 * idx_offset is added to every returned index (bank-row sharding across ranks). */
int fp_bank_topk(fp_ctx* ctx, const void* d_bank_bf16, int N, int D, const void* d_queries, int Q, int k,
                 int idx_offset, float* d_out_scores, int32_t* d_out_idx, void* stream);
/* merge per-shard candidates [Q,C] down to [Q,k] with the same ordering (after an RCCL all-gather). */
int fp_topk_merge(fp_ctx* ctx, const float* d_cand_scores, const int32_t* d_cand_idx, int Q, int C, int k,
                  float* d_out_scores, int32_t* d_out_idx, void* stream);
/* per-view fine re-rank (scripts/extract_proposals_ground.py:147-160, --topk k): d_views bf16 [sum_views, D] = the
 * per-mesh descriptor files back to back (np.load(...).to(bf16), NOT normalised), d_offsets i32 [n_mesh+1] row offsets,
 * d_cand i32 [Q,C] coarse candidates (mesh rows), d_queries bf16 [Q,D].  d_out f32 [Q,C] = numpy float32 mean of the
 * top-k per-view scores bf16(normalize_bf16(view) . f).  k <= 128, <= 1024 views per mesh. */
int fp_rerank_views(fp_ctx* ctx, const void* d_views, const int32_t* d_offsets, const int32_t* d_cand,
                    const void* d_queries, int Q, int C, int D, int k, float* d_out, void* stream);
/* F.normalize(x, dim=-1) on bf16 rows with the reference's rounding points: d_x_bf16 and d_y_bf16 bf16 [rows,D] (in place is allowed). */
int fp_l2_normalize(fp_ctx* ctx, const void* d_x_bf16, int rows, int D, void* d_y_bf16, void* stream);

/* ---- a7/a10: patchwise template score (pose_estimator.py:85-88, online_pose_estimator.py:68-79) ------- */
/* d_tmpl bf16 [T,P,D] raw template features (normalised on the fly), d_query bf16 [P,D] used AS GIVEN
 * (callers pass F.normalize'd or raw features exactly where the reference does).  d_weights f32 [T,P] or
 * NULL (mask_scores variant).  d_scores f32 [T]. */
int fp_template_score(fp_ctx* ctx, const void* d_tmpl, const void* d_query, const float* d_weights, int T, int P,
                      int D, float* d_scores, void* stream);
/* The same score for a PRE-NORMALISED template store: d_tmpl_normed = fp_l2_normalize of the raw [T*P, D]
 * features, done once when they enter the cache.  F.normalize of a bf16 tensor is a bf16 tensor, so this is the reference's
 * own intermediate (pose_estimator.py:85) and the scores are bit-identical to fp_template_score on the raw features; the
 * kernel is a streaming dot (one pass over T*P*D*2 bytes). */
int fp_template_score_normed(fp_ctx* ctx, const void* d_tmpl_normed, const void* d_query, const float* d_weights, int T,
                             int P, int D, float* d_scores, void* stream);

/* ---- a5: CropResizePad (src/utils/bbox_utils.py:20-56) as used by Proposals (src/pipeline/utils.py:32-52)
 * and MeshRenderer.generate_proposals (renderer.py:109-130) -------------------------------------------- */
/* d_images: src_fmt 0 = f32 [n_img,C,H,W] in [0,1]; 1 = u8 [n_img,H,W,C] -> float(double(x)/255) like
 * renderer.py:121; 2 = u8 [n_img,H,W,C] -> float(x)/255.f like Proposals (utils.py:20).  n_img is 1 (all boxes crop the same image, Proposals) or n (one image per box, renders).
 * d_boxes i32 [n,4] xyxy BEFORE extension.  d_masks u8 [n,H,W] or NULL; mask_mode 0 = ignore,
 * 1 = multiply pixels by the mask (mask_rgb=True, utils.py:39-40), 2 = output the mask itself as 0/1
 * (utils.py:35-37,48-51).  d_out: out_fmt 0 = f32, 1 = bf16, shape [n,C,target,target].
 * Nearest-neighbour index rules replicate F.interpolate exactly (bbox_utils.py:29-35,52-54).
 * A box the reference cannot crop — empty after the clip, a resized side of 0 px (torch raises inside F.interpolate, :35) or an
 * exactly square crop that comes out one pixel short of `target` — gets an all-zero crop here (the boxes are device data: no
 * read-back); the Python mirror classes raise on such boxes like the reference when the boxes are host-resident
 * (freepose_amd/src/utils/bbox_utils.py unresizable_box: the same arithmetic on the host). */
int fp_crop_resize_pad(fp_ctx* ctx, const void* d_images, int src_fmt, int n_img, int C, int H, int W,
                       const int32_t* d_boxes, int n, float bbox_extend, int target, const uint8_t* d_masks,
                       int mask_mode, void* d_out, int out_fmt, void* stream);

/* ---- f-3: TrackingRefiner photo crop (src/pipeline/refiner_utils.py:92-132 crop_image -> torchvision.ops.roi_align,
 * output 518x518, sampling_ratio 2, aligned=False) ------------------------------------------------------------------ */
/* d_images f32 [n_img,C,H,W]; d_rois f32 [n,5] = (image index, x1, y1, x2, y2); d_out f32 [n,C,pooled_h,pooled_w].
 * sampling_ratio <= 0 selects the adaptive ceil(roi/pooled) grid of the original operator. */
int fp_roi_align(fp_ctx* ctx, const float* d_images, int n_img, int C, int H, int W, const float* d_rois, int n,
                 int pooled_h, int pooled_w, int sampling_ratio, float spatial_scale, float* d_out, void* stream);

/* ---- a8/a10: rotation grids and neighbourhood (pose_estimator.py:121-147, online_pose_estimator.py:25-34,55-56) */
/* super-Fibonacci rotations, fp64 [n,3,3] row-major written to HOST memory (one-off setup, n=600/20000). */
int fp_generate_rotations(int n, double* h_out);
/* indices i with geodesic(R_i, R_prev) < thresh_deg; d_grid f64 [G,3,3] (device), h_Rprev9 f64 row-major
 * (host); count in *h_n; d_out_idx i32 [G]: the first *h_n entries are written, in ascending order (np.where order); the entries behind
 * them are unspecified.  Synchronises the stream (the count decides how many hypotheses are rendered next). */
int fp_geodesic_select(fp_ctx* ctx, const double* d_grid, int G, const double* h_Rprev9, double thresh_deg,
                       int32_t* d_out_idx, int* h_n, void* stream);

/* ---- a11: MeshRenderer (src/pipeline/retrieval/renderer.py:43-95; pyrender/OpenGL semantics) ---------- */
/* vertices f32 [V,3], faces i32 [F,3], per-vertex colours u8 [V,3] or NULL (white).  All host pointers. */
int fp_mesh_upload(fp_ctx* ctx, const float* h_verts, int V, const int32_t* h_faces, int F,
                   const uint8_t* h_colors, fp_mesh** out);
/* textured mesh, as pyrender.Mesh.from_trimesh(mesh) receives it from trimesh.load(obj, force='mesh') (renderer.py:43-45,70-72;
 * scripts/dino_inference_video.py:93-101, scripts/render_templates.py:58-66): per-corner texture coordinates uv f32 [F,3,2]
 * (OBJ `vt` convention: v up), diffuse texture u8 [th,tw,3] (image rows top to bottom), material diffuse factor kd f32 [3] or
 * NULL (= 1,1,1).  Fragments are shaded with a perspective-correct texture fetch (REPEAT wrap, trilinear over a box-filtered
 * mip chain built at upload — the sampler pyrender gives a trimesh texture; fp_mesh_set_filter(.., 0) = bilinear level 0); the
 * exact arithmetic is the contract at the top of csrc/raster.hip.  All host pointers. */
int fp_mesh_upload_textured(fp_ctx* ctx, const float* h_verts, int V, const int32_t* h_faces, int F, const float* h_uv,
                            const uint8_t* h_texture, int th, int tw, const float* h_kd3, fp_mesh** out);
int fp_mesh_destroy(fp_mesh* mesh);
/* ambient light factor of the scene the mesh is rendered in: 2 (default; renderer.py:53-55,80-82) or 5
 * (tracking_refiner.py:33) */
int fp_mesh_set_ambient(fp_mesh* mesh, float ambient);
/* output transfer: 1 (default) = gamma rule, u8 = round(255 (ambient c)^(1/2.2)) with sRGB-decoded texels (how a PBR ambient
 * term reaches the frame buffer); 0 = linear rule, u8 = min(255, 255 ambient c + .5).  pyrender's shader is third-party and
 * not in the reference tree, so neither is pinned; both are bit-exact against the oracle. */
int fp_mesh_set_shading(fp_mesh* mesh, int mode);
/* texture minification: 1 (default) = trilinear mip-maps, level of detail from the analytic UV derivatives of the fragment;
 * 0 = bilinear fetch of level 0 only.  Replaces the sampler state of pyrender's texture objects (renderer.py:43-47,70-74). */
int fp_mesh_set_filter(fp_mesh* mesh, int mode);
/* back-face culling: 0 (default, what every caller of the reference uses: renderer.py:66,93 pass SKIP_CULL_FACES) = both sides drawn;
 * 1 = `cull_faces=True` (renderer.py:63-64,90-91): triangles whose counter-clockwise-from-outside side faces away are not drawn. */
int fp_mesh_set_cull(fp_mesh* mesh, int mode);
/* vertex stage of the rasteriser alone: window coordinates in 24.8 fixed point d_xy i32 [Hn,V,2] (x right, y down, pixel
 * centres at +0.5; 0,0 for vertices at or behind the near plane) and camera-frame depth d_zc f32 [Hn,V].  Conventions pinned
 * against the reference's K -> OpenGL projection (bop_toolkit_lib/renderer_py.py:186-231, renderer.py:37-41). */
int fp_project_vertices(fp_ctx* ctx, const fp_mesh* mesh, const float* d_poses, int Hn, float scale, float fx, float fy,
                        float cx, float cy, int32_t* d_xy, float* d_zc, void* stream);
/* poses f32 [Hn,4,4] (OpenCV camera frame, object->camera), intrinsics fx,fy,cx,cy, image W x Hh.
 * scale multiplies the vertices (rendering_scale 0.25).  Outputs rgb u8 [Hn,Hh,W,3], depth f32 [Hn,Hh,W]
 * (metric eye depth, 0 = background).  Ambient-only shading, no culling (renderer.py:53-55,66). */
int fp_rasterize(fp_ctx* ctx, const fp_mesh* mesh, const float* d_poses, int Hn, float scale, float fx, float fy,
                 float cx, float cy, int W, int Hh, uint8_t* d_rgb, float* d_depth, void* stream);
/* fp_rasterize with the consumers of the depth image fused into the tile epilogue (renderer.py:98-130 takes the
 * depth>0 bounding box of every render, pose_estimator.py:104-112 the cloud extents of the winners): d_ext f64 [Hn,8] = exactly what
 * fp_depth_extents gives on the depth image, d_boxes i32 [Hn,4] = its first four columns as CropResizePad takes them.  d_depth,
 * d_ext, d_boxes may each be NULL (not d_ext and d_boxes both): without d_depth the 4 bytes per pixel are neither written nor read
 * back.  Same bits as fp_rasterize + fp_depth_extents. */
int fp_rasterize_extents(fp_ctx* ctx, const fp_mesh* mesh, const float* d_poses, int Hn, float scale, float fx, float fy,
                         float cx, float cy, int W, int Hh, uint8_t* d_rgb, float* d_depth, double* d_ext, int32_t* d_boxes,
                         void* stream);
/* a9/K17: per view, bbox of depth>0 (with the <100 px fallback square) and metric extents of the
 * back-projected cloud (float64 like utils.py:122-145): out f64 [Hn,8] = {xmin,ymin,xmax,ymax (px), dx, dy (m),
 * count, 0}. */
int fp_depth_extents(fp_ctx* ctx, const float* d_depth, int Hn, int Hh, int W, float fx, float fy, float cx,
                     float cy, double* d_out, void* stream);

/* ---- g: pose-error evaluation (bop_toolkit/scripts/eval_calc_errors.py:311-570 and bop_toolkit_lib/pose_error.py; the reference
 * renders with OpenGL and builds two kd-trees per estimate x ground-truth pair) ------------------------------------------------- */
/* chamfer (pose_error.py:188-201) and, with projected = 1, chamfer_proj (:204-218) of B pairs in one call:
 *   d_out f64 [B]: d_out[b] = mean_y(min_x |x - y|) + mean_x(min_y |x - y|)    (chamfer_distance(direction='bi', metric='l2'), :143-185; not squared)
 * over x = posed (projected) vertices of the mesh used at inference, y = those of the ground-truth model.
 * d_pts f64 [n_pts,3]: the vertex clouds of every model back to back.  d_table i32 [B,8] per pair: {first row of the estimate's cloud in
 * d_pts, its size, first row of the GT cloud, its size, first slot of the two centred clouds in the workspace (each pair owns size_e +
 * size_g consecutive slots out of ws_pts), 0, 0}; max_n = the largest cloud size.  d_xf f64 [B,40] per pair: {s_e, R_e[9], t_e[3],
 * R_g[9], t_g[3], centroid of the GT cloud in its model frame [3], K[9] (projected only), 0...}: pts_e * s_e (eval_calc_errors.py:380),
 * then misc.transform_pts_Rt / misc.project_pts in fp64; both clouds are centred on the posed (projected) GT centroid before the one
 * rounding to fp32; exact brute-force minimum of the squared fp32 differences, one fp64 sqrt per point, fixed-order fp64 sums (two
 * calls give the same bits).  |d_out - reference| <= 2e-6 (r + reference), r = the largest centred coordinate.
 * The table is device data and cannot be checked by the call: a row whose clouds are empty or reach outside d_pts / the ws_pts slots
 * is not read or written through, and its d_out is NaN (the call still returns FP_OK). */
int fp_chamfer(fp_ctx* ctx, const double* d_pts, int n_pts, const int32_t* d_table, const double* d_xf, int B, int max_n, int ws_pts,
               int projected, double* d_out, void* stream);
/* pixel counts behind cus (pose_error.py:357-386) and vsd (:17-112) for B pairs of rendered depth images d_depth_est / d_depth_gt
 * f32 [B,Hh,W] (fp_rasterize_extents output).  Without d_depth_test: d_out i32 [B,4] = {inter, union of depth > 0, 0, 0} and n_tau = 0.
 * With d_depth_test f32 [n_img,Hh,W] (test depth in the unit of the renders) and d_img_idx i32 [B] (the image of each pair):
 * d_out i32 [B,4+n_tau] = {inter, union, visib_inter, visib_union, per tau the number of visib_inter pixels with
 * |dist_gt - dist_est| / divisor >= tau} — misc.depth_im_to_dist_im_fast (misc.py:136-167) in fp64, visibility._estimate_visib_mask
 * mode bop19 and estimate_visib_mask_est (visibility.py:34-38,74-75) with the float32 difference, step cost (pose_error.py:80-102).
 * d_params f64 [B,8] = {fx, fy, cx, cy, delta, divisor (the diameter with normalized_by_diameter, else 1), 0, 0}; d_taus f64 [n_tau],
 * n_tau <= 16, all counted in the same pass.  Every count equals the reference's; the error value is formed by the host.
 * The depth stacks may have any float alignment: 16-byte loads are used when Hh * W is a multiple of 4 and the three base pointers
 * are 16-byte aligned, a scalar loop otherwise (same counts).  A d_img_idx outside [0, n_img) gives a row of zeros. */
int fp_depth_compare(fp_ctx* ctx, const float* d_depth_est, const float* d_depth_gt, int B, int Hh, int W, const float* d_depth_test,
                     int n_img, const int32_t* d_img_idx, const double* d_params, const double* d_taus, int n_tau, int32_t* d_out,
                     void* stream);

/* ---- h: object scale from the scene's depth map (`--depth_method depthmap`, MeanScaleEstimator) ------------------------------------ */
/* connected components of n binary masks d_masks u8 [n,H,W] (non-zero = foreground), connectivity 4 or 8: what
 * scipy.ndimage.label(mask, structure) numbers in src/pipeline/utils.py:71-84 (extract_largest_component).  d_labels i32 [n,H,W]:
 * 0 = background, else 1 + raster index (y * W + x) of the component's first pixel in scan order — ranked, these are scipy's labels.
 * Union-find with atomicMin on labels that only decrease: exact, and the same output on every call. */
int fp_label_components(fp_ctx* ctx, const uint8_t* d_masks, int n, int H, int W, int connectivity, int32_t* d_labels, void* stream);
/* generate_pointcloud + get_scale of src/pipeline/estimators/scale_estimators.py:117-187 for the n proposal masks of one image in one
 * call: largest 4-connected component (first in scan order among equal areas), isotropic erosion by erosion_radius halved until more
 * than min_vertices pixels survive (the un-eroded component once a radius below 1 has failed; 0 < erosion_radius <= 8), depth samples
 * within std_factor population standard deviations of the exact median — never fewer than min_vertices, and only min_vertices when no
 * sample is farther (the reference's argmax quirk, kept); ties are cut by (|z - median| ascending, raster index ascending) —
 * back-projection with fx, fy, cx, cy in float64, with align = 1 rotation into the principal axes (`svd=True`), d_scale f64 [n] = half
 * the largest extent.  d_depth f64 [H,W] is shared by all masks.  d_info i32 [n,4] = {area of the component, index of the radius used
 * (0 = erosion_radius, 1 = half of it, ...; the number of radii tried = un-eroded: 5 for radius 8), survivor count, points kept}.
 * d_keep u8 [n,H,W] or NULL: 1 on the pixels whose points entered the extent.  An empty mask gives area 0 and a NaN scale (FP_OK).
 * Everything but the last floating-point sums is exact; two calls give the same bits. */
int fp_depthmap_scale(fp_ctx* ctx, const double* d_depth, const uint8_t* d_masks, int n, int H, int W, double fx, double fy, double cx,
                      double cy, double erosion_radius, double std_factor, int min_vertices, int align, double* d_scale, int32_t* d_info,
                      uint8_t* d_keep, void* stream);

/* ---- e: multi-GPU.  One process per GPU; RCCL over xGMI.  The reference has no counterpart (SLURM array jobs +
 * files: scripts/dino_inference.py:51-54, merge_results.py); Python hosts use torch.distributed (freepose_amd/parallel.py), these
 * entry points serve hosts without it.  librccl is opened lazily on first use. ------------------------------------------- */
/* rank 0 creates the 128-byte RCCL unique id (ncclGetUniqueId) and hands it to the other ranks through the host's own channel */
int fp_comm_unique_id(void* out_id128);
/* collective over all `nranks` ranks (ncclCommInitRank).  Fails — status + fp_last_error(), never a hang — on a bad rank / nranks,
 * an all-zero id, a context that already has a communicator, or when the rendezvous does not complete within "comm_timeout_s"
 * (ranks that disagree on nranks or on the id, a rank that never arrives). */
int fp_comm_init(fp_ctx* ctx, int nranks, int rank, const void* unique_id128);
int fp_comm_destroy(fp_ctx* ctx);
int fp_comm_size(const fp_ctx* ctx);
int fp_comm_rank(const fp_ctx* ctx);
/* all-gather `bytes` device bytes from every rank into d_recv [nranks * bytes] (rank order); a copy without a communicator */
int fp_allgather_bytes(fp_ctx* ctx, const void* d_send, size_t bytes, void* d_recv, void* stream);
/* bank-row sharding: every rank passes its local top-k [Q,k] with GLOBAL row indices; the candidates of all ranks
 * are gathered and merged with the canonical (score desc, index asc) rule -> identical [Q,k_out] on every rank (d_out_scores f32,
 * d_out_idx i32) */
int fp_allgather_topk(fp_ctx* ctx, const float* d_scores, const int32_t* d_idx, int Q, int k, int k_out, float* d_out_scores,
                      int32_t* d_out_idx, void* stream);
/* proposal / frame / object sharding: gather n_rows fixed-length f64 result rows per rank (every rank passes the same n_rows;
 * pad with rows the caller can recognise) into d_out [nranks * n_rows, row_len] */
int fp_allgather_poses(fp_ctx* ctx, const double* d_rows, int n_rows, int row_len, double* d_out, void* stream);

/* ---- kernel-level entry points (unit parity tests, microbenchmarks; the ViT forward is built from these) */
/* C[M,N] = epi(X[M,K] W[N,K]^T + bias): epi 0 = bias, 1 = bias+GELU(erf), 2 = resid + gamma*(.) ; bf16, ld* in
 * elements (multiples of 8), K % 64 == 0, N % 16 == 0. */
int fp_op_gemm(fp_ctx* ctx, const void* d_X, int ldx, const void* d_W, int ldw, void* d_C, int ldc, const void* d_bias,
               const void* d_gamma, const void* d_resid, int ldr, int M, int N, int K, int epi, void* stream);
/* V part of qkv stored transposed per head: Vt[b,h,d,t] for rows m = b*npad + t, n = h*64 + d */
int fp_op_gemm_vt(fp_ctx* ctx, const void* d_X, int ldx, const void* d_W, int ldw, void* d_Vt, const void* d_bias, int M, int N,
                  int K, int npad, int heads, void* stream);
/* LayerNorm folded into the consuming linear layer, the way fp_vit_forward runs LN1 -> qkv and LN2 -> fc1 (hub DINOv2 block:
 * x + ls1 * attn(norm1(x)); x + ls2 * mlp(norm2(x)) — the nn.LayerNorm + nn.Linear pairs behind src/pipeline/retrieval/dino.py:18-19):
 *   LN(x) W^T + b  =  rstd (x W'^T - mean colsum(W')) + b',   W' = W diag(gamma_ln),  b' = b + W beta_ln
 * d_X bf16 [M,K] raw rows, d_g_ln / d_b_ln bf16 [K], d_W bf16 [N,K], d_bias bf16 [N].  mode 0: d_out bf16 [M,N] = linear,
 * 1: GELU(linear), 2: transposed per head like fp_op_gemm_vt (npad, heads).  Output features n < n_scaled are multiplied by row_scale
 * inside the fold (W' and b' of those rows; one rounding) — the ViT's q rows with log2(e) / sqrt(64); n_scaled = 0 for none.
 * Kernel-level entry used by the tests. */
int fp_op_ln_linear(fp_ctx* ctx, const void* d_X, int M, int K, const void* d_g_ln, const void* d_b_ln, float eps, const void* d_W,
                    int N, const void* d_bias, int mode, int npad, int heads, int n_scaled, float row_scale, void* d_out, void* stream);
/* fp_op_gemm with epilogue 2 (LayerScale + residual) that also emits the row statistics of what it wrote — the producer side of the
 * folded LayerNorm (per-64-column partial sums in the epilogue, summed in block order).  d_stat u32/f32 [M,6]: words 0-3 the 16-byte
 * init-MFMA record of the row as the consuming GEMM reads it — bf16 {sh, sl, sh, -mh, -ml, -mh, 0, 0}, sigma = sqrt(var + eps) and
 * -mean as two-piece bf16 splits —, word 4 rstd = 1 / sigma (f32), word 5 unused (never written). */
int fp_op_gemm_stats(fp_ctx* ctx, const void* d_X, int ldx, const void* d_W, int ldw, void* d_C, int ldc, const void* d_bias,
                     const void* d_gamma, const void* d_resid, int ldr, int M, int N, int K, float eps, float* d_stat, void* stream);
/* The patch-embed GEMM of fp_vit_forward (the Conv2d patch_embed.proj of hub DINOv2 behind src/pipeline/retrieval/dino.py:18 as a GEMM
 * on unfolded patches): row m = b*P + p of d_X lands in row b*npad + tok_off + p of the token buffer d_C (ldc elements per row) as
 * bf16(bf16(x W^T + bias) + pos[p]); d_pos bf16 [P,N].  M % P == 0, tok_off + P <= npad; the other rows of d_C are not written.
 * Kernel-level entry used by the tests. */
int fp_op_gemm_patch(fp_ctx* ctx, const void* d_X, int ldx, const void* d_W, int ldw, void* d_C, int ldc, const void* d_bias,
                     const void* d_pos, int M, int N, int K, int P, int npad, int tok_off, void* stream);
/* Producer -> consumer pair of the folded LayerNorm as fp_vit_forward chains them: d_Y bf16 [M,D] = resid + gamma * (X1 W1^T + b1)
 * (X1 [M,K1], W1 [D,K1], resid [M,D]; the epilogue also writes the partial row statistics), then d_out bf16 [M,N2] (ldo elements per
 * row) = LN(Y) W2^T + b2 (mode 0) or GELU of it (mode 1) by the LN-folded GEMM, n_scaled / row_scale as in fp_op_ln_linear.
 * route 0: the statistics are finalised by their own kernel first; route 1: the consumer launch is handed the partial sums with the
 * fields fp_vit_forward sets and the GEMM dispatch decides where they are finalised (fp_vit_forward itself finalises up front when the
 * launch takes the big tier and never hands such a launch the sums; route 1 there pins the dispatch's own fallback, which runs the same
 * finalisation kernel as route 0).  d_mfrag u32 [M,4] and d_rstd f32 [M] receive
 * the row records (layout: fp_op_gemm_stats) and 1 / sigma the consumer used.  Kernel-level entry used by the tests. */
int fp_op_ln_chain(fp_ctx* ctx, const void* d_X1, int K1, const void* d_W1, const void* d_b1, const void* d_gamma, const void* d_resid,
                   void* d_Y, int M, int D, const void* d_g_ln, const void* d_b_ln, float eps, const void* d_W2, int N2,
                   const void* d_b2, int mode, int n_scaled, float row_scale, int route, void* d_out, int ldo, void* d_mfrag,
                   float* d_rstd, void* stream);
/* One LN-folded consumer (fp_op_ln_linear's modes 0, 1, 2) on row records the caller supplies instead of records recomputed from the
 * rows: d_mfrag u32 [M,4] and d_rstd f32 [M] as fp_op_ln_chain, fp_op_row_stats or fp_op_stats_finalize return them.  This is how
 * fp_vit_forward's transposed-V launch of a block reads the records the qk launch of the same block wrote.  d_out: bf16 [M,N] with ldo
 * elements per row (modes 0, 1) or Vt [M/npad, heads, 64, npad] (mode 2, N == 64 * heads; ldo unused).  K % 64 == 0.  Kernel-level entry
 * used by the tests. */
int fp_op_ln_consume(fp_ctx* ctx, const void* d_X, int M, int K, const void* d_g_ln, const void* d_b_ln, const void* d_W, int N,
                     const void* d_bias, int mode, int npad, int heads, int n_scaled, float row_scale, const void* d_mfrag,
                     const float* d_rstd, void* d_out, int ldo, void* stream);
/* copies the first `bytes` bytes of the context's named workspace (the buffers a tower forward leaves behind: "vit.x", "vit.qk",
 * "clip.qkv", "clip_text.pool", ...) to host memory, after a device synchronisation; an unknown name or a workspace shorter than `bytes`
 * is an error.  Host-only entry used by the tests that replay a forward step by step. */
int fp_op_workspace_read(fp_ctx* ctx, const char* name, void* host, size_t bytes);
/* writes into `out` (at most out_bytes, NUL-terminated) the plan the GEMM dispatch of this context would execute on this device for a
 * launch C[M,N] = epi(X[M,K] W[N,K]^T) — epi = the library's nine epilogues 0 .. 8, ldx / ldw the operands' row strides, ln_part != 0: the
 * launch carries partial row statistics — under the context's "gemm_row_split"; launches nothing.  The text is
 *   <label> row0=<r> ring=<a>,<b> grid=<a>,<b>
 * with <label> one of tiny64 | small128 | big_hip | big_hip_stream | big_asm, split_big+<tier> / split_mid+<tier> (whole rounds on the
 * 256x256 / 128x128 tiles in front, <tier> = where the remaining rows run), finalize_then_<label> (the row statistics are finalised by a
 * kernel in front); row0 = the first row of the second part (0 = no split), ring = K-tile ring depth of each part (0: not on the 64x64
 * tier), grid = workgroups of each part.  Host-only entry used by the tests of the tile tiers. */
int fp_op_gemm_plan(fp_ctx* ctx, int M, int N, int K, int epi, int ldx, int ldw, int ln_part, char* out, size_t out_bytes);
/* writes into `out` (at most out_bytes, NUL-terminated) how fp_rasterize / fp_rasterize_extents of this context would launch a mesh of F
 * triangles under Hn poses on a W x H frame, under the context's "raster_tiled"; launches nothing.  The text is
 *   <tiled|global> T=<tile edge> tiles=<ntx>x<nty> chunks=<n> rounds=<n> bin=<workgroups per view> views=<groups of 8>+<rest>
 *   flush=<dword|bytes|none> lds=<bytes> big_area=.. big_tile_area=.. chunk=.. hits_round=.. small_span=.. max_tris=.. max_tile=..
 *   clamp=.. znear=..
 * (one line; tiles, chunks, rounds, bin and lds are 0 on the global path): the plan of csrc/raster_plan.h and the thresholds the kernels
 * were compiled with.  Host-only entry used by the tests of the rasteriser's branches. */
int fp_op_raster_plan(fp_ctx* ctx, int W, int H, int F, int Hn, char* out, size_t out_bytes);
/* d_x and d_y bf16 [n]: d_y[i] = bf16(0.5 x (1 + erf(x / sqrt 2))) elementwise on bf16 values in fp32: the direct expression the fc1 epilogue's GELU table
 * is filled from (hub DINOv2 Mlp act_layer = nn.GELU behind src/pipeline/retrieval/dino.py:18-19); the table-GELU GEMM is tested
 * against it on all 65 536 bf16 inputs */
int fp_op_gelu(const void* d_x, void* d_y, size_t n, void* stream);
/* flash attention forward on QK [B*npad, 2*H*64] (ldqk elements) + Vt [B,H,64,npad] -> O [B*npad, H*64].
 * q_prescaled != 0: the q columns already hold q * log2(e) / sqrt(64) (fp_vit_forward folds that factor into the q rows of its
 * LayerNorm-folded qkv weights — fp_op_ln_linear's n_scaled / row_scale — so the softmax needs no multiply-add per element) */
int fp_op_attention(const void* d_QK, int ldqk, const void* d_Vt, void* d_O, int ldo, int B, int H, int n_tok,
                    int npad, int q_prescaled, void* stream);
/* nn.LayerNorm over the last dimension with bf16 rounding of the result: d_X and d_Y bf16 [rows,D], d_gamma and d_beta bf16 [D] */
int fp_op_layernorm(const void* d_X, void* d_Y, const void* d_gamma, const void* d_beta, int rows, int D, float eps,
                    void* stream);
/* ImageNet normalise (torchvision Normalize on a bf16 tensor: subtract, round, divide, round — src/pipeline/retrieval/dino.py:12,16) +
 * patch unfold of bf16 crops [B,3,H,W] in [0,1] into the patch-embed GEMM's A operand [B*(H/ps)*(W/ps), KP], k = c*ps*ps + dy*ps + dx,
 * columns >= 3*ps*ps zero (the Conv2d patch_embed.proj of hub DINOv2 behind dino.py:18).  Kernel-level entry used by the tests. */
int fp_op_im2col_norm(const void* d_img, void* d_A, int B, int H, int W, int ps, int KP, void* stream);
/* The other helper kernels of the towers, one at a time (kernel-level entries used by the tests).  All tensors bf16 unless said
 * otherwise; a call with no rows / no elements returns 0 without launching anything.
 * fp_op_layernorm with the launch form of the towers' final norm, d_Y [rows,D]: output row r reads input row
 * (r / rows_per_b) * in_stride_b + in_off + r % rows_per_b (rows_per_b <= 0: row r); l2_normalize != 0 writes every row
 * F.normalize()d with fp_l2_normalize's arithmetic (D <= 1536).  D: a multiple of 8 up to 2048. */
int fp_op_layernorm_rows(const void* d_X, void* d_Y, const void* d_gamma, const void* d_beta, int rows, int D, float eps, int rows_per_b,
                         int in_stride_b, int in_off, int l2_normalize, void* stream);
/* bicubic (a = -0.5) antialiased resize of a position-embedding grid, d_src [G*G, D] -> d_dst [gh*gw, D] (hub DINOv2
 * interpolate_pos_encoding: F.interpolate(mode="bicubic", antialias=True) on the channel-last grid), fp32 arithmetic. */
int fp_op_posembed_aa(const void* d_src, void* d_dst, int G, int gh, int gw, int D, void* stream);
/* the rows of the token buffer d_X [B, npad, D] that the patch-embed GEMM does not write: row 0 = bf16(cls + pos0), rows 1..nreg = the
 * register tokens d_reg [nreg, D] (no position), rows [n_tok, npad) = 0.  Rows 1 + nreg .. n_tok - 1 are not touched. */
int fp_op_token_init(void* d_X, const void* d_cls, const void* d_pos0, const void* d_reg, int nreg, int B, int n_tok, int npad, int D,
                     void* stream);
/* row statistics of the folded LayerNorm straight from the rows d_X [rows, D] (D a multiple of 8 up to 1536): d_rec u32 [rows,4] the
 * row records and d_rstd f32 [rows] = 1 / sigma, layout as in fp_op_gemm_stats. */
int fp_op_row_stats(const void* d_X, int rows, int D, float eps, void* d_rec, float* d_rstd, void* stream);
/* the same records from per-64-column partial sums d_part f32 [D/64, part_ld, 2] = (sum x, sum x^2) of row m at [nb, m], added in
 * block order (what the LS_RES_STATS epilogue writes); part_ld >= rows, 0 = rows; D a multiple of 64. */
int fp_op_stats_finalize(const void* d_part, int rows, int D, float eps, int part_ld, void* d_rec, float* d_rstd, void* stream);
/* the weight side of the folded LayerNorm (fp_op_ln_linear): d_Wf [N,K] = bf16(W diag(gamma) s_n), s_n = row_scale for n < n_scaled and 1
 * otherwise; d_cb u32 [N,4] = bf16 {b'h, b'h, b'l, ch, ch, cl, 0, 0}, two-piece splits of b' = (bias + W beta) s_n and of
 * c = sum_k Wf[n,k] (over the ROUNDED Wf).  K a multiple of 8. */
int fp_op_ln_fold(const void* d_W, const void* d_gamma, const void* d_beta, const void* d_bias, int N, int K, int n_scaled, float row_scale,
                  void* d_Wf, void* d_cb, void* stream);
/* d_dst [cols, rows] = d_src [rows, cols]^T */
int fp_op_transpose(const void* d_src, void* d_dst, int rows, int cols, void* stream);

/* attention forward for a general head dimension on the plain output of one bias GEMM with N = 3 * width: QKV [B*npad, 3*heads*head_dim]
 * (ldqkv elements), columns [q | k | v], each heads x head_dim (nn.MultiheadAttention's in_proj order) -> O [B*npad, heads*head_dim]
 * (ldo elements), O[b,t,h*head_dim+d] = softmax_j(q.k_j * scale) v_j over the n_tok real tokens.  head_dim: a multiple of 8 in [8, 128];
 * npad % 16 == 0, n_tok <= npad; leading dimensions multiples of 8.  Rows [n_tok, npad) of QKV are never read (they may hold anything);
 * the same rows of O receive finite values.  bf16 in / out, fp32 accumulation and softmax statistics, any sequence length. */
int fp_op_attention_hd(const void* d_QKV, int ldqkv, void* d_O, int ldo, int B, int heads, int head_dim, int n_tok, int npad, float scale,
                       void* stream);
/* the same layout and contract under a CAUSAL mask (open_clip's text transformer): query t attends to the real keys 0 .. t only.  Key
 * tiles wholly above the diagonal are skipped; rows after the query inside a visited tile are loaded and weighted by exactly 0, so they
 * must be finite for V (any bytes for pad rows [n_tok, npad), which are never read).  Pad query rows receive finite values. */
int fp_op_attention_causal(const void* d_QKV, int ldqkv, void* d_O, int ldo, int B, int heads, int head_dim, int n_tok, int npad, float scale,
                           void* stream);

/* ---- CLIP image tower(src/pipeline/retrieval/clip.py: open_clip encode_image on a bf16 module) --------- */
typedef struct fp_clip fp_clip;
typedef struct {
    int width;      /* 1664 (ViT-bigG/14), 1280 (ViT-H/14), 1024 (ViT-L/14); a multiple of 64          */
    int depth;      /* 48 / 32 / 24                                                                    */
    int heads;      /* 16: head dimension width / heads, a multiple of 8 up to 128 (104 / 80 / 64)     */
    int mlp_dim;    /* 8192 / 5120 / 4096                                                              */
    int patch;      /* 14                                                                              */
    int grid;       /* 16: images are (patch * grid)^2, the positional embedding is not interpolated   */
    int embed_dim;  /* 1280 / 1024 / 768                                                               */
    float ln_eps;   /* 1e-5                                                                            */
    int quick_gelu; /* must be 0: only the exact-erf GELU towers are provided                          */
} fp_clip_arch;
int fp_clip_create(fp_ctx* ctx, const fp_clip_arch* arch, fp_clip** out);
int fp_clip_destroy(fp_clip* clip);
/* Register one tensor (bf16, device) by its open_clip visual state-dict name: conv1.weight, class_embedding, positional_embedding,
 * ln_pre.{weight,bias}, transformer.resblocks.{i}.{ln_1,ln_2}.{weight,bias}, transformer.resblocks.{i}.attn.{in_proj_weight,in_proj_bias},
 * transformer.resblocks.{i}.attn.out_proj.{weight,bias}, transformer.resblocks.{i}.mlp.{c_fc,c_proj}.{weight,bias},
 * ln_post.{weight,bias}, proj ([width, embed_dim], applied as x @ proj).  conv1.weight and proj are copied (padded / transposed); every
 * other tensor is referenced and must outlive the handle. */
int fp_clip_set_weight(fp_clip* clip, const char* name, const void* d_tensor, size_t numel, void* stream);
/* d_images bf16 [B,3,S,S] in [0,1] (S must equal patch * grid) -> d_out bf16 [B, embed_dim]: CLIP mean / std normalisation, patch
 * conv (no bias), [class; patches] + positional embedding, ln_pre, the blocks, ln_post on the class row, projection. */
int fp_clip_encode_image(fp_clip* clip, const void* d_images, int B, int S, void* d_out, void* stream);
double fp_clip_flops(const fp_clip* clip, int B);

/* ---- CLIP text tower (scale_estimators.py:91-94: open_clip encode_text on a bf16 module) ---------------- */
typedef struct fp_clip_text fp_clip_text;
typedef struct {
    int width;      /* 1280 (ViT-bigG/14), 1024 (ViT-H/14), 768 (ViT-L/14); a multiple of 64           */
    int depth;      /* 32 / 24 / 12                                                                    */
    int heads;      /* 20 / 16 / 12: head dimension width / heads (64), a multiple of 8 up to 128      */
    int mlp_dim;    /* 5120 / 4096 / 3072                                                              */
    int vocab;      /* 49408                                                                           */
    int ctx;        /* 77 tokens per prompt (padded to a multiple of 16 rows internally)               */
    int embed_dim;  /* 1280 / 1024 / 768                                                               */
    float ln_eps;   /* 1e-5                                                                            */
} fp_clip_text_arch;
int fp_clip_text_create(fp_ctx* ctx, const fp_clip_text_arch* arch, fp_clip_text** out);
int fp_clip_text_destroy(fp_clip_text* text);
/* Register one tensor (bf16, device) by its open_clip state-dict name: token_embedding.weight [vocab, width], positional_embedding
 * [ctx, width], transformer.resblocks.{i}.* as for the image tower, ln_final.{weight,bias}, text_projection ([width, embed_dim], applied
 * as x @ P).  text_projection is copied (transposed); every other tensor is referenced and must outlive the handle. */
int fp_clip_text_set_weight(fp_clip_text* text, const char* name, const void* d_tensor, size_t numel, void* stream);
/* d_ids i32 [B, ctx] -> d_out bf16 [B, embed_dim]: token + positional embedding, the blocks under the causal mask, ln_final on the row
 * of the largest id of each prompt (the first one: the end-of-text token), projection.  An id outside [0, vocab) is refused
 * (FP_ERR_INVALID; the embedding table is never read out of range).  Synchronises the stream once, after the embedding gather. */
int fp_clip_text_encode(fp_clip_text* text, const int32_t* d_ids, int B, void* d_out, void* stream);
double fp_clip_text_flops(const fp_clip_text* text, int B);

/* ---- exact k nearest rows (scipy.spatial.KDTree.query of GPT4ScaleEstimator, scale_estimators.py:48,66) -- */
/* d_table f32 [N,E], d_queries f32 [Q,E] -> d_out_idx i32 [Q,k], d_out_d2 f32 [Q,k] (SQUARED Euclidean distances, fp32, fixed
 * summation order), ordered by (distance ascending, row index ascending).  1 <= k <= 64, k <= N.
 * Brute force, sized for tables of a few thousand rows: the context keeps a workspace of Q * N floats (all squared distances; O(Q * N)
 * device memory, reused between calls), and the selection makes k serial passes over a query's N distances — O(Q * N * (E + k)) work. */
int fp_knn_l2(fp_ctx* ctx, const float* d_table, int N, int E, const float* d_queries, int Q, int k, int32_t* d_out_idx, float* d_out_d2,
              void* stream);

/* ---- f-3b: TrackingRefiner correspondences and pose from tracks ------------------------------------------ */
/* TrackingRefiner._compute_3d_points (src/pipeline/estimators/tracking_refiner.py:102-130), batched: which surface sample stands for each
 * patch cell.  d_samples f64 [S,3] object-frame surface samples shared by the B items, d_T f64 [B,16] row-major object -> camera
 * transforms, d_K f64 [B,9], d_cells i32 [B,C,2] the (x, y) patch cells to answer, d_ncells i32 [B] how many of an item's C slots are
 * real -> d_out i32 [B,C]: index of the chosen sample, -1 for a cell no sample projects into and for slots >= d_ncells[b].
 * Per sample, fp64 in this order: Xc = ((T00 x + T01 y) + T02 z) + T03 (Yc, Zc likewise), u' = (K00 Xc + K01 Yc) + K02 Zc (v', w'
 * likewise), u = u'/w', v = v'/w', cell = (floor(u/patch), floor(v/patch)), d2 = (u/patch - floor(u/patch) - 0.5)^2 + (v/patch -
 * floor(v/patch) - 0.5)^2; a sample with non-finite u or v belongs to no cell.  Of a cell's m members the q = ceil(0.25 m) smallest by
 * (d2, sample index) are kept, and of those the minimum by (Zc, d2, sample index) is returned (the reference's argsort -> [:ceil] ->
 * argmin).  Exact selection, no floating-point atomics: two calls give the same bits.  1 <= S <= 2^24, B <= 65535, C <= 2^20. */
int fp_patch_points(fp_ctx* ctx, const double* d_samples, int S, const double* d_T, const double* d_K, const int32_t* d_cells,
                    const int32_t* d_ncells, int B, int C, double patch, int32_t* d_out, void* stream);
/* cv2.solvePnP(p3d, p2d, K, [], flags=SOLVEPNP_EPNP) as called at tracking_refiner.py:173 and scripts/smooth_poses_video.py:182, for all
 * frames of an interval in one call.  d_pts3d f64 [N,3] shared by the B problems, d_pts2d f64 [B,N,2] (the layout of the tracker's
 * pred_tracks), d_vis u8 [B,N] or NULL (non-zero = the point is used), d_K9 f64 [9] (fx, cx, fy, cy are read: no skew), 4 <= N <= 4096
 * -> d_out f64 [B,16] = {R[9] row-major, t[3], mean reprojection error in pixels over the used points, number of used points,
 * status, 0}.  status 0: solved; 1: fewer than 4 used points; 2: the control-point basis is singular (coplanar or coincident points:
 * the smallest eigenvalue of the 3x3 scatter is <= 1e-12 x the largest).  With a non-zero status R, t and the error are NaN and the
 * call still returns FP_OK; such a problem does not disturb its neighbours in the batch.
 * EPnP (Lepetit, Moreno-Noguer, Fua, IJCV 2009) in the variant OpenCV ships, restated (not pinned to OpenCV): image points normalised
 * with K first, control points = centroid + principal axes scaled by sqrt(lambda/n), barycentrics, M^T M over the used points, the
 * eigenvectors of its four smallest eigenvalues, the 6x10 system, three beta initialisations, five Gauss-Newton steps each, sign by
 * positive mean depth, Horn's absolute orientation (3x3 SVD, determinant corrected), the candidate with the smallest mean
 * reprojection error.  All fp64; sums over points are reductions in a fixed tree order: two calls give the same bits. */
int fp_pnp_epnp(fp_ctx* ctx, const double* d_pts3d, const double* d_pts2d, const uint8_t* d_vis, const double* d_K9, int B, int N,
                double* d_out, void* stream);

/* ---- the built-in point tracker: pyramidal Lucas-Kanade with a forward-backward check ------------------------ */
/* A classical stand-in for the learned tracker the reference fetches from torch.hub (CoTracker2): Bouguet's pyramidal Lucas-Kanade, a
 * different kind of tracker with no parity claim against the reference, and not pinned to OpenCV's calcOpticalFlowPyrLK either.  The
 * algorithm is stated in DESIGN.md section 18 and csrc/lk_core.h and pinned to the numpy restatement tests/_lk_ref.py.
 * fp_lk_pyramid: d_frames u8 [T,H,W,3] (RGB) -> d_pyramid f32 [n_floats], the levels back to back, level l = [T, h_l, w_l] with h_0 = H, w_0 = W,
 * h_l = (h_{l-1} + 1) / 2.  Level 0 is Y = (77 R + 150 G + 29 B + 128) >> 8; level l is level l-1 under the separable [1 4 6 4 1] / 16,
 * rows then columns, replicate border, even pixels kept: (((a + e) + 4 (b + d)) + 6 c) / 16 in fp32 without FMA, bit for bit a float32
 * numpy restatement.  `levels` (1..8) is a request: a level whose smaller side is below 2 radius + 1 is dropped with all coarser ones,
 * level 0 always stays; the buffer holds the sum of T h_l w_l floats over the kept levels (ops.lk_layout computes the same sizes).
 * Refused with FP_ERR_INVALID and a message before anything is launched: null pointers, T outside 1..65535, H or W outside 1..16384, T H W above
 * 2^30, radius outside 1..15, levels outside 1..8. */
int fp_lk_pyramid(fp_ctx* ctx, const uint8_t* d_frames, int T, int H, int W, int levels, int radius, float* d_pyramid, void* stream);
/* d_pyramid as written by fp_lk_pyramid with the same T, H, W, levels, radius; d_queries f32 [N,3] = (t, x, y) in pixels of level 0
 * -> d_tracks f32 [T,N,2], d_vis u8 [T,N], d_diag f32 [T,N,4] = {forward-backward distance (px), smaller eigenvalue of G / window
 * pixels, mean |A - B| at the final position, flags} of the chain step that wrote the row (flags: 1 distance above fb_thresh, 2
 * eigenvalue below min_eig, 4 residual above max_residual, 8 outside the image, 16 lost earlier in the chain; the query's own row has
 * zeros and flag 8 when the query lies outside).  Every row is written and every value is finite.
 * A query's frame is int(t) held inside [0, T-1] and non-finite x, y become 0 (callers that want a refusal check on the host, as
 * freepose_amd.tracker does).  The query's row holds (x, y), visible when inside [0, W-1] x [0, H-1].  Chains move frame to frame from
 * t_q to T-1 and to 0: one LK run src -> dst from the chain's position, one back from the result; the step is good when the distance
 * between the returned point and the chain's position is <= fb_thresh, the eigenvalue >= min_eig, the residual <= max_residual and the
 * forward result inside the image; a row is visible when its step is good and the previous row of the chain was visible (loss is
 * sticky; the position is carried on regardless).  One LK run: from the coarsest level down, the (2 radius + 1)^2 window of A around
 * p / 2^l by bilinear sampling (coordinates clamped into the level first, so nothing is read outside the pyramid), gradients as half
 * central differences of such samples, G, exactly `iters` updates v += G^-1 b, then g <- 2 (g + v); a level whose G has a determinant
 * <= 0 or a smaller eigenvalue per pixel below 1e-4 contributes no update.  No early exit.
 * One wave per (query, direction), at most T-1 launches on the stream, no synchronisation; the fp32 pyramid is sampled and everything
 * else done in fp64 (chain positions in a [T,N,2] fp64 workspace of the context: d_tracks holds their float32 roundings, a chain never
 * continues from a rounded value), sums in a fixed order, no atomics: two
 * calls give the same bits.  Refused with FP_ERR_INVALID and a message before anything is launched: what fp_lk_pyramid refuses, N < 0 or
 * above 2^20, iters outside 1..64.  N = 0 does nothing; T = 1 writes the query rows and launches no chain step. */
int fp_lk_track(fp_ctx* ctx, const float* d_pyramid, int T, int H, int W, int levels, const float* d_queries, int N, int radius, int iters,
                float fb_thresh, float min_eig, float max_residual, float* d_tracks, uint8_t* d_vis, float* d_diag, void* stream);

/* ---- video evaluation: velocity errors of pose tracks ------------------------------------------------------ */
/* The scorer of scripts/eval_videos.py:186-208, i.e. src/utils/video_evaluation.py: get_average_rot_errors_dt (:4-11, get_rot_errors and
 * rot_error_in_cframe :37-63), get_average_proj_errors_dt (:25-34, get_translation_errors_proj and project :80-109),
 * get_average_depth_errors_dt (:14-22, get_translation_errors_depth :66-77) and align_object_origins / change_object_origin (:112-155),
 * for M tracks against V ground-truth trajectories in one call.
 * d_est f64 [M,Nmax,12] and d_gt f64 [V,Nmax,12]: per frame R[9] row-major then t[3]; rows past a track's own length are not read.
 * HOST tables (checked before anything is launched, copied before the call returns):
 *   h_meta   i32 [M,20] = {video (row of d_gt), n_frames N, n_sym, flags, dt[16]}; flags bit 0: sym_axis is given (otherwise S = I and
 *            n_sym is not used), bit 1: K is given (otherwise f = sqrt(w^2 + h^2), c = (w/2, h/2)), bit 2: no origin alignment (the
 *            translations are scored as given); only dt[0..D) are read
 *   h_params f64 [M,16] = {est_scale, gt_scale, w, h, sym_axis[3], K[9]}
 * Limits, refused with FP_ERR_INVALID and a message: 2 <= N <= Nmax, 1 <= dt <= N - 1, 1 <= D <= 16, 1 <= n_sym <= 1024, M <= 65535,
 * scales and frame size finite and > 0.
 * Per pair (t1, t2 = t1 + dt), all fp64:
 *   rot   = min over S of |log(R2e R1e^T) - log((R2g S) R1g^T)|, S = exp(sym_axis * a), a = linspace(-pi, pi, n_sym) (the axis is used
 *           as given, not normalised); log: angle atan2(|v|, (tr - 1) / 2) in [0, pi], a series below 1e-3, the axis from the symmetric
 *           part above pi - 1e-2 (csrc/video_eval_core.h)
 *   proj  = |(pi(t2e) - pi(t1e)) - (pi(t2g) - pi(t1g))|, pi(x) = (K x)[:2] / (K x)[2]
 *   depth = |(|t1e| / s_e - |t2e| / s_e) - (|t1g| / s_g - |t2g| / s_g)|
 * where the estimate's translations in proj and depth are first moved to the aligned object origin: per frame x = t_g / |t_g| * |t_e|,
 * o = R_e^T (x - t_e), kept when |o| < est_scale; the mean of the kept o, its length limited to est_scale / 2; t_e <- R_e o + t_e (no
 * frame kept: unchanged).
 * -> d_per_offset f64 [M,D,3]: mean over the N - dt pairs / dt, for (rot, proj, depth); d_final f64 [M,3]: the mean over the D offsets,
 * rot in degrees, proj / sqrt(w^2 + h^2) * 100.  Optional (NULL = not wanted): d_aligned f64 [M,Nmax,3] the moved translations (rows past
 * a track's own length are left as they are), d_pairs f64 [M,D,Nmax,3] the per-pair errors (rows t1 >= N - dt are left as they are).
 * No floating-point atomics, every sum in a fixed order: two calls give the same bits. */
int fp_video_errors(fp_ctx* ctx, const double* d_est, const double* d_gt, const int32_t* h_meta, const double* h_params, int M, int V,
                    int Nmax, int D, double* d_per_offset, double* d_final, double* d_aligned, double* d_pairs, void* stream);

/* ---- BOP scores: pose matching and recall counts for all thresholds at once --------------------------------- */
/* Replaces the per-threshold work of bop_toolkit/scripts/eval_calc_scores.py:275-290, i.e. bop_toolkit_lib/pose_matching.py match_poses
 * (:39-87, one-element errors) under match_poses_scene (:115-159) and the counting of score.py calc_localization_scores (:77-109), which
 * scripts/eval_bop19_pose.py:217-252 runs in one process per (error type, threshold).  One call matches every (scene, image, object)
 * group of an errors directory under all T thresholds.  All tables are DEVICE memory, packed by the host (freepose_amd.evaluation):
 *   d_err      f64 [P]     per group a row-major [E,G] block: rows = the group's estimates in matching order (score descending, ties in
 *                          file order, already cut to n_top), columns = its ground truths in visiting order; already normalised
 *   d_groups   i32 [Gr,4]  {err_offset, E, G, first_gt_row}; E = 0 and G = 0 are legal; the ranges [first_gt_row, + G) are disjoint
 *   d_gt_valid u8  [R]     1 = the ground truth may be matched and counts as a target
 *   d_gt_obj   i32 [R], d_gt_scene i32 [R]  index into the object / scene list (one object and one scene per group; rows outside every
 *                          group are not read and are never matched)
 *   d_th       f64 [T]     thresholds of correctness
 * Per group and threshold: each estimate in turn takes the valid, not yet matched ground truth with the lowest error < th (strict; NaN
 * never matches; equal errors go to the column visited first): the reference's greedy assignment, not an optimal one.
 * -> d_match i32 [T,R] row (within its group) of the estimate matched to each ground truth, or -1; d_tp_obj i32 [T,n_obj] and d_tp_scene
 * i32 [T,n_scene] matched ground truths; d_tar_obj i32 [n_obj] and d_tar_scene i32 [n_scene] targets = valid ground truths per group,
 * at most n_top of them when n_top > 0 (they do not depend on the threshold).
 * Refused with FP_ERR_INVALID and a message before anything is launched: T < 1, negative sizes, n_obj or n_scene < 1, a product with T
 * at or above 2^31, a null table of non-zero size.  A group whose row reaches outside P or R is skipped on the device.
 * Comparisons and integer atomics only: exact, and two calls give the same bits. */
int fp_bop_scores(fp_ctx* ctx, const double* d_err, const int32_t* d_groups, const uint8_t* d_gt_valid, const int32_t* d_gt_obj,
                  const int32_t* d_gt_scene, const double* d_th, int P, int Gr, int R, int T, int n_obj, int n_scene, int n_top,
                  int32_t* d_match, int32_t* d_tp_obj, int32_t* d_tp_scene, int32_t* d_tar_obj, int32_t* d_tar_scene, void* stream);

/* ---- ground-truth info: visibility, boxes, masks per instance; diameter and box per model ------------------- */
/* Replaces the per-instance work of bop_toolkit/scripts/calc_gt_info.py:125-173 and calc_gt_masks.py:107-126 (the toolkit renders with
 * OpenGL and runs numpy over whole images per instance): one fused pass per instance over a rendered depth canvas
 * d_depth_gt f32 [B,Hr,Wr] (fp_rasterize output) and the test depth image of its scene image, d_depth_test f32 [n_img,H,W] (in the unit
 * of the renders) selected by d_img_idx i32 [B].  The image is the window [oy, oy+H) x [ox, ox+W) of the canvas: calc_gt_info.py renders
 * on a 3W x 3H canvas with the principal point shifted by (W, H) (:70-74,116-128: Wr = 3W, Hr = 3H, ox = W, oy = H), calc_gt_masks.py at
 * image size (Wr = W, Hr = H, ox = oy = 0).  d_params f64 [B,8] = {fx, fy, cx, cy, delta, 0, 0, 0} with the IMAGE's intrinsics.
 * d_out i32 [B,12] per instance:
 *   [0] px_count_all    canvas pixels with depth > 0 (:145)
 *   [1] px_count_valid  window pixels with dist_gt > 0 and dist_test > 0 (:149)
 *   [2] px_count_visib  window pixels of visibility.estimate_visib_mask_gt mode bop19 (visibility.py:34-38): distance images as
 *                       misc.depth_im_to_dist_im_fast forms them in fp64 (misc.py:146-167), the float32 difference, delta in float32
 *   [3] 0
 *   [4..7]  min x, min y, max x, max y of the canvas pixels with depth > 0, minus (ox, oy): negative or beyond the image for a truncated
 *           silhouette (:164-167);  [8..11] the same over the visible mask (:172-173).  An empty set leaves {INT32_MAX, INT32_MAX,
 *           INT32_MIN, INT32_MIN}.
 * d_mask u8 [B,H,W] | NULL: 255 where dist_gt > 0 in the window, else 0 (calc_gt_masks.py:110,121); d_mask_visib u8 [B,H,W] | NULL: 255
 * on the visible mask (:113-126).  Every byte of both is written.
 * Refused with FP_ERR_INVALID and a message before anything is launched: a window that leaves the canvas, null stacks, B < 0 or above
 * 65535, n_img < 1, and a d_img_idx outside [0, n_img) (the B indices are copied to the host for this: the call synchronises the
 * stream once).  B = 0 is legal and does nothing.  16-byte loads are used when Wr, W and ox are multiples of 4 and the stacks are
 * 16-byte aligned, a scalar loop otherwise (same answers).  Integer atomics only: every value equals the reference's given the same
 * depth images, and two calls give the same bits. */
int fp_gt_visibility(fp_ctx* ctx, const float* d_depth_gt, int B, int Hr, int Wr, int ox, int oy, const float* d_depth_test, int n_img,
                     int H, int W, const int32_t* d_img_idx, const double* d_params, uint8_t* d_mask, uint8_t* d_mask_visib,
                     int32_t* d_out, void* stream);
/* bop_toolkit_lib/misc.py:289-303 calc_pts_diameter (a Python loop over all point pairs) and the bounding box of
 * scripts/calc_model_info.py:36-37 for M models in one call.  d_pts f64 [n_pts,3]: the vertex clouds back to back; d_ranges i32 [M,2] =
 * {first row, count} per model; d_out f64 [M,8] = {diameter, min x, min y, min z, size x, size y, size z, 0}, size = max - min.
 * Brute force over all pairs in fp64: per pair (dx dx + dy dy) + dz dz with d = p_i - p_j, added left to right without FMA — the value
 * (pts_diff * pts_diff).sum(axis=1) holds — the maximum of the squares, then ONE correctly rounded square root (sqrt is monotone: this
 * is the reference's maximum of square roots).  Tile pairs i-tile <= j-tile, per-block maxima in workspace slots, a final kernel
 * reduces them; no floating-point atomics: bit-exact, and two calls give the same bits.
 * Refused before anything is launched: null tables, M < 0 or above 65535, a range with count = 0 or outside [0, n_pts] (the ranges are
 * copied to the host for this: one stream synchronisation), a model above 2^21 points, more than 2^26 per-block slots in one call
 * (M x t (t + 1) / 2, t = ceil(largest count / 1024)).  M = 0 is legal and does nothing. */
int fp_pts_diameter(fp_ctx* ctx, const double* d_pts, int n_pts, const int32_t* d_ranges, int M, double* d_out, void* stream);

/* ---- measurement helpers (bench.py: HIP-event timing on the launch stream) ----------------------------- */
int fp_timer_create(void** out);
int fp_timer_start(void* timer, void* stream);
int fp_timer_stop(void* timer, void* stream);
int fp_timer_elapsed_ms(void* timer, float* h_ms); /* synchronises on the stop event */
int fp_timer_destroy(void* timer);
/* toggles per-kernel-class event timing inside fp_vit_forward (gemm / attention / other), read back in ms */
int fp_vit_profile(fp_vit* vit, int enable);
int fp_vit_profile_read(fp_vit* vit, float* h_ms_gemm, float* h_ms_attn, float* h_ms_other, double* h_gemm_flops);
/* number of GEMM kernel launches recorded since fp_vit_profile(vit, 1) (events are recorded without host syncs;
 * fp_vit_profile_read synchronises once and sums) */
long fp_vit_profile_gemm_launches(const fp_vit* vit);

#ifdef __cplusplus
}
#endif
#endif /* FREEPOSE_HIP_H */
