// CLIP visual tower (open_clip VisionTransformer: pre-LayerNorm, no LayerScale, class-token pooling, linear projection), gfx950 only.
// Reference op replaced: `self.model.encode_image(self.transform(images))` of CLIPFeatureExtractor (src/pipeline/retrieval/clip.py:15-18)
// on a module cast to bf16, i.e. every module output is rounded to bf16.  open_clip itself is not part of the reference tree: the
// state-dict names and the block structure below are the public ones of its VisionTransformer.
//
//   normalise (CLIP mean / std) + patch unfold -> conv1 as a GEMM (no bias) -> [class; patches] + positional_embedding -> ln_pre ->
//   depth x { x + out_proj(attn(ln_1 x)) ; x + c_proj(gelu(c_fc(ln_2 x))) } -> ln_post(class row) -> @ proj
//
// Built from the existing pieces: the bf16 GEMM tiers with the BIAS / BIAS_GELU / BIAS_LS_RES (gamma = 1) / PATCH (bias = 0) epilogues,
// the LayerNorm kernel, token_init with no register tokens, and attention_hd.hip (ViT-bigG/14 has 16 heads of 104).  The LayerNorm-folded
// GEMM route of the DINOv2 driver is not used: its statistics kernel stops at 1536 features.
#include <stdio.h>

#include <cmath>

#include "../../include/freepose_hip.h"
#include "tower_steps.h"

namespace {

// dst [cols, rows] = src [rows, cols]^T (the projection is stored [width, embed_dim] and applied as x @ proj; the GEMM wants [out, in])
__global__ void transpose_bf16_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int rows, int cols) {
    const size_t total = (size_t)rows * cols;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t c = i / rows, r = i - c * rows;
        dst[i] = src[r * cols + c];
    }
}

constexpr float CLIP_MEAN[3] = {0.48145466f, 0.4578275f, 0.40821073f}, CLIP_SD[3] = {0.26862954f, 0.26130258f, 0.27577711f};   // clip.py:12

}  // namespace

struct fp_clip {
    fp_ctx* ctx = nullptr;
    fp_clip_arch a{};
    TowerEmbedW emb;              // no bias (zeros), no register tokens
    int head_dim = 0;
    const bf16_t *lnprew = nullptr, *lnpreb = nullptr, *lnpostw = nullptr, *lnpostb = nullptr;
    bf16_t* projT = nullptr;      // [embed_dim, width] private transposed copy of proj
    bf16_t* ones = nullptr;       // gamma of the residual epilogue (no LayerScale in CLIP)
    bf16_t* zeros = nullptr;      // bias of the patch and projection GEMMs (neither layer has one)
    bool have_conv = false, have_proj = false;
    std::vector<TowerBlockW> blk;
};

extern "C" int fp_clip_create(fp_ctx* ctx, const fp_clip_arch* arch, fp_clip** out) {
    FP_REQUIRE(ctx && arch && out, "clip_create: null argument");
    FP_REQUIRE(arch->quick_gelu == 0, "clip_create: quick_gelu towers are not provided (exact-erf GELU only)");
    FP_REQUIRE(arch->width > 0 && arch->width % 64 == 0 && arch->heads > 0 && arch->width % arch->heads == 0,
               "clip_create: width=%d heads=%d (width must be a multiple of 64 and of heads)", arch->width, arch->heads);
    const int hd = arch->width / arch->heads;
    FP_REQUIRE(hd % 8 == 0 && hd >= 8 && hd <= 128, "clip_create: head dimension %d (must be a multiple of 8 in [8, 128])", hd);
    FP_REQUIRE(arch->width <= 2048, "clip_create: width=%d exceeds the LayerNorm kernel (2048)", arch->width);
    FP_REQUIRE(arch->mlp_dim > 0 && arch->mlp_dim % 64 == 0 && arch->embed_dim > 0 && arch->embed_dim % 16 == 0 && arch->depth > 0 &&
                   arch->patch > 0 && arch->grid > 0, "clip_create: bad arch (mlp_dim %% 64, embed_dim %% 16, depth, patch, grid)");
    fp_clip* v = new fp_clip();
    v->ctx = ctx;
    v->a = *arch;
    v->head_dim = hd;
    v->blk.resize(arch->depth);
    v->emb.patch = arch->patch; v->emb.mean = CLIP_MEAN; v->emb.sd = CLIP_SD;
    v->emb.KP = cdiv(3 * arch->patch * arch->patch, 64) * 64;
    const size_t W = arch->width, E = arch->embed_dim, nvec = std::max(W, E);
    if (hipMalloc((void**)&v->emb.pe_w, W * v->emb.KP * 2) != hipSuccess || hipMalloc((void**)&v->projT, E * W * 2) != hipSuccess ||
        hipMalloc((void**)&v->ones, nvec * 2) != hipSuccess || hipMalloc((void**)&v->zeros, nvec * 2) != hipSuccess) {
        fp_set_error("clip_create: hipMalloc failed");
        fp_clip_destroy(v);
        return FP_ERR_HIP;
    }
    std::vector<bf16_t> one(nvec, f2bf(1.0f));
    if (hipMemset(v->emb.pe_w, 0, W * v->emb.KP * 2) != hipSuccess || hipMemset(v->zeros, 0, nvec * 2) != hipSuccess ||
        hipMemcpy(v->ones, one.data(), nvec * 2, hipMemcpyHostToDevice) != hipSuccess) {
        fp_set_error("clip_create: initialising the device buffers failed");
        fp_clip_destroy(v);
        return FP_ERR_HIP;
    }
    v->emb.pe_b = v->zeros;
    *out = v;
    return FP_OK;
}

extern "C" int fp_clip_destroy(fp_clip* v) {
    if (!v) return FP_OK;
    if (v->emb.pe_w) (void)hipFree(v->emb.pe_w);
    if (v->projT) (void)hipFree(v->projT);
    if (v->ones) (void)hipFree(v->ones);
    if (v->zeros) (void)hipFree(v->zeros);
    delete v;
    return FP_OK;
}

extern "C" int fp_clip_set_weight(fp_clip* v, const char* name, const void* d, size_t numel, void* stream) {
    FP_REQUIRE(v && name && d, "clip_set_weight: null argument");
    const fp_clip_arch& a = v->a;
    const bf16_t* p = (const bf16_t*)d;
    const size_t D = a.width, M = a.mlp_dim, E = a.embed_dim;
    hipStream_t s = (hipStream_t)stream;
    std::string nm(name);
    if (nm == "conv1.weight") {
        const int rc = fp_tower_set_patch_weight("clip_set_weight", name, p, numel, v->emb, D, s);
        v->have_conv |= rc == FP_OK;
        return rc;
    }
    if (nm == "proj") {
        if (!fp_weight_numel("clip_set_weight", name, numel, D * E)) return FP_ERR_INVALID;
        hipLaunchKernelGGL(transpose_bf16_kernel, dim3((unsigned)std::min<size_t>((D * E + 255) / 256, 4096)), dim3(256), 0, s, p, v->projT, (int)D, (int)E);
        FP_LAUNCH_CHECK();
        v->have_proj = true;
        return FP_OK;
    }
    const WeightEnt top[] = {{"class_embedding", &v->emb.cls, D}, {"positional_embedding", &v->emb.pos, (size_t)(1 + a.grid * a.grid) * D},
                             {"ln_pre.weight", &v->lnprew, D}, {"ln_pre.bias", &v->lnpreb, D}, {"ln_post.weight", &v->lnpostw, D},
                             {"ln_post.bias", &v->lnpostb, D}};
    if (const int hit = fp_set_named_weight("clip_set_weight", name, name, top, p, numel)) return hit > 0 ? FP_OK : FP_ERR_INVALID;
    int bi = -1;
    char rest[64] = {0};
    if (sscanf(name, "transformer.resblocks.%d.%63s", &bi, rest) == 2 && bi >= 0 && bi < a.depth) {
        TowerBlockW& w = v->blk[bi];
        const WeightEnt tab[] = {
            {"ln_1.weight", &w.n1w, D}, {"ln_1.bias", &w.n1b, D},
            {"attn.in_proj_weight", &w.qkvw, 3 * D * D}, {"attn.in_proj_bias", &w.qkvb, 3 * D},
            {"attn.out_proj.weight", &w.projw, D * D}, {"attn.out_proj.bias", &w.projb, D},
            {"ln_2.weight", &w.n2w, D}, {"ln_2.bias", &w.n2b, D},
            {"mlp.c_fc.weight", &w.fc1w, M * D}, {"mlp.c_fc.bias", &w.fc1b, M},
            {"mlp.c_proj.weight", &w.fc2w, D * M}, {"mlp.c_proj.bias", &w.fc2b, D}};
        if (const int hit = fp_set_named_weight("clip_set_weight", name, rest, tab, p, numel)) return hit > 0 ? FP_OK : FP_ERR_INVALID;
    }
    fp_set_error("clip_set_weight: unknown tensor name '%s'", name);
    return FP_ERR_INVALID;
}

extern "C" int fp_clip_encode_image(fp_clip* v, const void* d_images, int B, int S, void* d_out, void* stream) {
    FP_REQUIRE(v && d_images && d_out, "clip_encode_image: null argument");
    const fp_clip_arch& a = v->a;
    hipStream_t s = (hipStream_t)stream;
    FP_REQUIRE(B > 0, "clip_encode_image: B=%d", B);
    FP_REQUIRE(S == a.patch * a.grid, "clip_encode_image: images are %d x %d, the tower takes %d x %d (patch %d, grid %d: the positional "
               "embedding is not interpolated)", S, S, a.patch * a.grid, a.patch * a.grid, a.patch, a.grid);
    FP_REQUIRE(v->have_conv && v->have_proj && v->emb.cls && v->emb.pos && v->lnprew && v->lnpreb && v->lnpostw && v->lnpostb,
               "clip_encode_image: embedding / ln_pre / ln_post / proj weights not set");
    for (int i = 0; i < a.depth; ++i) {
        FP_REQUIRE(v->blk[i].complete(), "clip_encode_image: weights of block %d not set", i);
    }
    const int D = a.width, P = a.grid * a.grid, n_tok = P + 1;
    const int npad = cdiv(n_tok, 16) * 16;
    const size_t M = (size_t)B * npad;
    FP_REQUIRE(M * (size_t)std::max(a.mlp_dim, 3 * D) * 2 < 0xffffffffull, "clip_encode_image: batch too large for 32-bit tile offsets (B=%d)", B);
    const int Mi = (int)M;

    bf16_t *A0, *X, *Y, *QKV, *AO, *H1, *POOL;
    int rc;
    fp_ctx* ctx = v->ctx;
    FP_WS(ctx, "clip.im2col", (size_t)B * P * v->emb.KP * 2, A0);
    FP_WS(ctx, "clip.x", M * D * 2, X);
    FP_WS(ctx, "clip.y", M * D * 2, Y);
    FP_WS(ctx, "clip.qkv", M * 3 * D * 2, QKV);
    FP_WS(ctx, "clip.ao", M * D * 2, AO);
    FP_WS(ctx, "clip.h1", M * (size_t)a.mlp_dim * 2, H1);
    FP_WS(ctx, "clip.pool", (size_t)B * D * 2, POOL);

    bf16_t* R = Y;    // residual stream
    bf16_t* T = X;    // LayerNorm output of the current half block
    const TowerRun t{ctx, nullptr, s, B, n_tok, npad, D, a.mlp_dim, a.ln_eps, R, T, AO, H1, v->ones};
    // ---- normalise + unfold, patch GEMM scattering into the token buffer, class row, ln_pre ----------------------------------------
    if ((rc = fp_tower_embed(t, v->emb, v->emb.pos + D, (const bf16_t*)d_images, S, S, A0, X))) return rc;
    if ((rc = fp_layernorm(X, Y, v->lnprew, v->lnpreb, Mi, D, a.ln_eps, 0, 0, 0, s))) return rc;
    const float scale = 1.0f / sqrtf((float)v->head_dim);
    for (int i = 0; i < a.depth; ++i) {
        const TowerBlockW& w = v->blk[i];
        if ((rc = fp_layernorm(R, T, w.n1w, w.n1b, Mi, D, a.ln_eps, 0, 0, 0, s))) return rc;
        if ((rc = GemmStep(T, D, w.qkvw, D, QKV, 3 * D, w.qkvb, Mi, 3 * D).run(ctx, s))) return rc;
        if ((rc = fp_attention_hd_fwd(QKV, 3 * D, AO, D, B, a.heads, v->head_dim, n_tok, npad, scale, s))) return rc;
        if ((rc = fp_tower_out_proj(t, w, nullptr))) return rc;
        if ((rc = fp_tower_mlp(t, w, nullptr, nullptr, nullptr, nullptr))) return rc;
    }
    // ---- ln_post on the class row of every crop, then the projection --------------------------------------------------------------------
    if ((rc = fp_layernorm(R, POOL, v->lnpostw, v->lnpostb, B, D, a.ln_eps, 1, npad, 0, s))) return rc;
    return GemmStep(POOL, D, v->projT, D, (bf16_t*)d_out, a.embed_dim, v->zeros, B, a.embed_dim).run(ctx, s);
}

extern "C" double fp_clip_flops(const fp_clip* v, int B) {
    if (!v) return 0.0;
    const fp_clip_arch& a = v->a;
    const double P = (double)a.grid * a.grid, N = P + 1, D = a.width, Mm = a.mlp_dim;
    const double per_block = 8.0 * N * D * D + 4.0 * N * D * Mm + 4.0 * N * N * D;
    return B * (a.depth * per_block + 2.0 * P * (3.0 * a.patch * a.patch) * D + 2.0 * D * a.embed_dim);
}
