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
#include "../../include/freepose_hip.h"
#include "tower_steps.h"

namespace {

constexpr float CLIP_MEAN[3] = {0.48145466f, 0.4578275f, 0.40821073f}, CLIP_SD[3] = {0.26862954f, 0.26130258f, 0.27577711f};   // clip.py:12

}  // namespace

struct fp_clip {
    fp_ctx* ctx = nullptr;
    fp_clip_arch a{};
    TowerEmbedW emb;              // no bias (the tower's zeros), no register tokens
    const bf16_t *lnprew = nullptr, *lnpreb = nullptr, *lnpostw = nullptr, *lnpostb = nullptr;
    bool have_conv = false;
    ClipTowerCommon tw;           // proj transposed, ones / zeros, the blocks
};

extern "C" int fp_clip_create(fp_ctx* ctx, const fp_clip_arch* arch, fp_clip** out) {
    FP_REQUIRE(ctx && arch && out, "clip_create: null argument");
    FP_REQUIRE(arch->quick_gelu == 0, "clip_create: quick_gelu towers are not provided (exact-erf GELU only)");
    if (int rc = ClipTowerCommon::check_arch("clip_create", arch->width, arch->heads, arch->mlp_dim, arch->embed_dim, arch->depth,
                                             arch->patch > 0 && arch->grid > 0, "patch, grid")) return rc;
    fp_clip* v = new fp_clip();
    v->ctx = ctx;
    v->a = *arch;
    v->emb.patch = arch->patch; v->emb.mean = CLIP_MEAN; v->emb.sd = CLIP_SD;
    v->emb.KP = cdiv(3 * arch->patch * arch->patch, 64) * 64;
    const size_t pe_bytes = (size_t)arch->width * v->emb.KP * 2;
    int rc = v->tw.alloc("clip_create", arch->width, arch->heads, arch->embed_dim, arch->depth);
    if (!rc && hipMalloc((void**)&v->emb.pe_w, pe_bytes) != hipSuccess) {
        fp_set_error("clip_create: hipMalloc failed");
        rc = FP_ERR_HIP;
    }
    if (!rc && hipMemset(v->emb.pe_w, 0, pe_bytes) != hipSuccess) {
        fp_set_error("clip_create: initialising the device buffers failed");
        rc = FP_ERR_HIP;
    }
    if (rc) {
        fp_clip_destroy(v);
        return rc;
    }
    v->emb.pe_b = v->tw.zeros;
    *out = v;
    return FP_OK;
}

extern "C" int fp_clip_destroy(fp_clip* v) {
    if (!v) return FP_OK;
    if (v->emb.pe_w) (void)hipFree(v->emb.pe_w);
    v->tw.free();
    delete v;
    return FP_OK;
}

extern "C" int fp_clip_set_weight(fp_clip* v, const char* name, const void* d, size_t numel, void* stream) {
    FP_REQUIRE(v && name && d, "clip_set_weight: null argument");
    const fp_clip_arch& a = v->a;
    const bf16_t* p = (const bf16_t*)d;
    const size_t D = a.width, M = a.mlp_dim, E = a.embed_dim;
    hipStream_t s = (hipStream_t)stream;
    if (!strcmp(name, "conv1.weight")) {
        const int rc = fp_tower_set_patch_weight("clip_set_weight", name, p, numel, v->emb, D, s);
        v->have_conv |= rc == FP_OK;
        return rc;
    }
    if (!strcmp(name, "proj")) return v->tw.set_proj("clip_set_weight", name, p, numel, D, E, s);
    const WeightEnt top[] = {{"class_embedding", &v->emb.cls, D}, {"positional_embedding", &v->emb.pos, (size_t)(1 + a.grid * a.grid) * D},
                             {"ln_pre.weight", &v->lnprew, D}, {"ln_pre.bias", &v->lnpreb, D}, {"ln_post.weight", &v->lnpostw, D},
                             {"ln_post.bias", &v->lnpostb, D}};
    int hit = fp_set_named_weight("clip_set_weight", name, name, top, p, numel);
    if (!hit) hit = fp_tower_resblock_weight("clip_set_weight", name, v->tw.blk, D, M, p, numel);
    if (hit) return hit > 0 ? FP_OK : FP_ERR_INVALID;
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
    FP_REQUIRE(v->have_conv && v->tw.have_proj && v->emb.cls && v->emb.pos && v->lnprew && v->lnpreb && v->lnpostw && v->lnpostb,
               "clip_encode_image: embedding / ln_pre / ln_post / proj weights not set");
    int rc;
    if ((rc = v->tw.all_blocks_complete("clip_encode_image"))) return rc;
    const int D = a.width, P = a.grid * a.grid, n_tok = P + 1;
    const int npad = cdiv(n_tok, 16) * 16;
    const size_t M = (size_t)B * npad;
    if ((rc = fp_tower_offsets_fit("clip_encode_image", M, D, a.mlp_dim, B))) return rc;

    bf16_t *A0, *X, *Y, *QKV, *AO, *H1, *POOL;
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
    const TowerRun t{ctx, nullptr, s, B, n_tok, npad, D, a.mlp_dim, a.ln_eps, R, T, AO, H1, v->tw.ones};
    // ---- normalise + unfold, patch GEMM scattering into the token buffer, class row, ln_pre ----------------------------------------
    if ((rc = fp_tower_embed(t, v->emb, v->emb.pos + D, (const bf16_t*)d_images, S, S, A0, X))) return rc;
    if ((rc = fp_layernorm(X, Y, v->lnprew, v->lnpreb, (int)M, D, a.ln_eps, 0, 0, 0, s))) return rc;
    if ((rc = fp_tower_blocks(t, v->tw.blk, QKV, a.heads, v->tw.head_dim, /*causal=*/false))) return rc;
    // ---- ln_post on the class row of every crop, then the projection --------------------------------------------------------------------
    if ((rc = fp_layernorm(R, POOL, v->lnpostw, v->lnpostb, B, D, a.ln_eps, 1, npad, 0, s))) return rc;
    return v->tw.project(ctx, POOL, D, a.embed_dim, d_out, B, s);
}

extern "C" double fp_clip_flops(const fp_clip* v, int B) {
    if (!v) return 0.0;
    const fp_clip_arch& a = v->a;
    const double P = (double)a.grid * a.grid, N = P + 1, D = a.width, Mm = a.mlp_dim;
    const double per_block = 8.0 * N * D * D + 4.0 * N * D * Mm + 4.0 * N * N * D;
    return B * (a.depth * per_block + 2.0 * P * (3.0 * a.patch * a.patch) * D + 2.0 * D * a.embed_dim);
}
