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
#include <string.h>

#include <cmath>

#include "../../include/freepose_hip.h"
#include "internal.h"

namespace {

struct ClipBlockW {
    const bf16_t *ln1w = nullptr, *ln1b = nullptr, *inw = nullptr, *inb = nullptr, *outw = nullptr, *outb = nullptr, *ln2w = nullptr,
                 *ln2b = nullptr, *fcw = nullptr, *fcb = nullptr, *pjw = nullptr, *pjb = nullptr;
};

// dst [cols, rows] = src [rows, cols]^T (the projection is stored [width, embed_dim] and applied as x @ proj; the GEMM wants [out, in])
__global__ void transpose_bf16_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int rows, int cols) {
    const size_t total = (size_t)rows * cols;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t c = i / rows, r = i - c * rows;
        dst[i] = src[r * cols + c];
    }
}

}  // namespace

struct fp_clip {
    fp_ctx* ctx = nullptr;
    fp_clip_arch a{};
    int KP = 0;                   // padded patch-embed K
    int head_dim = 0;
    const bf16_t *cls = nullptr, *pos = nullptr, *lnprew = nullptr, *lnpreb = nullptr, *lnpostw = nullptr, *lnpostb = nullptr;
    bf16_t* pe_w = nullptr;       // [width, KP] private padded copy of conv1.weight
    bf16_t* projT = nullptr;      // [embed_dim, width] private transposed copy of proj
    bf16_t* ones = nullptr;       // gamma of the residual epilogue (no LayerScale in CLIP)
    bf16_t* zeros = nullptr;      // bias of the patch and projection GEMMs (neither layer has one)
    bool have_conv = false, have_proj = false;
    std::vector<ClipBlockW> blk;
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
    v->KP = cdiv(3 * arch->patch * arch->patch, 64) * 64;
    const size_t W = arch->width, E = arch->embed_dim, nvec = std::max(W, E);
    if (hipMalloc((void**)&v->pe_w, W * v->KP * 2) != hipSuccess || hipMalloc((void**)&v->projT, E * W * 2) != hipSuccess ||
        hipMalloc((void**)&v->ones, nvec * 2) != hipSuccess || hipMalloc((void**)&v->zeros, nvec * 2) != hipSuccess) {
        fp_set_error("clip_create: hipMalloc failed");
        fp_clip_destroy(v);
        return FP_ERR_HIP;
    }
    std::vector<bf16_t> one(nvec, f2bf(1.0f));
    if (hipMemset(v->pe_w, 0, W * v->KP * 2) != hipSuccess || hipMemset(v->zeros, 0, nvec * 2) != hipSuccess ||
        hipMemcpy(v->ones, one.data(), nvec * 2, hipMemcpyHostToDevice) != hipSuccess) {
        fp_set_error("clip_create: initialising the device buffers failed");
        fp_clip_destroy(v);
        return FP_ERR_HIP;
    }
    *out = v;
    return FP_OK;
}

extern "C" int fp_clip_destroy(fp_clip* v) {
    if (!v) return FP_OK;
    if (v->pe_w) (void)hipFree(v->pe_w);
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
    auto need = [&](size_t n) -> bool {
        if (numel != n) { fp_set_error("clip_set_weight: %s has %zu elements, expected %zu", name, numel, n); return false; }
        return true;
    };
    std::string nm(name);
    if (nm == "conv1.weight") {
        const size_t K = (size_t)3 * a.patch * a.patch;
        if (!need(D * K)) return FP_ERR_INVALID;
        FP_HIP(hipMemcpy2DAsync(v->pe_w, (size_t)v->KP * 2, p, K * 2, K * 2, D, hipMemcpyDeviceToDevice, s));
        v->have_conv = true;
        return FP_OK;
    }
    if (nm == "proj") {
        if (!need(D * E)) return FP_ERR_INVALID;
        hipLaunchKernelGGL(transpose_bf16_kernel, dim3((unsigned)std::min<size_t>((D * E + 255) / 256, 4096)), dim3(256), 0, s, p, v->projT, (int)D, (int)E);
        FP_LAUNCH_CHECK();
        v->have_proj = true;
        return FP_OK;
    }
    if (nm == "class_embedding") { if (!need(D)) return FP_ERR_INVALID; v->cls = p; return FP_OK; }
    if (nm == "positional_embedding") { if (!need((size_t)(1 + a.grid * a.grid) * D)) return FP_ERR_INVALID; v->pos = p; return FP_OK; }
    if (nm == "ln_pre.weight") { if (!need(D)) return FP_ERR_INVALID; v->lnprew = p; return FP_OK; }
    if (nm == "ln_pre.bias") { if (!need(D)) return FP_ERR_INVALID; v->lnpreb = p; return FP_OK; }
    if (nm == "ln_post.weight") { if (!need(D)) return FP_ERR_INVALID; v->lnpostw = p; return FP_OK; }
    if (nm == "ln_post.bias") { if (!need(D)) return FP_ERR_INVALID; v->lnpostb = p; return FP_OK; }
    int bi = -1;
    char rest[64] = {0};
    if (sscanf(name, "transformer.resblocks.%d.%63s", &bi, rest) == 2 && bi >= 0 && bi < a.depth) {
        ClipBlockW& w = v->blk[bi];
        std::string r(rest);
        struct Ent { const char* n; const bf16_t** slot; size_t numel; } tab[] = {
            {"ln_1.weight", &w.ln1w, D}, {"ln_1.bias", &w.ln1b, D},
            {"attn.in_proj_weight", &w.inw, 3 * D * D}, {"attn.in_proj_bias", &w.inb, 3 * D},
            {"attn.out_proj.weight", &w.outw, D * D}, {"attn.out_proj.bias", &w.outb, D},
            {"ln_2.weight", &w.ln2w, D}, {"ln_2.bias", &w.ln2b, D},
            {"mlp.c_fc.weight", &w.fcw, M * D}, {"mlp.c_fc.bias", &w.fcb, M},
            {"mlp.c_proj.weight", &w.pjw, D * M}, {"mlp.c_proj.bias", &w.pjb, D}};
        for (auto& e : tab)
            if (r == e.n) { if (!need(e.numel)) return FP_ERR_INVALID; *e.slot = p; return FP_OK; }
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
    FP_REQUIRE(v->have_conv && v->have_proj && v->cls && v->pos && v->lnprew && v->lnpreb && v->lnpostw && v->lnpostb,
               "clip_encode_image: embedding / ln_pre / ln_post / proj weights not set");
    for (int i = 0; i < a.depth; ++i) {
        const ClipBlockW& w = v->blk[i];
        FP_REQUIRE(w.ln1w && w.ln1b && w.inw && w.inb && w.outw && w.outb && w.ln2w && w.ln2b && w.fcw && w.fcb && w.pjw && w.pjb,
                   "clip_encode_image: weights of block %d not set", i);
    }
    const int D = a.width, P = a.grid * a.grid, n_tok = P + 1;
    const int npad = cdiv(n_tok, 16) * 16;
    const size_t M = (size_t)B * npad;
    FP_REQUIRE(M * (size_t)std::max(a.mlp_dim, 3 * D) * 2 < 0xffffffffull, "clip_encode_image: batch too large for 32-bit tile offsets (B=%d)", B);
    const int Mi = (int)M;

    bf16_t *A0, *X, *Y, *QKV, *AO, *H1, *POOL;
    int rc;
    if ((rc = v->ctx->get("clip.im2col", (size_t)B * P * v->KP * 2, (void**)&A0))) return rc;
    if ((rc = v->ctx->get("clip.x", M * D * 2, (void**)&X))) return rc;
    if ((rc = v->ctx->get("clip.y", M * D * 2, (void**)&Y))) return rc;
    if ((rc = v->ctx->get("clip.qkv", M * 3 * D * 2, (void**)&QKV))) return rc;
    if ((rc = v->ctx->get("clip.ao", M * D * 2, (void**)&AO))) return rc;
    if ((rc = v->ctx->get("clip.h1", M * (size_t)a.mlp_dim * 2, (void**)&H1))) return rc;
    if ((rc = v->ctx->get("clip.pool", (size_t)B * D * 2, (void**)&POOL))) return rc;
    const int nosplit = v->ctx->opt_row_split == 0;
    auto gemm = [&](const bf16_t* Xp, int ldx, const bf16_t* Wp, int K, bf16_t* Cp, int N, const bf16_t* bias, int rows, int epi,
                    const bf16_t* resid) -> int {
        FpGemmArgs g{};
        g.no_split = nosplit;
        int r = v->ctx->sk_scratch(g, s);
        if (r) return r;
        g.X = Xp; g.ldx = ldx; g.W = Wp; g.ldw = K; g.C = Cp; g.ldc = N; g.bias = bias; g.M = rows; g.N = N; g.K = K;
        if (resid) { g.gamma = v->ones; g.resid = resid; g.ldr = N; }
        return fp_gemm_bf16(g, epi, s);
    };

    // ---- normalise + unfold, patch GEMM scattering into the token buffer, class row, ln_pre ----------------------------------------
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, sd[3] = {0.26862954f, 0.26130258f, 0.27577711f};   // clip.py:12
    if ((rc = fp_im2col_norm_ms((const bf16_t*)d_images, A0, B, S, S, a.patch, v->KP, mean, sd, s))) return rc;
    if ((rc = fp_token_init(X, v->cls, v->pos, nullptr, 0, B, n_tok, npad, D, s))) return rc;
    {
        FpGemmArgs g{};
        g.no_split = nosplit;
        if ((rc = v->ctx->sk_scratch(g, s))) return rc;
        g.X = A0; g.ldx = v->KP; g.W = v->pe_w; g.ldw = v->KP; g.C = X; g.ldc = D; g.bias = v->zeros;
        g.M = B * P; g.N = D; g.K = v->KP; g.pos = v->pos + D; g.P = P; g.npad = npad; g.tok_off = 1;
        if ((rc = fp_gemm_bf16(g, FP_EPI_PATCH, s))) return rc;
    }
    if ((rc = fp_layernorm(X, Y, v->lnprew, v->lnpreb, Mi, D, a.ln_eps, 0, 0, 0, s))) return rc;
    bf16_t* R = Y;    // residual stream
    bf16_t* T = X;    // LayerNorm output of the current half block
    const float scale = 1.0f / sqrtf((float)v->head_dim);
    for (int i = 0; i < a.depth; ++i) {
        const ClipBlockW& w = v->blk[i];
        if ((rc = fp_layernorm(R, T, w.ln1w, w.ln1b, Mi, D, a.ln_eps, 0, 0, 0, s))) return rc;
        if ((rc = gemm(T, D, w.inw, D, QKV, 3 * D, w.inb, Mi, FP_EPI_BIAS, nullptr))) return rc;
        if ((rc = fp_attention_hd_fwd(QKV, 3 * D, AO, D, B, a.heads, v->head_dim, n_tok, npad, scale, s))) return rc;
        if ((rc = gemm(AO, D, w.outw, D, R, D, w.outb, Mi, FP_EPI_BIAS_LS_RES, R))) return rc;
        if ((rc = fp_layernorm(R, T, w.ln2w, w.ln2b, Mi, D, a.ln_eps, 0, 0, 0, s))) return rc;
        if ((rc = gemm(T, D, w.fcw, D, H1, a.mlp_dim, w.fcb, Mi, FP_EPI_BIAS_GELU, nullptr))) return rc;
        if ((rc = gemm(H1, a.mlp_dim, w.pjw, a.mlp_dim, R, D, w.pjb, Mi, FP_EPI_BIAS_LS_RES, R))) return rc;
    }
    // ---- ln_post on the class row of every crop, then the projection --------------------------------------------------------------------
    if ((rc = fp_layernorm(R, POOL, v->lnpostw, v->lnpostb, B, D, a.ln_eps, 1, npad, 0, s))) return rc;
    if ((rc = gemm(POOL, D, v->projT, D, (bf16_t*)d_out, a.embed_dim, v->zeros, B, FP_EPI_BIAS, nullptr))) return rc;
    return FP_OK;
}

extern "C" double fp_clip_flops(const fp_clip* v, int B) {
    if (!v) return 0.0;
    const fp_clip_arch& a = v->a;
    const double P = (double)a.grid * a.grid, N = P + 1, D = a.width, Mm = a.mlp_dim;
    const double per_block = 8.0 * N * D * D + 4.0 * N * D * Mm + 4.0 * N * N * D;
    return B * (a.depth * per_block + 2.0 * P * (3.0 * a.patch * a.patch) * D + 2.0 * D * a.embed_dim);
}
