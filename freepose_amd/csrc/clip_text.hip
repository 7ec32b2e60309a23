// CLIP text tower (open_clip TextTransformer / CLIP.encode_text: token + positional embedding, pre-LayerNorm blocks under a causal
// mask, ln_final on the end-of-text token, linear projection), gfx950 only.
// Reference op replaced: `clip.model.encode_text(text)` of GPT4ScaleEstimator.generate_clip_features (src/pipeline/estimators/
// scale_estimators.py:91-94) on a module cast to bf16, i.e. every module output is rounded to bf16.  open_clip itself is not part of the
// reference tree: the state-dict names and the structure below are the public ones of its text transformer.
//
//   x[b,t] = token_embedding[ids[b,t]] + positional_embedding[t]                                    (bf16 add, rounded)
//   depth x { x + out_proj(causal_attn(ln_1 x)) ; x + c_proj(gelu(c_fc(ln_2 x))) }
//   pooled[b] = ln_final(x[b, argmax_t ids[b,t]])  ->  @ text_projection                             (first maximum)
//
// ln_final works per row, so normalising only the pooled row equals open_clip's "normalise every row, then index".  Built from the pieces
// of the image tower (tower_steps.h, the bf16 GEMM tiers, the LayerNorm kernel) plus attention_causal.hip and the two gathers below.
#include <stdio.h>

#include <cmath>

#include "../../include/freepose_hip.h"
#include "tower_steps.h"

namespace {

// X[b * npad + t] = bf16(tok[ids[b,t]] + pos[t]) for t < ctx, zeros for the pad rows [ctx, npad).  An id outside [0, vocab) never
// reaches the table: its row is zeros and *bad is raised (the host refuses the call).  One 16-byte chunk of 8 features per thread.
__global__ __launch_bounds__(256) void text_embed_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ tok, const bf16_t* __restrict__ pos,
                                                         bf16_t* __restrict__ X, int B, int ctx, int npad, int D, int vocab, int* __restrict__ bad) {
    const int chunks = D / 8;
    const size_t total = (size_t)B * npad * chunks;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t row = i / chunks;
        const int c = (int)(i - row * chunks), b = (int)(row / npad), t = (int)(row - (size_t)b * npad);
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (t < ctx) {
            const int id = ids[(size_t)b * ctx + t];
            if (id >= 0 && id < vocab) {
                const uint4 e = *(const uint4*)(tok + (size_t)id * D + 8 * c), q = *(const uint4*)(pos + (size_t)t * D + 8 * c);
                w.x = pack_bf2(lo_bf(e.x) + lo_bf(q.x), hi_bf(e.x) + hi_bf(q.x));
                w.y = pack_bf2(lo_bf(e.y) + lo_bf(q.y), hi_bf(e.y) + hi_bf(q.y));
                w.z = pack_bf2(lo_bf(e.z) + lo_bf(q.z), hi_bf(e.z) + hi_bf(q.z));
                w.w = pack_bf2(lo_bf(e.w) + lo_bf(q.w), hi_bf(e.w) + hi_bf(q.w));
            } else if (c == 0) {
                atomicOr(bad, 1);
            }
        }
        *(uint4*)(X + row * D + 8 * c) = w;
    }
}

// OUT[b] = X[b * npad + argmax_t ids[b,t]] (the first maximum: open_clip's text.argmax(dim=-1), the end-of-text token having the
// largest id of the vocabulary).  One workgroup per prompt; every thread finds the row on its own (ctx loads from one cached line run).
__global__ __launch_bounds__(256) void text_pool_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ X, bf16_t* __restrict__ OUT,
                                                        int ctx, int npad, int D) {
    const int b = blockIdx.x;
    const int* row = ids + (size_t)b * ctx;
    int best = row[0], at = 0;
    for (int t = 1; t < ctx; ++t) {
        const int v = row[t];
        if (v > best) { best = v; at = t; }
    }
    const uint4* src = (const uint4*)(X + ((size_t)b * npad + at) * D);
    uint4* dst = (uint4*)(OUT + (size_t)b * D);
    for (int c = threadIdx.x; c < D / 8; c += blockDim.x) dst[c] = src[c];
}

// dst [cols, rows] = src [rows, cols]^T (text_projection is stored [width, embed_dim] and applied as x @ P; the GEMM wants [out, in])
__global__ void text_transpose_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int rows, int cols) {
    const size_t total = (size_t)rows * cols;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t c = i / rows, r = i - c * rows;
        dst[i] = src[r * cols + c];
    }
}

}  // namespace

struct fp_clip_text {
    fp_ctx* ctx = nullptr;
    fp_clip_text_arch a{};
    int head_dim = 0, npad = 0;
    const bf16_t *tok = nullptr, *pos = nullptr, *lnfw = nullptr, *lnfb = nullptr;
    bf16_t* projT = nullptr;      // [embed_dim, width] private transposed copy of text_projection
    bf16_t* ones = nullptr;       // gamma of the residual epilogue (no LayerScale in CLIP)
    bf16_t* zeros = nullptr;      // bias of the projection GEMM (the layer has none)
    int* bad = nullptr;           // raised by the embedding gather on an id outside the vocabulary
    bool have_proj = false;
    std::vector<TowerBlockW> blk;
};

extern "C" int fp_clip_text_create(fp_ctx* ctx, const fp_clip_text_arch* arch, fp_clip_text** out) {
    FP_REQUIRE(ctx && arch && out, "clip_text_create: null argument");
    FP_REQUIRE(arch->width > 0 && arch->width % 64 == 0 && arch->heads > 0 && arch->width % arch->heads == 0,
               "clip_text_create: width=%d heads=%d (width must be a multiple of 64 and of heads)", arch->width, arch->heads);
    const int hd = arch->width / arch->heads;
    FP_REQUIRE(hd % 8 == 0 && hd >= 8 && hd <= 128, "clip_text_create: head dimension %d (must be a multiple of 8 in [8, 128])", hd);
    FP_REQUIRE(arch->width <= 2048, "clip_text_create: width=%d exceeds the LayerNorm kernel (2048)", arch->width);
    FP_REQUIRE(arch->mlp_dim > 0 && arch->mlp_dim % 64 == 0 && arch->embed_dim > 0 && arch->embed_dim % 16 == 0 && arch->depth > 0 &&
                   arch->vocab > 0 && arch->ctx > 0, "clip_text_create: bad arch (mlp_dim %% 64, embed_dim %% 16, depth, vocab, ctx)");
    fp_clip_text* v = new fp_clip_text();
    v->ctx = ctx;
    v->a = *arch;
    v->head_dim = hd;
    v->npad = cdiv(arch->ctx, 16) * 16;
    v->blk.resize(arch->depth);
    const size_t W = arch->width, E = arch->embed_dim, nvec = std::max(W, E);
    if (hipMalloc((void**)&v->projT, E * W * 2) != hipSuccess || hipMalloc((void**)&v->ones, nvec * 2) != hipSuccess ||
        hipMalloc((void**)&v->zeros, nvec * 2) != hipSuccess || hipMalloc((void**)&v->bad, sizeof(int)) != hipSuccess) {
        fp_set_error("clip_text_create: hipMalloc failed");
        fp_clip_text_destroy(v);
        return FP_ERR_HIP;
    }
    std::vector<bf16_t> one(nvec, f2bf(1.0f));
    if (hipMemset(v->zeros, 0, nvec * 2) != hipSuccess || hipMemset(v->bad, 0, sizeof(int)) != hipSuccess ||
        hipMemcpy(v->ones, one.data(), nvec * 2, hipMemcpyHostToDevice) != hipSuccess) {
        fp_set_error("clip_text_create: initialising the device buffers failed");
        fp_clip_text_destroy(v);
        return FP_ERR_HIP;
    }
    *out = v;
    return FP_OK;
}

extern "C" int fp_clip_text_destroy(fp_clip_text* v) {
    if (!v) return FP_OK;
    if (v->projT) (void)hipFree(v->projT);
    if (v->ones) (void)hipFree(v->ones);
    if (v->zeros) (void)hipFree(v->zeros);
    if (v->bad) (void)hipFree(v->bad);
    delete v;
    return FP_OK;
}

extern "C" int fp_clip_text_set_weight(fp_clip_text* v, const char* name, const void* d, size_t numel, void* stream) {
    FP_REQUIRE(v && name && d, "clip_text_set_weight: null argument");
    const fp_clip_text_arch& a = v->a;
    const bf16_t* p = (const bf16_t*)d;
    const size_t D = a.width, M = a.mlp_dim, E = a.embed_dim;
    hipStream_t s = (hipStream_t)stream;
    if (!strcmp(name, "text_projection")) {
        if (!fp_weight_numel("clip_text_set_weight", name, numel, D * E)) return FP_ERR_INVALID;
        hipLaunchKernelGGL(text_transpose_kernel, dim3((unsigned)std::min<size_t>((D * E + 255) / 256, 4096)), dim3(256), 0, s, p, v->projT, (int)D, (int)E);
        FP_LAUNCH_CHECK();
        v->have_proj = true;
        return FP_OK;
    }
    const WeightEnt top[] = {{"token_embedding.weight", &v->tok, (size_t)a.vocab * D}, {"positional_embedding", &v->pos, (size_t)a.ctx * D},
                             {"ln_final.weight", &v->lnfw, D}, {"ln_final.bias", &v->lnfb, D}};
    if (const int hit = fp_set_named_weight("clip_text_set_weight", name, name, top, p, numel)) return hit > 0 ? FP_OK : FP_ERR_INVALID;
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
        if (const int hit = fp_set_named_weight("clip_text_set_weight", name, rest, tab, p, numel)) return hit > 0 ? FP_OK : FP_ERR_INVALID;
    }
    fp_set_error("clip_text_set_weight: unknown tensor name '%s'", name);
    return FP_ERR_INVALID;
}

extern "C" int fp_clip_text_encode(fp_clip_text* v, const int32_t* d_ids, int B, void* d_out, void* stream) {
    FP_REQUIRE(v && d_ids && d_out, "clip_text_encode: null argument");
    const fp_clip_text_arch& a = v->a;
    hipStream_t s = (hipStream_t)stream;
    FP_REQUIRE(B > 0, "clip_text_encode: B=%d", B);
    FP_REQUIRE(v->have_proj && v->tok && v->pos && v->lnfw && v->lnfb, "clip_text_encode: embedding / ln_final / text_projection weights not set");
    for (int i = 0; i < a.depth; ++i) {
        FP_REQUIRE(v->blk[i].complete(), "clip_text_encode: weights of block %d not set", i);
    }
    const int D = a.width, n_tok = a.ctx, npad = v->npad;
    const size_t M = (size_t)B * npad;
    FP_REQUIRE(M * (size_t)std::max(a.mlp_dim, 3 * D) * 2 < 0xffffffffull, "clip_text_encode: batch too large for 32-bit tile offsets (B=%d)", B);
    const int Mi = (int)M;

    bf16_t *X, *Y, *QKV, *AO, *H1, *POOL, *POOLN;
    int rc;
    fp_ctx* ctx = v->ctx;
    FP_WS(ctx, "clip_text.x", M * D * 2, X);
    FP_WS(ctx, "clip_text.y", M * D * 2, Y);
    FP_WS(ctx, "clip_text.qkv", M * 3 * D * 2, QKV);
    FP_WS(ctx, "clip_text.ao", M * D * 2, AO);
    FP_WS(ctx, "clip_text.h1", M * (size_t)a.mlp_dim * 2, H1);
    FP_WS(ctx, "clip_text.pool", (size_t)B * D * 2, POOL);
    FP_WS(ctx, "clip_text.pooln", (size_t)B * D * 2, POOLN);

    // ---- token + positional embedding; an id outside the vocabulary ends the call before the tower runs ----------------------------------
    {
        const size_t total = M * (size_t)(D / 8);
        hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 8192)), dim3(256), 0, s, d_ids, v->tok, v->pos, X, B, n_tok,
                           npad, D, a.vocab, v->bad);
        FP_LAUNCH_CHECK();
        int bad = 0;
        FP_HIP(hipMemcpyAsync(&bad, v->bad, sizeof(int), hipMemcpyDeviceToHost, s));
        FP_HIP(hipStreamSynchronize(s));
        if (bad) {
            FP_HIP(hipMemsetAsync(v->bad, 0, sizeof(int), s));
            fp_set_error("clip_text_encode: a token id lies outside the vocabulary [0, %d)", a.vocab);
            return FP_ERR_INVALID;
        }
    }
    bf16_t* R = X;    // residual stream
    bf16_t* T = Y;    // LayerNorm output of the current half block
    const TowerRun t{ctx, nullptr, s, B, n_tok, npad, D, a.mlp_dim, a.ln_eps, R, T, AO, H1, v->ones};
    const float scale = 1.0f / sqrtf((float)v->head_dim);
    for (int i = 0; i < a.depth; ++i) {
        const TowerBlockW& w = v->blk[i];
        if ((rc = fp_layernorm(R, T, w.n1w, w.n1b, Mi, D, a.ln_eps, 0, 0, 0, s))) return rc;
        if ((rc = GemmStep(T, D, w.qkvw, D, QKV, 3 * D, w.qkvb, Mi, 3 * D).run(ctx, s))) return rc;
        if ((rc = fp_attention_causal_fwd(QKV, 3 * D, AO, D, B, a.heads, v->head_dim, n_tok, npad, scale, s))) return rc;
        if ((rc = fp_tower_out_proj(t, w, nullptr))) return rc;
        if ((rc = fp_tower_mlp(t, w, nullptr, nullptr, nullptr, nullptr))) return rc;
    }
    // ---- the end-of-text row of every prompt, ln_final, then the projection ---------------------------------------------------------------
    hipLaunchKernelGGL(text_pool_kernel, dim3(B), dim3(256), 0, s, d_ids, R, POOL, n_tok, npad, D);
    FP_LAUNCH_CHECK();
    if ((rc = fp_layernorm(POOL, POOLN, v->lnfw, v->lnfb, B, D, a.ln_eps, 0, 0, 0, s))) return rc;
    return GemmStep(POOLN, D, v->projT, D, (bf16_t*)d_out, a.embed_dim, v->zeros, B, a.embed_dim).run(ctx, s);
}

extern "C" double fp_clip_text_flops(const fp_clip_text* v, int B) {
    if (!v) return 0.0;
    const fp_clip_text_arch& a = v->a;
    const double N = a.ctx, D = a.width, Mm = a.mlp_dim;
    const double per_block = 8.0 * N * D * D + 4.0 * N * D * Mm + 2.0 * N * (N + 1) * D;   // the causal half of 4 N^2 D
    return B * (a.depth * per_block + 2.0 * D * a.embed_dim);
}
