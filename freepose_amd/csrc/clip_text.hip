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
// of the image tower (tower_steps.h, the bf16 GEMM tiers, the LayerNorm kernel) plus the causal flavour of attention_hd.hip and the two gathers below.
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

}  // namespace

struct fp_clip_text {
    fp_ctx* ctx = nullptr;
    fp_clip_text_arch a{};
    int npad = 0;
    const bf16_t *tok = nullptr, *pos = nullptr, *lnfw = nullptr, *lnfb = nullptr;
    int* bad = nullptr;           // raised by the embedding gather on an id outside the vocabulary
    ClipTowerCommon tw;           // text_projection transposed, ones / zeros, the blocks
};

extern "C" int fp_clip_text_create(fp_ctx* ctx, const fp_clip_text_arch* arch, fp_clip_text** out) {
    FP_REQUIRE(ctx && arch && out, "clip_text_create: null argument");
    if (int rc = ClipTowerCommon::check_arch("clip_text_create", arch->width, arch->heads, arch->mlp_dim, arch->embed_dim, arch->depth,
                                             arch->vocab > 0 && arch->ctx > 0, "vocab, ctx")) return rc;
    fp_clip_text* v = new fp_clip_text();
    v->ctx = ctx;
    v->a = *arch;
    v->npad = cdiv(arch->ctx, 16) * 16;
    int rc = v->tw.alloc("clip_text_create", arch->width, arch->heads, arch->embed_dim, arch->depth);
    if (!rc && hipMalloc((void**)&v->bad, sizeof(int)) != hipSuccess) {
        fp_set_error("clip_text_create: hipMalloc failed");
        rc = FP_ERR_HIP;
    }
    if (!rc && hipMemset(v->bad, 0, sizeof(int)) != hipSuccess) {
        fp_set_error("clip_text_create: initialising the device buffers failed");
        rc = FP_ERR_HIP;
    }
    if (rc) {
        fp_clip_text_destroy(v);
        return rc;
    }
    *out = v;
    return FP_OK;
}

extern "C" int fp_clip_text_destroy(fp_clip_text* v) {
    if (!v) return FP_OK;
    if (v->bad) (void)hipFree(v->bad);
    v->tw.free();
    delete v;
    return FP_OK;
}

extern "C" int fp_clip_text_set_weight(fp_clip_text* v, const char* name, const void* d, size_t numel, void* stream) {
    FP_REQUIRE(v && name && d, "clip_text_set_weight: null argument");
    const fp_clip_text_arch& a = v->a;
    const bf16_t* p = (const bf16_t*)d;
    const size_t D = a.width, M = a.mlp_dim, E = a.embed_dim;
    if (!strcmp(name, "text_projection")) return v->tw.set_proj("clip_text_set_weight", name, p, numel, D, E, (hipStream_t)stream);
    const WeightEnt top[] = {{"token_embedding.weight", &v->tok, (size_t)a.vocab * D}, {"positional_embedding", &v->pos, (size_t)a.ctx * D},
                             {"ln_final.weight", &v->lnfw, D}, {"ln_final.bias", &v->lnfb, D}};
    int hit = fp_set_named_weight("clip_text_set_weight", name, name, top, p, numel);
    if (!hit) hit = fp_tower_resblock_weight("clip_text_set_weight", name, v->tw.blk, D, M, p, numel);
    if (hit) return hit > 0 ? FP_OK : FP_ERR_INVALID;
    fp_set_error("clip_text_set_weight: unknown tensor name '%s'", name);
    return FP_ERR_INVALID;
}

extern "C" int fp_clip_text_encode(fp_clip_text* v, const int32_t* d_ids, int B, void* d_out, void* stream) {
    FP_REQUIRE(v && d_ids && d_out, "clip_text_encode: null argument");
    const fp_clip_text_arch& a = v->a;
    hipStream_t s = (hipStream_t)stream;
    FP_REQUIRE(B > 0, "clip_text_encode: B=%d", B);
    FP_REQUIRE(v->tw.have_proj && v->tok && v->pos && v->lnfw && v->lnfb, "clip_text_encode: embedding / ln_final / text_projection weights not set");
    int rc;
    if ((rc = v->tw.all_blocks_complete("clip_text_encode"))) return rc;
    const int D = a.width, n_tok = a.ctx, npad = v->npad;
    const size_t M = (size_t)B * npad;
    if ((rc = fp_tower_offsets_fit("clip_text_encode", M, D, a.mlp_dim, B))) return rc;

    bf16_t *X, *Y, *QKV, *AO, *H1, *POOL, *POOLN;
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
    const TowerRun t{ctx, nullptr, s, B, n_tok, npad, D, a.mlp_dim, a.ln_eps, R, T, AO, H1, v->tw.ones};
    if ((rc = fp_tower_blocks(t, v->tw.blk, QKV, a.heads, v->tw.head_dim, /*causal=*/true))) return rc;
    // ---- the end-of-text row of every prompt, ln_final, then the projection ---------------------------------------------------------------
    hipLaunchKernelGGL(text_pool_kernel, dim3(B), dim3(256), 0, s, d_ids, R, POOL, n_tok, npad, D);
    FP_LAUNCH_CHECK();
    if ((rc = fp_layernorm(POOL, POOLN, v->lnfw, v->lnfb, B, D, a.ln_eps, 0, 0, 0, s))) return rc;
    return v->tw.project(ctx, POOLN, D, a.embed_dim, d_out, B, s);
}

extern "C" double fp_clip_text_flops(const fp_clip_text* v, int B) {
    if (!v) return 0.0;
    const fp_clip_text_arch& a = v->a;
    const double N = a.ctx, D = a.width, Mm = a.mlp_dim;
    const double per_block = 8.0 * N * D * D + 4.0 * N * D * Mm + 2.0 * N * (N + 1) * D;   // the causal half of 4 N^2 D
    return B * (a.depth * per_block + 2.0 * D * a.embed_dim);
}
