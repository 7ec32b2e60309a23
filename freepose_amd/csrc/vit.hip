// DINOv2 ViT driver (hub *_reg models): weights, the LayerNorm fold, fp_vit_forward and its per-class timing.
#include <stdio.h>

#include "../../include/freepose_hip.h"
#include "tower_steps.h"

struct fp_vit {
    fp_ctx* ctx = nullptr;
    fp_vit_arch a{};
    TowerEmbedW emb;
    const bf16_t *normw = nullptr, *normb = nullptr;
    bf16_t* ones = nullptr;  // LayerScale gamma = 1 for checkpoints without ls*
    std::vector<TowerBlockW> blk;
    // LayerNorm folded into the consuming GEMMs (gemm_bf16.h FP_EPI_LN_*): per block W' = W diag(gamma_ln) for qkv / fc1 and the
    // (colsum(W'), b') pairs, built on the device the first time a forward runs after the weights changed
    struct VitFold { bf16_t *qkvw = nullptr, *fc1w = nullptr; uint4 *qkv_cb = nullptr, *fc1_cb = nullptr; };
    std::vector<VitFold> fold;
    int folded_upto = 0;             // blocks [0, folded_upto) carry valid folded weights (a forward folds only the blocks it runs)
    hipEvent_t fold_ev = nullptr;    // recorded behind the last fold; forwards on OTHER streams wait for it
    hipStream_t fold_stream = nullptr;
    bool refold = false;             // a weight was replaced after a fold: forwards in flight on other streams may still read the fold buffers
    // pos-embed cache per (gh,gw)
    std::map<std::pair<int, int>, bf16_t*> pos_cache;
    TowerProf prof;
};

extern "C" int fp_vit_create(fp_ctx* ctx, const fp_vit_arch* arch, fp_vit** out) {
    FP_REQUIRE(ctx && arch && out, "vit_create: null argument");
    FP_REQUIRE(arch->dim % 64 == 0 && arch->heads * 64 == arch->dim, "vit_create: dim=%d heads=%d (head dim must be 64)",
               arch->dim, arch->heads);
    FP_REQUIRE(arch->mlp_dim % 64 == 0 && arch->depth > 0 && arch->patch > 0, "vit_create: bad arch");
    fp_vit* v = new fp_vit();
    v->ctx = ctx;
    v->a = *arch;
    v->blk.resize(arch->depth);
    v->fold.resize(arch->depth);
    v->emb.patch = arch->patch; v->emb.n_reg = arch->n_reg; v->emb.mean = FP_IMAGENET_MEAN; v->emb.sd = FP_IMAGENET_SD;
    v->emb.KP = cdiv(3 * arch->patch * arch->patch, 64) * 64;
    if (hipMalloc((void**)&v->emb.pe_w, (size_t)arch->dim * v->emb.KP * 2) != hipSuccess ||
        hipMalloc((void**)&v->ones, (size_t)arch->dim * 2) != hipSuccess) {
        fp_set_error("vit_create: hipMalloc failed");
        delete v;
        return FP_ERR_HIP;
    }
    FP_HIP(hipMemset(v->emb.pe_w, 0, (size_t)arch->dim * v->emb.KP * 2));
    std::vector<bf16_t> one(arch->dim, f2bf(1.0f));
    FP_HIP(hipMemcpy(v->ones, one.data(), (size_t)arch->dim * 2, hipMemcpyHostToDevice));
    *out = v;
    return FP_OK;
}
extern "C" int fp_vit_destroy(fp_vit* v) {
    if (!v) return FP_OK;
    if (v->emb.pe_w) (void)hipFree(v->emb.pe_w);
    if (v->ones) (void)hipFree(v->ones);
    for (auto& kv : v->pos_cache) (void)hipFree(kv.second);
    for (auto& f : v->fold) {
        if (f.qkvw) (void)hipFree(f.qkvw);
        if (f.fc1w) (void)hipFree(f.fc1w);
        if (f.qkv_cb) (void)hipFree(f.qkv_cb);
        if (f.fc1_cb) (void)hipFree(f.fc1_cb);
    }
    for (auto& p : v->prof.ev_pool) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    if (v->fold_ev) (void)hipEventDestroy(v->fold_ev);
    delete v;
    return FP_OK;
}

extern "C" int fp_vit_set_weight(fp_vit* v, const char* name, const void* d, size_t numel, void* stream) {
    FP_REQUIRE(v && name && d, "vit_set_weight: null argument");
    const fp_vit_arch& a = v->a;
    const bf16_t* p = (const bf16_t*)d;
    const size_t D = a.dim;
    if (v->folded_upto > 0) v->refold = true;
    v->folded_upto = 0;   // any new tensor invalidates the folded LayerNorm weights (in-place updates of a registered tensor: re-register it)
    std::string s(name);
    if (s == "pos_embed") {
        if (!fp_weight_numel("vit_set_weight", name, numel, (size_t)(1 + a.pos_grid * a.pos_grid) * D)) return FP_ERR_INVALID;
        v->emb.pos = p;
        for (auto& kv : v->pos_cache) (void)hipFree(kv.second);
        v->pos_cache.clear();
        return FP_OK;
    }
    if (s == "mask_token") return FP_OK;  // unused at inference
    if (s == "patch_embed.proj.weight") return fp_tower_set_patch_weight("vit_set_weight", name, p, numel, v->emb, D, (hipStream_t)stream);
    const WeightEnt top[] = {{"cls_token", &v->emb.cls, D}, {"register_tokens", &v->emb.reg, (size_t)a.n_reg * D}, {"patch_embed.proj.bias", &v->emb.pe_b, D},
                             {"norm.weight", &v->normw, D}, {"norm.bias", &v->normb, D}};
    if (const int hit = fp_set_named_weight("vit_set_weight", name, name, top, p, numel)) return hit > 0 ? FP_OK : FP_ERR_INVALID;
    int bi = -1;
    char rest[64] = {0};
    if (sscanf(name, "blocks.%d.%63s", &bi, rest) == 2 && bi >= 0 && bi < a.depth) {
        TowerBlockW& w = v->blk[bi];
        const size_t M = a.mlp_dim;
        const WeightEnt tab[] = {
            {"norm1.weight", &w.n1w, D}, {"norm1.bias", &w.n1b, D},
            {"attn.qkv.weight", &w.qkvw, 3 * D * D}, {"attn.qkv.bias", &w.qkvb, 3 * D},
            {"attn.proj.weight", &w.projw, D * D}, {"attn.proj.bias", &w.projb, D},
            {"ls1.gamma", &w.ls1, D}, {"norm2.weight", &w.n2w, D}, {"norm2.bias", &w.n2b, D},
            {"mlp.fc1.weight", &w.fc1w, M * D}, {"mlp.fc1.bias", &w.fc1b, M},
            {"mlp.fc2.weight", &w.fc2w, D * M}, {"mlp.fc2.bias", &w.fc2b, D}, {"ls2.gamma", &w.ls2, D}};
        if (const int hit = fp_set_named_weight("vit_set_weight", name, rest, tab, p, numel)) return hit > 0 ? FP_OK : FP_ERR_INVALID;
    }
    fp_set_error("vit_set_weight: unknown tensor name '%s'", name);
    return FP_ERR_INVALID;
}

static int vit_pos(fp_vit* v, int gh, int gw, hipStream_t s, const bf16_t** out) {
    const fp_vit_arch& a = v->a;
    if (gh == a.pos_grid && gw == a.pos_grid) { *out = v->emb.pos + a.dim; return FP_OK; }  // no resize needed
    auto key = std::make_pair(gh, gw);
    auto it = v->pos_cache.find(key);
    if (it == v->pos_cache.end()) {
        bf16_t* buf = nullptr;
        FP_HIP(hipMalloc((void**)&buf, (size_t)gh * gw * a.dim * 2));
        int rc = fp_posembed_aa(v->emb.pos + a.dim, buf, a.pos_grid, gh, gw, a.dim, s);
        if (rc) { (void)hipFree(buf); return rc; }
        it = v->pos_cache.emplace(key, buf).first;
    }
    *out = it->second;
    return FP_OK;
}

// W' = W diag(gamma_ln), (colsum, b') for the qkv and fc1 layers of the first L blocks (device kernels on `s`, once per weight load)
static int vit_fold(fp_vit* v, int first, int L, hipStream_t s) {
    const fp_vit_arch& a = v->a;
    const size_t D = a.dim, Mm = a.mlp_dim;
    for (int i = first; i < L; ++i) {
        const TowerBlockW& w = v->blk[i];
        fp_vit::VitFold& f = v->fold[i];
        if (!f.qkvw) FP_HIP(hipMalloc((void**)&f.qkvw, 3 * D * D * 2));
        if (!f.qkv_cb) FP_HIP(hipMalloc((void**)&f.qkv_cb, 3 * D * sizeof(uint4)));
        if (!f.fc1w) FP_HIP(hipMalloc((void**)&f.fc1w, Mm * D * 2));
        if (!f.fc1_cb) FP_HIP(hipMalloc((void**)&f.fc1_cb, Mm * sizeof(uint4)));
        int rc;
        // q rows carry log2(e) / sqrt(head_dim): fp_attention_fwd(..., q_prescaled = true) below
        if ((rc = fp_ln_fold(w.qkvw, w.n1w, w.n1b, w.qkvb, f.qkvw, f.qkv_cb, (int)(3 * D), (int)D, (int)D, FP_ATTN_QSCALE, s))) return rc;
        if ((rc = fp_ln_fold(w.fc1w, w.n2w, w.n2b, w.fc1b, f.fc1w, f.fc1_cb, (int)Mm, (int)D, 0, 1.0f, s))) return rc;
    }
    return FP_OK;
}

extern "C" double fp_vit_flops(const fp_vit* v, int B, int H, int W, int layer) {
    const fp_vit_arch& a = v->a;
    const double P = (double)(H / a.patch) * (W / a.patch), N = P + 1 + a.n_reg, D = a.dim;
    const int L = std::min(layer, a.depth);
    const double mlp_ratio = (double)a.mlp_dim / a.dim;
    const double per_block = (8.0 + 4.0 * mlp_ratio) * N * D * D + 4.0 * N * N * D;  // 24 N D^2 + 4 N^2 D for ratio 4
    return B * (L * per_block + 2.0 * P * (3.0 * a.patch * a.patch) * D);
}

extern "C" int fp_vit_forward(fp_vit* v, const void* d_images, int B, int H, int W, int layer, int feature_type,
                              void* d_out, void* stream) {
    FP_REQUIRE(v && d_images && d_out, "vit_forward: null argument");
    const fp_vit_arch& a = v->a;
    hipStream_t s = (hipStream_t)stream;
    fp_ctx* ctx = v->ctx;
    FP_REQUIRE(B > 0 && H % a.patch == 0 && W % a.patch == 0, "vit_forward: B=%d H=%d W=%d (patch %d)", B, H, W, a.patch);
    FP_REQUIRE(feature_type >= 0 && feature_type <= 3, "vit_forward: feature_type %d", feature_type);
    FP_REQUIRE(v->emb.cls && v->emb.pos && v->emb.pe_b && v->normw && v->normb && (a.n_reg == 0 || v->emb.reg),
               "vit_forward: embedding / final-norm weights not set");
    // dino.py:18-21 breaks when blk_idx + 1 == layer: a layer outside [1, depth] (too large, zero or negative) never matches,
    // so all blocks run
    const int L = (layer >= 1 && layer <= a.depth) ? layer : a.depth;
    for (int i = 0; i < L; ++i) {
        FP_REQUIRE(v->blk[i].complete(), "vit_forward: weights of block %d not set", i);
    }
    const int D = a.dim, gh = H / a.patch, gw = W / a.patch, P = gh * gw;
    const int n_tok = P + 1 + a.n_reg;
    const int npad = cdiv(n_tok, 16) * 16;
    const size_t M = (size_t)B * npad;
    FP_REQUIRE(M * (size_t)a.mlp_dim * 2 < 0xffffffffull, "vit_forward: batch too large for 32-bit tile offsets (B=%d)", B);
    const int Mi = (int)M;

    bf16_t *A0, *X, *Y, *QK, *Vt, *AO, *H1;
    int rc;
    // LayerNorm 1 / 2 folded into the qkv / fc1 GEMMs (default; fp_ctx_set_option(ctx, "ln_fused", 0) runs the separate kernel)
    const bool lnf = ctx->opt_ln_fused != 0 && D % 64 == 0;
    LnStats st{nullptr, nullptr, nullptr, Mi, D, a.ln_eps};   // row records, rstd and the producers' partial sums of the residual stream
    if (lnf) {
        // only the blocks this call runs (their weights were checked above): a caller that registered 22 of 24 blocks never
        // touches the other two.  The fold is enqueued on `s`; a later forward on another stream waits for it through the event.
        // Ordering across streams: whatever this call does with the fold buffers — read blocks folded earlier, fold further blocks — comes
        // behind the last fold (the event is re-recorded on `s` only after `s` has waited for it, so waiting for the newest record
        // covers every earlier fold).  A RE-fold (a weight was replaced) overwrites buffers that forwards on other streams may still be
        // reading: the device is drained first — once per weight load, never on the steady path.
        if (v->fold_ev && s != v->fold_stream) FP_HIP(hipStreamWaitEvent(s, v->fold_ev, 0));
        if (v->folded_upto < L) {
            if (v->refold) {
                FP_HIP(hipDeviceSynchronize());
                v->refold = false;
            }
            if ((rc = vit_fold(v, v->folded_upto, L, s))) return rc;
            if (!v->fold_ev) FP_HIP(hipEventCreateWithFlags(&v->fold_ev, hipEventDisableTiming));
            FP_HIP(hipEventRecord(v->fold_ev, s));
            v->fold_stream = s;
            v->folded_upto = L;
        }
        FP_WS(ctx, "vit.ln_stat", M * sizeof(uint4), st.stat);
        FP_WS(ctx, "vit.ln_rstd", M * sizeof(float), st.rstd);
        FP_WS(ctx, "vit.ln_part", M * (size_t)(D / 64) * sizeof(float2), st.part);
    }
    FP_WS(ctx, "vit.im2col", (size_t)B * P * v->emb.KP * 2, A0);
    FP_WS(ctx, "vit.x", M * D * 2, X);
    FP_WS(ctx, "vit.y", M * D * 2, Y);
    FP_WS(ctx, "vit.qk", M * 2 * D * 2, QK);
    FP_WS(ctx, "vit.vt", M * D * 2 + 256, Vt);
    FP_WS(ctx, "vit.ao", M * D * 2, AO);
    FP_WS(ctx, "vit.h1", M * (size_t)a.mlp_dim * 2, H1);

    const bf16_t* pos_patch;
    if ((rc = vit_pos(v, gh, gw, s, &pos_patch))) return rc;

    // X is the residual stream; unfused, Y takes every LayerNorm's output
    const TowerRun t{ctx, &v->prof, s, B, n_tok, npad, D, a.mlp_dim, a.ln_eps, X, Y, AO, H1, v->ones};
    // ---- K0-K2: normalise + unfold, patch-embed GEMM scattering into the token buffer ----------
    if ((rc = fp_tower_embed(t, v->emb, pos_patch, (const bf16_t*)d_images, H, W, A0, X))) return rc;
    const bf16_t* in = lnf ? X : Y;   // what the qkv GEMMs read
    for (int i = 0; i < L; ++i) {
        const TowerBlockW& w = v->blk[i];
        const fp_vit::VitFold& f = v->fold[i];
        {
            ProfScope ps(&v->prof, s, TOWER_OTHER);
            // folded: block 0 takes the statistics of the rows patch-embed + token init wrote; later blocks the previous fc2's sums
            if ((rc = lnf ? st.ready(i == 0 ? X : nullptr, 2 * D, s) : fp_layernorm(X, Y, w.n1w, w.n1b, Mi, D, a.ln_eps, 0, 0, 0, s))) return rc;
        }
        {
            ProfScope ps(&v->prof, s, TOWER_GEMM);
            const bf16_t* qkvw = lnf ? f.qkvw : w.qkvw;
            GemmStep qk(in, D, qkvw, D, QK, 2 * D, w.qkvb, Mi, 2 * D), vt(in, D, qkvw + (size_t)2 * D * D, D, Vt, 8, w.qkvb + 2 * D, Mi, D);
            vt.transposed_v(npad, a.heads);
            // qk first: it takes the sums along and finalises them, V^T reads the records it wrote
            if (lnf && ((rc = st.attach(qk, f.qkv_cb)) || (rc = st.attach(vt, f.qkv_cb + 2 * D)))) return rc;
            if ((rc = qk.run(ctx, s))) return rc;
            if ((rc = vt.run(ctx, s))) return rc;
            t.count(2.0 * 3.0 * D * D, 2);
        }
        {
            ProfScope ps(&v->prof, s, TOWER_ATTN);
            // folded q rows carry log2(e) / sqrt(head_dim) (vit_fold)
            if ((rc = fp_attention_fwd(QK, 2 * D, Vt, AO, D, B, a.heads, n_tok, npad, /*q_prescaled=*/lnf, s))) return rc;
        }
        // proj feeds LN2 of this block; fc2 feeds LN1 of the next one (not after the last)
        if ((rc = fp_tower_out_proj(t, w, st.part))) return rc;
        if ((rc = fp_tower_mlp(t, w, lnf ? &st : nullptr, f.fc1w, f.fc1_cb, i + 1 < L ? st.part : nullptr))) return rc;
    }
    // ---- K8: final norm + token slice (dino.py:23-30) ------------------------------------------------
    {
        ProfScope ps(&v->prof, s, TOWER_OTHER);
        // class token: row 0 of a crop; registers: rows 1 .. n_reg; patches: the P rows behind them
        const int rows_per_b = feature_type == 0 ? 1 : (feature_type == 1 ? a.n_reg : P);
        const int off = feature_type == 0 ? 0 : (feature_type == 1 ? 1 : 1 + a.n_reg);
        if (rows_per_b > 0)
            if ((rc = fp_layernorm(X, (bf16_t*)d_out, v->normw, v->normb, B * rows_per_b, D, a.ln_eps, rows_per_b, npad,
                                   off, s, feature_type == 3)))
                return rc;
    }
    return FP_OK;
}

extern "C" int fp_vit_profile(fp_vit* v, int enable) {
    FP_REQUIRE(v, "vit_profile: null");
    TowerProf& p = v->prof;
    p.on = enable != 0;
    p.ev_used = 0;
    p.gemm_flops = 0;
    p.gemm_launches = 0;
    return FP_OK;
}
extern "C" int fp_vit_profile_read(fp_vit* v, float* g, float* at, float* o, double* fl) {
    FP_REQUIRE(v, "vit_profile_read: null");
    TowerProf& p = v->prof;
    float acc[3] = {0.f, 0.f, 0.f};
    for (size_t i = 0; i < p.ev_used; ++i) {
        FP_HIP(hipEventSynchronize(p.ev_pool[i].b));
        float ms = 0.f;
        FP_HIP(hipEventElapsedTime(&ms, p.ev_pool[i].a, p.ev_pool[i].b));
        acc[p.ev_pool[i].cls] += ms;
    }
    if (g) *g = acc[TOWER_GEMM];
    if (at) *at = acc[TOWER_ATTN];
    if (o) *o = acc[TOWER_OTHER];
    if (fl) *fl = p.gemm_flops;
    return FP_OK;
}
extern "C" long fp_vit_profile_gemm_launches(const fp_vit* v) { return v ? v->prof.gemm_launches : 0; }
