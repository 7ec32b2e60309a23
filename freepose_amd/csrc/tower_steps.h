// The steps the transformer drivers (vit.hip, clip.hip, clip_text.hip) and the kernel-level test entries (capi.hip) are built from: GEMM
// launches by the name of the layer form, the LayerNorm-statistics hand-off between a producing and a consuming GEMM, the per-class timing
// of a tower, the parts of a forward the DINOv2 and CLIP towers have in common, and the resblock tower the two CLIP towers are.
// Host code only; every launch goes through fp_ctx::gemm.
#pragma once
#include <stdio.h>
#include <string.h>

#include <cmath>

#include "internal.h"

// ---- GEMM launches by layer form -------------------------------------------------------------------------------------------------
// A linear layer C[M,N] (ldc) = X[M,K] (ldx) W[N,K]^T + bias (or its GELU), turned into one of the other forms by the members
struct GemmStep {
    FpGemmArgs g{};
    int epi;
    GemmStep(const bf16_t* X, int ldx, const bf16_t* W, int K, bf16_t* C, int ldc, const bf16_t* bias, int M, int N, bool gelu = false)
        : epi(gelu ? FP_EPI_BIAS_GELU : FP_EPI_BIAS) {
        g.X = X; g.ldx = ldx; g.W = W; g.ldw = K; g.C = C; g.ldc = ldc; g.bias = bias;
        g.M = M; g.N = N; g.K = K;
    }
    // C = resid + gamma * (the linear layer); with stat_part the epilogue also writes the partial row statistics of C ([N/64][M])
    GemmStep& residual(const bf16_t* gamma, const bf16_t* resid, int ldr, float2* stat_part = nullptr) {
        g.gamma = gamma; g.resid = resid; g.ldr = ldr; g.stat_part = stat_part;
        epi = stat_part ? FP_EPI_LS_RES_STATS : FP_EPI_BIAS_LS_RES;
        return *this;
    }
    // C is Vt[b,h,64,npad]: the rows m = b * npad + t of the linear layer, stored transposed per head
    GemmStep& transposed_v(int npad, int heads) {
        g.ldc = 8; g.npad = npad; g.heads = heads;
        epi = FP_EPI_VT;
        return *this;
    }
    // row m = b * P + p of the linear layer lands in row b * npad + tok_off + p of the token buffer C, plus pos[p]
    GemmStep& patch_embed(const bf16_t* pos, int P, int npad, int tok_off) {
        g.pos = pos; g.P = P; g.npad = npad; g.tok_off = tok_off;
        epi = FP_EPI_PATCH;
        return *this;
    }
    int run(fp_ctx* ctx, hipStream_t s) { return ctx->gemm(g, epi, s); }
};

// ---- LayerNorm folded into the consuming GEMM: who turns row sums into row records ---------------------------------------------------
// The rows of a [M,D] activation reach an LN-folded consumer (gemm_bf16.h FP_EPI_LN_*) as one record + rstd per row.  They come from
// the rows themselves (no producer ran: fp_row_stats) or from the partial sums a FP_EPI_LS_RES_STATS producer left in `part`; the sums
// are finalised by the consumer's prologue when it stays on the small tile tiers, by fp_stats_finalize in front of it otherwise.
struct LnStats {
    uint4* stat; float* rstd; float2* part;
    int M, D; float eps;
    bool pending = false;   // `part` holds sums no kernel has finalised yet: the next consumer attached takes them along
    // makes the row records ready for a consumer of width N.  rows: the activation itself when no producer wrote `part`
    int ready(const bf16_t* rows, int N, hipStream_t s) {
        pending = !rows && fp_gemm_fuses_ln_part(M, N);
        if (rows) return fp_row_stats(rows, stat, rstd, M, D, eps, s);
        return pending ? FP_OK : fp_stats_finalize(part, stat, rstd, M, D, eps, s);
    }
    // turns a linear / GELU / transposed-V step into its LN-folded form on the raw rows; cfrag: the layer's (b', colsum) records
    int attach(GemmStep& t, const uint4* cfrag) {
        FP_REQUIRE(t.epi == FP_EPI_BIAS || t.epi == FP_EPI_BIAS_GELU || t.epi == FP_EPI_VT, "ln attach: epilogue %d has no LN-folded form", t.epi);
        t.g.ln_mfrag = stat; t.g.ln_rstd = rstd; t.g.ln_cfrag = cfrag;
        t.epi = t.epi == FP_EPI_BIAS ? FP_EPI_LN_BIAS : (t.epi == FP_EPI_BIAS_GELU ? FP_EPI_LN_GELU : FP_EPI_LN_VT);
        if (pending) { t.g.ln_part = part; t.g.ln_part_ld = M; t.g.ln_part_nb = D / 64; t.g.ln_eps = eps; t.g.ln_inv_d = 1.0f / (float)D; }
        pending = false;   // that launch writes the records back: later consumers of the same rows read them
        return FP_OK;
    }
};

// ---- per-kernel-class timing of a tower ----------------------------------------------------------------------------------------------
// HIP events on the launch stream.  Events are only RECORDED while a forward runs (no host sync, so the timed region is not
// perturbed); the reader synchronises once and sums the elapsed times.
enum TowerCls { TOWER_GEMM = 0, TOWER_ATTN = 1, TOWER_OTHER = 2 };
struct TowerProf {
    bool on = false;
    struct EvPair { hipEvent_t a, b; int cls; };
    std::vector<EvPair> ev_pool;
    size_t ev_used = 0;
    double gemm_flops = 0;   // algorithmic (unpadded) FLOPs of the GEMM launches issued while profiling
    long gemm_launches = 0;
    void count(double flops, int launches) { if (on) { gemm_flops += flops; gemm_launches += launches; } }
};
struct ProfScope {
    TowerProf* p; hipStream_t s; size_t slot;
    ProfScope(TowerProf* p_, hipStream_t s_, TowerCls cls) : p(p_), s(s_), slot((size_t)-1) {   // p_ null: a tower without timing
        if (!p || !p->on) return;
        if (p->ev_used == p->ev_pool.size()) {
            TowerProf::EvPair e{};
            if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
            p->ev_pool.push_back(e);
        }
        slot = p->ev_used++;
        p->ev_pool[slot].cls = cls;
        (void)hipEventRecord(p->ev_pool[slot].a, s);
    }
    ~ProfScope() {
        if (slot != (size_t)-1) (void)hipEventRecord(p->ev_pool[slot].b, s);
    }
};

// ---- what the towers share -----------------------------------------------------------------------------------------------------------
struct TowerBlockW {   // weights of one block under the DINOv2 names (CLIP: ln_1, in_proj, out_proj, ln_2, c_fc, c_proj; no LayerScale)
    const bf16_t *n1w = nullptr, *n1b = nullptr, *qkvw = nullptr, *qkvb = nullptr, *projw = nullptr,
                 *projb = nullptr, *ls1 = nullptr, *n2w = nullptr, *n2b = nullptr, *fc1w = nullptr, *fc1b = nullptr,
                 *fc2w = nullptr, *fc2b = nullptr, *ls2 = nullptr;
    bool complete() const { return n1w && n1b && qkvw && qkvb && projw && projb && n2w && n2b && fc1w && fc1b && fc2w && fc2b; }
};
struct TowerRun {           // one forward: where it runs, the geometry of its token buffers ([B * npad, D], n_tok of each npad rows real)
    fp_ctx* ctx; TowerProf* prof; hipStream_t s;
    int B, n_tok, npad, D, mlp_dim;
    float eps;
    bf16_t *R, *T, *AO, *H1;   // residual stream, LayerNorm output (unused where the LayerNorm is folded), attention output, fc1 output
    const bf16_t* ones;        // LayerScale gamma of a block without one
    int M() const { return B * npad; }
    void count(double flops_per_row, int launches) const { if (prof) prof->count((double)B * n_tok * flops_per_row, launches); }   // pad rows are no work
};
struct TowerEmbedW {   // what a tower embeds images with; the model owns pe_w, the other pointers are registered weights
    int patch = 0, KP = 0, n_reg = 0;            // KP: 3 * patch^2 padded to the GEMM's K step
    const float *mean = nullptr, *sd = nullptr;  // per-channel normalisation of the model
    bf16_t* pe_w = nullptr;                      // [D, KP] zero-padded copy of the patch-embedding weight
    const bf16_t *pe_b = nullptr, *cls = nullptr, *pos = nullptr, *reg = nullptr;   // pos: [1 + grid^2, D], row 0 the class token's
};
// normalise + unfold into A0, class / register / pad rows, patch-embed GEMM scattering into the token buffer X.  pos_patch: the [P, D]
// position rows of the patches at this image size (e.pos + D, or a resized copy)
inline int fp_tower_embed(const TowerRun& t, const TowerEmbedW& e, const bf16_t* pos_patch, const bf16_t* img, int H, int W, bf16_t* A0, bf16_t* X) {
    const int P = (H / e.patch) * (W / e.patch);
    int rc;
    {
        ProfScope ps(t.prof, t.s, TOWER_OTHER);
        if ((rc = fp_im2col_norm_ms(img, A0, t.B, H, W, e.patch, e.KP, e.mean, e.sd, t.s))) return rc;
        if ((rc = fp_token_init(X, e.cls, e.pos, e.reg, e.n_reg, t.B, t.n_tok, t.npad, t.D, t.s))) return rc;
    }
    ProfScope ps(t.prof, t.s, TOWER_GEMM);
    GemmStep pe(A0, e.KP, e.pe_w, e.KP, X, t.D, e.pe_b, t.B * P, t.D);
    if ((rc = pe.patch_embed(pos_patch, P, t.npad, 1 + e.n_reg).run(t.ctx, t.s))) return rc;
    if (t.prof) t.prof->count(2.0 * t.B * P * (3.0 * e.patch * e.patch) * t.D, 1);
    return FP_OK;
}
// R += ls1 * (AO projw^T + projb): the out-projection half of a block; stat_part as in GemmStep::residual
inline int fp_tower_out_proj(const TowerRun& t, const TowerBlockW& w, float2* stat_part) {
    ProfScope ps(t.prof, t.s, TOWER_GEMM);
    GemmStep proj(t.AO, t.D, w.projw, t.D, t.R, t.D, w.projb, t.M(), t.D);
    if (int rc = proj.residual(w.ls1 ? w.ls1 : t.ones, t.R, t.D, stat_part).run(t.ctx, t.s)) return rc;
    t.count(2.0 * t.D * t.D, 1);
    return FP_OK;
}
// R += ls2 * (fc2 gelu(fc1 LN2(R))): the MLP half of a block.  Plain (st null): LN2(R) is written to T by the LayerNorm kernel and fc1
// reads T.  Folded: fc1 reads R with the folded weights fc1w / fc1_cb and takes its row statistics from st
inline int fp_tower_mlp(const TowerRun& t, const TowerBlockW& w, LnStats* st, const bf16_t* fc1w, const uint4* fc1_cb, float2* stat_part) {
    const int D = t.D, M = t.M(), N = t.mlp_dim;
    int rc;
    {
        ProfScope ps(t.prof, t.s, TOWER_OTHER);
        if ((rc = st ? st->ready(nullptr, N, t.s) : fp_layernorm(t.R, t.T, w.n2w, w.n2b, M, D, t.eps, 0, 0, 0, t.s))) return rc;
    }
    ProfScope ps(t.prof, t.s, TOWER_GEMM);
    GemmStep fc1(st ? t.R : t.T, D, st ? fc1w : w.fc1w, D, t.H1, N, w.fc1b, M, N, /*gelu=*/true);
    if (st && (rc = st->attach(fc1, fc1_cb))) return rc;
    if ((rc = fc1.run(t.ctx, t.s))) return rc;
    if ((rc = GemmStep(t.H1, N, w.fc2w, N, t.R, D, w.fc2b, M, D).residual(w.ls2 ? w.ls2 : t.ones, t.R, D, stat_part).run(t.ctx, t.s))) return rc;
    t.count(4.0 * D * N, 2);
    return FP_OK;
}

// ---- registering weights -------------------------------------------------------------------------------------------------------------
// numel check of <who>_set_weight (who: "vit_set_weight" / "clip_set_weight")
inline bool fp_weight_numel(const char* who, const char* name, size_t numel, size_t want) {
    if (numel != want) fp_set_error("%s: %s has %zu elements, expected %zu", who, name, numel, want);
    return numel == want;
}
// a table of names (of a block, or of the tower itself): 1 = `rest` names an entry of tab and its slot now points at p,
// -1 = it does but numel is wrong, 0 = no entry
struct WeightEnt { const char* n; const bf16_t** slot; size_t numel; };
template <size_t N>
inline int fp_set_named_weight(const char* who, const char* name, const char* rest, const WeightEnt (&tab)[N], const bf16_t* p, size_t numel) {
    for (const WeightEnt& e : tab)
        if (!strcmp(rest, e.n)) {
            if (!fp_weight_numel(who, name, numel, e.numel)) return -1;
            *e.slot = p;
            return 1;
        }
    return 0;
}
// copies a [D, 3 * patch^2] patch-embedding weight into the rows of the zero-padded [D, KP] buffer e.pe_w the patch GEMM reads
inline int fp_tower_set_patch_weight(const char* who, const char* name, const bf16_t* p, size_t numel, const TowerEmbedW& e, size_t D, hipStream_t s) {
    const size_t K = (size_t)3 * e.patch * e.patch;
    if (!fp_weight_numel(who, name, numel, D * K)) return FP_ERR_INVALID;
    FP_HIP(hipMemcpy2DAsync(e.pe_w, (size_t)e.KP * 2, p, K * 2, K * 2, D, hipMemcpyDeviceToDevice, s));
    return FP_OK;
}

// ---- the CLIP towers (clip.hip, clip_text.hip): open_clip's resblocks, which the image and the text transformer share ---------------
// "transformer.resblocks.<i>.<rest>" of a tower of width D and MLP width M: fp_set_named_weight's answer (0 also for any other name)
inline int fp_tower_resblock_weight(const char* who, const char* name, std::vector<TowerBlockW>& blk, size_t D, size_t M, const bf16_t* p, size_t numel) {
    int bi = -1;
    char rest[64] = {0};
    if (sscanf(name, "transformer.resblocks.%d.%63s", &bi, rest) != 2 || bi < 0 || bi >= (int)blk.size()) return 0;
    TowerBlockW& w = blk[bi];
    const WeightEnt tab[] = {
        {"ln_1.weight", &w.n1w, D}, {"ln_1.bias", &w.n1b, D},
        {"attn.in_proj_weight", &w.qkvw, 3 * D * D}, {"attn.in_proj_bias", &w.qkvb, 3 * D},
        {"attn.out_proj.weight", &w.projw, D * D}, {"attn.out_proj.bias", &w.projb, D},
        {"ln_2.weight", &w.n2w, D}, {"ln_2.bias", &w.n2b, D},
        {"mlp.c_fc.weight", &w.fc1w, M * D}, {"mlp.c_fc.bias", &w.fc1b, M},
        {"mlp.c_proj.weight", &w.fc2w, D * M}, {"mlp.c_proj.bias", &w.fc2b, D}};
    return fp_set_named_weight(who, name, rest, tab, p, numel);
}
// depth x { R += out_proj(attn(ln_1 R)) ; R += c_proj(gelu(c_fc(ln_2 R))) } on the plain [q | k | v] rows QKV [M, 3 D]
inline int fp_tower_blocks(const TowerRun& t, const std::vector<TowerBlockW>& blk, bf16_t* QKV, int heads, int head_dim, bool causal) {
    const int D = t.D, M = t.M();
    const float scale = 1.0f / sqrtf((float)head_dim);
    int rc;
    for (const TowerBlockW& w : blk) {
        if ((rc = fp_layernorm(t.R, t.T, w.n1w, w.n1b, M, D, t.eps, 0, 0, 0, t.s))) return rc;
        if ((rc = GemmStep(t.T, D, w.qkvw, D, QKV, 3 * D, w.qkvb, M, 3 * D).run(t.ctx, t.s))) return rc;
        if ((rc = (causal ? fp_attention_causal_fwd : fp_attention_hd_fwd)(QKV, 3 * D, t.AO, D, t.B, heads, head_dim, t.n_tok, t.npad, scale, t.s))) return rc;
        if ((rc = fp_tower_out_proj(t, w, nullptr))) return rc;
        if ((rc = fp_tower_mlp(t, w, nullptr, nullptr, nullptr, nullptr))) return rc;
    }
    return FP_OK;
}
// what both towers own besides their embeddings.  who: the entry's name, the first word of its refusals
struct ClipTowerCommon {
    int head_dim = 0;
    bf16_t* projT = nullptr;      // [embed_dim, width] private transposed copy of the projection
    bf16_t* ones = nullptr;       // gamma of the residual epilogue (no LayerScale in CLIP)
    bf16_t* zeros = nullptr;      // bias of the GEMMs whose layer has none (the projection; the image tower's patch embedding)
    bool have_proj = false;
    std::vector<TowerBlockW> blk;
    // rest_ok / rest_names: the fields only one of the towers has
    static int check_arch(const char* who, int width, int heads, int mlp_dim, int embed_dim, int depth, bool rest_ok, const char* rest_names) {
        FP_REQUIRE(width > 0 && width % 64 == 0 && heads > 0 && width % heads == 0, "%s: width=%d heads=%d (width must be a multiple of 64 and of heads)",
                   who, width, heads);
        const int hd = width / heads;
        FP_REQUIRE(hd % 8 == 0 && hd >= 8 && hd <= 128, "%s: head dimension %d (must be a multiple of 8 in [8, 128])", who, hd);
        FP_REQUIRE(width <= 2048, "%s: width=%d exceeds the LayerNorm kernel (2048)", who, width);
        FP_REQUIRE(mlp_dim > 0 && mlp_dim % 64 == 0 && embed_dim > 0 && embed_dim % 16 == 0 && depth > 0 && rest_ok,
                   "%s: bad arch (mlp_dim %% 64, embed_dim %% 16, depth, %s)", who, rest_names);
        return FP_OK;
    }
    int alloc(const char* who, int width, int heads, int embed_dim, int depth) {
        head_dim = width / heads;
        blk.resize(depth);
        const size_t W = width, E = embed_dim, nvec = std::max(W, E);
        if (hipMalloc((void**)&projT, E * W * 2) != hipSuccess || hipMalloc((void**)&ones, nvec * 2) != hipSuccess ||
            hipMalloc((void**)&zeros, nvec * 2) != hipSuccess) {
            fp_set_error("%s: hipMalloc failed", who);
            return FP_ERR_HIP;
        }
        std::vector<bf16_t> one(nvec, f2bf(1.0f));
        if (hipMemset(zeros, 0, nvec * 2) != hipSuccess || hipMemcpy(ones, one.data(), nvec * 2, hipMemcpyHostToDevice) != hipSuccess) {
            fp_set_error("%s: initialising the device buffers failed", who);
            return FP_ERR_HIP;
        }
        return FP_OK;
    }
    void free() {
        if (projT) (void)hipFree(projT);
        if (ones) (void)hipFree(ones);
        if (zeros) (void)hipFree(zeros);
    }
    // p: the [D, E] projection as open_clip stores it (applied as x @ p; the GEMM wants [out, in])
    int set_proj(const char* who, const char* name, const bf16_t* p, size_t numel, size_t D, size_t E, hipStream_t s) {
        if (!fp_weight_numel(who, name, numel, D * E)) return FP_ERR_INVALID;
        if (int rc = fp_transpose_bf16(p, projT, (int)D, (int)E, s)) return rc;
        have_proj = true;
        return FP_OK;
    }
    int all_blocks_complete(const char* who) const {
        for (size_t i = 0; i < blk.size(); ++i) FP_REQUIRE(blk[i].complete(), "%s: weights of block %d not set", who, (int)i);
        return FP_OK;
    }
    // out [B, E] = pooled [B, D] @ projection
    int project(fp_ctx* ctx, const bf16_t* pooled, int D, int E, void* out, int B, hipStream_t s) const {
        return GemmStep(pooled, D, projT, D, (bf16_t*)out, E, zeros, B, E).run(ctx, s);
    }
};
// the GEMM tiers address a launch's tiles with 32-bit byte offsets: M rows of the widest activation (fc1's or qkv's output) must fit
inline int fp_tower_offsets_fit(const char* who, size_t M, int D, int mlp_dim, int B) {
    FP_REQUIRE(M * (size_t)std::max(mlp_dim, 3 * D) * 2 < 0xffffffffull, "%s: batch too large for 32-bit tile offsets (B=%d)", who, B);
    return FP_OK;
}
