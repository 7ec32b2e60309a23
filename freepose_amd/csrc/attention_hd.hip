// Multi-head attention forward for a GENERAL head dimension (8 .. 128, multiple of 8), gfx950 only.
//
//   O[b, t, h*hd + d] = sum_j softmax_j( q[b,t,h] . k[b,j,h] * scale ) v[b,j,h,d]        over the n_tok real tokens j
//
// The input is the plain output of ONE bias GEMM with N = 3 * width: rows are B * npad tokens, columns [q | k | v], each heads x hd
// (nn.MultiheadAttention's in_proj order) — the layout of the CLIP towers (ViT-bigG/14: 16 heads of 104).  attention.hip stays the
// kernel of the DINOv2 path (head dimension 64, V stored transposed by its GEMM epilogue, DMA ring): this one trades its speed for
// generality and is sized for 257-token sequences and a handful of crops.
//
// Both products run on the matrix pipe, in the orientation of attention.hip:
//   S^T[key,q] = mfma(A = K rows,   B = Q rows)   a lane owns 16 keys of ONE query column (softmax statistics: 4 lanes per query)
//   O^T[d,q]   = mfma(A = V^T rows, B = P^T)      the P^T fragments are built in registers from the S^T accumulators: K rows enter
//                                                 the first product permuted (attn_hd_core.h fp_ahd_tile_key) so that a lane's
//                                                 accumulators are 8 CONSECUTIVE keys per 32-key step, the B-operand k order
// The head dimension is padded to the MFMA K granularity (32) with ZEROS IN LDS / registers; memory is never read past a head's
// columns, and key / query rows at or beyond n_tok are never read at all (they are zero-filled), so whatever bytes the pad rows of
// QKV hold — NaNs included — cannot reach a real row.  Pad query rows produce finite values (the mean of V over the real keys).
// One workgroup = 4 waves x 16 queries of one (crop, head).  Key tiles of 64 are staged through registers (the global loads of tile
// t+1 are in flight under the products of tile t) into one LDS image: K row-major, V transposed by the staging writes.  Online softmax
// over the key tiles with the running maximum raised every tile: any sequence length.
//
// CAUSAL = true is the attention of open_clip's text transformer, whose mask hides every key after the query:
//
//   O[b, t, h*hd + d] = sum_{j <= t} softmax_j( q[b,t,h] . k[b,j,h] * scale ) v[b,j,h,d]        over the real tokens j <= t
//
// Layout, contract, staging and both products are the ones above.  What differs:
//   * the workgroup of queries [q0, q0 + 64) walks the key tiles 0 .. floor(min(q0 + 63, n_tok - 1) / 64) only (attn_hd_core.h
//     fp_ahd_causal_num_tiles): tiles wholly above the diagonal are skipped, not masked — at 77 tokens the first query block does one
//     tile instead of two;
//   * inside a visited tile a logit with key > query is replaced like a pad key (fp_ahd_causal_visible), before the maximum, so its P is
//     exactly 0.  The rows of such FUTURE keys are real data and are loaded; V rows enter the second product multiplied by P = 0, which
//     is exact for finite values, and whatever the first product made of a future K row (infinities and NaNs included) is discarded by
//     the select.
// Pad query rows see every real key and produce finite values under either mask.
#include "internal.h"
#include "attn_hd_core.h"

namespace {

constexpr int KT = FP_AHD_KEY_TILE;   // keys per tile
constexpr int QBLK = FP_AHD_QUERY_BLOCK;   // queries per workgroup (4 waves x 16)
constexpr int VPITCH = FP_AHD_V_PITCH;   // bytes per V^T row in LDS (64 keys + one 16-byte slot: rows start on different banks)

struct AttnHdArgs {
    const bf16_t* QKV; int ldqkv;   // elements
    bf16_t* O; int ldo;
    int heads, hd, n_tok, npad;
    float scale_log2e;              // scale * log2(e)
};

template <int NKK, bool CAUSAL>   // padded head dimension = 32 * NKK; CAUSAL: query t attends to keys 0 .. t
__global__ __launch_bounds__(256) void attn_hd_kernel(AttnHdArgs p) {
    constexpr int HDP = 32 * NKK;
    constexpr int NCH = fp_ahd_chunks(NKK);  // 16-byte chunks per padded row
    constexpr int NDF = HDP / 16;           // 16-row fragments of O^T
    constexpr int KPITCH = fp_ahd_k_pitch(NKK);   // bytes per K row in LDS
    constexpr int KI = NKK;                 // K chunks per thread and tile: 64 * NCH / 256
    constexpr int VN = fp_ahd_vstage_items(NCH);   // V work items per tile: (key pair, chunk)
    constexpr int VI = (VN + 255) / 256;
    __shared__ __attribute__((aligned(16))) char sK[KT * KPITCH];
    __shared__ __attribute__((aligned(16))) char sV[HDP * VPITCH];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z;
    const int qblk = blockIdx.x * QBLK;
    const int q0 = qblk + wave * 16;
    const int qc = CAUSAL ? q0 + li : 0;   // this lane's query for the causal mask (the other flavour needs it only to load and to store)
    const bool idle = q0 >= p.npad;        // no row to store: the wave only takes part in staging and barriers
    const size_t rowbase = (size_t)b * p.npad;
    const bf16_t* gq = p.QKV + (size_t)h * p.hd;
    const bf16_t* gk = gq + (size_t)p.heads * p.hd;
    const bf16_t* gv = gk + (size_t)p.heads * p.hd;

    // ---- Q fragments (B operand): lane (li -> query, lg -> 8-wide d slot); rows >= n_tok and columns >= hd are zeros ------------
    bf16x8_t qf[NKK];
    {
        const int q = q0 + li;
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
            const int d0 = 32 * kk + 8 * lg;
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (fp_ahd_row_real(q, p.n_tok) && fp_ahd_chunk_real(d0, p.hd)) w = *(const uint4*)(gq + (rowbase + q) * p.ldqkv + d0);
            qf[kk] = __builtin_bit_cast(bf16x8_t, w);
        }
    }

    // ---- staging: global -> registers -> LDS (pad rows are zero-filled; future rows of a visited tile are real and are loaded) ---
    uint4 rk[KI], rv0[VI], rv1[VI];
    auto load_tile = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < KI; ++i) {
            const int c = tid + 256 * i, key = fp_ahd_kstage_key(c, NCH), d0 = fp_ahd_kstage_d0(c, NCH);
            rk[i] = make_uint4(0u, 0u, 0u, 0u);
            if (fp_ahd_row_real(kv0 + key, p.n_tok) && fp_ahd_chunk_real(d0, p.hd)) rk[i] = *(const uint4*)(gk + (rowbase + kv0 + key) * p.ldqkv + d0);
        }
#pragma unroll
        for (int i = 0; i < VI; ++i) {
            const int c = tid + 256 * i, pair = fp_ahd_vstage_pair(c), d0 = fp_ahd_vstage_d0(c);
            const int key = kv0 + 2 * pair;
            const bool chunk = c < VN && fp_ahd_chunk_real(d0, p.hd);
            rv0[i] = make_uint4(0u, 0u, 0u, 0u);
            rv1[i] = make_uint4(0u, 0u, 0u, 0u);
            if (chunk && fp_ahd_row_real(key, p.n_tok)) rv0[i] = *(const uint4*)(gv + (rowbase + key) * p.ldqkv + d0);
            if (chunk && fp_ahd_row_real(key + 1, p.n_tok)) rv1[i] = *(const uint4*)(gv + (rowbase + key + 1) * p.ldqkv + d0);
        }
    };
    auto write_tile = [&]() {
#pragma unroll
        for (int i = 0; i < KI; ++i) {
            const int c = tid + 256 * i;
            *(uint4*)(sK + fp_ahd_kstage_off(c, NCH, KPITCH)) = rk[i];
        }
#pragma unroll
        for (int i = 0; i < VI; ++i) {
            const int c = tid + 256 * i;
            if (c < VN) {
                auto put = [&](int w, uint32_t a, uint32_t e) {   // V^T[d][key pair]: the two keys' values of one feature side by side
                    *(uint32_t*)(sV + fp_ahd_vstage_off(c, 2 * w)) = (a & 0xffffu) | (e << 16);
                    *(uint32_t*)(sV + fp_ahd_vstage_off(c, 2 * w + 1)) = (a >> 16) | (e & 0xffff0000u);
                };
                put(0, rv0[i].x, rv1[i].x);
                put(1, rv0[i].y, rv1[i].y);
                put(2, rv0[i].z, rv1[i].z);
                put(3, rv0[i].w, rv1[i].w);
            }
        }
    };

    f32x4_t o[NDF];
#pragma unroll
    for (int i = 0; i < NDF; ++i) o[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float mrow = -1e30f;   // running maximum of the query's logits (log2 units), the same on the query's four lanes
    float lsum = 0.f;      // this lane's share of the running sum of P

    // the same count on every wave of the workgroup (causal: it depends on the block's first query only): the barriers below stay uniform
    const int ntile = CAUSAL ? fp_ahd_causal_num_tiles(qblk, p.n_tok) : fp_ahd_num_tiles(p.n_tok);
    load_tile(0);
    for (int t = 0; t < ntile; ++t) {
        const int kv0 = t * KT;
        __syncthreads();               // every wave has finished reading tile t-1
        write_tile();
        __syncthreads();
        if (t + 1 < ntile) load_tile(kv0 + KT);
        if (idle) continue;

        // ---- S^T = K Q^T ----------------------------------------------------------------------------------------------------------
        f32x4_t s[4];
#pragma unroll
        for (int fk = 0; fk < 4; ++fk) {
            s[fk] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < NKK; ++kk) {
                const bf16x8_t kf = *(const bf16x8_t*)(sK + fp_ahd_kfrag_off(fk, li, lg, kk, KPITCH));
                s[fk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kk], s[fk], 0, 0, 0);
            }
        }
        // ---- online softmax: the lane's 16 logits are keys kv0 + 32 (fk>>1) + 8 lg + 4 (fk&1) + r of query li ---------------------
        float mx = -1e30f;
#pragma unroll
        for (int fk = 0; fk < 4; ++fk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kv0 + fp_ahd_acc_key(fk, lg, r);
                const bool seen = CAUSAL ? fp_ahd_causal_visible(key, qc, p.n_tok) : fp_ahd_row_real(key, p.n_tok);
                s[fk][r] = seen ? s[fk][r] * p.scale_log2e : -1e30f;   // pad keys (causal: and future keys) are masked
                mx = fmaxf(mx, s[fk][r]);
            }
        mx = fmaxf(mx, lane_xor<16>(mx));
        mx = fmaxf(mx, lane_xor<32>(mx));
        // finite from the first tile on: key 0 is real (n_tok >= 1), lies in tile 0 and is visible to every query (0 <= q), so tile 0
        // gives every lane a finite mx.  A later tile of the causal walk may hold no visible key for a query (mx = -1e30): mnew stays
        // the finite mrow, alpha = 1, and every P of that tile is exp2(-1e30 - mnew) = 0
        const float mnew = fmaxf(mrow, mx);
        const float alpha = __builtin_amdgcn_exp2f(mrow - mnew);   // first tile: exp2(-1e30) = 0 on accumulators that are 0
        mrow = mnew;
        lsum *= alpha;
#pragma unroll
        for (int i = 0; i < NDF; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[i][r] *= alpha;
        bf16x8_t pf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            float e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = __builtin_amdgcn_exp2f(s[2 * ks + (j >> 2)][j & 3] - mnew);   // masked: exp2(-1e30) = 0
            const uint4 w = pack_bf8(e);
            // the sum runs over the bf16 values the second product multiplies by
            lsum += ((lo_bf(w.x) + hi_bf(w.x)) + (lo_bf(w.y) + hi_bf(w.y))) + ((lo_bf(w.z) + hi_bf(w.z)) + (lo_bf(w.w) + hi_bf(w.w)));
            pf[ks] = __builtin_bit_cast(bf16x8_t, w);
        }
        // ---- O^T += V^T P^T ---------------------------------------------------------------------------------------------------------
#pragma unroll
        for (int fd = 0; fd < NDF; ++fd) {
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8_t vf = *(const bf16x8_t*)(sV + fp_ahd_vfrag_off(fd, li, lg, ks));
                o[fd] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[ks], o[fd], 0, 0, 0);
            }
        }
    }
    if (idle) return;

    // ---- normalise and store: lane owns features 16 fd + 4 lg + r of query li ----------------------------------------------------------
    lsum += lane_xor<16>(lsum);
    lsum += lane_xor<32>(lsum);
    const float inv = 1.0f / lsum;       // >= 1: the row maximum contributes exp2(0)
    const int q = q0 + li;
    if (q < p.npad) {
        bf16_t* dst = p.O + (rowbase + q) * p.ldo + (size_t)h * p.hd;
#pragma unroll
        for (int fd = 0; fd < NDF; ++fd) {
            const int d0 = 16 * fd + 4 * lg;
            if (d0 < p.hd) {                   // hd % 8 == 0: a group of 4 features lies wholly inside or outside the head
                uint2 w;
                w.x = pack_bf2(o[fd][0] * inv, o[fd][1] * inv);
                w.y = pack_bf2(o[fd][2] * inv, o[fd][3] * inv);
                *(uint2*)(dst + d0) = w;
            }
        }
    }
}

// the checks and the launch of both entries; who: "attention_hd" / "attention_causal", the first word of every refusal
template <bool CAUSAL>
int launch(const bf16_t* QKV, int ldqkv, bf16_t* O, int ldo, int B, int heads, int head_dim, int n_tok, int npad, float scale, hipStream_t stream,
           const char* who) {
    FP_REQUIRE(QKV && O, "%s: null argument", who);
    FP_REQUIRE(fp_ahd_head_dim_ok(head_dim), "%s: head_dim=%d (must be a multiple of 8 in [8, 128])", who, head_dim);
    FP_REQUIRE(B > 0 && heads > 0 && n_tok > 0 && npad >= n_tok && npad % 16 == 0, "%s: bad shape B=%d heads=%d n_tok=%d npad=%d (npad %% 16 == 0, n_tok <= npad)",
               who, B, heads, n_tok, npad);
    FP_REQUIRE(ldqkv % 8 == 0 && ldo % 8 == 0 && ldqkv >= 3 * heads * head_dim && ldo >= heads * head_dim,
               "%s: leading dimensions ldqkv=%d ldo=%d (multiples of 8, at least 3 * width / width)", who, ldqkv, ldo);
    FP_REQUIRE(heads <= 65535 && B <= 65535, "%s: heads=%d B=%d exceed the grid", who, heads, B);
    AttnHdArgs a;
    a.QKV = QKV; a.ldqkv = ldqkv; a.O = O; a.ldo = ldo;
    a.heads = heads; a.hd = head_dim; a.n_tok = n_tok; a.npad = npad;
    a.scale_log2e = scale * 1.4426950408889634f;
    const dim3 grid(cdiv(npad, QBLK), heads, B);
    switch (fp_ahd_k_steps(head_dim)) {
        case 1: hipLaunchKernelGGL((attn_hd_kernel<1, CAUSAL>), grid, dim3(256), 0, stream, a); break;
        case 2: hipLaunchKernelGGL((attn_hd_kernel<2, CAUSAL>), grid, dim3(256), 0, stream, a); break;
        case 3: hipLaunchKernelGGL((attn_hd_kernel<3, CAUSAL>), grid, dim3(256), 0, stream, a); break;
        default: hipLaunchKernelGGL((attn_hd_kernel<4, CAUSAL>), grid, dim3(256), 0, stream, a); break;
    }
    FP_LAUNCH_CHECK();
    return FP_OK;
}

}  // namespace

// QKV [B*npad, 3*heads*head_dim] (ldqkv elements), O [B*npad, heads*head_dim] (ldo elements); scale multiplies q.k before the softmax
int fp_attention_hd_fwd(const bf16_t* QKV, int ldqkv, bf16_t* O, int ldo, int B, int heads, int head_dim, int n_tok, int npad, float scale,
                        hipStream_t stream) {
    return launch<false>(QKV, ldqkv, O, ldo, B, heads, head_dim, n_tok, npad, scale, stream, "attention_hd");
}
// the same under the causal mask: query t attends to keys 0 .. t
int fp_attention_causal_fwd(const bf16_t* QKV, int ldqkv, bf16_t* O, int ldo, int B, int heads, int head_dim, int n_tok, int npad, float scale,
                            hipStream_t stream) {
    return launch<true>(QKV, ldqkv, O, ldo, B, heads, head_dim, n_tok, npad, scale, stream, "attention_causal");
}
