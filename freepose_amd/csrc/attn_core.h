// Index arithmetic of attention.hip (the head-64 kernel of the ViT blocks): geometry, kernel flavours, dispatch and the LDS maps, free of
// device intrinsics so that a host program can run it under the sanitizers (tools/attn_host_check.cpp).  attention.hip takes its
// offsets from here; attn_hd_core.h shares the fragment geometry (fp_attn_tile_key / fp_attn_acc_key).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FP_HD __host__ __device__ __forceinline__
#else
#define FP_HD static inline
#endif

namespace fp_attn {
constexpr int HD = 64;      // head dim
constexpr int KVB = 64;     // keys per tile
constexpr int QW = 32;      // queries per wave (two 16-query halves)
constexpr int NWAVE = 4;
constexpr int QB = QW * NWAVE;   // queries per workgroup
constexpr int ROWB = 128;   // bytes per LDS row (64 bf16)
constexpr int TILE = KVB * ROWB;   // 8 KiB (K tile) == 64 d-rows * 128 B (V^T tile)
constexpr int STAGE = 2 * TILE;    // one ring slot: K tile, then V^T tile
constexpr int DMA_BYTES = 1024;    // one DMA instruction: 64 lanes x 16 bytes = 8 LDS rows
constexpr int DMA_PER_TILE = 2 * TILE / (NWAVE * DMA_BYTES);   // 4 per wave (2 of K, 2 of V^T): "vmcnt(4 n)" = n tiles may still be in flight
constexpr float LAZY_THR = 40.0f;   // logits; 40 * log2(e)/8 = 7.2 -> probabilities stay below 2^8 between rescales
constexpr float THR2 = LAZY_THR * 1.4426950408889634f / 8.0f;   // the same threshold on the pre-scaled path (base-2 exponents)

// attn_fwd_kernel<NSLOT, VAR>: VAR is a sum of these (the values are part of the kernels' mangled names)
enum Flavour : int {
    PRIO = 1,           // MFMA segments at raised wave priority                                     lab
    DEPHASE = 2,        // start delay spread over the workgroups of a CU                            lab
    SHORT_FIRST = 4,    // the tail tile goes first through a half-length body                       product, when fp_attn_short_tail
    JITV = 16,          // V^T fragments read just in time: 128 registers, 4 waves per SIMD          product, always (without: the 3-wave body, lab)
    PRESCALED = 64,     // q arrives times log2(e)/8: the S^T accumulators are the exponents         product, when q_prescaled
    PKFMA = 128,        // exponent by packed FMA (unscaled q only)                                  lab
    VSUM = 256,         // row sums on the vector ALU instead of the ones MFMA (with JITV only)      lab
};
}  // namespace fp_attn

// ---- dispatch -------------------------------------------------------------------------------------------------------------------------
struct fp_attn_flavour { int nslot, var; };
// key tiles that hold at least one real key
FP_HD int fp_attn_num_tiles(int n_tok) { return (n_tok + fp_attn::KVB - 1) / fp_attn::KVB; }
// the last tile's real keys all sit in its first 32-key half (and it is not the only tile)
FP_HD bool fp_attn_short_tail(int n_tok) {
    return n_tok > fp_attn::KVB && n_tok - (fp_attn_num_tiles(n_tok) - 1) * fp_attn::KVB <= fp_attn::KVB / 2;
}
// the kernel the product runs
FP_HD fp_attn_flavour fp_attn_product_flavour(int n_tok, bool q_prescaled) {
    return {2, fp_attn::JITV | (fp_attn_short_tail(n_tok) ? fp_attn::SHORT_FIRST : 0) | (q_prescaled ? fp_attn::PRESCALED : 0)};
}
// sequence position -> key tile: softmax accumulation does not care about the order, so the short tail goes first
FP_HD int fp_attn_tile_of(bool short_first, int ntile, int sq) { return short_first ? (sq == 0 ? ntile - 1 : sq - 1) : sq; }
// tiles after step t that may still be in flight when step t waits for its own (ring of nslot: nslot - 1 staged ahead)
FP_HD int fp_attn_in_flight(int nslot, int ntile, int t) { return nslot - 2 < ntile - 1 - t ? nslot - 2 : ntile - 1 - t; }
// 1-D grid: query blocks of [q_base, npad) x heads x crops
FP_HD int fp_attn_query_blocks(int npad, int q_base) { return (npad - q_base + fp_attn::QB - 1) / fp_attn::QB; }
FP_HD int fp_attn_grid(int B, int H, int npad, int q_base) { return fp_attn_query_blocks(npad, q_base) * H * B; }
// hardware block id -> logical id.  Hardware ids go round the 8 XCDs; the map hands XCD x a run of consecutive logical ids, so the
// query blocks of one (crop, head) share an XCD's L2 copy of that head's K / V^T.  A bijection of [0, nwg).
FP_HD int fp_attn_block_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, pos = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}
// logical id -> (crop b, head h, query block qb)
struct fp_attn_block { int b, h, qb; };
FP_HD fp_attn_block fp_attn_block_of(int id, int nqb, int H) {
    const int qb = id % nqb, bh = id / nqb;
    const int h = bh % H, b = bh / H;
    return {b, h, qb};
}
// first query of a wave; a wave with q0 >= npad has no row to store (q0 is a multiple of 32, npad of 16) and only stages and syncs
FP_HD int fp_attn_wave_q0(int q_base, int qb, int wave) { return q_base + qb * fp_attn::QB + wave * fp_attn::QW; }
FP_HD bool fp_attn_wave_idle(int q0, int npad) { return q0 >= npad; }
// a tile that can reach past the crop's npad rows is staged through clamped per-lane addresses
FP_HD bool fp_attn_stage_clamped(int kv0, int npad) { return kv0 + fp_attn::KVB > npad; }
FP_HD int fp_attn_clamp_key(int kv0, int row, int npad) { return kv0 + row < npad - 1 ? kv0 + row : npad - 1; }            // K source row
FP_HD int fp_attn_clamp_group(int kv0, int group, int npad) { return kv0 + group * 8 < npad - 8 ? kv0 + group * 8 : npad - 8; }   // first key of a V^T chunk

// ---- fragment geometry (shared with attention_hd.hip) ---------------------------------------------------------------------------------
// K fragment fk (0..3), MFMA A-row i (0..15)  ->  key row inside the 64-key tile.  With this permutation a lane's S^T registers of
// fragments (2s, 2s+1) are the 8 CONSECUTIVE keys 32 s + 8 lg + j: the B-operand k-order of the P^T fragment, no cross-lane exchange.
FP_HD int fp_attn_tile_key(int fk, int i) { return 32 * (fk >> 1) + 8 * (i >> 2) + 4 * (fk & 1) + (i & 3); }
// accumulator register r of fragment fk on a lane of 16-lane row lg  ->  key inside the tile (C row 4 lg + r of that fragment)
FP_HD int fp_attn_acc_key(int fk, int lg, int r) { return fp_attn_tile_key(fk, 4 * lg + r); }
// V^T fragment fd (0..3), MFMA A-row i  ->  feature d (the O^T accumulators of a lane are then the 16 consecutive d = 16 lg + 4 fd + r)
FP_HD int fp_attn_vt_row(int fd, int i) { return 16 * (i >> 2) + 4 * fd + (i & 3); }

// ---- LDS maps of one ring slot: K image at 0 (row = key), V^T image at TILE (row = feature), 8 chunks of 16 bytes per row --------------
// Chunk c of row r sits at physical chunk c ^ key(r); the keys make both the lane-linear DMA writes and the fragment reads conflict free.
FP_HD int fp_attn_key_krow(int row) { return ((((row >> 3) & 3) << 1) | ((row >> 1) & 1)) & 7; }
FP_HD int fp_attn_key_perm4(int row) {  // rows laid out 16a + 4f + b (a,b in 0..3)
    const int rl = row & 63;
    return (((rl >> 4) << 1) | ((rl & 3) >> 1)) & 7;
}
// DMA instruction `it` (0, 1) of a wave, per image: lane -> tile row and byte written (lane-linear from a wave-uniform base)
FP_HD int fp_attn_dma_row(int it, int wave, int lane) { return (it * fp_attn::NWAVE + wave) * 8 + (lane >> 3); }
FP_HD int fp_attn_dma_base(int it, int wave) { return (it * fp_attn::NWAVE + wave) * fp_attn::DMA_BYTES; }
FP_HD int fp_attn_dma_lds(int it, int wave, int lane) { return fp_attn_dma_base(it, wave) + lane * 16; }
// ... and the chunk of the source row it fetches: K chunk (8 features) / V^T chunk (8 keys)
FP_HD int fp_attn_dma_kchunk(int row, int lane) { return (lane & 7) ^ fp_attn_key_krow(row); }
FP_HD int fp_attn_dma_vchunk(int row, int lane) { return (lane & 7) ^ fp_attn_key_perm4(row); }
// Fragment reads.  The swizzle key of a fragment row depends on the lane alone: key_krow(tile_key(fk, li)) for every fk and
// key_perm4(vt_row(fd, li)) for every fd are this one number, so a read address is a lane base plus a compile-time step.
FP_HD int fp_attn_frag_key(int li) { return (((li >> 2) << 1) | ((li & 3) >> 1)) & 7; }
FP_HD int fp_attn_kfrag_base(int li) { return ((li >> 2) * 8 + (li & 3)) * fp_attn::ROWB; }                        // tile_key(0, li) rows
FP_HD int fp_attn_kfrag_step(int fk) { return (32 * (fk >> 1) + 4 * (fk & 1)) * fp_attn::ROWB; }                  // tile_key(fk, 0) rows
FP_HD int fp_attn_vfrag_base(int li) { return fp_attn::TILE + ((li >> 2) * 16 + (li & 3)) * fp_attn::ROWB; }      // vt_row(0, li) rows
FP_HD int fp_attn_vfrag_step(int fd) { return fd * 4 * fp_attn::ROWB; }                                           // vt_row(fd, 0) rows
// logical chunk 4 k4 + lg (k4 = kk: 32-feature step of K; ks: 32-key step of V^T) under the lane's key, in bytes
FP_HD int fp_attn_frag_chunk(int k4, int lg, int key) { return (((k4 << 2) | lg) ^ key) << 4; }
FP_HD int fp_attn_kfrag_off(int fk, int li, int lg, int kk) {
    return fp_attn_kfrag_base(li) + fp_attn_kfrag_step(fk) + fp_attn_frag_chunk(kk, lg, fp_attn_frag_key(li));
}
FP_HD int fp_attn_vfrag_off(int fd, int li, int lg, int ks) {
    return fp_attn_vfrag_base(li) + fp_attn_vfrag_step(fd) + fp_attn_frag_chunk(ks, lg, fp_attn_frag_key(li));
}
