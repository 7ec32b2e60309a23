// Index arithmetic of attention_hd.hip (both masks) and of the k-nearest-rows selection (retrieval.hip), kept free of device
// intrinsics so that a host program can run it under the sanitizers (tools/attn_hd_host_check.cpp, tools/attn_causal_host_check.cpp):
// supported shapes, the pad masks, the key-tile tail, the staging and fragment offsets into the LDS images,
// the row permutation that lines the first product's accumulators up with the second product's operand, the tile walk and visibility
// rule of the causal mask, and the tie rule of the nearest-row order.
#pragma once
#include <stdint.h>

#include "attn_core.h"   // FP_HD, and the fragment geometry this kernel shares with attention.hip

#define FP_AHD_KEY_TILE 64

// head dimensions the kernel takes: multiples of 8 (whole 16-byte chunks) up to 128
FP_HD bool fp_ahd_head_dim_ok(int hd) { return hd >= 8 && hd <= 128 && hd % 8 == 0; }
// 32-wide MFMA k steps that cover the head dimension (the rest of the last step is zero padding)
FP_HD int fp_ahd_k_steps(int hd) { return (hd + 31) / 32; }
// key tiles that hold at least one real key
FP_HD int fp_ahd_num_tiles(int n_tok) { return (n_tok + FP_AHD_KEY_TILE - 1) / FP_AHD_KEY_TILE; }
// a token row that exists (rows [n_tok, npad) are padding: never read, masked as keys)
FP_HD bool fp_ahd_row_real(int row, int n_tok) { return row < n_tok; }
// a 16-byte chunk of 8 features starting at d0 that belongs to the head (hd % 8 == 0: wholly inside or wholly outside)
FP_HD bool fp_ahd_chunk_real(int d0, int hd) { return d0 < hd; }
// K fragment fk, MFMA A-row i -> key row inside the tile; accumulator register r of fragment fk on 16-lane row lg -> key inside the tile
FP_HD int fp_ahd_tile_key(int fk, int i) { return fp_attn_tile_key(fk, i); }
FP_HD int fp_ahd_acc_key(int fk, int lg, int r) { return fp_attn_acc_key(fk, lg, r); }


// ---- LDS images of one key tile and the staging that fills them.  nch = 16-byte chunks per padded row (4 per 32-wide k step).
// K image: 64 rows of the padded head dimension, V image: its transpose (one row per feature, 64 keys); every row carries one spare
// 16-byte slot so that consecutive rows start on different banks.
#define FP_AHD_V_PITCH (FP_AHD_KEY_TILE * 2 + 16)
FP_HD constexpr int fp_ahd_chunks(int nkk) { return 4 * nkk; }
FP_HD constexpr int fp_ahd_k_pitch(int nkk) { return 64 * nkk + 16; }
// K staging item c (256 threads x nkk rounds cover the 64 x nch chunks once): key row in the tile, first feature of the chunk, byte
// offset of its 16-byte LDS write
FP_HD int fp_ahd_kstage_key(int c, int nch) { return c / nch; }
FP_HD int fp_ahd_kstage_d0(int c, int nch) { return (c % nch) * 8; }
FP_HD int fp_ahd_kstage_off(int c, int nch, int kpitch) { return fp_ahd_kstage_key(c, nch) * kpitch + fp_ahd_kstage_d0(c, nch) * 2; }
// V staging item c < 32 * nch: a PAIR of keys (2 pair, 2 pair + 1) and a chunk of 8 features; the item writes, for feature d0 + w, the
// two keys' values side by side (4 bytes) into row d0 + w of the transposed image
FP_HD constexpr int fp_ahd_vstage_items(int nch) { return 32 * nch; }
FP_HD int fp_ahd_vstage_pair(int c) { return c & 31; }
FP_HD int fp_ahd_vstage_d0(int c) { return (c >> 5) * 8; }
FP_HD int fp_ahd_vstage_off(int c, int w) { return (fp_ahd_vstage_d0(c) + w) * FP_AHD_V_PITCH + fp_ahd_vstage_pair(c) * 4; }
// 16-byte MFMA operand reads: K fragment fk, lane (li, lg), k step kk; V^T fragment fd, lane (li, lg), 32-key step ks
FP_HD int fp_ahd_kfrag_off(int fk, int li, int lg, int kk, int kpitch) { return fp_ahd_tile_key(fk, li) * kpitch + lg * 16 + kk * 64; }
FP_HD int fp_ahd_vfrag_off(int fd, int li, int lg, int ks) { return (16 * fd + li) * FP_AHD_V_PITCH + lg * 16 + ks * 64; }

// ---- causal attention (attention_hd.hip, CAUSAL = true): query t sees keys 0 .. t.  A workgroup owns FP_AHD_QUERY_BLOCK consecutive queries and
// walks the key tiles from 0 up to the one that holds the last key any of its queries sees; tiles wholly above the diagonal are never
// staged.  Pad queries (rows [n_tok, npad)) see every real key.
#define FP_AHD_QUERY_BLOCK 64
// key tiles the workgroup of queries [q0_block, q0_block + FP_AHD_QUERY_BLOCK) visits: 0 .. floor(min(q0_block + 63, n_tok - 1) / 64)
FP_HD int fp_ahd_causal_num_tiles(int q0_block, int n_tok) {
    const int last_q = q0_block + FP_AHD_QUERY_BLOCK - 1;
    const int last_key = last_q < n_tok - 1 ? last_q : n_tok - 1;
    return last_key / FP_AHD_KEY_TILE + 1;
}
// the logit (key, query) takes part in the softmax: a real key at or before the query
FP_HD bool fp_ahd_causal_visible(int key, int query, int n_tok) { return fp_ahd_row_real(key, n_tok) && key <= query; }

// ---- nearest rows: candidates are ordered by (squared distance ascending, row index ascending).  Distances are non-negative
// floats, whose bit patterns order like the values, so one 64-bit integer carries the whole rule.
FP_HD uint64_t fp_knn_key(uint32_t d2_bits, uint32_t row) { return ((uint64_t)d2_bits << 32) | row; }
FP_HD uint32_t fp_knn_key_row(uint64_t key) { return (uint32_t)(key & 0xffffffffu); }
FP_HD uint32_t fp_knn_key_bits(uint64_t key) { return (uint32_t)(key >> 32); }
