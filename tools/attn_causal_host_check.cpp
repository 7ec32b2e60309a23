// Host check of the index rules the causal flavour of attention_hd.hip adds to the others (csrc/attn_hd_core.h: fp_ahd_causal_num_tiles,
// fp_ahd_causal_visible), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ifreepose_amd/csrc tools/attn_causal_host_check.cpp -o attn_causal_host_check
// For a sweep of sequence lengths it replays, per query block, which key tiles the workgroup walks and which logits it keeps, against
// the definition (query t sees the real keys 0 .. t), on host arrays sized like the token buffer (an out-of-range row is a sanitizer
// report).  The staging and fragment offsets are those of attention_hd.hip and are checked by tools/attn_hd_host_check.cpp.
#include <stdio.h>

#include <vector>

#include "attn_hd_core.h"

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

int main() {
    CHECK(FP_AHD_QUERY_BLOCK == 64 && FP_AHD_KEY_TILE == 64);
    // the issue's example: 77 tokens, the first query block walks one tile, the second two
    CHECK(fp_ahd_causal_num_tiles(0, 77) == 1 && fp_ahd_causal_num_tiles(64, 77) == 2);
    for (int n_tok = 1; n_tok <= 300; ++n_tok) {
        const int npad = (n_tok + 15) / 16 * 16;
        const int nblk = (npad + FP_AHD_QUERY_BLOCK - 1) / FP_AHD_QUERY_BLOCK;
        std::vector<unsigned char> rows((size_t)npad, 1);                 // the token rows of one (prompt, head): reads must stay inside
        for (int blk = 0; blk < nblk; ++blk) {
            const int q0 = blk * FP_AHD_QUERY_BLOCK;
            const int ntile = fp_ahd_causal_num_tiles(q0, n_tok);
            // never more than the unmasked kernel walks, never fewer than one, and the last tile holds a real key
            CHECK(ntile >= 1 && ntile <= fp_ahd_num_tiles(n_tok) && (ntile - 1) * FP_AHD_KEY_TILE < n_tok);
            // the closed form of the header comment
            const int last_q = q0 + 63, last_key = last_q < n_tok - 1 ? last_q : n_tok - 1;
            CHECK(ntile == last_key / 64 + 1);
            // staging of the visited tiles touches real rows only (the kernel's load predicate)
            for (int t = 0; t < ntile; ++t)
                for (int key = 0; key < FP_AHD_KEY_TILE; ++key)
                    if (fp_ahd_row_real(t * FP_AHD_KEY_TILE + key, n_tok)) CHECK(rows[(size_t)t * FP_AHD_KEY_TILE + key] == 1);
            for (int q = q0; q < q0 + FP_AHD_QUERY_BLOCK && q < npad; ++q) {
                // logits kept over the visited tiles, by (fragment, lane row, register) like the kernel's softmax loop
                std::vector<int> kept((size_t)ntile * FP_AHD_KEY_TILE, 0);
                for (int t = 0; t < ntile; ++t) {
                    int in_tile = 0;
                    for (int fk = 0; fk < 4; ++fk)
                        for (int lg = 0; lg < 4; ++lg)
                            for (int r = 0; r < 4; ++r) {
                                const int key = t * FP_AHD_KEY_TILE + fp_ahd_acc_key(fk, lg, r);
                                if (fp_ahd_causal_visible(key, q, n_tok)) { kept[key]++; in_tile++; }
                            }
                    if (t == 0) CHECK(in_tile >= 1);     // the finite-maximum invariant: tile 0 shows every query at least key 0
                }
                CHECK(fp_ahd_causal_visible(0, q, n_tok));
                // exactly the definition: every real key <= q once — none of them in a skipped tile — and nothing else
                for (int key = 0; key < npad; ++key) {
                    const bool want = key < n_tok && key <= q;
                    if (key < (int)kept.size()) CHECK(kept[key] == (want ? 1 : 0));
                    else CHECK(!want);
                }
            }
            // a tile beyond the walk holds no visible logit for any query of the block (it is skipped, not masked)
            for (int key = ntile * FP_AHD_KEY_TILE; key < npad; ++key)
                for (int q = q0; q < q0 + FP_AHD_QUERY_BLOCK && q < npad; ++q) CHECK(!fp_ahd_causal_visible(key, q, n_tok));
        }
    }
    // the predicate itself
    CHECK(fp_ahd_causal_visible(5, 5, 6) && !fp_ahd_causal_visible(6, 5, 7) && !fp_ahd_causal_visible(5, 9, 5) && fp_ahd_causal_visible(4, 9, 5));
    printf(fails ? "attn_causal_host_check: %d FAILED\n" : "attn_causal_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
