// Host check of the index arithmetic of csrc/attention_hd.hip and of the nearest-row order (csrc/attn_hd_core.h), meant to be built
// with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ifreepose_amd/csrc tools/attn_hd_host_check.cpp -o attn_hd_host_check
// It replays, for every supported head dimension and a sweep of sequence lengths, what the kernel's staging and masking do on a host
// image of the LDS tiles (so an out-of-range index is a sanitizer report), and checks the permutation and tie rules exhaustively.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "attn_hd_core.h"

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

int main() {
    // shape rule
    for (int hd = -8; hd <= 200; ++hd) CHECK(fp_ahd_head_dim_ok(hd) == (hd >= 8 && hd <= 128 && hd % 8 == 0));
    CHECK(!fp_ahd_head_dim_ok(12) && !fp_ahd_head_dim_ok(136) && fp_ahd_head_dim_ok(104));
    // the K-row permutation is a bijection of the tile, and a lane's accumulators are 8 consecutive keys per 32-key step in operand order
    std::vector<int> seen(FP_AHD_KEY_TILE, 0);
    for (int fk = 0; fk < 4; ++fk)
        for (int i = 0; i < 16; ++i) {
            const int key = fp_ahd_tile_key(fk, i);
            CHECK(key >= 0 && key < FP_AHD_KEY_TILE);
            if (key >= 0 && key < FP_AHD_KEY_TILE) seen[key]++;
        }
    for (int k = 0; k < FP_AHD_KEY_TILE; ++k) CHECK(seen[k] == 1);
    for (int ks = 0; ks < 2; ++ks)
        for (int lg = 0; lg < 4; ++lg)
            for (int j = 0; j < 8; ++j) CHECK(fp_ahd_acc_key(2 * ks + (j >> 2), lg, j & 3) == 32 * ks + 8 * lg + j);
    // staging replay: every (thread, item) of a tile lands inside the LDS images, covers them exactly once, and reads only real rows / columns
    for (int hd = 8; hd <= 128; hd += 8) {
        const int nkk = fp_ahd_k_steps(hd), hdp = 32 * nkk, nch = fp_ahd_chunks(nkk);
        CHECK(hdp >= hd && hdp - hd < 32 && nch * 8 == hdp);
        const int kpitch = fp_ahd_k_pitch(nkk), vpitch = FP_AHD_V_PITCH;
        CHECK(kpitch >= hdp * 2 && kpitch % 16 == 0 && vpitch >= FP_AHD_KEY_TILE * 2 && vpitch % 16 == 0);
        for (int n_tok : {1, 15, 16, 17, 63, 64, 65, 257, 300}) {
            const int npad = (n_tok + 15) / 16 * 16;
            const int ntile = fp_ahd_num_tiles(n_tok);
            CHECK((ntile - 1) * FP_AHD_KEY_TILE < n_tok && ntile * FP_AHD_KEY_TILE >= n_tok);
            std::vector<unsigned char> sK((size_t)FP_AHD_KEY_TILE * kpitch, 0), sV((size_t)hdp * vpitch, 0);
            std::vector<unsigned char> gmem((size_t)npad * hd, 1);       // one head's [row][column] bytes: reads must stay inside
            for (int t = 0; t < ntile; ++t) {
                const int kv0 = t * FP_AHD_KEY_TILE;
                std::fill(sK.begin(), sK.end(), 0);
                std::fill(sV.begin(), sV.end(), 0);
                for (int tid = 0; tid < 256; ++tid) {
                    for (int i = 0; i < nkk; ++i) {
                        const int c = tid + 256 * i, key = fp_ahd_kstage_key(c, nch), d0 = fp_ahd_kstage_d0(c, nch);
                        CHECK(key >= 0 && key < FP_AHD_KEY_TILE && d0 >= 0 && d0 + 8 <= hdp);
                        if (fp_ahd_row_real(kv0 + key, n_tok) && fp_ahd_chunk_real(d0, hd))
                            for (int e = 0; e < 8; ++e) CHECK(gmem[(size_t)(kv0 + key) * hd + d0 + e] == 1);
                        for (int e = 0; e < 16; ++e) sK[(size_t)fp_ahd_kstage_off(c, nch, kpitch) + e]++;
                    }
                    const int vn = fp_ahd_vstage_items(nch);
                    for (int i = 0; i < (vn + 255) / 256; ++i) {
                        const int c = tid + 256 * i, pair = fp_ahd_vstage_pair(c), d0 = fp_ahd_vstage_d0(c);
                        if (c >= vn) continue;
                        CHECK(2 * pair + 1 < FP_AHD_KEY_TILE && d0 + 8 <= hdp);
                        for (int u = 0; u < 2; ++u)
                            if (fp_ahd_row_real(kv0 + 2 * pair + u, n_tok) && fp_ahd_chunk_real(d0, hd))
                                for (int e = 0; e < 8; ++e) CHECK(gmem[(size_t)(kv0 + 2 * pair + u) * hd + d0 + e] == 1);
                        for (int w = 0; w < 8; ++w)
                            for (int e = 0; e < 4; ++e) sV[(size_t)fp_ahd_vstage_off(c, w) + e]++;
                    }
                }
                for (int key = 0; key < FP_AHD_KEY_TILE; ++key)
                    for (int bb = 0; bb < hdp * 2; ++bb) CHECK(sK[(size_t)key * kpitch + bb] == 1);
                for (int d = 0; d < hdp; ++d)
                    for (int bb = 0; bb < FP_AHD_KEY_TILE * 2; ++bb) CHECK(sV[(size_t)d * vpitch + bb] == 1);
                // fragment reads stay inside the images
                for (int fk = 0; fk < 4; ++fk)
                    for (int li = 0; li < 16; ++li)
                        for (int lg = 0; lg < 4; ++lg)
                            for (int kk = 0; kk < nkk; ++kk) {
                                const size_t off = (size_t)fp_ahd_kfrag_off(fk, li, lg, kk, kpitch);
                                CHECK(off + 16 <= sK.size() && off % 16 == 0 && off % kpitch + 16 <= (size_t)hdp * 2);
                            }
                for (int fd = 0; fd < hdp / 16; ++fd)
                    for (int li = 0; li < 16; ++li)
                        for (int lg = 0; lg < 4; ++lg)
                            for (int ks = 0; ks < 2; ++ks) {
                                const size_t off = (size_t)fp_ahd_vfrag_off(fd, li, lg, ks);
                                CHECK(off + 16 <= sV.size() && off % 16 == 0 && off % vpitch + 16 <= (size_t)FP_AHD_KEY_TILE * 2);
                            }
            }
            // every real key is unmasked in exactly one (tile, fragment, lane row, register); every pad key is masked
            std::vector<int> cnt(ntile * FP_AHD_KEY_TILE, 0);
            for (int t = 0; t < ntile; ++t)
                for (int fk = 0; fk < 4; ++fk)
                    for (int lg = 0; lg < 4; ++lg)
                        for (int r = 0; r < 4; ++r) {
                            const int key = t * FP_AHD_KEY_TILE + fp_ahd_acc_key(fk, lg, r);
                            if (fp_ahd_row_real(key, n_tok)) cnt[key]++;
                        }
            for (int k = 0; k < (int)cnt.size(); ++k) CHECK(cnt[k] == (k < n_tok ? 1 : 0));
        }
    }
    // nearest-row order: (distance ascending, row ascending); equal distances fall back to the row
    {
        const float d[6] = {0.5f, 0.25f, 0.5f, 0.0f, 0.25f, 3.0e38f};
        std::vector<uint64_t> keys;
        for (uint32_t i = 0; i < 6; ++i) {
            uint32_t bits;
            memcpy(&bits, &d[i], 4);
            keys.push_back(fp_knn_key(bits, i));
        }
        std::sort(keys.begin(), keys.end());
        const uint32_t want[6] = {3, 1, 4, 0, 2, 5};
        for (int i = 0; i < 6; ++i) CHECK(fp_knn_key_row(keys[i]) == want[i]);
        float back;
        const uint32_t b0 = fp_knn_key_bits(keys[0]);
        memcpy(&back, &b0, 4);
        CHECK(back == 0.0f);
    }
    printf(fails ? "attn_hd_host_check: %d FAILED\n" : "attn_hd_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
