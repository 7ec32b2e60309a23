// Host check of the index arithmetic of csrc/attention.hip (csrc/attn_core.h), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ifreepose_amd/csrc tools/attn_host_check.cpp -o attn_host_check
// Without arguments it checks the dispatch rules and replays the DMA and fragment maps on a host image of one LDS ring slot whose every
// 16-byte chunk is labelled with what it holds (an out-of-range index is a sanitizer report).  With arguments "B,H,n_tok" or
// "B,H,lo-hi" it also prints one dispatch record per shape (npad = n_tok rounded up to 16):
//   dispatch B H n_tok npad ntile short_tail clamped_last idle_waves half_waves nwg | tile order | hardware block id -> logical id
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "attn_core.h"

using namespace fp_attn;

static int fails = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) { if (++fails <= 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } \
    } while (0)

struct Label { int row = -1, chunk = -1, writes = 0; };

static void check_dispatch() {
    // the block remap is a bijection of [0, nwg)
    for (int nwg = 1; nwg <= 4096; ++nwg) {
        std::vector<int> seen(nwg, 0);
        for (int bid = 0; bid < nwg; ++bid) {
            const int id = fp_attn_block_remap(bid, nwg);
            CHECK(id >= 0 && id < nwg);
            if (id >= 0 && id < nwg) seen[id]++;
        }
        for (int id = 0; id < nwg; ++id) CHECK(seen[id] == 1);
    }
    // logical id -> (crop, head, query block) enumerates the grid once, query blocks of one (crop, head) consecutive
    for (int B = 1; B <= 3; ++B)
        for (int H = 1; H <= 5; ++H)
            for (int npad = 16; npad <= 400; npad += 16) {
                const int nqb = fp_attn_query_blocks(npad, 0), nwg = fp_attn_grid(B, H, npad, 0);
                CHECK(nwg == nqb * H * B && (nqb - 1) * QB < npad && nqb * QB >= npad);
                for (int id = 0; id < nwg; ++id) {
                    const fp_attn_block k = fp_attn_block_of(id, nqb, H);
                    CHECK(k.b >= 0 && k.b < B && k.h >= 0 && k.h < H && k.qb >= 0 && k.qb < nqb && (k.b * H + k.h) * nqb + k.qb == id);
                }
            }
    for (int n_tok = 1; n_tok <= 4096; ++n_tok) {
        const int ntile = fp_attn_num_tiles(n_tok), tail = n_tok - (ntile - 1) * KVB;
        CHECK((ntile - 1) * KVB < n_tok && ntile * KVB >= n_tok);
        const bool sh = fp_attn_short_tail(n_tok);
        CHECK(sh == (n_tok > 64 && tail <= 32));
        const fp_attn_flavour f0 = fp_attn_product_flavour(n_tok, false), f1 = fp_attn_product_flavour(n_tok, true);
        CHECK(f0.nslot == 2 && f1.nslot == 2 && f0.var == (JITV | (sh ? SHORT_FIRST : 0)) && f1.var == (f0.var | PRESCALED));
        // tile_of is a permutation of the tiles, the tail first exactly when the predicate holds
        for (int first = 0; first < 2; ++first) {
            std::vector<int> seen(ntile, 0);
            for (int sq = 0; sq < ntile; ++sq) {
                const int t = fp_attn_tile_of(first, ntile, sq);
                CHECK(t >= 0 && t < ntile);
                if (t >= 0 && t < ntile) seen[t]++;
                CHECK(t == (first ? (sq == 0 ? ntile - 1 : sq - 1) : sq));
            }
            for (int t = 0; t < ntile; ++t) CHECK(seen[t] == 1);
        }
        CHECK(fp_attn_tile_of(sh, ntile, 0) == (sh ? ntile - 1 : 0));
        // the mask expression marks exactly the keys >= n_tok, every tile key once, and only a tile that passes the wave-uniform test has any
        for (int t = 0; t < ntile; ++t) {
            const int kv0 = t * KVB;
            std::vector<int> seen(KVB, 0);
            int masked = 0;
            for (int fk = 0; fk < 4; ++fk)
                for (int lg = 0; lg < 4; ++lg)
                    for (int r = 0; r < 4; ++r) {
                        const int k = fp_attn_acc_key(fk, lg, r);
                        CHECK(k >= 0 && k < KVB);
                        if (k >= 0 && k < KVB) seen[k]++;
                        masked += kv0 + k >= n_tok;
                    }
            for (int k = 0; k < KVB; ++k) CHECK(seen[k] == 1);
            CHECK(masked == (kv0 + KVB > n_tok ? kv0 + KVB - n_tok : 0));
            if (sh && t == ntile - 1)   // the half-length body computes fragments 0 and 1 only: they hold every real key of the tail
                for (int fk = 2; fk < 4; ++fk)
                    for (int i = 0; i < 16; ++i) CHECK(kv0 + fp_attn_tile_key(fk, i) >= n_tok);
        }
        // the clamped staging of a tile that reaches past npad rows: sources stay inside, and differ from the plain sources only where
        // the tile position is a masked key (npad == n_tok: the K rows are then copies of the last real key)
        for (int extra = 0; extra <= 64; extra += 16) {
            const int npad = (n_tok + 15) / 16 * 16 + extra;
            for (int t = 0; t < ntile; ++t) {
                const int kv0 = t * KVB;
                if (!fp_attn_stage_clamped(kv0, npad)) {
                    CHECK(kv0 + KVB <= npad);
                    continue;
                }
                CHECK(t == ntile - 1);
                for (int row = 0; row < KVB; ++row) {
                    const int key = fp_attn_clamp_key(kv0, row, npad);
                    CHECK(key >= 0 && key < npad);
                    if (key != kv0 + row) CHECK(kv0 + row >= npad && kv0 + row >= n_tok && key == npad - 1 && (npad != n_tok || key == n_tok - 1));
                }
                for (int g = 0; g < 8; ++g) {
                    const int k8 = fp_attn_clamp_group(kv0, g, npad);
                    CHECK(k8 >= 0 && k8 <= npad - 8 && k8 % 8 == 0);
                    if (k8 != kv0 + 8 * g) CHECK(kv0 + 8 * g >= npad && kv0 + 8 * g >= n_tok);
                }
            }
        }
    }
    // waves: q0 and idle
    for (int npad = 16; npad <= 2048; npad += 16) {
        const int nqb = fp_attn_query_blocks(npad, 0);
        for (int qb = 0; qb < nqb; ++qb)
            for (int w = 0; w < NWAVE; ++w) {
                const int q0 = fp_attn_wave_q0(0, qb, w);
                CHECK(q0 == qb * QB + w * QW && fp_attn_wave_idle(q0, npad) == (q0 >= npad));
                if (qb + 1 < nqb) CHECK(!fp_attn_wave_idle(q0, npad));
            }
    }
    // the wait ladder never claims more tiles pending than were issued after tile t, and never more than the ring holds
    CHECK(DMA_PER_TILE == 4);
    for (int nslot = 2; nslot <= 4; ++nslot)
        for (int ntile = 1; ntile <= 70; ++ntile)
            for (int t = 0; t < ntile; ++t) {
                const int pf = nslot - 1;                                      // staged ahead: tiles 0 .. pf-1 before the walk, t + pf at step t
                const int issued = ntile < t + pf ? ntile : t + pf;           // before the wait of step t
                const int a = fp_attn_in_flight(nslot, ntile, t);
                CHECK(a >= 0 && a <= issued - (t + 1) && a <= nslot - 2 && a == issued - (t + 1));
            }
}

static void check_lds_maps() {
    // a lane's registers of fragments (2s, 2s+1) are the eight consecutive keys 32 s + 8 lg + j
    for (int sx = 0; sx < 2; ++sx)
        for (int lg = 0; lg < 4; ++lg)
            for (int j = 0; j < 8; ++j) CHECK(fp_attn_acc_key(2 * sx + (j >> 2), lg, j & 3) == 32 * sx + 8 * lg + j);
    // the one swizzle key of a lane is the key of every fragment row it reads
    for (int li = 0; li < 16; ++li)
        for (int f = 0; f < 4; ++f) {
            CHECK(fp_attn_frag_key(li) == fp_attn_key_krow(fp_attn_tile_key(f, li)));
            CHECK(fp_attn_frag_key(li) == fp_attn_key_perm4(fp_attn_vt_row(f, li)));
        }
    // one ring slot filled through the DMA map: chunk `c` of K row `r` is labelled (r, c), chunk of 8 keys `g` of V^T row `d` (d, g)
    std::vector<Label> lds(STAGE / 16);
    for (int img = 0; img < 2; ++img)
        for (int it = 0; it < 2; ++it)
            for (int wave = 0; wave < NWAVE; ++wave)
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = fp_attn_dma_row(it, wave, lane);
                    const int chunk = img == 0 ? fp_attn_dma_kchunk(row, lane) : fp_attn_dma_vchunk(row, lane);
                    const int byte = img * TILE + fp_attn_dma_lds(it, wave, lane);
                    CHECK(row >= 0 && row < KVB && chunk >= 0 && chunk < 8 && byte % 16 == 0);
                    CHECK(fp_attn_dma_base(it, wave) % DMA_BYTES == 0 && byte - img * TILE == row * ROWB + (lane & 7) * 16);
                    Label& l = lds.at(byte / 16);
                    l.row = row; l.chunk = chunk; l.writes++;
                }
    for (const Label& l : lds) CHECK(l.writes == 1);
    // every row holds its eight chunks once
    for (int img = 0; img < 2; ++img)
        for (int row = 0; row < KVB; ++row) {
            int mask = 0;
            for (int c = 0; c < 8; ++c) {
                const Label& l = lds.at((img * TILE + row * ROWB) / 16 + c);
                CHECK(l.row == row);
                mask |= 1 << l.chunk;
            }
            CHECK(mask == 0xff);
        }
    // fragment reads: K fragment fk of lane (li, lg) at k step kk is features 32 kk + 8 lg .. of key tile_key(fk, li);
    // V^T fragment fd at 32-key step ks is keys 32 ks + 8 lg .. of feature vt_row(fd, li)
    for (int f = 0; f < 4; ++f)
        for (int li = 0; li < 16; ++li)
            for (int lg = 0; lg < 4; ++lg)
                for (int k4 = 0; k4 < 2; ++k4) {
                    const int ko = fp_attn_kfrag_off(f, li, lg, k4), vo = fp_attn_vfrag_off(f, li, lg, k4);
                    CHECK(ko % 16 == 0 && ko >= 0 && ko < TILE && vo % 16 == 0 && vo >= TILE && vo < STAGE);
                    const Label& k = lds.at(ko / 16);
                    CHECK(k.row == fp_attn_tile_key(f, li) && k.chunk == 4 * k4 + lg);
                    const Label& v = lds.at(vo / 16);
                    CHECK(v.row == fp_attn_vt_row(f, li) && v.chunk == 4 * k4 + lg);
                    CHECK(ko == fp_attn_kfrag_base(li) + fp_attn_kfrag_step(f) + fp_attn_frag_chunk(k4, lg, fp_attn_frag_key(li)));
                }
    // O^T accumulators of a lane are 16 consecutive features: C row 4 lg + r of fragment fd is feature 16 lg + 4 fd + r
    for (int fd = 0; fd < 4; ++fd)
        for (int lg = 0; lg < 4; ++lg)
            for (int r = 0; r < 4; ++r) CHECK(fp_attn_vt_row(fd, 4 * lg + r) == 16 * lg + 4 * fd + r);
}

static void print_dispatch(int B, int H, int n_tok) {
    const int npad = (n_tok + 15) / 16 * 16, ntile = fp_attn_num_tiles(n_tok), nqb = fp_attn_query_blocks(npad, 0);
    const bool sh = (fp_attn_product_flavour(n_tok, true).var & SHORT_FIRST) != 0;
    int idle = 0, half = 0;
    for (int w = 0; w < NWAVE; ++w) {
        const int q0 = fp_attn_wave_q0(0, nqb - 1, w);
        idle += fp_attn_wave_idle(q0, npad);
        half += !fp_attn_wave_idle(q0, npad) && q0 + 16 >= npad;
    }
    const int nwg = fp_attn_grid(B, H, npad, 0);
    printf("dispatch %d %d %d %d %d %d %d %d %d %d |", B, H, n_tok, npad, ntile, (int)sh, (int)fp_attn_stage_clamped((ntile - 1) * KVB, npad), idle, half, nwg);
    for (int sq = 0; sq < ntile; ++sq) printf(" %d", fp_attn_tile_of(sh, ntile, sq));
    printf(" |");
    for (int bid = 0; bid < nwg; ++bid) printf(" %d", fp_attn_block_remap(bid, nwg));
    printf("\n");
}

int main(int argc, char** argv) {
    check_dispatch();
    check_lds_maps();
    for (int i = 1; i < argc; ++i) {
        int B, H, lo, hi;
        const int n = sscanf(argv[i], "%d,%d,%d-%d", &B, &H, &lo, &hi);
        if (n < 3 || B < 1 || H < 1 || lo < 1 || (n == 4 && hi < lo)) {
            fprintf(stderr, "attn_host_check: bad shape '%s' (B,H,n_tok or B,H,lo-hi)\n", argv[i]);
            return 2;
        }
        for (int n_tok = lo; n_tok <= (n == 4 ? hi : lo); ++n_tok) print_dispatch(B, H, n_tok);
    }
    printf(fails ? "attn_host_check: %d FAILED\n" : "attn_host_check: ok\n", fails);
    return fails ? 1 : 0;
}
