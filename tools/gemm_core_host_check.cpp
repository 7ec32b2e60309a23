// Host check of the GEMM kernels' index arithmetic (csrc/gemm_core.h), meant to be built with the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ifreepose_amd/csrc tools/gemm_core_host_check.cpp -o gemm_core_host_check
// For every product geometry (and the lab's 8-wave 128x128 one) it replays the LDS-DMA map of a K stage into a labelled image and reads every
// fragment back through the read map, counts LDS bank conflicts of every fragment read and of the epilogue slab under the ds_read_b128 model
// of the micro-architecture notes, and checks the tile order, the accumulator layout, the K-tile ring with its waits, the stream-K partition
// and the LDS budget.  Prints one "conflict ..." line per geometry and "ok" at the end; exit status 1 and "FAILED ..." lines otherwise.
// tests/test_gemm_cases_cpu.py builds and runs it.
#include <stdio.h>
#include <string.h>

#include <deque>
#include <set>
#include <vector>

#include "gemm_core.h"
#include "gemm_plan.h"

using namespace fp_gemm;

static int fails = 0;
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) { if (fails < 40) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } \
    } while (0)

// ---- ds_read_b128 / ds_write_b128 bank model: bank = (a / 4) mod 64, four passes of 16 lanes each
static const int LANE_GROUPS[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                       {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                       {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                       {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
// conflict degree of one 16-byte access per lane: the most distinct addresses that meet in one bank within a pass (1 = conflict-free)
static int conflict_degree(const int (&addr)[64]) {
    int worst = 0;
    for (const auto& grp : LANE_GROUPS) {
        std::set<int> per_bank[64];
        for (const int lane : grp)
            for (int b = 0; b < 4; ++b) per_bank[(addr[lane] / 4 + b) % 64].insert(addr[lane]);
        for (const auto& s : per_bank) worst = (int)s.size() > worst ? (int)s.size() : worst;
    }
    return worst;
}

struct Label { int op, row, chunk; };   // op 0 = X, 1 = W
static bool same(const Label& a, int op, int row, int chunk) { return a.op == op && a.row == row && a.chunk == chunk; }

// ---- one geometry of gemm_bf16_kernel: DMA -> read round trip, clamped edge rows, bank conflicts, accumulator map, LDS budget
template <class G, int BM, int BN, int WM, int WN>
static void check_geometry(const char* name) {
    constexpr int NW = G::NW, TM = G::TM, TN = G::TN, TR = G::TR, TC = G::TC;
    constexpr bool TRANS = G::TRANS;
    std::vector<Label> img(G::STAGE / 16, Label{-1, -1, -1});
    auto key_x = [](int row) { return TRANS ? key_perm<TM>(row) : key_plain(row); };
    auto key_w = [](int row) { return TRANS ? key_plain(row) : key_perm<TN>(row); };
    int written = 0;
    for (int op = 0; op < 2; ++op)
        for (int it = 0; it < (op ? G::IW : G::IX); ++it)
            for (int wave = 0; wave < NW; ++wave)
                for (int lane = 0; lane < 64; ++lane) {
                    const DmaPiece d = op ? dma_piece<NW>(it, wave, lane, key_w) : dma_piece<NW>(it, wave, lane, key_x);
                    CHECK(d.row >= 0 && d.row < (op ? BN : BM) && d.src_slot >= 0 && d.src_slot < 8);
                    const int a = (op ? G::W_OFF : 0) + d.lds + lane * 16;
                    CHECK(a >= 0 && a + 16 <= G::STAGE);
                    CHECK(img[a / 16].op == -1);   // every 16-byte chunk of the stage is written once
                    img[a / 16] = Label{op, d.row, d.src_slot};
                    ++written;
                    // the source offset is row * ld * 2 + slot * 16, rows past the edge clamped to the last one
                    for (const int limit : {1, (op ? BN : BM) - 3, (op ? BN : BM) + 5}) {
                        const int g = clamp_row(64, d.row, 64 + limit);
                        CHECK(g >= 64 && g < 64 + limit && g == (64 + d.row < 64 + limit - 1 ? 64 + d.row : 64 + limit - 1));
                        CHECK(dma_src(g, 1024, d.src_slot) == (uint32_t)g * 2048u + (uint32_t)d.src_slot * 16u);
                    }
                }
    CHECK(written == G::STAGE / 16 && written == G::IPS * NW * 64);
    int worst_r = 0, worst_c = 0;
    for (int wave = 0; wave < NW; ++wave) {
        const int wm = wave / WN, wn = wave % WN;
        const int tile_r = TRANS ? wm * 16 * TM : wn * 16 * TN, tile_c = TRANS ? wn * 16 * TN : wm * 16 * TM;
        for (int kk = 0; kk < 2; ++kk) {
            for (int f = 0; f < TR; ++f) {
                int addr[64];
                for (int lane = 0; lane < 64; ++lane) {
                    const int li = lane & 15, lg = lane >> 4;
                    const FragMap m = frag_map<G>(wm, wn, li);
                    CHECK(m.keyR == key_perm<TR>(m.rowR0 + 4 * f) && m.rowR0 + 4 * f == tile_r + perm_row(TR, f, li));
                    addr[lane] = m.baseR + f * 4 * ROWB + slot_of(kk, lg, m.keyR);
                    CHECK(addr[lane] >= 0 && addr[lane] + 16 <= G::STAGE);
                    // the swapped-form v_mfma_f32_16x16x32_bf16 operand: lane (li, lg) supplies row li of the fragment, k-chunk 4 kk + lg
                    CHECK(same(img[addr[lane] / 16], TRANS ? 0 : 1, tile_r + perm_row(TR, f, li), 4 * kk + lg));
                }
                const int d = conflict_degree(addr);
                worst_r = d > worst_r ? d : worst_r;
            }
            for (int f = 0; f < TC; ++f) {
                int addr[64];
                for (int lane = 0; lane < 64; ++lane) {
                    const int li = lane & 15, lg = lane >> 4;
                    const FragMap m = frag_map<G>(wm, wn, li);
                    CHECK(m.keyC == key_plain(m.rowC0 + 16 * f));
                    addr[lane] = m.baseC + f * 16 * ROWB + slot_of(kk, lg, m.keyC);
                    CHECK(addr[lane] >= 0 && addr[lane] + 16 <= G::STAGE);
                    CHECK(same(img[addr[lane] / 16], TRANS ? 1 : 0, tile_c + init_record_c(f, li), 4 * kk + lg));
                }
                const int d = conflict_degree(addr);
                worst_c = d > worst_c ? d : worst_c;
            }
        }
    }
    // accumulator map: (i, j, r, lane) -> (C index, R index) is a bijection of the wave tile; fragment j's init record of lane li is the
    // operand row whose outputs acc[.][j][.] are; the row-major epilogues' block layout (RegAcc::load16 / AgprAcc::load16)
    std::vector<char> seen(16 * TC * 16 * TR, 0);
    for (int i = 0; i < TC; ++i)
        for (int j = 0; j < TR; ++j)
            for (int r = 0; r < 4; ++r)
                for (int lane = 0; lane < 64; ++lane) {
                    const int li = lane & 15, lg = lane >> 4;
                    const int c = acc_c_index(i, li), ri = acc_r_index(TR, j, lg, r);
                    CHECK(c >= 0 && c < 16 * TC && ri >= 0 && ri < 16 * TR);
                    CHECK(!seen[c * 16 * TR + ri]);
                    seen[c * 16 * TR + ri] = 1;
                    CHECK(ri == init_record_r(TR, j, 4 * lg + r) && c == init_record_c(i, li));
                    // block (I, G) of load16: v[4 j' + r] = acc[I][4 G + j'][r] is feature 64 G + 16 lg + 4 j' + r of token 16 I + li
                    if (!TRANS) CHECK(ri == 64 * (j / 4) + 16 * lg + 4 * (j % 4) + r && c == 16 * i + li && ri == asm_record_r(j, 4 * lg + r));
                    else CHECK(ri == lg * 4 * TR + 4 * j + r);   // transposed store: 4 TR consecutive tokens per lane
                }
    // LDS budget at the deepest ring (Geo's static_asserts hold the same at compile time)
    CHECK(G::dyn_lds(G::RING_MAX) + G::SLAB_BYTES <= fp_plan::LDS_BUDGET && G::RING_MAX >= 2 && G::RING_MAX <= 8);
    printf("conflict %s R=%d C=%d ips=%d ring_max=%d lds=%d\n", name, worst_r, worst_c, G::IPS, G::RING_MAX, G::dyn_lds(G::RING_MAX) + G::SLAB_BYTES);
}

// ---- the epilogue's slab: phase-1 write (lane (li, lg): row li, slots 2 lg and 2 lg + 1) and phase-2 read (slot lane & 7 of row 8 h + lane / 8)
static void check_slab() {
    std::vector<int> owner(fp_plan::EPI_STAGE_BYTES / 16, -1);
    int worst_w = 0, worst_r = 0;
    for (int half = 0; half < 2; ++half) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
            const int li = lane & 15, lg = lane >> 4;
            addr[lane] = slab_addr(li, 2 * lg + half);
            CHECK(addr[lane] >= 0 && addr[lane] + 16 <= fp_plan::EPI_STAGE_BYTES && owner[addr[lane] / 16] == -1);
            owner[addr[lane] / 16] = li * 8 + 2 * lg + half;   // (row, 8-feature chunk)
        }
        const int d = conflict_degree(addr);
        worst_w = d > worst_w ? d : worst_w;
    }
    for (int h = 0; h < 2; ++h) {
        int addr[64];
        for (int lane = 0; lane < 64; ++lane) {
            const int row = 8 * h + (lane >> 3), slot = lane & 7;
            addr[lane] = slab_addr(row, slot);
            CHECK(owner[addr[lane] / 16] == row * 8 + slot);
        }
        const int d = conflict_degree(addr);
        worst_r = d > worst_r ? d : worst_r;
    }
    printf("conflict slab write=%d read=%d\n", worst_w, worst_r);
}

// ---- the hand-scheduled kernel's image, from its lane constants: BT x BT tile on NWV waves (two wave rows)
static void check_asm_image(const char* name, int BT, int NWV) {
    const int WN = NWV / 2, RW = BT / NWV, PCS = BT / 8 / NWV, TC = BT / 2 / 16, TR = BT / WN / 16, XTILE = BT * 128;
    const uint32_t LD2 = 1u << 14;   // bytes per source row: offsets decode as row * LD2 + slot * 16
    std::vector<Label> img(2 * XTILE / 16, Label{-1, -1, -1});
    for (int wave = 0; wave < NWV; ++wave)
        for (int q = 0; q < PCS; ++q)
            for (int lane = 0; lane < 64; ++lane) {
                const uint32_t ox = asm_vX0(wave, RW, lane, LD2) + q * 8 * LD2;
                const uint32_t ow = (asm_vW0(wave, RW, lane, LD2) + q * 8 * LD2) ^ asm_w_piece_xor(q);
                const int dst = (wave * RW + 8 * q) * 128 + lane * 16;   // piece q of the wave, lane-linear
                CHECK(img[dst / 16].op == -1 && img[(XTILE + dst) / 16].op == -1);
                img[dst / 16] = Label{0, (int)(ox / LD2), (int)(ox % LD2) / 16};
                img[(XTILE + dst) / 16] = Label{1, (int)(ow / LD2), (int)(ow % LD2) / 16};
                CHECK((int)(ox / LD2) == wave * RW + 8 * q + (lane >> 3) && (int)(ow / LD2) == wave * RW + 8 * q + (lane >> 3) && ox % LD2 < 128 && ow % LD2 < 128);
            }
    int worst_x = 0, worst_w = 0;
    for (int wave = 0; wave < NWV; ++wave) {
        const int wm = wave / WN, wn = wave % WN;
        for (int kh = 0; kh < 2; ++kh) {
            for (int i = 0; i < TC; ++i) {
                int addr[64];
                for (int lane = 0; lane < 64; ++lane) {
                    const int li = lane & 15, lg = lane >> 4;
                    addr[lane] = (int)(asm_vAX(0, wm, BT, li, lg) ^ (64u * kh)) + i * 2048;
                    CHECK(addr[lane] >= 0 && addr[lane] + 16 <= XTILE);
                    CHECK(same(img[addr[lane] / 16], 0, wm * (BT / 2) + init_record_c(i, li), 4 * kh + lg));
                }
                const int d = conflict_degree(addr);
                worst_x = d > worst_x ? d : worst_x;
            }
            for (int jj = 0; jj < TR; ++jj) {
                int addr[64];
                for (int lane = 0; lane < 64; ++lane) {
                    const int li = lane & 15, lg = lane >> 4;
                    addr[lane] = (int)(asm_vAW(0, BT, wn, TR, li, lg) ^ (64u * kh)) + (jj >> 2) * 8192 + (jj & 3) * 512;
                    CHECK(addr[lane] >= XTILE && addr[lane] + 16 <= 2 * XTILE);
                    CHECK(same(img[addr[lane] / 16], 1, wn * 16 * TR + asm_record_r(jj, li), 4 * kh + lg));
                }
                const int d = conflict_degree(addr);
                worst_w = d > worst_w ? d : worst_w;
            }
        }
    }
    printf("conflict %s W=%d X=%d\n", name, worst_w, worst_x);
}

// ---- tile order
template <int SW>
static void check_order_one(int tiles_m, int tiles_n) {
    const int n = tiles_m * tiles_n;
    std::vector<char> seen(n, 0);
    for (int b = 0; b < n; ++b) {
        int tm = -1, tn = -1, tm2 = -1, tn2 = -1;
        fp_gemm_tile<SW>(b, n, tiles_m, tiles_n, tm, tn);
        fp_gemm_tile_of_id<SW>(fp_gemm_xcd_remap(b, n), tiles_m, tiles_n, tm2, tn2);
        CHECK(tm == tm2 && tn == tn2 && tm >= 0 && tm < tiles_m && tn >= 0 && tn < tiles_n);
        if (tm < 0 || tm >= tiles_m || tn < 0 || tn >= tiles_n) return;
        CHECK(!seen[tm * tiles_n + tn]);
        seen[tm * tiles_n + tn] = 1;
    }
    // a persistent grid G % 8 == 0: workgroup b walks tiles b, b + G, ...; every one of them lies in the logical-id run of XCD b & 7
    const int q = n >> 3, r = n & 7;
    for (int b = 0; b < n; ++b) {
        const int xcd = b & 7, lo = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q, id = fp_gemm_xcd_remap(b, n);
        CHECK(id >= lo && id < lo + q + (xcd < r ? 1 : 0));
    }
}
static void check_order(int tiles_m, int tiles_n) {
    check_order_one<4>(tiles_m, tiles_n);
    check_order_one<8>(tiles_m, tiles_n);
    check_order_one<16>(tiles_m, tiles_n);
}

// ---- K-tile ring and waits: `ips` LDS-DMA instructions per stage, a ring kernel (run-time wait) or a two-buffer one (drains)
static void check_ring(int ns, int nk, int ips, bool ring_kernel) {
    std::deque<int> inflight;            // stage of every outstanding DMA instruction, issue order (vmcnt retires in order)
    std::vector<int> slot_stage(ns, -1);
    auto issue = [&](int stage, int slot) {
        CHECK(slot == stage % ns);
        slot_stage[slot] = stage;
        for (int i = 0; i < ips; ++i) inflight.push_back(stage);
    };
    auto wait = [&](int imm) {
        CHECK(imm >= 0 && imm <= VMCNT_MAX);
        while ((int)inflight.size() > imm) inflight.pop_front();
    };
    auto landed = [&](int stage) { for (const int s : inflight) if (s == stage) return false; return true; };
    for (int s = 0; s < ns; ++s)
        if (s < nk) issue(s, s);
    wait(ring_kernel ? vmcnt_imm(ring_wait_first(nk, ns), ips) : (nk > 1 ? vmcnt_imm(1, ips) : 0));
    CHECK(landed(0));
    int cur = 0, last_read = -1;
    for (int kt = 0; kt < nk; ++kt) {
        CHECK(slot_stage[cur] == kt && landed(kt));   // both halves of stage kt are read from `cur`
        last_read = cur;
        const int nxt = ring_next(cur, ns);
        if (kt + 1 < nk) {
            wait(ring_kernel ? vmcnt_imm(ring_wait_step(kt, nk, ns), ips) : 0);
            CHECK(landed(kt + 1) && slot_stage[nxt] == kt + 1);
            // (barrier) every wave is done reading stage kt: its slot is free for stage kt + ns
            if (kt + ns < nk) { CHECK(slot_stage[cur] == kt); issue(kt + ns, cur); }
        }
        cur = nxt;
    }
    CHECK(ring_last_slot(nk, ns) == last_read);
    if (ns == 2) CHECK(((nk - 1) & 1) == last_read);   // the plain loop's form of the same slot
}

// ---- stream-K partition
static void check_stream_k(int ntiles, int nkt, int G) {
    const int U = ntiles * nkt;
    const SkPart p = sk_part(U, G);
    int u = 0;
    for (int w = 0; w < G; ++w) {
        CHECK(sk_first(p, w) == u && sk_end(p, w) > sk_first(p, w));
        for (int v = sk_first(p, w); v < sk_end(p, w); ++v) CHECK(sk_wg_of(p, v) == w);
        u = sk_end(p, w);
    }
    CHECK(u == U);
    for (int t = 0; t < ntiles; ++t) {
        const int ut0 = t * nkt, w_first = sk_wg_of(p, ut0), nsl = sk_wg_of(p, ut0 + nkt - 1) - w_first + 1;
        std::set<int> wgs;
        for (int k = 0; k < nkt; ++k) wgs.insert(sk_wg_of(p, ut0 + k));
        CHECK((int)wgs.size() == nsl && *wgs.begin() == w_first && *wgs.rbegin() == w_first + nsl - 1);
        // slice 0 (the one that carries the init) is the first workgroup's, and it holds K step 0
        CHECK(sk_first(p, w_first) <= ut0 && ut0 < sk_end(p, w_first));
        for (int sl = 1; sl < nsl; ++sl) CHECK(sk_first(p, w_first + sl) > ut0);   // later slices start inside the tile: kt0 > 0
    }
}

int main() {
    // the variant values are the kernels' mangled names
    static_assert(V_SETPRIO == 1 && V_PIPELINED == 2 && V_TABLE_GELU == 4 && V_WAVES16 == 8 && V_PERSIST == 32 && V_STREAM_IO == 64 && V_SPLIT_ISSUE == 128 &&
                      V_STRIP8 == 512 && V_RING_STRIP16 == 1024 && V_STREAM_K == 2048 && V_SPREAD == 4096, "variant bits");
    constexpr int BIG = V_TABLE_GELU | V_PERSIST | V_STREAM_IO | V_SPLIT_ISSUE, SMALL = V_PIPELINED | V_TABLE_GELU, TINY = SMALL | V_RING_STRIP16;
    static_assert(strip_width(BIG) == 4 && strip_width(SMALL) == 4 && strip_width(TINY) == 16 && strip_width(BIG | V_STRIP8) == 8 && strip_width(BIG | V_RING_STRIP16) == 16,
                  "strip widths: the product's tiny tier walks strips of 16");
    static_assert(ring(TINY) && !ring(SMALL) && !ring(BIG | V_RING_STRIP16) && persist(BIG) && !pipelined(BIG) && pipelined(TINY) && !stream_k(TINY) && !spread(TINY) &&
                      lut(FP_EPI_BIAS_GELU, SMALL) && lut(FP_EPI_LN_GELU, BIG) && !lut(FP_EPI_BIAS, BIG) && !lut(FP_EPI_BIAS_GELU, 0), "predicates");
    static_assert(vmcnt_imm(0, 16) == 0 && vmcnt_imm(3, 16) == 48 && vmcnt_imm(4, 16) == 63 && vmcnt_imm(7, 8) == 56, "vmcnt immediates");

    check_geometry<Geo<256, 256, 4, 4, FP_EPI_BIAS, BIG>, 256, 256, 4, 4>("big256_4x4");
    check_geometry<Geo<256, 256, 4, 4, FP_EPI_BIAS_GELU, BIG>, 256, 256, 4, 4>("big256_4x4_gelu");
    check_geometry<Geo<256, 256, 4, 4, FP_EPI_VT, BIG>, 256, 256, 4, 4>("big256_4x4_trans");
    check_geometry<Geo<128, 128, 2, 2, FP_EPI_BIAS, SMALL>, 128, 128, 2, 2>("small128_2x2");
    check_geometry<Geo<128, 128, 2, 2, FP_EPI_LN_GELU, SMALL>, 128, 128, 2, 2>("small128_2x2_gelu");
    check_geometry<Geo<128, 128, 2, 2, FP_EPI_LN_VT, SMALL>, 128, 128, 2, 2>("small128_2x2_trans");
    check_geometry<Geo<64, 64, 2, 1, FP_EPI_BIAS, TINY>, 64, 64, 2, 1>("tiny64_2x1");
    check_geometry<Geo<64, 64, 2, 1, FP_EPI_BIAS_GELU, TINY>, 64, 64, 2, 1>("tiny64_2x1_gelu");
    check_geometry<Geo<64, 64, 1, 1, FP_EPI_VT, TINY>, 64, 64, 1, 1>("tiny64_1x1_trans");
    check_geometry<Geo<128, 128, 4, 2, FP_EPI_BIAS, SMALL>, 128, 128, 4, 2>("lab128_4x2");
    check_geometry<Geo<128, 128, 2, 4, FP_EPI_VT, SMALL>, 128, 128, 2, 4>("lab128_2x4_trans");
    check_slab();
    check_asm_image("asm256_4waves", 256, 4);
    check_asm_image("asm256_8waves", 256, 8);
    check_asm_image("asm128_4waves", 128, 4);

    for (int tm = 1; tm <= 40; ++tm)
        for (int tn = 1; tn <= 40; ++tn) check_order(tm, tn);
    // the flagship batch: M = 288 crops x 1376 tokens at the ViT-L widths, on 256 and 128 tiles (N = 3072: a ragged last strip at 8 and 16)
    for (const int n : {1024, 2048, 3072, 4096})
        for (const int t : {256, 128}) check_order((int)fp_plan::cdiv(288L * 1376, t), n / t);
    check_order((int)fp_plan::cdiv(1376, 64), 1024 / 64);   // a single crop on the 64x64 tier

    for (int ns = 2; ns <= 8; ++ns)
        for (int nk = 1; nk <= 40; ++nk)
            for (const int ips : {4, 8, 16}) {   // 8-wave 128x128 / the small and tiny tiers / the one-wave tiny tier
                check_ring(ns, nk, ips, true);
                if (ns == 2) check_ring(ns, nk, ips, false);
            }
    // RELOC: the persistent walk puts the slabs into the buffer the tile's last K step read — never the one the next tile's prefetch targets
    for (int nkt = 1; nkt <= 40; ++nkt)
        for (int g0 = 0; g0 < 2; ++g0) {
            const int g_last = g0 + nkt - 1, prefetch = (g_last + 1) & 1, g_after = g_last + 1;
            CHECK(((g_after - 1) & 1) != prefetch && ((g_after - 1) & 1) == (g_last & 1));
        }

    for (int ntiles = 1; ntiles <= 12; ++ntiles)
        for (const int nkt : {1, 2, 3, 5, 16})
            for (int G = 1; G <= ntiles * nkt; ++G) check_stream_k(ntiles, nkt, G);

    if (fails) { printf("%d checks FAILED\n", fails); return 1; }
    puts("ok");
    return 0;
}
