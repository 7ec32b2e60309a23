// Index arithmetic of the bf16 GEMM kernels (gemm_bf16.hip, gemm_asm.hip, gemm_epilogue.h): the variant bits, the geometry of one
// instantiation, the LDS image (swizzle keys, DMA map, fragment-read map), the accumulator layout, the tile order, the K-tile ring and its
// waits, and the stream-K partition — free of device intrinsics, so that tools/gemm_core_host_check.cpp can run every map under the host
// sanitizers.  The kernels take their offsets from here.
#pragma once
#include <stdint.h>

#include "gemm_plan.h"

#ifndef FP_HD
#if defined(__HIPCC__)
#define FP_HD __host__ __device__ __forceinline__
#else
#define FP_HD static inline
#endif
#endif

namespace fp_gemm {

constexpr int BK = fp_plan::BK;          // bf16 per K stage
constexpr int ROWB = fp_plan::ROW_BYTES; // bytes per LDS row (64 bf16 = 8 slots of 16 bytes)
constexpr int DMA_BYTES = 1024;          // one LDS-DMA instruction: 64 lanes x 16 bytes = 8 LDS rows, lane-linear

// ---- gemm_bf16_kernel<BM, BN, WM, WN, EPI, VAR>: VAR is a sum of these (the values are part of the kernels' mangled names)
enum Variant : int {
    V_SETPRIO = 1,       // s_setprio around every MFMA block                                                      lab
    V_PIPELINED = 2,     // software-pipelined fragment reads (8-wave and smaller kernels)                         product: 128x128 and 64x64
    V_TABLE_GELU = 4,    // table GELU in the fc1 epilogues (0 = the direct erff expression)                       product, every tier
    V_WAVES16 = 8,       // names the 16-wave 256x256 tile in gemm_variant; no kernel reads it                     lab option only
    V_PERSIST = 32,      // persistent tile walk over a resident grid (plain loop)                                 product: 256x256
    V_STREAM_IO = 64,    // non-temporal output stores and residual loads                                          product: 256x256 above the streaming threshold
    V_SPLIT_ISSUE = 128, // X pieces behind the first fragment reads, W pieces behind the first MFMA block, raised
                         // MFMA priority (persistent kernel)                                                      product: 256x256
    V_STRIP8 = 512,      // column strips of 8 n-tiles                                                             lab
    // 1024 is read in TWO places.  With V_PIPELINED it gives the kernel a K-tile ring of run-time depth (ring()); in the tile order it
    // widens the column strips to 16 n-tiles (strip_width()), whatever the loop form.  The product's 64x64 tier carries it for the ring
    // and therefore also walks strips of 16; the lab's whole-N sweep of fc1 sets it on the persistent 256x256 kernel for the strips alone.
    V_RING_STRIP16 = 1024, //                                                                                      product: 64x64
    V_STREAM_K = 2048,   // balanced tier: the grid shares (tile, K step) units evenly (on the pipelined loop)      lab
    V_SPREAD = 4096,     // second half of a K step as one interleaved stream of MFMAs, DMA pieces and reads        lab
};
constexpr bool setprio(int var) { return (var & V_SETPRIO) != 0; }
constexpr bool pipelined(int var) { return (var & V_PIPELINED) != 0; }
constexpr bool table_gelu(int var) { return (var & V_TABLE_GELU) != 0; }
constexpr bool persist(int var) { return (var & V_PERSIST) != 0; }
constexpr bool stream_io(int var) { return (var & V_STREAM_IO) != 0; }
constexpr bool split_issue(int var) { return (var & V_SPLIT_ISSUE) != 0; }
constexpr bool ring(int var) { return pipelined(var) && (var & V_RING_STRIP16) != 0; }   // K-tile ring of run-time depth
constexpr int strip_width(int var) { return (var & V_RING_STRIP16) ? 16 : (var & V_STRIP8) ? 8 : 4; }   // n-tiles per column strip
constexpr bool lut(int epi, int var) { return fp_plan::epi_gelu(epi) && table_gelu(var); }   // the kernel keeps the GELU table in LDS
constexpr bool stream_k(int var) { return (var & V_STREAM_K) != 0; }
constexpr bool spread(int var) { return (var & V_SPREAD) != 0; }

// ---- gemm_variant (lab build): the low bits up to 1024 name a kernel variant as above; the bits from 256 on that change the PLAN or pick an
// alternative kernel are these.  2048 and 4096 are also kernel bits: an option value never reaches a template argument, launch_lab maps it.
enum LabOpt : int {
    LO_FORCE_SMALL = 256,          // never the 256x256 tier and no split
    LO_KEEP_SMALL = 2048,          // never the 64x64 tier
    LO_NEVER_SPLIT = 4096,
    LO_ASM_NEVER = 8192,           // the hand-scheduled big kernel never ...
    LO_ASM_ALWAYS = 16384,         // ... or wherever it supports the shape
    LO_TINY_UNLESS_BIG = 32768,    // one-wave tiles whenever not big
    LO_ASM_8WAVE = 65536,          // the hand-scheduled kernel's 8-wave geometry
    LO_TINY_TWO_BUFFERS = 131072,  // the 64x64 tier on two K-tile buffers
    LO_SMALL_8WAVE = 262144,       // the 128x128 tier on 8 waves
    LO_SPREAD = 524288,            // the small tiers with spread DMA issue (V_SPREAD)
    LO_ASM_SMALL = 1048576,        // the hand-scheduled 128x128 kernel as the small tier ...
    LO_ASM_SMALL_FILLED = 2097152, // ... only where the launch gives every CU a 128x128 tile
    LO_ASM_SMALL_LONG_K = 4194304, // ... only for K >= 2048
    LO_NEVER_STREAM = 8388608,
};
constexpr int LO_LOOP_MASK = V_SETPRIO | V_PIPELINED | V_TABLE_GELU;   // gemm_variant & 7: 0 = the plain baseline of the A/B runs, else 6

// ---- the geometry of one instantiation: what the kernel and its launcher both need
template <int BM, int BN, int WM, int WN, int EPI, int VAR>
struct Geo {
    static constexpr bool TRANS = fp_plan::epi_trans(EPI);
    static constexpr bool LUT = lut(EPI, VAR);
    // the table-GELU kernels keep no slab region: their slabs live in the K-tile buffer the tile's last K step read (gemm_bf16.hip)
    static constexpr bool RELOC = LUT;
    static constexpr bool RING = ring(VAR);
    static constexpr bool SK = stream_k(VAR);
    static constexpr int NW = WM * WN;
    static constexpr int TM = BM / WM / 16;   // 16-row fragments of X per wave
    static constexpr int TN = BN / WN / 16;   // 16-row fragments of W per wave
    // R operand = MFMA A slot (permuted rows, lane-contiguous outputs); C operand = B slot (plain rows)
    static constexpr int TR = TRANS ? TM : TN;
    static constexpr int TC = TRANS ? TN : TM;
    static constexpr int STAGE = (BM + BN) * ROWB;   // one K tile of both operands: X rows first, W rows behind
    static constexpr int W_OFF = BM * ROWB;
    static constexpr int IX = BM / 8 / NW;           // LDS-DMA instructions per wave per stage, X tile
    static constexpr int IW = BN / 8 / NW;
    static constexpr int IPS = IX + IW;
    static constexpr int TAB_BYTES = LUT ? fp_plan::GELU_TAB_BYTES : 0;                 // in front of the K-tile buffers (dynamic)
    static constexpr int SLAB_BYTES = RELOC ? 0 : NW * fp_plan::EPI_STAGE_BYTES;        // static LDS
    static constexpr int RING_MAX = RING ? fp_plan::ring_max(BM, BN, NW, LUT) : 2;      // deepest ring that fits
    static constexpr int SK_FLAG_BYTES = SK ? 16 : 0;                                   // arrival flag behind the ring
    static constexpr int dyn_lds(int ring_depth) { return TAB_BYTES + ring_depth * STAGE + SK_FLAG_BYTES; }
    static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "tile rows must split over waves");
    static_assert(TRANS || TR == 4, "the row-major epilogues read the accumulators in blocks of 64 features (acc_r_index)");
    static_assert(STAGE == fp_plan::stage_bytes(BM, BN) && TAB_BYTES + SLAB_BYTES == fp_plan::fixed_bytes(NW, LUT) &&
                      IPS == fp_plan::dma_per_stage(BM, BN, NW), "gemm_plan.h budgets another kernel");
    static_assert(dyn_lds(RING_MAX) + SLAB_BYTES <= fp_plan::LDS_BUDGET, "LDS budget");
};

// ---- the LDS image of a K tile: [rows][8 slots of 16 bytes]; slot s of row r sits at r * 128 + ((s ^ key(r)) << 4).  The key is applied to
// the lane's SOURCE address on the DMA side (the image is lane-linear) and again on the fragment read: the same involution on both sides.
FP_HD int key_plain(int row) { return (row >> 1) & 7; }
// rows of the permuted operand: fragment f of a 16 T-row wave tile holds rows perm_row(T, f, q), q = 0 .. 15
template <int T>
FP_HD int key_perm(int row) {
    const int rl = row % (16 * T);
    const int a = rl / (4 * T);
    const int b = rl & 3;
    return ((a << 1) | (b >> 1)) & 7;
}
FP_HD int perm_row(int T, int f, int q) { return (q >> 2) * 4 * T + 4 * f + (q & 3); }
FP_HD int slot_of(int kk, int lg, int key) { return (((kk << 2) | lg) ^ key) << 4; }   // byte offset of k-chunk 4 kk + lg in a row with `key`

// DMA piece `it` of wave `wave`: lane -> tile row and source slot; the piece lands lane-linear at lds (+ lane * 16) inside the operand's tile
struct DmaPiece { int row, src_slot, lds; };
template <int NW, class KeyFn>
FP_HD DmaPiece dma_piece(int it, int wave, int lane, KeyFn key) {
    DmaPiece d;
    d.row = (it * NW + wave) * 8 + (lane >> 3);
    const int k = key(d.row);
    d.src_slot = (lane & 7) ^ k;
    d.lds = (it * NW + wave) * DMA_BYTES;
    return d;
}
FP_HD int clamp_row(int origin, int row, int limit) { return origin + row < limit - 1 ? origin + row : limit - 1; }   // rows past the edge re-read the last one
// byte offset of a lane's 16 source bytes of K stage 0
FP_HD uint32_t dma_src(int grow, int ld, int src_slot) { return (uint32_t)grow * (uint32_t)ld * 2u + src_slot * 16; }

// fragment reads of lane (li = lane & 15, lg = lane >> 4) of wave (wm, wn): fragment f of the R operand at baseR + f * 4 rows, of the C operand at
// baseC + f * 16 rows, each + slot_of(kk, lg, key) — the keys do not depend on f
struct FragMap { int rowR0, keyR, rowC0, keyC, baseR, baseC; };
template <class G>
FP_HD FragMap frag_map(int wm, int wn, int li) {
    FragMap m;
    const int tile_r = G::TRANS ? wm * (16 * G::TM) : wn * (16 * G::TN);
    const int tile_c = G::TRANS ? wn * (16 * G::TN) : wm * (16 * G::TM);
    m.rowR0 = tile_r + (li >> 2) * 4 * G::TR + (li & 3);  // + 4 f   (= tile_r + perm_row(TR, f, li))
    m.keyR = (((li >> 2) << 1) | ((li & 3) >> 1)) & 7;    // = key_perm<TR>(row) for every f
    m.rowC0 = tile_c + li;                                // + 16 f
    m.keyC = (li >> 1) & 7;                               // = key_plain(16 f + li)
    m.baseR = (G::TRANS ? 0 : G::W_OFF) + m.rowR0 * ROWB;
    m.baseC = (G::TRANS ? G::W_OFF : 0) + m.rowC0 * ROWB;
    return m;
}

// ---- accumulators.  v_mfma_f32_16x16x32_bf16 with the R fragment in the A slot and the C fragment in the B slot: lane (li, lg) supplies
// row li, k-chunk lg of both, and receives acc[i][j][r] = sum_k R_j[4 lg + r][k] C_i[li][k].  Index inside the wave tile:
FP_HD int acc_r_index(int TR, int j, int lg, int r) { return perm_row(TR, j, 4 * lg + r); }   // TR = 4: 64 (j / 4) ... = 16 lg + 4 j + r
FP_HD int acc_c_index(int i, int li) { return 16 * i + li; }
// the init records (bias / folded LayerNorm start values) of fragment f that lane li supplies: the operand rows of the fragments above
FP_HD int init_record_r(int TR, int f, int li) { return perm_row(TR, f, li); }
FP_HD int init_record_c(int f, int li) { return 16 * f + li; }
FP_HD int init_record_c(int base, int f, int li) { return base + 16 * f + li; }   // (summed in this order: the kernels' address arithmetic)

// ---- the epilogue's row-coalescing slab of one wave: 16 rows x 128 bytes, slots swizzled with key_plain like the operand tiles.  Phase 1:
// lane (li, lg) writes its 32 bytes to row li, slots 2 lg and 2 lg + 1; phase 2: lane reads slot lane & 7 of row 8 h + (lane >> 3), h = 0, 1.
FP_HD int slab_addr(int row, int slot) { return row * ROWB + ((slot ^ key_plain(row)) << 4); }

// ---- tile order.  blockIdx -> logical id (XCD-contiguous, bijective) -> (tile_m, tile_n) in column STRIPS of SW n-tiles swept m-major: the 32
// tiles an XCD runs concurrently then cover 8 X row-panels x 4 W panels, so a strip's W slabs (<= 2 MB) stay in the XCD's 4 MB L2 for the whole
// sweep and each X panel is fetched once per strip.  (rocprofv3, fc1 with N = 4096: the plain row-major order streamed the 8 MB weight matrix
// once per 2 row-panels — FETCH_SIZE 9x the algorithmic bytes.)
}  // namespace fp_gemm
// workgroups are dealt to the 8 XCDs round-robin; the remap gives each XCD a CONTIGUOUS run of logical ids
FP_HD int fp_gemm_xcd_remap(int block, int nblocks) {
    const int q = nblocks >> 3, r = nblocks & 7, xcd = block & 7, pos = block >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}
// logical tile id -> (tile_m, tile_n) in column strips of SW n-tiles swept m-major
template <int SW = 4>
FP_HD void fp_gemm_tile_of_id(int id, int tiles_m, int tiles_n, int& tm, int& tn) {
    const int full = tiles_n / SW, tail = tiles_n - full * SW;
    const int in_full = full * tiles_m * SW;
    if (id < in_full) {
        const int strip = id / (tiles_m * SW), rem = id - strip * (tiles_m * SW);
        tm = rem / SW;
        tn = strip * SW + (rem - tm * SW);
    } else {
        const int rem = id - in_full;
        tm = rem / tail;
        tn = full * SW + (rem - tm * tail);
    }
}
template <int SW = 4>
FP_HD void fp_gemm_tile(int block, int nblocks, int tiles_m, int tiles_n, int& tm, int& tn) {
    fp_gemm_tile_of_id<SW>(fp_gemm_xcd_remap(block, nblocks), tiles_m, tiles_n, tm, tn);
}
namespace fp_gemm {

// ---- K-tile ring of the software-pipelined loop: NS slots, stage s of a segment goes to slot s % NS, NS - 1 stages in flight.  vmcnt counts
// LDS-DMA instructions in issue order, so "at most n later stages outstanding" is the immediate n * IPS (6 bits: capped at 63, which only
// makes the wait stricter when fewer instructions than that are outstanding — ring_depth never picks a ring with (NS - 1) * IPS > 63).
constexpr int VMCNT_MAX = 63;
constexpr int vmcnt_imm(int n, int ips) { return n * ips <= VMCNT_MAX ? n * ips : VMCNT_MAX; }
FP_HD int ring_next(int slot, int ns) { return slot + 1 == ns ? 0 : slot + 1; }
// before step 0: stage 0 must have landed; min(nk, ns) stages were issued
FP_HD int ring_wait_first(int nk, int ns) { return nk >= ns ? ns - 1 : 0; }
// inside step kt (kt + 1 < nk): stage kt + 1 must have landed; stages kt + 2 .. kt + ns - 1 may stay in flight (near the end of K fewer were issued: drain)
FP_HD int ring_wait_step(int kt, int nk, int ns) { return kt + ns - 1 < nk ? ns - 2 : 0; }
FP_HD int ring_last_slot(int nk, int ns) { return (nk - 1) % ns; }   // the slot the last K step read (RELOC slabs live there)

// ---- stream-K partition: G workgroups share U units (tile 0's K steps, tile 1's K steps, ...); the first `rem` take base + 1 units
struct SkPart { int base, rem; };
FP_HD SkPart sk_part(int units, int grid) { SkPart p; p.base = units / grid; p.rem = units - p.base * grid; return p; }
FP_HD int sk_first(SkPart p, int w) { return w * p.base + (w < p.rem ? w : p.rem); }              // workgroup w walks the units [first, end)
FP_HD int sk_end(SkPart p, int w) { return sk_first(p, w) + p.base + (w < p.rem ? 1 : 0); }
FP_HD int sk_wg_of(SkPart p, int u) {                                                            // the workgroup that walks unit u
    const int cut = p.rem * (p.base + 1);
    return u < cut ? u / (p.base + 1) : p.rem + (u - cut) / p.base;
}

// ---- the LDS image of the hand-scheduled kernel (gemm_asm.hip, gemm_asm_gen.py).  Same tiles, other keys: the X key is row & 7 (plain rows
// li of a fragment: conflict-free with 16-row fragments read at one k-chunk per lane group), the W key is key_perm of 64-row groups.  BT = tile
// edge, NWV = waves, RW = BT / NWV rows of each operand a wave stages, in pieces of 8 rows; piece q of a wave lands at
// (wave * RW + 8 q) * 128 of the operand's tile.  The loop adds q * 8 rows to vX0 / vW0 and XORs asm_w_piece_xor(q) into the W offset.
FP_HD uint32_t asm_vX0(uint32_t wave, uint32_t rw, uint32_t lane, uint32_t ldx2) {
    const uint32_t r8 = lane >> 3, s8 = lane & 7u;
    return (wave * rw + r8) * ldx2 + ((s8 ^ r8) << 4);                          // X: slot ^ (row & 7)
}
// W: slot ^ key_perm(row); the part of the key that depends on the piece is applied in the loop, the wave's part (8 waves of a 256-row tile: a
// wave's 32 rows are half a 64-row group) here
FP_HD uint32_t asm_vW0(uint32_t wave, uint32_t rw, uint32_t lane, uint32_t ldw2) {
    const uint32_t r8 = lane >> 3, s8 = lane & 7u;
    return (wave * rw + r8) * ldw2 + (((s8 ^ ((r8 >> 1) & 1u)) << 4) ^ (rw == 32 ? 64u * (wave & 1u) : 0u));
}
FP_HD uint32_t asm_w_piece_xor(uint32_t q) { return 32u * ((q >> 1) & 3u); }
FP_HD uint32_t asm_keyW(uint32_t li) { return 2u * (li >> 2) + ((li & 3u) >> 1); }
// fragment-read addresses of k-half 0 in buffer 0 (k-half 1: ^ 64; buffer 1: + two tiles): X fragment i at + i * 2048, W fragment jj at
// + (jj >> 2) * 8192 + (jj & 3) * 512
FP_HD uint32_t asm_vAX(uint32_t tab, uint32_t wm, uint32_t bt, uint32_t li, uint32_t lg) {
    return tab + (wm * (bt / 2) + li) * 128u + ((lg ^ (li & 7u)) << 4);
}
FP_HD uint32_t asm_vAW(uint32_t tab, uint32_t bm, uint32_t wn, uint32_t tr, uint32_t li, uint32_t lg) {
    return tab + bm * 128u + (wn * (16u * tr) + 16u * (li >> 2) + (li & 3u)) * 128u + ((lg ^ asm_keyW(li)) << 4);
}
// W rows of fragment jj in 64-row groups: the feature whose init record lane li supplies (= perm_row(4, jj & 3, li) + 64 (jj >> 2))
FP_HD int asm_record_r(int base, int jj, int li) { return base + 64 * (jj >> 2) + 16 * (li >> 2) + 4 * (jj & 3) + (li & 3); }
FP_HD int asm_record_r(int jj, int li) { return asm_record_r(0, jj, li); }

}  // namespace fp_gemm
