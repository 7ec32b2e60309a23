// bf16 MFMA GEMM with fused ViT epilogues, gfx950 only.
//
// Structure (one workgroup = BM x BN output tile, BK = 64 per pipeline stage):
//   * both operand tiles are staged HBM -> LDS with global_load_lds (16 B/lane, no VGPR round trip);
//     the LDS image is lane-linear, so the bank swizzle is applied to the per-lane SOURCE address and
//     again on the ds_read address (same involution on both sides);
//   * tiles are [rows][64 bf16] = 128-B rows; the 16-B slot index is XORed with a 3-bit key that is
//     distinct for the rows one ds_read_b128 lane group touches (tools/gemm_core_host_check.cpp prints the
//     conflict degree of every fragment read under the bank model of the micro-architecture notes);
//   * MFMA is v_mfma_f32_16x16x32_bf16 in the SWAPPED form: the operand whose index must end up
//     contiguous in a lane's accumulators (output features n for the normal epilogues, tokens m for
//     the transposed V store) goes into the A slot with a PERMUTED row->fragment map, so one lane owns
//     16 (or 32) consecutive outputs and the epilogue stores full 16-B vectors / 128-B lines;
//   * double-buffered LDS, one barrier per K tile, next tile's DMA issued before the MFMA block;
//   * XCD-aware tile order: consecutive tiles of one X row-panel stay on one XCD's L2.
// The index arithmetic of all of this — variant bits, geometry, swizzle keys, DMA and fragment maps, accumulator layout, tile order, ring
// and waits, stream-K partition — is stated in gemm_core.h and checked on a CPU by tools/gemm_core_host_check.cpp.
//
// Reference op being replaced: the nn.Linear calls inside the hub DINOv2 blocks driven by
// src/pipeline/retrieval/dino.py:16-23 (patch_embed.proj, attn.qkv, attn.proj, mlp.fc1, mlp.fc2).
#include "gemm_bf16.h"
#include "gemm_epilogue.h"
#include "internal.h"

#include <mutex>

// The PRODUCT build (libfreepose_hip.so) instantiates exactly one kernel per (epilogue, tile tier) — the variants below that the
// rounds' A/B runs selected — reads no environment variable and has no measurement hooks.  The LAB build (-DFP_LAB,
// libfreepose_hip_lab.so, loaded only by tools/) additionally compiles the alternative main loops / tile shapes and selects them
// through fp_lab_set_option("gemm_variant" / "gemm_dbg") or FP_GEMM_VARIANT / FP_GEMM_DBG.
#ifdef FP_LAB
#include <stdlib.h>
#endif
// the kernel variant bits (template parameter VAR) are fp_gemm::Variant of gemm_core.h.  The product always runs these; only the lab build
// can change them (gemm_variant; its default names the product's big tile: profiles/r02_ab.md, +4..6 % over 110 on every ViT shape)
#define FP_GEMM_VAR_BIG (fp_gemm::V_TABLE_GELU | fp_gemm::V_PERSIST | fp_gemm::V_STREAM_IO | fp_gemm::V_SPLIT_ISSUE)   // 16-wave 256x256
#define FP_GEMM_VAR_SMALL (fp_gemm::V_PIPELINED | fp_gemm::V_TABLE_GELU)                                              // 128x128 (4 waves)
#define FP_GEMM_VAR_TINY (FP_GEMM_VAR_SMALL | fp_gemm::V_RING_STRIP16)   // 64x64 (2 waves, 1 for the transposed store): K-tile ring, strips of 16
#define FP_GEMM_DEFAULT_VARIANT (FP_GEMM_VAR_BIG | fp_gemm::V_PIPELINED | fp_gemm::V_WAVES16)   // 238
static_assert(FP_GEMM_VAR_BIG == 228 && FP_GEMM_VAR_SMALL == 6 && FP_GEMM_VAR_TINY == 1030 && FP_GEMM_DEFAULT_VARIANT == 238, "the kernels' mangled names");

namespace {

using fp_gemm::BK;     // bf16 per K stage  (128-byte LDS rows)
using fp_gemm::ROWB;   // bytes per LDS row
using fp_gemm::key_perm;
using fp_gemm::key_plain;

// ---- measurement hooks of the lab build (gemm_dbg bits; wrong numerics, tools/step_ablate.py and tools/gemm_phases.py).  The product sees
// empty inlines: no hook costs it an instruction.
enum LabDbg : int {
    DBG_ZERO_INIT = 2,      // LN-folded kernels start from zero accumulators
    DBG_NO_EPILOGUE = 8,    // persistent kernels skip the epilogue (one store keeps the accumulators live)
    DBG_STAGGER = 32,       // staggered start of the persistent workgroups
    DBG_NO_DMA = 64,        // pipelined loop: no DMA in the steady state,
    DBG_NO_MFMA = 128,      // no MFMAs,
    DBG_NO_READS = 256,     // no fragment reads,
    DBG_NO_BARRIER = 512,   // no barrier — what a K step of the small tiers is made of: profiles/r05_ab.md
    DBG_PHASES = 1024,      // phase timestamps of every workgroup's wave 0 into the scratch buffer
    DBG_STAMPS = 2048,      // shader-clock stamps inside K step 8
};
#ifdef FP_LAB
__device__ __forceinline__ bool lab_on(const FpGemmArgs& p, int bit) { return FP_GEMM_DBG_BIT(p, bit); }
// stagger the resident workgroups over one tile period so that the chip's 256 epilogues (each a 128 KiB store burst) do not all hit the
// memory system at the same moment
__device__ __forceinline__ void lab_stagger(const FpGemmArgs& p) {
    if (lab_on(p, DBG_STAGGER)) {
        const int phase = (blockIdx.x >> 3) & 7;
        const int n = phase * (p.K / BK) * 6;      // ~ phase/8 of a tile: a K step is ~3 000 cycles = 48 x s_sleep(1)
        for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(1);
    }
}
// phase timestamps (100 MHz wall clock): 0 entry, 1 first K tile landed, 2 K loop done, 3 epilogue done (tools/step_ablate.py phases)
struct LabPhases { unsigned long long t[4] = {0, 0, 0, 0}, c0 = 0; };
__device__ __forceinline__ void lab_phase(const FpGemmArgs& p, LabPhases& ph, int i) {
    if (lab_on(p, DBG_PHASES)) {
        ph.t[i] = wall_clock64();
        if (i == 0) ph.c0 = __builtin_amdgcn_s_memtime();
    }
}
__device__ __forceinline__ void lab_phases_write(const FpGemmArgs& p, LabPhases& ph, int tid) {
    if (lab_on(p, DBG_PHASES) && p.sk_ws && tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ph.t[3] = wall_clock64();
        unsigned long long* o = (unsigned long long*)p.sk_ws + (size_t)blockIdx.x * 5;
        o[0] = ph.t[0]; o[1] = ph.t[1]; o[2] = ph.t[2]; o[3] = ph.t[3]; o[4] = __builtin_amdgcn_s_memtime() - ph.c0;   // shader clocks
    }
}
// shader-clock stamps inside K step 8 (wave 0 of every workgroup) — where the wave waits
struct LabStamps { bool on = false; unsigned long long st[8]; };
__device__ __forceinline__ void lab_stamps_arm(const FpGemmArgs& p, LabStamps& s, int kt) { s.on = lab_on(p, DBG_STAMPS) && kt == 8 && p.sk_ws; }
__device__ __forceinline__ void lab_stamp(LabStamps& s, int i) {
    if (s.on) { asm volatile("" ::: "memory"); s.st[i] = __builtin_amdgcn_s_memtime(); asm volatile("" ::: "memory"); }
}
__device__ __forceinline__ void lab_stamps_write(const FpGemmArgs& p, const LabStamps& s, int tid) {
    if (s.on && tid == 0) {
        unsigned long long* o = (unsigned long long*)p.sk_ws + 65536 + (size_t)blockIdx.x * 8;
        for (int i = 0; i < 8; ++i) o[i] = s.st[i];
    }
}
#else
__device__ __forceinline__ constexpr bool lab_on(const FpGemmArgs&, int) { return false; }
__device__ __forceinline__ void lab_stagger(const FpGemmArgs&) {}
struct LabPhases {};
__device__ __forceinline__ void lab_phase(const FpGemmArgs&, LabPhases&, int) {}
__device__ __forceinline__ void lab_phases_write(const FpGemmArgs&, LabPhases&, int) {}
struct LabStamps {};
__device__ __forceinline__ void lab_stamps_arm(const FpGemmArgs&, LabStamps&, int) {}
__device__ __forceinline__ void lab_stamp(LabStamps&, int) {}
__device__ __forceinline__ void lab_stamps_write(const FpGemmArgs&, const LabStamps&, int) {}
#endif

// "at most N later stages' LDS-DMA instructions outstanding" (vmcnt counts in issue order and takes an immediate: fp_gemm::vmcnt_imm);
// LG: also lgkmcnt(0)
template <int IPS, int N, bool LG>
__device__ __forceinline__ void wait_imm() {
    if constexpr (LG) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(fp_gemm::vmcnt_imm(N, IPS)) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(fp_gemm::vmcnt_imm(N, IPS)) : "memory");
}
// the run-time form of a ring kernel (n = 0 .. 7 stages; anything else drains); a two-buffer kernel always drains
template <int IPS, bool RING, bool LG>
__device__ __forceinline__ void wait_stages(int n) {
    if constexpr (!RING) {
        wait_imm<IPS, 0, LG>();
    } else {
        switch (n) {
            case 1: wait_imm<IPS, 1, LG>(); break;
            case 2: wait_imm<IPS, 2, LG>(); break;
            case 3: wait_imm<IPS, 3, LG>(); break;
            case 4: wait_imm<IPS, 4, LG>(); break;
            case 5: wait_imm<IPS, 5, LG>(); break;
            case 6: wait_imm<IPS, 6, LG>(); break;
            case 7: wait_imm<IPS, 7, LG>(); break;
            default: wait_imm<IPS, 0, LG>();
        }
    }
}

// which operand's pieces a stage() call issues
constexpr std::integral_constant<int, 1> STAGE_X{};
constexpr std::integral_constant<int, 2> STAGE_W{};
constexpr std::integral_constant<int, 3> STAGE_BOTH{};

// The kernel, in the order it runs: set_tile -> stage (prefetch) -> finalize_tile_rows -> init_acc -> one of the three K loops (persistent
// walk / plain / software-pipelined) -> [stream-K: the segment set-up in front, the partial-tile fix-up behind] -> epilogue.  The small stages are
// lambdas over the kernel's locals.  The three K loops and the stream-K fix-up stay INLINE, in the order the compiler has always seen them:
// moved into lambdas of their own (or into member functions of a context struct) hipcc schedules every product kernel differently — other
// register assignment, other order of fragment reads and MFMAs (profiles/gemm_kernel_refactor.md, steps left in place).
template <int BM, int BN, int WM, int WN, int EPI, int VAR>
__global__ __launch_bounds__(WM* WN * 64) void gemm_bf16_kernel(FpGemmArgs p) {
    using G = fp_gemm::Geo<BM, BN, WM, WN, EPI, VAR>;   // the geometry, shared with launch_cfg
    constexpr bool TRANS = G::TRANS;
    constexpr bool LNF = FpEpiTraits<EPI>::LN;     // LayerNorm folded into this GEMM's epilogue (gemm_bf16.h)
    constexpr int NW = G::NW, TM = G::TM, TN = G::TN, TR = G::TR, TC = G::TC, STAGE = G::STAGE, IX = G::IX, IW = G::IW;

    // dynamic LDS: [GELU table, 16 KiB, table-GELU kernels only][K-tile buffer 0][K-tile buffer 1][epilogue slabs, 2 KiB per wave].
    // The table-GELU kernels keep no slab region: the 16-wave 256x256 kernel has no room for table + slabs (16 + 128 + 32 KiB),
    // and the 4-wave 128x128 kernel would drop from two resident workgroups per CU to one (88 KiB instead of 80).  Their slabs
    // live in the K-tile buffer the LAST K step consumed (free during the epilogue: the next tile's first stage is prefetched
    // into the other one), behind one extra barrier per tile.
    constexpr bool LUT = G::LUT;
    constexpr bool RELOC = G::RELOC;
    constexpr int TAB = G::TAB_BYTES;
    extern __shared__ __attribute__((aligned(1024))) char smem_raw[];
    char* const smem = smem_raw + TAB;                                     // K-tile buffers start here

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    LabPhases lab_ph;
    lab_phase(p, lab_ph, 0);
    // The epilogue's row-coalescing slabs are a STATIC shared array of their own: the K-tile buffers are filled by LDS-DMA, and for LDS
    // accesses that may alias a DMA destination hipcc waits until the copy has landed (vmcnt(0)) — carved out of the same dynamic
    // array, the slabs made the first ds_write of every epilogue wait for the next tile's prefetch.  Distinct LDS variables carry
    // no-alias scopes through the LDS lowering.  (The table-GELU kernels declare none: their slabs live in a K-tile buffer, and
    // their table must sit at LDS address 0.)
    char* epi_stage = nullptr;                                              // row-coalescing slab of the epilogue
    if constexpr (!RELOC) {
        __shared__ __attribute__((aligned(1024))) char slab_mem[G::SLAB_BYTES];
        epi_stage = slab_mem + wave * fp_gemm::EPI_STAGE_BYTES;
    }
    if constexpr (LUT) {
        // gelu_tab16's inline-asm gathers use table-relative byte offsets as absolute LDS addresses
        if ((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)smem_raw != 0u) __builtin_trap();
        for (int o = tid * 16; o < fp_gemm::GELU_TAB_BYTES; o += NW * 64 * 16)
            *(uint4*)(smem_raw + o) = *(const uint4*)((const char*)p.gelu_tab + o);
        __syncthreads();   // (the pipelined loop's raw s_barrier does not wait for LDS writes)
    }
    // slab of this wave when the slabs share a K-tile buffer (RELOC): `buf` = the buffer the tile's last K step read
    auto reloc_stage = [&](int buf) {
        __syncthreads();                                                    // every wave is done reading that buffer
        return smem + buf * STAGE + wave * fp_gemm::EPI_STAGE_BYTES;
    };

    // ---- XCD-aware tile order (bijective for any grid size).  PERSIST: a resident grid walks the tiles t = block,
    // block + grid, ...; the grid is a multiple of 8, so a workgroup's tiles keep its XCD under the same remap.
    constexpr bool PERSIST = fp_gemm::persist(VAR);
    constexpr bool PIPELINED = fp_gemm::pipelined(VAR);
    // SK: the balanced tier.  The grid's G workgroups share the launch's U = ntiles x (K / 64) units evenly: workgroup w
    // (in XCD-contiguous logical order) walks the units [u, u1) of the sequence "tile 0's K steps, tile 1's K steps, ..." — whole tiles
    // end in the ordinary epilogue, a tile whose K range it shares with its neighbours goes through fp32 partial tiles (below).
    constexpr bool SK = G::SK;
    static_assert(!SK || (PIPELINED && !PERSIST), "the balanced tier is built on the software-pipelined loop");
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    const int ntiles = tiles_m * tiles_n;
    int m0, n0;

    // ---- per-lane DMA source offsets ------------------------------------------------------------
    uint32_t offX[IX], offW[IW];
    auto set_tile = [&](int t, int& tm0, int& tn0) {
        int tile_m, tile_n;
        if constexpr (SK) fp_gemm_tile_of_id<4>(t, tiles_m, tiles_n, tile_m, tile_n);   // t is already a logical tile id
        else fp_gemm_tile<fp_gemm::strip_width(VAR)>(t, ntiles, tiles_m, tiles_n, tile_m, tile_n);
        tm0 = tile_m * BM;
        tn0 = tile_n * BN;
        // per-lane DMA source offsets (fp_gemm::dma_piece): the swizzle key goes into the SOURCE slot, rows past the edge re-read the last one
#pragma unroll
        for (int it = 0; it < IX; ++it) {
            const fp_gemm::DmaPiece d = fp_gemm::dma_piece<NW>(it, wave, lane, [](int row) { return TRANS ? key_perm<TM>(row) : key_plain(row); });
            offX[it] = fp_gemm::dma_src(fp_gemm::clamp_row(tm0, d.row, p.M), p.ldx, d.src_slot);
        }
#pragma unroll
        for (int it = 0; it < IW; ++it) {
            const fp_gemm::DmaPiece d = fp_gemm::dma_piece<NW>(it, wave, lane, [](int row) { return TRANS ? key_plain(row) : key_perm<TN>(row); });
            offW[it] = fp_gemm::dma_src(fp_gemm::clamp_row(tn0, d.row, p.N), p.ldw, d.src_slot);
        }
    };
    int tile = blockIdx.x;
    if constexpr (PERSIST) lab_stagger(p);
    fp_gemm::SkPart skp = {0, 0};
    int sk_w = 0, sk_u = 0, sk_u1 = 0;
    if constexpr (SK) {
        sk_w = fp_gemm_xcd_remap(blockIdx.x, gridDim.x);
        skp = fp_gemm::sk_part(ntiles * (p.K / BK), gridDim.x);   // the units [sk_u, sk_u1) of this workgroup
        sk_u = fp_gemm::sk_first(skp, sk_w);
        sk_u1 = fp_gemm::sk_end(skp, sk_w);
        if (sk_u >= sk_u1) return;                        // (the launcher never asks for more workgroups than units)
    } else {
        set_tile(tile, m0, n0);
    }
    const char* gX = (const char*)p.X;
    const char* gW = (const char*)p.W;

    // the LDS-DMA pieces of K tile `kt` into buffer `buf`: the X pieces, the W pieces or both (STAGE_X / STAGE_W / STAGE_BOTH)
    auto stage = [&](auto which, int buf, int kt) {
        constexpr int WHICH = decltype(which)::value;
        char* sb = smem + buf * STAGE;
        const size_t kb = (size_t)kt * ROWB;
        if constexpr ((WHICH & 1) != 0) {
#pragma unroll
            for (int it = 0; it < IX; ++it) glds16(gX + offX[it] + kb, sb + (it * NW + wave) * fp_gemm::DMA_BYTES);
        }
        if constexpr ((WHICH & 2) != 0) {
#pragma unroll
            for (int it = 0; it < IW; ++it) glds16(gW + offW[it] + kb, sb + G::W_OFF + (it * NW + wave) * fp_gemm::DMA_BYTES);
        }
    };

    // ---- per-lane fragment read offsets (bytes inside a stage, before the k-step XOR) -----------
    const int li = lane & 15, lg = lane >> 4;
    // R operand rows: permuted  rl = (li>>2)*4*TR + 4*f + (li&3)
    // C operand rows: plain     rl = 16*f + li
    // (stated again as fp_gemm::frag_map, which the host check reads; taking the values from it here changes the product kernels' schedule)
    int rowR0, keyR, rowC0, keyC;
    {
        const int tile_r = TRANS ? wm * (16 * TM) : wn * (16 * TN);
        const int tile_c = TRANS ? wn * (16 * TN) : wm * (16 * TM);
        rowR0 = tile_r + (li >> 2) * 4 * TR + (li & 3);  // + 4*f
        keyR = (((li >> 2) << 1) | ((li & 3) >> 1)) & 7;  // = key_perm(row) for every f
        rowC0 = tile_c + li;                              // + 16*f
        keyC = (li >> 1) & 7;                             // key_plain(16 f + li) = (li>>1)&7 | ((16f>>1)&7)=0
    }
    const int baseR = (TRANS ? 0 : BM * ROWB) + rowR0 * ROWB;
    const int baseC = (TRANS ? BM * ROWB : 0) + rowC0 * ROWB;

    // Accumulators start at the BIAS of their output feature instead of zero (normal epilogues): the 64 v_mov per wave and tile
    // are needed either way, and the epilogue loses its 64 v_add + ~40 unpack instructions per wave and tile (vector ALU work
    // cannot hide under the matrix pipe on gfx950).  Same-box A/B of two builds: qk +0.9 %, proj +2.0 %, fc2 +0.7 %, fc1 0.
    // Layout (fp_gemm::acc_r_index): acc[i][4 grp + j][r] is feature n0 + 64 (wn + grp) + 16 lg + 4 j + r for every row block i.
    f32x4_t acc[TC][TR];
    auto init_acc = [&](int m0_of_init, int tn0) {
        // The accumulators start at bias[n] (plain epilogues) or at b'[n] sigma[m] - mean[m] cs[n] (LN-folded ones, gemm_bf16.h) — formed
        // by ONE MFMA per accumulator block from 16-byte operand records (only the k-chunk of lanes lg == 0 is non-zero) with the inline
        // constant 0 as C: no accumulator zeroing, no unpacking, no vector-ALU arithmetic at the tile boundary, where every VALU
        // instruction is paid four times (the SIMD's four waves in lock-step, matrix pipe idle).  bias * 1.0 is exact.
        const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
        const bf16x8_t zfrag = __builtin_bit_cast(bf16x8_t, make_uint4(0u, 0u, 0u, 0u));
        // feature index / token index of fragment f of the R operand (permuted rows) and of the C operand (plain rows)
        const int rperm = fp_gemm::init_record_r(TR, 0, li);       // + 4 f = init_record_r(TR, f, li)
        bf16x8_t fr0[TR], fc0[TC];
        if constexpr (LNF) {
            const int featw = tn0 + wn * (16 * TN), tokw = m0_of_init + wm * (16 * TM);
#pragma unroll
            for (int f = 0; f < TR; ++f) {
                const int idx = TRANS ? min(tokw + rperm + 4 * f, p.M - 1) : min(featw + rperm + 4 * f, p.N - 1);
                fr0[f] = lg == 0 ? __builtin_bit_cast(bf16x8_t, (TRANS ? p.ln_mfrag : p.ln_cfrag)[idx]) : zfrag;
            }
#pragma unroll
            for (int f = 0; f < TC; ++f) {
                const int idx = TRANS ? min(featw + fp_gemm::init_record_c(f, li), p.N - 1) : min(tokw + fp_gemm::init_record_c(f, li), p.M - 1);
                fc0[f] = lg == 0 ? __builtin_bit_cast(bf16x8_t, (TRANS ? p.ln_cfrag : p.ln_mfrag)[idx]) : zfrag;
            }
        } else if constexpr (!TRANS) {
            const int featw = tn0 + wn * (16 * TN);
#pragma unroll
            for (int f = 0; f < TR; ++f) {
                const int idx = min(featw + rperm + 4 * f, p.N - 1);
                fr0[f] = lg == 0 ? __builtin_bit_cast(bf16x8_t, make_uint4((uint32_t)p.bias[idx], 0u, 0u, 0u)) : zfrag;
            }
            const bf16x8_t onef = lg == 0 ? __builtin_bit_cast(bf16x8_t, make_uint4(0x3f80u, 0u, 0u, 0u)) : zfrag;
#pragma unroll
            for (int f = 0; f < TC; ++f) fc0[f] = onef;
        }
        if constexpr (LNF || !TRANS) {
            if (LNF && lab_on(p, DBG_ZERO_INIT)) {
#pragma unroll
                for (int i = 0; i < TC; ++i)
#pragma unroll
                    for (int j = 0; j < TR; ++j) acc[i][j] = zero4;
            } else {
#pragma unroll
                for (int i = 0; i < TC; ++i)
#pragma unroll
                    for (int j = 0; j < TR; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr0[j], fc0[i], zero4, 0, 0, 0);
            }
        } else {   // transposed V store: measured slower with the bias in the accumulators (-3.7 %: spills), it adds it in the epilogue
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int j = 0; j < TR; ++j) acc[i][j] = zero4;
        }
    };
    // (an alias that has to stay: with init_acc called directly at the persistent walk's tile boundary hipcc orders the re-arming moves of all
    //  persistent product kernels differently — profiles/gemm_kernel_refactor.md §2)
    auto zero_acc = [&]() { init_acc(m0, n0); };
    const int nkt = p.K / BK;
    constexpr bool RING = G::RING;                            // K-tile ring of run-time depth (software-pipelined loop, 64x64 tier)
    int last_slot = (nkt - 1) & 1;                            // ring slot the last K step read (RELOC slabs live there)
    const int NS = RING ? p.ring : 2;                         // ring depth of the software-pipelined loop
    // K range of the current segment: the whole tile, or (SK) the part of a tile inside this workgroup's unit range
    int kt0 = 0, nk = nkt, sk_tile = 0;
    bool sk_more = false;
    do {
    if constexpr (SK) {
        sk_tile = sk_u / nkt;
        kt0 = sk_u - sk_tile * nkt;
        nk = min(nkt - kt0, sk_u1 - sk_u);
        if (sk_more) __syncthreads();                     // every wave is done with the previous segment's K tiles and slabs
        set_tile(sk_tile, m0, n0);
    }
    if constexpr (PIPELINED && !PERSIST) {
        // the software-pipelined loop's first NS K tiles go out before anything else: they stream in while the row statistics are
        // finalised and the accumulators initialised below
        for (int s = 0; s < NS; ++s)
            if (s < nk) stage(STAGE_BOTH, s, kt0 + s);
    }
    // small tiers, row statistics not finalised yet (FpGemmArgs::ln_part): this tile's rows are finalised here (gemm_bf16.h)
    if constexpr (LNF && !TRANS && !PERSIST) fp_gemm_finalize_tile_rows<BM, NW * 64>(p, m0, tid);
    if (SK && kt0 > 0) {
        // a later K slice of a shared tile: its partial sum starts from zero (the slice that holds K step 0 carries the bias / LayerNorm init)
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int j = 0; j < TR; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    } else {
        init_acc(m0, n0);
    }

    auto load_frags = [&](const char* sb, int kk, bf16x8_t (&fr)[TR], bf16x8_t (&fc)[TC]) {
        const int slotR = fp_gemm::slot_of(kk, lg, keyR);
        const int slotC = fp_gemm::slot_of(kk, lg, keyC);
#pragma unroll
        for (int f = 0; f < TR; ++f) fr[f] = *(const bf16x8_t*)(sb + baseR + f * 4 * ROWB + slotR);
#pragma unroll
        for (int f = 0; f < TC; ++f) fc[f] = *(const bf16x8_t*)(sb + baseC + f * 16 * ROWB + slotC);
    };
    auto mma_block = [&](const bf16x8_t (&fr)[TR], const bf16x8_t (&fc)[TC]) {
        if constexpr (fp_gemm::setprio(VAR)) __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int j = 0; j < TR; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr[j], fc[i], acc[i][j], 0, 0, 0);
        if constexpr (fp_gemm::setprio(VAR)) __builtin_amdgcn_s_setprio(0);
    };

    if constexpr (PERSIST) {
        // ---- persistent plain loop: the LDS buffers alternate on a step counter that runs across tiles; during the
        // LAST k-step of a tile the first stage of the workgroup's next tile is already being fetched, so address
        // set-up, pipeline fill and workgroup launch hide behind that step's MFMAs and the epilogue, and the
        // epilogue's stores drain while the next tile computes.
        static_assert(!PIPELINED, "persistent form uses the plain loop");
        const int tstride = gridDim.x;
        int g = 0;
        stage(STAGE_BOTH, 0, 0);
        for (;;) {
            const bool has_next = tile + tstride < ntiles;
            int m0n = 0, n0n = 0;
            for (int kt = 0; kt < nkt; ++kt, ++g) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                const bool more = kt + 1 < nkt;
                if (!more && has_next) set_tile(tile + tstride, m0n, n0n);
                const bool do_stage = more || has_next;
                const int nbuf = (g + 1) & 1, nk = more ? kt + 1 : 0;
                const char* sb = smem + (g & 1) * STAGE;
                if constexpr (!fp_gemm::split_issue(VAR)) {
                    if (do_stage) stage(STAGE_BOTH, nbuf, nk);
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        bf16x8_t fr[TR], fc[TC];
                        load_frags(sb, kk, fr, fc);
                        mma_block(fr, fc);
                    }
                } else {
                    // split DMA issue: the X pieces go out behind the first fragment reads (their LDS latency covers the issue),
                    // the W pieces behind the first MFMA block; MFMA blocks run at raised priority.  Measured in tools/gemm_lab.hip:
                    // +4 % at K = 4096 / 8192, neutral at K = 1024.
                    bf16x8_t fr[TR], fc[TC];
                    load_frags(sb, 0, fr, fc);
                    if (do_stage) stage(STAGE_X, nbuf, nk);
                    __builtin_amdgcn_s_setprio(1);
                    mma_block(fr, fc);
                    __builtin_amdgcn_s_setprio(0);
                    if (do_stage) stage(STAGE_W, nbuf, nk);
                    load_frags(sb, 1, fr, fc);
                    __builtin_amdgcn_s_setprio(1);
                    mma_block(fr, fc);
                    __builtin_amdgcn_s_setprio(0);
                }
            }
            if (lab_on(p, DBG_NO_EPILOGUE)) {   // the main loop without its epilogue — one store keeps the accumulators live
                if (acc[0][0][0] == 123456.789f) p.C[0] = 0;
            } else {
            if constexpr (RELOC) epi_stage = reloc_stage((g - 1) & 1);
            fp_gemm::epilogue<BM, BN, WM, WN, EPI, VAR, TC, TR>(p, acc, m0, n0, wm, wn, li, lg, epi_stage, smem_raw);
            }
            if (!has_next) return;
            tile += tstride;
            m0 = m0n;
            n0 = n0n;
            zero_acc();
        }
    } else if constexpr (!PIPELINED) {
        // ---- plain double-buffered loop: one barrier per K tile, fragments read right before use ----
        stage(STAGE_BOTH, 0, 0);
        for (int kt = 0; kt < nkt; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (kt + 1 < nkt) stage(STAGE_BOTH, (kt + 1) & 1, kt + 1);
            const char* sb = smem + (kt & 1) * STAGE;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                bf16x8_t fr[TR], fc[TC];
                load_frags(sb, kk, fr, fc);
                mma_block(fr, fc);
            }
        }
    } else {
        // ---- software-pipelined loop: fragments of k-step j+1 are read while k-step j's MFMAs run; the single
        // barrier of a tile sits at its SECOND k-step, where every wave has finished reading the tile, so the DMA
        // of tile t+2 is issued half a tile earlier and the next tile's first fragments are already in flight.
        // Ring of NS K-tile buffers, NS - 1 stages in flight: 2 for the 128x128 tier, 2 .. 8 (p.ring) for the 64x64 tier.  A launch of
        // the small tiers is a few workgroups per CU, each walking K alone: with two buffers every K step waits for one fresh memory
        // round trip (weights come from HBM: 0.7 us per step measured on a single-crop ViT-L forward), with a deeper ring the round
        // trips overlap.  The launcher takes the deepest ring that still keeps the whole grid resident (LDS per workgroup = NS x 16
        // KiB).  Same K order, same MFMA sequence: the bits do not depend on the depth.
        bf16x8_t frA[TR], fcA[TC], frB[TR], fcB[TC];
        constexpr int IPS = G::IPS;   // LDS-DMA instructions per stage and wave
        // (the first NS stages were issued at the top of the kernel) stage 0 has landed when at most the later stages' instructions are
        // outstanding; any vector-memory operation issued since (row statistics, init records) only makes this wait stricter
        if (RING) wait_stages<IPS, RING, false>(fp_gemm::ring_wait_first(nk, NS));
        else if (nk > 1) wait_imm<IPS, 1, false>();
        else wait_imm<IPS, 0, false>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        lab_phase(p, lab_ph, 1);
        // `settle`: pass a fragment set through an empty asm.  hipcc cannot count LDS reads across the loop back-edge
        // and would otherwise emit lgkmcnt(0) AFTER the prefetch reads are issued (waiting for the prefetch itself);
        // with the settle placed BEFORE the prefetch its wait covers only reads issued a whole MFMA block earlier.
        auto settle = [&](bf16x8_t (&fr)[TR], bf16x8_t (&fc)[TC]) {
#pragma unroll
            for (int f = 0; f < TR; ++f) asm volatile("" : "+v"(fr[f]));
#pragma unroll
            for (int f = 0; f < TC; ++f) asm volatile("" : "+v"(fc[f]));
        };
        constexpr bool SPREAD = fp_gemm::spread(VAR);
        // second half of a K step, interleaved: MFMA block B (TC x TR) with [DMA: the IPS pieces of stage `kt_dma` into slot `dslot`] and
        // the TR + TC fragment reads of the next step's first half (from `nsb`)
        auto spread_half = [&](auto dma_c, int dslot, int kt_dma, const char* nsb) {
            constexpr bool DMA = decltype(dma_c)::value;
            constexpr int NM = TC * TR, NP = IX + IW, NR = TR + TC;
            char* db = smem + dslot * STAGE;
            const size_t kb = (size_t)kt_dma * ROWB;
            const int slotR = fp_gemm::slot_of(0, lg, keyR), slotC = fp_gemm::slot_of(0, lg, keyC);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const int i = m / TR, j = m % TR;
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frB[j], fcB[i], acc[i][j], 0, 0, 0);
                if constexpr (DMA) {
                    if ((m * NP) / NM != ((m + 1) * NP) / NM) {          // piece q goes out behind MFMA m
                        const int q = (m * NP) / NM;
                        if (q < IX) glds16(gX + offX[q] + kb, db + (q * NW + wave) * 1024);
                        else glds16(gW + offW[q - IX] + kb, db + BM * ROWB + ((q - IX) * NW + wave) * 1024);
                    }
                }
                if ((m * NR) / NM != ((m + 1) * NR) / NM) {              // fragment read f behind MFMA m
                    const int f = (m * NR) / NM;
                    if (f < TR) frA[f] = *(const bf16x8_t*)(nsb + baseR + f * 4 * ROWB + slotR);
                    else fcA[f - TR] = *(const bf16x8_t*)(nsb + baseC + (f - TR) * 16 * ROWB + slotC);
                }
            }
            // pin the order: per MFMA at most one DMA piece and one fragment read behind it
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (DMA && (m * NP) / NM != ((m + 1) * NP) / NM) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                if ((m * NR) / NM != ((m + 1) * NR) / NM) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
        };
        load_frags(smem, 0, frA, fcA);
        int cur = 0;   // ring slot of stage kt
        for (int kt = 0; kt < nk; ++kt) {
            const char* sb = smem + cur * STAGE;
            const int nxt = cur + 1 == NS ? 0 : cur + 1;   // = fp_gemm::ring_next(cur, NS), spelled out: the call moves an instruction of two product kernels
            LabStamps stamps;
            lab_stamps_arm(p, stamps, kt);
            lab_stamp(stamps, 0);
            settle(frA, fcA);
            lab_stamp(stamps, 1);
            if (!lab_on(p, DBG_NO_READS)) load_frags(sb, 1, frB, fcB);
            if (!lab_on(p, DBG_NO_MFMA)) mma_block(frA, fcA);
            lab_stamp(stamps, 2);
            if (kt + 1 < nk) {
                // stage kt+1 must have landed; stages kt+2 .. kt+NS-1 may stay in flight (near the end of K fewer were issued: drain)
                wait_stages<IPS, RING, true>(fp_gemm::ring_wait_step(kt, nk, NS));
                lab_stamp(stamps, 3);
                if (!lab_on(p, DBG_NO_BARRIER)) __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                lab_stamp(stamps, 4);
                if constexpr (SPREAD) {
                    // SPREAD: the second half of the step as ONE interleaved stream — an LDS-DMA piece holds its issuing wave
                    // for ~50 clocks (profiles/r05_ab.md: 8 pieces in a row = 400 of a step's 1670 clocks with the matrix pipe idle), so
                    // each piece goes out behind a pair of MFMAs of block B, the next step's first fragment reads between them
                    settle(frB, fcB);
                    if (kt + NS < nk) spread_half(std::true_type{}, cur, kt0 + kt + NS, smem + nxt * STAGE);
                    else spread_half(std::false_type{}, cur, 0, smem + nxt * STAGE);
                    cur = nxt;
                    continue;
                }
                if (kt + NS < nk && !lab_on(p, DBG_NO_DMA)) stage(STAGE_BOTH, cur, kt0 + kt + NS);   // every wave is done reading stage kt: its slot takes stage kt + NS
                lab_stamp(stamps, 5);
                settle(frB, fcB);
                lab_stamp(stamps, 6);
                if (!lab_on(p, DBG_NO_READS)) load_frags(smem + nxt * STAGE, 0, frA, fcA);
            }
            if (!lab_on(p, DBG_NO_MFMA)) mma_block(frB, fcB);
            lab_stamp(stamps, 7);
            lab_stamps_write(p, stamps, tid);
            cur = nxt;
        }
        last_slot = (nk - 1) % NS;   // = fp_gemm::ring_last_slot(nk, NS)
        lab_phase(p, lab_ph, 2);
    }

    bool finish = true;                                   // this workgroup runs the tile's epilogue
    if constexpr (SK) {
        if (nk < nkt) {
            // ---- a K slice of a tile shared with neighbouring workgroups.  Every slice writes its fp32 partial tile (agent-coherent
            // stores: the workgroups sit on different XCDs, whose L2s are not coherent with each other) to one of its two scratch slots
            // and counts itself in; the LAST to arrive adds the slices IN K ORDER — slice 0 carries the bias / LayerNorm init — so the
            // sum does not depend on who that is, and runs the epilogue.  Nobody waits for anybody.
            typedef fp_gemm::u32x4_t u32x4;
            constexpr int TILE_F = BM * BN;                // floats per partial tile
            const int ut0 = sk_tile * nkt;
            const int w_first = fp_gemm::sk_wg_of(skp, ut0), nsl = fp_gemm::sk_wg_of(skp, ut0 + nkt - 1) - w_first + 1;
            const int voff = (wave * 64 + lane) * 16;      // fragment f of the lane sits at voff + f * NW * 1024
            {
                const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
                    (void*)(p.sk_ws + (size_t)(2 * sk_w + (kt0 > 0 ? 0 : 1)) * TILE_F), 0, TILE_F * 4, 0x00020000);
#pragma unroll
                for (int i = 0; i < TC; ++i)
#pragma unroll
                    for (int j = 0; j < TR; ++j)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][j]), rw, voff + (i * TR + j) * NW * 1024, 0, 16);   // sc1
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            int* const flag = (int*)(smem + NS * STAGE);   // the spare bytes behind the K-tile ring (Geo::SK_FLAG_BYTES)
            if (tid == 0) *flag = __hip_atomic_fetch_add(p.sk_cnt + sk_tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            finish = *flag == nsl - 1;
            if (finish) {
                if (tid == 0) __hip_atomic_store(p.sk_cnt + sk_tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
                for (int sl = 0; sl < nsl; ++sl) {
                    const int w = w_first + sl;
                    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(
                        (void*)(p.sk_ws + (size_t)(2 * w + (sl == 0 ? 1 : 0)) * TILE_F), 0, TILE_F * 4, 0x00020000);
#pragma unroll
                    for (int i = 0; i < TC; ++i)
#pragma unroll
                        for (int j = 0; j < TR; ++j) {
                            const f32x4_t v = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(rr, voff + (i * TR + j) * NW * 1024, 0, 16));
                            acc[i][j] = sl == 0 ? v : acc[i][j] + v;
                        }
                }
            }
        }
    }
    if (finish) {
        if constexpr (RELOC) epi_stage = reloc_stage(last_slot);
        fp_gemm::epilogue<BM, BN, WM, WN, EPI, VAR, TC, TR>(p, acc, m0, n0, wm, wn, li, lg, epi_stage, smem_raw);
    }
    lab_phases_write(p, lab_ph, tid);
    if constexpr (SK) {
        sk_u += nk;
        sk_more = sk_u < sk_u1;
    }
    } while (SK && sk_more);
}

// bf16(gelu_erf(x)) for the 8192 input patterns of the table window, evaluated with the device expression of the direct variant
__global__ void gelu_table_kernel(uint16_t* tab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= fp_gemm::GELU_TAB_ENTRIES) return;
    const float x = __uint_as_float(fp_gemm::gelu_tab_pattern(i) << 16);
    tab[i] = (uint16_t)(__float_as_uint(rbf(fp_gemm::gelu_erf(x))) >> 16);
}

__global__ void gelu_direct_kernel(const bf16_t* x, bf16_t* y, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (bf16_t)(__float_as_uint(rbf(fp_gemm::gelu_erf(__uint_as_float((uint32_t)x[i] << 16)))) >> 16);
}

// Launches ONE kernel: `grid` workgroups, `ring` K-tile buffers where the kernel has a ring of run-time depth.  Which kernel, how many
// workgroups and how deep a ring is the plan's business (gemm_plan.h); here the kernel's constants are held to the ones the plan budgets with.
template <int BM, int BN, int WM, int WN, int EPI, int VAR>
int launch_cfg(const FpGemmArgs& a, hipStream_t stream, int ring, int grid) {
    using G = fp_gemm::Geo<BM, BN, WM, WN, EPI, VAR>;   // (holds the kernel's constants to the ones gemm_plan.h budgets with)
    auto kern = gemm_bf16_kernel<BM, BN, WM, WN, EPI, VAR>;
    FP_DYN_LDS_ONCE(kern, G::dyn_lds(G::RING_MAX));      // dynamic part; the slabs are static (see the kernel)
    if constexpr (G::SK) {                               // balanced tier: `grid` workgroups share the (tile, K step) units
        const int tiles = cdiv(a.M, BM) * cdiv(a.N, BN);
        FP_REQUIRE(grid > 0 && grid <= tiles * (a.K / BK) && a.sk_ws && a.sk_cnt && tiles <= a.sk_cnt_n &&
                       (size_t)grid * 2 * BM * BN * 4 <= a.sk_ws_bytes, "gemm: balanced tier without scratch (grid %d, %d tiles)", grid, tiles);
    }
    FpGemmArgs ar = a;
    ar.ring = G::RING ? ring : 2;
    FP_REQUIRE(grid > 0 && ar.ring >= 2 && ar.ring <= G::RING_MAX, "gemm: plan outside the kernel's limits (grid %d, ring %d)", grid, ar.ring);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(G::NW * 64), G::dyn_lds(ar.ring), stream, ar);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

fp_plan::Shape shape_of(const FpGemmArgs& a, int epi);

#ifdef FP_LAB
// ---- LAB BUILD ONLY: the options the plan is made under, and launches of kernels the plan does not know
int lab_variant() {
    static int env_var = [] { const char* e = getenv("FP_GEMM_VARIANT"); return e ? atoi(e) : FP_GEMM_DEFAULT_VARIANT; }();
    return fp_opt_get(FP_OPT_GEMM_VARIANT, env_var);
}
// the gemm_variant bits that change the plan (A/B only) are fp_gemm::LabOpt; gemm_stream_mb = the streaming threshold in MiB (0 = always
// stream), gemm_ring = cap on the 64x64 tier's ring (up to 8)
fp_plan::Options lab_options() {
    using namespace fp_gemm;
    const int var = lab_variant();
    fp_plan::Options o;
    o.force_small = var & LO_FORCE_SMALL;
    o.never_split = var & LO_NEVER_SPLIT;
    o.keep_small = var & LO_KEEP_SMALL;
    o.tiny_unless_big = var & LO_TINY_UNLESS_BIG;
    o.asm_never = var & LO_ASM_NEVER;
    o.asm_always = var & LO_ASM_ALWAYS;
    o.asm_ln = true;
    o.asm_small = var & LO_ASM_SMALL;
    o.asm_small_filled = var & LO_ASM_SMALL_FILLED;
    o.asm_small_long_k = var & LO_ASM_SMALL_LONG_K;
    o.stream_bytes = (var & LO_NEVER_STREAM) ? 1L << 60 : (long)fp_opt_get(FP_OPT_GEMM_STREAM_MB, (int)(fp_plan::FP_GEMM_STREAM_BYTES >> 20)) << 20;
    o.ring_cap = fp_opt_get(FP_OPT_GEMM_RING, fp_plan::RING_CAP);
    return o;
}
// an alternative kernel for a tier the plan chose (sk_grid > 0: on the balanced tier's grid): its grid and ring by the plan's rules
template <int BM, int BN, int WM, int WN, int EPI, int VAR>
int launch_alt(const FpGemmArgs& a, hipStream_t stream, int sk_grid = 0) {
    const int n = fp_gemm_device_cus();
    long grid = fp_gemm::stream_k(VAR) ? sk_grid : (long)cdiv(a.M, BM) * cdiv(a.N, BN);
    const int ring = fp_plan::ring_depth(grid, a.K / BK, BM, BN, WM * WN, fp_gemm::lut(EPI, VAR), fp_plan::ncu_resident(n), lab_options().ring_cap);
    if (fp_gemm::persist(VAR)) grid = fp_plan::resident_grid(grid, fp_plan::ncu_persistent(n), fp_plan::LDS_BUDGET);
    return launch_cfg<BM, BN, WM, WN, EPI, VAR>(a, stream, ring, (int)grid);
}

// The lab's alternatives for the tier the plan chose, in one place: launches the alternative and returns its status, or LAB_NOT_HANDLED when
// no lab option applies to this tier and epilogue (the product kernel of launch_part then runs).  Option bits (fp_gemm::LabOpt) are mapped to
// kernel bits (fp_gemm::Variant) here and nowhere else.
constexpr int LAB_NOT_HANDLED = -12345;
template <int EPI>
int launch_lab(const FpGemmArgs& a, const fp_plan::Part& p, hipStream_t stream) {
    using namespace fp_gemm;
    constexpr bool TRANS = FpEpiTraits<EPI>::TRANS;
    constexpr bool PLAIN = EPI < FP_EPI_LN_BIAS;   // the plain epilogues have alternative kernels (A/B runs: gemm_variant & 7 = 0 the baseline, else 6)
    constexpr int WM8 = TRANS ? 2 : 4, WN8 = TRANS ? 4 : 2;   // the 128x128 tier on 8 waves
    constexpr int V6 = FP_GEMM_VAR_SMALL;
    const int var = lab_variant();
    const bool other_loop = PLAIN && var != FP_GEMM_DEFAULT_VARIANT, baseline = (var & LO_LOOP_MASK) == 0;
    if (p.tier < fp_plan::BIG_HIP) {
        // BALANCED TIER (round 5, measured and not shipped, profiles/r05_ab.md §1): G workgroups share the launch's (tile, K step) units
        // evenly (stream-K); a tile whose K range is spread over several workgroups is completed by the last of them to arrive, which adds
        // the fp32 partial tiles in K order.  Forms: gemm_sk = 2 / 3 / 4 -> 128x128 / 64x64 / 128x128-on-a-ring units, gemm_sk_grid = G.
        if constexpr (EPI != FP_EPI_PATCH) {
            const int f = fp_opt_get(FP_OPT_GEMM_SK, 0), g = fp_opt_get(FP_OPT_GEMM_SK_GRID, 0);
            if (f >= 2 && f <= 4 && a.sk_ws && a.sk_cnt && a.sk_mode != 1) {
                const int ncu = fp_plan::ncu_dispatch(fp_gemm_device_cus());
                const long units = (long)cdiv(a.M, f == 3 ? 64 : 128) * cdiv(a.N, f == 3 ? 64 : 128) * (a.K / BK);
                int sk_grid = (int)std::min<long>(units, g > 0 ? g : (f == 3 ? 4L : f == 4 ? 1L : 2L) * ncu);
                sk_grid = (int)std::min<long>(sk_grid, (long)(a.sk_ws_bytes / (f == 3 ? 2 * 64 * 64 * 4 : 2 * 128 * 128 * 4)));
                if (f == 2) return launch_alt<128, 128, 2, 2, EPI, FP_GEMM_VAR_SMALL | V_STREAM_K>(a, stream, sk_grid);
                if (f == 3) return launch_alt<64, 64, fp_plan::tiny_waves(EPI), 1, EPI, FP_GEMM_VAR_TINY | V_STREAM_K>(a, stream, sk_grid);
                return launch_alt<128, 128, 2, 2, EPI, FP_GEMM_VAR_SMALL | V_RING_STRIP16 | V_STREAM_K>(a, stream, sk_grid);
            }
        }
        // the hand-scheduled 128x128 kernel in place of both small tiers (Options::asm_small)
        if constexpr (!TRANS) {
            if (fp_plan::asm_small_used(shape_of(a, EPI), a.M, fp_plan::ncu_dispatch(fp_gemm_device_cus()), lab_options())) return fp_gemm_asm_small(a, EPI, stream);
        }
    }
    switch (p.tier) {
        case fp_plan::TINY64:
            if constexpr (PLAIN) {
                if (other_loop) return baseline ? launch_alt<64, 64, 1, 1, EPI, 0>(a, stream) : launch_alt<64, 64, 1, 1, EPI, V6>(a, stream);
            }
            if constexpr (!TRANS) {
                if (var & LO_TINY_TWO_BUFFERS) return launch_alt<64, 64, 2, 1, EPI, FP_GEMM_VAR_SMALL>(a, stream);
            }
            if (var & LO_SPREAD) return launch_alt<64, 64, fp_plan::tiny_waves(EPI), 1, EPI, FP_GEMM_VAR_TINY | V_SPREAD>(a, stream);
            break;
        case fp_plan::SMALL128:
            if constexpr (PLAIN) {
                if (other_loop) return baseline ? launch_alt<128, 128, 2, 2, EPI, 0>(a, stream) : launch_alt<128, 128, 2, 2, EPI, V6>(a, stream);
            }
            if (var & LO_SPREAD)
                return (var & LO_SMALL_8WAVE) ? launch_alt<128, 128, WM8, WN8, EPI, FP_GEMM_VAR_SMALL | V_SPREAD>(a, stream)
                                              : launch_alt<128, 128, 2, 2, EPI, FP_GEMM_VAR_SMALL | V_SPREAD>(a, stream);
            if (var & LO_SMALL_8WAVE) return launch_alt<128, 128, WM8, WN8, EPI, FP_GEMM_VAR_SMALL>(a, stream);
            break;
        case fp_plan::BIG_ASM:
            if constexpr (!TRANS) {
                if (var & LO_ASM_8WAVE) return fp_gemm_asm(a, EPI, 8, stream);   // the 8-wave geometry
            }
            break;
        case fp_plan::BIG_HIP:
        case fp_plan::BIG_HIP_STREAM:
            if constexpr (!TRANS) {
                if ((var & LO_ASM_8WAVE) && fp_plan::asm_supported(shape_of(a, EPI), lab_options())) return fp_gemm_asm(a, EPI, 8, stream);
            }
            if constexpr (PLAIN) {
                if (other_loop) {
                    constexpr int T = V_TABLE_GELU;
                    if (var & V_WAVES16) {   // 16-wave workgroup (4 waves/SIMD), 64x64 per wave
                        switch (var & (V_PERSIST | V_STREAM_IO)) {
                            case V_PERSIST: return launch_alt<256, 256, 4, 4, EPI, T | V_PERSIST>(a, stream);
                            case V_STREAM_IO: return launch_alt<256, 256, 4, 4, EPI, T | V_STREAM_IO>(a, stream);
                            case V_PERSIST | V_STREAM_IO:
                                if ((var & V_SPLIT_ISSUE) && (var & V_STRIP8)) return launch_alt<256, 256, 4, 4, EPI, FP_GEMM_VAR_BIG | V_STRIP8>(a, stream);
                                if ((var & V_SPLIT_ISSUE) && (var & V_RING_STRIP16)) return launch_alt<256, 256, 4, 4, EPI, FP_GEMM_VAR_BIG | V_RING_STRIP16>(a, stream);   // whole-N sweep of fc1 (round 6)
                                return (var & V_SPLIT_ISSUE) ? launch_alt<256, 256, 4, 4, EPI, FP_GEMM_VAR_BIG>(a, stream)
                                                             : launch_alt<256, 256, 4, 4, EPI, T | V_PERSIST | V_STREAM_IO>(a, stream);
                            default: return launch_alt<256, 256, 4, 4, EPI, T>(a, stream);
                        }
                    }
                    // measured on MI355X (profiles/): 6 is the fastest; 0 is kept as the plain baseline for A/B runs
                    return baseline ? launch_alt<256, 256, 2, 4, EPI, 0>(a, stream) : launch_alt<256, 256, 2, 4, EPI, V6>(a, stream);
                }
            }
            break;
    }
    return LAB_NOT_HANDLED;
}
#endif

fp_plan::Shape shape_of(const FpGemmArgs& a, int epi) { return {a.M, a.N, a.K, epi, a.ldx, a.ldw, a.ln_part != nullptr, a.no_split != 0}; }

// The arguments of one part of a launch, rows [p.row0, p.row0 + p.rows): the one place a row offset is applied
FpGemmArgs part_args(const FpGemmArgs& a, const fp_plan::Part& p) {
    FpGemmArgs b = a;
    const size_t r = (size_t)p.row0;
    b.M = p.rows;
    if (p.rows < a.M) b.no_split = 1;          // a part of a split is never split again
    if (b.stat_ld == 0) b.stat_ld = a.M;       // stat_part keeps the whole problem's row stride
    b.X = a.X + r * a.ldx;
    b.C = a.C + r * a.ldc;
    if (a.resid) b.resid = a.resid + r * a.ldr;
    if (a.ln_mfrag) b.ln_mfrag = a.ln_mfrag + r;
    if (a.ln_rstd) b.ln_rstd = a.ln_rstd + r;
    if (a.ln_part) b.ln_part = a.ln_part + r;
    if (a.stat_part) b.stat_part = a.stat_part + r;
    return b;
}

// One part of the plan on the tier it names: one kernel per (epilogue, tile tier).  The lab build asks launch_lab first.
template <int EPI>
int launch_part(const FpGemmArgs& a, const fp_plan::Part& p, hipStream_t stream) {
    constexpr bool TRANS = FpEpiTraits<EPI>::TRANS;
    const bool big = p.tier >= fp_plan::BIG_HIP;
    // (fuses_ln_part shares BIG_MIN_TILES: a launch that still carries partial sums was promised the small tiers, which finalise them in
    //  their prologue — the 256x256 kernels would read stale records)
    FP_REQUIRE(!(big && a.ln_part), "gemm: partial row statistics on the big tier (M=%d N=%d)", a.M, a.N);
#ifdef FP_LAB
    if (const int rc = launch_lab<EPI>(a, p, stream); rc != LAB_NOT_HANDLED) return rc;
#endif
    switch (p.tier) {
        case fp_plan::TINY64: return launch_cfg<64, 64, fp_plan::tiny_waves(EPI), 1, EPI, FP_GEMM_VAR_TINY>(a, stream, p.ring, p.grid);
        case fp_plan::SMALL128: return launch_cfg<128, 128, 2, 2, EPI, FP_GEMM_VAR_SMALL>(a, stream, p.ring, p.grid);
        case fp_plan::BIG_ASM:
            if constexpr (!TRANS) return fp_gemm_asm(a, EPI, 4, stream);
            break;
        case fp_plan::BIG_HIP:
        case fp_plan::BIG_HIP_STREAM:
            // an output above the streaming threshold is stored non-temporally (gemm_plan.h: streaming policy)
            return p.tier == fp_plan::BIG_HIP ? launch_cfg<256, 256, 4, 4, EPI, FP_GEMM_VAR_BIG & ~fp_gemm::V_STREAM_IO>(a, stream, p.ring, p.grid)
                                              : launch_cfg<256, 256, 4, 4, EPI, FP_GEMM_VAR_BIG>(a, stream, p.ring, p.grid);
    }
    fp_set_error("gemm: tier %d has no kernel for epilogue %d", (int)p.tier, EPI);
    return FP_ERR_INVALID;
}

int launch_epi(const FpGemmArgs& a, int epi, const fp_plan::Part& p, hipStream_t stream) {
    switch (epi) {
        case FP_EPI_BIAS: return launch_part<FP_EPI_BIAS>(a, p, stream);
        case FP_EPI_BIAS_GELU: return launch_part<FP_EPI_BIAS_GELU>(a, p, stream);
        case FP_EPI_BIAS_LS_RES: return launch_part<FP_EPI_BIAS_LS_RES>(a, p, stream);
        case FP_EPI_PATCH: return launch_part<FP_EPI_PATCH>(a, p, stream);
        case FP_EPI_VT: return launch_part<FP_EPI_VT>(a, p, stream);
        case FP_EPI_LN_BIAS: return launch_part<FP_EPI_LN_BIAS>(a, p, stream);
        case FP_EPI_LN_GELU: return launch_part<FP_EPI_LN_GELU>(a, p, stream);
        case FP_EPI_LN_VT: return launch_part<FP_EPI_LN_VT>(a, p, stream);
        default: return launch_part<FP_EPI_LS_RES_STATS>(a, p, stream);
    }
}

}  // namespace

int fp_gemm_device_cus() {
    static const int n = [] { int dev = 0, n = 256; (void)hipGetDevice(&dev); (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev); return n; }();
    return n;
}

fp_plan::Plan fp_gemm_plan(const fp_plan::Shape& s) {
#ifdef FP_LAB
    return fp_plan::make_plan(s, fp_gemm_device_cus(), lab_options());
#else
    return fp_plan::make_plan(s, fp_gemm_device_cus());
#endif
}

// Per-device GELU table (16 KiB), built on first use; fp_ctx_create calls this so that no launch path ever allocates.
int fp_gemm_gelu_table(const uint16_t** out) {
    static std::mutex mu;
    static uint16_t* tabs[64] = {};
    int dev = 0;
    FP_HIP(hipGetDevice(&dev));
    FP_REQUIRE(dev >= 0 && dev < 64, "gemm: device index %d out of range", dev);
    std::lock_guard<std::mutex> lk(mu);
    if (!tabs[dev]) {
        uint16_t* t = nullptr;
        FP_HIP(hipMalloc((void**)&t, fp_gemm::GELU_TAB_BYTES));
        hipLaunchKernelGGL(gelu_table_kernel, dim3(fp_gemm::GELU_TAB_ENTRIES / 256), dim3(256), 0, 0, t);
        FP_LAUNCH_CHECK();
        FP_HIP(hipDeviceSynchronize());
        tabs[dev] = t;
    }
    if (out) *out = tabs[dev];
    return FP_OK;
}

int fp_gemm_bf16(const FpGemmArgs& a_in, int epi, hipStream_t stream) {
    FpGemmArgs a = a_in;
#ifdef FP_LAB
    static const int dbg_env = [] { const char* e = getenv("FP_GEMM_DBG"); return e ? atoi(e) : 0; }();
    a.dbg = fp_opt_get(FP_OPT_GEMM_DBG, dbg_env);
#endif
    if (epi == FP_EPI_BIAS_GELU || epi == FP_EPI_LN_GELU) {
        const int rc = fp_gemm_gelu_table(&a.gelu_tab);
        if (rc != FP_OK) return rc;
    }
    FP_REQUIRE(a.M > 0 && a.N > 0 && a.K > 0, "gemm: empty problem M=%d N=%d K=%d", a.M, a.N, a.K);
    FP_REQUIRE(a.K % BK == 0, "gemm: K=%d must be a multiple of %d", a.K, BK);
    FP_REQUIRE(a.N % 16 == 0, "gemm: N=%d must be a multiple of 16", a.N);
    FP_REQUIRE(((size_t)a.M * a.ldx * 2) < 0xffffffffull && ((size_t)a.N * a.ldw * 2) < 0xffffffffull,
               "gemm: operand larger than 4 GiB (M=%d ldx=%d)", a.M, a.ldx);
    FP_REQUIRE((a.ldx % 8) == 0 && (a.ldw % 8) == 0 && (a.ldc % 8) == 0, "gemm: leading dims must be multiples of 8");
    switch (epi) {
        case FP_EPI_BIAS:
        case FP_EPI_BIAS_GELU: break;
        case FP_EPI_BIAS_LS_RES: FP_REQUIRE(a.gamma && a.resid, "gemm: LS_RES epilogue needs gamma and resid"); break;
        case FP_EPI_PATCH: FP_REQUIRE(a.pos && a.P > 0 && a.npad > 0, "gemm: PATCH epilogue needs pos/P/npad"); break;
        case FP_EPI_LN_BIAS:
        case FP_EPI_LN_GELU:
            FP_REQUIRE(a.ln_mfrag && a.ln_rstd && a.ln_cfrag && a.N % 64 == 0 && a.M >= 16,
                       "gemm: LN-folded epilogue needs ln_mfrag, ln_rstd, ln_cfrag, N %% 64 == 0 and M >= 16 (M=%d N=%d)", a.M, a.N);
            break;
        case FP_EPI_LN_VT:
            FP_REQUIRE(a.ln_mfrag && a.ln_rstd && a.ln_cfrag, "gemm: LN-folded epilogue needs ln_mfrag, ln_rstd and ln_cfrag");
            [[fallthrough]];
        case FP_EPI_VT:
            FP_REQUIRE(a.npad % 16 == 0 && a.M % 16 == 0 && a.heads > 0 && a.N == a.heads * 64,
                       "gemm: VT epilogue needs npad%%16==0, M%%16==0, N==heads*64");
            break;
        case FP_EPI_LS_RES_STATS:
            FP_REQUIRE(a.gamma && a.resid && a.stat_part && a.N % 64 == 0, "gemm: LS_RES_STATS epilogue needs gamma, resid, stat_part, N %% 64 == 0");
            break;
        default: fp_set_error("gemm: unknown epilogue %d", epi); return FP_ERR_INVALID;
    }
    // plan, then launch: who finalises the row statistics, then each part on its tier
    const fp_plan::Plan plan = fp_gemm_plan(shape_of(a, epi));
    if (plan.finalize_first) {
        FP_REQUIRE(a.ln_part_nb > 0 && a.ln_part_ld >= a.M, "gemm: ln_part needs ln_part_nb and ln_part_ld");
        const int rc = fp_stats_finalize(a.ln_part, a.ln_mfrag, a.ln_rstd, a.M, a.ln_part_nb * 64, a.ln_eps, stream, a.ln_part_ld);
        if (rc != FP_OK) return rc;
        a.ln_part = nullptr;
    }
    for (int i = 0; i < plan.nparts; ++i) {
        const int rc = launch_epi(part_args(a, plan.part[i]), epi, plan.part[i], stream);
        if (rc != FP_OK) return rc;
    }
    return FP_OK;
}

int fp_gemm_gelu_direct(const bf16_t* x, bf16_t* y, size_t n, hipStream_t stream) {
    if (n == 0) return FP_OK;
    hipLaunchKernelGGL(gelu_direct_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, y, n);
    FP_LAUNCH_CHECK();
    return FP_OK;
}

const char* fp_gemm_kernel_name(int epi) {
    (void)epi;
    return "gemm_bf16_kernel";
}
