// v3d_gemm: multi-tap bf16 MFMA contraction for gfx950 (see include/v3d_hip.h for the op contract).
//
// One kernel family covers nn.Linear / 1x1 conv (1 tap), Conv2d 3x3 incl. stride-2 and fused nearest-2x upsample
// (9 taps, implicit GEMM over channels-last pixels) and the (3,1,1) temporal conv (3 taps along the frame stride).
// v_mfma_f32_16x16x32_bf16 with the WEIGHT fragment as the A operand, so each lane ends up with 4 consecutive output
// channels of one pixel (8-byte bf16 stores, float4 bias loads).
//
// The main loops (v1, v2, v3, v6 here, the LDS-haloed family in conv.hip) share the tap / row addressing (RowInfo) and the fused epilogue of
// gemm_common.h; which one a call gets is decided by plan_gemm below - the table there lists every kernel, its tile and when it is chosen.
//   v3 / v6: persistent blocks, buffer-load LDS-DMA ring across tile boundaries, two wave groups per SIMD offset by half a step around ONE
//      barrier per 32 k - see the block comment at gemm_kernel_v3.
//   v2: one tile per block, 2-3 blocks per CU; HBM/L2 -> LDS by global_load_lds_dwordx4 into an NS-deep ring of BK = 32 / 64 stages, counted
//      s_waitcnt vmcnt(N) + one raw s_barrier per stage (never vmcnt(0) inside the loop); conv zero padding / M, N tails read a 64 KiB zero page.
//   v1: register-staged double buffer with bounds-checked buffer loads.
// LDS rows are 64 B (128 B for BK = 64); the 16-byte chunk position of a row is XOR-swizzled on the per-lane SOURCE address (the
// LDS-DMA destination is lane-linear) so every ds_read_b128 lane group hits 16 distinct 16-byte slots.
#include <stdlib.h>

#include <map>
#include <mutex>
#include <vector>
#include <type_traits>

#include "gemm_common.h"

// Tile walk and stage order (same-box A/B, profiles/r02b_gemm_ab.txt):
//   tile walk (V3dGemmParams::group_m, tile_coords): groups of 8 tile rows for >= 96 tile rows, else 4; v6 walks row-major.  Measured (TF/s,
//     row-major -> 4 -> 8): GEGLU projection N = 10240: 824 -> 877 -> 861, N = 5120: 714 -> 703 -> 737; temporal qkv N = 3840: 674 -> 738 -> 726;
//     the feed-forward out-projections +3 %; convolutions (N <= 5 tile columns) +-2 %.
//   stage order: (tap outer, k inner).  (k outer, tap inner) removes the 7-19x L2-miss re-reads of the K >= 640 convolutions but recomputes the
//     per-lane row offsets every 32-k step: 25-30 % SLOWER on every convolution (1044 -> 769 TF/s at 1920 -> 640) - the loaders have no VALU to
//     spare, the re-reads come from the Infinity Cache and are not what bounds these launches.

namespace {

// 64 KiB of zeros: an invalid (padding / tail) lane of the LDS-DMA points here and can still be advanced by k0 like a
// real row pointer (K * 2 bytes <= 64 KiB is checked on the host), so the main loop has no per-step selects.
__device__ __attribute__((aligned(256))) unsigned int g_zero_page[16384] = {0};

// =====================================================================================================================
// v2: LDS-DMA ring pipeline
// =====================================================================================================================
// A stage holds KS k-slices of 32: LDS rows of 64 B (KS=1) or 128 B (KS=2).
// Chunk-position swizzle per 4-row block b = (row >> 2) & 3: {0, 2, 3, 1}.  With 64-byte rows the 256-byte LDS bank row
// holds 4 rows x 4 chunks; the 16-lane groups of ds_read_b128 ({0-3,12-15,20-27}, {4-11,16-19,28-31}, ...) read rows
// {0-3,12-15} at chunk c and rows {4-11} at chunk c^1: positions {f0, f3, 1^f1, 1^f2} and {f1, f2, 1^f0, 1^f3} (and the
// same XOR 2 for the upper half-wave) are all distinct for f = {0,2,3,1} -> 16 distinct slots per group, no conflicts.
// With 128-byte rows (2 rows per bank row, 8 chunk positions) the same argument gives f(row) = (row >> 1) & 7.
template <int KS>
__device__ __forceinline__ int swz_row(int row) {
    if (KS == 1) return (0x78 >> (((row >> 2) & 3) * 2)) & 3;
    return (row >> 1) & 7;
}

template <int BM, int BN, int WGM, int WGN, int NS, int KS, int MODE, bool GEGLU>
__global__ __launch_bounds__(64 * WGM * WGN, (64 * WGM * WGN) == 256 ? 2 : 1) void gemm_kernel_v2(GP p) {
    constexpr int BK2 = 32 * KS;             // k extent of one stage
    constexpr int ROWB = BK2 * 2;            // bytes per LDS row
    constexpr int RPP = 1024 / ROWB;         // rows per 1-KiB piece (one wave-wide LDS-DMA): 16 or 8
    constexpr int CPR = ROWB / 16;           // 16-byte chunks per row: 4 or 8
    constexpr int NW = WGM * WGN;            // waves per block
    constexpr int WM = BM / WGM;             // wave tile rows (pixels)
    constexpr int WN = BN / WGN;             // wave tile cols (out channels)
    constexpr int MF = WM / 16, NF = WN / 16;
    constexpr int APW = BM / RPP / NW;       // A pieces per wave per stage
    constexpr int BPW = BN / RPP / NW;
    static_assert(APW >= 1 && BPW >= 1 && APW * NW * RPP == BM && BPW * NW * RPP == BN, "tile / wave-count mismatch");
    constexpr int PIECES = APW + BPW;
    constexpr int STAGE_BYTES = (BM + BN) * ROWB;
    static_assert(PIECES * (NS - 2) < 64, "vmcnt range");
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NS * STAGE_BYTES];   // the ONLY __shared__ object

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;

    const int bid = xcd_remap(blockIdx.x, p.mt * p.nt);
    int tile_m, tile_n;
    tile_coords(p, bid, tile_m, tile_n);
    const long long m0 = (long long)tile_m * BM;
    const long long n0 = (long long)tile_n * BN;
    const long long z = blockIdx.y;                       // batch index, or split index of a split-K launch (sA = sW = 0 then)
    const bf16_t* __restrict__ A = p.A + z * p.sA;
    const bf16_t* __restrict__ W = p.W + z * p.sW;
    const bf16_t* zero = reinterpret_cast<const bf16_t*>(g_zero_page);

    // ---- LDS-DMA source addressing: lane l of a piece covers row (l / CPR), LDS chunk position (l % CPR) of that row;
    //      the position holds logical k-chunk pos ^ swz(row)  ->  this lane loads that logical chunk.  The swizzle of a
    //      row only depends on its index modulo 16, and every piece starts at a multiple of RPP rows.
    const int prow = lane / CPR;
    int kchunk_a[APW], kchunk_b[BPW];
#pragma unroll
    for (int i = 0; i < APW; ++i) kchunk_a[i] = (lane % CPR) ^ swz_row<KS>((wave + NW * i) * RPP + prow);
#pragma unroll
    for (int i = 0; i < BPW; ++i) kchunk_b[i] = (lane % CPR) ^ swz_row<KS>((wave + NW * i) * RPP + prow);
    RowInfo<MODE> ri[APW];
#pragma unroll
    for (int i = 0; i < APW; ++i) ri[i].init(p, m0 + (wave + NW * i) * RPP + prow);
    const bf16_t* arow[APW];   // source row pointer (+ k-chunk) for the current tap; invalid rows point into the zero page
    const bf16_t* brow[BPW];
    auto set_tap = [&](int tap) {
#pragma unroll
        for (int i = 0; i < APW; ++i) {
            long long s;
            const bool ok = ri[i].tap(p, tap, s);
            arow[i] = (ok ? A + (s + p.a_row0) * p.lda : zero) + kchunk_a[i] * 8;
        }
#pragma unroll
        for (int i = 0; i < BPW; ++i) {
            const long long n = n0 + (wave + NW * i) * RPP + prow;
            brow[i] = ((n < p.N) ? W + ((long long)tap * p.N + n) * p.ldw : zero) + kchunk_b[i] * 8;
        }
    };
    const int ksteps = (int)(p.K / BK2);                 // host guarantees K % BK2 == 0 for this kernel
    // split-K: this block contracts the flat (tap, k) step range [s0, s1) only
    const int total_steps = ksteps * ntaps<MODE>();
    const int s0 = p.split_n > 1 ? (int)((long long)total_steps * blockIdx.y / p.split_n) : 0;
    const int s1 = p.split_n > 1 ? (int)((long long)total_steps * (blockIdx.y + 1) / p.split_n) : total_steps;
    const int nsteps = s1 - s0;
    int ld_tap = s0 / ksteps;
    int ld_k0 = (s0 - ld_tap * ksteps) * BK2;
    set_tap(ld_tap);
    // steps issued past the end of the contraction (ring tail) re-read valid rows of the last tap: harmless dummies that
    // keep the per-wave DMA count per stage constant for the counted vmcnt waits
    auto issue = [&](int stage) {
        unsigned char* sbase = lds + stage * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < APW; ++i)
            __builtin_amdgcn_global_load_lds((const void*)(arow[i] + ld_k0), (__attribute__((address_space(3))) void*)(sbase + (wave + NW * i) * 1024), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < BPW; ++i)
            __builtin_amdgcn_global_load_lds((const void*)(brow[i] + ld_k0), (__attribute__((address_space(3))) void*)(sbase + BM * ROWB + (wave + NW * i) * 1024), 16, 0, 0);
        ld_k0 += BK2;
        if (ld_k0 >= p.K) {
            ld_k0 = 0;
            if (ntaps<MODE>() > 1 && ++ld_tap < ntaps<MODE>()) set_tap(ld_tap);
        }
    };

    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // fragment read offsets: row (lane & 15) of a 16-row fragment, logical chunk kk*4 + (lane >> 4), stored at chunk ^ swz
    int frag_off[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) frag_off[kk] = (lane & 15) * ROWB + (((kk * 4 + (lane >> 4)) ^ swz_row<KS>(lane & 15)) * 16);
    const int a_base = wm * WM * ROWB;
    const int b_base = BM * ROWB + wn * WN * ROWB;

#pragma unroll
    for (int s = 0; s < NS - 1; ++s) issue(s);

    // main-loop waves outrank co-resident blocks that are in their (VALU-dense) epilogue: without it the two do not overlap -
    // time(K) = time(epilogue only) + time(main loop only) on the GEGLU projections (tools/gemm_floor.py)
    __builtin_amdgcn_s_setprio(2);
    for (int t = 0; t < nsteps; ++t) {
        // this wave's pieces of stage t have landed when at most PIECES*(NS-2) newer DMA ops are outstanding
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PIECES * (NS - 2)) : "memory");
        __builtin_amdgcn_s_barrier();   // everyone's pieces landed; everyone finished reading stage (t-1) % NS
        asm volatile("" ::: "memory");
        issue((t + NS - 1) % NS);       // refill the stage consumed in the previous iteration
        const unsigned char* sb = lds + (t % NS) * STAGE_BYTES;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            bf16x8 xf[MF], wf[NF];
#pragma unroll
            for (int i = 0; i < MF; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(sb + a_base + frag_off[kk] + i * 16 * ROWB);
#pragma unroll
            for (int j = 0; j < NF; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(sb + b_base + frag_off[kk] + j * 16 * ROWB);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
        }
    }
    __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // drain the (dummy) tail DMAs before the ring is reused / released
    __builtin_amdgcn_s_barrier();                      // every wave has finished reading the last stage
    asm volatile("" ::: "memory");
    constexpr int NFO_ = GEGLU ? NF / 2 : NF;
    constexpr int STAGE_REGION = MF * 16 * (NFO_ * 32 + 16);
    constexpr bool CAN_STAGE = NW * STAGE_REGION <= NS * STAGE_BYTES;   // else: direct MFMA-layout stores
    epilogue<MF, NF, GEGLU, CAN_STAGE>(p, acc, m0 + wm * WM, n0 + wn * WN, z, lane, lds + (CAN_STAGE ? wave * STAGE_REGION : 0));
}

// =====================================================================================================================
// v1: register-staged double buffer (buffer loads with hardware bounds checking)
// =====================================================================================================================
constexpr int BK = 64;
constexpr int LROW = BK + 8;  // padded LDS row (bf16 elements) = 144 B, keeps 16-B alignment

template <int BM, int BN, int MODE, bool GEGLU>
__global__ __launch_bounds__(256, 2) void gemm_kernel_v1(GP p) {
    constexpr int AI = BM / 32;
    constexpr int BI = BN / 32;
    constexpr int WM = BM / 2, WN = BN / 2;
    constexpr int MF = WM / 16, NF = WN / 16;
    __shared__ __attribute__((aligned(16))) bf16_t sA[2][BM * LROW];
    __shared__ __attribute__((aligned(16))) bf16_t sB[2][BN * LROW];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int bid = xcd_remap(blockIdx.x, p.mt * p.nt);
    int tile_m, tile_n;
    tile_coords(p, bid, tile_m, tile_n);
    const long long m0 = (long long)tile_m * BM;
    const long long n0 = (long long)tile_n * BN;
    const long long z = blockIdx.y;
    const bufrsrc_t rsA = make_rsrc(p.A + z * p.sA, p.a_bytes);
    const bufrsrc_t rsW = make_rsrc(p.W + z * p.sW, p.w_bytes);
    const int kc = tid & 7;
    const int r0 = tid >> 3;
    RowInfo<MODE> ri[AI];
#pragma unroll
    for (int i = 0; i < AI; ++i) ri[i].init(p, m0 + r0 + 32 * i);
    u32x4 ra[AI], rb[BI];
    unsigned aoff[AI], boff[BI];
    const int ksteps = (int)((p.K + BK - 1) / BK);
    const int nsteps = ksteps * ntaps<MODE>();
    int ld_tap = 0, ld_k0 = 0;
    auto set_tap = [&](int tap) {
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            long long srow;
            const bool ok = ri[i].tap(p, tap, srow);
            aoff[i] = ok ? (unsigned)(((srow + p.a_row0) * p.lda + kc * 8) * 2) : kInvalid;
        }
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            const long long n = n0 + r0 + 32 * i;
            boff[i] = (n < p.N) ? (unsigned)((((long long)tap * p.N + n) * p.ldw + kc * 8) * 2) : kInvalid;
        }
    };
    set_tap(0);
    auto gload = [&]() {
        const bool kok = (ld_k0 + kc * 8) < p.K;
        const unsigned kb = (unsigned)ld_k0 * 2u;
#pragma unroll
        for (int i = 0; i < AI; ++i) ra[i] = buf_load16(rsA, (kok && aoff[i] != kInvalid) ? aoff[i] + kb : kInvalid);
#pragma unroll
        for (int i = 0; i < BI; ++i) rb[i] = buf_load16(rsW, (kok && boff[i] != kInvalid) ? boff[i] + kb : kInvalid);
        ld_k0 += BK;
        if (ld_k0 >= p.K) {
            ld_k0 = 0;
            ++ld_tap;
            if (ntaps<MODE>() > 1 && ld_tap < ntaps<MODE>()) set_tap(ld_tap);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < AI; ++i) *reinterpret_cast<u32x4*>(&sA[buf][(r0 + 32 * i) * LROW + kc * 8]) = ra[i];
#pragma unroll
        for (int i = 0; i < BI; ++i) *reinterpret_cast<u32x4*>(&sB[buf][(r0 + 32 * i) * LROW + kc * 8]) = rb[i];
    };
    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    gload();
    lstore(0);
    __syncthreads();
    const int frow = lane & 15;
    const int fk = (lane >> 4) * 8;
    for (int step = 0; step < nsteps; ++step) {
        const int buf = step & 1;
        if (step + 1 < nsteps) gload();
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
            bf16x8 xf[MF], wf[NF];
#pragma unroll
            for (int i = 0; i < MF; ++i)
                xf[i] = *reinterpret_cast<const bf16x8*>(&sA[buf][(wm * WM + i * 16 + frow) * LROW + kk * 32 + fk]);
#pragma unroll
            for (int j = 0; j < NF; ++j)
                wf[j] = *reinterpret_cast<const bf16x8*>(&sB[buf][(wn * WN + j * 16 + frow) * LROW + kk * 32 + fk]);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
        }
        if (step + 1 < nsteps) lstore(buf ^ 1);
        __syncthreads();
    }
    epilogue<MF, NF, GEGLU, false>(p, acc, m0 + wm * WM, n0 + wn * WN, z, lane, nullptr);
}

// =====================================================================================================================
// v3: persistent 8-wave ping-pong pipeline on big tiles (256 x 256, or 192 x 320 for the N = 320 family)
// =====================================================================================================================
// Why: a 128 x 128 tile needs (128+128)*2 B of LDS fill per k for 2*128*128 flop = 64 B/clk/CU at the MFMA peak, which is
// the whole L1/TA fill rate of a CU -- the v2 kernels sit at ~43 % MFMA busy with both resident waves of a SIMD parked on
// vmcnt at the same time (profiles/r01_gemm_ablation.txt + PMC).  A 256 x 256 tile halves the fill per flop; it leaves one
// workgroup per CU, so the overlap that v2 got from independent co-resident blocks has to be built into the block:
//   * 8 waves = 2 groups of 4 (waves w and w+4 share a SIMD).  Every step of 32 k has two slots separated by s_barrier;
//     in a slot one group runs its 32 MFMAs from registers while the other group issues LDS-DMA for 3 stages ahead and
//     ds_reads its fragments of the next stage, then they swap (group 1 runs one slot behind group 0).
//   * persistent: a block walks tiles b, b+G, b+2G ... (XCD-aware order); the (tile, tap, k) stage sequence is flat, so
//     the ring keeps prefetching across tile boundaries and a group's epilogue overlaps the other group's MFMA slot.
//   * counted s_waitcnt vmcnt(8): two younger stages (4 DMA ops each per wave) may stay in flight; epilogue stores in
//     flight only make the count conservative (loads return in order among themselves).

template <int BM, int BN, int WGM, int WGN, int MODE, bool GEGLU, int EMF, int NS = 4, int SPAD = 16, bool GN = false>
__global__ __launch_bounds__(512, NS == 3 ? 4 : 2) void gemm_kernel_v3(GP p, int ntiles) {   // (HIP: 2nd arg = min waves per SIMD)
    // NS = 4: one block per CU (128 KiB ring).  NS = 3 with a 256 x 128 tile: 72 KiB ring + 8 KiB staging = 80 KiB -> TWO blocks per
    // CU (128 VGPRs per wave), so one block's VALU-bound epilogue (GEGLU) overlaps the other block's main loop.
    constexpr int ROWB = 64, NW = 8;
    static_assert(WGM * WGN == NW, "8 waves");
    constexpr int WM = BM / WGM, WN = BN / WGN;
    constexpr int MF = WM / 16, NF = WN / 16;
    static_assert(MF % EMF == 0, "epilogue chunking");
    constexpr int NPIECE = (BM + BN) / 16;          // 1-KiB pieces (16 rows x 64 B) per stage
    constexpr int PPW = NPIECE / NW;                // pieces per wave per stage
    static_assert(PPW * NW == NPIECE && PPW * 2 < 64, "tile / wave-count mismatch");
    constexpr int APIECES = BM / 16;
    constexpr int STAGE_BYTES = (BM + BN) * ROWB;
    constexpr int NFO = GEGLU ? NF / 2 : NF;
    constexpr int EPI_REGION = EMF * 16 * (NFO * 32 + SPAD);
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NS * STAGE_BYTES + NW * EPI_REGION];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int wm = wave / WGN, wn = wave % WGN;
    const bf16_t* __restrict__ A = p.A;
    const bf16_t* __restrict__ W = p.W;
    unsigned char* estage = lds + NS * STAGE_BYTES + wave * EPI_REGION;

    const int G = gridDim.x;
    const int my_tiles = (ntiles - (int)blockIdx.x + G - 1) / G;
    auto tile_origin = [&](int it, long long& m0, long long& n0) __attribute__((always_inline)) {
        const int id = xcd_remap((int)blockIdx.x + it * G, ntiles);
        int tm, tn;
        tile_coords(p, id, tm, tn);
        n0 = (long long)tn * BN;
        m0 = (long long)tm * BM;
    };

    // ---- loader state (runs up to 3 stages ahead of the consumer, across tile boundaries).  Raw buffer loads straight to
    //      LDS: per-lane byte offset (row, k-chunk) in a VGPR that only changes per tile / tap, the k position in an SGPR
    //      soffset -> no vector ALU work per step; padding rows / tails use an out-of-range offset (the load writes zeros).
    const bufrsrc_t rsA = make_rsrc(A, p.a_bytes);
    const bufrsrc_t rsW = make_rsrc(W, p.w_bytes);
    const int prow = lane >> 2;
    const unsigned kchunk_b = (unsigned)(((lane & 3) ^ swz_row<1>(prow)) * 16);   // every piece starts at a multiple of 16 rows
    RowInfo<MODE> ri[PPW];
    unsigned voff[PPW];
    long long ld_n0 = 0;
    int ld_it = 0, ld_tap = 0, ld_k0 = 0;
    auto set_tap = [&](int tap) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int q = wave + NW * i;
            if (q < APIECES) {
                long long s_;
                const bool ok = ri[i].tap(p, tap, s_);
                voff[i] = ok ? (unsigned)((s_ + p.a_row0) * p.lda * 2) + kchunk_b : kInvalid;
            } else {
                const long long n = ld_n0 + (q - APIECES) * 16 + prow;
                voff[i] = (n < p.N) ? (unsigned)(((long long)tap * p.N + n) * p.ldw * 2) + kchunk_b : kInvalid;
            }
        }
    };
    auto set_tile = [&](int it) __attribute__((always_inline)) {
        long long m0;
        tile_origin(it, m0, ld_n0);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int q = wave + NW * i;
            if (q < APIECES) ri[i].init(p, m0 + q * 16 + prow);
        }
        set_tap(0);
    };
    set_tile(0);
    auto issue_piece = [&](int stage, int i, int so) __attribute__((always_inline)) {
        const int q = wave + NW * i;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(q < APIECES ? rsA : rsW, (__attribute__((address_space(3))) void*)(lds + stage * STAGE_BYTES + q * 1024), 16, (int)voff[i], so, 0, 0);
    };
    auto issue_advance = [&]() __attribute__((always_inline)) {
        ld_k0 += 32;
        if (ld_k0 >= (int)p.K) {
            ld_k0 = 0;
            if (++ld_tap < ntaps<MODE>()) {
                set_tap(ld_tap);
            } else {
                ld_tap = 0;
                if (++ld_it < my_tiles) set_tile(ld_it);   // past the last tile: harmless re-reads keep the DMA count constant
                else if (ntaps<MODE>() > 1) set_tap(0);
            }
        }
    };
    auto issue = [&](int stage) __attribute__((always_inline)) {
        // the k offset is wave-uniform, but in the multi-tap modes the compiler takes it for lane-varying, keeps it in a vector register and
        // wraps EVERY LDS-DMA issue of the main loop into a readfirstlane "waterfall" loop (rounds 1-2 shipped the 3x3 and temporal
        // convolutions that way; tools/check_loop_scratch.py flags it now).  One explicit readfirstlane per step: conv3x3 launches -5...-9 %.
        const int so = __builtin_amdgcn_readfirstlane(ld_k0 * 2);
#pragma unroll
        for (int i = 0; i < PPW; ++i) issue_piece(stage, i, so);
        issue_advance();
    };

    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frag_off = (lane & 15) * ROWB + (((lane >> 4) ^ swz_row<1>(lane & 15)) * 16);
    const int a_base = wm * WM * ROWB;
    const int b_base = BM * ROWB + wn * WN * ROWB;
    bf16x8 xf[MF], wf[NF];

    const int nsteps = (int)(p.K / 32) * ntaps<MODE>();

#pragma unroll
    for (int st = 0; st < NS - 1; ++st) issue(st);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NS - 2)) : "memory");
    __builtin_amdgcn_s_barrier();   // B_0: stage 0 landed
    __builtin_amdgcn_sched_barrier(0);
    // One barrier B_{s+1} per step ("stage s+1 landed, stage s-... buffers reusable").  Group 0 passes it AFTER its MFMAs of
    // step s, group 1 BEFORE them: between two barriers group 0 runs {read s, MFMA s} while group 1 runs {MFMA s-1, read s},
    // so one group's LDS reads / DMA issue always face the other group's MFMAs on the same SIMD.
    int s = 0;        // flat step counter
    int rd = 0;       // ring slot of step s; the refill target (step s + NS - 1) is the slot before it
    for (int it = 0; it < my_tiles; ++it) {
        for (int kt = 0; kt < nsteps; ++kt, ++s) {
            {
                const unsigned char* sb = lds + rd * STAGE_BYTES;
#pragma unroll
                for (int i = 0; i < MF; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(sb + a_base + frag_off + i * 16 * ROWB);
#pragma unroll
                for (int j = 0; j < NF; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(sb + b_base + frag_off + j * 16 * ROWB);
            }
            // refill the ring 3 stages ahead (the buffer of step s-1: its last reader, group 1, finished before B_s) while the
            // fragment reads are in flight
            issue(rd == 0 ? NS - 1 : rd - 1);
            rd = (rd + 1 == NS) ? 0 : rd + 1;
            // group 1 must have its fragments in registers before it passes the barrier (the slot is refilled after it);
            // group 0 goes straight into its MFMAs and lets the compiler's counted lgkmcnt waits release them fragment by fragment
            if (grp == 1) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
            if (grp == 1) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NS - 2)) : "memory");   // own pieces of stage s+1 landed
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            if (grp == 0) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NS - 2)) : "memory");   // own pieces of stage s+1 landed
                __builtin_amdgcn_s_barrier();
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---------------- tile finished for this group: retire it while the other group keeps the MFMA pipe busy
        long long e_m0, e_n0;
        tile_origin(it, e_m0, e_n0);
        if constexpr (!GEGLU && EMF == 1 && SPAD == 16) {
            // hand-managed epilogue (gemm_common.h e4_*): asm loads one fragment ahead of their use, one wait per 16-row fragment.  The host only
            // launches these kernels when e4_ok holds (whole wave tiles inside or outside the output, aligned operands, bf16 output).
            const long long mw0 = e_m0 + wm * WM, nw0 = e_n0 + wn * WN;
            if (mw0 < p.M && nw0 < p.N) {
                int lane_e = lane;
                asm volatile("" : "+v"(lane_e));          // (keeps what the epilogue derives from the lane id out of the loop-invariant set: no spills)
                auto rowfn = [&](int f) __attribute__((always_inline)) -> long long { return mw0 + f * 16; };
                E4GnRun<WM, MF> run;
                if constexpr (GN) run.init(mw0, p.gn_rps);
                auto flushfn = [&](int f, long long, unsigned& slot, unsigned& sid) __attribute__((always_inline)) -> bool { return run.step(f, slot, sid); };
                e4_retire_tile<MF, NF, GN>(p, acc, nw0, lane_e, estage, rowfn, flushfn);
            }
        } else
        {
            const long long mw0 = e_m0 + wm * WM, nw0 = e_n0 + wn * WN;
            const bool inside = mw0 < p.M && nw0 < p.N;
            const bool res_pre = p.res1 && !p.out_fp32 && (p.ldr1 % 8 == 0) && (reinterpret_cast<uintptr_t>(p.res1) % 16 == 0) && inside;
            u32x4 r0 = {0u, 0u, 0u, 0u}, r1 = r0, r2 = r0;
            if (res_pre) {
                r0 = load_res_piece<0, EMF, NF, GEGLU>(p, mw0, nw0, lane);
                r1 = load_res_piece<1, EMF, NF, GEGLU>(p, mw0, nw0, lane);
                r2 = load_res_piece<2, EMF, NF, GEGLU>(p, mw0, nw0, lane);
            }
            float4 bv[NF];
#pragma unroll
            for (int j = 0; j < NF; ++j)
                bv[j] = (p.bias && inside) ? *reinterpret_cast<const float4*>(p.bias + (int)nw0 + (lane >> 4) * 4 + j * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
            GnAcc<GN ? NF : 1> gn;
            long long sid0 = 0;
            unsigned rem0 = 0;
            if constexpr (GN) {
                gn_zero(gn);
                sid0 = mw0 / p.gn_rps;
                rem0 = (unsigned)(mw0 - sid0 * p.gn_rps);
            }
            if (!GN || inside) v3_retire_chunks<0, MF / EMF, EMF, NF, GEGLU, SPAD, GN>(p, acc, mw0, nw0, lane, estage, r0, r1, r2, res_pre, bv, gn, sid0, rem0);
        }
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// =====================================================================================================================
// v6: persistent 4-wave blocks, TWO per CU, for the HBM-bound linears (K <= 640: to_out / proj_in / proj_out / skip of the 64 x 64 and 32 x 32 levels)
// =====================================================================================================================
// Why (round 6, tools/v3_timeline_k320.py -> profiles/r06_timeline_k320_*.txt): on M = 147456, N = K = 320 the v3 block spends 25 k cycles in the ten
// steps of a tile (8 k of them waiting for rows from HBM) and then 14 k (bias only) to 33 k (bias + vector + residual) cycles in the tile's epilogue,
// with NO load of the next tile issued meanwhile beyond the three ring stages - every CU of the chip alternates between a read phase and a
// (read +) write phase, each bound by the bytes one block keeps in flight, and the launch moves 3.4 TB/s.  The work of a CU has to be two
// independent streams whose phases overlap.  The wave groups of a v3 block cannot be that (one s_barrier per workgroup), so here the groups
// are BLOCKS: 256 threads, 192 x 160 tiles (wave tile 96 x 80 as v3's 192 x 320: same fragments, same hand-managed epilogue), a 3-stage
// ring of 22-KiB stages -> 79 KiB of LDS and 256 registers per wave: two blocks per CU, each with its own ring, barrier and tile sequence.
// While one block retires a tile the other runs its main loop: its LDS-DMA stream and the first block's residual loads / row stores share
// the memory system instead of taking turns.  The two N-halves of a row tile are consecutive tile ids (row-major walk) = blocks 8 apart on one
// XCD: the second reader of the 192 activation rows finds them in that XCD's L2.
// One wave per SIMD and block, so a wave runs {fragment reads, DMA issue, MFMAs, counted wait, barrier} in sequence and the co-resident block's
// wave fills the matrix pipe meanwhile - unsynchronised, which is fine for launches that are bound by HBM, not by the matrix pipe.
template <int BM, int BN, int NS, int MODE>
__global__ __launch_bounds__(256, 2) void gemm_kernel_v6(GP p, int ntiles) {
    constexpr int ROWB = 64, NW = 4, WGN = 2;
    constexpr int WM = BM / 2, WN = BN / WGN, MF = WM / 16, NF = WN / 16;
    static_assert(NF == 5 || NF == 4, "the hand-managed epilogue retires 80- or 64-channel wave tiles");
    constexpr int NPIECE = (BM + BN) / 16, PPW = (NPIECE + NW - 1) / NW, APIECES = BM / 16, ARI = (APIECES + NW - 1) / NW;
    static_assert(PPW * (NS - 2) < 64, "vmcnt range");
    constexpr int STAGE_BYTES = NPIECE * 1024;
    constexpr int DUMMY_OFF = NS * STAGE_BYTES, NDUMMY = PPW * NW - NPIECE;        // pieces past the stage keep every wave's DMA count per stage equal
    constexpr int EPI_OFF = DUMMY_OFF + NDUMMY * 1024, EPI_REGION = 16 * (NF * 32 + 16);
    __shared__ __attribute__((aligned(1024))) unsigned char lds[EPI_OFF + NW * EPI_REGION];      // the ONLY __shared__ object
    static_assert(sizeof(lds) <= 80 * 1024, "two blocks per CU");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    unsigned char* estage = lds + EPI_OFF + wave * EPI_REGION;
    const int G = gridDim.x;
    const int my_tiles = (ntiles - (int)blockIdx.x + G - 1) / G;
    auto tile_origin = [&](int it, long long& m0, long long& n0) __attribute__((always_inline)) {
        const int id = xcd_remap((int)blockIdx.x + it * G, ntiles);
        int tm, tn;
        tile_coords(p, id, tm, tn);
        n0 = (long long)tn * BN;
        m0 = (long long)tm * BM;
    };
    // ---- loader (as v3): piece q = wave + 4 i: q < APIECES activation rows, q < NPIECE weight rows, else a dummy into its own KiB
    const bufrsrc_t rsA = make_rsrc(p.A, p.a_bytes);
    const bufrsrc_t rsW = make_rsrc(p.W, p.w_bytes);
    const int prow = lane >> 2;
    const unsigned kchunk_b = (unsigned)(((lane & 3) ^ swz_row<1>(prow)) * 16);
    RowInfo<MODE> ri[ARI];
    unsigned voff[PPW];
    long long ld_n0 = 0;
    int ld_it = 0, ld_tap = 0, ld_k0 = 0;
    auto set_tap = [&](int tap) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int q = wave + NW * i;
            if (i < ARI && q < APIECES) {
                long long s_;
                const bool ok = ri[i < ARI ? i : 0].tap(p, tap, s_);
                voff[i] = ok ? (unsigned)((s_ + p.a_row0) * p.lda * 2) + kchunk_b : kInvalid;
            } else {
                const long long n = ld_n0 + (q - APIECES) * 16 + prow;
                voff[i] = (q < NPIECE && n < p.N) ? (unsigned)(((long long)tap * p.N + n) * p.ldw * 2) + kchunk_b : kInvalid;
            }
        }
    };
    auto set_tile = [&](int it) __attribute__((always_inline)) {
        long long m0;
        tile_origin(it, m0, ld_n0);
#pragma unroll
        for (int i = 0; i < ARI; ++i) {
            const int q = wave + NW * i;
            if (q < APIECES) ri[i].init(p, m0 + q * 16 + prow);
        }
        set_tap(0);
    };
    set_tile(0);
    auto issue = [&](int stage) __attribute__((always_inline)) {
        const int so = __builtin_amdgcn_readfirstlane(ld_k0 * 2);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int q = wave + NW * i;
            const int dst = q < NPIECE ? stage * STAGE_BYTES + q * 1024 : DUMMY_OFF + (q - NPIECE) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(q < APIECES ? rsA : rsW, (__attribute__((address_space(3))) void*)(lds + dst), 16, (int)voff[i], so, 0, 0);
        }
        ld_k0 += 32;
        if (ld_k0 >= (int)p.K) {
            ld_k0 = 0;
            if (++ld_tap < ntaps<MODE>()) {
                set_tap(ld_tap);
            } else {
                ld_tap = 0;
                if (++ld_it < my_tiles) set_tile(ld_it);      // past the last tile: harmless re-reads keep the DMA count constant
                else if (ntaps<MODE>() > 1) set_tap(0);
            }
        }
    };
    f32x4 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frag_off = (lane & 15) * ROWB + (((lane >> 4) ^ swz_row<1>(lane & 15)) * 16);
    const int a_base = wm * WM * ROWB;
    const int b_base = BM * ROWB + wn * WN * ROWB;
    bf16x8 xf[MF], wf[NF];
    const int nsteps = (int)(p.K / 32) * ntaps<MODE>();
#pragma unroll
    for (int st = 0; st < NS - 1; ++st) issue(st);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NS - 2)) : "memory");
    __builtin_amdgcn_s_barrier();   // stage 0 landed
    __builtin_amdgcn_sched_barrier(0);
    int rd = 0;       // ring slot of the current step; the refill target (step s + NS - 1) is the slot before it, whose readers passed the last barrier
    for (int it = 0; it < my_tiles; ++it) {
        for (int kt = 0; kt < nsteps; ++kt) {
            {
                const unsigned char* sb = lds + rd * STAGE_BYTES;
#pragma unroll
                for (int i = 0; i < MF; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(sb + a_base + frag_off + i * 16 * ROWB);
#pragma unroll
                for (int j = 0; j < NF; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(sb + b_base + frag_off + j * 16 * ROWB);
            }
            issue(rd == 0 ? NS - 1 : rd - 1);
            rd = (rd + 1 == NS) ? 0 : rd + 1;
            __builtin_amdgcn_s_setprio(1);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PPW * (NS - 2)) : "memory");   // own pieces of the next stage landed
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        long long e_m0, e_n0;
        tile_origin(it, e_m0, e_n0);
        const long long mw0 = e_m0 + wm * WM, nw0 = e_n0 + wn * WN;
        if (mw0 < p.M && nw0 < p.N) {
            int lane_e = lane;
            asm volatile("" : "+v"(lane_e));          // (keeps what the epilogue derives from the lane id out of the loop-invariant set: no spills)
            auto rowfn = [&](int f) __attribute__((always_inline)) -> long long { return mw0 + f * 16; };
            auto flushfn = [&](int, long long, unsigned&, unsigned&) __attribute__((always_inline)) -> bool { return false; };
            e4_retire_tile<MF, NF, false>(p, acc, nw0, lane_e, estage, rowfn, flushfn);
        }
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- split-K finalize: out = epilogue(sum over splits of ws) element-wise (4 consecutive channels per thread) ---------------------
__global__ __launch_bounds__(256) void splitk_finalize_kernel(GP p) {
    const long long n4 = p.N / 4;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.M * n4) return;
    const long long m = idx / n4;
    const int n = (int)(idx - m * n4) * 4;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sp = 0; sp < p.split_n; ++sp) {
        const float4 w = *reinterpret_cast<const float4*>(p.ws + ((long long)sp * p.M + m) * p.N + n);
        a.x += w.x; a.y += w.y; a.z += w.z; a.w += w.w;
    }
    if (p.bias) {
        const float4 b = *reinterpret_cast<const float4*>(p.bias + n);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    if (p.add) {
        const float4 b = *reinterpret_cast<const float4*>(p.add + (m / p.add_rpg) * p.add_ld + n);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    }
    float ca = p.c_acc, c1 = p.c_res1, c2 = p.c_res2;
    if (p.coef) {
        const float* cf = p.coef + (m / p.coef_rpg) * 3;
        ca = cf[0]; c1 = cf[1]; c2 = cf[2];
    }
    float o[4] = {ca * a.x, ca * a.y, ca * a.z, ca * a.w};
    if (p.res1) {
        const uint2 rr = *reinterpret_cast<const uint2*>(p.res1 + m * p.ldr1 + n);
        o[0] += c1 * bflo(rr.x); o[1] += c1 * bfhi(rr.x); o[2] += c1 * bflo(rr.y); o[3] += c1 * bfhi(rr.y);
    }
    if (p.res2) {
        const uint2 rr = *reinterpret_cast<const uint2*>(p.res2 + m * p.ldr2 + n);
        o[0] += c2 * bflo(rr.x); o[1] += c2 * bfhi(rr.x); o[2] += c2 * bflo(rr.y); o[3] += c2 * bfhi(rr.y);
    }
    if (p.out_fp32)
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(p.out) + m * p.ldo + n) = make_float4(o[0], o[1], o[2], o[3]);
    else
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(p.out) + m * p.ldo + n) = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
}

// library-owned fp32 workspaces of the split-K path: ONE PER STREAM (two streams splitting at the same time must not share partial
// sums), grow-only, and a retired (outgrown) slab is never freed: a HIP graph captured earlier may still replay launches that
// point into it.  Growth is geometric, so the retired slabs add up to less than twice the live one.  A request that would have to
// allocate while its stream is being captured returns nullptr (hipMalloc is illegal in a capture) and the caller falls back to
// the unsplit launch.  Partials are written with plain stores, one slab per split: fp32 atomics into one slab were tried first and
// made the launch 1.4-2.5x slower than not splitting at all (8.8 M atomics per 8x8 conv).
float* splitk_workspace(size_t floats, hipStream_t st) {
    struct Slab { float* ptr; size_t cap; };
    static std::mutex mu;
    static std::map<hipStream_t, Slab> slabs;
    std::lock_guard<std::mutex> lock(mu);
    Slab& s = slabs[st];
    if (floats > s.cap) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
        const size_t want = floats + floats / 2;
        float* fresh = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&fresh), want * sizeof(float)) != hipSuccess) return nullptr;
        s.ptr = fresh;      // the old slab stays allocated (see above)
        s.cap = want;
    }
    return s.ptr;
}

// ---- launch record (tests / tools / bench.py --shard-sim): what the last v3d_gemm of this thread launched, written once per call from its plan:
// family, tile, tile count, co-resident blocks per CU (the runtime's occupancy answer for that kernel), split-K ways, stream-K tail.
thread_local V3dLaunchInfo g_last_launch = {0, 0, 0, 0, 0, 0, 0};
long long g_gn_epilogue_launches = 0;      // (tests: how many launches of this process gathered GroupNorm statistics in a v3 <GN> epilogue)
template <typename K>
int v3d_occupancy(K kernel, int threads) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, 0) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        n = 1;
    }
    return n;
}
#define V3D_LAUNCH(KERNEL, ...)                                                                                          \
    do {                                                                                                                 \
        static const int occ_ = v3d_occupancy(KERNEL, pl.threads);                                                       \
        occ = occ_;                                                                                                      \
        hipLaunchKernelGGL(KERNEL, dim3(pl.grid_x, pl.grid_y, 1), dim3(pl.threads), 0, st, __VA_ARGS__);                 \
    } while (0)

// ---- policy: the A/B knobs, read from the environment once ------------------------------------------------------------------------------------------
struct GemmPolicy {
    int impl;      // V3D_GEMM_IMPL: 0 = heuristic, 1 = v1 only, 2 = v1/v2 only, 3 = v3 wherever it is legal
    int splitk;    // V3D_GEMM_SPLITK: 0 = never, N = force N-way where legal, -1 (unset) = heuristic
    int v3s;       // V3D_GEMM_V3S: 0 disables the two-blocks-per-CU GEGLU kernel, 1 = K < 640 only, 2 = every GEGLU projection.  In isolation it ties with the
                   // 256 x 256 kernel (402 vs 396 us); inside the sampler it is +0.9 % end to end (same-box A/B), 2 another +0.35 %
    int v6;        // V3D_GEMM_V6: 0 = never, 1 = where v3's tiles quantise badly (the rule in plan_gemm), 2 = every legal launch
    int streamk;   // V3D_STREAMK: 0 = classic tile assignment everywhere
};
const GemmPolicy& env_policy() {
    static const GemmPolicy pol = [] {
        auto rd = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        return GemmPolicy{rd("V3D_GEMM_IMPL", 0), rd("V3D_GEMM_SPLITK", -1), rd("V3D_GEMM_V3S", 2), rd("V3D_GEMM_V6", 1), rd("V3D_STREAMK", 1)};
    }();
    return pol;
}

// ---- plan: which kernel a call gets -----------------------------------------------------------------------------------------------------------------
//   id                 family  tile (BM x BN)  waves / blocks per CU      chosen when
//   K_V1                  1    128 x 64|128    4 / 2                      K % 32 != 0 (the 8-channel input conv, odd test shapes), K > 32768, V3D_GEMM_IMPL=1
//   K_V2_128_3x32         2    128 x 128       4 / 3, BK 32 x 3 stages    v2 launches (small M, ragged edges, batched) of <= 40 stages of 32
//   K_V2_128_2x64         2    128 x 128       4 / 2, BK 64 x 2           ... longer contractions with K % 64 == 0
//   K_V2_128_4x32         2    128 x 128       4 / 2, BK 32 x 4           ... longer contractions with K % 64 != 0
//   K_V2_256x64_2x64/3x32 2    256 x 64        4 / 2, BK 64 x 2 | 32 x 3  v2 launches where 64-wide N tiles waste less than 128-wide ones (N = 320 and friends)
//   K_V2_256x128          2    256 x 128       4 / 2, BK 32 x 3           v2 launches of GEGLU projections at K >= 640 / 3 x 3 convs at K <= 128 with M >= 4096
//   K_SPLITK              2    128 x 64|128    4 / 2, BK 64 x 2 + finalize  v2 launches whose tiles cover <= 3/4 of the CUs with >= 96 steps (the 8 x 8 level)
//   K_V3_256              3    256 x 256       8 / 1 persistent           default wherever v3's tiles fill the CUs about as well as v2's would
//   K_V3_256_GEGLU42      3    256 x 256       8 / 1, waves 4 x 2         ... GEGLU projections at K < 640 that the two-per-CU kernel does not take
//   K_V3_256_GN           3    256 x 256       8 / 1, statistics epilogue ... with gn_stats (whole groups per wave column, enough slots)
//   K_V3_192x320 (_GN)    3    192 x 320       8 / 1 (statistics epilogue) ... the N % 320 == 0 family
//   K_V3_256x128_GEGLU    3    256 x 128       8 / 2                      GEGLU projections with >= 2 tiles per CU (V3D_GEMM_V3S)
//   K_V6                  6    192 x 160       4 / 2 persistent           linear / temporal launches where v3's tiles leave a partial round (rule below)
//   K_HALO1 .. 4          5    192 x 320       8 / 1 persistent, stream-K tail   gn_in_table: 3 x 3 conv at W = 64 / 32 / 16, temporal conv (conv.hip v3d_conv_halo_variant)
enum GemmKernel {
    K_V1, K_V2_128_2x64, K_V2_128_3x32, K_V2_128_4x32, K_V2_256x64_2x64, K_V2_256x64_3x32, K_V2_256x128, K_SPLITK,
    K_V3_256, K_V3_256_GEGLU42, K_V3_256_GN, K_V3_192x320, K_V3_192x320_GN, K_V3_256x128_GEGLU, K_V6, K_HALO1, K_HALO2, K_HALO3, K_HALO4,
    K_COUNT, K_NONE = -1      // K_NONE: gn_in_table on a shape the haloed kernels do not take
};
struct GemmPlan {
    int kernel, family, bm, bn, mt, nt;
    long long tiles;                           // as the launch record reports them (x batch, x split-K ways)
    unsigned grid_x, grid_y;
    int threads, group_m, splitk;              // splitk: ways, 0 = not split
    int sk_tail, sk_full, sk_units;            // stream-K tail (0 = classic), see V3dGemmParams
    size_t sk_slot_bytes;
    bool gn_in_epilogue;                       // the launch gathers gn_stats itself (else v3d_gemm runs the stand-alone kernel)
    int mode;
    bool geglu;
};

// operands of the 4-wide epilogue accesses (8-byte bf16 / 16-byte fp32 vectors): shared by the v3 tile contract and the split-K finalize
// (bias: 16-byte alignment is an argument check of fill_params)
bool vec4_operands(const GP& p) {
    auto al = [](const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) % a) == 0; };
    return al(p.out, 16) && (!p.add || (al(p.add, 16) && p.add_ld % 4 == 0)) && (!p.res1 || (al(p.res1, 8) && p.ldr1 % 4 == 0)) &&
           (!p.res2 || (al(p.res2, 8) && p.ldr2 % 4 == 0));
}
// the v3 kernels only carry the branch-free epilogue: every wave tile (wm x wn) must be fully inside or fully outside the
// output and all vector-access alignment conditions of the fast path must hold
bool v3_ok(const GP& p, int wm, int wn) { return p.M % wm == 0 && p.N % wn == 0 && p.ldo % (p.out_fp32 ? 4 : 8) == 0 && vec4_operands(p); }

// pure: no HIP call, no environment, no state.  `p` = checked arguments (fill_params).
GemmPlan plan_gemm(const GP& p, int mode, bool geglu, int batch, int cus, const GemmPolicy& pol) {
    GemmPlan pl = {};
    pl.kernel = K_NONE;
    pl.group_m = -1;                           // tile walk: the heuristic of tile_coords (v6 sets its own)
    pl.mode = mode;
    pl.geglu = geglu;
    auto cdiv = [](long long a, long long b) { return (a + b - 1) / b; };
    auto tile = [&](int kernel, int family, int bm, int bn, int threads) {
        pl.kernel = kernel; pl.family = family; pl.bm = bm; pl.bn = bn; pl.threads = threads;
        pl.mt = (int)cdiv(p.M, bm); pl.nt = (int)cdiv(p.N, bn);
        pl.tiles = (long long)pl.mt * pl.nt;
    };
    auto persistent = [&](long long slots) { pl.grid_x = (unsigned)(pl.tiles < slots ? pl.tiles : slots); pl.grid_y = 1; return pl; };
    // a launch of t tiles on G block slots idles (ceil(t / G) G - t) / G of its last round, and the N tail of its last tile column
    auto fill = [&](long long bm, long long bn, long long slots) {
        const long long t = cdiv(p.M, bm) * cdiv(p.N, bn);
        return (double)t / (double)(cdiv(t, slots) * slots) * ((double)p.N / (double)(cdiv(p.N, bn) * bn));
    };
    const int taps = mode == V3D_GEMM_LINEAR ? 1 : (mode == V3D_GEMM_CONV3X3 ? 9 : 3);
    const bool dma_ok = v3d_k_steps_ok(p);     // the LDS-DMA kernels: whole 32-k steps, rows within reach of the zero page

    if (p.gn_in) {   // GroupNorm (+SiLU) of the input in the operand path: only the LDS-haloed kernels (their epilogue gathers gn_stats itself)
        const int halo = v3d_conv_halo_variant(p, mode);
        if (!halo) return pl;
        tile(K_HALO1 + halo - 1, 5, 192, 320, 512);
        pl.gn_in_epilogue = p.gn_stats != nullptr;
        // stream-K tail: the last round's tiles are cut at 32-channel chunks and shared out over all CUs.  Worth it when the partial round leaves >= 1/8 of
        // the chip idle, every block still gets a piece of >= 4 chunks, and the idle time it removes ((G - R) / G of a tile) is >= 2 chunks (18 / 6 steps):
        // the hand-off costs 10-15 us per owner (publish 245 KB write-through, flag, read back).
        const int G = cus, R = (int)(pl.tiles % G), units = (int)(p.K / 32);
        if (pol.streamk && R != 0 && (G - R) * 8 >= G && (long long)R * units / G >= 4 && (long long)(G - R) * units / G >= 2) {
            pl.sk_tail = R; pl.sk_full = (int)(pl.tiles / G); pl.sk_slot_bytes = (size_t)192 * 320 * 4;
            pl.grid_x = (unsigned)G; pl.grid_y = 1;
        } else {
            persistent(G);
        }
        pl.sk_units = units;
        return pl;
    }

    // Tile quantisation of the persistent kernels (round 6).  The 32 x 32 and 16 x 16 levels of the U-Net sit at 1.4 - 2.25 rounds of v3 tiles.  gemm_kernel_v6's
    // 192 x 160 tiles on 512 slots halve the granule: measured (profiles/r06_v6_ab.txt) -9 ... -14 % on the M = 9216 projections (N = 2560 / 3840) and the
    // N = K = 640 linears, -5 % on the 32 x 32 temporal convolution, a tie where v3's tiles fill >= 0.9 of their rounds or K = 2560 (v2 is as good there),
    // +1 ... 6 % where v3 runs whole rounds (N = 320 at 64 x 64, M = 36864 x N = 1280) - those stay where they were.  Also measured and dropped (same record): a SPLIT
    // launch (v3 on the rows that make whole rounds, the tail rows as a second launch on 192 x 160 / 96 x 160 tiles: +5 ... 8 % slower than either single launch - the
    // second launch's ramp costs more than the idle half round), 192 x 128 tiles for N = 1280 at M = 9216 (480 tiles on 512 slots: +4 ... 18 % slower than v3's 192
    // tiles at 0.75 of a round), and 96 x 160 tiles for launches whose v3 tiles cover half the CUs or fewer (the 8 x 8 level, the 4 - 6-image ranks of a frame
    // shard: +-3 %, and 1.6x slower than split-K at K = 5120).
    const bool n320 = !geglu && p.N % 320 == 0;                 // v3's 192 x 320 tile (wave tile 96 x 80; 147456 rows = 768 tiles = 3 per CU)
    const int bm3 = n320 ? 192 : 256, bn3 = n320 ? 320 : 256;
    const double fill3 = fill(bm3, bn3, cus);
    if (pol.v6 && pol.impl == 0 && mode != V3D_GEMM_CONV3X3 && !geglu && batch == 1 && dma_ok && p.M % 192 == 0 && p.N % 160 == 0 && !p.gn_stats && e4_ok(p, 96, 80)) {
        const long long t6 = (p.M / 192) * (p.N / 160), slots = 2ll * cus;
        if (t6 >= slots && (pol.v6 >= 2 || (p.K <= 1280 && fill3 < 0.9 && fill(192, 160, slots) >= fill3))) {
            tile(K_V6, 6, 192, 160, 256);
            pl.group_m = 0;      // row-major walk: the N-tiles of a row tile are consecutive ids -> blocks 8 apart on one XCD share its activation rows in L2
            return persistent(slots);
        }
    }
    // N tile of the v2 kernels: 128 unless a 64-wide tile wastes less (e.g. N = 320: 5 x 64 exact vs 3 x 128 = 17 % padding)
    // (64-row tiles for the small-M 8x8 level were measured slower than under-filled 128-row tiles: conv_L3 461 vs 586 TF/s)
    const int bn2 = cdiv(p.N, 64) * 64 < cdiv(p.N, 128) * 128 ? 64 : 128;
    // v3 (persistent big tiles) unless forced off (V3D_GEMM_IMPL=1/2), forced on (=3), or the tile count fills the CUs badly
    if (pol.impl != 1 && pol.impl != 2 && batch == 1 && dma_ok && p.N >= 256) {
        // epilogue-bound GEGLU projections (K = 320): 256 x 128 tile, two blocks per CU
        if (geglu && (p.K < 640 || pol.v3s >= 2) && pol.v3s && v3_ok(p, 64, 64) && cdiv(p.M, 256) * cdiv(p.N, 128) >= 2ll * cus) {
            tile(K_V3_256x128_GEGLU, 3, 256, 128, 512);
            return persistent(2ll * cus);
        }
        // measured (profiles/r01f_op_times_v3.txt): v3 wins wherever its tiles fill the CUs about as well as v2's (128 x bn2 tiles, 2 blocks per CU) do
        const bool want = pol.impl == 3 || fill3 >= 0.9 * fill(128, bn2, 2ll * cus);
        // (non-GEGLU v3 kernels only carry the hand-managed epilogue: its operand contract on top of the tile-shape one)
        const bool eok = geglu || (n320 ? e4_ok(p, 96, 80) : e4_ok(p, 128, 64));
        if (want && eok && (n320 ? v3_ok(p, 96, 80) : v3_ok(p, 128, 128))) {
            // statistics epilogue: every writer (wave tile x statistics group) stores into its own slot - needs whole groups per wave column (80 / 64 channels)
            // and gn_rps / (wave tile rows) + 2 slots
            const bool gn = !geglu && p.gn_stats && (n320 ? 80 : 64) % p.gn_cpg == 0 && p.gn_nslots >= p.gn_rps / (n320 ? 96 : 128) + 2;
            // GEGLU halves the output width: with waves laid out 4 (M) x 2 (N) a wave owns 128 weight rows = 64 output channels = whole
            // 128-byte lines of every output row (the 2 x 4 layout wrote 64-byte half lines from two different waves)
            // measured (tools/gemm_floor.py, M = 147456, N = 2560): K = 320: 396 us vs 416 us (2 x 4) vs 402 us (two 256 x 128 blocks
            // per CU) vs 421 us (v2); at K >= 640 the 2 x 4 layout with 32-row chunks is ahead again (tools/gemm_sweep.py)
            tile(n320 ? (gn ? K_V3_192x320_GN : K_V3_192x320) : gn ? K_V3_256_GN : (geglu && p.K < 640) ? K_V3_256_GEGLU42 : K_V3_256, 3, bm3, bn3, 512);
            pl.gn_in_epilogue = gn;
            return persistent(cus);
        }
    }
    // v2 / v1: one 128 x bn2 tile per block
    tile(K_V1, 1, 128, bn2, 256);
    pl.grid_x = (unsigned)pl.tiles; pl.grid_y = (unsigned)batch;
    // split-K: the 8x8 level has 180 tiles of 128 x 128 for 256 CUs and contractions of 160-720 steps, so a launch lasts as long as
    // ONE tile (conv 8x8 1280->1280: 153 us, 444 TF/s).  Splitting the flat (tap, k) range 2-4 ways fills the CUs; the partial sums
    // meet in an fp32 workspace (one slab per split) and a small finalize kernel applies the epilogue.
    if (!geglu) {
        const long long steps = (long long)taps * (p.K / 32);
        int ways = pol.splitk;
        if (ways < 0) ways = (pl.tiles * 4 <= (long long)cus * 3 && steps >= 96) ? (int)((3ll * cus + pl.tiles - 1) / pl.tiles) : 1;   // 8x8 conv: 546 / 693 / 617 / 699 TF/s at 1 / 2 / 3 / 4
        if (ways > 4) ways = 4;
        if (ways > steps / 32) ways = (int)(steps / 32);
        if (ways > 1 && batch == 1 && pol.impl != 1 && p.K % 64 == 0 && p.K * 2 <= 65536 && p.N % 4 == 0 && p.ldo % 4 == 0 && vec4_operands(p)) {
            pl.kernel = K_SPLITK; pl.family = 2; pl.splitk = ways;
            pl.grid_y = (unsigned)ways;
            pl.tiles *= ways;
            return pl;
        }
    }
    const long long stages = (long long)taps * cdiv(p.K, 32);
    if (pol.impl == 1 || !dma_ok) {
        // stays v1 (impl 0 / 2 / 3 all land here for v2-class shapes with ragged contractions)
    } else if (bn2 == 64) {
        // 64-wide N tiles: a 256 x 64 tile with the 4 waves stacked along M (wave tile 64 x 64) doubles the MFMAs per barrier and halves the weight
        // re-reads (lin_L0_320x320 433 -> 487, convt_L0_320 568 -> 734 TF/s); BK 64 x 2 stages, BK 32 x 3 when K % 64 != 0
        tile(p.K % 64 == 0 ? K_V2_256x64_2x64 : K_V2_256x64_3x32, 2, 256, 64, 256);
    } else if (((geglu && p.K >= 640) || (mode == V3D_GEMM_CONV3X3 && p.K <= 128)) && p.M >= 4096) {
        // wide GEGLU projections at K >= 640 and the 128-channel VAE convs: 256 x 128 tile on 4 waves (wave tile 128 x 64, 32 MFMAs per barrier,
        // 25 % fewer LDS-fill bytes per flop), BK 32 x 3 stages: 72 KiB -> 2 blocks / CU (lin_L1_ff1_geglu 662 -> 779, lin_L2_ff1_geglu 708 -> 865 TF/s)
        tile(K_V2_256x128, 2, 256, 128, 256);
    } else if (stages <= 40) {
        // measured on MI355X (profiles/r01_gemm_sweep.txt): short contractions (<= 40 stages of 32: every K <= 1280 linear, the 128-channel
        // VAE convs) are bound by per-tile fill/drain bubbles -> more co-resident blocks: BK 32 x 3 stages, 48 KiB LDS, 3 blocks / CU
        pl.kernel = K_V2_128_3x32; pl.family = 2;
    } else {
        pl.kernel = p.K % 64 == 0 ? K_V2_128_2x64 : K_V2_128_4x32;      // long contractions prefer fewer barriers per MFMA: BK 64 x 2 stages (one in flight)
        pl.family = 2;
    }
    pl.grid_x = (unsigned)pl.tiles;
    pl.tiles *= batch;
    return pl;
}

// ---- workspaces of the stream-K tail (device side: gemm_common.h sk_*) ---------------------------------------------------------------------------------
struct SkWorkspace {
    hipStream_t st;
    float* ws;
    unsigned* flags;
    size_t slot_bytes;
    int G;
};
std::vector<SkWorkspace> g_sk;       // (one per stream that ever launched a stream-K tail; never freed: captured graphs point into them)
std::mutex g_sk_mu;
long long g_sk_launches = 0;

// one workspace per stream (launches on one stream run back to back; two streams must not share slots); never allocated inside a capture
bool sk_workspace(GP& p, size_t slot_bytes, int G, hipStream_t st) {
    std::lock_guard<std::mutex> lock(g_sk_mu);
    const SkWorkspace* w = nullptr;
    for (const SkWorkspace& c : g_sk)
        if (c.st == st && c.slot_bytes >= slot_bytes && c.G == G) w = &c;
    if (!w) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return false; }
        SkWorkspace n = {st, nullptr, nullptr, slot_bytes, G};
        if (hipMalloc(reinterpret_cast<void**>(&n.ws), (size_t)G * slot_bytes) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&n.flags), ((size_t)G * 8 + 16) * 4) != hipSuccess ||
            hipMemset(n.flags, 0, ((size_t)G * 8 + 16) * 4) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        g_sk.push_back(n);
        w = &g_sk.back();
    }
    p.sk_ws = w->ws;
    p.sk_flags = w->flags;
    ++g_sk_launches;
    return true;
}

// ---- launch: one case per kernel id, no shape logic --------------------------------------------------------------------------------------------------
constexpr int kNoWorkspace = 1;      // launch_plan: the plan's split-K slab / stream-K workspace cannot be had (stream capture, hipMalloc failure); nothing was launched

template <int MODE, bool GEGLU>
int launch_kernel(const GemmPlan& pl, GP& p, hipStream_t st, int& occ) {
    const int ntiles = (int)pl.tiles;
    switch (pl.kernel) {
        case K_V1:
            if (pl.bn == 64) V3D_LAUNCH((gemm_kernel_v1<128, 64, MODE, GEGLU>), p);
            else V3D_LAUNCH((gemm_kernel_v1<128, 128, MODE, GEGLU>), p);
            break;
        case K_V2_128_2x64: V3D_LAUNCH((gemm_kernel_v2<128, 128, 2, 2, 2, 2, MODE, GEGLU>), p); break;
        case K_V2_128_3x32: V3D_LAUNCH((gemm_kernel_v2<128, 128, 2, 2, 3, 1, MODE, GEGLU>), p); break;
        case K_V2_128_4x32: V3D_LAUNCH((gemm_kernel_v2<128, 128, 2, 2, 4, 1, MODE, GEGLU>), p); break;
        case K_V2_256x64_2x64: V3D_LAUNCH((gemm_kernel_v2<256, 64, 4, 1, 2, 2, MODE, GEGLU>), p); break;
        case K_V2_256x64_3x32: V3D_LAUNCH((gemm_kernel_v2<256, 64, 4, 1, 3, 1, MODE, GEGLU>), p); break;
        case K_V2_256x128: V3D_LAUNCH((gemm_kernel_v2<256, 128, 2, 2, 3, 1, MODE, GEGLU>), p); break;
        case K_SPLITK:
            if constexpr (!GEGLU) {
                float* ws = splitk_workspace((size_t)pl.splitk * (size_t)p.M * (size_t)p.N, st);
                if (!ws) return kNoWorkspace;
                GP q = p;                 // the split launch: plain fp32 partial sums, slab `split`
                q.split_n = pl.splitk;
                q.out = ws; q.out_fp32 = 1; q.ldo = p.N; q.sO = p.M * p.N; q.sA = 0; q.sW = 0;
                q.bias = nullptr; q.add = nullptr; q.res1 = nullptr; q.res2 = nullptr; q.coef = nullptr;
                q.c_acc = 1.f; q.c_res1 = 0.f; q.c_res2 = 0.f;
                if (pl.bn == 64) V3D_LAUNCH((gemm_kernel_v2<128, 64, 2, 2, 2, 2, MODE, GEGLU>), q);
                else V3D_LAUNCH((gemm_kernel_v2<128, 128, 2, 2, 2, 2, MODE, GEGLU>), q);
                p.split_n = pl.splitk;
                p.ws = ws;
                hipLaunchKernelGGL(splitk_finalize_kernel, dim3((unsigned)((p.M * (p.N / 4) + 255) / 256)), dim3(256), 0, st, p);
                return v3d_check_launch("v3d_gemm(split-K)");
            }
            break;
        // epilogue chunk of the generic v3 kernel: 2 row fragments for GEGLU (its staged rows are half as wide), 1 otherwise (LDS budget next to the ring)
        case K_V3_256: V3D_LAUNCH((gemm_kernel_v3<256, 256, 2, 4, MODE, GEGLU, GEGLU ? 2 : 1>), p, ntiles); break;
        case K_V3_256_GEGLU42:
            if constexpr (GEGLU) V3D_LAUNCH((gemm_kernel_v3<256, 256, 4, 2, MODE, GEGLU, 1>), p, ntiles);
            break;
        case K_V3_256x128_GEGLU:
            if constexpr (GEGLU && MODE == V3D_GEMM_LINEAR) V3D_LAUNCH((gemm_kernel_v3<256, 128, 4, 2, MODE, GEGLU, 1, 3, 0>), p, ntiles);
            break;
        case K_V3_256_GN:
            if constexpr (!GEGLU) V3D_LAUNCH((gemm_kernel_v3<256, 256, 2, 4, MODE, GEGLU, 1, 4, 16, true>), p, ntiles);
            break;
        case K_V3_192x320:
            if constexpr (!GEGLU) V3D_LAUNCH((gemm_kernel_v3<192, 320, 2, 4, MODE, GEGLU, 1>), p, ntiles);
            break;
        case K_V3_192x320_GN:
            if constexpr (!GEGLU) V3D_LAUNCH((gemm_kernel_v3<192, 320, 2, 4, MODE, GEGLU, 1, 4, 16, true>), p, ntiles);
            break;
        case K_V6:
            if constexpr ((MODE == V3D_GEMM_LINEAR || MODE == V3D_GEMM_CONVT3) && !GEGLU) {
                V3D_LAUNCH((gemm_kernel_v6<192, 160, 3, MODE>), p, ntiles);
                return v3d_check_launch("v3d_gemm(v6)");
            }
            break;
    }
    return v3d_check_launch("v3d_gemm");
}

int launch_plan(const GemmPlan& pl, GP& p0, hipStream_t st) {
    GP p = p0;
    p.mt = pl.mt; p.nt = pl.nt; p.group_m = pl.group_m;
    int occ = 1, rc;
    if (pl.family == 5) {
        p.sk_units = pl.sk_units;
        if (pl.sk_tail) {
            if (!sk_workspace(p, pl.sk_slot_bytes, (int)pl.grid_x, st)) return kNoWorkspace;
            p.sk_tail = pl.sk_tail; p.sk_full = pl.sk_full;
        }
        rc = v3d_conv_halo_launch(p, pl.kernel - K_HALO1 + 1, (int)pl.grid_x, (int)pl.tiles, (void*)st);
    } else if (pl.mode == V3D_GEMM_LINEAR) {
        rc = pl.geglu ? launch_kernel<V3D_GEMM_LINEAR, true>(pl, p, st, occ) : launch_kernel<V3D_GEMM_LINEAR, false>(pl, p, st, occ);
    } else if (pl.mode == V3D_GEMM_CONV3X3) {
        rc = launch_kernel<V3D_GEMM_CONV3X3, false>(pl, p, st, occ);
    } else {
        rc = launch_kernel<V3D_GEMM_CONVT3, false>(pl, p, st, occ);
    }
    if (rc == kNoWorkspace) return rc;
    if (pl.family == 3 && pl.gn_in_epilogue) ++g_gn_epilogue_launches;
    g_last_launch = V3dLaunchInfo{pl.family, pl.bm, pl.bn, pl.tiles, occ, pl.splitk, pl.sk_tail};
    return rc;
}

// argument checks (all of them) + the kernels' parameter block
int fill_params(const v3d_gemm_args* a, GP& p) {
    V3D_REQUIRE(a != nullptr, "v3d_gemm: null args");
    V3D_REQUIRE(a->A && a->W && a->out, "v3d_gemm: null A/W/out");
    V3D_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, "v3d_gemm: bad M/N/K (%lld,%lld,%lld)", (long long)a->M, (long long)a->N, (long long)a->K);
    V3D_REQUIRE(a->K % 8 == 0 && a->lda % 8 == 0, "v3d_gemm: K and lda must be multiples of 8 (K=%lld lda=%lld)", (long long)a->K, (long long)a->lda);
    V3D_REQUIRE(((uintptr_t)a->A & 15) == 0 && ((uintptr_t)a->W & 15) == 0, "v3d_gemm: A/W must be 16-byte aligned");
    V3D_REQUIRE(a->batch >= 1 && a->batch <= 65535, "v3d_gemm: bad batch %d", a->batch);
    V3D_REQUIRE(!a->geglu || (a->N % 32 == 0 && a->mode == V3D_GEMM_LINEAR), "v3d_gemm: geglu needs LINEAR mode and N %% 32 == 0");
    V3D_REQUIRE(!a->add || a->add_rpg > 0, "v3d_gemm: add_rpg must be > 0");
    V3D_REQUIRE(!a->coef || a->coef_rpg > 0, "v3d_gemm: coef_rpg must be > 0");
    V3D_REQUIRE(a->sA % 8 == 0 && a->sW % 8 == 0, "v3d_gemm: batch strides must keep 16-byte alignment");
    V3D_REQUIRE(a->a_rows > 0 && a->a_row0 >= 0, "v3d_gemm: a_rows (rows addressable behind A) must be given");
    V3D_REQUIRE(!a->bias || ((uintptr_t)a->bias & 15) == 0, "v3d_gemm: bias must be 16-byte aligned");
    const long long mtiles = (a->M + 127) / 128, ntiles = (a->N + 63) / 64;
    V3D_REQUIRE(mtiles * ntiles < (1ll << 31), "v3d_gemm: grid too large");
    const int taps = a->mode == V3D_GEMM_LINEAR ? 1 : (a->mode == V3D_GEMM_CONV3X3 ? 9 : 3);
    const long long ldw = a->ldw ? a->ldw : a->K;
    V3D_REQUIRE(ldw >= a->K && ldw % 8 == 0, "v3d_gemm: ldw must be >= K and a multiple of 8");
    const unsigned long long a_bytes = (unsigned long long)a->a_rows * a->lda * 2ull;
    const unsigned long long w_bytes = ((unsigned long long)(taps * a->N - 1) * ldw + a->K) * 2ull;
    V3D_REQUIRE(a_bytes <= kMaxBufBytes && w_bytes <= kMaxBufBytes, "v3d_gemm: operand larger than 4 GiB - 256 B (A %llu B, W %llu B)", a_bytes, w_bytes);
    p.A = (const bf16_t*)a->A; p.W = (const bf16_t*)a->W; p.out = a->out;
    p.bias = a->bias; p.add = a->add; p.res1 = (const bf16_t*)a->res1; p.res2 = (const bf16_t*)a->res2; p.coef = a->coef;
    p.M = a->M; p.N = a->N; p.K = a->K;
    p.lda = a->lda; p.ldw = ldw; p.ldo = a->ldo; p.ldr1 = a->ldr1; p.ldr2 = a->ldr2;
    p.add_rpg = a->add_rpg; p.add_ld = a->add_ld; p.coef_rpg = a->coef_rpg;
    p.c_acc = a->c_acc; p.c_res1 = a->c_res1; p.c_res2 = a->c_res2;
    p.out_fp32 = a->out_fp32;
    p.a_row0 = a->a_row0; p.a_bytes = (unsigned)a_bytes; p.w_bytes = (unsigned)w_bytes;
    p.Hin = a->Hin; p.Win = a->Win; p.Hout = a->Hout; p.Wout = a->Wout; p.stride = a->stride;
    p.upshift = 0;
    p.pad_lo = 1;
    p.T = a->T; p.tmin = a->tmin; p.tmax = a->tmax; p.S = a->S;
    p.halo_rows = a->mode == V3D_GEMM_CONVT3 ? a->halo_rows : 0;
    p.sA = a->sA; p.sW = a->sW; p.sO = a->sO;
    p.mt = p.nt = 0;
    p.group_m = -1;
    p.split_n = 1;
    p.ws = nullptr;
    p.sk_tail = p.sk_full = p.sk_units = 0; p.sk_ws = nullptr; p.sk_flags = nullptr;
    p.gn_stats = nullptr; p.gn_rps = 0; p.gn_cpg = 0; p.gn_nslots = 0;
    if (a->gn_stats) {
        V3D_REQUIRE(!a->geglu && !a->out_fp32 && a->batch == 1, "v3d_gemm: gn_stats needs a bf16, non-GEGLU, unbatched output");
        V3D_REQUIRE(a->gn_cpg > 0 && a->gn_cpg % 2 == 0 && a->N == 32ll * a->gn_cpg, "v3d_gemm: gn_stats needs N = 32 * gn_cpg (got N=%lld cpg=%d)", (long long)a->N, a->gn_cpg);
        V3D_REQUIRE(a->gn_rps >= 16 && a->gn_rps % 16 == 0 && a->gn_rps < (1ll << 30) && a->M % a->gn_rps == 0, "v3d_gemm: gn_rps must be a multiple of 16 that divides M");
        V3D_REQUIRE(a->ldo == a->N && ((uintptr_t)a->gn_stats & 7) == 0, "v3d_gemm: gn_stats needs a dense output (ldo == N) and an 8-byte aligned buffer");
        V3D_REQUIRE(a->gn_nslots >= 1, "v3d_gemm: gn_nslots must be >= 1");
        p.gn_stats = a->gn_stats; p.gn_rps = a->gn_rps; p.gn_cpg = a->gn_cpg; p.gn_nslots = a->gn_nslots;
    }
    // GroupNorm (+SiLU) of the input in the operand path / two-source input: only the LDS-haloed kernels (conv.hip) take these
    p.A2 = (const bf16_t*)a->A2; p.K1 = a->A2 ? a->K1 : a->K; p.lda2 = a->lda2; p.a2_bytes = 0;
    p.gn_in = a->gn_in_table; p.gn_in_rps = a->gn_in_rps; p.gn_in_silu = a->gn_in_silu; p.gn_in_bytes = 0;
    if (a->A2) {
        V3D_REQUIRE(a->gn_in_table != nullptr, "v3d_gemm: a two-source input (A2) is only defined together with gn_in_table");
        const unsigned long long a2b = (unsigned long long)a->a_rows * a->lda2 * 2ull;
        V3D_REQUIRE(a->lda2 >= a->K - a->K1 && a2b <= kMaxBufBytes, "v3d_gemm: bad lda2 / A2 larger than 4 GiB - 256 B");
        p.a2_bytes = (unsigned)a2b;
    }
    if (a->gn_in_table) {
        V3D_REQUIRE(a->gn_in_rps > 0 && a->gn_in_rows > 0, "v3d_gemm: gn_in_table needs gn_in_rps and gn_in_rows");
        const unsigned long long tb = (unsigned long long)a->gn_in_rows * a->K * 8ull;
        V3D_REQUIRE(tb <= kMaxBufBytes && a->batch == 1 && !a->geglu, "v3d_gemm: gn_in_table too large / batched / GEGLU");
        p.gn_in_bytes = (unsigned)tb;
    }
    switch (a->mode) {
        case V3D_GEMM_LINEAR: break;
        case V3D_GEMM_CONV3X3:
            V3D_REQUIRE(a->up == 1 || a->up == 2, "v3d_gemm: up must be 1 or 2");
            V3D_REQUIRE(a->stride == 1 || a->stride == 2, "v3d_gemm: stride must be 1 or 2");
            V3D_REQUIRE(a->Hin > 0 && a->Win > 0 && a->Hout > 0 && a->Wout > 0, "v3d_gemm: bad conv geometry");
            V3D_REQUIRE(a->M % ((long long)a->Hout * a->Wout) == 0, "v3d_gemm: M must be n_img*Hout*Wout");
            V3D_REQUIRE(a->pad_mode == 0 || a->pad_mode == 1, "v3d_gemm: pad_mode must be 0 or 1");
            p.upshift = a->up - 1;
            p.pad_lo = a->pad_mode ? 0 : 1;
            break;
        case V3D_GEMM_CONVT3:
            V3D_REQUIRE(a->T > 0 && a->S > 0, "v3d_gemm: convt3 needs T,S");
            V3D_REQUIRE(a->halo_rows >= 0, "v3d_gemm: halo_rows must be >= 0");
            if (a->halo_rows > 0) {
                V3D_REQUIRE(a->M % ((long long)a->T * a->S) == 0 && a->halo_rows == a->M / a->T, "v3d_gemm: split-halo layout needs M = B*T*S and halo_rows = B*S");
                V3D_REQUIRE(a->a_row0 >= a->halo_rows && a->a_rows >= a->a_row0 + a->M + a->halo_rows, "v3d_gemm: split-halo layout: A must hold halo_rows rows on either side of the M local rows");
                V3D_REQUIRE(a->tmin >= -1 && a->tmax <= a->T, "v3d_gemm: split-halo layout carries one halo frame per side");
            }
            break;
        default:
            v3d_set_error("v3d_gemm: unknown mode %d", a->mode);
            return V3D_ERR_ARG;
    }
    return V3D_OK;
}

}  // namespace

// tests / tools only (not part of the ABI header): out[8] = family, bm, bn, tiles, blocks per CU, split-K ways, stream-K tail, CUs
extern "C" int v3d_debug_last_gemm_launch(long long* out) {
    out[0] = g_last_launch.family; out[1] = g_last_launch.bm; out[2] = g_last_launch.bn; out[3] = g_last_launch.tiles;
    out[4] = g_last_launch.blocks_per_cu; out[5] = g_last_launch.splitk; out[6] = g_last_launch.streamk; out[7] = v3d_num_cus();
    return 0;
}

// tests only (CPU): what plan_gemm chooses for these arguments on a device of `cus` CUs under policy5 = {IMPL, SPLITK, V3S, V6, STREAMK} (NULL: the
// environment's).  Pointers in `a` are only inspected for null-ness and alignment.  out[10] = kernel id, family, bm, bn, tiles, grid, split-K ways,
// stream-K tail tiles (0 = classic), gn_in_epilogue, number of kernel ids
extern "C" int v3d_debug_gemm_plan(const v3d_gemm_args* a, int cus, const int* policy5, long long* out) {
    GP p;
    const int frc = fill_params(a, p);
    if (frc != V3D_OK) return frc;
    const GemmPolicy pol = policy5 ? GemmPolicy{policy5[0], policy5[1], policy5[2], policy5[3], policy5[4]} : env_policy();
    const GemmPlan pl = plan_gemm(p, a->mode, a->geglu != 0, a->batch, cus, pol);
    out[0] = pl.kernel; out[1] = pl.family; out[2] = pl.bm; out[3] = pl.bn; out[4] = pl.tiles; out[5] = (long long)pl.grid_x * pl.grid_y;
    out[6] = pl.splitk; out[7] = pl.sk_tail; out[8] = pl.gn_in_epilogue; out[9] = K_COUNT;
    return V3D_OK;
}

// tests only (not part of the ABI header)
extern "C" long long v3d_debug_gn_epilogue_launches(void) { return g_gn_epilogue_launches; }

// tests only (CPU): the work list block b of a G-block launch would build for `ntiles` tiles of `units` granules - the device code's own table
// (gemm_common.h sk_build_table), so the decomposition can be checked for every shape without a GPU.  out[12]: items, donor flag, then two
// pieces of (tile, u0, u1, role, d0, d1) - the table's layout without its padding.  Returns 0 when no tail is planned for this launch.
extern "C" int v3d_debug_sk_table(int ntiles, int units, int G, int b, int min_units, int min_saved, int* out) {
    const int R = ntiles % G;
    if (R == 0 || (G - R) * 8 < G || (long long)R * units / G < min_units || (long long)(G - R) * units / G < min_saved) return 0;
    V3dGemmParams p = {};
    p.sk_tail = R;
    p.sk_full = ntiles / G;
    p.sk_units = units;
    int tab[SK_TAB_BYTES / 4] = {0};
    sk_build_table(p, b, G, ntiles, units, tab);
    out[0] = tab[0];
    out[1] = tab[1];
    for (int k = 0; k < 2; ++k)
        for (int j = 0; j < 6; ++j) out[2 + 6 * k + j] = tab[4 + 8 * k + j];
    return 1;
}

// tests only: launches with a stream-K tail; hand-offs that gave up waiting (must stay 0)
extern "C" long long v3d_debug_sk_launches(void) { return g_sk_launches; }
extern "C" long long v3d_debug_sk_timeouts(void) {
    long long t = 0;
    std::lock_guard<std::mutex> lock(g_sk_mu);
    for (const SkWorkspace& c : g_sk) {
        unsigned v = 0;
        if (hipMemcpy(&v, c.flags + (size_t)c.G * 8, 4, hipMemcpyDeviceToHost) == hipSuccess) t += v;
    }
    return t;
}

extern "C" int v3d_gemm_gn_in_supported(const v3d_gemm_args* a) {
    GP p;
    if (!a || !a->gn_in_table || fill_params(a, p) != V3D_OK) return 0;
    return plan_gemm(p, a->mode, false, 1, v3d_num_cus(), env_policy()).kernel != K_NONE;
}

extern "C" int v3d_gemm(const v3d_gemm_args* a, v3d_stream_t stream) {
    GP p;
    const int frc = fill_params(a, p);
    if (frc != V3D_OK) return frc;
    hipStream_t st = (hipStream_t)stream;
    GemmPolicy pol = env_policy();
    GemmPlan pl = plan_gemm(p, a->mode, a->geglu != 0, a->batch, v3d_num_cus(), pol);
    V3D_REQUIRE(pl.kernel != K_NONE, "v3d_gemm: gn_in_table is set but this shape is not one of the LDS-haloed kernels' (v3d_gemm_gn_in_supported): "
                                     "normalise the input with v3d_groupnorm_apply first");
    int rc = launch_plan(pl, p, st);
    if (rc == kNoWorkspace) {      // the same call without the feature that needs a workspace
        pol.splitk = 0;
        pol.streamk = 0;
        pl = plan_gemm(p, a->mode, a->geglu != 0, a->batch, v3d_num_cus(), pol);
        rc = launch_plan(pl, p, st);
    }
    if (rc != V3D_OK || !p.gn_stats || pl.gn_in_epilogue) return rc;
    // the kernel that ran has no statistics epilogue (v1 / v2 tiles, split-K, ragged shapes): same result from the stand-alone kernel
    return v3d_groupnorm_stats(a->out, a->N, nullptr, 0, a->gn_stats, a->gn_nslots, a->M / a->gn_rps, a->gn_rps, 32, 1, stream);
}
